"""Numpy model of the deep-frame stage (engine.depth_lut / depth_range, tpiv_depth_map, tpiv_depth_histogram), written
from the definitions, value by value and bound by bound, without the cumulative-sum shortcuts of the engine."""
import numpy as np

BINS = 65536


def lut(lo, hi, curve="linear"):
    """uint8 [65536]: with c = clip(v, lo, hi) - lo and d = hi - lo, "linear": (c * 510 + d) // (2 * d) in int64 (255 c / d
    rounded half up), "sqrt": floor(255 * sqrt(c / d) + 0.5) in float64."""
    assert 0 <= lo < hi <= BINS - 1
    v = np.arange(BINS, dtype=np.int64)
    c = np.minimum(np.maximum(v, lo), hi) - lo
    d = np.int64(hi - lo)
    if curve == "linear":
        out = (c * 510 + d) // (2 * d)
    elif curve == "sqrt":
        out = np.floor(255.0 * np.sqrt(c.astype(np.float64) / float(d)) + 0.5).astype(np.int64)
    else:
        raise ValueError(curve)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def range_(hist, clip_low=0.0, clip_high=1e-4):
    """(lo, hi): lo = the largest l with count(v < l) <= floor(clip_low * N), hi = the smallest h with count(v > h) <=
    floor(clip_high * N); hi <= lo: hi = lo + 1, except lo = 65535: (65534, 65535)."""
    h = np.asarray(hist, dtype=np.int64)
    assert h.shape == (BINS,)
    N = int(h.sum())
    if N <= 0:
        raise ValueError("empty histogram")
    k_lo, k_hi = int(np.floor(clip_low * N)), int(np.floor(clip_high * N))
    lo, below = 0, 0                       # below = count(v < l) for the l under test
    for l in range(1, BINS):
        below += int(h[l - 1])
        if below > k_lo:
            break
        lo = l
    hi, above = BINS - 1, 0                # above = count(v > h) for the h under test
    for hh in range(BINS - 2, -1, -1):
        above += int(h[hh + 1])
        if above > k_hi:
            break
        hi = hh
    if hi <= lo:
        lo, hi = (BINS - 2, BINS - 1) if lo == BINS - 1 else (lo, lo + 1)
    return lo, hi


def map_(frames, table):
    """uint8 array of the frames' shape: table[sample]."""
    f = np.asarray(frames)
    assert f.dtype == np.uint16 and table.shape == (BINS,) and table.dtype == np.uint8
    return table[f.astype(np.int64)]


def hist(frames):
    return np.bincount(np.asarray(frames).astype(np.int64).reshape(-1), minlength=BINS).astype(np.int64)
