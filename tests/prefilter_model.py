"""The spatial pre-filters as include/torchpiv_hip.h defines them for tpiv_prefilter, in plain numpy integers -- the
yardstick of the device kernel (the reference has no such step).

Per frame f (uint8 [H, W]), odd size k in 3..63, r = k // 2:
    g = max(f, bg) - bg with a background, g = f without one (neighbours included);
    the neighbourhood of a pixel is the k x k square around it clipped to the image (no padding value), c its pixel count;
    kind "min":   out = g - min(neighbourhood of g);
    kind "mean":  S = sum(neighbourhood of g), m = (2 S + c) // (2 c), out = max(g - m, 0);
    kind None:    out = g;
    cap (1..255, optional), last: out = min(out, cap).
Every step is integer arithmetic, so a device that does the same gives the same bytes.
"""
import numpy as np


def _check(kind, size, cap):
    if kind not in (None, "min", "mean"):
        raise ValueError(f"kind {kind!r}")
    if kind is not None and (size is None or size % 2 == 0 or not 3 <= size <= 63):
        raise ValueError(f"size {size!r}")
    if cap is not None and not 1 <= cap <= 255:
        raise ValueError(f"cap {cap!r}")


def _windows(g, r, fill):
    """The 2r + 1 shifted views of g along its last axis, g padded with `fill`: a reduction over a window clipped to the
    image is the reduction over these when `fill` is the reduction's neutral value."""
    H, W = g.shape[-2:]
    pad = np.full(g.shape[:-1] + (W + 2 * r,), fill, dtype=g.dtype)
    pad[..., r:r + W] = g
    for d in range(2 * r + 1):
        yield pad[..., d:d + W]


def _sliding(g, r, op, fill):
    """op-reduction (np.minimum / np.add) of g over the (2r + 1)^2 neighbourhood clipped to the image, rows then columns."""
    acc = None
    for w in _windows(g, r, fill):
        acc = w.copy() if acc is None else op(acc, w)
    acc = np.swapaxes(acc, -1, -2)
    out = None
    for w in _windows(acc, r, fill):
        out = w.copy() if out is None else op(out, w)
    return np.swapaxes(out, -1, -2)


def counts(H, W, r):
    """c [H, W]: the number of in-image pixels of each pixel's neighbourhood."""
    y, x = np.arange(H), np.arange(W)
    cy = np.minimum(y + r, H - 1) - np.maximum(y - r, 0) + 1
    cx = np.minimum(x + r, W - 1) - np.maximum(x - r, 0) + 1
    return cy[:, None] * cx[None, :]


def prefilter(frames, kind, size=None, cap=None, background=None):
    """frames uint8 [H, W] or [n, H, W]; background uint8 [H, W] or None.  Returns uint8 of the frames' shape."""
    _check(kind, size, cap)
    f = np.asarray(frames)
    assert f.dtype == np.uint8 and f.ndim in (2, 3)
    g = f.astype(np.int64)
    if background is not None:
        bg = np.asarray(background).astype(np.int64)
        assert bg.shape == f.shape[-2:]
        g = np.maximum(g, bg) - bg
    out = g
    if kind == "min":
        out = g - _sliding(g, size // 2, np.minimum, 255)
    elif kind == "mean":
        S = _sliding(g, size // 2, np.add, 0)
        c = counts(f.shape[-2], f.shape[-1], size // 2)
        out = np.maximum(g - (2 * S + c) // (2 * c), 0)
    if cap is not None:
        out = np.minimum(out, cap)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def brute_force(frame, kind, size=None, cap=None, background=None):
    """The definition read literally: a double loop over the pixels of one frame [H, W]."""
    _check(kind, size, cap)
    f = np.asarray(frame)
    H, W = f.shape
    g = [[int(f[y, x]) for x in range(W)] for y in range(H)]
    if background is not None:
        g = [[max(g[y][x], int(background[y, x])) - int(background[y, x]) for x in range(W)] for y in range(H)]
    out = np.zeros((H, W), dtype=np.uint8)
    r = (size or 1) // 2
    for y in range(H):
        for x in range(W):
            nb = [g[yy][xx] for yy in range(max(y - r, 0), min(y + r, H - 1) + 1)
                  for xx in range(max(x - r, 0), min(x + r, W - 1) + 1)]
            o = g[y][x]
            if kind == "min":
                o -= min(nb)
            elif kind == "mean":
                o = max(o - (2 * sum(nb) + len(nb)) // (2 * len(nb)), 0)
            if cap is not None:
                o = min(o, cap)
            out[y, x] = o
    return out
