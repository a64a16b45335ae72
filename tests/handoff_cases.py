"""Inputs of tests/test_gpu_handoff.py, in numpy (no GPU): per window size two synthetic particle pairs with a uniform
displacement, a planted predictor table with its mask byte, the coverage classes of the combine, and the oracle's own
staging and correlation on them (tests/test_handoff_model.py checks on the CPU that the reference alone populates every
class, so a case that proves nothing fails without a GPU).

Planted raw predictor values (TABLE): every rint tie of DWS (raw / 2 = +-0.5, +-1.5, +-2.5), both zeros, +-0.5 (rint = 0:
the clause never fires), the largest double below 0.5, +-1e-17 (a zero of either sign after rint), 0.75 and 1.25 (rint > 0
and well below the true displacement: du > u0), 3.0 and 6.0 (rint > 0, near / above it: du <= u0), negatives.  Magnitudes
are 0 or lie in [1e-30, 64]: below float32's normal range float(u / 2) and float(u) * 0.5f may differ by design (the
compact CWS reader halves in float32), and that range is not planted.

The table is cycled over the cell index k of the whole batch (u: entry k mod T, v: entry (k + 7) mod T, so the two
components of a cell sit in different classes); the mask byte is 1 where (k mod T + k div T) mod 4 == 0 -- a quarter of
the cells, every entry once in four table cycles, which two cycles per pair and two pairs provide."""
import functools

import numpy as np

from handoff_model import clause, handoff
from oracle import piv_oracle as O

TABLE = np.array([0.0, -0.0, 0.5, -0.5, 0.49999999999999994, 1.0, -1.0, 1.5, -1.5, 2.5, -2.5, 3.0, -3.0, 5.0, -5.0,
                  1e-17, -1e-17, 0.75, 1.25, 6.0], dtype=np.float64)
T = TABLE.size
V_OFFSET = 7
SIZES = (8, 16, 32, 64, 28, 10, 22, 15, 128)
FAST_SIZES = (32, 22)             # CWS_Fast: the four-field form only


def displacement(ws):
    """True displacement (dx, dy) of the pairs: both positive and non-integral; smaller for the windows of 8 and 10 pixels,
    where 3.2 px leaves too few particle pairs inside a window for the unshifted cells."""
    return (1.7, 1.3) if ws <= 10 else (3.2, 2.6)


def geometry(ws):
    """(H, W, ov, n_rows, n_cols): overlap ws // 2; 9 x 15 windows for ws <= 16, 7 x 9 for the larger ones -- odd counts
    (135, 63; 270, 126 per launch), no multiple of 64 nor of the 4, 2, 1 windows a tile wavefront holds, so the last
    wavefront and the last queue item are partial; >= 2 T cells per pair.  The frames are a few pixels larger than the grid."""
    ov = ws // 2
    st = ws - ov
    nr, nc = (9, 15) if ws <= 16 else (7, 9)
    H, W = ws + (nr - 1) * st + 1, ws + (nc - 1) * st + 3
    assert tuple(O.field_shape((H, W), ws, ov)) == (nr, nc) and nr * nc >= 2 * T and (2 * nr * nc) % 64 and (nr * nc) % 2
    return H, W, ov, nr, nc


def _render(px, py, amp, H, W, sigma=1.0):
    img = np.zeros(H * W)
    cx, cy = np.rint(px), np.rint(py)
    for oy in range(-3, 4):
        yy = cy + oy
        wy = np.exp(-((yy - py) ** 2) / (2 * sigma * sigma))
        for ox in range(-3, 4):
            xx = cx + ox
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            w = amp * wy * np.exp(-((xx - px) ** 2) / (2 * sigma * sigma))
            np.add.at(img, (yy[ok] * W + xx[ok]).astype(np.int64), w[ok])
    return img.reshape(H, W)


def _pair(H, W, dx, dy, density, seed):
    rng = np.random.default_rng(seed)
    pad = 12.0
    n = int(density * (H + 2 * pad) * (W + 2 * pad))
    px = rng.uniform(-pad, W + pad, n)
    py = rng.uniform(-pad, H + pad, n)
    amp = rng.uniform(100.0, 200.0, n)
    a = _render(px, py, amp, H, W) + 8.0 + rng.normal(0.0, 1.5, (H, W))
    b = _render(px + dx, py + dy, amp, H, W) + 8.0 + rng.normal(0.0, 1.5, (H, W))
    return a, b


@functools.lru_cache(maxsize=None)
def frames(ws):
    """(a, b) uint8 [2, H, W]: two different pairs.  The lower right corner of each frame b holds OTHER particles (those of
    an unrelated image), so the windows there have no correlation peak and the pass finds invalid vectors."""
    H, W, ov, nr, nc = geometry(ws)
    dx, dy = displacement(ws)
    density = 0.08 if ws <= 10 else 0.04
    A, B = [], []
    for pair in range(2):
        a, b = _pair(H, W, dx, dy, density, 1000 * ws + pair)
        _, other = _pair(H, W, dx, dy, density, 1000 * ws + 500 + pair)
        r0, c0 = int(0.6 * H), int(0.6 * W)
        b[r0:, c0:] = other[r0:, c0:]
        A.append(np.clip(np.rint(a), 0, 255).astype(np.uint8))
        B.append(np.clip(np.rint(b), 0, 255).astype(np.uint8))
    A, B = np.stack(A), np.stack(B)
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


@functools.lru_cache(maxsize=None)
def planted(ws):
    """(u_raw, v_raw float64, mask uint8), each [2, n_rows, n_cols]."""
    _, _, _, nr, nc = geometry(ws)
    k = np.arange(2 * nr * nc)
    u = TABLE[k % T].reshape(2, nr, nc)
    v = TABLE[(k + V_OFFSET) % T].reshape(2, nr, nc)
    m = (((k % T) + (k // T)) % 4 == 0).astype(np.uint8).reshape(2, nr, nc)
    for t in (u, v, m):
        t.setflags(write=False)
    return u, v, m


def table_coverage(ws):
    """Properties of the planted input alone: every table entry under both mask values, in u and in v."""
    u, v, m = planted(ws)
    ok = True
    for w in (u, v):
        for t in TABLE:
            same = (w == t) & (np.signbit(w) == np.signbit(t))
            ok = ok and (same & (m == 1)).any() and (same & (m == 0)).any()
    return ok


def coverage(mode, du, dv, invalid, u_raw, v_raw, mask):
    """The classes a case must populate, counted in cells, from a pass's raw result and the planted predictor."""
    u0, v0, _, _ = handoff(mode, u_raw, v_raw, mask)
    inv = np.asarray(invalid) != 0
    cu, cv = clause(du, u0), clause(dv, v0)
    out = {
        "clause_alone": int(((cu | cv) & ~inv).sum()),
        "above_but_rint0": int(((((du > u0) & (np.rint(u0) == 0)) | ((dv > v0) & (np.rint(v0) == 0))) & ~inv).sum()),
        "rint_pos_not_above": int(((((np.rint(u0) > 0) & (du <= u0)) | ((np.rint(v0) > 0) & (dv <= v0))) & ~inv).sum()),
        "invalid": int(inv.sum()),
        "one_mask_only": int(((cu | inv) != (cv | inv)).sum()),
    }
    if mode == "DWS":
        tie = (np.abs(u_raw / 2 - np.trunc(u_raw / 2)) == 0.5) | (np.abs(v_raw / 2 - np.trunc(v_raw / 2)) == 0.5)
        out["dws_tie"] = int(tie.sum())
        out["dws_tie_masked"] = int((tie & (np.asarray(mask) != 0)).sum())
    return out


def oracle_raw(mode, ws):
    """du, dv float64 and invalid bool [2, n_rows, n_cols] of the ORACLE's pass on frames(ws) with the planted predictor:
    its staging (O.shift_dws / O.shift_cws, as the oracle's passes call them), its correlation, its peak analysis."""
    A, B = frames(ws)
    H, W, ov, nr, nc = geometry(ws)
    u_raw, v_raw, mask = planted(ws)
    _, _, u2, v2 = handoff(mode, u_raw, v_raw, mask)
    idx = O.window_index((H, W), ws, ov)
    outs = []
    for p in range(2):
        if mode == "CWS":
            f = lambda t: t[p].astype(np.float32).reshape(-1)[:, None, None]
            aa = O.shift_cws(A[p], idx, -f(u2), -f(v2))
            bb = O.shift_cws(B[p], idx, f(u2), f(v2))
        else:
            f = lambda t: t[p].astype(np.int64).reshape(-1)[:, None, None]
            aa = O.shift_dws(A[p], idx, -f(u2), -f(v2))
            bb = O.shift_dws(B[p], idx, f(u2), f(v2))
        corr = O.xcorr_fft(aa, bb)
        corr = corr - corr.min(axis=(-2, -1), keepdims=True)
        outs.append(O.corr_to_disp(corr, nr, nc, True))
    return tuple(np.stack([o[i] for o in outs]) for i in range(3))
