"""Tile-wise adaptive histogram equalization (CLAHE) as include/torchpiv_hip.h defines it for tpiv_equalize, in plain numpy
integers -- the yardstick of the device kernels (the reference has no such step).

Parameters: tile (8..256) and clip_q8 (256..65536: the clip limit in 1/256 of the uniform bin height).  Per frame g
(uint8 [H, W]):

  tile grid, per axis of length n:  k = max(1, (2n + tile) // (2 tile)) tiles with the edges e_i = (i n) // k, i = 0..k.
  per tile with N pixels and the histogram h[256]:
      L = max(1, (clip_q8 N) >> 16);  E = sum max(h - L, 0);  r = E % 256
      h'[b] = min(h[b], L) + E // 256 + ((b + 1) r // 256 - b r // 256)          (one redistribution; sum h' = N)
      C = cumsum(h');  b0 = the lowest bin with h > 0;  d = N - C[b0]
      lut[b] = (510 max(C[b] - C[b0], 0) + d) // (2 d), 0 everywhere when d == 0
  per pixel p of an axis, in doubled coordinates:  P = 2p + 1, tile centres c_i = e_i + e_(i+1),
      i = clamp(the last i with c_i <= P, 0, k - 2), D = c_(i+1) - c_i, w1 = clamp(P - c_i, 0, D), w0 = D - w1
      (k == 1: the one tile with weight 1, D = 1)
  out = (2 s + Dy Dx) // (2 Dy Dx) with s = the sum over the four neighbour tiles of wy wx lut_tile[g].

Every step is integer arithmetic and every intermediate fits 32 bits (asserted), so a device that does the same gives the
same bytes.
"""
import numpy as np

TILE_MIN, TILE_MAX = 8, 256
CLIP_Q8_MIN, CLIP_Q8_MAX = 256, 65536


def clip_q8_of(clip):
    """The integer clip limit of a float clip in [1, 256], as the Python layer derives it."""
    return int(round(float(clip) * 256))


def _check(tile, clip_q8):
    if not TILE_MIN <= tile <= TILE_MAX:
        raise ValueError(f"tile {tile!r}")
    if not CLIP_Q8_MIN <= clip_q8 <= CLIP_Q8_MAX:
        raise ValueError(f"clip_q8 {clip_q8!r}")


def edges(n, tile):
    """e_0 .. e_k of an axis of n pixels."""
    k = max(1, (2 * n + tile) // (2 * tile))
    return [(i * n) // k for i in range(k + 1)]


def axis_weights(n, tile):
    """Per pixel of an axis: (i, w0, w1, D) as int64 arrays -- the lower neighbour tile and the doubled weights."""
    e = np.asarray(edges(n, tile), dtype=np.int64)
    k = len(e) - 1
    p = np.arange(n, dtype=np.int64)
    if k == 1:
        z = np.zeros(n, dtype=np.int64)
        return z, z + 1, z, z + 1
    c = e[:-1] + e[1:]
    P = 2 * p + 1
    i = np.clip(np.searchsorted(c, P, side="right") - 1, 0, k - 2)
    D = c[i + 1] - c[i]
    w1 = np.clip(P - c[i], 0, D)
    return i, D - w1, w1, D


def tile_lut(h, clip_q8):
    """The table of one tile from its histogram h (256 counts): (lut uint8 [256], h' int64 [256])."""
    h = np.asarray(h, dtype=np.int64)
    assert h.shape == (256,) and h.min() >= 0
    N = int(h.sum())
    assert N > 0 and 510 * N < 2 ** 31
    L = max(1, (clip_q8 * N) >> 16)
    E = int(np.maximum(h - L, 0).sum())
    r = E % 256
    b = np.arange(256, dtype=np.int64)
    h2 = np.minimum(h, L) + E // 256 + (((b + 1) * r) // 256 - (b * r) // 256)
    assert int(h2.sum()) == N
    C = np.cumsum(h2)
    b0 = int(np.nonzero(h)[0][0])
    d = N - int(C[b0])
    if d == 0:
        return np.zeros(256, dtype=np.uint8), h2
    num = 510 * np.maximum(C - C[b0], 0) + d
    assert num.max() < 2 ** 31
    lut = num // (2 * d)
    assert lut.min() >= 0 and lut.max() <= 255
    return lut.astype(np.uint8), h2


def luts(frames, tile, clip_q8):
    """The tables of frames uint8 [n, H, W]: uint8 [n, ky, kx, 256]."""
    _check(tile, clip_q8)
    f = np.asarray(frames)
    assert f.dtype == np.uint8 and f.ndim == 3
    n, H, W = f.shape
    ey, ex = edges(H, tile), edges(W, tile)
    out = np.zeros((n, len(ey) - 1, len(ex) - 1, 256), dtype=np.uint8)
    for j in range(n):
        for ty in range(len(ey) - 1):
            for tx in range(len(ex) - 1):
                t = f[j, ey[ty]:ey[ty + 1], ex[tx]:ex[tx + 1]]
                out[j, ty, tx] = tile_lut(np.bincount(t.ravel(), minlength=256), clip_q8)[0]
    return out


def blend(frames, tables, tile):
    """The per-pixel blend of the four neighbour tables: uint8 of the frames' shape [n, H, W]."""
    f = np.asarray(frames)
    n, H, W = f.shape
    iy, wy0, wy1, Dy = axis_weights(H, tile)
    ix, wx0, wx1, Dx = axis_weights(W, tile)
    ky, kx = tables.shape[1:3]
    iy1, ix1 = np.minimum(iy + 1, ky - 1), np.minimum(ix + 1, kx - 1)
    DD = Dy[:, None] * Dx[None, :]
    assert DD.max() <= 640 * 640
    out = np.empty_like(f)
    for j in range(n):
        t = tables[j].astype(np.int64)
        g = f[j].astype(np.int64)
        s = (wy0[:, None] * wx0[None, :] * t[iy[:, None], ix[None, :], g]
             + wy0[:, None] * wx1[None, :] * t[iy[:, None], ix1[None, :], g]
             + wy1[:, None] * wx0[None, :] * t[iy1[:, None], ix[None, :], g]
             + wy1[:, None] * wx1[None, :] * t[iy1[:, None], ix1[None, :], g])
        assert (2 * s + DD).max() < 2 ** 28
        o = (2 * s + DD) // (2 * DD)
        assert o.min() >= 0 and o.max() <= 255
        out[j] = o
    return out


def equalize(frames, tile, clip_q8, return_luts=False):
    """frames uint8 [H, W] or [n, H, W].  Returns uint8 of the frames' shape (and the tables [n, ky, kx, 256])."""
    f = np.asarray(frames)
    assert f.dtype == np.uint8 and f.ndim in (2, 3)
    f3 = f[None] if f.ndim == 2 else f
    t = luts(f3, tile, clip_q8)
    out = blend(f3, t, tile).reshape(f.shape)
    return (out, t) if return_luts else out


def brute_force(frame, tile, clip_q8):
    """The definition read literally, in Python integers: loops over the tiles' pixels and over the pixels of one frame
    [H, W].  Returns (out uint8 [H, W], the tables as a nested list [ky][kx] of 256 ints, the h' likewise)."""
    _check(tile, clip_q8)
    f = np.asarray(frame)
    H, W = f.shape
    ey, ex = edges(H, tile), edges(W, tile)
    ky, kx = len(ey) - 1, len(ex) - 1
    tab = [[None] * kx for _ in range(ky)]
    red = [[None] * kx for _ in range(ky)]
    for ty in range(ky):
        for tx in range(kx):
            h = [0] * 256
            for y in range(ey[ty], ey[ty + 1]):
                for x in range(ex[tx], ex[tx + 1]):
                    h[int(f[y, x])] += 1
            N = sum(h)
            L = max(1, (clip_q8 * N) >> 16)
            E = sum(max(v - L, 0) for v in h)
            r = E % 256
            h2 = [min(h[b], L) + E // 256 + (((b + 1) * r) // 256 - (b * r) // 256) for b in range(256)]
            C, acc = [], 0
            for v in h2:
                acc += v
                C.append(acc)
            b0 = min(b for b in range(256) if h[b] > 0)
            d = N - C[b0]
            tab[ty][tx] = [0 if d == 0 else (510 * max(C[b] - C[b0], 0) + d) // (2 * d) for b in range(256)]
            red[ty][tx] = h2

    def axis(p, e):
        k = len(e) - 1
        if k == 1:
            return 0, 0, 1, 0, 1
        c = [e[i] + e[i + 1] for i in range(k)]
        P = 2 * p + 1
        below = [i for i in range(k) if c[i] <= P]
        i = min(max(below[-1] if below else 0, 0), k - 2)
        D = c[i + 1] - c[i]
        w1 = min(max(P - c[i], 0), D)
        return i, i + 1, D - w1, w1, D

    out = np.zeros((H, W), dtype=np.uint8)
    for y in range(H):
        ia, ib, wy0, wy1, Dy = axis(y, ey)
        for x in range(W):
            ja, jb, wx0, wx1, Dx = axis(x, ex)
            g = int(f[y, x])
            s = (wy0 * wx0 * tab[ia][ja][g] + wy0 * wx1 * tab[ia][jb][g]
                 + wy1 * wx0 * tab[ib][ja][g] + wy1 * wx1 * tab[ib][jb][g])
            out[y, x] = (2 * s + Dy * Dx) // (2 * Dy * Dx)
    return out, tab, red
