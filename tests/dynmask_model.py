"""Numpy model of the per-pair masks (torchpiv_amd/csrc/dynmask.hip, the per-pair kernels of mask.hip,
include/torchpiv_hip.h): the segmentation of a moving body from the frames themselves, and the per-pair forms of the
pixel step, the coverage count and the step that writes excluded cells into the fields.  Brute force on purpose -- every
offset of a neighbourhood is visited, one by one -- so nothing here shares a line with the device code."""
import numpy as np


def _clipped(img, rho, reduce, neutral):
    """reduce (np.minimum / np.maximum) over the (2 rho + 1)^2 square around every pixel, clipped to the image: the image
    is padded with the value that never wins, and every offset of the square is taken in turn."""
    H, W = img.shape
    pad = np.full((H + 2 * rho, W + 2 * rho), neutral, img.dtype)
    pad[rho:rho + H, rho:rho + W] = img
    out = np.full((H, W), neutral, img.dtype)
    for dy in range(2 * rho + 1):
        for dx in range(2 * rho + 1):
            out = reduce(out, pad[dy:dy + H, dx:dx + W])
    return out


def check(kind, size, level, grow):
    assert kind in ("bright", "dark") and size % 2 == 1 and 3 <= size <= 63 and 0 <= level <= 255
    assert grow >= 0 and size // 2 + grow <= 31


def core(g, kind, size, level):
    """bool [H, W]: bright: min over N_r of g >= level; dark: max over N_r of g <= level (r = size // 2)."""
    r = size // 2
    g = np.asarray(g, np.uint8)
    if kind == "bright":
        return _clipped(g, r, np.minimum, np.uint8(255)) >= level
    return _clipped(g, r, np.maximum, np.uint8(0)) <= level


def obj(g, kind, size, level, grow=0):
    """bool [H, W]: any core pixel in N_(r + grow)."""
    check(kind, size, level, grow)
    c = core(g, kind, size, level).astype(np.uint8)
    return _clipped(c, size // 2 + grow, np.maximum, np.uint8(0)) != 0


def pair_mask(a, b, kind, size, level, grow=0, static=None):
    """uint8 [H, W] of bytes 0 / 1: obj(a) | obj(b) | (static != 0)."""
    m = obj(a, kind, size, level, grow) | obj(b, kind, size, level, grow)
    if static is not None:
        m = m | (np.asarray(static) != 0)
    return m.astype(np.uint8)


def masks(A, B, kind, size, level, grow=0, static=None):
    """uint8 [n, H, W]: pair_mask of every pair of the stacks A, B [n, H, W]."""
    A, B = np.asarray(A), np.asarray(B)
    out = np.zeros(A.shape, np.uint8)
    for f in range(A.shape[0]):
        out[f] = pair_mask(A[f], B[f], kind, size, level, grow, static)
    return out


def field_shape(H, W, ws, ov):
    return (H - ws) // (ws - ov) + 1, (W - ws) // (ws - ov) + 1


def apply_pairs(frames, masks_):
    """frames uint8 [n, H, W] with the pixels of frame f that mask f marks (non-zero) set to 0."""
    out = np.array(frames, copy=True)
    for f in range(out.shape[0]):
        out[f][np.asarray(masks_[f]) != 0] = 0
    return out


def coverage_pairs(masks_, ws, ov):
    """int32 [n, n_rows, n_cols]: non-zero bytes of mask f in window (i, j) = rows i (ws - ov) ... + ws, columns likewise."""
    n, H, W = masks_.shape
    nr, nc = field_shape(H, W, ws, ov)
    step = ws - ov
    count = np.zeros((n, nr, nc), np.int32)
    for f in range(n):
        for i in range(nr):
            for j in range(nc):
                count[f, i, j] = np.count_nonzero(masks_[f, i * step:i * step + ws, j * step:j * step + ws])
    return count


def grids(count, ws, threshold):
    """bool: excluded cells, count > limit with limit = int(threshold * ws * ws) -- one float64 product, truncated."""
    return count > int(float(threshold) * float(ws * ws))


def fields_pairs(u, v, inv, grids_, value, status=None):
    """Copies of u, v, inv [batch, n_rows, n_cols] (and status) with the cells of pair f that grid f excludes at
    u = v = +0.0, inv = value, status = 2."""
    g = np.asarray(grids_) != 0
    u, v, inv = u.copy(), v.copy(), inv.copy()
    u[g] = 0.0
    v[g] = 0.0
    inv[g] = value
    if status is None:
        return u, v, inv
    status = status.copy()
    status[g] = 2
    return u, v, inv, status
