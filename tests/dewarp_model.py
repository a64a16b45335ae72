"""Numpy model of the geometric rectification (torchpiv_amd/csrc/dewarp.hip, include/torchpiv_hip.h): the Q8 backward map
from a homography, a polynomial or a pair of coordinate arrays, the Q10 Catmull-Rom table, both interpolations in
integer arithmetic, the offsets form, and the same interpolations in unrounded float64.  Nothing here shares a line with
torchpiv_amd.engine or with the device code."""
import numpy as np

POLY_ORDER = {3: 1, 6: 2, 10: 3}


def grid(H, W):
    """(x, y): output pixel coordinates, float64 [H, W] each."""
    y, x = np.mgrid[0:H, 0:W]
    return x.astype(np.float64), y.astype(np.float64)


def homography_coords(M, H, W):
    """Source coordinates (sx, sy) of every output pixel under the 3 x 3 matrix M: (x, y, 1) -> source, homogeneous."""
    M = np.asarray(M, dtype=np.float64)
    x, y = grid(H, W)
    X = M[0, 0] * x + M[0, 1] * y + M[0, 2]
    Y = M[1, 0] * x + M[1, 1] * y + M[1, 2]
    D = M[2, 0] * x + M[2, 1] * y + M[2, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return X / D, Y / D


def poly_terms(xn, yn, K):
    """The K terms of the polynomial in the normalised coordinates, in the documented order: 1, x, y | x^2, x y, y^2 |
    x^3, x^2 y, x y^2, y^3."""
    t = [np.ones_like(xn), xn, yn]
    if K >= 6:
        t += [xn * xn, xn * yn, yn * yn]
    if K >= 10:
        t += [xn * xn * xn, xn * xn * yn, xn * yn * yn, yn * yn * yn]
    return t


def normalised(x, y, H, W):
    """Output pixel coordinates to [-1, 1]: 2 x / (W - 1) - 1 (0 for an axis of one pixel)."""
    xn = 2.0 * x / (W - 1) - 1.0 if W > 1 else np.zeros_like(x)
    yn = 2.0 * y / (H - 1) - 1.0 if H > 1 else np.zeros_like(y)
    return xn, yn


def poly_coords(P, H, W):
    P = np.asarray(P, dtype=np.float64)
    x, y = grid(H, W)
    xn, yn = normalised(x, y, H, W)
    terms = poly_terms(xn, yn, P.shape[1])
    sx, sy = np.zeros((H, W)), np.zeros((H, W))
    for k, t in enumerate(terms):
        sx = sx + P[0, k] * t
        sy = sy + P[1, k] * t
    return sx, sy


def quantize(sx, sy, H, W):
    """int32 [H, W, 2]: q = floor(s * 256 + 0.5), x first; outside (and non-finite) entries (-1, -1)."""
    sx, sy = np.asarray(sx, dtype=np.float64), np.asarray(sy, dtype=np.float64)
    ok = np.isfinite(sx) & np.isfinite(sy)
    qx = np.floor(np.where(ok, sx, -1.0) * 256.0 + 0.5)
    qy = np.floor(np.where(ok, sy, -1.0) * 256.0 + 0.5)
    ok &= (qx >= 0) & (qy >= 0) & (qx <= (W - 1) * 256) & (qy <= (H - 1) * 256)
    m = np.full((H, W, 2), -1, dtype=np.int32)
    m[..., 0][ok] = qx[ok].astype(np.int32)
    m[..., 1][ok] = qy[ok].astype(np.int32)
    return m


def outside(m):
    H, W = m.shape[:2]
    return (m[..., 0] < 0) | (m[..., 1] < 0) | (m[..., 0] > (W - 1) * 256) | (m[..., 1] > (H - 1) * 256)


def cubic_table():
    """int16 [256, 4]: Catmull-Rom (a = -0.5) weights of t = f / 256 on the taps -1, 0, 1, 2 in Q10, floor(c 1024 + 0.5),
    the remainder to 1024 into weight 1 (f < 128) or 2 (f >= 128)."""
    T = np.zeros((256, 4), dtype=np.int64)
    for f in range(256):
        t = f / 256.0
        c = (-0.5 * t ** 3 + t ** 2 - 0.5 * t, 1.5 * t ** 3 - 2.5 * t ** 2 + 1.0, -1.5 * t ** 3 + 2.0 * t ** 2 + 0.5 * t,
             0.5 * t ** 3 - 0.5 * t ** 2)
        w = [int(np.floor(ck * 1024.0 + 0.5)) for ck in c]
        w[1 if f < 128 else 2] += 1024 - sum(w)
        T[f] = w
    return T.astype(np.int16)


def cubic_weights_float(t):
    return np.stack([-0.5 * t ** 3 + t ** 2 - 0.5 * t, 1.5 * t ** 3 - 2.5 * t ** 2 + 1.0,
                     -1.5 * t ** 3 + 2.0 * t ** 2 + 0.5 * t, 0.5 * t ** 3 - 0.5 * t ** 2], axis=-1)


def _taps(ix, iy, first, count, H, W):
    xs = np.stack([np.clip(ix + first + k, 0, W - 1) for k in range(count)], axis=-1)      # [H, W, count]
    ys = np.stack([np.clip(iy + first + k, 0, H - 1) for k in range(count)], axis=-1)
    return xs, ys


def accumulate(frame, m, interp):
    """The integer accumulator of every pixel before rounding, shift and clamp (int64 [H, W]); outside pixels hold 0."""
    H, W = frame.shape
    qx, qy = m[..., 0].astype(np.int64), m[..., 1].astype(np.int64)
    ix, iy, fx, fy = qx >> 8, qy >> 8, qx & 255, qy & 255
    if interp == "linear":
        xs, ys = _taps(ix, iy, 0, 2, H, W)
        wx = np.stack([256 - fx, fx], axis=-1)
        wy = np.stack([256 - fy, fy], axis=-1)
    else:
        T = cubic_table().astype(np.int64)
        xs, ys = _taps(ix, iy, -1, 4, H, W)
        wx, wy = T[fx], T[fy]
    p = frame.astype(np.int64)[ys[..., :, None], xs[..., None, :]]                         # [H, W, taps y, taps x]
    acc = (wy[..., :, None] * wx[..., None, :] * p).sum(axis=(-1, -2))
    return np.where(outside(m), 0, acc)


def dewarp(frames, m, interp="cubic", fill=0):
    """uint8 frames [n, H, W] or [H, W] through the map m int32 [H, W, 2]."""
    f3 = frames[None] if frames.ndim == 2 else frames
    out = np.empty(f3.shape, dtype=np.uint8)
    out_px = outside(m)
    for k in range(f3.shape[0]):
        acc = accumulate(f3[k], m, interp)
        v = (acc + 32768) >> 16 if interp == "linear" else np.clip((acc + (1 << 19)) >> 20, 0, 255)
        out[k] = np.where(out_px, fill, v).astype(np.uint8)
    return out[0] if frames.ndim == 2 else out


def dewarp_offsets(flat, offsets, H, W, m, interp="cubic", fill=0):
    """The offsets form: frame f = flat[offsets[f] : offsets[f] + H W]."""
    stack = np.stack([flat[o:o + H * W].reshape(H, W) for o in offsets])
    return dewarp(stack, m, interp, fill)


def dewarp_float(frame, sx, sy, interp):
    """Unrounded float64 interpolation at the real coordinates (edge replicate); NaN where the position is outside."""
    H, W = frame.shape
    ok = np.isfinite(sx) & np.isfinite(sy)
    sx, sy = np.where(ok, sx, 0.0), np.where(ok, sy, 0.0)
    ok &= (sx >= 0) & (sy >= 0) & (sx <= W - 1) & (sy <= H - 1)
    ix, iy = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    tx, ty = sx - ix, sy - iy
    if interp == "linear":
        xs, ys = _taps(ix, iy, 0, 2, H, W)
        wx, wy = np.stack([1 - tx, tx], axis=-1), np.stack([1 - ty, ty], axis=-1)
    else:
        xs, ys = _taps(ix, iy, -1, 4, H, W)
        wx, wy = cubic_weights_float(tx), cubic_weights_float(ty)
    p = frame.astype(np.float64)[ys[..., :, None], xs[..., None, :]]
    v = (wy[..., :, None] * wx[..., None, :] * p).sum(axis=(-1, -2))
    return np.where(ok, v, np.nan)


# ---- the maps of the tests ------------------------------------------------------------------------------------------
def rotation_perspective(H, W, degrees=7.0, px=4e-4, py=-3e-4):
    """3 x 3: a rotation about the frame centre with a perspective row -- outside pixels on all four sides."""
    a = np.deg2rad(degrees)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    T0 = np.array([[1, 0, -cx], [0, 1, -cy], [0, 0, 1.0]])
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [px, py, 1.0]])
    T1 = np.array([[1, 0, cx], [0, 1, cy], [0, 0, 1.0]])
    return T1 @ R @ T0


def scene(H, W, seed=5):
    """uint8 [2, H, W]: random noise with 0 and 255 samples, and a 0 / 255 checkerboard."""
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 256, (H, W)).astype(np.uint8)
    noise.flat[0], noise.flat[-1] = 0, 255
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([noise, (((x + y) & 1) * 255).astype(np.uint8)])
