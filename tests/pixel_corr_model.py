"""numpy model of single-pixel ensemble correlation as include/torchpiv_hip.h defines it (tpiv_pixel_corr_add /
tpiv_pixel_corr_peaks), and the channel scene its tests use.  Integer parts in int64; float parts one IEEE float64 operation
at a time, in the header's order (numpy's divide and sqrt round correctly, so a device that does too gives the same bits up
to the logarithms of the sub-pixel fit).

The scene: a steady channel flow u(y) along x -- a parabola of 3 px at the centre row that reaches zero 8 rows from either
wall, zero in those outer rows, v = 0 -- seeded with 0.03 particles per pixel of e^-2 diameter 2.5 px.  Frames are 64 x 264:
bins start at the frame's left edge, so a 128-pixel row bin is out of reach of both edges (status 0) only from the second
bin column on, and 264 = 2 x 128 + 8 is the narrowest width divisible by 4 that leaves radius 5 behind it."""
import math

import numpy as np

STATUS = {"valid": 0, "border": 1, "flat": 2, "range": 3, "fit": 4}
EPS = 1e-7
SCENE_SHAPE = (64, 264)
SCENE_BIN = (1, 128)
SCENE_RADIUS = 5
SCENE_PAIRS = 32
WALL = 8
U_MAX = 3.0


def _bin2(bin):
    return (int(bin), int(bin)) if isinstance(bin, (int, np.integer)) else (int(bin[0]), int(bin[1]))


def shifted(img, dy, dx):
    """out[..., y, x] = img[..., y + dy, x + dx], 0 outside the frame."""
    H, W = img.shape[-2:]
    out = np.zeros_like(img)
    ys, ye = max(0, -dy), min(H, H - dy)
    xs, xe = max(0, -dx), min(W, W - dx)
    if ys < ye and xs < xe:
        out[..., ys:ye, xs:xe] = img[..., ys + dy:ye + dy, xs + dx:xe + dx]
    return out


def bin_sums(img, bin):
    """[..., H, W] -> [..., n_by, n_bx]: sums over the bins; the rows and columns left over belong to no bin."""
    ky, kx = _bin2(bin)
    H, W = img.shape[-2:]
    nby, nbx = H // ky, W // kx
    t = img[..., :nby * ky, :nbx * kx].reshape(img.shape[:-2] + (nby, ky, nbx, kx))
    return t.sum(axis=(-3, -1))


def accumulate(A, B, bin, radius, shift=(0, 0), acc=None, mom=None):
    """(acc int64 [n_by, n_bx, D, D], mom int64 [4, H, W]) of the pairs A, B uint8 [n, H, W], added to the ones given."""
    A, B = np.asarray(A).astype(np.int64), np.asarray(B).astype(np.int64)
    n, H, W = A.shape
    ky, kx = _bin2(bin)
    R, D = int(radius), 2 * int(radius) + 1
    out = np.zeros((H // ky, W // kx, D, D), np.int64)
    for j in range(D):
        for i in range(D):
            prod = (A * shifted(B, shift[0] + j - R, shift[1] + i - R)).sum(axis=0)
            out[:, :, j, i] = bin_sums(prod, (ky, kx))
    m = np.stack([A.sum(axis=0), (A * A).sum(axis=0), B.sum(axis=0), (B * B).sum(axis=0)])
    return (out if acc is None else acc + out), (m if mom is None else mom + m)


def border_bins(H, W, bin, radius, shift=(0, 0)):
    """bool [n_by, n_bx]: some p + s + d of the bin leaves the frame."""
    ky, kx = _bin2(bin)
    R = int(radius)
    y0 = np.arange(H // ky)[:, None] * ky
    x0 = np.arange(W // kx)[None, :] * kx
    return ((y0 + shift[0] - R < 0) | (y0 + ky - 1 + shift[0] + R > H - 1) | (x0 + shift[1] - R < 0)
            | (x0 + kx - 1 + shift[1] + R > W - 1))


def coefficients(acc, mom, n_pairs, bin, radius, shift=(0, 0)):
    """(C float64 [n_by, n_bx, D, D], flat bool [n_by, n_bx]): the coefficient planes and where va = 0 or some vb[d] = 0."""
    acc, mom = np.asarray(acc, np.int64), np.asarray(mom, np.int64)
    N = np.int64(n_pairs)
    R, D = int(radius), 2 * int(radius) + 1
    num, vb = np.empty_like(acc), np.empty_like(acc)
    va = N * bin_sums(mom[1], bin) - bin_sums(mom[0] * mom[0], bin)
    var_b = N * mom[3] - mom[2] * mom[2]
    for j in range(D):
        for i in range(D):
            dy, dx = shift[0] + j - R, shift[1] + i - R
            num[:, :, j, i] = N * acc[:, :, j, i] - bin_sums(mom[0] * shifted(mom[2], dy, dx), bin)
            vb[:, :, j, i] = bin_sums(shifted(var_b, dy, dx), bin)
    assert max(np.abs(num).max(), np.abs(va).max(), np.abs(vb).max()) < 2 ** 57
    with np.errstate(all="ignore"):
        C = num.astype(np.float64) / np.sqrt(va.astype(np.float64)[:, :, None, None] * vb.astype(np.float64))
    return C, (va == 0) | (vb == 0).any(axis=(2, 3))


def peak_of(C, radius, shift=(0, 0)):
    """(u, v, peak, ratio, status) of one finite plane C [D, D] (border and flat are decided before)."""
    R, D = int(radius), 2 * int(radius) + 1
    M = (C - C.min()) + EPS
    j, i = divmod(int(np.argmax(M)), D)              # (the first arg-max in raster order)
    nan = float("nan")
    if j in (0, D - 1) or i in (0, D - 1):
        return nan, nan, nan, nan, STATUS["range"]
    with np.errstate(all="ignore"):
        lm = np.log(M[j, i])
        lxp, lxm = np.log(M[j, i + 1]), np.log(M[j, i - 1])
        lyp, lym = np.log(M[j + 1, i]), np.log(M[j - 1, i])
        dx = (lxm - lxp) / (2.0 * (lxp + lxm) - 4.0 * lm)
        dy = (lym - lyp) / (2.0 * (lyp + lym) - 4.0 * lm)
    if not (abs(dx) <= 1.0) or not (abs(dy) <= 1.0):
        return nan, nan, nan, nan, STATUS["fit"]
    rest = M.copy()
    rest[max(j - 2, 0):j + 3, max(i - 2, 0):i + 3] = 0.0
    return (float(shift[1] + i - R) + dx, float(shift[0] + j - R) + dy, float(C[j, i]), float(M[j, i] / rest.max()),
            STATUS["valid"])


def peaks(acc, mom, n_pairs, shape, bin, radius, shift=(0, 0)):
    """dict of u, v, peak, ratio float64 and status uint8 [n_by, n_bx] and corr float64 [n_by, n_bx, D, D]."""
    H, W = shape
    C, flat = coefficients(acc, mom, n_pairs, bin, radius, shift)
    border = border_bins(H, W, bin, radius, shift)
    nby, nbx = flat.shape
    out = {k: np.full((nby, nbx), np.nan) for k in ("u", "v", "peak", "ratio")}
    status = np.zeros((nby, nbx), np.uint8)
    corr = C.copy()
    for r in range(nby):
        for c in range(nbx):
            if border[r, c] or flat[r, c]:
                status[r, c] = STATUS["border"] if border[r, c] else STATUS["flat"]
                corr[r, c] = 0.0
                continue
            u, v, pk, ra, st = peak_of(C[r, c], radius, shift)
            out["u"][r, c], out["v"][r, c], out["peak"][r, c], out["ratio"][r, c], status[r, c] = u, v, pk, ra, st
    out.update(status=status, corr=corr)
    return out


def single_pixel(A, B, bin, radius, shift=(0, 0)):
    acc, mom = accumulate(A, B, bin, radius, shift)
    return peaks(acc, mom, len(A), A.shape[1:], bin, radius, shift)


# ---- the scene --------------------------------------------------------------------------------------------------------
def profile(y, H=SCENE_SHAPE[0]):
    """The constructed u(y) in pixels at image rows y (pixel centres at integers)."""
    y = np.asarray(y, dtype=np.float64)
    yc, half = (H - 1) / 2.0, H / 2.0 - WALL
    return np.where(np.abs(y - yc) < half, U_MAX * (1.0 - ((y - yc) / half) ** 2), 0.0)


def scene(n=SCENE_PAIRS, shape=SCENE_SHAPE, seed=0, density=0.03, diameter=2.5, peak=200.0, noise=1.0, offset=8.0):
    """(A, B) uint8 [n, H, W]: particles at p drawn at p - d / 2 in frame a and p + d / 2 in frame b, d = (profile(p_y), 0);
    Gaussian images exp(-8 r^2 / diameter^2) (diameter: where the image has fallen to e^-2), amplitudes 0.5..1 of `peak`,
    Gaussian noise and an offset, rounded and clipped to uint8."""
    H, W = shape
    rng = np.random.default_rng(90210 + int(seed))
    pad = 8.0
    X, Y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    frames = [[], []]
    for _ in range(n):
        m = rng.poisson(density * (H + 2 * pad) * (W + 2 * pad))
        px, py = rng.random(m) * (W + 2 * pad) - pad, rng.random(m) * (H + 2 * pad) - pad
        amp = (0.5 + 0.5 * rng.random(m)) * peak
        d = profile(py, H)
        gy = np.exp(-8.0 * (Y[None, :] - py[:, None]) ** 2 / diameter ** 2) * amp[:, None]
        for k, sign in enumerate((-0.5, 0.5)):
            gx = np.exp(-8.0 * (X[None, :] - (px + sign * d)[:, None]) ** 2 / diameter ** 2)
            img = gy.T @ gx + offset + rng.normal(0.0, noise, (H, W))
            frames[k].append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return np.stack(frames[0]), np.stack(frames[1])


def interior_rows(H=SCENE_SHAPE[0], radius=SCENE_RADIUS):
    """The rows of one-row bins out of reach of the top and bottom edge."""
    return np.arange(radius, H - radius)


def profile_error(u_rows, rows, H=SCENE_SHAPE[0]):
    """(rms, max) of u - profile over the rows given."""
    e = np.asarray(u_rows, dtype=np.float64) - profile(rows, H)
    return float(math.sqrt(np.mean(e * e))), float(np.abs(e).max())
