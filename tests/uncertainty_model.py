"""numpy model of tpiv_uncertainty (include/torchpiv_hip.h): Wieneke's correlation-statistics estimate of a vector's
random error, in the fixed-point form of the kernel.  Every sum is an exact integer (int64), so the device's stats rows
equal the model's bit for bit; the float64 epilogue is one square root and three logarithms per component.

Vectorised over windows: one call takes all windows of a field (or any list of window origins)."""
import numpy as np

HALF_MAX = 32767


def half_shift(u):
    """Q8 half shift of a displacement: clamp(rint(u * 128), -32767, 32767); (values int64, finite bool)."""
    u = np.asarray(u, np.float64)
    ok = np.isfinite(u)
    h = np.clip(np.rint(np.where(ok, u, 0.0) * 128.0), -HALF_MAX, HALF_MAX).astype(np.int64)
    return h, ok


def lags(R):
    """The half plane of lags (k, l): rows 1..R with every column, row 0 with the columns 1..R; 2R(R+1) lags."""
    return [(0, l) for l in range(1, R + 1)] + [(k, l) for k in range(1, R + 1) for l in range(-R, R + 1)]


def _patch(img, y0, x0, hy, hx, ws, R):
    """Frame img uint8 [H, W] sampled at ((y0 + i) << 8) + hy, ((x0 + j) << 8) + hx for i, j = -R .. ws + R: int64
    [n, P, P] in Q2 grey levels.  y0, x0, hy, hx int64 [n]."""
    H, W = img.shape
    idx = np.arange(-R, ws + R + 1, dtype=np.int64)
    qy = ((y0[:, None] + idx[None, :]) << 8) + hy[:, None]
    qx = ((x0[:, None] + idx[None, :]) << 8) + hx[:, None]
    iy, fy = qy >> 8, qy & 255
    ix, fx = qx >> 8, qx & 255
    r0, r1 = np.clip(iy, 0, H - 1), np.clip(iy + 1, 0, H - 1)
    c0, c1 = np.clip(ix, 0, W - 1), np.clip(ix + 1, 0, W - 1)
    p = img.astype(np.int64)
    wy0, wy1 = (256 - fy)[:, :, None], fy[:, :, None]
    wx0, wx1 = (256 - fx)[:, None, :], fx[:, None, :]
    acc = wy0 * (wx0 * p[r0[:, :, None], c0[:, None, :]] + wx1 * p[r0[:, :, None], c1[:, None, :]]) \
        + wy1 * (wx0 * p[r1[:, :, None], c0[:, None, :]] + wx1 * p[r1[:, :, None], c1[:, None, :]])
    return (acc + 8192) >> 14


def _sigma(C0, S2, var):
    """The float64 epilogue, every operation rounded on its own."""
    with np.errstate(all="ignore"):
        sd = np.sqrt(var.astype(np.float64))
        s2, c0 = S2.astype(np.float64), C0.astype(np.float64)
        cp, cm = (s2 + sd) * 0.5, (s2 - sd) * 0.5
        bad = (C0 <= 0) | ~(cm > 0) | ~(c0 * c0 > cp * cm)
        lp, lm, l0 = np.log(cp), np.log(cm), np.log(c0)
        num = lp - lm
        den = 4.0 * l0 - 2.0 * lm - 2.0 * lp
        sig = num / den
    nan = np.full(sig.shape, np.nan)
    return np.where(bad, nan, sig), np.where(bad, nan, num), np.where(bad, nan, den)


def windows(a, b, y0, x0, u, v, ws, R, invalid=None, parts=False):
    """The estimate for n windows at origins (y0, x0) of frames a, b uint8 [H, W] with displacements u, v float64 [n].
    Returns (su, sv float64 [n], stats int64 [n, 8]); with parts also the model's numerators and denominators
    (num_u, den_u, num_v, den_v) of the closing quotient, NaN where sigma is."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape == b.shape and a.ndim == 2
    y0, x0 = np.asarray(y0, np.int64).ravel(), np.asarray(x0, np.int64).ravel()
    hx, okx = half_shift(np.asarray(u, np.float64).ravel())
    hy, oky = half_shift(np.asarray(v, np.float64).ravel())
    ok = okx & oky
    if invalid is not None:
        ok &= np.asarray(invalid).ravel() == 0
    A = _patch(a, y0, x0, -hy, -hx, ws, R)
    B = _patch(b, y0, x0, hy, hx, ws, R)
    N = ws * ws
    core = slice(R, R + ws)
    ma = (A[:, core, core].sum(axis=(1, 2)) + N // 2) // N
    mb = (B[:, core, core].sum(axis=(1, 2)) + N // 2) // N
    A -= ma[:, None, None]
    B -= mb[:, None, None]
    C0 = (A[:, core, core] * B[:, core, core]).sum(axis=(1, 2))
    comp = []
    for axis in (2, 1):                                   # x: neighbour [i][j + 1]; y: neighbour [i + 1][j]
        if axis == 2:
            a0, a1, b0, b1 = A[:, :-1, :-1], A[:, :-1, 1:], B[:, :-1, :-1], B[:, :-1, 1:]
        else:
            a0, a1, b0, b1 = A[:, :-1, :-1], A[:, 1:, :-1], B[:, :-1, :-1], B[:, 1:, :-1]
        d = a0 * b1 - a1 * b0
        S2 = (a0 * b1 + a1 * b0)[:, core, core].sum(axis=(1, 2))
        dc = d[:, core, core]
        S00 = (dc * dc).sum(axis=(1, 2))
        var = S00.copy()
        n = np.zeros_like(S00)
        for k, l in lags(R):
            S = (dc * d[:, R + k:R + k + ws, R + l:R + l + ws]).sum(axis=(1, 2))
            counted = 20 * S > S00
            var += np.where(counted, 2 * S, 0)
            n += counted
        comp.append((S2, S00, var, n))
    (S2x, S00x, varx, nx), (S2y, S00y, vary, ny) = comp
    su, numu, denu = _sigma(C0, S2x, varx)
    sv, numv, denv = _sigma(C0, S2y, vary)
    stats = np.stack([C0, S2x, S00x, varx, S2y, S00y, vary, nx + 256 * ny], axis=1)
    stats[~ok] = 0
    for arr in (su, sv, numu, denu, numv, denv):
        arr[~ok] = np.nan
    return (su, sv, stats, (numu, denu, numv, denv)) if parts else (su, sv, stats)


def field_shape(H, W, ws, ov):
    st = ws - ov
    return (H - ws) // st + 1, (W - ws) // st + 1


def field(a, b, u, v, ws, ov, R=3, invalid=None, parts=False):
    """The estimate for a field u, v float64 [nr, nc] at geometry (ws, ov): su, sv [nr, nc], stats int64 [nr, nc, 8]."""
    nr, nc = u.shape
    assert (nr, nc) == field_shape(a.shape[0], a.shape[1], ws, ov)
    st = ws - ov
    r, c = np.divmod(np.arange(nr * nc), nc)
    out = windows(a, b, r * st, c * st, u, v, ws, R, invalid=invalid, parts=parts)
    su, sv, stats = out[0].reshape(nr, nc), out[1].reshape(nr, nc), out[2].reshape(nr, nc, 8)
    return (su, sv, stats, tuple(p.reshape(nr, nc) for p in out[3])) if parts else (su, sv, stats)
