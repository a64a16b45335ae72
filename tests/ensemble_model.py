"""numpy float64 model of ensemble (sum-of-correlation) PIV as include/torchpiv_hip.h defines it (tpiv_ensemble_add /
tpiv_ensemble_peaks / tpiv_plan_ensemble_*), built from the oracle's own functions, and the sparse scene its tests use.

Per pass: the raw map C_i[w] of every pair i and window w (pass 1: windows divided by their mean, B:513-514, the zero map
when either window sums to 0; shifted passes: the oracle's shift_dws / shift_cws staging at ONE half shift per window for
every pair, not normalised), S = sum_i C_i in float64, M = S / n, and corr_to_disp on M - min M.  A shifted pass then
combines with the shared predictor like IterPass._finish.

The maps here carry their pedestal (the mean level sum(a) sum(b) / ws^2 of a raw correlation, exactly ws^2 for a normalised
live window): `pedestal` returns it, because the device transforms mean-free windows and so accumulates S minus the
pedestals -- a per-window constant that M - min M does not see.
"""
import math

import numpy as np

from oracle import piv_oracle as O

VAL_RATIO, VAL_WIN = 1.2, 3


# ---- the scene ------------------------------------------------------------------------------------------------------
def flow(x, y, H):
    """The constructed displacement (dx, dy) at positions (x, y) of an H-row frame."""
    return 2.3 + 0.6 * np.sin(2 * math.pi * np.asarray(y, dtype=np.float64) / H), np.full(np.shape(x), -1.4)


def scene(seed, H=160, W=160, density=2.0 / (32 * 32), sigma=1.0, noise=2.0, offset=8.0, flow_fn=None):
    """(a, b) uint8 [H, W]: the construction of deform_model.scene (particles at p rendered at p - d(p) / 2 in frame a and at
    p + d(p) / 2 in frame b), generator seed 4177 + seed, about two particles per 32 x 32 window.  flow_fn(x, y) -> (dx, dy):
    another displacement than flow()."""
    import torch
    from torchpiv_amd import synth
    g = torch.Generator(device="cpu")
    g.manual_seed(4177 + int(seed))
    pad = 10.0
    n = int(density * (H + 2 * pad) * (W + 2 * pad))
    px = torch.rand(n, generator=g, dtype=torch.float64) * (W + 2 * pad) - pad
    py = torch.rand(n, generator=g, dtype=torch.float64) * (H + 2 * pad) - pad
    amp = ((0.5 + 0.5 * torch.rand(n, generator=g, dtype=torch.float64)) * 200.0).float()
    na = torch.randn(H, W, generator=g) * noise
    nb = torch.randn(H, W, generator=g) * noise
    dx, dy = flow(px.numpy(), py.numpy(), H) if flow_fn is None else flow_fn(px.numpy(), py.numpy())
    dx, dy = torch.from_numpy(np.asarray(dx, dtype=np.float64)), torch.from_numpy(np.asarray(dy, dtype=np.float64))
    frames = []
    for sign, nz in ((-0.5, na), (0.5, nb)):
        img = synth._render((px + sign * dx).float(), (py + sign * dy).float(), amp, H, W, sigma, "cpu") + offset + nz
        frames.append(img.round().clamp_(0, 255).to(torch.uint8).numpy())
    return frames[0], frames[1]


def recording(n, H=160, W=160, **kw):
    """(A, B) uint8 [n, H, W]: n pairs of the scene, seeds 0 .. n - 1."""
    pairs = [scene(s, H, W, **kw) for s in range(n)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def truth(H, W, ws, ov):
    """(du, dv) [n_rows, n_cols]: the constructed displacement at the window centres r st + (ws - 1) / 2."""
    nr, nc = O.field_shape((H, W), ws, ov)
    st = ws - ov
    yc = np.arange(nr) * st + (ws - 1) / 2.0
    xc = np.arange(nc) * st + (ws - 1) / 2.0
    X, Y = np.meshgrid(xc, yc)
    return flow(X, Y, H)


def rms(u, v, tu, tv, ok=None):
    e2 = (u - tu) ** 2 + (v - tv) ** 2
    return float(np.sqrt(e2[ok].mean() if ok is not None else e2.mean()))


# ---- maps -----------------------------------------------------------------------------------------------------------
def staged(mode, a, b, ws, ov, u2=None, v2=None):
    """The windows one pair contributes, float64 [N, ws, ws] each, and which of them count: pass 1 (mode 0) the windows
    divided by their mean, `live` False where either sums to 0; "DWS" / "CWS" the oracle's staging at the half shift
    u2, v2 [n_rows, n_cols] (float64; DWS: integral values), every window live."""
    if mode in (0, None, "PASS1"):
        wa = O.windows(a, ws, ov).astype(np.float64)
        wb = O.windows(b, ws, ov).astype(np.float64)
        sa, sb = wa.sum(axis=(1, 2)), wb.sum(axis=(1, 2))
        live = (sa != 0) & (sb != 0)
        with np.errstate(all="ignore"):
            wa = wa / wa.mean(axis=(1, 2), keepdims=True)
            wb = wb / wb.mean(axis=(1, 2), keepdims=True)
        wa[~live] = 0.0
        wb[~live] = 0.0
        return wa, wb, live
    idx = O.window_index(a.shape, ws, ov)
    if mode == "DWS":
        ux = np.asarray(u2).astype(np.int64).reshape(-1)[:, None, None]
        vy = np.asarray(v2).astype(np.int64).reshape(-1)[:, None, None]
        wa, wb = O.shift_dws(a, idx, -ux, -vy), O.shift_dws(b, idx, ux, vy)
    elif mode == "CWS":
        ux = np.asarray(u2).astype(np.float32).reshape(-1)[:, None, None]
        vy = np.asarray(v2).astype(np.float32).reshape(-1)[:, None, None]
        wa, wb = O.shift_cws(a, idx, -ux, -vy), O.shift_cws(b, idx, ux, vy)
    else:
        raise KeyError(mode)
    return wa.astype(np.float64), wb.astype(np.float64), np.ones(len(wa), dtype=bool)


def pair_maps(mode, a, b, ws, ov, u2=None, v2=None):
    """(C [N, ws, ws] float64 in fftshift layout, pedestal [N], wa, wb, live) of one pair: the raw map with its pedestal."""
    wa, wb, live = staged(mode, a, b, ws, ov, u2, v2)
    C = O.xcorr_fft(wa, wb)
    C[~live] = 0.0
    ped = wa.sum(axis=(1, 2)) * wb.sum(axis=(1, 2)) / float(ws * ws)
    return C, ped, wa, wb, live


def summed(mode, A, B, ws, ov, u2=None, v2=None):
    """S = sum_i C_i over the pairs of A, B [n, H, W] in float64, the summed pedestals [N] and sum_i |C_i - pedestal_i|
    (the scale of the float32 summation error of the mean-free maps the device adds)."""
    S = P = Sabs = None
    for a, b in zip(A, B):
        C, ped, _, _, _ = pair_maps(mode, a, b, ws, ov, u2, v2)
        free = np.abs(C - ped[:, None, None])       # (a dead pass-1 window: zero map, zero pedestal)
        S = C if S is None else S + C
        P = ped if P is None else P + ped
        Sabs = free if Sabs is None else Sabs + free
    return S, P, Sabs


def peaks(S, n, n_rows, n_cols, val_ratio=VAL_RATIO, val_win=VAL_WIN):
    """(du, dv, invalid) of the summed maps S of n pairs: corr_to_disp on M - min M, M = S / n."""
    M = S / float(n)
    M = M - M.min(axis=(-2, -1), keepdims=True)
    du, dv, inv = O.corr_to_disp(M, n_rows, n_cols, True, val_ratio, val_win)
    return du, dv, inv.astype(bool)


def combine(du, dv, inv, u0, v0, u2, v2):
    """IterPass._finish behind the peak: u = 2 u2 + du, fallback to u0 where (du > u0 and rint(u0) > 0) or invalid."""
    u, v = 2 * u2 + du, 2 * v2 + dv
    mu = ((du > u0) & (np.rint(u0) > 0)) | inv
    mv = ((dv > v0) & (np.rint(v0) > 0)) | inv
    return np.where(mu, u0, u), np.where(mv, v0, v)


def predictor(mode, shape, ws_c, ov_c, ws_f, ov_f, u_c, v_c, inv_c):
    """The shared predictor of a shifted pass from the ensemble field of the pass before (IterCWS / IterDWS.__call__ up to
    the staging): u0, v0 after the invalid-zeroing and the half shift u2, v2 (CWS: halves taken before the zeroing; DWS:
    rint(u0 / 2) after it)."""
    xc, yc = O.coordinates(shape, ws_c, ov_c)
    xf, yf = O.coordinates(shape, ws_f, ov_f)
    sx, sy = xf[0, :], yf[:, 0]
    u0 = O.spline_predict(yc, xc, u_c, sy, sx)
    v0 = O.spline_predict(yc, xc, v_c, sy, sx)
    val = O.spline_predict(yc, xc, np.asarray(inv_c, dtype=np.float64), sy, sx) >= .5
    if mode == "CWS":
        u2, v2 = u0 / 2, v0 / 2
        u0[val] = 0.0
        v0[val] = 0.0
    else:
        u0[val] = 0.0
        v0[val] = 0.0
        u2, v2 = np.rint(u0 / 2), np.rint(v0 / 2)
    return u0, v0, u2, v2


def ensemble_pass1(A, B, ws, ov):
    nr, nc = O.field_shape(A.shape[1:], ws, ov)
    S, _, _ = summed(0, A, B, ws, ov)
    return peaks(S, len(A), nr, nc)


def ensemble_iter(mode, A, B, ws, ov, u0, v0, u2, v2):
    nr, nc = O.field_shape(A.shape[1:], ws, ov)
    S, _, _ = summed(mode, A, B, ws, ov, u2, v2)
    du, dv, inv = peaks(S, len(A), nr, nc)
    u, v = combine(du, dv, inv, u0, v0, u2, v2)
    return u, v, inv


def chain(A, B, ws, ov, n_pass, mode, pass_scale=2.0):
    """The plan's ensemble chain without mask or outlier test: [(u, v, invalid)] per pass."""
    out = []
    shape = A.shape[1:]
    w, o = ws, ov
    u, v, inv = ensemble_pass1(A, B, w, o)
    out.append((u, v, inv))
    for _ in range(1, n_pass):
        wf, of = int(w // pass_scale), int(o // pass_scale)
        u0, v0, u2, v2 = predictor(mode, shape, w, o, wf, of, u, v, inv)
        u, v, inv = ensemble_iter(mode, A, B, wf, of, u0, v0, u2, v2)
        out.append((u, v, inv))
        w, o = wf, of
    return out
