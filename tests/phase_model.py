"""numpy float64 model of the spectrally filtered passes (phase-only and robust phase correlation) as
include/torchpiv_hip.h defines them (tpiv_plan_set_correlation), built around the oracle's own functions, and the striped
scene its tests use.

Per window pair as the pass stages it (ensemble_model.staged; the first pass takes the raw windows: no division by the mean),
mean-free:  P = conj(F wa) (F wb);  m = mean |P|, tau = floor m;  W = g_y[|ky~|] g_x[|kx~|] (float32 tables, one float32
product);  Q = W P / max(|P|, tau), 0 where |P| = 0;  C = fftshift of the unnormalised inverse of Q.  A window without
mean-free energy in either frame has the zero map.  corr_to_disp on C - min C follows, and a shifted pass combines with the
predictor like IterPass._finish (ensemble_model.combine).

filtered_map(..., f32=True) is the same evaluated with torch.fft in complex64: the yardstick for what a float32 device
evaluation may differ by.  packed=True forms P the way the tile kernels do, from ONE complex transform of wa + i wb
(A = (Z(k) + conj Z(-k)) / 2, B = (Z(k) - conj Z(-k)) / 2i): in float32 that differs from two real transforms exactly where
one frame's spectrum has exact zeros (2 x 2 grains, noise-free periodic content) -- the other frame's rounding noise leaks
into those bins, u |B|^2 where the separate transforms give 0, and the floor passes it on as u |B|^2 / tau.
"""
import math

import numpy as np
import torch

from oracle import piv_oracle as O
import ensemble_model as EM

VAL_RATIO, VAL_WIN = EM.VAL_RATIO, EM.VAL_WIN
FLOOR = 2.0 ** -10
RPC_DIAMETER = 2.8


def diameters(correlation):
    """(d_x, d_y, floor) of "phase", "rpc" or {"kind", "diameter", "floor"}."""
    if isinstance(correlation, str):
        correlation = {"kind": correlation}
    kind = correlation.get("kind", "rpc")
    d = (0.0, 0.0) if kind == "phase" else correlation.get("diameter", RPC_DIAMETER)
    if not isinstance(d, (tuple, list)):
        d = (d, d)
    return float(d[0]), float(d[1]), float(correlation.get("floor", FLOOR))


def table(ws, d):
    """g[j] = float32(exp(-(pi d / (2 ws))^2 j^2)), j = 0 .. ws/2: float64 exp, one rounding."""
    j = np.arange(ws // 2 + 1, dtype=np.float64)
    return np.exp(-(math.pi * d / (2.0 * ws)) ** 2 * j * j).astype(np.float32)


def weight(ws, dx, dy):
    """W [ws, ws] (ky, kx), un-shifted bin order, float32: g_y[|ky~|] g_x[|kx~|] as one float32 product."""
    k = np.arange(ws)
    ka = np.where(k <= ws // 2, k, ws - k)
    return (table(ws, dy)[ka][:, None] * table(ws, dx)[ka][None, :]).astype(np.float32)


def windows(mode, a, b, ws, ov, u2=None, v2=None):
    """The staged windows of one pair, float64 [N, ws, ws] each, before the mean removal: pass 1 the raw windows (no
    division by the mean), shifted passes ensemble_model.staged."""
    if mode in (0, None, "PASS1"):
        return O.windows(a, ws, ov).astype(np.float64), O.windows(b, ws, ov).astype(np.float64)
    wa, wb, _ = EM.staged(mode, a, b, ws, ov, u2, v2)
    return wa, wb


def filtered_map(wa, wb, dx, dy, floor=FLOOR, f32=False, packed=False):
    """(C [N, ws, ws] float64 in fftshift layout, empty [N]) of staged windows wa, wb [N, ws, ws].  f32: the same steps in
    float32 / complex64 (torch.fft), returned as float64.  packed: P from one complex transform of wa + i wb."""
    ws = wa.shape[-1]
    rt, ct = (torch.float32, torch.complex64) if f32 else (torch.float64, torch.complex128)
    ta = torch.from_numpy(np.ascontiguousarray(wa)).to(rt)
    tb = torch.from_numpy(np.ascontiguousarray(wb)).to(rt)
    ta = ta - ta.mean(dim=(-2, -1), keepdim=True)
    tb = tb - tb.mean(dim=(-2, -1), keepdim=True)
    empty = ((ta * ta).sum(dim=(-2, -1)) == 0) | ((tb * tb).sum(dim=(-2, -1)) == 0)
    if packed:
        Z = torch.fft.fft2(torch.complex(ta, tb))
        Zm = torch.roll(torch.flip(Z, dims=(-2, -1)), shifts=(1, 1), dims=(-2, -1)).conj()       # conj Z(-k)
        P = ((Z + Zm) / 2).conj() * ((Z - Zm) / 2j)
    else:
        P = torch.fft.fft2(ta).conj() * torch.fft.fft2(tb)
    mag = P.abs()
    tau = floor * mag.mean(dim=(-2, -1), keepdim=True)
    W = torch.from_numpy(weight(ws, dx, dy)).to(rt)
    den = torch.maximum(mag, tau)
    scale = torch.where(mag > 0, W / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))
    Q = P * scale.to(ct)
    Q[empty] = 0
    C = torch.fft.ifft2(Q).real * float(ws * ws)
    C = torch.fft.fftshift(C, dim=(-2, -1))
    return C.to(torch.float64).numpy(), empty.numpy()


def peak_scale(ws, dx, dy):
    """sum W: the peak of a pure circular shift."""
    return float(weight(ws, dx, dy).astype(np.float64).sum())


def peaks(C, empty, mode, n_rows, n_cols, val_ratio=VAL_RATIO, val_win=VAL_WIN):
    """(du, dv, invalid) of the maps: corr_to_disp on C - min C; an empty window of the first pass is dead as a zero-sum
    window of the plain first pass is (u = v = 0, valid), an empty window of a shifted pass keeps what the zero map gives
    (invalid)."""
    M = C - C.min(axis=(-2, -1), keepdims=True)
    du, dv, inv = O.corr_to_disp(M, n_rows, n_cols, True, val_ratio, val_win)
    inv = inv.astype(bool)
    if mode in (0, None, "PASS1"):
        e = empty.reshape(n_rows, n_cols)
        du, dv, inv = np.where(e, 0.0, du), np.where(e, 0.0, dv), np.where(e, False, inv)
    return du, dv, inv


def pass1(a, b, ws, ov, correlation="rpc", f32=False):
    dx, dy, floor = diameters(correlation)
    nr, nc = (int(x) for x in O.field_shape(a.shape, ws, ov))
    wa, wb = windows(0, a, b, ws, ov)
    C, empty = filtered_map(wa, wb, dx, dy, floor, f32)
    return peaks(C, empty, 0, nr, nc)


def iterate(mode, a, b, ws, ov, u0, v0, u2, v2, correlation="rpc", f32=False):
    dx, dy, floor = diameters(correlation)
    nr, nc = (int(x) for x in O.field_shape(a.shape, ws, ov))
    wa, wb = windows(mode, a, b, ws, ov, u2, v2)
    C, empty = filtered_map(wa, wb, dx, dy, floor, f32)
    du, dv, inv = peaks(C, empty, mode, nr, nc)
    u, v = EM.combine(du, dv, inv, u0, v0, u2, v2)
    return u, v, inv


def chain(a, b, ws, ov, n_pass, mode, correlation="rpc", pass_scale=2.0, f32=False):
    """The plan's chain of one pair without mask or outlier test: [(u, v, invalid)] per pass.  correlation=None: the plain
    chain of the oracle (pass 1 in float64, shifted passes as the oracle runs them)."""
    out = []
    w, o = ws, ov
    if correlation is None:
        u, v, x, y, inv = O.pass1(a, b, w, o, validate=True)
        out.append((u, v, inv.astype(bool)))
        for _ in range(1, n_pass):
            wf, of = int(w // pass_scale), int(o // pass_scale)
            u, v, x, y, inv = O.ITER[mode](a.shape, wf, of)(a, b, x, y, u, v, inv)
            out.append((u, v, inv.astype(bool)))
            w, o = wf, of
        return out
    u, v, inv = pass1(a, b, w, o, correlation, f32)
    out.append((u, v, inv))
    for _ in range(1, n_pass):
        wf, of = int(w // pass_scale), int(o // pass_scale)
        u0, v0, u2, v2 = EM.predictor(mode, a.shape, w, o, wf, of, u, v, inv)
        u, v, inv = iterate(mode, a, b, wf, of, u0, v0, u2, v2, correlation, f32)
        out.append((u, v, inv))
        w, o = wf, of
    return out


# ---- the scenes -----------------------------------------------------------------------------------------------------
def stripes(H, W, period=12, level=60.0):
    """level where ((x // (period / 2)) % 2) == 0: vertical stripes, the same in both frames."""
    x = np.arange(W)
    return np.broadcast_to(level * (((x // (period // 2)) % 2) == 0), (H, W)).astype(np.float64)


def striped_scene(seed, H=256, W=256, density=0.03, period=12, level=60.0):
    """ensemble_model.scene with the static pattern added to both frames, rounded and clipped to uint8."""
    a, b = EM.scene(seed, H, W, density=density)
    s = stripes(H, W, period, level)
    fa = np.clip(np.rint(a.astype(np.float64) + s), 0, 255).astype(np.uint8)
    fb = np.clip(np.rint(b.astype(np.float64) + s), 0, 255).astype(np.uint8)
    return fa, fb


def score(u, v, inv, H, W, ws, ov):
    """(invalid vectors, vectors more than 1 px off among the valid ones, RMS over the valid vectors within 1 px) against
    the constructed flow."""
    tu, tv = EM.truth(H, W, ws, ov)
    err = np.hypot(u - tu, v - tv)
    ok = ~inv
    far = ok & (err > 1.0)
    near = ok & ~far
    return int(inv.sum()), int(far.sum()), (EM.rms(u, v, tu, tv, near) if near.any() else float("nan"))
