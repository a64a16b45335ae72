"""numpy / torch-CPU float64 model of the weighted interrogation windows as include/torchpiv_hip.h defines them
(tpiv_plan_set_weighting), built around the oracle's own functions.  Nothing here shares a line with torchpiv_amd.engine or
with the device code.

Per window pair as the pass stages it (phase_model.windows: the first pass takes the raw windows, shifted passes the
oracle's DWS / CWS staging):
  1. W = g_y[y] g_x[x] as one float32 product of the float32 tables; "gaussian": g[i] = float32(exp(-t^2 / (2 sigma^2))),
     t = (2 i - (ws - 1)) / ws; "uniform": ones;
  2. a' = wa - mean(wa);  3. mu = sum W a' / sum W;  4. x_a = W (a' - mu), divided by mean(wa) in the first pass;
  5. C = fftshift of the circular cross-correlation of x_a and x_b (sum_i x_a[i] x_b[i + d]: the oracle's xcorr_fft);
  6. a window whose energy sum x^2 is exactly 0 in either frame, or a first-pass window whose pixel sum is 0, is empty:
     the zero map; dead in the first pass (u = v = 0, valid), the zero map's verdict (invalid) in a shifted pass.
corr_to_disp on C - min C follows, and a shifted pass combines with the predictor like IterPass._finish.

weighted_map(..., f32=True) is the same evaluated with torch.fft in float32 / complex64: the yardstick for what a float32
device evaluation may differ by.
"""
import numpy as np
import torch

from oracle import piv_oracle as O
import ensemble_model as EM
import phase_model as PM
import deform_model as DM

SIGMA = 0.4
SIGMA_MIN, SIGMA_MAX = 0.2, 4.0


def sigmas(weighting):
    """(kind, sigma_x, sigma_y) of "gaussian", "uniform" or {"kind", "sigma"}."""
    if isinstance(weighting, str):
        weighting = {"kind": weighting}
    kind = weighting.get("kind", "gaussian")
    s = weighting.get("sigma", SIGMA)
    if not isinstance(s, (tuple, list)):
        s = (s, s)
    return kind, float(s[0]), float(s[1])


def table(ws, sigma, kind="gaussian"):
    """g[0 .. ws - 1] float32: float64 exp, one rounding; "uniform": ones."""
    if kind == "uniform":
        return np.ones(ws, dtype=np.float32)
    i = np.arange(ws, dtype=np.float64)
    t = (2.0 * i - (ws - 1)) / ws
    return np.exp(-(t ** 2) / (2.0 * sigma ** 2)).astype(np.float32)


def weight(ws, weighting):
    """W [ws, ws] (y, x) float32: g_y[y] g_x[x] as one float32 product."""
    kind, sx, sy = sigmas(weighting)
    return (table(ws, sy, kind)[:, None] * table(ws, sx, kind)[None, :]).astype(np.float32)


def weighted_windows(w, W, first, f32=False):
    """(x [N, ws, ws], empty [N]) of staged windows w [N, ws, ws]: steps 2 to 4 and the window's part of step 6, in float64
    or (f32) float32."""
    rt = torch.float32 if f32 else torch.float64
    t = torch.from_numpy(np.ascontiguousarray(w)).to(rt)
    Wt = torch.from_numpy(np.ascontiguousarray(W)).to(rt)
    mean = t.mean(dim=(-2, -1), keepdim=True)
    rem = t - mean
    mu = (Wt * rem).sum(dim=(-2, -1), keepdim=True) / Wt.sum()
    x = Wt * (rem - mu)
    nothing = torch.zeros(len(t), dtype=torch.bool)
    if first:
        nothing = t.sum(dim=(-2, -1)) == 0
        x = torch.where(nothing[:, None, None], torch.zeros_like(x), x / torch.where(mean == 0, torch.ones_like(mean), mean))
    empty = nothing | ((x * x).sum(dim=(-2, -1)) == 0)
    return x, empty


def weighted_map(wa, wb, W, first, f32=False):
    """(C [N, ws, ws] float64 in fftshift layout, empty [N]) of staged windows wa, wb [N, ws, ws]."""
    xa, ea = weighted_windows(wa, W, first, f32)
    xb, eb = weighted_windows(wb, W, first, f32)
    empty = ea | eb
    C = torch.fft.fftshift(torch.fft.irfft2(torch.fft.rfft2(xa).conj() * torch.fft.rfft2(xb), s=xa.shape[-2:]), dim=(-2, -1))
    C[empty] = 0
    return C.to(torch.float64).numpy(), empty.numpy()


def shift_scale(wa, wb, W, first):
    """Per window: the peak-to-minimum range of the model map of a pure-shift pair -- the map of (x, x shifted) is the
    circular auto-correlation of x moved to the shift, so its range is the auto-correlation's; a general pair has two of
    them, and the scale is their geometric mean (the same number when wb is a shifted wa).  0 for an empty window."""
    out = []
    for w in (wa, wb):
        C, _ = weighted_map(w, w, W, first)
        out.append(C.max(axis=(1, 2)) - C.min(axis=(1, 2)))
    return np.sqrt(out[0] * out[1])


peaks = PM.peaks          # corr_to_disp on C - min C; an empty first-pass window is dead
windows = PM.windows      # the staged windows of a pass, before step 2


def pass1(a, b, ws, ov, weighting="gaussian", f32=False):
    nr, nc = (int(x) for x in O.field_shape(a.shape, ws, ov))
    wa, wb = windows(0, a, b, ws, ov)
    C, empty = weighted_map(wa, wb, weight(ws, weighting), True, f32)
    return peaks(C, empty, 0, nr, nc)


def iterate(mode, a, b, ws, ov, u0, v0, u2, v2, weighting="gaussian", f32=False):
    nr, nc = (int(x) for x in O.field_shape(a.shape, ws, ov))
    wa, wb = windows(mode, a, b, ws, ov, u2, v2)
    C, empty = weighted_map(wa, wb, weight(ws, weighting), False, f32)
    du, dv, inv = peaks(C, empty, mode, nr, nc)
    u, v = EM.combine(du, dv, inv, u0, v0, u2, v2)
    return u, v, inv


def chain(a, b, ws, ov, n_pass, mode, weighting="gaussian", pass_scale=2.0, f32=False):
    """The plan's chain of one pair without mask or outlier test: [(u, v, invalid)] per pass."""
    out = []
    w, o = ws, ov
    u, v, inv = pass1(a, b, w, o, weighting, f32)
    out.append((u, v, inv))
    for _ in range(1, n_pass):
        wf, of = int(w // pass_scale), int(o // pass_scale)
        u0, v0, u2, v2 = EM.predictor(mode, a.shape, w, o, wf, of, u, v, inv)
        u, v, inv = iterate(mode, a, b, wf, of, u0, v0, u2, v2, weighting, f32)
        out.append((u, v, inv))
        w, o = wf, of
    return out


def deform_rounds(a, b, u, v, inv, ws, ov, n, weighting="gaussian", interp="cubic", smooth=True):
    """n deformation rounds (deform_model.rounds) whose residual pass is the weighted first pass at (ws, ov)."""
    return DM.rounds(a, b, u, v, inv, ws, ov, n, lambda wa, wb: pass1(wa, wb, ws, ov, weighting), interp, smooth)
