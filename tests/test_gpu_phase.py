"""The spectrally filtered passes (correlation="phase" / "rpc", xcorr_spec.hip) on the device against the float64 model of
tests/phase_model.py: every instance's map cell by cell, its fields, the plan chain on the striped scene, and the host paths.

Maps.  The device map against the model on the device's OWN staged windows (tpiv_debug_pass_spec reports them).  Per window:
half the spread of (device - model) over sum W -- the offset-free error in units of the peak of a pure shift.  The gate is
not a fixed number: it is 4 x the worst such figure of the CPU float32 evaluation (torch.fft, complex64) of the same windows
of the same case, the margin tests/test_gpu_f64_pass1.py gives a device transform over a CPU transform of equal precision.
That CPU evaluation is the model's own: two real transforms, P = conj(F wa)(F wb).
One term is added, per window, and only where it applies: the kernels take P from ONE packed transform of wa + i wb, and
where one frame's spectrum is exactly 0 in a bin (the pair of 0 / 255 noise in 2 x 2 grains: both Nyquist lines of frame
a) two real transforms return P = 0 exactly, while a packed transform carries the other frame's rounding noise into that
bin, which the floor hands on as dP / tau.  leak_bound derives the term from the constants of DESIGN.md 3.4b (DESIGN.md 3.5k
writes it out): (F + 1) u |Z| (|W B| over the zero bins of A + |W A| over the zero bins of B) / (tau sum W); it is 0 for a
window without such a bin: all but those of the grain pair and a few border windows whose clamped rows repeat.  The CPU's packed complex64 evaluation
(phase_model.filtered_map, packed=True) is printed and recorded beside it as information: it shows the same leak (2.3e-6 of
sum W at 16 x 16, the device 2.2e-6; two real transforms 1.6e-7).
An empty window (no mean-free energy in a frame) has a map that is exactly zero.
Fields.  u, v, invalid against corr_to_disp on the model map plus the combine: 1e-3 px (BASELINE.json's gate for float32
passes), identical validity, no window excused; that no arg-max margin, peak ratio or fit denominator of the model lies inside
twice the map gate is asserted on the model first (decisions_inside).  For empty windows only `invalid` is compared.
The seeds of the inputs were chosen on the CPU (oracle-staged windows) before any device run: see six_pairs.

TPIV_PHASE_REPORT=<file>: the figures are appended there as JSON lines (profiles/phase/measurements.json keeps a run's).
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import piv_oracle as O
import ensemble_model as EM
import phase_model as PM
from test_gpu_ensemble import half_shifts
from test_gpu_shifted_maps import expected_fields, neighbours

GATE_PX = 1e-3
MARGIN = 4.0
MODES = (0, "DWS", "CWS")
RPC24 = {"kind": "rpc", "diameter": (2.0, 4.0)}
DENSITY = {16: 0.06, 32: 0.03, 64: 0.015}
REPORT = os.environ.get("TPIV_PHASE_REPORT")


def report(**kw):
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(json.dumps(kw) + "\n")


def mode_name(m):
    return m or "PASS1"


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


# ---- inputs ---------------------------------------------------------------------------------------------------------
def geometry(ws, ov, grid):
    """Frame shape: a 3 x 4 grid with a 5-pixel remainder, a 3 x 3 grid with the same remainder (16 and 32: a partly
    filled last window group), or one window per frame (idle window slots)."""
    st = ws - ov
    if grid == "1x1":
        return ws + 3, ws + 5
    if grid == "3x3":
        return ws + 2 * st + 5, ws + 2 * st + 5
    return ws + 2 * st + 5, ws + 3 * st + 5


def six_pairs(mode, ws, ov, grid, seed=1):
    """(A, B uint8 [6, H, W], u2, v2), run as two batches of three so that items cross a pair boundary:
      0, 5: particle pairs whose displacement is twice the planted half shift of the nearest window plus (0.3, -0.2) (the
            staged windows correlate at every planted shift; pass 1: the model's flow),
      1:    such a pair with stripes of period 16 added to both frames,
      2:    0 / 255 noise in 2 x 2 grains (b a rolled copy with 5 % redrawn),
      3:    frame a zero,   4: frame b constant.
    (Seeds: chosen on the model with oracle-staged windows before any device run, so that no decision of any case lies
    inside twice the map gate -- seed 1 everywhere but at DWS 16/8 on the 3 x 4 grid, where one window of the grain pair
    has a decision inside its (leak-widened) band in the "rpc" run; seed 2 leaves none there with either filter:
    CASE_SEED.)"""
    H, W = geometry(ws, ov, grid)
    nr, nc = (int(x) for x in O.field_shape((H, W), ws, ov))
    st = ws - ov
    u2, v2 = (None, None) if mode == 0 else half_shifts(mode, ws, nr, nc)

    def flow_fn(x, y):
        r = np.clip(np.rint((y - (ws - 1) / 2.0) / st), 0, nr - 1).astype(int)
        c = np.clip(np.rint((x - (ws - 1) / 2.0) / st), 0, nc - 1).astype(int)
        return 2 * u2[r, c] + 0.3, 2 * v2[r, c] - 0.2
    parts = [EM.scene(100 * ws + 10 * seed + i, H, W, density=DENSITY[ws], flow_fn=None if mode == 0 else flow_fn)
             for i in range(4)]
    s = PM.stripes(H, W, period=16, level=60.0)
    striped = tuple(np.clip(np.rint(f.astype(np.float64) + s), 0, 255).astype(np.uint8) for f in parts[1])
    rng = np.random.default_rng(7 * ws + ov + seed)
    ra = np.repeat(np.repeat(rng.integers(0, 2, ((H + 1) // 2, (W + 1) // 2)) * 255, 2, axis=0), 2, axis=1)[:H, :W].astype(np.uint8)
    rb = np.roll(ra, (-1, 2), axis=(0, 1))
    rb = np.where(rng.random((H, W)) < 0.05, rng.integers(0, 2, (H, W)) * 255, rb).astype(np.uint8)
    pairs = [parts[0], striped, (ra, rb), (np.zeros((H, W), np.uint8), parts[2][1]),
             (parts[2][0], np.full((H, W), 90, np.uint8)), parts[3]]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), u2, v2


CASE_SEED = {("DWS", 16, 8, "3x4"): 2}


def figures(got, want, top):
    """Per window: half the spread of (got - want) over the peak scale."""
    d = (got - want).reshape(len(got), -1)
    return (d.max(axis=1) - d.min(axis=1)) / (2.0 * top)


def fit_inside(c, i_m, i_1, i_2, delta):
    """fit_bound of tests/test_gpu_shifted_maps.py as a yes / no -- does the fit (log c2 - log c1) / (2 (log c1 + log c2) -
    4 log cm) have a cell whose interval reaches 0, or a denominator whose interval contains 0, when every cell may move by
    delta -- with one refinement that the filtered maps need.  The cell that IS the map minimum does not move: both sides
    subtract their own minimum, so it holds exactly 1e-7 on either side as long as the arg-min is the same cell, i.e. as long
    as the second-smallest cell is more than 2 delta above it.  (A phase-only map of a window pair with a flat spectrum and a
    fractional shift is a Dirichlet kernel, whose first negative lobe -- the peak's own neighbour -- is the minimum of the
    whole map: without the refinement every such window would count as undecided, although both sides compute
    log(1e-7) there.)"""
    rows = np.arange(len(c))
    amin = np.argmin(c, axis=1)
    two = np.partition(c, 1, axis=1)[:, :2]
    pinned = (two[:, 1] - two[:, 0]) > 2 * delta
    vals = [c[rows, i] for i in (i_m, i_1, i_2)]
    dl = [np.where((i == amin) & pinned, 0.0, delta) for i in (i_m, i_1, i_2)]
    with np.errstate(all="ignore"):
        lo = [np.log(np.maximum(x - d, 0.0)) for x, d in zip(vals, dl)]
        hi = [np.log(x + d) for x, d in zip(vals, dl)]
        den = (2 * (lo[1] + lo[2]) - 4 * hi[0], 2 * (hi[1] + hi[2]) - 4 * lo[0])
        f0 = (np.log(vals[2]) - np.log(vals[1])) / (2 * (np.log(vals[1]) + np.log(vals[2])) - 4 * np.log(vals[0]))
    return ~np.isfinite(lo[0]) | ~np.isfinite(lo[1]) | ~np.isfinite(lo[2]) | ((den[0] <= 0) & (den[1] >= 0)) | ~np.isfinite(f0)


def decisions_inside(M, beta):
    """Windows of maps M [n, ws, ws] (minimum 0) with a discrete decision inside the band of an offset-free map error beta
    (delta = 2 beta per cell after both sides subtract their minimum, as expected_fields of tests/test_gpu_shifted_maps.py
    has it): the arg-max margin and the peak ratio from there, the fit by fit_inside."""
    n, ws, _ = M.shape
    near = expected_fields(M, beta)[5]
    c = M.reshape(n, -1) + O.EPS
    m = np.argmax(c, axis=1)
    left, right, top, bot = neighbours(m, ws, ws)
    fit = fit_inside(c, m, left, right, 2.0 * beta) | fit_inside(c, m, top, bot, 2.0 * beta)
    return near["argmax"] | near["ratio"] | fit


U32 = 2.0 ** -24
ETA = 6.66                  # per radix-2 level of the float32 codelets (piv_kernels.h: EXACT_ETA)


def leak_bound(fa, fb, dx, dy, floor):
    """Per window, in units of sum W: what the packed transform may add to the map where one frame's spectrum is exactly 0.
    There A_k = 0, the packed A_k = (Z_k + conj Z_-k) / 2 is pure transform error, sum over those bins |dA_k|^2 <= |dZ|^2
    <= ((F + 1) u |Z|)^2 with F = 2 eta log2 ws (|Z|^2 = N (|a'|^2 + |b'|^2)), dP_k = conj(dA_k) B_k, and
    |P_k| is far below tau, so dQ_k = W_k dP_k / tau; by Cauchy-Schwarz the map moves by at most
    (F + 1) u |Z| sqrt(sum_k W_k^2 |B_k|^2) / tau, and likewise with A and B exchanged.  "Exactly 0": below 1e-9 of the
    frame's largest bin in the float64 transform (a float64 transform leaves 1e-13 there).  0 for a window without such
    bins apart from the DC bin, where both spectra vanish and nothing leaks."""
    n, ws, _ = fa.shape
    a = fa - fa.mean(axis=(1, 2), keepdims=True)
    b = fb - fb.mean(axis=(1, 2), keepdims=True)
    A, B = np.fft.fft2(a), np.fft.fft2(b)
    W = PM.weight(ws, dx, dy).astype(np.float64)
    magA, magB = np.abs(A), np.abs(B)
    za = magA <= 1e-9 * magA.max(axis=(1, 2), keepdims=True)
    zb = magB <= 1e-9 * magB.max(axis=(1, 2), keepdims=True)
    tau = floor * (magA * magB).mean(axis=(1, 2))
    znorm = np.sqrt(ws * ws * ((a * a).sum(axis=(1, 2)) + (b * b).sum(axis=(1, 2))))
    F = 2 * ETA * np.log2(ws)
    spill = np.sqrt((np.where(za, W * magB, 0.0) ** 2).sum(axis=(1, 2))) + np.sqrt((np.where(zb, W * magA, 0.0) ** 2).sum(axis=(1, 2)))
    with np.errstate(all="ignore"):
        out = (F + 1) * U32 * znorm * spill / (tau * W.sum())
    return np.where(spill > 0, out, 0.0)


def model_on(mode, wa, wb, correlation, u2, v2, shape):
    """Everything the model says about staged windows wa, wb [B, N, ws, ws] of a case: the float64 map, the CPU float32
    figures, the map gate, the fields with the combine against a zero predictor (tpiv_debug_pass_spec: u0 = v0 = 0), and
    the windows with a decision inside twice the gate."""
    B, N, ws, _ = wa.shape
    nr, nc = shape
    dx, dy, floor = PM.diameters(correlation)
    top = PM.peak_scale(ws, dx, dy)
    fa, fb = wa.reshape(B * N, ws, ws).astype(np.float64), wb.reshape(B * N, ws, ws).astype(np.float64)
    C64, empty = PM.filtered_map(fa, fb, dx, dy, floor)
    C32, empty32 = PM.filtered_map(fa, fb, dx, dy, floor, f32=True)
    cpu = figures(C32, C64, top)
    cpu_packed = figures(PM.filtered_map(fa, fb, dx, dy, floor, f32=True, packed=True)[0], C64, top)
    leak = np.where(empty, 0.0, leak_bound(fa, fb, dx, dy, floor))
    gate = MARGIN * float(cpu[~empty].max()) + leak             # per window
    M = C64 - C64.min(axis=(1, 2), keepdims=True)
    close = decisions_inside(M, gate * top) & ~empty
    du, dv, inv = PM.peaks(C64, empty, mode, B * N, 1)
    du, dv, inv = du.reshape(B, nr, nc), dv.reshape(B, nr, nc), inv.reshape(B, nr, nc)
    if mode == 0:
        u, v = du, dv
    else:
        z = np.zeros((nr, nc))
        u, v = EM.combine(du, dv, inv, z, z, u2, v2)
    return {"C64": C64, "empty": empty, "empty32": empty32, "cpu": cpu, "cpu_packed": cpu_packed, "leak": leak, "gate": gate, "top": top, "u": u, "v": v,
            "inv": inv, "close": close}


CASES = [(m, ws, ov, "3x4") for m in MODES for ws in (16, 32, 64) for ov in (ws // 2, 0)] + \
        [(m, ws, ws // 2, "1x1") for m in MODES for ws in (16, 32, 64)] + \
        [(m, ws, ws // 2, "3x3") for m in MODES for ws in (16, 32)]
RUNS = [(c, "rpc24") for c in CASES] + [(c, "phase") for c in CASES if c[2] == c[1] // 2]
FILTERS = {"rpc24": RPC24, "phase": "phase"}


def run_id(r):
    c, f = r
    return f"{mode_name(c[0])}-{c[1]}-{c[2]}-{c[3]}-{f}"


@functools.lru_cache(maxsize=None)
def run_case(run):
    """Device and model results of a run, computed once and shared by the tests below (read-only)."""
    from torchpiv_amd import engine as eng
    (mode, ws, ov, grid), filt = run
    corr = FILTERS[filt]
    A, B, u2, v2 = six_pairs(mode, ws, ov, grid, CASE_SEED.get(run[0], 1))
    H, W = A.shape[1:]
    nr, nc = (int(x) for x in O.field_shape((H, W), ws, ov))
    outs = []
    for lo in (0, 3):
        kw = {}
        if mode != 0:
            kw = dict(u2=dev(np.broadcast_to(u2, (3, nr, nc))), v2=dev(np.broadcast_to(v2, (3, nr, nc))))
        outs.append([t.cpu().numpy() for t in eng.debug_pass(mode, dev(A[lo:lo + 3]), dev(B[lo:lo + 3]), ws, ov,
                                                             correlation=corr, **kw)])
    u, v, inv, win, cmap = (np.concatenate([o[k] for o in outs]) for k in range(5))
    m = model_on(mode, win[:, :, 0], win[:, :, 1], corr, u2, v2, (nr, nc))
    m.update(dev_u=u, dev_v=v, dev_inv=inv.astype(bool), dev_map=cmap.reshape(-1, ws, ws).astype(np.float64))
    return m


# ---- maps -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_maps(eng, run):
    r = run_case(run)
    got, empty = r["dev_map"], r["empty"]
    assert np.isfinite(got).all()
    assert np.array_equal(r["empty"], r["empty32"])
    flat = got.reshape(len(got), -1)
    # (the hook stores C - min + 1e-7 in float32: the zero map is float32(1e-7) in every cell)
    assert (flat[empty] == np.float64(np.float32(1e-7))).all(), (run_id(run), "an empty window's map must be exactly zero")
    fig = figures(got, r["C64"], r["top"])
    plain = ~empty & (r["leak"] == 0)            # windows without an exactly-zero bin: 4 x the CPU float32 figure alone
    worst, cpu, packed = float(fig[plain].max()), float(r["cpu"][~empty].max()), float(r["cpu_packed"][~empty].max())
    leaky = ~empty & (r["leak"] > 0)
    wl = float(fig[leaky].max()) if leaky.any() else 0.0
    bl = float(r["leak"][leaky].min()) if leaky.any() else 0.0
    print(f"  {run_id(run):28s} device {worst:.2e}  CPU float32 {cpu:.2e}  ratio {worst / cpu:.2f}; {int(leaky.sum())} windows with "
          f"exactly-zero bins: device {wl:.2e}, smallest leak bound {bl:.2e} (CPU packed complex64, all windows: {packed:.2e}); "
          f"{int(empty.sum())} of {len(empty)} windows empty")
    report(section="maps", run=run_id(run), device=worst, cpu_float32=cpu, device_zero_bin_windows=wl,
           smallest_leak_bound=bl, zero_bin_windows=int(leaky.sum()), cpu_float32_packed=packed)
    over = ~empty & (fig > r["gate"])
    assert not over.any(), (run_id(run), np.flatnonzero(over), fig[over], r["gate"][over])


# ---- fields ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_fields(eng, run):
    r = run_case(run)
    assert not r["close"].any(), (run_id(run), "the inputs leave a decision inside twice the map gate", np.flatnonzero(r["close"]))
    assert np.array_equal(r["dev_inv"], r["inv"]), (run_id(run), np.argwhere(r["dev_inv"] != r["inv"])[:5])
    live = ~r["empty"].reshape(r["inv"].shape)
    worst = max(float(np.abs(r["dev_u"] - r["u"])[live].max()), float(np.abs(r["dev_v"] - r["v"])[live].max()))
    print(f"  {run_id(run):28s} worst |field - model| {worst:.2e} px, {int(r['inv'].sum())} of {r['inv'].size} invalid")
    report(section="fields", run=run_id(run), worst_px=worst)
    assert worst <= GATE_PX, (run_id(run), worst)


# ---- plan chain -----------------------------------------------------------------------------------------------------
HC = 160
CHAIN_DENSITY = {64: 0.03, 32: 0.06}


@functools.lru_cache(maxsize=None)
def striped4(ws):
    pairs = [PM.striped_scene(s, HC, HC, density=CHAIN_DENSITY[ws]) for s in range(4)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


@pytest.mark.gpu
@pytest.mark.parametrize("ws,mode", [(64, "CWS"), (64, "DWS"), (32, "CWS")], ids=lambda x: str(x))
def test_plan_chain(eng, ws, mode):
    """Two filtered passes on four 160 x 160 pairs of the striped scene, every pass judged on its own: pass 1 against the
    model on the frames, the shifted pass against the model at the predictor the plan's own operator makes of the device's
    first-pass fields.  1e-3 px, validity identical outside windows with a decision inside twice the map gate (at most 2 %
    of a pass's windows).  And the benefit, on the device fields: with "rpc" no invalid vector and none more than 1 px
    off; for 64/32 -> 32/16 CWS an RMS against the constructed flow of at most a quarter of the plain plan's."""
    A, B = striped4(ws)
    dA, dB = dev(A), dev(B)
    ov = ws // 2
    plan = eng.Plan(HC, HC, ws, ov, n_pass=2, mode=mode, max_batch=4, correlation="rpc")
    assert all("xcorr_spec_kernel" in plan.kernel_name(p) for p in range(2))
    u, v, inv = plan.run(dA, dB)
    first = plan.pass_fields(0, 4)
    u0, v0, u2, v2 = (t.cpu().numpy() for t in plan.debug_predict(1, *first))
    steps = [tuple(t.cpu().numpy() for t in first), tuple(t.cpu().numpy() for t in (u, v, inv))]
    dx, dy, floor = PM.diameters("rpc")
    worst = 0.0
    for p, (w, o, nr, nc) in enumerate(plan.geometry):
        top = PM.peak_scale(w, dx, dy)
        for i in range(4):
            if p == 0:
                wa, wb = PM.windows(0, A[i], B[i], w, o)
            else:
                wa, wb = PM.windows(mode, A[i], B[i], w, o, u2[i], v2[i])
            C64, empty = PM.filtered_map(wa, wb, dx, dy, floor)
            C32, _ = PM.filtered_map(wa, wb, dx, dy, floor, f32=True)
            gate = MARGIN * float(figures(C32, C64, top)[~empty].max()) + np.where(empty, 0.0, leak_bound(wa, wb, dx, dy, floor))
            M = C64 - C64.min(axis=(1, 2), keepdims=True)
            close = decisions_inside(M, gate * top).reshape(nr, nc)
            du, dv, minv = PM.peaks(C64, empty, 0 if p == 0 else mode, nr, nc)
            mu, mv = (du, dv) if p == 0 else EM.combine(du, dv, minv, u0[i], v0[i], u2[i], v2[i])
            gu, gv, ginv = steps[p][0][i], steps[p][1][i], steps[p][2][i].astype(bool)
            assert close.mean() <= 0.02, (p, i, float(close.mean()))
            assert np.array_equal(ginv[~close], minv[~close]), (p, i)
            ok = ~close & ~empty.reshape(nr, nc)
            worst = max(worst, float(np.abs(gu - mu)[ok].max()), float(np.abs(gv - mv)[ok].max()))
    assert worst <= GATE_PX, worst
    # ---- the benefit, on the device fields
    off = eng.Plan(HC, HC, ws, ov, n_pass=2, mode=mode, max_batch=4)
    pu, pv, pinv = (t.cpu().numpy() for t in off.run(dA, dB))
    wl, ol, nr, nc = plan.geometry[-1]
    gu, gv, ginv = steps[1]
    rms_rpc, rms_plain, n_plain = [], [], 0
    for i in range(4):
        n_inv, n_far, rms = PM.score(gu[i], gv[i], ginv[i].astype(bool), HC, HC, wl, ol)
        assert n_inv == 0 and n_far == 0, (i, n_inv, n_far)
        rms_rpc.append(rms)
        pn, _, prms = PM.score(pu[i], pv[i], pinv[i].astype(bool), HC, HC, wl, ol)
        n_plain += pn
        rms_plain.append(prms)
    print(f"  {ws}/{ov} -> {wl}/{ol} {mode}: chain against the model {worst:.2e} px; RMS against the flow rpc "
          f"{np.mean(rms_rpc):.3f} px (no invalid vector), plain {np.mean(rms_plain):.3f} px ({n_plain} of {4 * nr * nc} invalid)")
    report(section="chain", chain=f"{ws}/{ov}->{wl}/{ol} {mode}", rpc_rms_px=float(np.mean(rms_rpc)),
           plain_rms_px=float(np.mean(rms_plain)), plain_invalid=n_plain, chain_vs_model_px=worst)
    if (ws, mode) == (64, "CWS"):
        for a_, b_ in zip(rms_rpc, rms_plain):
            assert a_ <= 0.25 * b_, (a_, b_)
    plan.close()
    off.close()


# ---- off means off --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_off_means_off(eng):
    """A plan without the keyword, one with correlation=None and one switched on and off again: the same kernel names, the
    same bits.  The same calls give the same bits, with the filter too."""
    A, B = striped4(64)
    dA, dB = dev(A), dev(B)
    for mode in ("CWS", "DWS"):
        p0 = eng.Plan(HC, HC, 32, 16, n_pass=2, mode=mode, max_batch=4)
        p1 = eng.Plan(HC, HC, 32, 16, n_pass=2, mode=mode, max_batch=4, correlation=None)
        p2 = eng.Plan(HC, HC, 32, 16, n_pass=2, mode=mode, max_batch=4, correlation="rpc")
        names = [p0.kernel_name(p) for p in range(2)]
        assert names == [p1.kernel_name(p) for p in range(2)] and all("spec" not in n for n in names)
        assert all("xcorr_spec_kernel" in p2.kernel_name(p) for p in range(2))
        r0 = [t.cpu().numpy().tobytes() for t in p0.run(dA, dB)]
        r2 = [t.cpu().numpy().tobytes() for t in p2.run(dA, dB)]
        assert r2 == [t.cpu().numpy().tobytes() for t in p2.run(dA, dB)]
        assert r2 != r0
        p2.set_correlation(None)
        assert names == [p2.kernel_name(p) for p in range(2)]
        for pl in (p1, p2):
            assert r0 == [t.cpu().numpy().tobytes() for t in pl.run(dA, dB)], mode
        assert r0 == [t.cpu().numpy().tobytes() for t in p0.run(dA, dB)]
        for pl in (p0, p1, p2):
            pl.close()


# ---- every path -----------------------------------------------------------------------------------------------------
def _fields(gen):
    out = {}
    for i, x, y, u, v in gen:
        out[i] = tuple(f.cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f) for f in (u, v))
    return out


def _same(f1, f2):
    assert sorted(f1) == sorted(f2)
    for i in f1:
        for k in (0, 1):
            assert np.ascontiguousarray(f1[i][k]).tobytes() == np.ascontiguousarray(f2[i][k]).tobytes(), (i, k)


@pytest.mark.gpu
@pytest.mark.parametrize("extra", ["plain", "mask", "outlier"])
def test_every_path(eng, tmp_path, extra):
    """One pair at a time, batched(), the file path and ResidentPIV with device_out give the fields of the plan on two
    96 x 112 pairs (a dark block leaves each pair a few invalid vectors: the reference drops a pair without any); once
    with mask= and once with outlier="median" to show that they compose."""
    from PIL import Image
    import torchpiv_amd.backend as T
    Hp, Wp = 96, 112
    pairs = [EM.scene(40 + i, Hp, Wp, density=0.03) for i in range(2)]
    A, B = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    A[:, 36:68, 44:76] = 0              # (wide enough that four 16 x 16 windows stay inside it under their shift)
    B[:, 36:68, 44:76] = 0
    for i in range(2):
        Image.fromarray(A[i], "L").save(tmp_path / f"image{i}_a.bmp")
        Image.fromarray(B[i], "L").save(tmp_path / f"image{i}_b.bmp")
    img = np.zeros((Hp, Wp), np.uint8)
    img[:, :20] = 1
    kw = {"plain": {}, "mask": {"mask": img}, "outlier": {"outlier": "median"}}[extra]
    base = dict(multipass=2, multipass_mode="CWS", correlation="rpc", **kw)
    dA, dB = dev(A), dev(B)
    res = T.ResidentPIV(dA, dB, 32, 16, **base)
    want = _fields(res.batched(2))
    assert len(want) == 2
    res.device_out = True
    _same(_fields(res.batched(2)), want)
    piv = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", 32, 16, **base)
    _same(_fields(piv.batched(2)), want)
    piv.call_batch = 1
    out = list(piv())
    assert len(out) == 2
    for i, (x, y, u, v) in enumerate(out):
        assert np.asarray(u).tobytes() == want[i][0].tobytes() and np.asarray(v).tobytes() == want[i][1].tobytes()
    # the plan on the same frames (mask=: the pixel step is the host classes' own)
    fa, fb = dA, dB
    if extra == "mask":
        fa, fb = eng.apply_mask(dA, dev(img)), eng.apply_mask(dB, dev(img))
    plan = eng.Plan(Hp, Wp, 32, 16, n_pass=2, mode="CWS", max_batch=2, correlation="rpc", **kw)
    u, v, inv = (t.cpu().numpy() for t in plan.run(fa, fb))
    for i in range(2):
        bad = inv[i].astype(bool)
        assert bad.any()
        pu, pv = T.post_validate(u[i].copy(), v[i].copy(), bad)
        assert np.allclose(want[i][0], np.flip(pu, axis=0) * 1000, rtol=0, atol=1e-9)         # scale 1, dt 1: x 1000 (B:894-898)
        assert np.allclose(want[i][1], -np.flip(pv, axis=0) * 1000, rtol=0, atol=1e-9)
    # ... and not the fields of a run without the keyword
    plain = _fields(T.ResidentPIV(dA, dB, 32, 16, multipass=2, multipass_mode="CWS", **kw).batched(2))
    assert any(i not in plain or plain[i][0].tobytes() != want[i][0].tobytes() for i in want)
    for p in (res, piv, plan):
        p.close()


# ---- refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_through_the_c_abi(eng):
    """Every refusal of tpiv_plan_set_correlation and tpiv_debug_pass_spec, and a failed call changes nothing."""
    import ctypes as C
    from torchpiv_amd import _lib
    lib = _lib.lib
    A, B = striped4(64)
    dA, dB = dev(A[:2]), dev(B[:2])

    def set_corr(plan, kind, dx, dy, floor, tab):
        return lib.tpiv_plan_set_correlation(plan._h, kind, dx, dy, floor, None if tab is None else tab.ctypes.data,
                                             0 if tab is None else tab.size)
    good = eng.correlation_tables(eng.correlation_arg("rpc"), [32, 16])
    plan = eng.Plan(HC, HC, 32, 16, n_pass=2, mode="CWS", max_batch=2)
    before = [t.cpu().numpy().tobytes() for t in plan.run(dA, dB)]
    names = [plan.kernel_name(p) for p in range(2)]
    for args in ((3, 2.8, 2.8, 2.0 ** -10, good), (-1, 2.8, 2.8, 2.0 ** -10, good), (2, -1.0, 2.8, 2.0 ** -10, good),
                 (2, 2.8, 16.5, 2.0 ** -10, good), (2, 2.8, 2.8, 2.0 ** -21, good), (2, 2.8, 2.8, 0.1, good),
                 (2, float("nan"), 2.8, 2.0 ** -10, good), (1, 2.0, 0.0, 2.0 ** -10, good), (2, 2.8, 2.8, 2.0 ** -10, None),
                 (2, 2.8, 2.8, 2.0 ** -10, good[:-1])):
        assert set_corr(plan, *args) == _lib.EINVAL, args
        assert names == [plan.kernel_name(p) for p in range(2)]
    assert before == [t.cpu().numpy().tobytes() for t in plan.run(dA, dB)]
    # combinations, both ways round
    assert lib.tpiv_plan_set_uncertainty(plan._h, 1, 3) == _lib.OK
    assert set_corr(plan, 2, 2.8, 2.8, 2.0 ** -10, good) == _lib.EINVAL and b"uncertainty" in lib.tpiv_last_error()
    assert lib.tpiv_plan_set_uncertainty(plan._h, 0, 3) == _lib.OK
    assert lib.tpiv_plan_set_deform(plan._h, 1, _lib.DEWARP_LINEAR, 1, None) == _lib.OK
    assert set_corr(plan, 2, 2.8, 2.8, 2.0 ** -10, good) == _lib.EINVAL and b"deform" in lib.tpiv_last_error()
    assert lib.tpiv_plan_set_deform(plan._h, 0, 0, 1, None) == _lib.OK
    assert lib.tpiv_plan_set_ensemble(plan._h, 1) == _lib.OK
    assert set_corr(plan, 2, 2.8, 2.8, 2.0 ** -10, good) == _lib.EINVAL and b"ensemble" in lib.tpiv_last_error()
    assert lib.tpiv_plan_set_ensemble(plan._h, 0) == _lib.OK
    assert names == [plan.kernel_name(p) for p in range(2)]
    assert set_corr(plan, 2, 2.8, 2.8, 2.0 ** -10, good) == _lib.OK
    on = [t.cpu().numpy().tobytes() for t in plan.run(dA, dB)]
    assert on != before
    assert lib.tpiv_plan_set_uncertainty(plan._h, 1, 3) == _lib.EINVAL and b"correlation" in lib.tpiv_last_error()
    assert lib.tpiv_plan_set_deform(plan._h, 1, _lib.DEWARP_LINEAR, 1, None) == _lib.EINVAL
    assert lib.tpiv_plan_set_ensemble(plan._h, 1) == _lib.EINVAL
    assert set_corr(plan, 2, 99.0, 2.8, 2.0 ** -10, good) == _lib.EINVAL          # a failed call leaves the filter as it was
    assert on == [t.cpu().numpy().tobytes() for t in plan.run(dA, dB)]
    assert set_corr(plan, 0, 0.0, 0.0, 0.0, None) == _lib.OK
    assert before == [t.cpu().numpy().tobytes() for t in plan.run(dA, dB)]
    plan.close()
    # window sizes: the message names the size
    for ws, n_pass, bad in ((8, 1, 8), (128, 1, 128), (24, 1, 24), (32, 3, 8)):
        pl = eng.Plan(256, 256, ws, ws // 2, n_pass=n_pass, mode="CWS", max_batch=1)
        sizes = [g[0] for g in pl.geometry]
        tab = np.ones(sum(2 * (w // 2 + 1) for w in sizes), np.float32)
        assert set_corr(pl, 1, 0.0, 0.0, 2.0 ** -10, tab) == _lib.EUNSUPPORTED
        assert str(bad).encode() in lib.tpiv_last_error()
        pl.close()
    # the one-pass entry: sizes and CWS_Fast
    z = dev(np.zeros((1, 256, 256), np.uint8))
    for ws in (8, 24, 128):
        with pytest.raises(NotImplementedError, match=str(ws)):
            eng.debug_pass(0, z, z, ws, ws // 2, correlation="phase")
    nr, nc = eng.field_shape(256, 256, 32, 16)
    f = dev(np.zeros((1, nr, nc)))
    with pytest.raises(NotImplementedError, match="CWS_Fast"):
        eng.debug_pass("CWS_Fast", z, z, 32, 16, u2=f, v2=f, correlation="rpc")
    # the host classes refuse ensemble() with the keyword
    import torchpiv_amd.backend as T
    res = T.ResidentPIV(dA, dB, 32, 16, multipass=2, correlation="rpc")
    with pytest.raises(ValueError, match="correlation"):
        res.ensemble()
    res.close()
    tab = dev(np.ones(34, np.float32))
    work = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    rc = lib.tpiv_debug_pass_spec(_lib.MODE_CWS_FAST, 2, 2.0 ** -10, tab.data_ptr(), z.data_ptr(), z.data_ptr(), 1, 256, 256,
                                  32, 16, f.data_ptr(), f.data_ptr(), f.data_ptr(), None, None, None, None, None,
                                  work.data_ptr(), work.numel(), None)
    assert rc == _lib.EUNSUPPORTED


# ---- timing and the exact scheme's read-outs on a filtered plan -----------------------------------------------------
@pytest.mark.gpu
def test_timing_and_exact_readouts_on_a_default_precision_plan(eng):
    """A filtered plan at the default precision ("exact") holds the exact scheme's counter and sub-events but records none:
    get_timing works (and keeps working), exact_fallbacks refuses after a filtered run and answers after a plain one, and
    runs of both kinds inside one timing window are averaged each over its own."""
    A, B = striped4(64)
    dA, dB = dev(A[:2]), dev(B[:2])
    plan = eng.Plan(HC, HC, 64, 32, n_pass=2, mode="CWS", max_batch=2, correlation="rpc")
    plan.set_timing(True)
    for rep_ in range(2):
        plan.run(dA, dB)
        plan.run(dA, dB)
        t, n = plan.get_timing()
        assert n == 2 and all(v > 0 for v in t.values()), (rep_, t, n)
    with pytest.raises(ValueError):
        plan.exact_fallbacks()
    plan.run(dA, dB)                                 # one filtered and one plain run in the same window
    plan.set_correlation(None)
    plan.run(dA, dB)
    assert plan.exact_fallbacks() >= 0
    t, n = plan.get_timing()
    assert n == 2 and all(v > 0 for v in t.values())
    plan.close()


# ---- precision has no effect ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_precision_has_no_effect(eng):
    A, B = striped4(64)
    dA, dB = dev(A[:2]), dev(B[:2])
    got = []
    for prec in ("fast", "f64", "exact", "reference"):
        plan = eng.Plan(HC, HC, 64, 32, n_pass=2, mode="CWS", max_batch=2, precision=prec, correlation="rpc")
        got.append([t.cpu().numpy().tobytes() for t in plan.run(dA, dB)])
        plan.close()
    assert all(g == got[0] for g in got)
    # the workspace too: one-pass plans with few windows, whose float64 records alone are smaller than the float32 layout
    for ws, batch in ((64, 1), (32, 1), (16, 1)):
        h = 2 * ws if ws < 64 else HC
        fa, fb = dev(A[:1, :h, :h]), dev(B[:1, :h, :h])
        got = []
        for prec in ("fast", "f64", "exact", "reference"):
            plan = eng.Plan(h, h, ws, ws // 2, n_pass=1, max_batch=batch, precision=prec, correlation="rpc")
            got.append([t.cpu().numpy().tobytes() for t in plan.run(fa, fb)])
            plan.close()
        assert all(g == got[0] for g in got), ws
