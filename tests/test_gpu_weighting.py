"""Weighted interrogation windows (weighting="gaussian" / "uniform", xcorr_win.hip) on the device against the float64 model
of tests/weighting_model.py: every instance's map cell by cell, its fields, "uniform" against the plain float32 pass, the
plan chain with and without deform= on the scene of tests/deform_model.py, and the host paths.  The method is that of
tests/test_gpu_phase.py.

Maps.  The device map against the model on the device's OWN staged windows (tpiv_debug_pass_weighted reports them).  Per
window: half the spread of (device - model) over the peak-to-minimum range of the model map of a pure-shift pair
(weighting_model.shift_scale: the range of the weighted window's circular auto-correlation; for a general pair the
geometric mean of the two frames' ranges).  The gate is not a fixed number: it is 4 x the worst such figure of the CPU
float32 evaluation (torch.fft, complex64) of the same windows of the same case, the margin tests/test_gpu_f64_pass1.py gives
a device transform over a CPU transform of equal precision.  An empty window (no energy in a frame) has a map that is
exactly zero.
Fields.  u, v, invalid against corr_to_disp on the model map plus the combine: 1e-3 px (BASELINE.json's gate for float32
passes), identical validity, no window excused; that no arg-max margin, peak ratio or fit denominator of the model lies
inside twice the map gate is asserted on the model first (test_gpu_phase.decisions_inside).  For empty windows only
`invalid` is compared.
The seeds of the inputs were chosen on the CPU (oracle-staged windows) before any device run: CASE_SEED.

TPIV_WEIGHTING_REPORT=<file>: the figures are appended there as JSON lines (profiles/weighting/measurements.json keeps a
run's).
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import piv_oracle as O
import deform_model as DM
import ensemble_model as EM
import weighting_model as WM
from test_gpu_phase import six_pairs, decisions_inside

GATE_PX = 1e-3
MARGIN = 4.0
MODES = (0, "DWS", "CWS")
ANISO = {"kind": "gaussian", "sigma": (0.3, 0.6)}
REPORT = os.environ.get("TPIV_WEIGHTING_REPORT")


def report(**kw):
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(json.dumps(kw) + "\n")


def mode_name(m):
    return m or "PASS1"


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


def bits(ts):
    return [t.cpu().numpy().tobytes() for t in ts]


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def figures(got, want, scale):
    """Per window: half the spread of (got - want) over the window's scale (0 where the scale is 0: an empty window)."""
    d = (got - want).reshape(len(got), -1)
    with np.errstate(all="ignore"):
        return np.where(scale > 0, (d.max(axis=1) - d.min(axis=1)) / (2.0 * scale), 0.0)


def model_on(mode, wa, wb, weighting, u2, v2, shape):
    """Everything the model says about staged windows wa, wb [B, N, ws, ws] of a case: the float64 map, the CPU float32
    figures, the map gate, the fields with the combine against a zero predictor (tpiv_debug_pass_weighted: u0 = v0 = 0), and
    the windows with a decision inside twice the gate."""
    B, N, ws, _ = wa.shape
    nr, nc = shape
    W = WM.weight(ws, weighting)
    first = mode == 0
    fa, fb = wa.reshape(B * N, ws, ws).astype(np.float64), wb.reshape(B * N, ws, ws).astype(np.float64)
    C64, empty = WM.weighted_map(fa, fb, W, first)
    C32, empty32 = WM.weighted_map(fa, fb, W, first, f32=True)
    scale = WM.shift_scale(fa, fb, W, first)
    cpu = figures(C32, C64, scale)
    gate = MARGIN * float(cpu[~empty].max())
    M = C64 - C64.min(axis=(1, 2), keepdims=True)
    close = decisions_inside(M, gate * scale) & ~empty
    du, dv, inv = WM.peaks(C64, empty, mode, B * N, 1)
    du, dv, inv = du.reshape(B, nr, nc), dv.reshape(B, nr, nc), inv.reshape(B, nr, nc)
    if first:
        u, v = du, dv
    else:
        z = np.zeros((nr, nc))
        u, v = EM.combine(du, dv, inv, z, z, u2, v2)
    return {"C64": C64, "empty": empty, "empty32": empty32, "cpu": cpu, "gate": gate, "scale": scale, "u": u, "v": v,
            "inv": inv, "close": close}


CASES = [(m, ws, ov, "3x4") for m in MODES for ws in (16, 32, 64) for ov in (ws // 2, 0, 3 * ws // 4)] + \
        [(m, ws, ws // 2, "1x1") for m in MODES for ws in (16, 32, 64)] + \
        [(m, ws, ws // 2, "3x3") for m in MODES for ws in (16, 32)]
RUNS = [(c, "gaussian") for c in CASES] + [(c, "aniso") for c in CASES if c[2] == c[1] // 2 and c[3] == "3x4"]
WEIGHTS = {"gaussian": "gaussian", "aniso": ANISO, "uniform": "uniform"}
# (mode, ws, ov, grid) -> seed of six_pairs, where seed 1 leaves a decision of the model inside twice the map gate (found on
# the CPU with oracle-staged windows, before any device run)
CASE_SEED = {}


def run_id(r):
    c, f = r
    return f"{mode_name(c[0])}-{c[1]}-{c[2]}-{c[3]}-{f}"


def case_inputs(case):
    mode, ws, ov, grid = case
    return six_pairs(mode, ws, ov, grid, CASE_SEED.get(case, 1))


@functools.lru_cache(maxsize=None)
def run_case(run):
    """Device and model results of a run, computed once and shared by the tests below (read-only)."""
    from torchpiv_amd import engine as eng
    (mode, ws, ov, grid), wname = run
    wt = WEIGHTS[wname]
    A, B, u2, v2 = case_inputs(run[0])
    H, W = A.shape[1:]
    nr, nc = (int(x) for x in O.field_shape((H, W), ws, ov))
    outs = []
    for lo in (0, 3):
        kw = {}
        if mode != 0:
            kw = dict(u2=dev(np.broadcast_to(u2, (3, nr, nc))), v2=dev(np.broadcast_to(v2, (3, nr, nc))))
        outs.append([t.cpu().numpy() for t in eng.debug_pass(mode, dev(A[lo:lo + 3]), dev(B[lo:lo + 3]), ws, ov,
                                                             weighting=wt, **kw)])
    u, v, inv, win, cmap = (np.concatenate([o[k] for o in outs]) for k in range(5))
    m = model_on(mode, win[:, :, 0], win[:, :, 1], wt, u2, v2, (nr, nc))
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
    assert empty.any() and not empty.all()
    flat = got.reshape(len(got), -1)
    # (the hook stores C - min + 1e-7 in float32: the zero map is float32(1e-7) in every cell)
    assert (flat[empty] == np.float64(np.float32(1e-7))).all(), (run_id(run), "an empty window's map must be exactly zero")
    fig = figures(got, r["C64"], r["scale"])
    worst, cpu = float(fig[~empty].max()), float(r["cpu"][~empty].max())
    print(f"  {run_id(run):30s} device {worst:.2e}  CPU float32 {cpu:.2e}  ratio {worst / cpu:.2f}; "
          f"{int(empty.sum())} of {len(empty)} windows empty")
    report(section="maps", run=run_id(run), device=worst, cpu_float32=cpu, ratio=worst / cpu)
    over = ~empty & (fig > r["gate"])
    assert not over.any(), (run_id(run), np.flatnonzero(over), fig[over], r["gate"])


# ---- fields ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_fields(eng, run):
    r = run_case(run)
    assert not r["close"].any(), (run_id(run), "the inputs leave a decision inside twice the map gate", np.flatnonzero(r["close"]))
    assert np.array_equal(r["dev_inv"], r["inv"]), (run_id(run), np.argwhere(r["dev_inv"] != r["inv"])[:5])
    assert np.isfinite(r["dev_u"]).all() and np.isfinite(r["dev_v"]).all()
    live = ~r["empty"].reshape(r["inv"].shape)
    worst = max(float(np.abs(r["dev_u"] - r["u"])[live].max()), float(np.abs(r["dev_v"] - r["v"])[live].max()))
    print(f"  {run_id(run):30s} worst |field - model| {worst:.2e} px, {int(r['inv'].sum())} of {r['inv'].size} invalid")
    report(section="fields", run=run_id(run), worst_px=worst)
    assert worst <= GATE_PX, (run_id(run), worst)
    if run[0][0] == 0:        # first pass: an empty window is dead -- u = v = 0, valid
        dead = ~live
        assert not r["dev_u"][dead].any() and not r["dev_v"][dead].any() and not r["dev_inv"][dead].any()


# ---- "uniform" against the plain float32 pass -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c[2] == c[1] // 2 and c[3] == "3x4"], ids=lambda c: run_id((c, "uniform")))
def test_uniform_is_the_plain_float32_pass(eng, case):
    """The particle pairs (0 and 5) of the case through the weighted kernel with all-ones tables and through the plain
    float32 kernel (precision="fast", no keyword): 1e-3 px and identical validity outside the decision band of the model."""
    mode, ws, ov, grid = case
    A, B, u2, v2 = case_inputs(case)
    A, B = A[[0, 5]], B[[0, 5]]
    nr, nc = (int(x) for x in O.field_shape(A.shape[1:], ws, ov))
    kw = {}
    if mode != 0:
        kw = dict(u2=dev(np.broadcast_to(u2, (2, nr, nc))), v2=dev(np.broadcast_to(v2, (2, nr, nc))))
    wu, wv, winv, win, _ = (t.cpu().numpy() for t in eng.debug_pass(mode, dev(A), dev(B), ws, ov, weighting="uniform", **kw))
    pu, pv, pinv, pwin, _ = (t.cpu().numpy() for t in eng.debug_pass(mode, dev(A), dev(B), ws, ov, precision="fast", **kw))
    assert np.array_equal(win, pwin)                     # the same staging
    m = model_on(mode, win[:, :, 0], win[:, :, 1], "uniform", u2, v2, (nr, nc))
    ok = ~m["close"].reshape(2, nr, nc)
    assert ok.mean() >= 0.98
    assert np.array_equal(winv.astype(bool)[ok], pinv.astype(bool)[ok])
    worst = max(float(np.abs(wu - pu)[ok].max()), float(np.abs(wv - pv)[ok].max()))
    print(f"  {run_id((case, 'uniform')):30s} worst |uniform - plain float32| {worst:.2e} px")
    report(section="uniform vs plain", run=run_id((case, "uniform")), worst_px=worst)
    assert worst <= GATE_PX, worst


# ---- plan chain -----------------------------------------------------------------------------------------------------
HC = 160


@functools.lru_cache(maxsize=None)
def deform4():
    pairs = [DM.scene(s, HC, HC) for s in range(4)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def judge_pass(first, mode, wa, wb, weighting, shape, got, predictor=None):
    """One pass of one pair against the model on windows wa, wb: validity identical and fields within 1e-3 px outside the
    windows with a decision inside twice the map gate (at most 2 % of them)."""
    nr, nc = shape
    ws = wa.shape[-1]
    W = WM.weight(ws, weighting)
    C64, empty = WM.weighted_map(wa, wb, W, first)
    C32, _ = WM.weighted_map(wa, wb, W, first, f32=True)
    scale = WM.shift_scale(wa, wb, W, first)
    gate = MARGIN * float(figures(C32, C64, scale)[~empty].max())
    M = C64 - C64.min(axis=(1, 2), keepdims=True)
    close = (decisions_inside(M, gate * scale) & ~empty).reshape(nr, nc)
    du, dv, minv = WM.peaks(C64, empty, 0 if first else mode, nr, nc)
    mu, mv = (du, dv) if first else EM.combine(du, dv, minv, *predictor)
    gu, gv, ginv = got
    assert close.mean() <= 0.02, float(close.mean())
    assert np.array_equal(ginv.astype(bool)[~close], minv[~close])
    ok = ~close & ~empty.reshape(nr, nc)
    return max(float(np.abs(gu - mu)[ok].max()), float(np.abs(gv - mv)[ok].max()))


@pytest.mark.gpu
def test_plan_chain_and_deformation_rounds(eng):
    """64/48 -> 32/24 CWS with "gaussian" on four 160 x 160 pairs of the deform scene, every pass judged on its own: pass 1
    against the model on the frames, the shifted pass against the model at the predictor the plan's own operator makes of
    the device's first-pass fields.  Then the same plan with deform=3: it equals, bit for bit, the rounds unrolled from the
    function level with the weighted first pass as the residual pass (the way tests/test_gpu_deform.py unrolls them), and
    the residual pass of every round is judged against the model on that round's warped frames.  The final RMS against the
    constructed flow is below the "uniform" plan's, with and without the rounds."""
    A, B = deform4()
    dA, dB = dev(A), dev(B)
    wt = "gaussian"
    plan = eng.Plan(HC, HC, 64, 48, n_pass=2, mode="CWS", max_batch=4, weighting=wt)
    assert all("xcorr_win_kernel" in plan.kernel_name(p) for p in range(2))
    u, v, inv = plan.run(dA, dB)
    first = plan.pass_fields(0, 4)
    u0, v0, u2, v2 = (t.cpu().numpy() for t in plan.debug_predict(1, *first))
    steps = [tuple(t.cpu().numpy() for t in first), tuple(t.cpu().numpy() for t in (u, v, inv))]
    worst = 0.0
    for p, (w, o, nr, nc) in enumerate(plan.geometry):
        for i in range(4):
            if p == 0:
                wa, wb = WM.windows(0, A[i], B[i], w, o)
                pred = None
            else:
                wa, wb = WM.windows("CWS", A[i], B[i], w, o, u2[i], v2[i])
                pred = (u0[i], v0[i], u2[i], v2[i])
            worst = max(worst, judge_pass(p == 0, "CWS", wa, wb, wt, (nr, nc), tuple(s[i] for s in steps[p]), pred))
    assert worst <= GATE_PX, worst
    # ---- deform=3: the unrolled rounds, bit for bit, and every round's residual pass against the model
    ws, ov, nr, nc = plan.geometry[-1]
    on = eng.Plan(HC, HC, 64, 48, n_pass=2, mode="CWS", max_batch=4, weighting=wt, deform=3)
    du_, dv_, dinv_ = on.run(dA, dB)
    cu, cv, cinv = u, v, inv
    worst_round = 0.0
    for k in range(3):
        nd = eng.deform_nodes(cu, cv, cinv, smooth=True)
        fa, fb = eng.deform_warp(dA, dB, nd, ws, ov, interp="cubic")
        ru, rv, rval = eng.debug_pass(0, fa, fb, ws, ov, weighting=wt)[:3]
        ha, hb = fa.cpu().numpy(), fb.cpu().numpy()
        for i in range(4):
            wa, wb = WM.windows(0, ha[i], hb[i], ws, ov)
            worst_round = max(worst_round, judge_pass(True, 0, wa, wb, wt, (nr, nc),
                                                      (ru[i].cpu().numpy(), rv[i].cpu().numpy(), rval[i].cpu().numpy())))
        cu, cv, cinv = eng.deform_combine(nd, ru, rv, rval)
    assert bits((du_, dv_, dinv_)) == bits((cu, cv, cinv))
    stage = on.deform_stage(4)
    assert torch.equal(stage[1], fa) and torch.equal(stage[2], fb) and bits(stage[3:5]) == bits((ru, rv))
    assert worst_round <= GATE_PX, worst_round
    # either order of the two calls
    other = eng.Plan(HC, HC, 64, 48, n_pass=2, mode="CWS", max_batch=4, deform=3)
    other.set_weighting(wt)
    assert bits(other.run(dA, dB)) == bits((du_, dv_, dinv_))
    other.close()
    # ---- the benefit, on the device fields
    tu, tv = DM.truth(HC, HC, ws, ov)

    def rms_of(fu, fv, finv):
        fu, fv, finv = (t.cpu().numpy() for t in (fu, fv, finv))
        return float(np.mean([DM.rms_interior(fu[i], fv[i], tu, tv, ~finv[i].astype(bool))[0] for i in range(4)]))
    uni = eng.Plan(HC, HC, 64, 48, n_pass=2, mode="CWS", max_batch=4, weighting="uniform")
    uni3 = eng.Plan(HC, HC, 64, 48, n_pass=2, mode="CWS", max_batch=4, weighting="uniform", deform=3)
    g0, g3 = rms_of(u, v, inv), rms_of(du_, dv_, dinv_)
    t0, t3 = rms_of(*uni.run(dA, dB)), rms_of(*uni3.run(dA, dB))
    print(f"  64/48 -> 32/24 CWS: passes against the model {worst:.2e} px, rounds {worst_round:.2e} px; RMS against the flow "
          f"gaussian {g0:.3f} px, uniform {t0:.3f} px; with deform=3 gaussian {g3:.3f} px, uniform {t3:.3f} px")
    report(section="chain", chain="64/48->32/24 CWS", passes_vs_model_px=worst, rounds_vs_model_px=worst_round,
           gaussian_rms_px=g0, uniform_rms_px=t0, gaussian_deform3_rms_px=g3, uniform_deform3_rms_px=t3)
    assert g0 < t0 and g3 < t3, (g0, t0, g3, t3)
    for p in (plan, on, uni, uni3):
        p.close()


# ---- off means off --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_off_means_off(eng):
    """A plan without the keyword, one with weighting=None and one switched on and off again: the same kernel names, the
    same bits.  The same calls give the same bits, with the weight too."""
    A, B = deform4()
    dA, dB = dev(A), dev(B)
    for mode in ("CWS", "DWS"):
        p0 = eng.Plan(HC, HC, 32, 16, n_pass=2, mode=mode, max_batch=4)
        p1 = eng.Plan(HC, HC, 32, 16, n_pass=2, mode=mode, max_batch=4, weighting=None)
        p2 = eng.Plan(HC, HC, 32, 16, n_pass=2, mode=mode, max_batch=4, weighting="gaussian")
        names = [p0.kernel_name(p) for p in range(2)]
        assert names == [p1.kernel_name(p) for p in range(2)] and all("win" not in n for n in names)
        assert all("xcorr_win_kernel" in p2.kernel_name(p) for p in range(2))
        r0 = bits(p0.run(dA, dB))
        r2 = bits(p2.run(dA, dB))
        assert r2 == bits(p2.run(dA, dB))
        assert r2 != r0
        p2.set_weighting(None)
        assert names == [p2.kernel_name(p) for p in range(2)]
        for pl in (p1, p2):
            assert r0 == bits(pl.run(dA, dB)), mode
        assert r0 == bits(p0.run(dA, dB))
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
    """One pair at a time, batched(), the file path, ResidentPIV with device_out and run_folder give the fields of the
    plan on two 96 x 112 pairs (a dark block leaves each pair a few invalid vectors: the reference drops a pair without
    any); once with mask= and once with outlier="median" to show that they compose."""
    from PIL import Image
    import torchpiv_amd.backend as T
    from torchpiv_amd import runner
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
    base = dict(multipass=2, multipass_mode="CWS", weighting="gaussian", **kw)
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
    seen = {}
    table, done = runner.run_folder(str(tmp_path), "cuda:0", "bmp", 32, 16, batch_size=2, on_pair=lambda i, o: seen.__setitem__(
        i, tuple(np.asarray(o[k].cpu() if isinstance(o[k], torch.Tensor) else o[k]).copy() for k in ("Vx[m/s]", "Vy[m/s]"))), **base)
    assert done == 2 and sorted(seen) == [0, 1]
    for i in seen:
        assert np.array_equal(seen[i][0], want[i][0], equal_nan=True) and np.array_equal(seen[i][1], want[i][1], equal_nan=True)
    # the plan on the same frames (mask=: the pixel step is the host classes' own)
    fa, fb = dA, dB
    if extra == "mask":
        fa, fb = eng.apply_mask(dA, dev(img)), eng.apply_mask(dB, dev(img))
    plan = eng.Plan(Hp, Wp, 32, 16, n_pass=2, mode="CWS", max_batch=2, weighting="gaussian", **kw)
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
    """Every refusal of tpiv_plan_set_weighting and tpiv_debug_pass_weighted; nothing is launched, and a failed call
    changes nothing."""
    from torchpiv_amd import _lib
    lib = _lib.lib
    A, B = deform4()
    dA, dB = dev(A[:2]), dev(B[:2])

    def set_wt(plan, kind, sx, sy, tab):
        return lib.tpiv_plan_set_weighting(plan._h, kind, sx, sy, None if tab is None else tab.ctypes.data,
                                           0 if tab is None else tab.size)
    good = eng.weighting_tables(eng.weighting_arg("gaussian"), [32, 16])
    ones = np.ones_like(good)

    def spoiled(value, at=5):
        t = good.copy()
        t[at] = value
        return t
    plan = eng.Plan(HC, HC, 32, 16, n_pass=2, mode="CWS", max_batch=2)
    before = bits(plan.run(dA, dB))
    names = [plan.kernel_name(p) for p in range(2)]
    for args in ((3, 0.4, 0.4, good), (-1, 0.4, 0.4, good), (2, 0.19, 0.4, good), (2, 0.4, 4.5, good),
                 (2, float("nan"), 0.4, good), (2, 0.4, 0.4, None), (2, 0.4, 0.4, good[:-1]),
                 (2, 0.4, 0.4, np.concatenate([good, good[:1]])), (2, 0.4, 0.4, spoiled(0.0)), (2, 0.4, 0.4, spoiled(-0.5)),
                 (2, 0.4, 0.4, spoiled(1.5)), (2, 0.4, 0.4, spoiled(float("nan"))), (2, 0.4, 0.4, spoiled(float("inf"), 95)),
                 (1, 0.0, 0.0, spoiled(0.5)), (1, 0.0, 0.0, ones[:-1])):
        assert set_wt(plan, *args) == _lib.EINVAL, args
        assert names == [plan.kernel_name(p) for p in range(2)]
    assert before == bits(plan.run(dA, dB))
    # combinations, both ways round
    assert lib.tpiv_plan_set_uncertainty(plan._h, 1, 3) == _lib.OK
    assert set_wt(plan, 2, 0.4, 0.4, good) == _lib.EINVAL and b"uncertainty" in lib.tpiv_last_error()
    assert lib.tpiv_plan_set_uncertainty(plan._h, 0, 3) == _lib.OK
    assert lib.tpiv_plan_set_ensemble(plan._h, 1) == _lib.OK
    assert set_wt(plan, 2, 0.4, 0.4, good) == _lib.EINVAL and b"ensemble" in lib.tpiv_last_error()
    assert lib.tpiv_plan_set_ensemble(plan._h, 0) == _lib.OK
    ctab = eng.correlation_tables(eng.correlation_arg("rpc"), [32, 16])
    assert lib.tpiv_plan_set_correlation(plan._h, 2, 2.8, 2.8, 2.0 ** -10, ctab.ctypes.data, ctab.size) == _lib.OK
    assert set_wt(plan, 2, 0.4, 0.4, good) == _lib.EINVAL and b"correlation" in lib.tpiv_last_error()
    assert lib.tpiv_plan_set_correlation(plan._h, 0, 0.0, 0.0, 0.0, None, 0) == _lib.OK
    assert names == [plan.kernel_name(p) for p in range(2)]
    assert before == bits(plan.run(dA, dB))
    assert set_wt(plan, 2, 0.4, 0.4, good) == _lib.OK
    on = bits(plan.run(dA, dB))
    assert on != before
    assert lib.tpiv_plan_set_uncertainty(plan._h, 1, 3) == _lib.EINVAL and b"weighting" in lib.tpiv_last_error()
    assert lib.tpiv_plan_set_ensemble(plan._h, 1) == _lib.EINVAL and b"weighting" in lib.tpiv_last_error()
    assert lib.tpiv_plan_set_correlation(plan._h, 2, 2.8, 2.8, 2.0 ** -10, ctab.ctypes.data, ctab.size) == _lib.EINVAL
    assert b"weighting" in lib.tpiv_last_error()
    assert set_wt(plan, 2, 9.0, 0.4, good) == _lib.EINVAL              # a failed call leaves the weight as it was
    assert set_wt(plan, 2, 0.4, 0.4, spoiled(0.0)) == _lib.EINVAL
    assert on == bits(plan.run(dA, dB))
    assert all("xcorr_win_kernel" in plan.kernel_name(p) for p in range(2))
    # deform= combines, in this order too
    assert lib.tpiv_plan_set_deform(plan._h, 1, _lib.DEWARP_LINEAR, 1, None) == _lib.OK
    assert bits(plan.run(dA, dB)) != on
    assert lib.tpiv_plan_set_deform(plan._h, 0, 0, 1, None) == _lib.OK
    assert set_wt(plan, 1, 0.0, 0.0, ones) == _lib.OK                  # "uniform"
    assert bits(plan.run(dA, dB)) != on
    assert set_wt(plan, 0, 0.0, 0.0, None) == _lib.OK
    assert before == bits(plan.run(dA, dB))
    plan.close()
    # window sizes: the message names the size
    for ws, n_pass, bad in ((8, 1, 8), (128, 1, 128), (48, 1, 48), (32, 3, 8)):
        pl = eng.Plan(256, 256, ws, ws // 2, n_pass=n_pass, mode="CWS", max_batch=1)
        sizes = [g[0] for g in pl.geometry]
        tab = np.ones(sum(2 * w for w in sizes), np.float32)
        assert set_wt(pl, 1, 0.0, 0.0, tab) == _lib.EUNSUPPORTED
        assert str(bad).encode() in lib.tpiv_last_error()
        pl.close()
    # the one-pass entry: sizes and CWS_Fast
    z = dev(np.zeros((1, 256, 256), np.uint8))
    for ws in (8, 48, 128):
        with pytest.raises(NotImplementedError, match=str(ws)):
            eng.debug_pass(0, z, z, ws, ws // 2, weighting="gaussian")
    nr, nc = eng.field_shape(256, 256, 32, 16)
    f = dev(np.zeros((1, nr, nc)))
    with pytest.raises(NotImplementedError, match="CWS_Fast"):
        eng.debug_pass("CWS_Fast", z, z, 32, 16, u2=f, v2=f, weighting="gaussian")
    tab = dev(np.ones(64, np.float32))
    work = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    for mode, ws, want in ((_lib.MODE_CWS_FAST, 32, _lib.EUNSUPPORTED), (0, 8, _lib.EUNSUPPORTED), (0, 48, _lib.EUNSUPPORTED),
                           (0, 128, _lib.EUNSUPPORTED)):
        rc = lib.tpiv_debug_pass_weighted(mode, tab.data_ptr(), z.data_ptr(), z.data_ptr(), 1, 256, 256, ws, ws // 2,
                                          f.data_ptr(), f.data_ptr(), f.data_ptr(), None, None, None, None, None,
                                          work.data_ptr(), work.numel(), None)
        assert rc == want, (mode, ws, rc)
    # the host classes refuse ensemble() with the keyword
    import torchpiv_amd.backend as T
    res = T.ResidentPIV(dA, dB, 32, 16, multipass=2, weighting="gaussian")
    with pytest.raises(ValueError, match="weighting"):
        res.ensemble()
    res.close()


# ---- precision has no effect ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_precision_has_no_effect(eng):
    A, B = deform4()
    dA, dB = dev(A[:2]), dev(B[:2])
    got = []
    for prec in ("fast", "f64", "exact", "reference"):
        plan = eng.Plan(HC, HC, 64, 32, n_pass=2, mode="CWS", max_batch=2, precision=prec, weighting="gaussian")
        got.append(bits(plan.run(dA, dB)))
        plan.close()
    assert all(g == got[0] for g in got)
    # the workspace too: one-pass plans with few windows, whose float64 records alone are smaller than the float32 layout,
    # with the rounds of deform= behind them (set in either order)
    for ws in (64, 32, 16):
        h = 2 * ws if ws < 64 else HC
        fa, fb = dev(A[:1, :h, :h]), dev(B[:1, :h, :h])
        got = []
        for prec in ("fast", "f64", "exact", "reference"):
            plan = eng.Plan(h, h, ws, ws // 2, n_pass=1, max_batch=1, precision=prec, weighting="gaussian", deform=1)
            got.append(bits(plan.run(fa, fb)))
            plan.close()
        assert all(g == got[0] for g in got), ws
    # the exact scheme's read-outs behave as after a filtered run
    plan = eng.Plan(HC, HC, 64, 32, n_pass=2, mode="CWS", max_batch=2, weighting="gaussian")
    plan.run(dA, dB)
    with pytest.raises(ValueError):
        plan.exact_fallbacks()
    plan.set_weighting(None)
    plan.run(dA, dB)
    assert plan.exact_fallbacks() >= 0
    plan.close()
