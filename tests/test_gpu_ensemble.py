"""Ensemble (sum-of-correlation) PIV on the device against the float64 model of tests/ensemble_model.py: the accumulating
instances of the tile kernel (xcorr_ens.hip) cell by cell, the peak launch, the plan chain with its shared predictor and
settle step, and the host classes.

Maps.  acc against S - P (the model's float64 sum minus the pedestals: the device transforms mean-free windows), per cell,
inside  sum_i Gamma(ws) u S_i  +  (n - 1) u sum_i |C_i|:  the per-map float32 bound of tests/test_gpu_shifted_maps.py
(gamma_u, scales: DESIGN.md 3.4b) summed over the pairs, and the standard bound of a recursive float32 sum of n terms
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 4.4 to first order: whatever the grouping of the
adds -- one call, several calls, pair by pair -- at most n - 1 roundings of partial sums that never exceed sum |C_i|).
Fields.  |du|, |dv| <= 1e-3 px (BASELINE.json's gate for float32 passes), identical validity, no window excused; that the
inputs leave every discrete decision (arg-max, peak ratio, the fit's denominator) outside the map bound is checked on the
model first (expected_fields of tests/test_gpu_shifted_maps.py with the bound as its band).

Measured on one MI355X (profiles/ensemble/measurements.json has the full record): maps at most 0.016 of the bound (pass 1;
0.009 shifted passes), fields at most 3.0e-7 px from the model with identical masks, one pair against the ordinary passes
at most 4.0e-7 px; the chains 6.9e-6 px from the model's; RMS against the constructed flow 0.049 px (ensemble) against
0.167 px (mean of per-pair fields) at 64/32 -> 32/16 CWS, 0.063 against 0.72 at 32/16 -> 16/8 CWS, 0.163 against 0.53 DWS.
TPIV_ENSEMBLE_REPORT=<file>: the figures are appended there as JSON lines.
"""
import functools
import inspect
import json
import os

import numpy as np
import pytest
import torch

from oracle import piv_oracle as O
import ensemble_model as EM
from test_exact_scheme import gamma_u
from test_gpu_shifted_maps import expected_fields, scales

U32 = 2.0 ** -24
GATE = 1e-3
MODES = (0, "DWS", "CWS")
MODE_ID = {0: 0, "DWS": 1, "CWS": 2}                 # test_gpu_shifted_maps' PASS1 / DWS / CWS
CHUNKINGS = ((5,), (3, 2), (1, 1, 1, 1, 1))
REPORT = os.environ.get("TPIV_ENSEMBLE_REPORT")      # optional: a JSON-lines file the measured figures are appended to


def report(**kw):
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(json.dumps(kw) + "\n")


def mode_name(m):
    return m or "PASS1"


# ---- cases 1, 2, 4: inputs ------------------------------------------------------------------------------------------
def geometry(ws, ov, grid):
    """Frame shape for a 3 x 4 grid plus a remainder of 5 pixels, or for one window (plus 3 / 5 pixels)."""
    st = ws - ov
    if grid == "1x1":
        return ws + min(3, st - 1), ws + min(5, st - 1)
    return ws + 2 * st + 5, ws + 3 * st + 5


def half_shifts(mode, ws, nr, nc):
    """The planted half shift [nr, nc] x 2: fractional, integral in one coordinate (CWS: the nearest-sample quirk), zero,
    and at the corner windows outward shifts that push their samples past the frame (the flat-index clamp: the bottom and
    right corners clear the 5-pixel remainder).  DWS: the same rounded (tpiv_ensemble_add takes integral values there)."""
    pat = [(1.375, -0.625), (2.0, 0.4375), (0.0, 0.0), (-0.8125, 1.0), (0.5625, 0.3125), (-1.0, -2.0)]
    u2, v2 = np.zeros((nr, nc)), np.zeros((nr, nc))
    for k in range(nr * nc):
        u2.flat[k], v2.flat[k] = pat[k % len(pat)]
    # frame a is read at x - u2, frame b at x + u2: either sign leaves the frame at a window that touches its edge
    u2[0, 0], v2[0, 0] = -2.375, -1.625
    u2[0, -1], v2[0, -1] = 3.375, -1.375
    u2[-1, 0], v2[-1, 0] = -1.625, 3.625
    u2[-1, -1], v2[-1, -1] = 3.125, 3.375
    if mode == "DWS":
        u2, v2 = np.rint(u2), np.rint(v2)
    return u2, v2


def five_pairs(mode, ws, ov, grid, seed=1):
    """(A, B uint8 [5, H, W], u2, v2): three particle pairs whose displacement is twice the planted half shift of the
    nearest window plus (0.3, -0.2) (so that the staged windows correlate at every planted shift; pass 1: the model's
    flow), one pair of 0 / 255 noise in 2 x 2 grains (b a rolled copy with 5 % redrawn), one pair whose frame a is zero.
    (seed 1: with seed 0 one 16 x 16 window of the DWS case without overlap has its peak ratio inside the map bound of 1.2 --
    found on the model, before any device run; seeds 1 .. 5 leave every decision of every case outside it.)"""
    H, W = geometry(ws, ov, grid)
    nr, nc = (int(x) for x in O.field_shape((H, W), ws, ov))
    st = ws - ov
    u2, v2 = (None, None) if mode == 0 else half_shifts(mode, ws, nr, nc)

    def flow_fn(x, y):
        r = np.clip(np.rint((y - (ws - 1) / 2.0) / st), 0, nr - 1).astype(int)
        c = np.clip(np.rint((x - (ws - 1) / 2.0) / st), 0, nc - 1).astype(int)
        return 2 * u2[r, c] + 0.3, 2 * v2[r, c] - 0.2
    dens = {16: 0.06, 32: 0.03, 64: 0.015}[ws]
    pairs = [EM.scene(100 * ws + 10 * seed + i, H, W, density=dens, flow_fn=None if mode == 0 else flow_fn) for i in range(3)]
    rng = np.random.default_rng(7 * ws + ov + seed)
    ra = np.repeat(np.repeat(rng.integers(0, 2, ((H + 1) // 2, (W + 1) // 2)) * 255, 2, axis=0), 2, axis=1)[:H, :W].astype(np.uint8)
    rb = np.roll(ra, (-1, 2), axis=(0, 1))
    rb = np.where(rng.random((H, W)) < 0.05, rng.integers(0, 2, (H, W)) * 255, rb).astype(np.uint8)
    pairs.append((ra, rb))
    pairs.append((np.zeros((H, W), np.uint8), pairs[1][1].copy()))
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), u2, v2


def raw_windows(mode, a, b, ws, ov, u2, v2):
    """The windows scales() takes: pass 1 the raw ones (it normalises itself), shifted passes the staged ones."""
    if mode == 0:
        return O.windows(a, ws, ov).astype(np.float64), O.windows(b, ws, ov).astype(np.float64)
    wa, wb, _ = EM.staged(mode, a, b, ws, ov, u2, v2)
    return wa, wb


def model_case(mode, A, B, ws, ov, u2, v2):
    """The model's side of a case: want = S - P [N, ws, ws], the cell bound [N, ws, ws], the window bound [N]."""
    S, P, Sabs = EM.summed(mode, A, B, ws, ov, u2, v2)
    gam = gamma_u(ws, "radix2") * U32
    per_map = np.zeros(len(S))
    for a, b in zip(A, B):
        wa, wb = raw_windows(mode, a, b, ws, ov, u2, v2)
        s, _ = scales(wa, wb, MODE_ID[mode])
        per_map += gam * np.nan_to_num(s)
    bound = per_map[:, None, None] + (len(A) - 1) * U32 * Sabs
    return S - P[:, None, None], bound, per_map


def model_fields(mode, want, n, nr, nc, band, u2, v2):
    """(u, v, invalid) of the model and the windows where a discrete decision lies inside the band (none may)."""
    M = want / float(n)
    M = M - M.min(axis=(1, 2), keepdims=True)
    du, dv, inv, bu, bv, near = expected_fields(M, band / float(n))
    du, dv, inv = du.reshape(nr, nc), dv.reshape(nr, nc), inv.reshape(nr, nc)
    close = near["argmax"] | near["ratio"] | near["fit"]
    if mode == 0:
        return du, dv, inv, close
    u0, v0 = 2 * u2, 2 * v2                        # the planted predictor: exercises the fallback rule of the combine
    u, v = EM.combine(du, dv, inv, u0, v0, u2, v2)
    return u, v, inv, close


CASES = [(m, ws, ov, "3x4") for m in MODES for ws in (16, 32, 64) for ov in (ws // 2, 0)] + \
        [(m, ws, ws // 2, "1x1") for m in MODES for ws in (16, 32, 64)]


def case_id(c):
    return f"{mode_name(c[0])}-{c[1]}-{c[2]}-{c[3]}"


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


def add_chunks(eng, mode, A, B, ws, ov, chunks, u2=None, v2=None):
    acc, i = None, 0
    for n in chunks:
        acc = eng.ensemble_add(mode, A[i:i + n], B[i:i + n], ws, ov, acc=acc, u2=u2, v2=v2)
        i += n
    return acc


@functools.lru_cache(maxsize=None)
def run_case(case):
    """Device and model results of a case, computed once and shared by the tests below (read-only)."""
    from torchpiv_amd import engine as eng
    mode, ws, ov, grid = case
    A, B, u2, v2 = five_pairs(mode, ws, ov, grid)
    H, W = A.shape[1:]
    nr, nc = (int(x) for x in O.field_shape((H, W), ws, ov))
    want, bound, per_map = model_case(mode, A, B, ws, ov, u2, v2)
    dA, dB = dev(A), dev(B)
    t2 = (None, None) if mode == 0 else (dev(u2), dev(v2))
    out = {"want": want, "bound": bound, "shape": (H, W, nr, nc), "u2": u2, "v2": v2, "acc": {}, "fields": {}}
    for chunks in CHUNKINGS:
        for rep in range(2):
            acc = add_chunks(eng, mode, dA, dB, ws, ov, chunks, *t2)
            pred = {} if mode == 0 else dict(u0=2 * t2[0], v0=2 * t2[1], u2=t2[0], v2=t2[1])
            f = eng.ensemble_peaks(mode, acc, 5, H, W, ws, ov, **pred)
            out["acc"][chunks, rep] = acc.cpu().numpy()
            out["fields"][chunks, rep] = tuple(t[0].cpu().numpy() for t in f)
    out["model_fields"] = model_fields(mode, want, 5, nr, nc, bound.max(axis=(1, 2)), u2, v2)
    return out


# ---- case 1 -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_maps(eng, case):
    """acc of five pairs, added as (5), (3, 2) and (1, 1, 1, 1, 1), against the model's float64 sum, cell by cell."""
    r = run_case(case)
    worst = 0.0
    for chunks in CHUNKINGS:
        got = r["acc"][chunks, 0].astype(np.float64)
        assert np.isfinite(got).all()
        err = np.abs(got - r["want"])
        zero = r["bound"] == 0
        assert not err[zero].any(), (case_id(case), chunks, "a zero map must stay zero")
        q = (err[~zero] / r["bound"][~zero]).max() if (~zero).any() else 0.0
        worst = max(worst, float(q))
    print(f"  {case_id(case):20s} worst |acc - model| / bound {worst:.3f}")
    report(section="maps", case=case_id(case), worst_ratio=worst)
    assert worst < 1, (case_id(case), worst)


# ---- case 2 -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fields(eng, case):
    """ensemble_peaks on those accumulators against corr_to_disp (and the combine) on the model's mean map."""
    r = run_case(case)
    mu, mv, minv, close = r["model_fields"]
    assert not close.any(), (case_id(case), "the inputs leave a decision inside the map bound", np.flatnonzero(close))
    worst = 0.0
    for chunks in CHUNKINGS:
        u, v, inv = r["fields"][chunks, 0]
        assert np.array_equal(inv.astype(bool), minv), (case_id(case), chunks)
        worst = max(worst, float(np.abs(u - mu).max()), float(np.abs(v - mv).max()))
    print(f"  {case_id(case):20s} worst |field - model| {worst:.2e} px, {int(minv.sum())} of {minv.size} invalid")
    report(section="fields", case=case_id(case), worst_px=worst)
    assert worst <= GATE, (case_id(case), worst)


# ---- case 4 -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c[3] == "3x4" and c[2] != 0], ids=case_id)
def test_same_calls_same_bits(eng, case):
    r = run_case(case)
    for chunks in CHUNKINGS:
        assert np.array_equal(r["acc"][chunks, 0].view(np.uint32), r["acc"][chunks, 1].view(np.uint32)), (case_id(case), chunks)
        for x, y in zip(r["fields"][chunks, 0], r["fields"][chunks, 1]):
            assert x.tobytes() == y.tobytes(), (case_id(case), chunks)


# ---- case 3 -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ws", [16, 32, 64])
def test_one_pair_is_the_ordinary_pass(eng, ws):
    """n = 1: the ensemble field of one pair against engine.pass1(precision="fast") and engine.iterate of that pair."""
    H = W = 3 * ws + ws // 2 + 5
    ov = ws // 2
    a, b = EM.scene(5, H, W, density={16: 0.06, 32: 0.03, 64: 0.015}[ws])
    da, db = dev(a)[None], dev(b)[None]
    u, v, inv = eng.ensemble_peaks(0, eng.ensemble_add(0, da, db, ws, ov), 1, H, W, ws, ov)
    pu, pv, pinv = eng.pass1(da, db, ws, ov, precision="fast")
    assert torch.equal(inv, pinv)
    d1 = max(float((u - pu).abs().max()), float((v - pv).abs().max()))
    assert d1 <= GATE, d1
    worst = d1
    nr, nc = eng.field_shape(H, W, ws, ov)
    for mode in ("DWS", "CWS"):
        u2, v2 = half_shifts(mode, ws, nr, nc)
        u2, v2 = 0.5 * u2, 0.5 * v2                      # (moderate: the pair's displacement is the scene's, not the plant's)
        if mode == "DWS":
            u2, v2 = np.rint(u2), np.rint(v2)
        t = [dev(x)[None] for x in (2 * u2, 2 * v2, u2, v2)]
        acc = eng.ensemble_add(mode, da, db, ws, ov, u2=t[2], v2=t[3])
        eu, ev, einv = eng.ensemble_peaks(mode, acc, 1, H, W, ws, ov, *t)
        iu, iv, iinv = eng.iterate(mode, da, db, ws, ov, *t, precision="fast")
        assert torch.equal(einv, iinv), mode
        d = max(float((eu - iu).abs().max()), float((ev - iv).abs().max()))
        assert d <= GATE, (mode, d)
        worst = max(worst, d)
    print(f"  ws {ws}: ensemble of one pair against the ordinary passes, worst {worst:.2e} px")
    report(section="one_pair", ws=ws, worst_px=worst)


# ---- case 5 -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ws", [16, 32, 64])
def test_zero_windows(eng, ws):
    """A block of zeros in every frame (a window with no contribution at all: constant mean map, invalid, u = v = 0) and
    in one frame only (that pair's contribution skipped): maps and fields equal the model, no NaN."""
    ov, n = ws // 2, 3
    H = W = ws + 4 * (ws - ov) + 3
    A, B = EM.recording(n, H, W, density={16: 0.06, 32: 0.03, 64: 0.015}[ws])
    A, B = A.copy(), B.copy()
    A[:, :ws, :ws] = 0                                  # window (0, 0) of every pair, frame a
    B[1, 2 * (ws - ov):2 * (ws - ov) + ws, 2 * (ws - ov):2 * (ws - ov) + ws] = 0        # window (2, 2) of pair 1, frame b
    nr, nc = (int(x) for x in O.field_shape((H, W), ws, ov))
    want, bound, _ = model_case(0, A, B, ws, ov, None, None)
    acc = eng.ensemble_add(0, dev(A), dev(B), ws, ov)
    got = acc.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    assert not got[0].any()                             # nothing was added: exactly the zero map
    skipped, _, _ = model_case(0, A[[0, 2]], B[[0, 2]], ws, ov, None, None)
    k = 2 * nc + 2
    assert np.abs(got[k] - skipped[k]).max() <= bound[k].max()
    zero = bound == 0
    assert not np.abs(got - want)[zero].any()
    assert (np.abs(got - want)[~zero] / bound[~zero]).max() < 1
    u, v, inv = (t[0].cpu().numpy() for t in eng.ensemble_peaks(0, acc, n, H, W, ws, ov))
    mu, mv, minv = EM.peaks(want, n, nr, nc)
    assert minv[0, 0] and inv[0, 0] == 1 and u[0, 0] == 0 and v[0, 0] == 0
    assert np.array_equal(inv.astype(bool), minv)
    live = np.ones_like(minv)
    live[0, 0] = False
    assert max(np.abs(u - mu)[live].max(), np.abs(v - mv)[live].max()) <= GATE


# ---- case 6 -------------------------------------------------------------------------------------------------------
N_REC, HREC = 32, 160


@functools.lru_cache(maxsize=None)
def recording32():
    return EM.recording(N_REC, HREC, HREC)


def chunks_of(dA, dB, bs):
    return lambda: ((dA[i:i + bs], dB[i:i + bs]) for i in range(0, dA.shape[0], bs))


def unrolled_chain(eng, plan, dA, dB, mode, bs, settle=None):
    """The plan's ensemble chain from the function seam: ensemble_add, ensemble_peaks, Plan.debug_predict; settle(p, u, v,
    inv) -> (u, v, inv) stands for the plan's settle step.  Returns [(u, v, inv)] per pass."""
    out, H, W = [], plan.H, plan.W
    n = dA.shape[0]
    for p, (ws, ov, nr, nc) in enumerate(plan.geometry):
        m = 0 if p == 0 else mode
        pred = {}
        if p:
            u0, v0, u2, v2 = plan.debug_predict(p, *out[-1])
            pred = dict(u0=u0, v0=v0, u2=u2, v2=v2)
        acc = None
        for a, b in chunks_of(dA, dB, bs)():
            acc = eng.ensemble_add(m, a, b, ws, ov, acc=acc, u2=pred.get("u2"), v2=pred.get("v2"))
        u, v, inv = eng.ensemble_peaks(m, acc, n, H, W, ws, ov, **pred)
        if settle is not None:
            u, v, inv = settle(p, u, v, inv)
        out.append((u, v, inv))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("ws,mode", [(32, "CWS"), (32, "DWS"), (64, "CWS")], ids=lambda x: str(x))
def test_plan_chain(eng, ws, mode):
    """Two ensemble passes on the sparse scene (32 pairs, four add calls per pass): Plan.run_ensemble is bit-identical to
    the unrolled chain of seam functions and within the gate of the model's chain with the same validity; and the benefit:
    against the constructed flow the ensemble field is at least twice as close as the mean of the valid per-pair fields of
    the same plan's run()."""
    A, B = recording32()
    dA, dB = dev(A), dev(B)
    ov, bs = ws // 2, 8
    plan = eng.Plan(HREC, HREC, ws, ov, n_pass=2, mode=mode, max_batch=bs, ensemble=True)
    u, v, inv = plan.run_ensemble(chunks_of(dA, dB, bs))
    maps, n_added = plan.ensemble_maps()
    assert n_added == 0 or n_added == N_REC
    steps = unrolled_chain(eng, plan, dA, dB, mode, bs)
    for got, want in zip((u, v, inv), steps[-1]):
        assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    model = EM.chain(A, B, ws, ov, 2, mode)
    worst = 0.0
    for p, ((gu, gv, ginv), (mu, mv, minv)) in enumerate(zip(steps, model)):
        gu, gv, ginv = gu[0].cpu().numpy(), gv[0].cpu().numpy(), ginv[0].cpu().numpy().astype(bool)
        assert np.array_equal(ginv, minv), (p, int((ginv != minv).sum()))
        worst = max(worst, float(np.abs(gu - mu).max()), float(np.abs(gv - mv).max()))
    assert worst <= GATE, worst
    # ---- benefit, at the last pass's grid
    wl, ol, nr, nc = plan.geometry[-1]
    tu, tv = EM.truth(HREC, HREC, wl, ol)
    su, sv, cnt = np.zeros((nr, nc)), np.zeros((nr, nc)), np.zeros((nr, nc))
    for a, b in chunks_of(dA, dB, bs)():
        pu, pv, pinv = (t.cpu().numpy() for t in plan.run(a, b))
        ok = pinv == 0
        su += np.where(ok, pu, 0.0).sum(axis=0)
        sv += np.where(ok, pv, 0.0).sum(axis=0)
        cnt += ok.sum(axis=0)
    has = cnt > 0
    avg = EM.rms((su / np.maximum(cnt, 1)), (sv / np.maximum(cnt, 1)), tu, tv, has)
    eu, ev, einv = u[0].cpu().numpy(), v[0].cpu().numpy(), inv[0].cpu().numpy().astype(bool)
    ens = EM.rms(eu, ev, tu, tv, has & ~einv)
    print(f"  {ws}/{ov} -> {wl}/{ol} {mode}: chain against the model {worst:.2e} px; RMS against the flow: ensemble {ens:.3f} px "
          f"({einv.mean():.1%} invalid), mean of valid per-pair fields {avg:.3f} px ({1 - cnt.sum() / (N_REC * nr * nc):.1%} "
          f"of the single-pair vectors invalid)")
    report(section="d_accuracy", chain=f"{ws}/{ov}->{wl}/{ol} {mode}", ensemble_rms_px=ens, mean_of_fields_rms_px=avg,
           chain_vs_model_px=worst)
    assert ens <= 0.5 * avg, (ens, avg)
    plan.close()


# ---- case 7 -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_settle_acts_on_ensemble_fields(eng):
    """mask= over a corner and outlier="median": excluded cells are zero and invalid to the predictor, and a planted wrong
    vector (a bright dot pattern that every pair repeats in one window, displaced against the flow) is flagged and replaced
    before the next predictor -- all bit-identical to the unrolled functions (mask_fields, median_test)."""
    A, B = recording32()
    A, B = A.copy(), B.copy()
    rng = np.random.default_rng(3)
    y0, x0 = 64, 96                                         # window (2, 3) of the 32/0 grid: windows that do not overlap,
    for _ in range(10):                                     # so that the pattern (both exposures) lies in this one alone
        py, px = int(rng.integers(y0 + 2, y0 + 20)), int(rng.integers(x0 + 10, x0 + 28))
        A[:, py:py + 2, px:px + 2] = 255
        B[:, py + 6:py + 8, px - 7:px - 5] = 255            # displaced by (-7, +6): against the flow (2.3, -1.4)
    img = np.zeros((HREC, HREC), np.uint8)
    img[:40, :40] = 1
    dA, dB = dev(A), dev(B)
    bs, mode = 8, "CWS"
    plan = eng.Plan(HREC, HREC, 32, 0, n_pass=2, mode=mode, max_batch=bs, ensemble=True, mask={"image": img, "pixels": "keep"},
                    outlier="median")
    grids = [plan.mask_grid(p) for p in range(2)]
    assert grids[0][0, 0] and grids[1][:2, :2].all()
    passes = []
    for p in range(2):
        plan.ensemble_begin(p)
        for a, b in chunks_of(dA, dB, bs)():
            plan.ensemble_add(a, b)
        passes.append(tuple(t.clone() for t in plan.ensemble_end()))
    flags = {}

    def settle(p, u, v, inv):
        last = p == 1
        eng.mask_fields(u, v, inv, grids[p], 1)
        status, mu, mv = eng.median_test(u, v, inv, want_medians=True)
        flag = (status & 1) != 0
        flags[p] = flag[0].cpu().numpy()
        if last:
            inv = inv | flag.to(torch.uint8)
        else:
            u, v = torch.where(flag, mu, u), torch.where(flag, mv, v)
        eng.mask_fields(u, v, inv, grids[p], 0 if last else 1)
        return u.contiguous(), v.contiguous(), inv.contiguous()
    steps = unrolled_chain(eng, plan, dA, dB, mode, bs, settle=settle)
    for p in range(2):
        for got, want in zip(passes[p], steps[p]):
            assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), p
    u0, v0, inv0 = (t[0].cpu().numpy() for t in passes[0])
    g0 = grids[0].cpu().numpy()
    assert not u0[g0].any() and not v0[g0].any() and (inv0[g0] == 1).all()
    assert flags[0][2, 3], "the planted vector was not flagged"
    tu, tv = EM.truth(HREC, HREC, 32, 0)
    assert abs(u0[2, 3] - tu[2, 3]) < 1.0 and abs(v0[2, 3] - tv[2, 3]) < 1.0       # replaced by the neighbourhood median
    uL, vL, invL = (t[0].cpu().numpy() for t in passes[1])
    g1 = grids[1].cpu().numpy()
    assert not uL[g1].any() and (invL[g1] == 0).all()
    plan.close()


# ---- case 8 -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_off_means_off(eng):
    """A plan with ensemble on runs run() exactly as a plan without."""
    A, B = recording32()
    dA, dB = dev(A[:4]), dev(B[:4])
    kw = {"ensemble": True} if "ensemble" in inspect.signature(eng.Plan.__init__).parameters else {}
    for mode in ("CWS", "DWS"):
        p1 = eng.Plan(HREC, HREC, 32, 16, n_pass=2, mode=mode, max_batch=4, **kw)
        p0 = eng.Plan(HREC, HREC, 32, 16, n_pass=2, mode=mode, max_batch=4)
        r1, r0 = p1.run(dA, dB), p0.run(dA, dB)
        for x, y in zip(r1, r0):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), mode
        p1.close()
        p0.close()


# ---- case 9 -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(eng):
    A, B = recording32()
    dA, dB = dev(A[:8]), dev(B[:8])
    for ws, n_pass in ((8, 1), (128, 1), (24, 1), (32, 3)):
        with pytest.raises(NotImplementedError):
            eng.Plan(256, 256, ws, ws // 2, n_pass=n_pass, ensemble=True)
    for ws in (8, 24, 128):
        with pytest.raises(NotImplementedError, match=str(ws)):
            eng.ensemble_add(0, dev(np.zeros((1, 256, 256), np.uint8)), dev(np.zeros((1, 256, 256), np.uint8)), ws, ws // 2)
    with pytest.raises(ValueError):
        eng.Plan(HREC, HREC, 32, 16, ensemble=True, uncertainty="cs")
    with pytest.raises(ValueError):
        eng.Plan(HREC, HREC, 32, 16, ensemble=True, deform=1)
    off = eng.Plan(HREC, HREC, 32, 16, max_batch=4)
    with pytest.raises(ValueError):
        off.ensemble_begin(0)
    with pytest.raises(ValueError):
        off.run_ensemble(chunks_of(dA, dB, 4))
    off.close()
    plan = eng.Plan(HREC, HREC, 32, 16, n_pass=2, mode="CWS", max_batch=4, ensemble=True)
    with pytest.raises(ValueError):
        plan.ensemble_add(dA[:4], dB[:4])                   # before begin
    with pytest.raises(ValueError):
        plan.ensemble_end()                                 # before begin
    with pytest.raises(ValueError):
        plan.ensemble_begin(1)                              # pass 0 has not been ended
    plan.ensemble_begin(0)
    with pytest.raises(ValueError):
        plan.ensemble_end()                                 # nothing added
    with pytest.raises(ValueError):
        plan.ensemble_add(dA[:8], dB[:8])                   # above max_batch
    with pytest.raises(ValueError):
        plan.ensemble_add(dA[:4, :100], dB[:4, :100])       # wrong frame shape
    with pytest.raises((ValueError, RuntimeError)):
        plan.ensemble_add(torch.from_numpy(A[:4]), torch.from_numpy(B[:4]))              # wrong device: host tensors
    with pytest.raises(ValueError):
        plan.ensemble_begin(1)                              # still: pass 0 is open, not ended
    # the plan is usable afterwards: the whole chain, equal to a fresh plan's
    got = plan.run_ensemble(chunks_of(dA, dB, 4))
    fresh = eng.Plan(HREC, HREC, 32, 16, n_pass=2, mode="CWS", max_batch=4, ensemble=True)
    want = fresh.run_ensemble(chunks_of(dA, dB, 4))
    for x, y in zip(got, want):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    plan.close()
    fresh.close()


# ---- case 10 ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_host_classes(eng, tmp_path):
    """ResidentPIV.ensemble() and OfflinePIV.ensemble() over BMP files: identical bits, equal to Plan.run_ensemble + the
    finish on the prepared frames; again with background="min" and an indices subset; a second call returns the same."""
    from PIL import Image
    import torchpiv_amd.backend as T
    A, B = recording32()
    n = 12
    A, B = A[:n].copy(), B[:n].copy()
    A[:, 100:120, 30:60] = np.maximum(A[:, 100:120, 30:60], 40)      # a static glare: what background="min" removes
    B[:, 100:120, 30:60] = np.maximum(B[:, 100:120, 30:60], 40)
    for i in range(n):
        Image.fromarray(A[i], "L").save(tmp_path / f"image{i:02d}_a.bmp")
        Image.fromarray(B[i], "L").save(tmp_path / f"image{i:02d}_b.bmp")
    dA, dB = dev(A), dev(B)
    base = dict(multipass=2, multipass_mode="CWS", dt=2, scale=0.5)
    for kw, indices in (({}, None), ({"background": "min"}, [1, 2, 3, 5, 8, 9, 10, 11])):
        res = T.ResidentPIV(dA, dB, 32, 16, **base, **kw)
        off = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", 32, 16, **base, **kw)
        r1 = res.ensemble(indices=indices, batch_size=4)
        o1 = off.ensemble(indices=indices, batch_size=4)
        r2 = res.ensemble(indices=indices, batch_size=4)
        assert r1 is not None and o1 is not None
        for x, y, z in zip(r1, o1, r2):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes() == np.asarray(z).tobytes(), kw
        # the same from the plan: prepared frames (the model of the chain: frame minus the minimum over the chosen pairs'
        # frames is NOT what "min" means -- it is the minimum over the whole recording), run_ensemble, finish
        idx = list(range(n)) if indices is None else indices
        fa, fb = dA, dB
        if kw:
            fa = eng.subtract_background(dA, eng.frame_min(dA))
            fb = eng.subtract_background(dB, eng.frame_min(dB))
        sel = torch.tensor(idx, device="cuda")
        fa, fb = fa.index_select(0, sel), fb.index_select(0, sel)
        plan = eng.Plan(HREC, HREC, 32, 16, n_pass=2, mode="CWS", max_batch=4, ensemble=True)
        u, v, inv = plan.run_ensemble(chunks_of(fa, fb, 4))
        u, v, inv = u[0].cpu().numpy(), v[0].cpu().numpy(), inv[0].cpu().numpy().astype(bool)
        assert not inv.all()
        if inv.any():
            u, v = T.post_validate(u.copy(), v.copy(), inv)
        x, y = T.get_coordinates((HREC, HREC), 16, 8)
        want = (x * 0.5, y * 0.5, np.flip(u, axis=0) * 0.5 / 2 * 1000, -np.flip(v, axis=0) * 0.5 / 2 * 1000)
        for g, w in zip(r1, want):
            assert np.allclose(np.asarray(g), w, rtol=0, atol=1e-12), kw
        plan.close()
        res.close()
        off.close()
