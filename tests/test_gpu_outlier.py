"""Normalized median test on the device (outlier.hip) and through the plan and the host paths: tpiv_median_test against
the numpy model of tests/outlier_model.py bit for bit, the plan's hook between the passes and after the last one, off
means off, the effect on frames with planted spurious peaks, and outlier="median" through OfflinePIV / ResidentPIV /
run_folder."""
import numpy as np
import pytest
import torch

import outlier_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _field(shape, density, seed, all_invalid=False):
    """A smooth field with noise, planted spikes (single and adjacent), exact ties, -0.0 / +0.0 and a random mask."""
    rng = np.random.default_rng(seed)
    B, R, C = shape
    r, c = np.mgrid[0:R, 0:C]
    u = 2.0 + 0.05 * r + rng.normal(0, 0.05, shape)
    v = -1.0 + 0.03 * c + rng.normal(0, 0.05, shape)
    n = B * R * C
    flat_u, flat_v = u.reshape(-1), v.reshape(-1)
    k = max(1, n // 25)
    at = rng.choice(n, size=min(n, k), replace=False)
    flat_u[at] += rng.choice([-9.0, 7.0, 12.0], size=at.size)
    flat_v[at[: at.size // 2]] -= 8.0
    # runs of equal values (ties among the neighbours, all-equal neighbourhoods) and zeros of both signs
    tie = rng.random(shape) < 0.15
    u[tie] = 2.5
    v[tie] = np.round(v[tie] * 4) / 4
    z = rng.random(shape) < 0.10
    u[z] = np.where(rng.random(int(z.sum())) < 0.5, 0.0, -0.0)
    z2 = rng.random(shape) < 0.10
    v[z2] = np.where(rng.random(int(z2.sum())) < 0.5, 0.0, -0.0)
    inv = np.ones(shape, np.uint8) if all_invalid else (rng.random(shape) < density).astype(np.uint8)
    return u, v, inv


def _check(eng, u, v, inv, **par):
    st, mu, mv = eng.median_test(torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda(), torch.from_numpy(inv).cuda(),
                                 want_medians=True, **par)
    st_only = eng.median_test(torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda(), torch.from_numpy(inv).cuda(), **par)
    torch.cuda.synchronize()
    wst, wmu, wmv = M.median_test(u, v, inv, **par)
    st = st.cpu().numpy()
    assert np.array_equal(st, wst), (np.argwhere(st != wst)[:5], par)
    assert np.array_equal(st_only.cpu().numpy(), wst)                      # the call without medians decides the same
    assert np.array_equal(_bits(mu.cpu().numpy()), _bits(wmu)), np.argwhere(_bits(mu.cpu().numpy()) != _bits(wmu))[:5]
    assert np.array_equal(_bits(mv.cpu().numpy()), _bits(wmv)), np.argwhere(_bits(mv.cpu().numpy()) != _bits(wmv))[:5]
    return wst


# [5, 63, 63] is one cell short of the 64 x 8 tile in the columns, [2, 127, 130] two past a tile edge; [3, 70, 75] is a
# multiple of the tile in neither direction
SHAPES = [(1, 1, 1), (1, 2, 2), (3, 1, 9), (2, 9, 1), (5, 63, 63), (2, 127, 130), (3, 70, 75)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("density", [0.0, 0.1, 0.6, "all"])
def test_median_test_equals_the_model_bit_for_bit(eng, shape, density):
    u, v, inv = _field(shape, 0.0 if density == "all" else density, seed=shape[1] * 131 + shape[2],
                       all_invalid=density == "all")
    st = _check(eng, u, v, inv)
    if density == 0.0 and shape[1] >= 9 and shape[2] >= 9:
        assert (st & 1).any() and not (st & 1).all()                       # the case decides something
    if density == "all":
        assert np.array_equal(st, np.full(shape, 2, np.uint8))


@pytest.mark.parametrize("min_neighbours", range(1, 9))
def test_every_min_neighbours(eng, min_neighbours):
    for density in (0.1, 0.6):
        u, v, inv = _field((2, 33, 70), density, seed=7 + min_neighbours)
        _check(eng, u, v, inv, min_neighbours=min_neighbours)
    # other parameters than the defaults
    u, v, inv = _field((1, 20, 66), 0.2, seed=3)
    _check(eng, u, v, inv, threshold=1.25, eps=0.0, min_neighbours=min_neighbours)


def test_arguments_and_aliasing(eng):
    from torchpiv_amd._lib import check, lib
    u = torch.zeros(2, 8, 8, dtype=torch.float64, device="cuda")
    inv = torch.zeros(2, 8, 8, dtype=torch.uint8, device="cuda")
    st = torch.zeros(2, 8, 8, dtype=torch.uint8, device="cuda")
    for bad in (dict(threshold=0.0), dict(eps=-1.0), dict(min_neighbours=0), dict(min_neighbours=9)):
        with pytest.raises(ValueError):
            eng.median_test(u, u.clone(), inv, **bad)
    with pytest.raises(TypeError):
        eng.median_test(u.float(), u.float(), inv)
    with pytest.raises(ValueError):                                          # the medians would overwrite an input
        check(lib.tpiv_median_test(u.data_ptr(), u.data_ptr(), inv.data_ptr(), 2, 8, 8, 2.0, 0.1, 3, st.data_ptr(),
                                   u.data_ptr(), None, 0))
    with pytest.raises(ValueError):                                          # the status map is the mask
        check(lib.tpiv_median_test(u.data_ptr(), u.data_ptr(), inv.data_ptr(), 2, 8, 8, 2.0, 0.1, 3, inv.data_ptr(),
                                   None, None, 0))
    # a NaN faults nothing
    u[0, 3, 3] = float("nan")
    eng.median_test(u, u.clone(), inv, want_medians=True)
    torch.cuda.synchronize()


def test_two_adjacent_outliers_are_judged_on_the_snapshot(eng):
    """Two neighbouring spikes: each one's median and flag come from the other's ORIGINAL value.  An implementation that
    replaced in place would hand the second cell the first one's median instead of its spike."""
    u = np.full((1, 5, 6), 1.0) + np.arange(6) * 0.01
    v = np.full((1, 5, 6), -2.0)
    u[0, 2, 2], u[0, 2, 3] = 30.0, -40.0
    inv = np.zeros((1, 5, 6), np.uint8)
    st = _check(eng, u, v, inv)
    assert st[0, 2, 2] == 1 and st[0, 2, 3] == 1
    _, mu, _ = M.median_test(u, v, inv)
    # what an in-place pass would have given for the second spike differs from the snapshot's answer
    u_seq = u.copy()
    u_seq[0, 2, 2] = mu[0, 2, 2]
    assert M.median_test(u_seq, v, inv)[1][0, 2, 3] != mu[0, 2, 3]


# ---------------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------------
PH, PW = 256, 320


@pytest.fixture(scope="module")
def pairs():
    from torchpiv_amd import synth
    A, B = synth.make_batch(3, PH, PW, kind="wavy", noise=1.5)
    A, B = A.clone(), B.clone()
    # spurious content: a block of frame b replaced by frame a displaced far from the flow, and a dead block
    B[:, 64:104, 96:136] = torch.roll(A, shifts=(-7, 9), dims=(1, 2))[:, 64:104, 96:136]
    B[1, 160:200, 200:260] = 0
    return A.cuda(), B.cuda()


def _np(*ts):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


@pytest.mark.parametrize("mode,precision", [("CWS", "exact"), ("DWS", "fast")])
def test_plan_pass0_replaces_flagged_vectors_by_their_medians(eng, pairs, mode, precision):
    """Pass 0 of a two-pass plan with the test on, against the model applied to the fields of a one-pass plan of the same
    first-pass geometry with the test off.  (With the test off the two plans' pass-0 fields are bit-identical -- the
    first pass sees nothing of what follows it -- which is asserted first.)"""
    A, B = pairs
    n = A.shape[0]
    one = eng.Plan(PH, PW, 32, 16, n_pass=1, mode=mode, max_batch=n, precision=precision)
    u1, v1, i1 = _np(*one.run(A, B))
    off = eng.Plan(PH, PW, 32, 16, n_pass=2, mode=mode, max_batch=n, precision=precision)
    off.run(A, B)
    uo, vo, io = _np(*off.pass_fields(0, n))
    assert np.array_equal(_bits(uo), _bits(u1)) and np.array_equal(_bits(vo), _bits(v1)) and np.array_equal(io, i1)
    on = eng.Plan(PH, PW, 32, 16, n_pass=2, mode=mode, max_batch=n, precision=precision, outlier="median")
    on.run(A, B)
    up, vp, ip = _np(*on.pass_fields(0, n))
    st, = _np(on.outlier_status(0, n))
    wst, mu, mv = M.median_test(u1, v1, i1)
    assert np.array_equal(st, wst)
    assert (wst & 1).sum() > 0
    wu, wv = M.replaced(u1, v1, wst, mu, mv)
    assert np.array_equal(_bits(up), _bits(wu)) and np.array_equal(_bits(vp), _bits(wv))
    assert np.array_equal(ip, i1)                                          # the mask stays the peak-ratio test's
    assert (_bits(up) != _bits(u1)).any()
    for p in (one, off, on):
        p.close()


@pytest.mark.parametrize("mode,precision,n_pass", [("CWS", "exact", 2), ("DWS", "fast", 2), ("CWS", "exact", 1)])
def test_plan_last_pass_flags_join_the_mask(eng, pairs, mode, precision, n_pass):
    A, B = pairs
    n = A.shape[0]
    on = eng.Plan(PH, PW, 32, 16, n_pass=n_pass, mode=mode, max_batch=n, precision=precision, outlier="median")
    u, v, inv = _np(*on.run(A, B))
    st, = _np(on.outlier_status(n_pass - 1, n))
    peak = st >> 1
    wst, mu, mv = M.median_test(u, v, peak)
    assert np.array_equal(st & 1, wst & 1)
    assert np.array_equal(inv, peak | (st & 1))
    f = (st & 1) != 0
    assert f.sum() > 0
    # the delivered vectors of flagged cells are the pass's own, not the medians
    assert (_bits(u)[f] != _bits(mu)[f]).any() and not np.array_equal(_bits(u)[f], _bits(mu)[f])
    if n_pass == 1:       # the one-pass plan without the test: same u, v, and its mask is the status map's bit 1
        offp = eng.Plan(PH, PW, 32, 16, n_pass=1, mode=mode, max_batch=n, precision=precision)
        u0, v0, i0 = _np(*offp.run(A, B))
        assert np.array_equal(_bits(u0), _bits(u)) and np.array_equal(_bits(v0), _bits(v)) and np.array_equal(i0, peak)
        offp.close()
    on.close()


@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("mode", ["CWS", "DWS"])
def test_plan_without_the_keyword(eng, pairs, mode, precision):
    """A plan that is never told of the test (this function uses nothing the feature adds, so it runs on the commit
    before it as well): its runs repeat bit for bit, a second plan gives the same bits, and its first pass is the
    function-level tpiv_pass1, which the feature does not touch."""
    A, B = pairs
    n = A.shape[0]
    ref = eng.Plan(PH, PW, 32, 16, n_pass=2, mode=mode, max_batch=n, precision=precision)
    want = _np(*ref.run(A, B))
    want0 = _np(*ref.pass_fields(0, n))
    again = _np(*ref.run(A, B))
    other = eng.Plan(PH, PW, 32, 16, n_pass=2, mode=mode, max_batch=n, precision=precision)
    got = _np(*other.run(A, B))
    for g, w in zip(again + got, want + want):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8))
    for g, w in zip(_np(*eng.pass1(A, B, 32, 16, precision=precision)), want0):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8))
    ref.close()
    other.close()


@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("mode", ["CWS", "DWS"])
def test_off_means_off(eng, pairs, mode, precision):
    """outlier=None, kind 0, and a plan switched to kind 0 after having run with the test on give the bits of a plan that
    was never told of the test; outlier_status raises for all of them."""
    from torchpiv_amd._lib import check, lib
    A, B = pairs
    n = A.shape[0]
    ref = eng.Plan(PH, PW, 32, 16, n_pass=2, mode=mode, max_batch=n, precision=precision)
    want = _np(*ref.run(A, B))
    want0 = _np(*ref.pass_fields(0, n))
    with pytest.raises(ValueError):
        ref.outlier_status(0, n)
    none = eng.Plan(PH, PW, 32, 16, n_pass=2, mode=mode, max_batch=n, precision=precision, outlier=None)
    check(lib.tpiv_plan_set_outlier(none._h, 0, 2.0, 0.1, 3))
    sw = eng.Plan(PH, PW, 32, 16, n_pass=2, mode=mode, max_batch=n, precision=precision, outlier="median")
    sw.run(A, B)
    check(lib.tpiv_plan_set_outlier(sw._h, 0, 2.0, 0.1, 3))
    for p in (none, sw):
        got = _np(*p.run(A, B))
        got0 = _np(*p.pass_fields(0, n))
        for g, w in zip(got + got0, want + want0):
            assert np.array_equal(g.view(np.uint8), w.view(np.uint8))
        with pytest.raises(ValueError):
            p.outlier_status(0, n)
        p.close()
    with pytest.raises(ValueError):
        check(lib.tpiv_plan_set_outlier(ref._h, 2, 2.0, 0.1, 3))
    with pytest.raises(ValueError):
        check(lib.tpiv_plan_set_outlier(ref._h, 1, 2.0, 0.1, 0))
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------
# the point of the feature, on frames
# ---------------------------------------------------------------------------------------------------------------------
FH = FW = 256
FLOW = (2.3, -1.6)                       # synth's "uniform" flow (u, v) in px
PLANT = (9, -7)                          # displacement of the planted patches (u, v): 8.6 px from the flow
PATCH = 28                               # patch edge, centred on a 32 px first-pass window
SPOTS = [(3, 4), (7, 10), (11, 5), (5, 11)]     # first-pass windows (row, column) of the 15 x 15 grid, >= 4 windows apart
N_PAIRS = 4
FALSE_FLAG_CAP = 0.01                    # as tests/test_outlier_host.py checks for the model alone
FAR_TOL = 0.2                            # px; see test_planted_spurious_peaks_are_caught_between_the_passes


def planted_frames(plant=True):
    """N_PAIRS pairs of synth's uniform flow; in frame b, around the centre of each window of SPOTS, a PATCH x PATCH block
    is replaced by frame a displaced by PLANT -- the window's correlation then has a sharp peak at PLANT.  plant=False:
    the clean pairs."""
    from torchpiv_amd import synth
    A, B = synth.make_batch(N_PAIRS, FH, FW, kind="uniform", noise=1.0)
    if not plant:
        return A, B
    B = B.clone()
    moved = torch.roll(A, shifts=(PLANT[1], PLANT[0]), dims=(1, 2))        # moved[y, x] = a[y - dv, x - du]
    for r, c in SPOTS:
        y0, x0 = 16 * r + 16 - PATCH // 2, 16 * c + 16 - PATCH // 2        # window r covers rows 16 r ... 16 r + 31
        B[:, y0:y0 + PATCH, x0:x0 + PATCH] = moved[:, y0:y0 + PATCH, x0:x0 + PATCH]
    return A, B


def delivered(u, v, inv):
    """What a caller receives of one pair: valid vectors as they are, invalid ones filled by the reference's
    post-validation (border interpolation, Delaunay fill); the field as it is where nothing is invalid."""
    from torchpiv_amd import backend
    if not inv.any():
        return u, v
    fu, fv = backend.post_validate(u.copy(), v.copy(), inv.astype(bool))
    assert fu is not None, "the pair would be dropped"
    return fu, fv


def frames_figures(eng):
    """Runs the chain 32/16 -> 16/8 CWS "exact" without and with the test; returns the figures test_planted... asserts."""
    A, B = (t.cuda() for t in planted_frames())
    n = A.shape[0]
    fig = {}
    off = eng.Plan(FH, FW, 32, 16, n_pass=2, mode="CWS", max_batch=n, precision="exact")
    uo, vo, io = _np(*off.run(A, B))
    u0, v0, i0 = _np(*off.pass_fields(0, n))
    on = eng.Plan(FH, FW, 32, 16, n_pass=2, mode="CWS", max_batch=n, precision="exact", outlier="median")
    un, vn, inn = _np(*on.run(A, B))
    st0, stl = _np(on.outlier_status(0, n), on.outlier_status(1, n))
    err0 = np.hypot(u0 - FLOW[0], v0 - FLOW[1])
    rr, cc = np.array(SPOTS).T
    fig["planted_valid_and_wrong"] = int(((err0[:, rr, cc] > 1.0) & (i0[:, rr, cc] == 0)).sum())
    model0 = M.median_test(u0, v0, i0)[0] & 1
    fig["planted_model_flags"] = int(model0[:, rr, cc].sum())
    fig["planted_flagged_in_pass0"] = int(((st0 & 1)[:, rr, cc] & model0[:, rr, cc]).sum())
    fig["model_equals_status0"] = bool(np.array_equal(st0 & 1, model0))
    # exactly true of pass 0: outside the flagged cells the two plans hold the same bits, and the masks are equal
    u0n, v0n, i0n = _np(*on.pass_fields(0, n))
    keep0 = model0 == 0
    fig["pass0_unflagged_bit_identical"] = bool(np.array_equal(_bits(u0n)[keep0], _bits(u0)[keep0])
                                                and np.array_equal(_bits(v0n)[keep0], _bits(v0)[keep0])
                                                and np.array_equal(i0n, i0))
    # ... and of the last pass: its flags are the model's on the fields it delivers, everywhere
    fig["model_equals_status_last"] = bool(np.array_equal(stl & 1, M.median_test(un, vn, stl >> 1)[0] & 1))
    # final grid (31 x 31, 8 px spacing, centres at 8 + 8 i): cells near a planted place / away from all of them
    yc, xc = np.mgrid[0:31, 0:31] * 8.0 + 8.0
    d = np.min([np.maximum(np.abs(yc - (16 * r + 16)), np.abs(xc - (16 * c + 16))) for r, c in SPOTS], axis=0)
    near, far = d <= 32.0, d > 64.0           # within two first-pass steps of a patch centre / more than four away
    bad_off = bad_on = near_off = 0
    far_diff = far_diff_all = 0.0
    far_compared = 0
    planted = np.zeros((15, 15), bool)
    planted[rr, cc] = True
    for k in range(n):
        duo = delivered(uo[k], vo[k], io[k])
        dun = delivered(un[k], vn[k], inn[k])
        eo = np.hypot(duo[0] - FLOW[0], duo[1] - FLOW[1])
        en = np.hypot(dun[0] - FLOW[0], dun[1] - FLOW[1])
        bad_off += int((eo > 1.0).sum())
        bad_on += int((en > 1.0).sum())
        near_off += int((eo[near] > 1.0).sum())
        # the DELIVERED fields (filled cells included) far from the patches, with the exception the feature itself makes
        # in a clean flow: cells the last pass flags (they are filled instead of kept), and cells within 1.5 first-pass
        # steps of a first-pass vector the model flags away from the patches (it is replaced, and predicts them)
        exc = (stl[k] & 1) != 0
        for r, c in np.argwhere((model0[k] != 0) & ~planted):
            exc |= np.maximum(np.abs(yc - (16 * r + 16)), np.abs(xc - (16 * c + 16))) <= 24.0
        dk = np.maximum(np.abs(duo[0] - dun[0]), np.abs(duo[1] - dun[1]))
        far_diff_all = max(far_diff_all, float(dk[far & ((stl[k] & 1) == 0)].max()))
        far_diff = max(far_diff, float(dk[far & ~exc].max()))
        far_compared += int((far & ~exc).sum())
    fig.update(bad_off=bad_off, bad_on=bad_on, near_bad_off=near_off, far_max_diff=far_diff,
               far_max_diff_incl_clean_pass0_flags=far_diff_all, far_cells=int(n * far.sum()), far_compared=far_compared)
    # the clean flow (no patch) through the same plan with the test: what it flags there is false
    Ac, Bc = (t.cuda() for t in planted_frames(plant=False))
    uc, vc, ic = _np(*on.run(Ac, Bc))
    stc, = _np(on.outlier_status(1, n))
    ok = (stc >> 1) == 0
    fig["clean_flag_share"] = float((stc & 1).mean())
    fig["clean_rms"] = float(np.sqrt(np.mean(np.concatenate([(uc - FLOW[0])[ok], (vc - FLOW[1])[ok]]) ** 2)))
    fig["clean_equals_model"] = bool(np.array_equal(stc & 1, M.median_test(uc, vc, stc >> 1)[0] & 1))
    off.close()
    on.close()
    return fig


def test_planted_spurious_peaks_are_caught_between_the_passes(eng):
    """Four pairs of a uniform flow (2.3, -1.6) px with four planted patches each (PLANT = (9, -7) px, 28 x 28 px centred
    on 32 px first-pass windows), chain 32/16 -> 16/8 CWS, "exact".  (A 24 px patch is not enough: half of the planted
    windows then keep the true peak or fail the peak ratio.)  frames_figures prints every figure before it is asserted.

    FIGURES.  Not measured on the device.  The numpy model and the CPU oracle (oracle.piv_oracle, whose fields the device
    matches to about 1e-6 px) give on these frames: 15 of 16 planted windows valid and more than 1 px off in pass 0 (the
    16th fails the peak ratio), 16 of 16 flagged by the model; delivered vectors more than 1 px off 195 without the
    keyword (192 within two first-pass steps of a patch) and 80 with it, of 3 844; far_max_diff 0.079 px over 698 of the
    724 far cells (0.130 px with only the last pass's flags excepted); clean pairs: 13 of 3 844 cells flagged (0.34 %,
    all on the border rows and columns), clean_rms 0.049 px.

    Asserted:
    - at least 12 of the 16 planted windows carry a valid first-pass vector more than 1 px off (the precondition that
      makes this test fail without the feature), and without the keyword vectors more than 1 px off are delivered
      within two first-pass steps of the patches;
    - exactly: with the keyword the pass-0 status map is the model's, every planted window the model flags is flagged,
      outside the flagged cells the pass-0 fields of the two plans are bit-identical and so are the masks, and the last
      pass's flags are the model's on the fields it delivers, over the whole field;
    - the count of delivered vectors (valid, or filled by the post-validation) more than 1 px off falls from bad_off
      to bad_on <= 100 (a quarter over the 80 that the numpy model and the CPU oracle give on these frames; counts at a
      1 px threshold, which the 1e-6 px between oracle and device, or between boxes, do not move).  What remains are
      cells of the fine grid whose own 16 px window lies inside a patch: the correlation there really peaks at PLANT,
      and a block of them outvotes its neighbourhood (iterating the test, or a wider neighbourhood, is out of scope);
    - more than four first-pass steps from every patch centre the DELIVERED fields of the two runs (filled cells
      included) agree to FAR_TOL = 0.2 px.  They are not bit-identical: the spline predictor has global support -- up to
      nine coarse vectors change per patch by at most 6.7 px per component, the operator's weights decay like 0.268 per
      cell and multiply over the two axes, so 3.5 steps from the nearest changed column the predictor
      moves by at most (0.268^3.5 + 0.268^4.5 + 0.268^5.5) x (1 + 2 x 0.268) x 6.7 = 0.14 px, and the converged CWS
      result by no more than its predictor; 0.2 px leaves the sub-pixel response of the pass on top.  Excepted, as
      cells the test flags in the clean flow: cells the last pass flags, and cells within 1.5 first-pass steps of a
      first-pass vector that the model flags away from the patches (that vector is replaced and predicts them: one
      such border vector, moved by 0.23 px, accounts for the 0.13 px of far_max_diff_incl_clean_pass0_flags);
    - on the same pairs WITHOUT patches the plan's last-pass flags are the model's and their share stays under
      FALSE_FLAG_CAP = 1 %, with the valid vectors' rms error against the true flow (clean_rms) under the 0.07 px up to
      which tests/test_outlier_host.py shows the model alone under that cap."""
    fig = frames_figures(eng)
    print("outlier frames figures:", fig)
    assert fig["planted_valid_and_wrong"] >= 12
    assert fig["near_bad_off"] > 0
    assert fig["model_equals_status0"] and fig["pass0_unflagged_bit_identical"] and fig["model_equals_status_last"]
    assert fig["planted_model_flags"] >= 12 and fig["planted_flagged_in_pass0"] == fig["planted_model_flags"]
    assert fig["bad_on"] < fig["bad_off"] and fig["bad_on"] <= 100
    assert fig["far_cells"] > 500 and fig["far_compared"] > 0.9 * fig["far_cells"]
    assert fig["far_max_diff"] < FAR_TOL
    assert fig["clean_equals_model"]
    assert fig["clean_flag_share"] < FALSE_FLAG_CAP
    assert fig["clean_rms"] < 0.07


# ---------------------------------------------------------------------------------------------------------------------
# the host paths
# ---------------------------------------------------------------------------------------------------------------------
def _fields(gen):
    return {i: (np.asarray(u), np.asarray(v)) for i, x, y, u, v in gen}


def _same(f1, f2):
    assert sorted(f1) == sorted(f2)
    for i in f1:
        assert np.array_equal(f1[i][0], f2[i][0], equal_nan=True) and np.array_equal(f1[i][1], f2[i][1], equal_nan=True), i


def _write_folder(path, A, B):
    from PIL import Image
    for i in range(A.shape[0]):
        Image.fromarray(A[i].numpy(), "L").save(path / f"image{i}_a.bmp")
        Image.fromarray(B[i].numpy(), "L").save(path / f"image{i}_b.bmp")


@pytest.mark.parametrize("outlier", ["median", {"threshold": 3.0, "min_neighbours": 6}])
def test_host_paths_agree_with_the_keyword(tmp_path, outlier):
    """batched(), __call__ through batched() and the one-pair loop (call_batch = 1) of OfflinePIV, ResidentPIV and
    run_folder give the same fields bit for bit with outlier= set, as they do without it -- and not the fields of a run
    without it."""
    import torchpiv_amd as T
    from torchpiv_amd import runner
    A, B = planted_frames()
    _write_folder(tmp_path, A, B)
    kw = dict(multipass=2, multipass_mode="CWS", outlier=outlier)
    res = T.ResidentPIV(A.cuda(), B.cuda(), 32, 16, **kw)
    want = _fields(res.batched(3))
    assert len(want) > 0
    plain = _fields(T.ResidentPIV(A.cuda(), B.cuda(), 32, 16, multipass=2, multipass_mode="CWS").batched(3))
    common = [i for i in want if i in plain]
    assert any(not np.array_equal(want[i][0], plain[i][0], equal_nan=True) for i in common) or sorted(want) != sorted(plain)
    # stats: the vectors the last pass flagged, over all pairs (dropped ones included) -- the plan's own status maps
    plan = res._get_plan(FH, FW, max_batch=A.shape[0])
    plan.run(A.cuda(), B.cuda())
    flagged = int((plan.outlier_status(1, A.shape[0]) & 1).sum())
    assert flagged > 0 and res.stats["outliers_flagged"] == flagged and res.stats["pairs"] == A.shape[0]
    assert "outliers_flagged" in T.ResidentPIV(A.cuda(), B.cuda(), 32, 16).stats
    piv = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", 32, 16, **kw)
    _same(_fields(piv.batched(4)), want)
    assert piv.stats["outliers_flagged"] == flagged
    _same(_fields(piv.batched(2, indices=[3, 0])), {i: want[i] for i in (3, 0) if i in want})
    order = sorted(want)
    for call_batch in (32, 1):
        p2 = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", 32, 16, **kw)
        p2.call_batch = call_batch
        out = list(p2())
        assert len(out) == len(order) and p2.stats["outliers_flagged"] == flagged
        for i, (x, y, u, v) in zip(order, out):
            assert np.array_equal(u, want[i][0], equal_nan=True) and np.array_equal(v, want[i][1], equal_nan=True)
        p2.close()
    seen = {}
    runner.run_folder(str(tmp_path), "cuda:0", "bmp", 32, 16, multipass=2, outlier=outlier,
                      on_pair=lambda i, out: seen.__setitem__(i, out["Vx[m/s]"]))
    assert sorted(seen) == order and all(np.array_equal(seen[i], want[i][0], equal_nan=True) for i in seen)
    piv.close()
    res.close()
