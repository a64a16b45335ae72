"""Correlation-statistics uncertainty on the device (uncertainty.hip) and through the plan and the host paths:
tpiv_uncertainty against the numpy model of tests/uncertainty_model.py -- the integer sums bit for bit, the NaN pattern
exactly, sigma to the rounding of three logarithms --, the plan's hook behind the last pass, off means off, and
uncertainty= through ResidentPIV / OfflinePIV."""

import numpy as np
import pytest
import torch

import uncertainty_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _shape(ws, ov):
    st = ws - ov
    return ws + 2 * st + 1, ws + 3 * st + 2               # 3 x 4 windows and a ragged remainder


# (ws, ov, R): R in {0, 3, 4} at 16 and 32, 4 at 128, 3 elsewhere
GEOMETRIES = [(5, 0, 3), (8, 4, 3), (12, 5, 3), (16, 8, 0), (16, 8, 3), (16, 8, 4), (28, 14, 3), (32, 16, 0), (32, 16, 3),
              (32, 16, 4), (64, 32, 3), (128, 64, 4)]
REL_TOL = 1e-9           # on cells whose model numerator and denominator are both >= PART_MIN: three device logarithms,
PART_MIN = 1e-4          # each good to ~1 ulp of values <= 43.7 (7e-15): <= 2e-14 on the numerator, 7e-14 on the denominator

_frames_cache = {}


def _synth_frames(ws, ov):
    """Three pairs of synth's uniform flow with noise at the geometry's frame shape (made once per shape)."""
    from torchpiv_amd import synth
    H, W = _shape(ws, ov)
    if (H, W) not in _frames_cache:
        pairs = [synth.make_pair(H, W, idx, kind="uniform", noise=4.0) for idx in range(3)]
        _frames_cache[(H, W)] = (np.stack([p[0].numpy() for p in pairs]), np.stack([p[1].numpy() for p in pairs]))
    return _frames_cache[(H, W)]


def _flow_fields(ws, ov, seed):
    rng = np.random.default_rng(seed)
    return 2.3 + rng.uniform(-0.3, 0.3, (3, 3, 4)), -1.6 + rng.uniform(-0.3, 0.3, (3, 3, 4))


def _model(A, B, u, v, ws, ov, R, inv):
    outs = [M.field(A[k], B[k], u[k], v[k], ws, ov, R=R, invalid=None if inv is None else inv[k], parts=True)
            for k in range(A.shape[0])]
    su, sv, st = (np.stack([o[i] for o in outs]) for i in range(3))
    parts = [np.stack([o[3][i] for o in outs]) for i in range(4)]
    return su, sv, st, parts


def _compare(eng, A, B, u, v, ws, ov, R, inv=None):
    """engine.uncertainty(..., want_stats=True) against the model on a batch; returns the model's (su, sv, stats, finite
    values, values outside the PART_MIN condition)."""
    dev = [torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in (A, B, u, v)]
    dinv = None if inv is None else torch.from_numpy(inv).cuda()
    su, sv, st = eng.uncertainty(*dev, ws, ov, invalid=dinv, radius=R, want_stats=True)
    su2, sv2 = eng.uncertainty(*dev, ws, ov, invalid=dinv, radius=R)
    torch.cuda.synchronize()
    su, sv, st = su.cpu().numpy(), sv.cpu().numpy(), st.cpu().numpy()
    wsu, wsv, wst, (nu, du, nv, dv) = _model(A, B, u, v, ws, ov, R, inv)
    assert st.dtype == np.int64 and np.array_equal(st, wst), np.argwhere(st != wst)[:6]
    assert np.array_equal(_bits(su2.cpu().numpy()), _bits(su)) and np.array_equal(_bits(sv2.cpu().numpy()), _bits(sv))
    finite = outside = 0
    for got, want, num, den in ((su, wsu, nu, du), (sv, wsv, nv, dv)):
        assert np.array_equal(np.isnan(got), np.isnan(want)), np.argwhere(np.isnan(got) != np.isnan(want))[:6]
        ok = np.isfinite(want)
        assert (got[ok] > 0).all() and np.isfinite(got[ok]).all()
        tight = ok & (np.nan_to_num(num) >= PART_MIN) & (np.nan_to_num(den) >= PART_MIN)
        rel = np.abs(got[tight] - want[tight]) / want[tight]
        if rel.size:
            print(f"uncertainty ws={ws} ov={ov} R={R}: {int(tight.sum())} values, max rel {rel.max():.2e}, "
                  f"min num {num[tight].min():.2e}, min den {den[tight].min():.2e}")
        assert (rel <= REL_TOL).all(), rel.max()
        finite += int(ok.sum())
        outside += int((ok & ~tight).sum())
    return wsu, wsv, wst, finite, outside


@pytest.mark.parametrize("ws,ov,R", GEOMETRIES)
def test_particle_frames_equal_the_model(eng, ws, ov, R):
    """Scene (i): synth's uniform flow with noise, u = 2.3 + U(-0.3, 0.3), v = -1.6 + U(-0.3, 0.3) per cell; batch 3 and
    batch 1, with and without a mask.  The caps keep the comparison from passing on NaNs or on exclusions."""
    A, B = _synth_frames(ws, ov)
    u, v = _flow_fields(ws, ov, seed=ws * 100 + R)
    _, _, _, finite, outside = _compare(eng, A, B, u, v, ws, ov, R)
    total = 2 * u.size
    print(f"uncertainty ws={ws} ov={ov} R={R}: finite {finite}/{total}, outside the condition {outside}")
    if ws >= 8:
        assert finite >= 0.75 * total
    if ws >= 32:
        assert finite >= 0.95 * total
    assert outside <= 0.02 * finite
    inv = (np.random.default_rng(ws + R).random(u.shape) < 0.3).astype(np.uint8) * 5        # any non-zero byte
    inv[0, 0, 0], inv[0, 0, 1] = 1, 0
    wsu, _, wst, _, _ = _compare(eng, A, B, u, v, ws, ov, R, inv)
    assert np.isnan(wsu[inv != 0]).all() and not wst[inv != 0].any() and wst[inv == 0].any()
    _compare(eng, A[1:2], B[1:2], u[1:2], v[1:2], ws, ov, R)
    _compare(eng, A[2:3], B[2:3], u[2:3], v[2:3], ws, ov, R, inv[2:3])


@pytest.mark.parametrize("ws,ov,R", GEOMETRIES)
def test_planted_displacements_equal_the_model(eng, ws, ov, R):
    """Scene (ii): the same frames, fields uniform in +-ws/4 and planted cells: zeros of both signs, whole pixels, the
    largest fraction (fx = 255), a tie of the rounding, displacements that leave the frame (every tap clamped) and
    non-finite values."""
    A, B = _synth_frames(ws, ov)
    rng = np.random.default_rng(ws * 7 + R)
    u = rng.uniform(-ws / 4, ws / 4, (3, 3, 4))
    v = rng.uniform(-ws / 4, ws / 4, (3, 3, 4))
    fu, fv = u.reshape(-1), v.reshape(-1)
    fu[0:6] = [0.0, -0.0, 2.0, -1.0, 255 / 128, 1 / 256]
    fv[6:8] = [200.0, -200.0]
    fu[8] = np.nan
    fv[9] = np.inf
    fu[20], fv[21] = 3 / 256, -np.inf
    wsu, wsv, wst, _, _ = _compare(eng, A, B, u, v, ws, ov, R)
    # (a patch that has left the frame is edge replicate: constant along the axis it left by, not flat, so the cells with
    #  v = +-200 are compared like any other)
    for cell in (8, 9, 21):
        assert np.isnan(wsu.reshape(-1)[cell]) and np.isnan(wsv.reshape(-1)[cell])
    assert not wst.reshape(-1, 8)[[8, 9, 21]].any() and wst.reshape(-1, 8)[0].any()
    _compare(eng, A[:1], B[:1], u[:1], v[:1], ws, ov, R, np.eye(3, 4, dtype=np.uint8)[None])


@pytest.mark.parametrize("ws,ov,R", GEOMETRIES)
def test_white_noise_frames_equal_the_model(eng, ws, ov, R):
    """Scene (iii): uncorrelated frames -- negative C0, lags of either sign, most peaks refused."""
    H, W = _shape(ws, ov)
    rng = np.random.default_rng(ws * 13 + R)
    A = rng.integers(0, 256, (3, H, W)).astype(np.uint8)
    B = rng.integers(0, 256, (3, H, W)).astype(np.uint8)
    B[2] = np.roll(A[2], (-2, 2), axis=(0, 1))            # ... and one pair that does correlate, at (2, -2)
    u, v = _flow_fields(ws, ov, seed=ws + 31 * R)
    u[2], v[2] = 2.0 + (u[2] - 2.3), -2.0 + (v[2] + 1.6)
    _compare(eng, A, B, u, v, ws, ov, R)
    _compare(eng, A[2:], B[2:], u[2:], v[2:], ws, ov, R, np.eye(3, 4, dtype=np.uint8)[None])


def test_flat_and_checkerboard_frames_at_the_largest_size(eng):
    """Scene (iv) at ws = 128, R = 4: all-0 and all-255 frames (every sum zero, NaN), the 0 / 255 checkerboard at whole and
    fractional shifts, and the checkerboard against stripes of period 4, whose |d| = 2 x 510^2 on every other pixel gives
    sums of the size the integer bounds allow for."""
    ws, ov, R = 128, 64, 4
    H, W = _shape(ws, ov)
    yy, xx = np.mgrid[0:H, 0:W]
    board = (((yy + xx) & 1) * 255).astype(np.uint8)
    stripes_x, stripes_y = (((xx >> 1) & 1) * 255).astype(np.uint8), (((yy >> 1) & 1) * 255).astype(np.uint8)
    zero, full = np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8)
    A = np.stack([zero, full, board, board, board])
    B = np.stack([zero, full, board, stripes_x, stripes_y])
    rng = np.random.default_rng(128)
    u = rng.integers(-16, 17, (5, 3, 4)) / 8.0
    v = rng.integers(-16, 17, (5, 3, 4)) / 8.0
    u[:, 0, 0] = v[:, 0, 0] = 0.0
    u[:, 0, 1], v[:, 0, 1] = 0.5, 0.25
    wsu, wsv, wst, _, _ = _compare(eng, A, B, u, v, ws, ov, R)
    assert not wst[:2].any() and np.isnan(wsu[:2]).all() and np.isnan(wsv[:2]).all()
    assert np.abs(wst[3:, :, :, [2, 5]]).max() > 2 ** 48                  # S00 of the striped pairs: the large sums are there
    _compare(eng, A[3:4], B[3:4], u[3:4], v[3:4], ws, ov, R, np.eye(3, 4, dtype=np.uint8)[None])


def test_refusals(eng):
    from torchpiv_amd import _lib

    def call(a, b, H, W, ws, ov, u, v, inv, R, su, sv, st, batch=1):
        ptr = lambda t: None if t is None else t.data_ptr()
        return _lib.lib.tpiv_uncertainty(ptr(a), ptr(b), batch, H, W, ws, ov, ptr(u), ptr(v), ptr(inv), R, ptr(su), ptr(sv),
                                         ptr(st), torch.cuda.current_stream().cuda_stream)

    H = W = 140
    a = torch.zeros(1, H, W, dtype=torch.uint8, device="cuda")
    f = lambda: torch.zeros(1, 7, 7, dtype=torch.float64, device="cuda")      # 32/16 on 140 x 140: 7 x 7
    u, v, su, sv = f(), f(), f(), f()
    su.fill_(-7.0)
    good = (a, a, H, W, 32, 16, u, v, None, 3, su, sv, None)
    bad = {"ws = 130": {4: 130, 5: 65}, "ws = 3": {4: 3, 5: 1}, "R = 5": {9: 5}, "R = -1": {9: -1}, "ov = ws": {5: 32},
           "ov < 0": {5: -1}, "frame below ws": {2: 16}, "null a": {0: None}, "null u": {6: None}, "null su": {10: None},
           "null sv": {11: None}, "su is u": {10: u}, "sv is v": {11: v}, "su is sv": {11: su}}
    for name, change in bad.items():
        args = list(good)
        for k, val in change.items():
            args[k] = val
        rc = call(*args)
        assert rc == _lib.EINVAL, name
        with pytest.raises(ValueError, match="uncertainty"):
            _lib.check(rc)
    # su partly over u, and the stats over an input
    flat = torch.zeros(2 * 49 + 8 * 49, dtype=torch.float64, device="cuda")
    assert call(a, a, H, W, 32, 16, flat[:49], v, None, 3, flat[40:89], sv, None) == _lib.EINVAL
    assert call(a, a, H, W, 32, 16, flat[:49], v, None, 3, su, sv, flat[48:].view(torch.int64)) == _lib.EINVAL
    torch.cuda.synchronize()
    assert (su == -7.0).all()                                                  # nothing was launched
    # batch 0 succeeds and launches nothing -- even with null pointers
    assert call(None, None, H, W, 32, 16, None, None, None, 3, None, None, None, batch=0) == _lib.OK
    assert call(*good) == _lib.OK
    torch.cuda.synchronize()
    assert torch.isnan(su).all()                                               # flat frames: no peak
    # the wrapper: ValueError for each, and for fields of another grid
    z = torch.zeros(1, 140, 140, dtype=torch.uint8, device="cuda")
    for ws, ov, R, shape in ((130, 65, 3, (1, 1, 1)), (3, 1, 3, (1, 69, 69)), (32, 16, 5, (1, 7, 7)), (32, 16, 3, (1, 7, 6))):
        with pytest.raises(ValueError):
            eng.uncertainty(z, z, torch.zeros(shape, dtype=torch.float64, device="cuda"),
                            torch.zeros(shape, dtype=torch.float64, device="cuda"), ws, ov, radius=R)
    with pytest.raises(ValueError):
        eng.Plan(140, 140, 130, 65, uncertainty="cs")
    with pytest.raises(ValueError):
        eng.Plan(140, 140, 32, 16, uncertainty="mc")


# ---------------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------------
PH, PW = 96, 128


def scene_pairs(n=4):
    """n pairs of synth's uniform flow with noise, 96 x 128; in frame b an 18 x 18 block of white noise: a few windows of
    the last pass (16/8) fail the peak ratio there, so that no pair is dropped for having no invalid vector."""
    from torchpiv_amd import synth
    A, B = synth.make_batch(n, PH, PW, kind="uniform", noise=4.0)
    B = B.clone()
    rng = np.random.default_rng(7)
    B[:, 40:58, 60:78] = torch.from_numpy(rng.integers(0, 256, (n, 18, 18)).astype(np.uint8))
    return A, B


def mask_image():
    img = torch.zeros(PH, PW, dtype=torch.uint8)
    img[:, :20] = 1
    return img


@pytest.mark.parametrize("outlier,mask", [(None, False), ("median", False), (None, True), ("median", True)])
def test_plan_estimate_is_the_function_on_what_the_run_returns(eng, outlier, mask):
    A, B = (t.cuda() for t in scene_pairs(3))
    kw = dict(n_pass=2, mode="CWS", max_batch=4, precision="exact", outlier=outlier)
    if mask:
        kw["mask"] = mask_image()
        A, B = eng.apply_mask(A, mask_image().cuda()), eng.apply_mask(B, mask_image().cuda())
    off = eng.Plan(PH, PW, 32, 16, **kw)
    on = eng.Plan(PH, PW, 32, 16, uncertainty="cs", **kw)
    on.set_timing(True)
    off.set_timing(True)
    u0, v0, i0 = off.run(A, B)
    u, v, inv = on.run(A, B)
    su, sv = on.uncertainty(3)
    torch.cuda.synchronize()
    # the run itself is untouched by the option
    assert torch.equal(u0.view(torch.int64), u.view(torch.int64)) and torch.equal(v0.view(torch.int64), v.view(torch.int64))
    assert torch.equal(i0, inv)
    t_on, t_off = on.get_timing(), off.get_timing()
    assert list(t_on[0]) == list(t_off[0]) and len(t_on[0]) == 3 and t_on[1] == t_off[1] == 1
    ws, ov, nr, nc = on.geometry[-1]
    assert (ws, ov) == (16, 8) and tuple(su.shape) == (3, nr, nc)
    dead = inv.clone()
    if mask:
        grid = on.mask_grid(1)
        assert grid.any() and not grid.all()
        dead |= grid.to(torch.uint8)[None]
    wu, wv = eng.uncertainty(A, B, u, v, ws, ov, invalid=dead, radius=3)
    assert torch.equal(su.view(torch.int64), wu.view(torch.int64)) and torch.equal(sv.view(torch.int64), wv.view(torch.int64))
    assert torch.isnan(su[dead != 0]).all() and torch.isnan(sv[dead != 0]).all()
    assert int((inv != 0).sum()) > 0 and torch.isfinite(su[dead == 0]).float().mean() > 0.9
    if outlier:
        flagged = (on.outlier_status(1, 3) & 1) != 0
        assert torch.isnan(su[flagged]).all()
    # a smaller batch on the same plan, another radius through the dict, and off again
    u1, v1, i1 = on.run(A[1:2], B[1:2])
    s1 = on.uncertainty(1)
    assert torch.equal(s1[0].view(torch.int64), su[1:2].view(torch.int64))
    with pytest.raises(ValueError):
        off.uncertainty(3)
    r2 = eng.Plan(PH, PW, 32, 16, uncertainty={"radius": 2}, **kw)
    u2, v2, i2 = r2.run(A, B)
    w2 = eng.uncertainty(A, B, u2, v2, ws, ov, invalid=dead, radius=2)
    assert torch.equal(r2.uncertainty(3)[0].view(torch.int64), w2[0].view(torch.int64))
    assert not torch.equal(w2[0].view(torch.int64), wu.view(torch.int64))
    for p in (off, on, r2):
        p.close()


# ---------------------------------------------------------------------------------------------------------------------
# the host paths
# ---------------------------------------------------------------------------------------------------------------------
def _write_folder(path, A, B):
    from PIL import Image
    for i in range(A.shape[0]):
        Image.fromarray(A[i].numpy(), "L").save(path / f"image{i}_a.bmp")
        Image.fromarray(B[i].numpy(), "L").save(path / f"image{i}_b.bmp")


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _expected(eng, res, A, B, radius, scale, dt, mask=None):
    """Per pair (su, sv, dead) as delivered: the plan's estimate on the frames the passes see, flipped along axis 0 and
    scaled with the reference's expression; dead = invalid or excluded cells, flipped."""
    n = A.shape[0]
    plan = res._get_plan(PH, PW, max_batch=n)
    Ad, Bd = A.cuda(), B.cuda()
    if mask is not None:
        Ad, Bd = eng.apply_mask(Ad, mask.cuda()), eng.apply_mask(Bd, mask.cuda())
    u, v, inv = plan.run(Ad, Bd)
    su, sv = plan.uncertainty(n)
    dead = inv != 0
    if mask is not None:
        dead |= plan.mask_grid(plan.n_pass - 1)[None]
    ws, ov, _, _ = plan.geometry[-1]
    raw = eng.uncertainty(Ad, Bd, u, v, ws, ov, radius=radius)               # without a mask: the estimator's own NaNs
    out = {}
    for k in range(n):
        fs = [np.flip(_np(s[k]), axis=0) * scale / dt * 1000 for s in (su, sv)]
        d = np.flip(_np(dead[k]), axis=0)
        own = np.flip(_np(torch.isnan(raw[0][k])), axis=0), np.flip(_np(torch.isnan(raw[1][k])), axis=0)
        assert np.array_equal(np.isnan(fs[0]), d | own[0]) and np.array_equal(np.isnan(fs[1]), d | own[1])
        assert d.any() and not d.all()
        out[k] = (fs[0], fs[1], d)
    return out


def _check_tuples(got, want, plain, fill=None):
    assert sorted(got) == sorted(plain) and len(got) > 0
    for i, (u, v, su, sv) in got.items():
        assert np.array_equal(_np(u), plain[i][0], equal_nan=True) and np.array_equal(_np(v), plain[i][1], equal_nan=True), i
        for got, exp in ((_np(su), want[i][0]), (_np(sv), want[i][1])):      # finite values bit for bit, sign included
            fin = np.isfinite(exp)
            assert np.array_equal(np.isnan(got), np.isnan(exp)) and np.array_equal(_bits(got)[fin], _bits(exp)[fin]), i
        assert np.isnan(_np(su))[want[i][2]].all() and np.isnan(_np(sv))[want[i][2]].all()
        assert (_np(su)[np.isfinite(_np(su))] > 0).all() and (_np(sv)[np.isfinite(_np(sv))] > 0).all()


def test_resident_paths_deliver_the_plan_estimate(eng):
    import torchpiv_amd as T
    A, B = scene_pairs(4)
    scale, dt = 0.5, 2
    kw = dict(multipass=2, multipass_mode="CWS", scale=scale, dt=dt)
    plain_piv = T.ResidentPIV(A.cuda(), B.cuda(), 32, 16, **kw)
    plain = {o[0]: (o[3], o[4]) for o in plain_piv.batched(3)}
    assert all(len(o) == 5 for o in plain_piv.batched(3)) and all(len(o) == 4 for o in plain_piv())
    res = T.ResidentPIV(A.cuda(), B.cuda(), 32, 16, uncertainty="cs", **kw)
    want = _expected(eng, res, A, B, 3, scale, dt)
    outs = list(res.batched(3))                     # two launches in flight: 3 pairs, then 1
    assert all(len(o) == 7 for o in outs)
    _check_tuples({o[0]: o[3:] for o in outs}, want, plain)
    calls = list(res())
    assert all(len(o) == 6 for o in calls) and len(calls) == len(plain)
    _check_tuples({i: o[2:] for i, o in zip(sorted(plain), calls)}, want, plain)
    res.device_out = True
    outs = list(res.batched(2))
    assert all(len(o) == 7 and all(isinstance(t, torch.Tensor) and t.is_cuda for t in o[3:]) for o in outs)
    _check_tuples({o[0]: o[3:] for o in outs}, want, plain)
    res.close()
    plain_piv.close()
    # with a mask: NaN in the excluded cells, where u, v carry the fill value
    img = mask_image()
    mk = dict(mask={"image": img, "fill": -5.0}, **kw)
    plain_piv = T.ResidentPIV(A.cuda(), B.cuda(), 32, 16, **mk)
    plain = {o[0]: (o[3], o[4]) for o in plain_piv.batched(4)}
    res = T.ResidentPIV(A.cuda(), B.cuda(), 32, 16, uncertainty="cs", **mk)
    want = _expected(eng, res, A, B, 3, scale, dt, mask=img)
    outs = list(res.batched(4))
    _check_tuples({o[0]: o[3:] for o in outs}, want, plain)
    grid = res.mask_grid()
    assert grid.any() and all((o[3][grid] == -5.0).all() and np.isnan(o[5][grid]).all() and np.isnan(o[6][grid]).all()
                              for o in outs)
    res.close()
    plain_piv.close()


def test_offline_paths_deliver_the_plan_estimate(eng, tmp_path):
    import torchpiv_amd as T
    A, B = scene_pairs(4)
    _write_folder(tmp_path, A, B)
    scale, dt = 0.5, 2
    kw = dict(multipass=2, multipass_mode="CWS", scale=scale, dt=dt)
    plain_piv = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", 32, 16, **kw)
    plain = {o[0]: (o[3], o[4]) for o in plain_piv.batched(4)}
    assert all(len(o) == 5 for o in plain_piv.batched(4)) and all(len(o) == 4 for o in plain_piv())
    plain_piv.close()
    res = T.ResidentPIV(A.cuda(), B.cuda(), 32, 16, uncertainty={"radius": 2}, **kw)
    want = _expected(eng, res, A, B, 2, scale, dt)
    res.close()
    piv = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", 32, 16, uncertainty={"radius": 2}, **kw)
    outs = list(piv.batched(3))
    assert all(len(o) == 7 for o in outs)
    _check_tuples({o[0]: o[3:] for o in outs}, want, plain)
    order = sorted(plain)
    for call_batch in (32, 1):                      # through batched(), and the one-pair path: finished on the host
        p2 = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", 32, 16, uncertainty={"radius": 2}, **kw)
        p2.call_batch = call_batch
        calls = list(p2())
        assert all(len(o) == 6 for o in calls) and len(calls) == len(order)
        _check_tuples({i: o[2:] for i, o in zip(order, calls)}, want, plain)
        p2.close()
    piv.device_out = True
    outs = list(piv.batched(4))
    assert all(len(o) == 7 and all(isinstance(t, torch.Tensor) and t.is_cuda for t in o[3:]) for o in outs)
    _check_tuples({o[0]: o[3:] for o in outs}, want, plain)
    piv.close()
