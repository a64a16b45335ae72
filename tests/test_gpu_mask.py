"""Geometric mask on the device (mask.hip) and through the plan and the host paths: tpiv_apply_mask, tpiv_mask_coverage and
tpiv_mask_fields against the numpy model of tests/mask_model.py, the plan's mask steps behind every pass (with and
without the median test), off means off, mask= through OfflinePIV / ResidentPIV, and the scene that motivates the
feature.  Every comparison is bit for bit."""
import numpy as np
import pytest
import torch

import mask_model as M
import mask_scene as S
import outlier_model as OM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _np(*ts):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


def _same_fields(got, want, what=""):
    for k, name in enumerate(("u", "v", "invalid")):
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if g.dtype == np.float64:
            g, w = g.view(np.uint64), w.view(np.uint64)
        assert np.array_equal(g, w), (what, name, int((g != w).sum()), np.argwhere(g != w)[:5])


# ---------------------------------------------------------------------------------------------------------------------
# the three kernels against the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3, 5])
@pytest.mark.parametrize("shape", [(16, 16), (37, 53), (64, 64)], ids=["vector", "bytes_tail9", "unaligned"])
def test_apply_mask_equals_the_model(eng, n, shape):
    """16 x 16: the 16-byte path; 37 x 53 = 1961 pixels: the byte path with a tail of 9; 64 x 64 through views that start
    one byte into their buffers: the byte path by alignment.  In place and out of place, mask bytes from {0, 1, 7, 255}."""
    H, W = shape
    rng = np.random.default_rng(n * 100 + H)
    f = rng.integers(1, 256, (n, H, W), dtype=np.uint8)
    m = rng.choice(np.array([0, 1, 7, 255], np.uint8), (H, W))
    want = M.apply(f, m)
    off = 1 if shape == (64, 64) else 0

    def dev(arr):          # a contiguous device view of arr that starts `off` bytes into its buffer
        buf = torch.zeros(arr.size + off + 16, dtype=torch.uint8, device="cuda")
        view = buf[off:off + arr.size].view(arr.shape)
        view.copy_(torch.from_numpy(arr))
        return view, buf
    fd, fbuf = dev(f)
    md, _ = dev(m)
    assert not n or fd.data_ptr() % 16 == off
    out = eng.apply_mask(fd, md)                                    # a fresh tensor
    od, obuf = dev(np.full_like(f, 0xAA))
    assert eng.apply_mask(fd, md, out=od) is od                     # into given memory
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(od.cpu().numpy(), want)
    assert np.array_equal(fd.cpu().numpy(), f)                      # the frames are not written ...
    assert (obuf[:off] == 0).all() and (obuf[off + f.size:] == 0).all()          # ... and nothing outside out is
    assert eng.apply_mask(fd, md, out=fd) is fd                     # in place
    torch.cuda.synchronize()
    assert np.array_equal(fd.cpu().numpy(), want)
    assert (fbuf[:off] == 0).all() and (fbuf[off + f.size:] == 0).all()
    if n:
        assert (want[:, m != 0] == 0).all() and (want[:, m == 0] != 0).all()


def test_apply_mask_single_frame_and_arguments(eng):
    f = torch.full((16, 32), 9, dtype=torch.uint8, device="cuda")
    m = torch.zeros(16, 32, dtype=torch.uint8, device="cuda")
    m[3, 5] = 200
    out = eng.apply_mask(f, m)
    assert out.shape == f.shape and int(out.sum()) == 9 * (16 * 32 - 1) and int(out[3, 5]) == 0
    # a partial overlap raises and launches nothing
    flat = torch.full((3 * 512 + 256,), 5, dtype=torch.uint8, device="cuda")
    frames, shifted = flat[:3 * 512].view(3, 16, 32), flat[256:256 + 3 * 512].view(3, 16, 32)
    with pytest.raises(ValueError):
        eng.apply_mask(frames, m, out=shifted)
    torch.cuda.synchronize()
    assert (flat == 5).all()
    for bad_mask in (m[:8], m.float(), m.cpu(), m.t()):
        with pytest.raises((ValueError, RuntimeError)):
            eng.apply_mask(f, bad_mask)
    with pytest.raises(ValueError):
        eng.apply_mask(f, m, out=torch.empty(16, 16, dtype=torch.uint8, device="cuda"))


def _masks(H, W):
    rng = np.random.default_rng(H)
    corners = np.zeros((H, W), np.uint8)
    corners[0, 0], corners[0, W - 1], corners[H - 1, 0], corners[H - 1, W - 1] = 1, 7, 255, 128
    rand = (rng.random((H, W)) < 0.3).astype(np.uint8) * rng.choice(np.array([1, 7, 255], np.uint8), (H, W))
    return {"zero": np.zeros((H, W), np.uint8), "all": np.full((H, W), 3, np.uint8), "random30": rand, "corners": corners}


COVER = [((97, 131), 8, 0), ((97, 131), 8, 4), ((97, 131), 16, 8), ((97, 131), 32, 16), ((97, 131), 33, 16),
         ((97, 131), 42, 21), ((97, 131), 64, 32), ((300, 520), 256, 128)]


@pytest.mark.parametrize("shape,ws,ov", COVER, ids=[f"{c[1]}_{c[2]}" for c in COVER])
def test_mask_coverage_and_grid_equal_the_model(eng, shape, ws, ov):
    """The counts of tpiv_mask_coverage and the grids a one-pass plan derives from them at thresholds 0, 0.5 and 1, for
    every mask of _masks: ragged frames (97 x 131, 300 x 520), odd and non-power-of-two window sizes, windows larger than
    a wavefront's 64 lanes and smaller."""
    H, W = shape
    plan = eng.Plan(H, W, ws, ov, n_pass=1, max_batch=1, precision="fast")
    with pytest.raises(ValueError):
        plan.mask_grid(0)                                           # no mask yet
    for name, m in _masks(H, W).items():
        want = M.coverage(m, ws, ov)
        md = torch.from_numpy(m).cuda()
        got, = _np(eng.mask_coverage(md, ws, ov))
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (name, np.argwhere(got != want)[:5])
        if name == "all":
            assert (got == ws * ws).all()
        if name == "corners":
            assert got[0, 0] == 1 and got[0, -1] == ((W - ws) % (ws - ov) == 0) and got.sum() <= 4
        for thr in (0.0, 0.5, 1.0):
            plan.set_mask(md, thr)
            grid, = _np(plan.mask_grid(0))
            assert grid.dtype == np.bool_ and np.array_equal(grid, M.grid(want, ws, thr)), (name, thr)
            if thr == 1.0:
                assert not grid.any()                                # limit = ws * ws: nothing is excluded
            if thr == 0.0:
                assert np.array_equal(grid, want > 0)
    plan.close()


@pytest.mark.parametrize("shape", [(3, 5, 7), (3, 1, 1), (0, 5, 7)])
@pytest.mark.parametrize("value", [0, 1])
@pytest.mark.parametrize("with_status", [False, True])
def test_mask_fields_equals_the_model(eng, shape, value, with_status):
    rng = np.random.default_rng(shape[1] * 7 + value)
    B, R, C = shape
    u, v = rng.normal(size=shape), rng.normal(size=shape)
    inv = rng.integers(0, 2, shape).astype(np.uint8)
    st = rng.integers(0, 4, shape).astype(np.uint8)
    grid = np.ones((R, C), np.uint8) if R * C == 1 else (rng.random((R, C)) < 0.4).astype(np.uint8) * 9
    if R * C > 1:
        grid[1, 2], grid[0, 0] = 1, 0
        if B:
            u[0, 1, 2], v[1, 1, 2] = np.nan, -0.0                   # a NaN and a negative zero in an excluded cell
            u[0, 0, 0] = np.nan                                     # ... and a NaN outside the grid stays
    want = M.fields(u, v, inv, grid, value, status=st if with_status else None)
    dev = [torch.from_numpy(x).cuda() for x in ((u, v, inv, st) if with_status else (u, v, inv))]
    got = eng.mask_fields(*dev[:3], torch.from_numpy(grid).cuda(), value, status=dev[3] if with_status else None)
    assert all(g is d for g, d in zip(got, dev))                   # in place
    got = _np(*got)
    for g, w in zip(got, want):
        assert np.array_equal(np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8))
    if B:
        ex = grid != 0
        assert (_bits(got[0])[:, ex] == 0).all() and (_bits(got[1])[:, ex] == 0).all() and (got[2][:, ex] == value).all()
    # a bool grid is taken as well; a bad invalid_value raises
    if B and not with_status:
        again = eng.mask_fields(*[torch.from_numpy(x).cuda() for x in (u, v, inv)], torch.from_numpy(grid != 0).cuda(), value)
        for g, w in zip(_np(*again), want):
            assert np.array_equal(np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8))
        with pytest.raises(ValueError):
            eng.mask_fields(*dev[:3], torch.from_numpy(grid).cuda(), 2)


# ---------------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------------
PH, PW = S.SH, S.SW


@pytest.fixture(scope="module")
def pairs(eng):
    """Three pairs of the block scene as they come and with the masked pixels zeroed (device), and the mask image."""
    A, B = S.block_pairs(3)
    m = S.block_mask()
    md = torch.from_numpy(m).cuda()
    A, B = A.cuda(), B.cuda()
    return A, B, eng.apply_mask(A, md), eng.apply_mask(B, md), m


def _grids(m):
    return [M.grid(M.coverage(m, w, o), w, 0.5) for w, o in ((32, 16), (16, 8))]


def test_the_block_mask_excludes_and_partly_covers_cells_in_every_pass():
    m = S.block_mask()
    for (w, o), g in zip(((32, 16), (16, 8)), _grids(m)):
        c = M.coverage(m, w, o)
        assert g.any() and not g.all() and ((c > 0) & ~g).any() and (c == 0).any()


@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("mode", ["CWS", "DWS"])
def test_off_means_off(eng, pairs, mode, precision):
    """mask=None, an all-zero image with pixels="keep", and a plan switched off with NULL after a masked run give the bits
    of a plan that was never told of the mask, in the fields of every pass; mask_grid raises for the ones without."""
    A, B, _, _, m = pairs
    n = A.shape[0]
    kw = dict(n_pass=2, mode=mode, max_batch=n, precision=precision)
    ref = eng.Plan(PH, PW, 32, 16, **kw)
    want = _np(*ref.run(A, B)) + _np(*ref.pass_fields(0, n))
    none = eng.Plan(PH, PW, 32, 16, mask=None, **kw)
    zero = eng.Plan(PH, PW, 32, 16, mask={"image": np.zeros((PH, PW), np.uint8), "pixels": "keep"}, **kw)
    sw = eng.Plan(PH, PW, 32, 16, mask=m, **kw)
    masked = _np(*sw.run(A, B))
    assert not np.array_equal(_bits(masked[0]), _bits(want[0]))             # the mask did something ...
    sw.set_mask(None)                                                       # ... and is gone again
    for p, has_grid in ((none, False), (zero, True), (sw, False)):
        got = _np(*p.run(A, B)) + _np(*p.pass_fields(0, n))
        _same_fields(got[:3], want[:3], "last pass")
        _same_fields(got[3:], want[3:], "pass 0")
        if has_grid:
            assert not _np(p.mask_grid(0))[0].any() and not _np(p.mask_grid(1))[0].any()
        else:
            with pytest.raises(ValueError):
                p.mask_grid(0)
        p.close()
    ref.close()


@pytest.mark.parametrize("mode,precision", [("CWS", "exact"), ("DWS", "fast")])
def test_plan_pass0_excludes_the_masked_cells(eng, pairs, mode, precision):
    """Pass 0 of a two-pass plan with the mask, on the zeroed frames, against the model applied to the fields of a one-pass
    plan of the same first-pass geometry without a mask on the same frames."""
    _, _, A0, B0, m = pairs
    n = A0.shape[0]
    one = eng.Plan(PH, PW, 32, 16, n_pass=1, mode=mode, max_batch=n, precision=precision)
    u1, v1, i1 = _np(*one.run(A0, B0))
    on = eng.Plan(PH, PW, 32, 16, n_pass=2, mode=mode, max_batch=n, precision=precision, mask=m)
    on.run(A0, B0)
    g0 = _grids(m)[0]
    assert np.array_equal(_np(on.mask_grid(0))[0], g0)
    _same_fields(_np(*on.pass_fields(0, n)), M.fields(u1, v1, i1, g0, 1), "pass 0")
    assert (i1[:, g0] == 0).any() or (_bits(u1)[:, g0] != 0).any()         # the step changed something
    # a one-pass plan with the mask: its only pass is the last one -- excluded cells are valid zero vectors
    last = eng.Plan(PH, PW, 32, 16, n_pass=1, mode=mode, max_batch=n, precision=precision, mask=m)
    _same_fields(_np(*last.run(A0, B0)), M.fields(u1, v1, i1, g0, 0), "one pass")
    for p in (one, on, last):
        p.close()


@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("mode", ["CWS", "DWS"])
def test_plan_later_passes_follow_the_masked_predictor(eng, pairs, mode, precision):
    """For p >= 1 the plan's fields equal the model applied to the function-level pass fed with the plan's own predictor
    of the masked fields of pass p - 1 (three passes: 32/16 -> 16/8 -> 8/4)."""
    _, _, A0, B0, m = pairs
    n = A0.shape[0]
    plan = eng.Plan(PH, PW, 32, 16, n_pass=3, mode=mode, max_batch=n, precision=precision, mask=m)
    last = plan.run(A0, B0)
    fields = [plan.pass_fields(p, n) if p < 2 else last for p in range(3)]
    for p in (1, 2):
        w, o = plan.geometry[p][:2]
        g = M.grid(M.coverage(m, w, o), w, 0.5)
        assert np.array_equal(_np(plan.mask_grid(p))[0], g) and g.any() and ((M.coverage(m, w, o) > 0) & ~g).any()
        seam = eng.iterate(mode, A0, B0, w, o, *plan.debug_predict(p, *fields[p - 1]), precision=precision)
        _same_fields(_np(*fields[p]), M.fields(*_np(*seam), g, 1 if p < 2 else 0), f"pass {p}")
    # the predictor saw the excluded cells of pass 0 as invalid zero vectors
    u0, v0, i0 = _np(*fields[0])
    g0 = _grids(m)[0]
    assert (i0[:, g0] == 1).all() and (_bits(u0)[:, g0] == 0).all() and (_bits(v0)[:, g0] == 0).all()
    plan.close()


@pytest.mark.parametrize("mode,precision", [("CWS", "exact"), ("DWS", "fast")])
def test_plan_with_the_median_test(eng, pairs, mode, precision):
    """mask= and outlier="median" in one plan: the test runs on the masked fields, where excluded cells are invalid (no
    neighbour counts them), and the mask step is applied once more to what the test wrote.  The status map of both passes
    is the model's with the excluded cells at exactly 2."""
    _, _, A0, B0, m = pairs
    n = A0.shape[0]
    g0, g1 = _grids(m)
    one = eng.Plan(PH, PW, 32, 16, n_pass=1, mode=mode, max_batch=n, precision=precision)
    raw0 = _np(*one.run(A0, B0))
    on = eng.Plan(PH, PW, 32, 16, n_pass=2, mode=mode, max_batch=n, precision=precision, mask=m, outlier="median")
    ul, vl, il = _np(*on.run(A0, B0))
    # pass 0: mask, test (flagged vectors replaced by their medians, the peak-ratio mask kept), mask
    mu0, mv0, mi0 = M.fields(*raw0, g0, 1)
    st, medu, medv = OM.median_test(mu0, mv0, mi0)
    ru, rv = OM.replaced(mu0, mv0, st, medu, medv)
    wu, wv, wi, wst = M.fields(ru, rv, mi0, g0, 1, status=st)
    f0 = on.pass_fields(0, n)
    _same_fields(_np(*f0), (wu, wv, wi), "pass 0")
    st0, = _np(on.outlier_status(0, n))
    assert np.array_equal(st0, wst) and (st0[:, g0] == 2).all() and (st0 & 1).any()
    # last pass: mask (invalid to the test), test (flags join the mask), mask (valid zero vectors, status 2)
    seam = _np(*eng.iterate(mode, A0, B0, 16, 8, *on.debug_predict(1, *f0), precision=precision))
    mu1, mv1, mi1 = M.fields(*seam, g1, 1)
    st, _, _ = OM.median_test(mu1, mv1, mi1)
    wu, wv, wi, wst = M.fields(mu1, mv1, mi1 | (st & 1), g1, 0, status=st)
    _same_fields((ul, vl, il), (wu, wv, wi), "last pass")
    st1, = _np(on.outlier_status(1, n))
    assert np.array_equal(st1, wst) and (st1[:, g1] == 2).all() and (il[:, g1] == 0).all()
    # what stats["outliers_flagged"] counts never includes an excluded cell
    flags, = _np(on.outlier_flag_counts(n))
    assert np.array_equal(flags, (wst & 1).sum(axis=(1, 2))) and ((wst & 1)[:, g1] == 0).all()
    one.close()
    on.close()


# ---------------------------------------------------------------------------------------------------------------------
# the host paths
# ---------------------------------------------------------------------------------------------------------------------
def _fields(gen):
    out = {}
    for i, x, y, u, v in gen:
        out[i] = tuple(f.cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f) for f in (u, v))
    return out


def _same(f1, f2):
    assert sorted(f1) == sorted(f2)
    for i in f1:
        assert np.array_equal(_bits(f1[i][0]), _bits(f2[i][0])) and np.array_equal(_bits(f1[i][1]), _bits(f2[i][1])), i


def _write_folder(path, A, B):
    from PIL import Image
    for i in range(A.shape[0]):
        Image.fromarray(A[i].numpy(), "L").save(path / f"image{i}_a.bmp")
        Image.fromarray(B[i].numpy(), "L").save(path / f"image{i}_b.bmp")


@pytest.mark.parametrize("fill", [0.0, float("nan")], ids=["fill0", "fillnan"])
def test_host_paths_agree_and_deliver_the_fill(tmp_path, fill):
    """The one-pair loop of OfflinePIV (call_batch = 1), batched(2) with device_out off and on, and ResidentPIV yield the
    same fields bit for bit with mask= on the same four pairs; excluded cells carry exactly the bits of fill; mask_grid()
    is the model's grid of the last pass, flipped; a run on frames zeroed beforehand with pixels="keep" gives the same
    bits; the caller's tensors of ResidentPIV stay as they were."""
    import torchpiv_amd as T
    A, B = S.block_pairs(4)
    m = S.block_mask()
    _write_folder(tmp_path, A, B)
    kw = dict(multipass=2, multipass_mode="CWS", mask={"image": m, "fill": fill})
    grid = np.flip(_grids(m)[1], axis=0)
    Ad, Bd = A.cuda(), B.cuda()
    res = T.ResidentPIV(Ad, Bd, 32, 16, **kw)
    want = _fields(res.batched(3))
    assert len(want) >= 2                                        # (pairs the post-validation drops yield nothing)
    assert np.array_equal(res.mask_grid(), grid)
    torch.cuda.synchronize()
    assert torch.equal(Ad.cpu(), A) and torch.equal(Bd.cpu(), B)
    fill_bits = _bits(np.array([fill]))[0]
    for u, v in want.values():
        assert (_bits(u)[grid] == fill_bits).all() and (_bits(v)[grid] == fill_bits).all()
    _same(_fields(res.batched(2, indices=[3, 1, 0])), {i: want[i] for i in (3, 1, 0) if i in want})      # gathered pairs
    assert torch.equal(Ad.cpu(), A) and torch.equal(Bd.cpu(), B)
    res.device_out = True
    _same(_fields(res.batched(4)), want)
    # frames zeroed beforehand, pixels="keep": the same bits
    md = torch.from_numpy(m).cuda()
    from torchpiv_amd import engine
    pre = T.ResidentPIV(engine.apply_mask(Ad, md), engine.apply_mask(Bd, md), 32, 16, multipass=2, multipass_mode="CWS",
                        mask={"image": m, "fill": fill, "pixels": "keep"})
    _same(_fields(pre.batched(4)), want)
    # another fill value changes the excluded cells and nothing else
    other = _fields(T.ResidentPIV(Ad, Bd, 32, 16, multipass=2, multipass_mode="CWS", mask={"image": m, "fill": 7.5}).batched(4))
    assert sorted(other) == sorted(want)
    for i in want:
        for k in (0, 1):
            assert np.array_equal(_bits(other[i][k])[~grid], _bits(want[i][k])[~grid]) and (other[i][k][grid] == 7.5).all()
    # ... and not the fields of a run without the mask
    plain = _fields(T.ResidentPIV(Ad, Bd, 32, 16, multipass=2, multipass_mode="CWS").batched(4))
    assert any(i not in plain or not np.array_equal(_bits(want[i][0]), _bits(plain[i][0])) for i in want)
    # files
    piv = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", 32, 16, **kw)
    assert np.array_equal(piv.mask_grid(), grid)
    _same(_fields(piv.batched(2)), want)
    piv.device_out = True
    _same(_fields(piv.batched(2)), want)
    piv.device_out = False
    piv.call_batch = 1
    out = list(piv())
    order = sorted(want)
    assert len(out) == len(order)
    for i, (x, y, u, v) in zip(order, out):
        assert np.array_equal(_bits(u), _bits(want[i][0])) and np.array_equal(_bits(v), _bits(want[i][1]))
    for p in (piv, res, pre):
        p.close()


# ---------------------------------------------------------------------------------------------------------------------
# the point of the feature
# ---------------------------------------------------------------------------------------------------------------------
def _delivered(u, v, inv):
    """What a caller receives of one pair: invalid vectors filled by the reference's post-validation; the field as it is
    where nothing is invalid or the pair would be dropped."""
    from torchpiv_amd import backend
    if not inv.any():
        return u, v
    fu, fv = backend.post_validate(u.copy(), v.copy(), inv.astype(bool))
    return (u, v) if fu is None else (fu, fv)


def test_a_lit_static_band_no_longer_pulls_vectors_to_zero(eng):
    """Four pairs of synth's uniform flow (2.3, -1.6) px, 256 x 256, with rows 103...146 of both frames replaced by
    max(frame, static texture); 32/16 in one pass and 32/16 -> 16/8 CWS, "exact".  Without the mask more than five windows
    of grid rows 5...9 lie over 0.5 px from the flow (the CPU oracle: 65...70 per pair, 2.7 px mean on rows 6...8); with it
    no cell of the first-pass grid that is not excluded does (the oracle: at most 0.50 px, row means 0.17 px or less).
    For the two-pass chain the count of delivered vectors outside the excluded cells that are over 0.5 px off is lower
    with the mask than without; the counts are printed."""
    A, B, m = S.band_batch(4)
    A, B, md = A.cuda(), B.cuda(), torch.from_numpy(m).cuda()
    A0, B0 = eng.apply_mask(A, md), eng.apply_mask(B, md)
    n = A.shape[0]
    g0, g1 = _grids(m)
    assert np.flatnonzero(g0[:, 0]).tolist() == [6, 7, 8]

    def err(u, v):
        return np.hypot(u - S.FLOW[0], v - S.FLOW[1])
    off1 = eng.Plan(256, 256, 32, 16, n_pass=1, max_batch=n)
    u, v, _ = _np(*off1.run(A, B))
    bad_off1 = int((err(u, v)[:, 5:10] > 0.5).sum())
    fb_off = off1.exact_fallbacks()
    on1 = eng.Plan(256, 256, 32, 16, n_pass=1, max_batch=n, mask=m)
    u, v, inv = _np(*on1.run(A0, B0))
    fb_on = on1.exact_fallbacks()
    e_on = err(u, v)[:, ~g0]
    print(f"mask, one pass: windows of rows 5..9 over 0.5 px without the mask {bad_off1}; non-excluded cells with it: "
          f"max {e_on.max():.3f} px, over 0.5 px {int((e_on > 0.5).sum())}; exact-mode undecided windows {fb_off} -> {fb_on} "
          f"of {n * 225}")
    assert bad_off1 > 5
    assert not (e_on > 0.5).any()
    assert (_bits(u)[:, g0] == 0).all() and (inv[:, g0] == 0).all()
    counts = {}
    for name, kw, fa, fb in (("off", {}, A, B), ("on", {"mask": m}, A0, B0)):
        plan = eng.Plan(256, 256, 32, 16, n_pass=2, mode="CWS", max_batch=n, **kw)
        u, v, inv = _np(*plan.run(fa, fb))
        bad = 0
        for k in range(n):
            du, dv = _delivered(u[k], v[k], inv[k])
            bad += int((err(du, dv)[~g1] > 0.5).sum())
        counts[name] = bad
        plan.close()
    print(f"mask, 32/16 -> 16/8 CWS: delivered non-excluded vectors over 0.5 px off, of {n * int((~g1).sum())}: "
          f"without the mask {counts['off']}, with it {counts['on']}")
    assert counts["on"] < counts["off"]
    off1.close()
    on1.close()
