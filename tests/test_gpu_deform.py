"""Iterative image deformation on the device (deform.hip) and through the plan and the host paths: tpiv_deform_nodes,
tpiv_deform_warp and tpiv_deform_combine against the numpy model of tests/deform_model.py bit for bit -- the warp on both
of its paths, the LDS patches and the per-pixel gather --, the refusals, the plan's rounds against the unrolled chain of
functions, off means off, the accuracy on a flow with gradients, and deform= through ResidentPIV / OfflinePIV /
run_folder."""

import numpy as np
import pytest
import torch

import deform_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def _bits(t):
    return t.contiguous().view(torch.int64)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# nodes
# ---------------------------------------------------------------------------------------------------------------------
def _node_fields(nr, nc, batch, seed):
    """Fields with 30 % invalid cells at random, and planted cells: a rounding tie, values past the clamp, NaN and inf in
    valid cells; pair 1 (when there is one) is invalid everywhere but one cell: an isolated valid cell."""
    rng = np.random.default_rng(seed)
    u = rng.normal(0.0, 3.0, (batch, nr, nc))
    v = rng.normal(0.0, 3.0, (batch, nr, nc))
    inv = ((rng.random((batch, nr, nc)) < 0.3) * rng.integers(1, 256, (batch, nr, nc))).astype(np.uint8)   # any non-zero byte
    fu, fv, fi = u.reshape(batch, -1), v.reshape(batch, -1), inv.reshape(batch, -1)
    n = nr * nc
    planted = [(0.5 / 128, -1.5 / 128), (500.0, -1e300), (np.nan, 1.0), (1.0, np.inf), (-np.inf, np.nan), (2.5 / 128, 0.0)]
    for k, (pu, pv) in enumerate(planted):
        if k < n:
            fu[0, k], fv[0, k], fi[0, k] = pu, pv, 0
    if batch > 1:
        fi[1, :] = 1
        fi[1, n // 2] = 0
    return u, v, inv


@pytest.mark.parametrize("nr,nc", [(1, 1), (1, 5), (2, 2), (3, 4), (9, 13), (18, 35)])
def test_nodes_equal_the_model(eng, nr, nc):
    """(18, 35): more than one 16 x 16 block per axis, so the halo crosses block borders."""
    for batch in (3, 1):
        u, v, inv = _node_fields(nr, nc, batch, seed=100 * nr + nc + batch)
        for smooth in (True, False):
            got = eng.deform_nodes(_dev(u), _dev(v), _dev(inv), smooth=smooth)
            want = M.nodes(u, v, inv, smooth)
            assert got.dtype == torch.int16 and tuple(got.shape) == (batch, nr, nc, 2)
            diff = np.argwhere(got.cpu().numpy() != want)
            assert diff.size == 0, (batch, smooth, diff[:6])
    # all cells invalid: zeros
    z = torch.ones(1, nr, nc, dtype=torch.uint8, device="cuda")
    f = torch.full((1, nr, nc), 2.5, dtype=torch.float64, device="cuda")
    assert not eng.deform_nodes(f, f, z).any()


# ---------------------------------------------------------------------------------------------------------------------
# warp
# ---------------------------------------------------------------------------------------------------------------------
WARP_GEOMETRIES = [(8, 4, 40, 52), (12, 5, 45, 61), (16, 8, 70, 93), (32, 16, 96, 128), (64, 32, 130, 172),
                   (32, 16, 40, 44)]        # the last: a frame that holds one window, a 1 x 1 grid


def _warp_frames(H, W, seed):
    """Three pairs: particle images, white noise with 0 and 255 samples, and a 0 / 255 checkerboard against noise."""
    rng = np.random.default_rng(seed)
    a0, b0 = M.scene(seed, H, W)
    noise = rng.integers(0, 256, (2, H, W)).astype(np.uint8)
    noise[0].flat[0], noise[0].flat[-1] = 0, 255
    y, x = np.mgrid[0:H, 0:W]
    board = (((x + y) & 1) * 255).astype(np.uint8)
    return np.stack([a0, noise[0], board]), np.stack([b0, noise[1], noise[1]])


def _warp_fields(ws, nr, nc, seed):
    """name -> nodes int16 [3, nr, nc, 2]."""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:nr, 0:nc]
    smooth = np.stack([np.rint(3 * 256 * np.sin(2 * np.pi * (r + k) / 12.0)) for k in range(3)])
    smooth = np.stack([smooth, np.rint(0.5 * smooth[:, ::-1, ::-1]) + 37], axis=-1)
    q = ws * 256 // 8                                               # +-ws/4 px of displacement = +-ws/8 px of half shift
    clamped = np.empty((3, nr, nc, 2))
    clamped[..., 0], clamped[..., 1] = 12800, -12800                # +-200 px of displacement everywhere: one footprint
    return {"zero": np.zeros((3, nr, nc, 2)),
            "smooth": smooth,
            "random": rng.integers(-q, q + 1, (3, nr, nc, 2)),
            "far": rng.choice([-12800, 12800], (3, nr, nc, 2)),    # +-200 px per node: every position clamped, gathered
            "far uniform": clamped}


@pytest.mark.parametrize("interp", ["cubic", "linear"])
def test_warp_equals_the_model_on_both_paths(eng, interp):
    lds_seen = gather_seen = 0
    for ws, ov, H, W in WARP_GEOMETRIES:
        nr, nc = M.field_shape(H, W, ws, ov)
        A, B = _warp_frames(H, W, seed=ws + H)
        dA, dB = _dev(A), _dev(B)
        tiles = 3 * ((W + 63) // 64) * ((H + 31) // 32)
        for name, nd in _warp_fields(ws, nr, nc, seed=ws * 3 + W).items():
            nd = nd.astype(np.int16)
            want_a, want_b = M.warp(A, B, nd, ws, ov, interp)
            counter = torch.zeros(2, dtype=torch.int32, device="cuda")
            wa, wb = eng.deform_warp(dA, dB, _dev(nd), ws, ov, interp=interp, counter=counter)
            ga, gb = eng.deform_warp(dA, dB, _dev(nd), ws, ov, interp=interp, gather=True)
            w1a, w1b = eng.deform_warp(dA[1:2], dB[1:2], _dev(nd[1:2]), ws, ov, interp=interp)      # batch 1, another base
            lds, gathered = (int(t) for t in counter.cpu())
            where = (ws, ov, H, W, name)
            assert lds + gathered == tiles, where
            for got, want in ((wa, want_a), (wb, want_b), (ga, want_a), (gb, want_b)):
                diff = np.argwhere(got.cpu().numpy() != want)
                assert diff.size == 0, (where, diff[:6])
            assert torch.equal(w1a[0], wa[1]) and torch.equal(w1b[0], wb[1]), where
            if name == "zero":
                assert torch.equal(wa, dA) and torch.equal(wb, dB) and gathered == 0, where
            if name in ("smooth", "far uniform"):
                assert gathered == 0, (where, lds, gathered)
            # nodes of both signs at +-200 px inside a tile: its footprint spans the frame, which a 48 x 96 patch holds
            # only where the frame itself is that small
            if name == "far" and (H > 48 or W > 96):
                assert gathered > 0, (where, lds, gathered)
            # +-8 px of half shift per node at 64/32: the spread over a tile's nodes passes the 12 rows the cubic patch
            # has to spare in some tiles (the smaller windows stay below it: +-4 px and less)
            if name == "random" and ws == 64 and interp == "cubic":
                assert gathered > 0, (where, lds, gathered)
            lds_seen += lds
            gather_seen += gathered
    assert lds_seen > 0 and gather_seen > 0


def test_warp_byte_path_on_unaligned_tensors(eng):
    """Frames and outputs at odd addresses: the patches fill byte by byte and the stores are bytes."""
    ws, ov, H, W = 32, 16, 96, 128
    nr, nc = M.field_shape(H, W, ws, ov)
    A, B = _warp_frames(H, W, seed=5)
    nd = _warp_fields(ws, nr, nc, seed=9)["smooth"].astype(np.int16)
    flat_a = torch.zeros(3 * H * W + 1, dtype=torch.uint8, device="cuda")
    flat_b = torch.zeros(3 * H * W + 3, dtype=torch.uint8, device="cuda")
    flat_a[1:] = _dev(A).view(-1)
    flat_b[3:] = _dev(B).view(-1)
    ua, ub = flat_a[1:].view(3, H, W), flat_b[3:].view(3, H, W)
    assert ua.data_ptr() % 2 == 1 and ua.is_contiguous()
    wa, wb = eng.deform_warp(ua, ub, _dev(nd), ws, ov)
    want_a, want_b = M.warp(A, B, nd, ws, ov, "cubic")
    assert np.array_equal(wa.cpu().numpy(), want_a) and np.array_equal(wb.cpu().numpy(), want_b)


# ---------------------------------------------------------------------------------------------------------------------
# combine, refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_combine_equals_the_model(eng):
    rng = np.random.default_rng(11)
    for shape in ((3, 9, 13), (1, 1, 1), (2, 17, 40)):
        nd = rng.integers(-16383, 16384, shape + (2,)).astype(np.int16)
        du, dv = rng.normal(0, 1, shape), rng.normal(0, 1e-3, shape)
        du.flat[0], dv.flat[0] = np.nan, -0.0
        dval = (rng.random(shape) < 0.2).astype(np.uint8) * 3
        u, v, inv = eng.deform_combine(_dev(nd), _dev(du), _dev(dv), _dev(dval))
        wu, wv, winv = M.combine(nd, du, dv, dval)
        assert np.array_equal(u.cpu().numpy().view(np.uint64), wu.view(np.uint64))
        assert np.array_equal(v.cpu().numpy().view(np.uint64), wv.view(np.uint64))
        assert np.array_equal(inv.cpu().numpy(), winv)


def test_refusals(eng):
    from torchpiv_amd import _lib
    L = _lib.lib
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: None if t is None else t.data_ptr()
    H, W, ws, ov = 70, 96, 16, 8
    nr, nc = M.field_shape(H, W, ws, ov)
    a = torch.zeros(2, H, W, dtype=torch.uint8, device="cuda")
    b = torch.zeros(2, H, W, dtype=torch.uint8, device="cuda")
    wa, wb = torch.full_like(a, 7), torch.full_like(a, 7)
    nodes = torch.zeros(2, nr, nc, 2, dtype=torch.int16, device="cuda")
    table = eng._dewarp_table(a.device)
    counter = torch.zeros(2, dtype=torch.int32, device="cuda")

    def refused(rc, name):
        assert rc == _lib.EINVAL, name
        with pytest.raises(ValueError, match="deform"):
            _lib.check(rc)

    # warp: (a, b, batch, H, W, ws, ov, nodes, table, interp, wa, wb, counter)
    good = [a, b, 2, H, W, ws, ov, nodes, table, 1, wa, wb, counter]
    bad = {"null a": {0: None}, "null b": {1: None}, "null nodes": {7: None}, "cubic without table": {8: None},
           "null wa": {10: None}, "null wb": {11: None}, "interp 2": {9: 2}, "interp -1": {9: -1}, "ws = 1": {5: 1, 6: 0},
           "ws = 258": {5: 258, 6: 0}, "ov = ws": {6: 16}, "ov < 0": {6: -1}, "frame below ws": {3: 8}, "batch < 0": {2: -1},
           "W too large": {4: 1 << 22}, "wa is a": {10: a}, "wb is b": {11: b}, "wa is wb": {11: wa},
           "counter in wa": {12: wa.view(torch.int32)}, "nodes misaligned": {7: nodes.view(-1)[1:]}}
    for name, change in bad.items():
        args = list(good)
        for k, val in change.items():
            args[k] = val
        refused(L.tpiv_deform_warp(*[ptr(x) if isinstance(x, torch.Tensor) or x is None else x for x in args], st), name)
    flat = torch.zeros(4 * H * W, dtype=torch.uint8, device="cuda")
    refused(L.tpiv_deform_warp(ptr(flat[:2 * H * W]), ptr(b), 2, H, W, ws, ov, ptr(nodes), ptr(table), 1,
                               ptr(flat[H * W:3 * H * W]), ptr(wb), None, st), "wa partly over a")
    torch.cuda.synchronize()
    assert (wa == 7).all() and (wb == 7).all() and not counter.any()            # nothing was launched
    assert L.tpiv_deform_warp(None, None, 0, H, W, ws, ov, None, None, 1, None, None, None, st) == _lib.OK      # batch 0
    assert L.tpiv_deform_warp(ptr(a), ptr(b), 2, H, W, ws, ov, ptr(nodes), None, 0, ptr(wa), ptr(wb), None, st) == _lib.OK
    torch.cuda.synchronize()
    assert not wa.any() and not wb.any()                                         # linear needs no table; zero frames

    # nodes: (u, v, invalid, batch, n_rows, n_cols, smooth, nodes)
    u = torch.zeros(2, nr, nc, dtype=torch.float64, device="cuda")
    v = torch.zeros_like(u)
    inv = torch.zeros(2, nr, nc, dtype=torch.uint8, device="cuda")
    nodes.fill_(5)
    good = [u, v, inv, 2, nr, nc, 1, nodes]
    bad = {"null u": {0: None}, "null v": {1: None}, "null invalid": {2: None}, "null nodes": {7: None}, "batch < 0": {3: -1},
           "no rows": {4: 0}, "no columns": {5: 0}, "nodes over u": {7: u.view(torch.int16)},
           "nodes misaligned": {7: torch.zeros(4 * nr * nc + 1, dtype=torch.int16, device="cuda")[1:]}}
    for name, change in bad.items():
        args = list(good)
        for k, val in change.items():
            args[k] = val
        refused(L.tpiv_deform_nodes(*[ptr(x) if isinstance(x, torch.Tensor) or x is None else x for x in args], st), name)
    torch.cuda.synchronize()
    assert (nodes == 5).all()
    assert L.tpiv_deform_nodes(None, None, None, 0, nr, nc, 1, None, st) == _lib.OK

    # combine: (nodes, du, dv, dval, batch, n_rows, n_cols, u, v, invalid)
    du, dv, dval = torch.ones_like(u), torch.ones_like(u), torch.ones_like(inv)
    u.fill_(-7.0)
    good = [nodes, du, dv, dval, 2, nr, nc, u, v, inv]
    bad = {"null nodes": {0: None}, "null du": {1: None}, "null dval": {3: None}, "null u": {7: None}, "null invalid": {9: None},
           "batch < 0": {4: -1}, "no rows": {5: 0}, "u is du": {7: du}, "v is u": {8: u}, "invalid is dval": {9: dval},
           "u over nodes": {7: nodes.view(-1).view(torch.float64)}}
    for name, change in bad.items():
        args = list(good)
        for k, val in change.items():
            args[k] = val
        refused(L.tpiv_deform_combine(*[ptr(x) if isinstance(x, torch.Tensor) or x is None else x for x in args], st), name)
    torch.cuda.synchronize()
    assert (u == -7.0).all() and not inv.any()
    assert L.tpiv_deform_combine(None, None, None, None, 0, nr, nc, None, None, None, st) == _lib.OK

    # the wrappers and the plan
    with pytest.raises(ValueError):
        eng.deform_warp(a, b, nodes[:, :-1], ws, ov)
    with pytest.raises(ValueError):
        eng.deform_warp(a, b, nodes, ws, ov, interp="nearest")
    with pytest.raises(ValueError):
        eng.deform_combine(nodes[:, :-1], du, dv, dval)
    with pytest.raises(ValueError, match="deform"):
        eng.Plan(H, W, 32, 16, deform=9)
    plain = eng.Plan(H, W, 32, 16)
    with pytest.raises(ValueError):
        plain.deform_stage(1)
    with pytest.raises(ValueError):
        plain.deform_ms()
    on = eng.Plan(H, W, 32, 16, deform=1)
    with pytest.raises(ValueError):
        on.deform_ms()                                                           # before the first run
    plain.close()
    on.close()


# ---------------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------------
PH, PW = 96, 128


def scene_pairs(n=4, kind="wavy"):
    """n pairs of synth's wavy (or uniform) flow with noise, 96 x 128; in frame b an 18 x 18 block of white noise: a few
    windows of the last pass (16/8) fail the peak ratio there, so that no pair is dropped for having no invalid vector."""
    from torchpiv_amd import synth
    A, B = synth.make_batch(n, PH, PW, kind=kind, noise=4.0)
    B = B.clone()
    rng = np.random.default_rng(7)
    B[:, 40:58, 60:78] = torch.from_numpy(rng.integers(0, 256, (n, 18, 18)).astype(np.uint8))
    return A, B


def mask_image():
    img = torch.zeros(PH, PW, dtype=torch.uint8)
    img[:, :20] = 1
    return img


def _chain(eng, off, A, B, n, interp, smooth, test, grid, precision="exact"):
    """The rounds as the header prescribes them, from the functions of the function level."""
    u, v, inv = off.run(A, B)
    ws, ov, _, _ = off.geometry[-1]
    stage = status = None
    for k in range(1, n + 1):
        final = k == n
        nd = eng.deform_nodes(u, v, inv, smooth=smooth)
        wa, wb = eng.deform_warp(A, B, nd, ws, ov, interp=interp)
        du, dv, dval = eng.pass1(wa, wb, ws, ov, precision=precision)
        stage = (nd, wa, wb, du, dv, dval)
        cu, cv, cval = eng.deform_combine(nd, du, dv, dval)
        if grid is not None:
            eng.mask_fields(cu, cv, cval, grid, 1 if test else 0)
        if not test:
            u, v, inv = cu, cv, cval
            continue
        status, mu, mv = eng.median_test(cu, cv, cval, want_medians=True)
        flag = (status & 1) != 0
        if final:
            u, v, inv = cu, cv, ((cval != 0) | flag).to(torch.uint8)
        else:
            u, v, inv = torch.where(flag, mu, cu), torch.where(flag, mv, cv), cval
        if grid is not None:
            eng.mask_fields(u, v, inv, grid, 0, status=status)
    return u, v, inv, stage, status


@pytest.mark.parametrize("outlier,mask", [(None, False), ("median", False), (None, True), ("median", True)])
@pytest.mark.parametrize("n,interp,smooth", [(1, "cubic", True), (3, "cubic", True), (2, "linear", False)])
def test_plan_equals_the_unrolled_chain(eng, outlier, mask, n, interp, smooth):
    A, B = (t.cuda() for t in scene_pairs(3))
    kw = dict(n_pass=2, mode="CWS", max_batch=4, precision="exact", outlier=outlier)
    grid = None
    if mask:
        kw["mask"] = mask_image()
        A, B = eng.apply_mask(A, mask_image().cuda()), eng.apply_mask(B, mask_image().cuda())
    off = eng.Plan(PH, PW, 32, 16, **kw)
    on = eng.Plan(PH, PW, 32, 16, deform={"iterations": n, "interp": interp, "smooth": smooth}, **kw)
    if mask:
        grid = off.mask_grid(1)
        assert grid.any() and not grid.all()
    wu, wv, winv, wstage, wstatus = _chain(eng, off, A, B, n, interp, smooth, outlier is not None, grid)
    u, v, inv = on.run(A, B)
    stage = on.deform_stage(3)
    torch.cuda.synchronize()
    assert _same(u, wu) and _same(v, wv) and torch.equal(inv, winv)
    for got, want in zip(stage, wstage):
        assert got.dtype == want.dtype and torch.equal(got.view(torch.uint8), want.contiguous().view(torch.uint8))
    if outlier:
        assert torch.equal(on.outlier_status(1, 3), wstatus)
    if mask:
        assert not u[:, grid].any() and not inv[:, grid].any()
    u0, v0, _ = off.run(A, B)
    assert not _same(u, u0)                                      # the rounds did something
    assert on.deform_ms() > 0.0
    # a smaller batch on the same plan
    u1, v1, i1 = on.run(A[1:2], B[1:2])
    assert _same(u1, wu[1:2]) and _same(v1, wv[1:2]) and torch.equal(i1, winv[1:2])
    s1 = on.deform_stage(1)
    assert torch.equal(s1[1], wstage[1][1:2]) and _same(s1[3], wstage[3][1:2])
    off.close()
    on.close()


def _settled(eng, u, v, inv, grid, feeds):
    """What a plan with mask= and the median test puts behind a pass, from the function level (in place on u, v, inv where
    it can be).  feeds: the predictor reads the fields next -- flagged vectors are replaced by their medians and excluded
    cells stay invalid; behind the last pass the flags join the mask and excluded cells end up valid."""
    eng.mask_fields(u, v, inv, grid, 1)
    status, mu, mv = eng.median_test(u, v, inv, want_medians=True)
    flag = (status & 1) != 0
    if feeds:
        u, v = torch.where(flag, mu, u), torch.where(flag, mv, v)
    else:
        inv = ((inv != 0) | flag).to(torch.uint8)
    eng.mask_fields(u, v, inv, grid, 1 if feeds else 0, status=status)
    return u, v, inv, status


@pytest.mark.parametrize("mode,precision", [("CWS", "exact"), ("DWS", "fast")])
def test_three_pass_plan_with_everything_on_equals_the_unrolled_chain(eng, mode, precision):
    """32/16 -> 16/8 -> 8/4 with outlier=, mask=, deform= and uncertainty= on: the one plan in the suite with a middle
    pass, which is predicted into, run by the shifted-pass kernel, settled for the predictor and predicted from, and the
    one where the spare fields of the median step serve two geometries.  Expected: the function level alone."""
    import types
    A, B = (t.cuda() for t in scene_pairs(3))
    m = mask_image()
    A, B = eng.apply_mask(A, m.cuda()), eng.apply_mask(B, m.cuda())
    n, interp, smooth = 2, "cubic", True
    on = eng.Plan(PH, PW, 32, 16, n_pass=3, mode=mode, max_batch=4, precision=precision, outlier="median", mask=m,
                  deform={"iterations": n}, uncertainty="cs")
    assert [g[:2] for g in on.geometry] == [(32, 16), (16, 8), (8, 4)]
    grids = [on.mask_grid(p) for p in range(3)]
    # the passes
    fields, status = [], []
    u, v, inv = eng.pass1(A, B, 32, 16, precision=precision)
    for p in range(3):
        if p:
            ws, ov = on.geometry[p][:2]
            u, v, inv = eng.iterate(mode, A, B, ws, ov, *on.debug_predict(p, u, v, inv), precision=precision)
        u, v, inv, st = _settled(eng, u, v, inv, grids[p], feeds=p < 2)
        fields.append((u, v, inv))
        status.append(st)
    n_flag1, n_inv2 = int((status[1] & 1).sum()), int((inv != 0).sum())
    print(f"{mode} {precision}: excluded at 16/8 {int(grids[1].sum())} of {grids[1].numel()}, flagged at 16/8 {n_flag1}, "
          f"invalid behind 8/4 {n_inv2}")
    assert grids[1].any() and not grids[1].all()
    assert n_flag1 > 0 and n_inv2 > 0
    # the rounds on what the last pass left, then the estimate on the frames of the run
    last = types.SimpleNamespace(run=lambda a, b: fields[2], geometry=on.geometry)
    wu, wv, winv, wstage, wstatus = _chain(eng, last, A, B, n, interp, smooth, True, grids[2], precision=precision)
    dead = winv | grids[2].to(torch.uint8)[None]
    wsu, wsv = eng.uncertainty(A, B, wu, wv, 8, 4, invalid=dead, radius=3)
    status[2] = wstatus

    def check(batch, sl):
        u, v, inv = on.run(A[sl], B[sl])
        su, sv = on.uncertainty(batch)
        stage = on.deform_stage(batch)
        torch.cuda.synchronize()
        assert _same(u, wu[sl]) and _same(v, wv[sl]) and torch.equal(inv, winv[sl])
        for p in range(2):
            fu, fv, fi = on.pass_fields(p, batch)
            assert _same(fu, fields[p][0][sl]) and _same(fv, fields[p][1][sl]) and torch.equal(fi, fields[p][2][sl]), p
        for p in range(3):
            assert torch.equal(on.outlier_status(p, batch), status[p][sl]), p
        for got, want in zip(stage, wstage):
            assert got.dtype == want.dtype and torch.equal(got.view(torch.uint8), want[sl].contiguous().view(torch.uint8))
        assert _same(su, wsu[sl]) and _same(sv, wsv[sl])
        assert torch.equal(torch.isnan(su), torch.isnan(wsu[sl])) and torch.isnan(su[dead[sl] != 0]).all()

    check(3, slice(0, 3))
    assert not _same(wu, fields[2][0])                           # the rounds did something
    check(1, slice(1, 2))                                        # a smaller batch on the same plan
    on.close()


def test_single_pass_plan_deforms_behind_pass_one(eng):
    A, B = (t.cuda() for t in scene_pairs(2))
    off = eng.Plan(PH, PW, 16, 8, n_pass=1, max_batch=2, precision="f64")
    on = eng.Plan(PH, PW, 16, 8, n_pass=1, max_batch=2, precision="f64", deform=2)
    u, v, inv = off.run(A, B)
    for _ in range(2):
        nd = eng.deform_nodes(u, v, inv)
        wa, wb = eng.deform_warp(A, B, nd, 16, 8)
        u, v, inv = eng.deform_combine(nd, *eng.pass1(wa, wb, 16, 8, precision="f64"))
    gu, gv, ginv = on.run(A, B)
    assert _same(gu, u) and _same(gv, v) and torch.equal(ginv, inv)
    off.close()
    on.close()


def test_off_means_off(eng):
    A, B = (t.cuda() for t in scene_pairs(3))
    kw = dict(n_pass=2, mode="CWS", max_batch=3, precision="exact", outlier="median", mask=mask_image())
    plain = eng.Plan(PH, PW, 32, 16, **kw)
    plans = [eng.Plan(PH, PW, 32, 16, deform=d, **kw) for d in (None, 0, {"iterations": 0, "interp": "linear"})]
    on = eng.Plan(PH, PW, 32, 16, deform=2, **kw)
    for p in [plain, on] + plans:
        p.set_timing(True)
    want = plain.run(A, B)
    t_plain = plain.get_timing()
    n_plain = plain.exact_fallbacks()
    for p in plans:
        got = p.run(A, B)
        assert p.deform is None
        assert _same(got[0], want[0]) and _same(got[1], want[1]) and torch.equal(got[2], want[2])
        t = p.get_timing()
        assert list(t[0]) == list(t_plain[0]) and t[1] == t_plain[1] == 1
        assert torch.equal(p.mask_grid(1), plain.mask_grid(1)) and torch.equal(p.outlier_status(0, 3), plain.outlier_status(0, 3))
        assert p.exact_fallbacks() == n_plain
        with pytest.raises(ValueError):
            p.deform_stage(3)
    # a deforming plan keeps the slots, the grids and the count of pass 1
    on.run(A, B)
    t = on.get_timing()
    assert list(t[0]) == list(t_plain[0]) and len(t[0]) == 3 and t[1] == 1
    assert on.exact_fallbacks() == n_plain
    assert torch.equal(on.mask_grid(1), plain.mask_grid(1))
    assert torch.equal(on.outlier_status(0, 3), plain.outlier_status(0, 3))
    for p in [plain, on] + plans:
        p.close()


def test_accuracy_on_a_flow_with_gradients(eng):
    """The scene of deform_model (peak gradient 0.196 px / px), 3 pairs of 256 x 256, 32/16 two-pass CWS "exact": the RMS
    vector error against the constructed flow with deform=3 must be at most half of the plain field's, over the interior
    cells (a one-cell rim left out) valid in both runs, which must be at least 95 % of the interior, per pair."""
    H = W = 256
    pairs = [M.scene(seed, H, W) for seed in range(3)]
    A, B = _dev(np.stack([p[0] for p in pairs])), _dev(np.stack([p[1] for p in pairs]))
    kw = dict(n_pass=2, mode="CWS", max_batch=3, precision="exact")
    off, on = eng.Plan(H, W, 32, 16, **kw), eng.Plan(H, W, 32, 16, deform=3, **kw)
    u0, v0, i0 = (t.cpu().numpy() for t in off.run(A, B))
    u3, v3, i3 = (t.cpu().numpy() for t in on.run(A, B))
    tu, tv = M.truth(H, W, 16, 8)
    for k in range(3):
        ok = (i0[k] == 0) & (i3[k] == 0)
        plain, share = M.rms_interior(u0[k], v0[k], tu, tv, ok)
        deformed, _ = M.rms_interior(u3[k], v3[k], tu, tv, ok)
        print(f"deform device accuracy, pair {k}: plain CWS {plain:.4f} px, deform=3 {deformed:.4f} px, "
              f"ratio {deformed / plain:.3f}, share {share:.4f}")
        assert share >= 0.95, (k, share)
        assert deformed <= 0.5 * plain, (k, deformed, plain)
    print(f"deform_ms {on.deform_ms():.3f} for 3 rounds of 3 pairs")
    off.close()
    on.close()


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


DEFORM = {"iterations": 2, "interp": "cubic", "smooth": True}
KW = dict(multipass=2, multipass_mode="CWS", scale=0.5, dt=2)


@pytest.fixture(scope="module")
def delivered(eng):
    """pair -> (u, v) as the EXISTING delivery gives them for a deforming plan: an object made without the keyword whose
    plan is replaced by a plan with it, so that the plan's run goes through the post-validation, flip and scaling as they
    are.  Also the same without deformation, to see that the option changes the values."""
    import torchpiv_amd as T
    A, B = scene_pairs(4, kind="uniform")           # (the wavy flow at this size loses a pair to "to many false vectors")
    plain_piv = T.ResidentPIV(A.cuda(), B.cuda(), 32, 16, **KW)
    plain = {o[0]: (_np(o[3]), _np(o[4])) for o in plain_piv.batched(4)}
    plain_piv.close()
    host = T.ResidentPIV(A.cuda(), B.cuda(), 32, 16, **KW)
    host._plan = eng.Plan(PH, PW, 32, 16, n_pass=2, mode="CWS", max_batch=4, device=host._device, precision="exact",
                          deform=DEFORM)
    want = {o[0]: (_np(o[3]), _np(o[4])) for o in host.batched(4)}
    assert host._plan.deform == DEFORM                       # the planted plan was the one that ran
    host.close()
    assert sorted(want) == sorted(plain) == [0, 1, 2, 3]
    assert any(not np.array_equal(want[i][0], plain[i][0], equal_nan=True) for i in want)
    return A, B, want


def _check(got, want):
    assert sorted(got) == sorted(want)
    for i, (u, v) in got.items():
        assert np.array_equal(_np(u), want[i][0], equal_nan=True) and np.array_equal(_np(v), want[i][1], equal_nan=True), i


def test_resident_paths_deliver_the_plan_fields(eng, delivered):
    import torchpiv_amd as T
    A, B, want = delivered
    res = T.ResidentPIV(A.cuda(), B.cuda(), 32, 16, deform=DEFORM, **KW)
    outs = list(res.batched(3))                     # two launches: 3 pairs, then 1
    assert all(len(o) == 5 for o in outs)
    _check({o[0]: (o[3], o[4]) for o in outs}, want)
    calls = list(res())
    assert all(len(o) == 4 for o in calls)
    _check({i: (o[2], o[3]) for i, o in zip(sorted(want), calls)}, want)
    res.device_out = True
    outs = list(res.batched(2))
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for o in outs for t in o[3:])
    _check({o[0]: (o[3], o[4]) for o in outs}, want)
    res.close()


def test_offline_paths_and_run_folder_deliver_the_plan_fields(eng, delivered, tmp_path):
    import torchpiv_amd as T
    from torchpiv_amd import runner
    A, B, want = delivered
    _write_folder(tmp_path, A, B)
    piv = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", 32, 16, deform=DEFORM, **KW)
    outs = list(piv.batched(3))
    assert all(len(o) == 5 for o in outs)
    _check({o[0]: (o[3], o[4]) for o in outs}, want)
    piv.device_out = True
    outs = list(piv.batched(4))
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for o in outs for t in o[3:])
    _check({o[0]: (o[3], o[4]) for o in outs}, want)
    piv.close()
    order = sorted(want)
    for call_batch in (32, 1):                      # through batched(), and the one-pair path
        p2 = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", 32, 16, deform=DEFORM, **KW)
        p2.call_batch = call_batch
        calls = list(p2())
        assert all(len(o) == 4 for o in calls) and len(calls) == len(order)
        _check({i: (o[2], o[3]) for i, o in zip(order, calls)}, want)
        p2.close()
    seen = {}
    table, done = runner.run_folder(str(tmp_path), "cuda:0", "bmp", 32, 16, multipass=2, multipass_mode="CWS", scale=0.5,
                                    dt=2, batch_size=3, deform=DEFORM,
                                    on_pair=lambda i, out: seen.__setitem__(i, (_np(out["Vx[m/s]"]).copy(), _np(out["Vy[m/s]"]).copy())))
    assert done == 4 and table is not None
    _check(seen, want)
