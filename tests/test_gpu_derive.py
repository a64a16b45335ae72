"""derive= on the device: tpiv_field_fit (fieldfit.hip) against the numpy model of tests/derive_model.py bit for bit,
its argument errors, engine.derive against the model's expressions, and the dict that closes every delivered tuple of
ResidentPIV / OfflinePIV / ensemble() / run_folder against engine.derive(engine.field_fit(...)) of that tuple's own
fields."""
import numpy as np
import pytest
import torch

import derive_model as M

pytestmark = pytest.mark.gpu

CASES = [(r, o) for r in (1, 2, 3) for o in (1, 2)]


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def _grids(eng):
    """(batch, rows, columns): the small grids, then three for the tile layout -- one column and one row past a tile (the
    seams in both directions, the halo crossing them), two tile columns and a bit at batch 3 (the batch stride), and two
    tile rows of a tile column that is one cell short."""
    tr, tc = eng.FIELD_FIT_TILE
    assert (tr, tc) == (8, 64)
    return [(1, 1, 1), (2, 1, 7), (2, 7, 1), (2, 2, 2), (2, 5, 5), (2, tr + 1, tc + 1), (3, 9, 2 * tc + 2), (2, 2 * tr, tc - 1)]


GRID_IDS = ["1x1", "1x7", "7x1", "2x2", "5x5", "seams", "batch3", "short_tile"]


def _field(shape, seed):
    """Noisy smooth fields that differ from pair to pair, with zeros of both signs and exact ties."""
    rng = np.random.default_rng(seed)
    B, R, C = shape
    r, c = np.mgrid[0:R, 0:C]
    k = np.arange(B).reshape(B, 1, 1)
    u = 2.0 + 0.05 * r * (k + 1) - 0.02 * c + rng.normal(0, 0.3, shape)
    v = -1.0 + 0.03 * c - 0.04 * r * (k + 1) + rng.normal(0, 0.3, shape)
    z = rng.random(shape) < 0.15
    u[z] = np.where(rng.random(int(z.sum())) < 0.5, 0.0, -0.0)
    z = rng.random(shape) < 0.15
    v[z] = np.where(rng.random(int(z.sum())) < 0.5, 0.0, -0.0)
    t = rng.random(shape) < 0.1
    u[t] = 2.5
    return u, v


def _same(eng, u, v, skip, radius, order):
    dev = [torch.from_numpy(a).cuda() for a in (u, v)] + [None if skip is None else torch.from_numpy(skip).cuda()]
    keep = [None if t is None else t.clone() for t in dev]
    fit, count, fitted = eng.field_fit(*dev, radius=radius, order=order)
    torch.cuda.synchronize()
    for t, k in zip(dev, keep):                                        # the inputs are not written
        assert t is None or t.view(torch.uint8).equal(k.view(torch.uint8))
    wfit, wcount, wfitted = M.field_fit(u, v, skip, radius, order)
    fit, count, fitted = fit.cpu().numpy(), count.cpu().numpy(), fitted.cpu().numpy()
    assert fit.dtype == np.float64 and count.dtype == np.uint8 and fitted.dtype == np.int8
    assert fit.shape == (6,) + u.shape and count.shape == u.shape and fitted.shape == u.shape
    assert count.tobytes() == wcount.tobytes(), np.argwhere(count != wcount)[:5]
    assert fitted.tobytes() == wfitted.tobytes(), np.argwhere(fitted != wfitted)[:5]
    assert fit.tobytes() == np.ascontiguousarray(wfit).tobytes(), \
        np.argwhere(fit.view(np.uint64) != np.ascontiguousarray(wfit).view(np.uint64))[:5]
    return wfit, wcount, wfitted


@pytest.mark.parametrize("grid", range(8), ids=GRID_IDS)
@pytest.mark.parametrize("radius,order", CASES)
def test_field_fit_equals_the_model_bit_for_bit(eng, radius, order, grid):
    shape = _grids(eng)[grid]
    u, v = _field(shape, seed=1000 * grid + 10 * radius + order)
    rng = np.random.default_rng(grid)
    seen = set()
    for density in (None, 0.0, 0.3, 0.7, 0.9, 1.0):
        skip = None if density is None else (rng.random(shape) < density).astype(np.uint8)
        if skip is not None and density > 0:
            skip[skip != 0] = rng.integers(1, 256, int((skip != 0).sum()))          # any non-zero byte skips
        _, count, fitted = _same(eng, u, v, skip, radius, order)
        seen |= set(np.unique(fitted).tolist())
        if density == 1.0:
            assert (fitted == -1).all() and (count == 0).all()
    # not finite in u only, in v only: such a cell is no data in either component
    bu, bv = u.copy(), v.copy()
    n = u.size
    at = rng.choice(n, size=min(n, max(2, n // 12)), replace=False)
    bu.reshape(-1)[at[0::2]] = rng.choice([np.nan, np.inf, -np.inf], size=at[0::2].size)
    bv.reshape(-1)[at[1::2]] = rng.choice([np.nan, np.inf, -np.inf], size=at[1::2].size)
    _, count, _ = _same(eng, bu, bv, None, radius, order)
    _same(eng, bu, bv, (rng.random(shape) < 0.3).astype(np.uint8), radius, order)
    assert count.reshape(-1)[at].max() <= (2 * radius + 1) ** 2 - 1 or n == 1
    if grid >= 5:
        assert {order, 0, -1} <= seen                                  # the case walks down the ladder


def test_pairs_of_a_batch_are_fitted_apart(eng):
    """The same pair in two places of a batch gives the same planes, and a 2-D call is the batch of one."""
    u, v = _field((3, 12, 70), seed=5)
    skip = (np.random.default_rng(5).random(u.shape) < 0.3).astype(np.uint8)
    u[2], v[2], skip[2] = u[0], v[0], skip[0]
    fit, count, fitted = _same(eng, u, v, skip, 2, 2)
    assert fit[:, 0].tobytes() == fit[:, 2].tobytes() and fit[:, 0].tobytes() != fit[:, 1].tobytes()
    one = eng.field_fit(torch.from_numpy(u[1]).cuda(), torch.from_numpy(v[1]).cuda(), torch.from_numpy(skip[1]).cuda())
    assert tuple(one[0].shape) == (6, 12, 70) and tuple(one[1].shape) == (12, 70) and tuple(one[2].shape) == (12, 70)
    assert one[0].cpu().numpy().tobytes() == np.ascontiguousarray(fit[:, 1]).tobytes()
    assert one[2].cpu().numpy().tobytes() == fitted[1].tobytes()


def test_arguments_and_aliasing(eng):
    from torchpiv_amd._lib import EINVAL, OK, lib
    u = torch.randn(2, 8, 8, dtype=torch.float64, device="cuda")
    v = torch.randn(2, 8, 8, dtype=torch.float64, device="cuda")
    skip = torch.zeros(2, 8, 8, dtype=torch.uint8, device="cuda")
    fit = torch.full((6, 2, 8, 8), 7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((2, 8, 8), 99, dtype=torch.uint8, device="cuda")
    ordr = torch.full((2, 8, 8), 99, dtype=torch.int8, device="cuda")
    keep = (u.clone(), v.clone())

    def call(*a):
        return lib.tpiv_field_fit(*a, 0)
    p = [t.data_ptr() for t in (u, v, skip, fit, cnt, ordr)]
    for args in ((p[0], p[1], p[2], 2, 8, 8, 0, 2, p[3], p[4], p[5]), (p[0], p[1], p[2], 2, 8, 8, 4, 2, p[3], p[4], p[5]),
                 (p[0], p[1], p[2], 2, 8, 8, 2, 0, p[3], p[4], p[5]), (p[0], p[1], p[2], 2, 8, 8, 2, 3, p[3], p[4], p[5]),
                 (p[0], p[1], p[2], 2, 0, 8, 2, 2, p[3], p[4], p[5]), (p[0], p[1], p[2], 2, 8, 0, 2, 2, p[3], p[4], p[5]),
                 (p[0], p[1], p[2], 2, 8, 8, 2, 2, p[0], p[4], p[5]),               # the planes over u
                 (p[0], p[1], p[2], 2, 8, 8, 2, 2, p[3], p[2], p[5]),               # the count over the skip bytes
                 (p[0], p[1], p[2], 2, 8, 8, 2, 2, p[3], p[4], p[4] + 64),          # two outputs overlap
                 (p[0], p[1], p[2], 2, 8, 8, 2, 2, p[3], p[3] + 8 * 700, p[5]),
                 (None, p[1], p[2], 2, 8, 8, 2, 2, p[3], p[4], p[5]), (p[0], p[1], p[2], 2, 8, 8, 2, 2, None, p[4], p[5])):
        assert call(*args) == EINVAL, args
    assert call(p[0], p[1], p[2], 0, 8, 8, 2, 2, p[3], p[4], p[5]) == OK            # batch 0: nothing to do
    torch.cuda.synchronize()
    # nothing was launched: the outputs are as they were, and so are the inputs
    assert (fit == 7.0).all() and (cnt == 99).all() and (ordr == 99).all()
    assert u.equal(keep[0]) and v.equal(keep[1])
    for bad in (dict(radius=0), dict(radius=4), dict(order=0), dict(order=3), dict(radius=True), dict(order=2.0)):
        with pytest.raises(ValueError):
            eng.field_fit(u, v, skip, **bad)
    with pytest.raises(TypeError):
        eng.field_fit(u.float(), v.float(), skip)
    with pytest.raises(TypeError):
        eng.field_fit(u, v, skip.bool())
    with pytest.raises(ValueError):
        eng.field_fit(u, v[:1], skip)
    with pytest.raises(ValueError):
        eng.field_fit(u[0, 0], v[0, 0])
    assert call(p[0], p[1], None, 2, 8, 8, 2, 2, p[3], p[4], p[5]) == OK            # skip is optional
    torch.cuda.synchronize()
    assert (ordr == 2).all() and (cnt[:, 2:6, 2:6] == 25).all() and u.equal(keep[0]) and v.equal(keep[1])


def test_derive_equals_the_model_expressions(eng):
    u, v = _field((2, 11, 70), seed=9)
    skip = (np.random.default_rng(9).random(u.shape) < 0.5).astype(np.uint8)
    fit = eng.field_fit(torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda(), torch.from_numpy(skip).cuda(), 1, 2)
    assert set(np.unique(fit[2].cpu().numpy()).tolist()) >= {0, 1, 2}          # NaN slopes and NaN planes are part of it
    planes = fit[0].cpu().numpy()
    for hx, hy in ((0.4, -0.4), (3.0, 7.0), (-1.7, 0.013)):
        got = eng.derive(fit, hx, hy)
        want = M.derive(planes, hx, hy)
        assert list(got) == list(eng.DERIVE_QUANTITIES) == list(want)
        for k in got:
            g, w = got[k].cpu().numpy(), want[k]
            assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)), k
            fin = np.isfinite(w)
            assert fin.any()
            if k == "swirl":       # the device's float64 square root is good to about an ulp, not correctly rounded
                assert (np.abs(g[fin] - w[fin]) <= 1e-14 * np.abs(w[fin])).all()
                assert (w[fin] > 0).any() and (w[fin] == 0).any()
            else:
                assert g[fin].tobytes() == w[fin].tobytes(), k
    sub = eng.derive(fit[0], 0.4, 0.4, ("q", "dudx"))
    assert list(sub) == ["q", "dudx"]
    for bad in (("q", "q"), "curl", ()):
        with pytest.raises(ValueError):
            eng.derive(fit, 0.4, 0.4, bad)
    with pytest.raises(ValueError):
        eng.derive(fit, 0.0, 0.4)
    with pytest.raises(ValueError):
        eng.derive(fit[0][:5], 0.4, 0.4)
    with pytest.raises(TypeError):
        eng.derive(fit[0].float(), 0.4, 0.4)


# ---------------------------------------------------------------------------------------------------------------------
# delivery
# ---------------------------------------------------------------------------------------------------------------------
PH, PW, NP = 96, 80, 6
NAMES = ("vorticity", "dudx", "swirl", "u_smooth", "q")
KW = dict(multipass=2, multipass_mode="CWS", scale=0.5, dt=2)


@pytest.fixture(scope="module")
def pairs():
    """Six pairs of synth's wavy flow; a square of noise in frame b makes a few vectors of the last pass (16 / 8) fail the
    peak ratio, so that no pair is dropped for having no invalid vector (at most 3 x 3 windows see it: a ring below a
    quarter of the 11 x 9 cells)."""
    from torchpiv_amd import synth
    A = torch.empty(NP, PH, PW, dtype=torch.uint8)
    B = torch.empty(NP, PH, PW, dtype=torch.uint8)
    for i in range(NP):
        A[i], B[i] = synth.make_pair(PH, PW, i, kind="wavy", noise=2.0)
    rng = np.random.default_rng(3)
    B[:, 40:54, 32:46] = torch.from_numpy(rng.integers(0, 256, (NP, 14, 14)).astype(np.uint8))
    return A, B


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _check_dict(eng, d, x, y, u, v, excluded, par, device=False):
    """d is engine.derive(engine.field_fit(...)) of the delivered u, v and excluded cells, NaN in the excluded cells."""
    par = eng.derive_arg(par)
    assert isinstance(d, dict) and list(d) == list(par["quantities"])
    for f in d.values():
        assert (isinstance(f, torch.Tensor) and f.is_cuda) if device else isinstance(f, np.ndarray)
    x, y, u, v = (_np(t) for t in (x, y, u, v))
    skip = None if excluded is None else torch.from_numpy(np.ascontiguousarray(excluded).astype(np.uint8)).cuda()
    fit = eng.field_fit(torch.from_numpy(np.ascontiguousarray(u)).cuda(), torch.from_numpy(np.ascontiguousarray(v)).cuda(),
                        skip, par["radius"], par["order"])
    want = eng.derive(fit, x[0, 1] - x[0, 0], y[1, 0] - y[0, 0], par["quantities"])
    for k, f in d.items():
        g, w = _np(f), want[k].cpu().numpy().copy()
        assert g.dtype == np.float64 and g.shape == u.shape
        if excluded is not None:
            w[excluded] = np.nan
            assert np.isnan(g[excluded]).all()
        assert np.array_equal(np.isnan(g), np.isnan(w)), k
        fin = np.isfinite(w)
        assert fin.mean() > 0.5 and g[fin].tobytes() == w[fin].tobytes(), k


def _plain(outs):
    return {o[0]: (o[3], o[4]) for o in outs}


def _same_fields(got, plain):
    assert sorted(got) == sorted(plain) and len(got) >= 3
    for i in got:
        for g, w in zip(got[i], plain[i]):
            assert _np(g).tobytes() == _np(w).tobytes(), i


def test_resident_paths(eng, pairs):
    import torchpiv_amd as T
    A, B = (t.cuda() for t in pairs)
    off = T.ResidentPIV(A, B, 32, 16, **KW)
    plain = _plain(off.batched(4))
    none = T.ResidentPIV(A, B, 32, 16, derive=None, **KW)
    outs = list(none.batched(4))
    assert all(len(o) == 5 for o in outs) and all(len(o) == 4 for o in none())
    _same_fields(_plain(outs), plain)
    off.close()
    none.close()
    res = T.ResidentPIV(A, B, 32, 16, derive=NAMES, **KW)
    outs = list(res.batched(4))                       # two launches: 4 pairs, then 2
    assert all(len(o) == 6 for o in outs)
    _same_fields(_plain(outs), plain)
    for o in outs:
        _check_dict(eng, o[5], o[1], o[2], o[3], o[4], None, NAMES)
    assert not np.array_equal(outs[0][5]["vorticity"], outs[1][5]["vorticity"])
    calls = list(res())
    assert all(len(o) == 5 for o in calls) and len(calls) == len(plain)
    for o in calls:
        _check_dict(eng, o[4], *o[:4], None, NAMES)
    res.device_out = True
    outs = list(res.batched(3))
    assert all(len(o) == 6 and o[3].is_cuda for o in outs)
    _same_fields(_plain(outs), plain)
    for o in outs:
        _check_dict(eng, o[5], o[1], o[2], o[3], o[4], None, NAMES, device=True)
    res.close()
    # another operator through the dict
    par = {"quantities": ("shear", "divergence"), "radius": 1, "order": 1}
    res = T.ResidentPIV(A, B, 32, 16, derive=par, **KW)
    outs = list(res.batched(6))
    for o in outs:
        _check_dict(eng, o[5], o[1], o[2], o[3], o[4], None, par)
    res.close()


def test_resident_with_mask_dynamic_mask_and_uncertainty(eng, pairs):
    import torchpiv_amd as T
    A, B = (t.cuda() for t in pairs)
    img = torch.zeros(PH, PW, dtype=torch.uint8)
    img[:, :22] = 1
    for device_out in (False, True):
        res = T.ResidentPIV(A, B, 32, 16, derive=NAMES, mask={"image": img, "fill": -5.0}, **KW)
        res.device_out = device_out
        grid = res.mask_grid()
        assert grid.any() and not grid.all()
        outs = list(res.batched(4))
        assert len(outs) >= 3
        for o in outs:
            assert (_np(o[3])[grid] == -5.0).all()
            _check_dict(eng, o[5], o[1], o[2], o[3], o[4], grid, NAMES, device=device_out)
            for f in o[5].values():
                assert np.array_equal(np.isnan(_np(f)), grid)                     # NaN exactly on mask_grid()
        res.close()
    # one mask per pair: a block that moves with the pair index
    masks = torch.zeros(NP, PH, PW, dtype=torch.uint8)
    for i in range(NP):
        masks[i, 8 * i:8 * i + 40, 50:] = 1
    for device_out in (False, True):
        res = T.ResidentPIV(A, B, 32, 16, derive=NAMES, dynamic_mask={"stack": masks, "fill": -5.0}, **KW)
        res.device_out = device_out
        outs = list(res.batched(4))
        assert len(outs) >= 3
        grids = []
        for o in outs:
            ex = (_np(o[3]) == -5.0) & (_np(o[4]) == -5.0)
            assert ex.any() and not ex.all()
            grids.append(ex)
            _check_dict(eng, o[5], o[1], o[2], o[3], o[4], ex, NAMES, device=device_out)
        assert any(not np.array_equal(grids[0], g) for g in grids[1:])
        res.close()
    res = T.ResidentPIV(A, B, 32, 16, derive=("q",), uncertainty="cs", **KW)
    ref = T.ResidentPIV(A, B, 32, 16, uncertainty="cs", **KW)
    want = {o[0]: o[3:] for o in ref.batched(4)}
    outs = list(res.batched(4))
    assert all(len(o) == 8 for o in outs) and sorted(o[0] for o in outs) == sorted(want)
    for o in outs:
        for g, w in zip(o[3:7], want[o[0]]):
            assert np.array_equal(g, w, equal_nan=True)
        _check_dict(eng, o[7], o[1], o[2], o[3], o[4], None, ("q",))               # d last, behind su, sv
    calls = list(res())
    assert all(len(o) == 7 and isinstance(o[6], dict) for o in calls)
    res.close()
    ref.close()


def _write_folder(path, A, B):
    from PIL import Image
    for i in range(A.shape[0]):
        Image.fromarray(A[i].numpy(), "L").save(path / f"image{i}_a.bmp")
        Image.fromarray(B[i].numpy(), "L").save(path / f"image{i}_b.bmp")


def test_file_paths_ensemble_run_folder_and_sharded(eng, pairs, tmp_path):
    import torchpiv_amd as T
    from torchpiv_amd import dist, runner
    A, B = pairs
    folder = tmp_path / "frames"
    folder.mkdir()
    _write_folder(folder, A, B)
    off = T.OfflinePIV(str(folder), "cuda:0", "bmp", 32, 16, **KW)
    plain = _plain(off.batched(4))
    off.close()
    piv = T.OfflinePIV(str(folder), "cuda:0", "bmp", 32, 16, derive=NAMES, **KW)
    outs = list(piv.batched(4))
    assert all(len(o) == 6 for o in outs)
    _same_fields(_plain(outs), plain)
    for o in outs:
        _check_dict(eng, o[5], o[1], o[2], o[3], o[4], None, NAMES)
    piv.call_batch = 1                                     # the one-pair path
    calls = list(piv())
    assert len(calls) == len(plain) and all(len(o) == 5 for o in calls)
    for o, i in zip(calls, sorted(plain)):
        assert o[2].tobytes() == plain[i][0].tobytes()
        _check_dict(eng, o[4], *o[:4], None, NAMES)
    with pytest.raises(ValueError, match="derive= is not gathered"):
        dist.run_sharded(piv)
    piv.close()
    # the one-pair path with a mask: the grid goes into the fit, NaN in its cells
    img = torch.zeros(PH, PW, dtype=torch.uint8)
    img[70:, :] = 1
    piv = T.OfflinePIV(str(folder), "cuda:0", "bmp", 32, 16, derive=("dvdy", "v_smooth"), mask={"image": img, "fill": 9.0}, **KW)
    piv.call_batch = 1
    grid = piv.mask_grid()
    calls = list(piv())
    assert len(calls) >= 3 and grid.any() and not grid.all()
    for o in calls:
        assert (o[2][grid] == 9.0).all()
        _check_dict(eng, o[4], *o[:4], grid, ("dvdy", "v_smooth"))
    piv.close()
    # ensemble(): one field, one dict
    res = T.ResidentPIV(A.cuda(), B.cuda(), 32, 16, derive=NAMES, **KW)
    ref = T.ResidentPIV(A.cuda(), B.cuda(), 32, 16, **KW)
    got, want = res.ensemble(), ref.ensemble()
    assert len(got) == 5 and len(want) == 4
    for g, w in zip(got[:4], want):
        assert g.tobytes() == w.tobytes()
    _check_dict(eng, got[4], *got[:4], None, NAMES)
    res.close()
    ref.close()
    # run_folder: two more planes in every stack, two more columns for on_pair, the same table
    seen = {}
    kw = dict(multipass=2, multipass_mode="CWS", scale=0.5, dt=2, batch_size=4, save_opt="Save all binary")
    table, done = runner.run_folder(str(folder), "cuda:0", "bmp", 32, 16, derive=("vorticity", "q"),
                                    save_dir=str(tmp_path / "with"), on_pair=lambda i, out: seen.update({i: out}), **kw)
    table0, done0 = runner.run_folder(str(folder), "cuda:0", "bmp", 32, 16, save_dir=str(tmp_path / "without"), **kw)
    assert done == done0 == len(plain) and list(table) == list(table0)
    for k in table:
        assert np.array_equal(table[k], table0[k], equal_nan=True), k
    assert sorted(seen) == sorted(plain)
    for i, out in seen.items():
        assert list(out) == list(runner.KEYS_PAIR) + ["vorticity[1/s]", "q[1/s^2]"]
        assert out["Vx[m/s]"].tobytes() == plain[i][0].tobytes()
        _check_dict(eng, {"vorticity": out["vorticity[1/s]"], "q": out["q[1/s^2]"]}, out["x[mm]"], out["y[mm]"],
                    out["Vx[m/s]"], out["Vy[m/s]"], None, ("vorticity", "q"))
    stacks = sorted((tmp_path / "with").glob("frames_pair*.npy"))
    stacks0 = sorted((tmp_path / "without").glob("frames_pair*.npy"))
    assert len(stacks) == len(stacks0) == len(plain)
    nr, nc = plain[sorted(plain)[0]][0].shape
    assert all(np.load(f).shape == (6, nr, nc) for f in stacks) and all(np.load(f).shape == (4, nr, nc) for f in stacks0)
    first = np.load(stacks[0])
    assert any(first[4].tobytes() == out["vorticity[1/s]"].tobytes() and first[5].tobytes() == out["q[1/s^2]"].tobytes()
               for out in seen.values())
