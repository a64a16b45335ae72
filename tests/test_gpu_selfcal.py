"""Stereo self-calibration on the device: engine.stereo_triangulate (tpiv_stereo_triangulate, stereo.hip) against the numpy
model of tests/selfcal_model.py -- the points, the gap and the status bit for bit, the count equal and the nine sums bit for
bit as well (the model sums in the device's order: lane t of 1024 over its cells, then the halving tree) -- at cell counts
on both sides of the sums' lanes and of the two-cells-per-lane form, the refusals, and StereoPIV.self_calibrate end to end
on the model's scene: a sheet at z = 0.5 + 0.02 X - 0.015 Y mm that the calibration believes at z = 0.

The end-to-end gates are 1.5 x the worst of the CPU path's three seeds (tests/selfcal_model.py: HEIGHT_LEFT, D_LEFT; the
margin of test_gpu_stereo.py's physics gate, for the same reason: seed-to-seed scatter, the device differs from the CPU
path by ~1e-6 px)."""
import numpy as np
import pytest
import torch

import selfcal_model as S
import stereo_model as M

pytestmark = pytest.mark.gpu

POINTS = ("X", "Y", "Z", "gap")
MODEL = {"X": "Mx", "Y": "My", "Z": "Mz", "gap": "gap"}


@pytest.fixture(scope="module")
def eng():
    from torchpiv_amd import engine
    return engine


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _inputs(batch, cells, seed):
    """Disparities of a noisy tilted sheet at `cells` scattered cells, analytic (the two rectified positions' midpoint and
    difference), a few of them far off; NaN, +-inf in dx, dy and a cell without a position planted at fixed flat places."""
    rng = np.random.default_rng(seed)
    X, Y = rng.uniform(-8, 8, cells), rng.uniform(-6, 6, cells)
    pos = []
    for P in M.cameras():
        px, py = M.rectified(P, M.SCALE, M.ORIGIN, X[None], Y[None], S.sheet(X, Y)[None] + rng.normal(0, 0.02, (batch, cells)))
        pos.append((M.ORIGIN[0] + M.SCALE * px, M.ORIGIN[1] - M.SCALE * py))
    Xc, Yc = (pos[0][0][0] + pos[1][0][0]) / 2, (pos[0][1][0] + pos[1][1][0]) / 2           # item 0's midpoints are the cells
    dx, dy = pos[1][0] - pos[0][0], pos[1][1] - pos[0][1]
    dy += rng.normal(0, 0.002, dy.shape)                                 # the lines of sight miss each other a little
    n = batch * cells
    fx, fy = dx.reshape(-1), dy.reshape(-1)
    far = rng.random(n) < 0.05
    fx[far] += rng.normal(0, 0.3, int(far.sum()))
    fy[far] += rng.normal(0, 0.05, int(far.sum()))
    if cells > 1:
        for k, val in enumerate((np.nan, np.inf, -np.inf)):
            fx[(7 * k + 3) % n] = val
            fy[(7 * k + 5) % n] = val
        Xc[11 % cells] = np.nan
    skip = (rng.random(cells) < 0.15).astype(np.uint8) * rng.integers(1, 256, cells).astype(np.uint8)
    return dx, dy, Xc, Yc, skip


def _centres():
    return tuple(M.centre(P) for P in M.cameras())


CASES = {}


def _case(batch, cells):
    """The inputs and the model's results of one shape, made once: {(skip?, limits?): model}."""
    key = (batch, cells)
    if key not in CASES:
        dx, dy, X, Y, skip = _inputs(batch, cells, 1000 * batch + cells)
        C1, C2 = _centres()
        centre = (float(np.nanmean(X)), float(np.nanmean(Y)), 0.4)
        want = {}
        for with_skip in (False, True):
            for limits in (False, True):
                kw = dict(gap_max=0.004, plane=S.SHEET, tol=0.05) if limits else {}
                want[with_skip, limits] = (kw, S.triangulate(dx, dy, X, Y, C1, C2, skip=skip if with_skip else None,
                                                             centre=centre, **kw))
        CASES[key] = (dx, dy, X, Y, skip, centre, want)
    return CASES[key]


def _same(rec, want, points, label):
    if points:
        for name in POINTS:
            got = getattr(rec, name).cpu().numpy()
            same = _bits(got) == _bits(want[MODEL[name]])
            assert got.shape == want[MODEL[name]].shape and same.all(), \
                f"{label}: {name} differs from the model in {int((~same).sum())} cells, first at {tuple(np.argwhere(~same)[0])}"
    else:
        assert len(rec) == 3 and not hasattr(rec, "X")
    assert np.array_equal(rec.status.cpu().numpy(), want["status"]), label
    count, sums = rec.count.cpu().numpy(), rec.sums.cpu().numpy()
    assert count.dtype == np.int32 and np.array_equal(count, want["count"]), (label, count, want["count"])
    assert np.array_equal(_bits(sums), _bits(want["sums"])), (label, sums, want["sums"])


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("cells", [1, 63, 1025, 2050])
def test_triangulate_equals_the_model_bit_for_bit(eng, batch, cells):
    dx, dy, X, Y, skip, centre, want = _case(batch, cells)
    C1, C2 = _centres()
    dev = [torch.from_numpy(q).cuda() for q in (dx, dy, X, Y)]
    kd = torch.from_numpy(skip).cuda()
    keep = [q.clone() for q in dev + [kd]]
    seen = set()
    for (with_skip, limits), (kw, model) in want.items():
        for points in (True, False):
            label = f"batch {batch}, cells {cells}, skip {with_skip}, limits {limits}, points {points}"
            rec = eng.stereo_triangulate(*dev, C1, C2, skip=kd if with_skip else None, centre=centre, points=points, **kw)
            _same(rec, model, points, label)
        seen |= set(np.unique(model["status"]).tolist())
        if not limits:
            assert not ({4, 5} & set(np.unique(model["status"]).tolist()))       # infinite limits: no test
    torch.cuda.synchronize()
    for was, now in zip(keep, dev + [kd]):
        assert torch.equal(was.view(torch.uint8), now.view(torch.uint8)), "an input was written"
    if cells > 63:
        assert seen == {0, 1, 2, 3, 4, 5}


def test_unaligned_views_and_inputs_without_the_batch_axis(eng):
    """An even cell count whose planes are only 8-byte aligned takes the one-cell-per-lane form; an input without the batch
    axis comes back without it; a bool skip is a uint8 skip; a 2-D cell shape is kept."""
    dx, dy, X, Y, skip, centre, want = _case(3, 2050)
    C1, C2 = _centres()
    kw, model = want[True, True]
    off = []
    for q in (dx, dy, X, Y):
        big = torch.zeros(q.size + 1, dtype=torch.float64, device="cuda")
        big[1:] = torch.from_numpy(q.reshape(-1)).cuda()
        off.append(big[1:].view(q.shape))
        assert off[-1].data_ptr() % 16 == 8 and off[-1].is_contiguous()
    bigk = torch.zeros(2051, dtype=torch.uint8, device="cuda")
    bigk[1:] = torch.from_numpy(skip).cuda()
    rec = eng.stereo_triangulate(*off, C1, C2, skip=bigk[1:], centre=centre, **kw)
    _same(rec, model, True, "unaligned")
    flat = eng.stereo_triangulate(off[0][1], off[1][1], off[2], off[3], C1, C2, skip=bigk[1:] != 0, centre=centre, **kw)
    one = {k: q[1] for k, q in model.items()}
    _same(flat, one, True, "no batch axis")
    assert flat.X.shape == (2050,) and flat.count.dim() == 0 and flat.sums.shape == (9,) and flat[4] is flat.status
    grid = eng.stereo_triangulate(*[q.view(3, 41, 50) for q in off[:2]], *[q.view(41, 50) for q in off[2:]], C1, C2,
                                  skip=bigk[1:].view(41, 50), centre=centre, **kw)
    assert grid.Z.shape == (3, 41, 50) and torch.equal(grid.Z.view(-1).view(torch.int64), rec.Z.view(-1).view(torch.int64))
    assert torch.equal(grid.sums.view(torch.int64), rec.sums.view(torch.int64))
    with pytest.raises(ValueError, match="one shape"):
        eng.stereo_triangulate(off[0], off[1][:2], off[2], off[3], C1, C2)
    with pytest.raises(ValueError, match="skip"):
        eng.stereo_triangulate(*off, C1, C2, skip=bigk[:2050].view(41, 50))
    with pytest.raises(TypeError):
        eng.stereo_triangulate(off[0].float(), *off[1:], C1, C2)
    for bad in ({"gap_max": -1.0}, {"tol": np.nan}, {"plane": (0, 0)}, {"centre": None}):
        with pytest.raises(ValueError, match=next(iter(bad))):
            eng.stereo_triangulate(*off, C1, C2, **bad)


def test_refusals_launch_nothing():
    import ctypes as C
    from torchpiv_amd import _lib
    dx, dy, X, Y, skip, centre, _ = _case(3, 63)
    fd = [torch.from_numpy(q).cuda() for q in (dx, dy, X, Y)]
    kd = torch.from_numpy(skip).cuda()
    n = 3 * 63
    out = [torch.full((n,), 7.0, dtype=torch.float64, device="cuda") for _ in range(4)]
    status = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    count = torch.full((3,), 9, dtype=torch.int32, device="cuda")
    sums = torch.full((27,), 7.0, dtype=torch.float64, device="cuda")
    cams = (C.c_double * 6)(*np.concatenate(_centres()))
    three = (C.c_double * 3)(0.0, 0.0, 0.0)

    def call(fields=fd, skp=kd, batch=3, cells=63, cam=cams, gap_max=1.0, plane=three, tol=1.0, mid=three, outs=out,
             st=status, c=count, s=sums):
        ptr = lambda q: None if q is None else q.data_ptr()            # noqa: E731
        return _lib.lib.tpiv_stereo_triangulate(*[ptr(q) for q in fields], ptr(skp), batch, cells, cam, gap_max, plane, tol,
                                                mid, *[ptr(q) for q in outs], ptr(st), ptr(c), ptr(s), None)
    err = _lib.lib.tpiv_last_error
    assert call(fields=[None] + fd[1:]) == _lib.EINVAL and b"null pointer" in err()
    assert call(fields=fd[:3] + [None]) == _lib.EINVAL and call(cam=None) == _lib.EINVAL and call(plane=None) == _lib.EINVAL
    assert call(mid=None) == _lib.EINVAL and call(st=None) == _lib.EINVAL and call(c=None) == _lib.EINVAL
    assert call(s=None) == _lib.EINVAL and b"null pointer" in err()
    assert call(outs=out[:3] + [None]) == _lib.EINVAL and b"all four or not at all" in err()
    assert call(outs=[None] + out[1:]) == _lib.EINVAL
    assert call(batch=-1) == _lib.EINVAL and call(cells=0) == _lib.EINVAL and b"empty grid" in err()
    assert call(gap_max=-1.0) == _lib.EINVAL and b"gap_max" in err() and call(gap_max=float("nan")) == _lib.EINVAL
    assert call(tol=-1e-9) == _lib.EINVAL and b"tol" in err() and call(tol=float("nan")) == _lib.EINVAL
    assert call(outs=[fd[0]] + out[1:]) == _lib.EINVAL and b"aliases an input" in err()
    assert call(st=kd) == _lib.EINVAL and call(s=fd[2]) == _lib.EINVAL
    assert call(outs=[out[1]] + out[1:]) == _lib.EINVAL and b"two outputs overlap" in err()
    assert call(batch=1 << 27, cells=63) == _lib.EINVAL and b"too large" in err()
    assert call(batch=0) == _lib.OK and call(batch=0, outs=[None] * 4, skp=None) == _lib.OK
    torch.cuda.synchronize()
    assert all(bool((q == 7.0).all()) for q in out + [sums]) and bool((status == 9).all()) and bool((count == 9).all())
    assert call(gap_max=float("inf"), tol=float("inf")) == _lib.OK and call(outs=[None] * 4, skp=None) == _lib.OK
    torch.cuda.synchronize()
    assert not bool((status == 9).any()) and not bool((count == 9).any())


# ---------------------------------------------------------------------------------------------------------------------
# end to end on the model's scene
# ---------------------------------------------------------------------------------------------------------------------
SEED = 0


@pytest.fixture(scope="module")
def frames():
    return [torch.from_numpy(q).cuda() for q in S.scene(SEED, frame_b=True)]


def _stereo(frames, **kw):
    import torchpiv_amd as T
    return T.StereoPIV((frames[0], frames[1]), (frames[2], frames[3]), M.cameras(), S.WS, S.OV, scale=M.SCALE, origin=M.ORIGIN,
                       **kw)


def _fields(piv):
    return {o[0]: o[3:] for o in piv.batched(4)}


@pytest.fixture(scope="module")
def applied(frames):
    """One apply=True run, shared: (the object, the record, what the object was before)."""
    piv = _stereo(frames)
    before = {"P": piv.projections(), "planes": piv.planes(), "fields": _fields(piv), "stats": piv.stats}
    rec = piv.self_calibrate(batch_size=4)
    yield piv, rec, before
    piv.close()


def test_self_calibrate_finds_the_sheet(applied):
    from torchpiv_amd import get_coordinates
    piv, rec, before = applied
    for k, r in enumerate(rec["rounds"]):
        print(f"round {k + 1}: plane ({r['plane'][0]:+.5f}, {r['plane'][1]:+.6f}, {r['plane'][2]:+.6f}) rms {r['rms']:.5f} "
              f"count {r['count']} height {r['height']:.5f} gap {r['gap']:.5f} |d| {r['d']:.5f}")
    assert before["stats"]["delivered"] == 6
    st = piv.stats                                                      # reset by the run; read before anything else runs
    assert st["delivered"] == 0 and st["pair_rms"] == {}
    assert rec["converged"] and len(rec["rounds"]) <= 4
    assert abs(rec["rounds"][0]["plane"][0] - S.SHEET[0]) < 0.03       # round 1 stops 2 % short: the passes' bias
    x, y = get_coordinates((M.H, M.W), S.WS, S.OV)
    X, Y = S.cells(x, y)
    free = ~piv.cameras()[0].mask_grid()
    height = S.sheet_height(rec["T"], X, Y, free)
    R = rec["T"][:3, :3]
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-13 and abs(np.linalg.det(R) - 1) < 1e-13
    got = piv.projections()
    assert all(np.array_equal(a, b) for a, b in zip(got, rec["P"])) and not np.array_equal(got[0], before["P"][0])
    assert all(np.abs(P0 @ rec["T"] - P1).max() <= 1e-9 * np.abs(P1).max() for P0, P1 in zip(before["P"], got))
    assert not np.array_equal(piv.planes()[0][0], before["planes"][0][0])
    x2, y2, dx, dy = piv.disparity(batch_size=4)
    d = float(np.median(np.hypot(dx, dy)[free]))
    print(f"self-calibration: sheet height left {height:.6f} mm (gate {1.5 * S.HEIGHT_LEFT:.6f}), median |d| left {d:.6f} mm "
          f"(gate {1.5 * S.D_LEFT:.6f}), {int(free.sum())} cells, {len(rec['rounds'])} rounds")
    assert height <= 1.5 * S.HEIGHT_LEFT
    assert d <= 1.5 * S.D_LEFT
    after = _fields(piv)
    assert sorted(after) == list(range(6))
    for i, f in after.items():
        assert all(np.isfinite(q).all() for q in f[:3]), i
    assert piv.stats["delivered"] == 6 and sorted(piv.stats["pair_rms"]) == list(range(6))


def test_apply_false_leaves_the_object_as_it_was(applied, frames):
    _, rec, before = applied
    piv = _stereo(frames)
    got = piv.self_calibrate(batch_size=4, apply=False)
    assert got["converged"] == rec["converged"] and got["rounds"] == rec["rounds"]
    assert np.array_equal(_bits(got["T"]), _bits(rec["T"]))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got["P"], rec["P"]))
    assert all(np.array_equal(a, b) for a, b in zip(piv.projections(), before["P"]))
    for (a1, b1), (a2, b2) in zip(piv.planes(), before["planes"]):
        assert np.array_equal(_bits(a1), _bits(a2)) and np.array_equal(_bits(b1), _bits(b2))
    now = _fields(piv)
    assert sorted(now) == sorted(before["fields"])
    for i in now:
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(now[i], before["fields"][i])), i
    piv.close()


def test_a_subset_of_pairs_and_another_grid(frames):
    piv = _stereo(frames)
    x, y, dx, dy = piv.disparity(indices=[4, 1], wind_size=64, overlap=32)
    assert x.shape == y.shape == dx.shape == dy.shape == (3, 4) and abs(x[0, 1] - x[0, 0] - 32 * M.SCALE) < 1e-12
    rec = piv.self_calibrate(indices=[4, 1], iterations=1, wind_size=64, overlap=32, apply=False)
    assert len(rec["rounds"]) == 1 and 3 <= rec["rounds"][0]["count"] <= 12 and not rec["converged"]
    assert abs(rec["rounds"][0]["plane"][0] - S.SHEET[0]) < 0.05
    assert piv.planes()[0][0].shape == (7, 9)                           # the object's own grid is untouched
    with pytest.raises(RuntimeError, match="fewer than min_cells = 13"):
        piv.self_calibrate(indices=[4, 1], iterations=1, wind_size=64, overlap=32, apply=False, min_cells=13)
    with pytest.raises(ValueError, match="no pairs"):
        piv.self_calibrate(indices=[])
    piv.close()


def test_a_from_folders_object_refuses(tmp_path):
    from PIL import Image
    import torchpiv_amd as T
    fr = S.scene(SEED, pairs=1, frame_b=True)
    dirs = []
    for c in range(2):
        d = tmp_path / f"camera{c + 1}"
        d.mkdir()
        Image.fromarray(fr[2 * c][0], "L").save(d / "image0_a.bmp")
        Image.fromarray(fr[2 * c + 1][0], "L").save(d / "image0_b.bmp")
        dirs.append(str(d))
    files = T.StereoPIV.from_folders(dirs[0], dirs[1], "cuda:0", "bmp", M.cameras(), S.WS, S.OV, scale=M.SCALE, origin=M.ORIGIN)
    with pytest.raises(NotImplementedError, match="resident frames only"):
        files.self_calibrate()
    assert all(np.array_equal(a, b) for a, b in zip(files.projections(), M.cameras()))
    files.close()
