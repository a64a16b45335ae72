"""StereoPIV on the device: engine.stereo_reconstruct (tpiv_stereo_reconstruct, stereo.hip) against the numpy model of
tests/stereo_model.py bit for bit -- grids on both sides of a wavefront, of a workgroup (at one and at two cells per lane)
and of a workgroup's pairs, with and without sigmas and skip, with +-0, ties, NaN and +-inf in every field and in the
tangents --, the per-pair summary, the refusals, StereoPIV.batched against the model's reconstruction of what two separately
built ResidentPIV objects deliver, the folder form, a pair that one camera drops, and the physics: the prescribed (dX, dY,
dZ) of the model's scene, which camera 1 alone gets wrong by |a W|.

The scene is 128 x 160 with six pairs at 32/16, one pass.  The two-pass case runs 32/16 -> 16/8 CWS: 64/32 leaves three
rows of windows on 128 rows, and the predictor (like the reference's RectBivariateSpline) needs four."""
import numpy as np
import pytest
import torch

import dewarp_model as D
import stereo_model as M

pytestmark = pytest.mark.gpu

FIELDS = ("U", "V", "W", "res", "sU", "sV", "sW")


@pytest.fixture(scope="module")
def eng():
    from torchpiv_amd import engine
    return engine


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _inputs(batch, rows, cols, seed):
    """Fields, sigmas, tangent planes and skip with the special values planted at fixed flat positions (wrapped into the
    grid when it is smaller): +-0, exact ties u1 == u2 and v1 == v2, NaN and +-inf in each of the four fields, in the
    sigmas and in the tangents, and a cell whose two cameras share their tangents."""
    rng = np.random.default_rng(seed)
    cells = rows * cols
    f = rng.normal(0, 200, (4, batch, cells))
    s = rng.uniform(0.5, 20, (4, batch, cells))
    t = np.stack([rng.normal(-0.7, 0.02, cells), rng.normal(0, 0.02, cells), rng.normal(0.58, 0.02, cells),
                  rng.normal(0, 0.02, cells)])
    skip = (rng.random(cells) < 0.15).astype(np.uint8) * rng.integers(1, 256, cells).astype(np.uint8)
    n = batch * cells
    flat = f.reshape(4, n)
    at = iter(range(0, 10 ** 6))
    for k in range(4):
        for val in (0.0, -0.0, np.nan, np.inf, -np.inf):
            flat[k, (3 * next(at) + 1) % n] = val
    p = (3 * next(at) + 1) % n
    flat[0, p] = flat[2, p] = 17.25                                   # u1 == u2
    p = (3 * next(at) + 1) % n
    flat[1, p] = flat[3, p] = -3.5                                    # v1 == v2
    p = (3 * next(at) + 1) % n
    flat[:, p] = (1.0, -0.0, 1.0, 0.0)                                # both ties at once: du = dv = 0
    sflat = s.reshape(4, n)
    for k in range(4):
        for val in (np.nan, np.inf, 0.0):
            sflat[k, (3 * next(at) + 1) % n] = val
    for k in range(4):
        for j, val in enumerate((np.nan, np.inf, -np.inf, 0.0)):
            t[k, (5 * (4 * k + j) + 2) % cells] = val
    c = (5 * 16 + 2) % cells
    t[2, c], t[3, c] = t[0, c], t[1, c]                               # a1 == a2 and b1 == b2: g == 0
    shape = (batch, rows, cols)
    return ([q.reshape(shape) for q in f], [q.reshape(shape) for q in s], [q.reshape(rows, cols) for q in t],
            skip.reshape(rows, cols))


def _grids(eng):
    th, pairs = eng.STEREO_BLOCK
    assert (th, pairs) == (256, 8) and eng.STEREO_SUM_THREADS == 1024
    return [(1, 1, 1), (2, 1, 7), (2, 7, 1), (3, 5, 5),
            (2, 1, 63), (2, 5, 13), (2, 1, th - 1), (2, 1, th + 1),           # one cell per lane (odd cell counts)
            (2, 2, 63), (2, 2, 65), (2, 2, th - 1), (2, 2, th + 1),           # two cells per lane (even cell counts)
            (pairs - 1, 3, 3), (pairs + 1, 3, 3), (2 * pairs + 1, 2, 5),      # a workgroup's pairs
            (3, 9, 130), (3, 9, 131)]                                         # the summary's lanes take a second cell


def _dev(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _check(eng, f, s, t, skip, fill, label):
    fd, td = _dev(f), _dev(t)
    sd = None if s is None else _dev(s)
    kd = None if skip is None else torch.from_numpy(skip).cuda()
    keep = [q.clone() for q in fd + td + (sd or []) + ([kd] if kd is not None else [])]
    rec = eng.stereo_reconstruct(*fd, *td, sigma=sd, skip=kd, fill=fill)
    again = eng.stereo_reconstruct(*fd, *td, sigma=sd, skip=kd, fill=fill)
    torch.cuda.synchronize()
    for was, now in zip(keep, fd + td + (sd or []) + ([kd] if kd is not None else [])):
        assert torch.equal(was.view(torch.uint8), now.view(torch.uint8)), f"{label}: an input was written"
    want = M.reconstruct(*f, *t, sigma=s, skip=skip, fill=fill)
    assert len(rec) == (10 if s is not None else 7)
    for name in FIELDS[:4 if s is None else 7] + ("status",):
        got = getattr(rec, name).cpu().numpy()
        assert got.shape == want[name].shape and got.dtype == want[name].dtype, (label, name)
        same = _bits(got) == _bits(want[name])
        assert same.all(), f"{label}: {name} differs from the model in {int((~same).sum())} cells, first at " \
                           f"{tuple(np.argwhere(~same)[0])}: {got[~same][0]!r} against {want[name][~same][0]!r}"
    count, rms = rec.pair_count.cpu().numpy(), rec.pair_rms.cpu().numpy()
    assert count.dtype == np.int32 and np.array_equal(count, want["pair_count"]), (label, count, want["pair_count"])
    assert np.array_equal(np.isnan(rms), want["pair_count"] == 0), label
    live = want["pair_count"] > 0
    assert np.allclose(rms[live], want["pair_rms"][live], rtol=1e-12, atol=0), (label, rms, want["pair_rms"])
    for a, b in zip(rec, again):                                       # the same call, the same bytes
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"{label}: two calls differ"
    return want


@pytest.mark.parametrize("with_sigma", [False, True], ids=["fields", "sigmas"])
@pytest.mark.parametrize("with_skip", [False, True], ids=["all", "skip"])
def test_reconstruct_equals_the_model_bit_for_bit(eng, with_sigma, with_skip):
    seen = set()
    for k, (batch, rows, cols) in enumerate(_grids(eng)):
        f, s, t, skip = _inputs(batch, rows, cols, 100 + k)
        want = _check(eng, f, s if with_sigma else None, t, skip if with_skip else None, -2.5 if with_skip else 0.0,
                      f"grid {(batch, rows, cols)}")
        seen |= set(np.unique(want["status"]).tolist())
    assert seen == ({0, 1, 2, 3} if with_skip else {0, 2, 3})


def test_unaligned_and_flat_inputs(eng):
    """An even cell count whose planes are only 8-byte aligned takes the one-cell-per-lane form; a 2-D input comes back
    without the batch axis; a bool skip is a uint8 skip."""
    f, s, t, skip = _inputs(3, 6, 43, 7)
    n = 3 * 6 * 43
    big = [torch.zeros(n + 1, dtype=torch.float64, device="cuda") for _ in range(4)]
    fd = []
    for b, q in zip(big, f):
        b[1:] = torch.from_numpy(q.reshape(-1)).cuda()
        fd.append(b[1:].view(3, 6, 43))
        assert fd[-1].data_ptr() % 16 == 8 and fd[-1].is_contiguous()
    td, sd = _dev(t), _dev(s)
    kd = torch.from_numpy(skip != 0).cuda()
    rec = eng.stereo_reconstruct(*fd, *td, sigma=sd, skip=kd, fill=1.5)
    want = M.reconstruct(*f, *t, sigma=s, skip=skip, fill=1.5)
    for name in FIELDS + ("status",):
        assert np.array_equal(_bits(getattr(rec, name).cpu().numpy()), _bits(want[name])), name
    one = eng.stereo_reconstruct(*[q[1] for q in fd], *td, skip=kd)
    want = M.reconstruct(*[q[1] for q in f], *t, skip=skip)
    assert len(one) == 7 and one.U.shape == (6, 43) and one.pair_rms.dim() == 0 and int(one.pair_count) == want["pair_count"]
    for name in FIELDS[:4] + ("status",):
        assert np.array_equal(_bits(getattr(one, name).cpu().numpy()), _bits(want[name])), name
    assert one[0] is one.U and one[4] is one.status and not hasattr(one, "sU")
    # a strided view is gathered, not refused
    wide = torch.from_numpy(np.ascontiguousarray(np.repeat(f[0], 2, axis=2))).cuda()
    got = eng.stereo_reconstruct(wide[:, :, ::2], *fd[1:], *td)
    assert torch.equal(got.W.view(torch.int64), eng.stereo_reconstruct(*fd, *td).W.view(torch.int64))


def test_all_excluded_pair_and_summary_order(eng):
    f, s, t, skip = _inputs(3, 9, 130, 3)
    f[0][1] = np.nan                                                  # pair 1 has no data at all
    want = _check(eng, f, None, t, None, 0.0, "a pair without data")
    assert want["pair_count"][1] == 0 and want["pair_count"][0] > 1000
    skip = np.ones((9, 130), np.uint8)
    want = _check(eng, f, s, t, skip, np.nan, "everything skipped")
    assert (want["pair_count"] == 0).all()


def test_refusals_launch_nothing(eng):
    from torchpiv_amd import _lib
    f, s, t, skip = _inputs(2, 4, 6, 1)
    fd, sd, td, kd = _dev(f), _dev(s), _dev(t), torch.from_numpy(skip).cuda()
    with pytest.raises(ValueError, match="sigma takes the four"):
        eng.stereo_reconstruct(*fd, *td, sigma=sd[:3])
    with pytest.raises(TypeError):
        eng.stereo_reconstruct(fd[0].float(), *fd[1:], *td)
    with pytest.raises(TypeError):
        eng.stereo_reconstruct(*fd, *td, skip=kd.to(torch.int32))
    with pytest.raises(TypeError):
        eng.stereo_reconstruct(*fd, *[q.float() for q in td])
    with pytest.raises(ValueError, match="one shape"):
        eng.stereo_reconstruct(fd[0][:1], *fd[1:], *td)
    with pytest.raises(ValueError, match="one shape"):
        eng.stereo_reconstruct(*[q[0, 0] for q in fd], *td)
    with pytest.raises(ValueError, match="tangent planes and skip"):
        eng.stereo_reconstruct(*fd, td[0][:3], *td[1:])
    with pytest.raises(ValueError, match="tangent planes and skip"):
        eng.stereo_reconstruct(*fd, *td, skip=kd[:, :5])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eng.stereo_reconstruct(fd[0].cpu(), *fd[1:], *td)
    with pytest.raises(ValueError, match="fill"):
        eng.stereo_reconstruct(*fd, *td, fill="0")
    # the C entry with real device memory: every refusal returns its code and leaves the outputs as they were
    n = 2 * 24
    out = [torch.full((n,), 7.0, dtype=torch.float64, device="cuda") for _ in range(7)]
    status = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    rms = torch.full((2,), 7.0, dtype=torch.float64, device="cuda")
    count = torch.full((2,), 9, dtype=torch.int32, device="cuda")

    def call(fields=fd, sig=sd, skp=kd, tan=td, batch=2, cells=24, outs=out, st=status, r=rms, c=count):
        ptr = lambda q: None if q is None else q.data_ptr()            # noqa: E731
        return _lib.lib.tpiv_stereo_reconstruct(*[ptr(q) for q in fields], *[ptr(q) for q in sig], ptr(skp),
                                                *[ptr(q) for q in tan], batch, cells, 0.0, *[ptr(q) for q in outs], ptr(st),
                                                ptr(r), ptr(c), None)
    assert call(fields=[None] + fd[1:]) == _lib.EINVAL and call(tan=td[:3] + [None]) == _lib.EINVAL
    assert call(outs=out[:3] + [None] + out[4:]) == _lib.EINVAL and call(st=None) == _lib.EINVAL
    assert call(r=None) == _lib.EINVAL and call(c=None) == _lib.EINVAL
    assert call(batch=-1) == _lib.EINVAL and call(cells=0) == _lib.EINVAL
    assert call(sig=sd[:2] + [None, None]) == _lib.EINVAL and call(sig=[None] + sd[1:]) == _lib.EINVAL
    assert call(outs=out[:4] + [None] + out[5:]) == _lib.EINVAL            # the sigmas need their three outputs
    assert call(outs=[fd[0]] + out[1:]) == _lib.EINVAL and b"aliases an input" in _lib.lib.tpiv_last_error()
    assert call(outs=out[:2] + [td[1]] + out[3:]) == _lib.EINVAL
    assert call(outs=[out[1]] + out[1:]) == _lib.EINVAL and b"two outputs overlap" in _lib.lib.tpiv_last_error()
    assert call(batch=1 << 27, cells=24) == _lib.EINVAL and b"too large" in _lib.lib.tpiv_last_error()
    assert call(batch=0) == _lib.OK
    torch.cuda.synchronize()
    assert all(bool((q == 7.0).all()) for q in out + [rms]) and bool((status == 9).all()) and bool((count == 9).all())
    assert call() == _lib.OK and call(sig=[None] * 4, outs=out[:4] + [None] * 3, skp=None) == _lib.OK
    torch.cuda.synchronize()
    assert not bool((status == 9).any())


# ---------------------------------------------------------------------------------------------------------------------
# end to end on the model's scene
# ---------------------------------------------------------------------------------------------------------------------
WS, OV, SEED = 32, 16, 0
DROPPED = 2                     # the pair whose two frames camera 2 sees identical: no invalid vector, dropped by camera 2


@pytest.fixture(scope="module")
def scene():
    """The scene of seed 0 as numpy stacks (A1, B1, A2, B2); in `dropped` camera 2's frame b of pair DROPPED is its frame a."""
    fr = M.scene(SEED)
    B2 = fr[3].copy()
    B2[DROPPED] = fr[2][DROPPED]
    return {"plain": fr, "dropped": (fr[0], fr[1], fr[2], B2)}


def _unseen():
    maps = [D.quantize(*D.homography_coords(M.homography(P, M.SCALE, M.ORIGIN), M.H, M.W), M.H, M.W) for P in M.cameras()]
    return D.outside(maps[0]) | D.outside(maps[1])


def _caller_mask():
    m = np.zeros((M.H, M.W), np.uint8)
    m[:40, 100:] = 200                                                # a corner of the sheet that the caller excludes
    return m


def _separately(frames, mask, fill, **kw):
    """{pair: (x, y, u, v[, su, sv])} of two ResidentPIV objects built by hand: the model's homographies, one mask."""
    import torchpiv_amd as T
    out, grids = [], []
    for c, P in enumerate(M.cameras()):
        a, b = (torch.from_numpy(q).cuda() for q in frames[2 * c:2 * c + 2])
        piv = T.ResidentPIV(a, b, WS, OV, scale=M.SCALE, dewarp={"homography": M.homography(P, M.SCALE, M.ORIGIN)},
                            mask={"image": mask, "fill": fill}, **kw)
        out.append({o[0]: o[1:] for o in piv.batched(4)})
        grids.append(piv.mask_grid())
        piv.close()
    assert np.array_equal(grids[0], grids[1])
    return out[0], out[1], grids[0]


def _stereo(frames, **kw):
    import torchpiv_amd as T
    cams = [tuple(torch.from_numpy(q).cuda() for q in frames[2 * c:2 * c + 2]) for c in range(2)]
    return T.StereoPIV(cams[0], cams[1], M.cameras(), WS, OV, scale=M.SCALE, origin=M.ORIGIN, **kw)


def _compare(piv, got, one, two, grid, fill, sigma):
    planes = piv.planes()
    both = sorted(set(one) & set(two))
    assert sorted(got) == both
    for i in both:
        x, y = one[i][0], one[i][1]
        assert np.array_equal(got[i][0], x) and np.array_equal(got[i][1], y)
        sg = None if not sigma else (one[i][4], one[i][5], two[i][4], two[i][5])
        want = M.reconstruct(one[i][2], one[i][3], two[i][2], two[i][3], *planes[0], *planes[1], sigma=sg,
                             skip=grid.astype(np.uint8), fill=fill)
        names = FIELDS[:7 if sigma else 4]
        assert len(got[i]) == 2 + len(names)
        for name, field in zip(names, got[i][2:]):
            assert isinstance(field, np.ndarray) and np.array_equal(_bits(field), _bits(want[name])), (i, name)
    return both


def test_batched_one_pass_with_uncertainty(scene):
    frames = scene["plain"]
    piv = _stereo(frames, uncertainty="cs")
    got = {o[0]: o[1:] for o in piv.batched(4)}
    one, two, grid = _separately(frames, _unseen(), 0.0, uncertainty="cs")
    both = _compare(piv, got, one, two, grid, 0.0, True)
    assert both == list(range(6)) and not grid.any()        # (the unseen corners stay below half of any 32 x 32 window)
    st = piv.stats
    assert (st["delivered"], st["dropped_camera1_only"], st["dropped_camera2_only"], st["dropped_both"]) == (6, 0, 0, 0)
    assert sorted(st["pair_rms"]) == both and all(np.isfinite(v) and v > 0 for v in st["pair_rms"].values())
    nosigma = np.isnan(one[0][4]) | np.isnan(one[0][5]) | np.isnan(two[0][4]) | np.isnan(two[0][5])
    assert np.array_equal(np.isnan(got[0][6]), nosigma) and nosigma.any() and not nosigma.all()
    # the planes are the model's, at the window centres of the pass that delivers
    from torchpiv_amd import get_coordinates
    x, y = get_coordinates((M.H, M.W), WS, OV)
    for c, P in enumerate(M.cameras()):
        ma, mb = M.planes(P, x, y, M.SCALE, M.ORIGIN)
        assert np.abs(piv.planes()[c][0] - ma).max() < 1e-13 and np.abs(piv.planes()[c][1] - mb).max() < 1e-13
    # __call__ yields the same without the index; device_out yields tensors
    piv.device_out = True
    for k, out in enumerate(piv()):
        assert len(out) == 9 and all(isinstance(q, torch.Tensor) and q.is_cuda for q in out[2:])
        assert np.array_equal(_bits(out[4].cpu().numpy()), _bits(got[k][4]))
    piv.close()


def test_batched_two_passes_with_a_callers_mask(scene):
    frames = scene["plain"]
    mask = {"image": _caller_mask(), "fill": -9.0, "threshold": 0.25}
    piv = _stereo(frames, multipass=2, multipass_mode="CWS", mask=mask)
    got = {o[0]: o[1:] for o in piv.batched(3, indices=[5, 0, 1, 3])}
    import torchpiv_amd as T
    out, grids = [], []
    for c, P in enumerate(M.cameras()):
        a, b = (torch.from_numpy(q).cuda() for q in frames[2 * c:2 * c + 2])
        solo = T.ResidentPIV(a, b, WS, OV, multipass=2, multipass_mode="CWS", scale=M.SCALE,
                             dewarp={"homography": M.homography(P, M.SCALE, M.ORIGIN)},
                             mask=dict(mask, image=(_unseen() | (mask["image"] != 0))))
        out.append({o[0]: o[1:] for o in solo.batched(3, indices=[5, 0, 1, 3])})
        grids.append(solo.mask_grid())
        solo.close()
    both = _compare(piv, got, out[0], out[1], grids[0], -9.0, False)
    assert both == [0, 1, 3, 5] and got[0][2].shape == (15, 19)
    assert grids[0][-4:, -6:].all() and (got[5][4][grids[0]] == -9.0).all()       # the caller's corner, top right as delivered
    piv.close()


def test_a_pair_that_one_camera_drops_and_the_folder_form(scene, tmp_path):
    from PIL import Image
    frames = scene["dropped"]
    piv = _stereo(frames)
    got = {o[0]: o[1:] for o in piv.batched(4)}
    one, two, grid = _separately(frames, _unseen(), 0.0)
    assert DROPPED in one and DROPPED not in two
    both = _compare(piv, got, one, two, grid, 0.0, False)
    assert both == [0, 1, 3, 4, 5]
    st = piv.stats
    assert (st["delivered"], st["dropped_camera1_only"], st["dropped_camera2_only"], st["dropped_both"]) == (5, 0, 1, 0)
    assert piv.cameras()[1].stats["dropped_no_invalid"] == 1 and DROPPED not in st["pair_rms"]
    piv.close()
    dirs = []
    for c in range(2):
        d = tmp_path / f"camera{c + 1}"
        d.mkdir()
        for i in range(6):
            Image.fromarray(frames[2 * c][i], "L").save(d / f"image{i}_a.bmp")
            Image.fromarray(frames[2 * c + 1][i], "L").save(d / f"image{i}_b.bmp")
        dirs.append(str(d))
    import torchpiv_amd as T
    files = T.StereoPIV.from_folders(dirs[0], dirs[1], "cuda:0", "bmp", M.cameras(), WS, OV, scale=M.SCALE, origin=M.ORIGIN)
    assert len(files) == 6
    seen = {o[0]: o[1:] for o in files.batched(4)}
    assert sorted(seen) == both
    for i in both:
        for a, b in zip(seen[i], got[i]):
            assert np.array_equal(_bits(a), _bits(b)), i
    assert files.stats["dropped_camera2_only"] == 1
    files.close()


def test_physics_of_the_scene(scene):
    """Against the PRESCRIBED field: the rms errors of U, V, W over the non-excluded cells of the six pairs stay within 1.5 x
    the worst of the CPU path's three seeds (tests/stereo_model.py: PHYSICS_RMS -- the seed-to-seed scatter of the comparable
    dewarp scene is 7 %, a sign error is of the order |a W| = 175), and camera 1's own u misses U by more than three times
    that gate: the perspective error that the reconstruction removes."""
    from torchpiv_amd import get_coordinates
    frames = scene["plain"]
    piv = _stereo(frames)
    got = {o[0]: o[1:] for o in piv.batched(6)}
    grid = piv.cameras()[0].mask_grid()
    piv.close()
    one, _, grid2 = _separately(frames, _unseen(), 0.0)
    assert sorted(got) == list(range(6)) and np.array_equal(grid, grid2)
    x, y = get_coordinates((M.H, M.W), WS, OV)
    truth = [q * 1000.0 for q in M.truth(x, y)]                      # mm -> the delivered unit (scale / dt * 1000, dt = 1)
    keep = ~grid
    rms = [float(np.sqrt(np.mean([(got[i][2 + k] - truth[k])[keep] ** 2 for i in range(6)]))) for k in range(3)]
    cam1 = float(np.sqrt(np.mean([(one[i][2] - truth[0])[keep] ** 2 for i in range(6)])))
    gate = [1.5 * q for q in M.PHYSICS_RMS]
    print(f"stereo scene: rms error of U, V, W = {rms[0]:.3f}, {rms[1]:.3f}, {rms[2]:.3f} (gates {gate[0]:.3f}, {gate[1]:.3f}, "
          f"{gate[2]:.3f}) over {int(keep.sum())} cells x 6 pairs; camera 1's u against U: {cam1:.1f}")
    assert all(r <= g for r, g in zip(rms, gate))
    assert cam1 > 3.0 * gate[0]


def test_disparity_measures_where_the_sheet_lies():
    """The sheet at z0 = 0.5 mm instead of 0: the median dx over the non-excluded cells against (a2 - a1) z0 = 0.639 mm, within
    1.5 x the worst deviation of the CPU path's three seeds (tests/stereo_model.py: DISPARITY_DEVIATION, 0.012 mm -- the
    bias of the passes, not of the geometry; a wrong sign misses by 1.28 mm).  from_folders objects refuse."""
    fr = M.scene(SEED, z0=M.DISPARITY_Z0, thickness=M.DISPARITY_THICKNESS, holes=False)
    piv = _stereo(fr)
    x, y, dx, dy = piv.disparity(batch_size=4)
    (a1, b1), (a2, b2) = piv.planes()
    keep = ~piv.cameras()[0].mask_grid()
    some = piv.disparity(indices=[4, 1])
    piv.close()
    assert dx.shape == dy.shape == a1.shape == (7, 9) and some[2].shape == (7, 9)
    want = np.median(((a2 - a1) * M.DISPARITY_Z0)[keep])
    got, side = float(np.median(dx[keep])), float(np.median(dy[keep]))
    print(f"disparity: median dx {got:.5f} mm against {want:.5f} (gate {1.5 * M.DISPARITY_DEVIATION:.5f}), median dy {side:.5f} "
          f"against {np.median(((b2 - b1) * M.DISPARITY_Z0)[keep]):.6f}; two pairs only: {float(np.median(some[2][keep])):.5f}")
    assert abs(want - 0.63878) < 1e-4
    assert abs(got - want) <= 1.5 * M.DISPARITY_DEVIATION
    assert abs(float(np.median(some[2][keep])) - want) < 0.1 * want        # the same sheet from a third of the pairs
