"""StereoPIV, the parts that need no GPU: the camera geometry of engine.stereo_* against the exact pinhole of
tests/stereo_model.py, the numpy model of the reconstruction against np.linalg.lstsq and its error propagation against a
Monte-Carlo, the status codes and the per-pair summary, the refusals of the class, and the new symbol in the header, the
binding and the library.

LSTSQ_GATE is 4 x the worst figure measured with this file (python tests/test_stereo_host.py prints it;
profiles/stereo/README.md has the record): the model and lstsq solve the same 4 x 3 systems by different eliminations, so
their distance is rounding, not method."""
import os
import re

import numpy as np
import pytest

import stereo_model as M
from torchpiv_amd.engine import stereo_fit          # the model is the yardstick of this feature: no feature, no tests

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# measured: 7.26e-15 (U, V, W and res of the model against lstsq, relative to the largest of |u1|, |v1|, |u2|, |v2| of the
# cell over min(1, |da|): the condition of W)
LSTSQ_GATE = 4 * 7.26e-15


# ---- calibration ---------------------------------------------------------------------------------------------------------

def _target(P, noise=0.0):
    """A two-plane 7 x 7 dot target (z = 0 and z = 2 mm, 2.5 mm pitch) and where camera P sees it."""
    g = (np.arange(7) - 3) * 2.5
    X, Y, Z = (q.ravel() for q in np.meshgrid(g, g * 0.8, np.array([0.0, 2.0]), indexing="ij"))
    world = np.stack([X, Y, Z], axis=1)
    x, y = M.project(P, X, Y, Z)
    return world, np.stack([x, y], axis=1) + noise


@pytest.mark.parametrize("cam", [0, 1])
def test_calibration_round_trip(cam):
    from torchpiv_amd import engine
    P = M.cameras()[cam]
    world, image = _target(P)
    got = engine.stereo_fit(world, image)
    assert got.shape == (3, 4) and got.dtype == np.float64
    # re-projection over the frame: the world points that the rectified frame's pixels stand for, and off the sheet
    y, x = np.mgrid[0:M.H:9, 0:M.W:9]
    X, Y = M.ORIGIN[0] + M.SCALE * x, M.ORIGIN[1] - M.SCALE * y
    worst = 0.0
    for z in (-1.0, 0.0, 2.0):
        wx, wy = M.project(P, X, Y, z)
        gx, gy = M.project(got, X, Y, z)
        worst = max(worst, np.abs(gx - wx).max(), np.abs(gy - wy).max())
    print(f"camera {cam + 1}: re-projection error {worst:.3e} px")
    assert worst <= 1e-6
    # the sign: positive depth at the target, the third row a unit vector, the centre where the model put it
    depth = got[2, :3] @ world.T + got[2, 3]
    assert (depth > 0).all() and abs(np.linalg.norm(got[2, :3]) - 1.0) < 1e-12
    assert np.allclose(engine.stereo_centre(got), M.centre(P), rtol=0, atol=1e-5)
    assert np.allclose(depth, P[2, :3] @ world.T + P[2, 3], rtol=0, atol=1e-5)


def test_calibration_refusals():
    from torchpiv_amd import engine
    world, image = _target(M.cameras()[0])
    with pytest.raises(ValueError, match="at least 6 points"):
        engine.stereo_fit(world[:5], image[:5])
    bad = world.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        engine.stereo_fit(bad, image)
    bad = image.copy()
    bad[0, 0] = np.inf
    with pytest.raises(ValueError, match="finite"):
        engine.stereo_fit(world, bad)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        engine.stereo_fit(world[:, :2], image)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        engine.stereo_fit(world, image[:-1])
    flat = world[:, 2] == 0.0                                         # one plane of the target: 49 coplanar points
    with pytest.raises(ValueError, match="do not determine a camera"):
        engine.stereo_fit(world[flat], image[flat])
    tilted = world[flat].copy()                                       # coplanar in a plane that is not z = const
    tilted[:, 2] = 0.3 * tilted[:, 0] - 0.2 * tilted[:, 1] + 1.0
    x, y = M.project(M.cameras()[0], *tilted.T)
    with pytest.raises(ValueError, match="do not determine a camera"):
        engine.stereo_fit(tilted, np.stack([x, y], axis=1))
    with pytest.raises(ValueError, match="coincide"):
        engine.stereo_fit(np.ones((8, 3)), image[:8])
    # six points in general position are enough
    pick = [0, 13, 27, 48, 60, 97]
    got = engine.stereo_fit(world[pick], image[pick])
    assert np.allclose(engine.stereo_centre(got), M.centre(M.cameras()[0]), rtol=0, atol=1e-3)


# ---- homography and tangents ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cam", [0, 1])
def test_homography_takes_rectified_pixels_to_camera_pixels(cam):
    from torchpiv_amd import engine
    P = M.cameras()[cam]
    G = engine.stereo_homography(P, M.SCALE, M.ORIGIN)
    assert G.shape == (3, 3) and np.array_equal(G, M.homography(P, M.SCALE, M.ORIGIN))
    rng = np.random.default_rng(11)
    x, y = rng.uniform(0, M.W - 1, 500), rng.uniform(0, M.H - 1, 500)
    cx, cy = M.project(P, M.ORIGIN[0] + M.SCALE * x, M.ORIGIN[1] - M.SCALE * y, 0.0)
    # the inverse of the backward map applied to the P-projected world points gives their rectified pixels back
    h = np.linalg.solve(G, np.stack([cx, cy, np.ones_like(cx)]))
    assert np.abs(h[0] / h[2] - x).max() <= 1e-9 and np.abs(h[1] / h[2] - y).max() <= 1e-9
    # and through dewarp_map's float path: the source coordinates of every pixel are the projections of its world point
    sx, sy = engine.dewarp_coords({"homography": G}, M.H, M.W)
    yy, xx = np.mgrid[0:M.H, 0:M.W]
    wx, wy = M.project(P, M.ORIGIN[0] + M.SCALE * xx, M.ORIGIN[1] - M.SCALE * yy, 0.0)
    assert np.abs(sx - wx).max() <= 1e-9 and np.abs(sy - wy).max() <= 1e-9
    m = engine.dewarp_map({"homography": G}, M.H, M.W)
    inside = ~engine.dewarp_outside(m)
    assert inside.mean() > 0.9 and not inside.all()                   # the far corners of the sheet are not seen
    assert np.abs(m[..., 0][inside] / 256.0 - wx[inside]).max() <= 0.5 / 256 + 1e-9


@pytest.mark.parametrize("cam", [0, 1])
def test_tangents_are_the_first_order_of_the_pinhole(cam):
    from torchpiv_amd import engine
    P = M.cameras()[cam]
    rng = np.random.default_rng(5)
    X, Y = rng.uniform(-8, 8, 200), rng.uniform(-6, 6, 200)
    a, b = engine.stereo_tangents(P, X, Y)
    ma, mb = M.tangents(P, X, Y)
    assert np.abs(a - ma).max() < 1e-13 and np.abs(b - mb).max() < 1e-13       # (the centre by another elimination)
    assert (np.sign(a) == -np.sign(M.ANGLES[cam])).all() and abs(abs(a).mean() - np.tan(np.deg2rad(abs(M.ANGLES[cam])))) < 0.02
    x0, y0 = M.rectified(P, M.SCALE, M.ORIGIN, X, Y, 0.0)
    errs = []
    for dz in (0.4, 0.04, 0.004):
        x1, y1 = M.rectified(P, M.SCALE, M.ORIGIN, X, Y, dz)
        fa, fb = (x1 - x0) * M.SCALE / dz, -(y1 - y0) * M.SCALE / dz          # seen motion per mm of dZ: X right, Y up
        errs.append(max(np.abs(fa - a).max(), np.abs(fb - b).max()))
    print(f"camera {cam + 1}: finite difference minus tangent at dZ = 0.4, 0.04, 0.004 mm: {errs}")
    assert errs[0] > errs[1] > errs[2] and errs[1] < errs[0] / 5 and errs[2] < errs[1] / 5 and errs[2] < 1e-5
    # the rectification is what the model says it is: the camera pixel of the moved point, taken back through the map
    G = engine.stereo_homography(P, M.SCALE, M.ORIGIN)
    cx, cy = M.project(P, X, Y, 0.04)
    h = np.linalg.solve(G, np.stack([cx, cy, np.ones_like(cx)]))
    x1, y1 = M.rectified(P, M.SCALE, M.ORIGIN, X, Y, 0.04)
    assert np.abs(h[0] / h[2] - x1).max() < 1e-8 and np.abs(h[1] / h[2] - y1).max() < 1e-8


def test_tangents_refuse_a_camera_behind_the_sheet():
    from torchpiv_amd import engine
    P = M.pinhole(35.0)
    behind = P.copy()
    behind[:, 2] *= -1.0                                             # mirrored in the sheet: C_z < 0
    assert engine.stereo_centre(behind)[2] < 0
    with pytest.raises(ValueError, match="in front of the sheet"):
        engine.stereo_tangents(behind, 0.0, 0.0)
    inplane = M.pinhole(90.0)
    inplane[:, 3] = -inplane[:, :3] @ np.array([500.0, 0.0, -1e-6])  # the centre a nanometre behind z = 0
    with pytest.raises(ValueError, match="in front of the sheet"):
        engine.stereo_tangents(inplane, 0.0, 0.0)
    for bad in (np.zeros((3, 3)), np.full((3, 4), np.nan), "P"):
        with pytest.raises(ValueError, match=r"\[3, 4\]"):
            engine.stereo_tangents(bad, 0.0, 0.0)
    for scale in (0.0, -1.0, np.nan, np.inf, "1", None, True):
        with pytest.raises(ValueError, match="scale"):
            engine.stereo_homography(P, scale)
    with pytest.raises(ValueError, match="origin"):
        engine.stereo_homography(P, 0.1, (0.0, np.nan))
    with pytest.raises(ValueError, match="origin"):
        engine.stereo_homography(P, 0.1, 3.0)


def test_planes_flip_like_the_delivered_fields():
    from torchpiv_amd import engine
    # 5 rows x 8 columns of window centres on a frame whose world origin is far off its centre, camera off-centre too
    P = M.pinhole(35.0, centre_px=(20.0, 90.0))
    origin, scale = (-3.0, 7.5), 0.11
    xs, ys = 8.0 + 16.0 * np.arange(8), 8.0 + 16.0 * np.arange(5)
    x, y = np.meshgrid(xs, ys)
    a, b = engine.stereo_planes(P, x, y, scale, origin)
    assert a.shape == b.shape == (5, 8) and a.flags.c_contiguous and b.flags.c_contiguous and a.dtype == np.float64
    ma, mb = M.planes(P, x, y, scale, origin)
    assert np.abs(a - ma).max() < 1e-13 and np.abs(b - mb).max() < 1e-13
    C = M.centre(P)
    for r in range(5):
        for c in range(8):
            Xw, Yw = origin[0] + scale * xs[c], origin[1] - scale * ys[4 - r]        # delivered row r is window row 4 - r
            assert abs(a[r, c] - (Xw - C[0]) / C[2]) < 1e-13 and abs(b[r, c] - (Yw - C[1]) / C[2]) < 1e-13
    assert (np.diff(b, axis=0) > 0).all()                # Y grows with the delivered row index: up
    assert not np.array_equal(b, np.flip(b, axis=0))
    with pytest.raises(ValueError, match="one shape"):
        engine.stereo_planes(P, x, y[:-1], scale, origin)


# ---- the model of the reconstruction ---------------------------------------------------------------------------------------

def _geometries():
    """Three sets of tangent planes over a 6 x 7 grid: the model's cameras, a symmetric +-45 degree pair, and a pair that
    also differs in b (one camera above the sheet's axis)."""
    x, y = np.meshgrid(16.0 + 16.0 * np.arange(7), 16.0 + 16.0 * np.arange(6))
    out = [M.planes(P, x, y, M.SCALE, M.ORIGIN) for P in M.cameras()]
    sym = [M.planes(M.pinhole(t), x, y, M.SCALE, M.ORIGIN) for t in (45.0, -45.0)]
    P3 = M.pinhole(25.0)
    P3[:, 3] = -P3[:, :3] @ (M.centre(P3) + np.array([0.0, 150.0, 0.0]))
    return [(out[0], out[1]), (sym[0], sym[1]), (out[1], M.planes(P3, x, y, M.SCALE, M.ORIGIN))]


def lstsq_distance():
    rng = np.random.default_rng(20262)
    worst = 0.0
    cases = [(g1, g2, rng.normal(0, 300, (4, 3) + g1[0].shape)) for g1, g2 in _geometries()]
    a = rng.normal(0, 0.6, (4, 6, 7))                                     # random tangents too
    cases.append(((a[0], a[1]), (a[2], a[3]), rng.normal(0, 3, (4, 3, 6, 7))))
    for (a1, b1), (a2, b2), f in cases:
        rec = M.reconstruct(*f, a1, b1, a2, b2)
        assert (rec["status"] == 0).all()
        for k in range(f.shape[1]):
            for r in range(a1.shape[0]):
                for c in range(a1.shape[1]):
                    cell = [q[k, r, c] for q in f]
                    want = M.lstsq(*cell, a1[r, c], b1[r, c], a2[r, c], b2[r, c])
                    got = [rec[n][k, r, c] for n in ("U", "V", "W", "res")]
                    da = np.hypot(a1[r, c] - a2[r, c], b1[r, c] - b2[r, c])
                    size = np.abs(cell).max() / min(1.0, da)
                    worst = max(worst, max(abs(g - w) for g, w in zip(got, want)) / size)
    return worst


def test_model_agrees_with_lstsq():
    worst = lstsq_distance()
    print(f"model against lstsq: worst relative difference {worst:.3e} (gate {LSTSQ_GATE:.3e})")
    assert worst <= LSTSQ_GATE


@pytest.mark.parametrize("case", [0, 1, 2])
def test_sigma_formulas_against_monte_carlo(case):
    """The propagated sU, sV, sW of one cell against the scatter of the reconstruction of N = 2e5 noisy draws: the standard
    error of a standard deviation is sigma / sqrt(2 N); the gate is four of them."""
    N = 200000
    (a1, b1), (a2, b2) = _geometries()[case]
    r, c = ((0, 0), (5, 6), (2, 3))[case]
    planes = [np.full(N, q[r, c]) for q in (a1, b1, a2, b2)]
    sig = [(7.0, 5.0, 9.0, 4.0), (3.0, 3.0, 3.0, 3.0), (1.0, 12.0, 6.0, 2.0)][case]
    rng = np.random.default_rng(100 + case)
    truth = (120.0, -60.0, 90.0)
    clean = [truth[0] + planes[0] * truth[2], truth[1] + planes[1] * truth[2],
             truth[0] + planes[2] * truth[2], truth[1] + planes[3] * truth[2]]
    noisy = [q + rng.normal(0, s, N) for q, s in zip(clean, sig)]
    rec = M.reconstruct(*noisy, *planes, sigma=[np.full(N, s) for s in sig])
    for name, field, t in (("sU", "U", truth[0]), ("sV", "V", truth[1]), ("sW", "W", truth[2])):
        want = rec[name][0]
        assert np.all(rec[name] == want)
        got = rec[field].std()
        print(f"geometry {case}: {name} formula {want:.4f}, Monte-Carlo {got:.4f}, "
              f"relative difference {abs(got - want) / want:.2e} (gate {4 / np.sqrt(2 * N):.2e})")
        assert abs(got - want) <= 4.0 * want / np.sqrt(2.0 * N)
        assert abs(rec[field].mean() - t) <= 5.0 * want / np.sqrt(N)        # and the reconstruction is unbiased


def test_status_precedence_fill_and_summary():
    rng = np.random.default_rng(9)
    (a1, b1), (a2, b2) = _geometries()[0]
    a1, b1, a2, b2 = (q.copy() for q in (a1, b1, a2, b2))
    f = rng.normal(0, 100, (4, 3, 6, 7))
    sg = rng.uniform(1, 5, (4, 3, 6, 7))
    skip = np.zeros((6, 7), np.uint8)
    skip[0, :3] = (1, 7, 255)
    a1[0, 1] = np.nan                                   # skipped AND without geometry: skipped wins
    a2[1, 0], b2[1, 0] = a1[1, 0], b1[1, 0]              # g == 0
    b1[1, 1] = np.inf
    f[0, 0, 1, 0] = np.nan                               # no geometry AND no data: no geometry wins
    f[2, 1, 2, 2] = np.nan                               # no data, pair 1 only
    f[3, 2, 2, 3] = -np.inf
    f[1, 0, 0, 0] = np.nan                               # skipped AND no data: skipped wins
    sg[1, 0, 3, 3] = np.nan                              # a non-finite sigma takes the three sigmas only
    skip_all = np.ones((6, 7), np.uint8)
    rec = M.reconstruct(*f, a1, b1, a2, b2, sigma=list(sg), skip=skip, fill=-7.5)
    want = np.zeros((3, 6, 7), np.uint8)
    want[:, 0, :3] = 1
    want[:, 1, :2] = 3
    want[1, 2, 2] = want[2, 2, 3] = 2
    assert np.array_equal(rec["status"], want) and rec["status"].dtype == np.uint8
    for n in ("U", "V", "W"):
        assert (rec[n][want == 1] == -7.5).all() and np.isnan(rec[n][want >= 2]).all() and np.isfinite(rec[n][want == 0]).all()
    for n in ("res", "sU", "sV", "sW"):
        assert np.isnan(rec[n][want != 0]).all()
    assert np.isfinite(rec["res"][want == 0]).all() and np.isfinite(rec["U"][0, 3, 3])
    holes = np.isnan(rec["sU"]) & (want == 0)
    assert holes.sum() == 1 and holes[0, 3, 3] and np.isnan(rec["sV"][0, 3, 3]) and np.isnan(rec["sW"][0, 3, 3])
    assert rec["pair_count"].dtype == np.int32 and rec["pair_count"].tolist() == [42 - 5, 42 - 6, 42 - 6]
    for k in range(3):
        ok = want[k] == 0
        assert np.isclose(rec["pair_rms"][k], np.sqrt((rec["res"][k][ok] ** 2).mean()), rtol=1e-14, atol=0)
    rec = M.reconstruct(*f, a1, b1, a2, b2, skip=skip_all, fill=np.nan)
    assert (rec["status"] == 1).all() and rec["pair_count"].tolist() == [0, 0, 0] and np.isnan(rec["pair_rms"]).all()
    assert np.isnan(rec["U"]).all() and "sU" not in rec
    one = M.reconstruct(*f[:, 1], a1, b1, a2, b2, skip=skip)           # a single pair without the batch axis
    full = M.reconstruct(*f, a1, b1, a2, b2, skip=skip)
    assert one["U"].shape == (6, 7) and np.array_equal(one["W"], full["W"][1], equal_nan=True)
    assert one["pair_count"] == full["pair_count"][1] and one["pair_rms"] == full["pair_rms"][1]


# ---- the class's refusals (no GPU is touched before them) --------------------------------------------------------------------

def test_stereo_piv_refuses_before_any_gpu_call():
    import torch
    import torchpiv_amd as T
    P = M.cameras()
    fr = torch.zeros(2, 64, 96, dtype=torch.uint8)            # host tensors: anything that reached the GPU would raise otherwise
    cams = dict(cam1=(fr, fr), cam2=(fr, fr))
    ok = dict(P=P, wind_size=32, overlap=16, scale=0.1)
    for kw, text in (({"dewarp": {"homography": np.eye(3)}}, "dewarp="), ({"dynamic_mask": {"kind": "bright", "size": 5, "level": 9}},
                                                                         "dynamic_mask="), ({"derive": "vorticity"}, "derive=")):
        with pytest.raises(ValueError, match=text):
            T.StereoPIV(**cams, **ok, **kw)
    for scale in (0.0, -0.1, np.nan, np.inf):
        with pytest.raises(ValueError, match="scale"):
            T.StereoPIV(**cams, **dict(ok, scale=scale))
    behind = P[0].copy()
    behind[:, 2] *= -1.0
    for bad, text in (((P[0], behind), "camera 2.*in front of the sheet"), ((np.zeros((3, 3)), P[1]), r"camera 1.*\[3, 4\]"),
                      ((np.full((3, 4), np.inf), P[1]), r"camera 1.*\[3, 4\]"), (P[0], "P = ")):
        with pytest.raises(ValueError, match=text):
            T.StereoPIV(**cams, **dict(ok, P=bad))
    with pytest.raises(ValueError, match="frame shapes differ"):
        T.StereoPIV((fr, fr), (fr[:, :, :80], fr[:, :, :80]), **ok)
    with pytest.raises(ValueError, match="pair counts differ"):
        T.StereoPIV((fr, fr), (fr[:1], fr[:1]), **ok)
    with pytest.raises(ValueError, match="mask: image of shape"):
        T.StereoPIV(**cams, **ok, mask=np.zeros((64, 90), np.uint8))
    assert "StereoPIV" in dir(T)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------

def test_symbol_in_header_binding_and_library():
    from torchpiv_amd import _lib, engine
    hdr = open(os.path.join(ROOT, "include", "torchpiv_hip.h")).read()
    kern = open(os.path.join(ROOT, "torchpiv_amd", "csrc", "piv_kernels.h")).read()
    make = open(os.path.join(ROOT, "torchpiv_amd", "csrc", "Makefile")).read()
    assert re.search(r"\bint\s+tpiv_stereo_reconstruct\s*\(", hdr)
    assert "launch_stereo_reconstruct" in kern and re.search(r"KERNEL_UNITS = .*\bstereo\b", make)
    tile = re.search(r"STEREO_BLOCK_THREADS = (\d+), STEREO_BLOCK_PAIRS = (\d+), STEREO_SUM_THREADS = (\d+)", kern)
    assert (int(tile.group(1)), int(tile.group(2))) == engine.STEREO_BLOCK and int(tile.group(3)) == engine.STEREO_SUM_THREADS
    assert "tpiv_stereo_reconstruct" in _lib.SIGNATURES and hasattr(_lib.lib, "tpiv_stereo_reconstruct")
    assert len(_lib.SIGNATURES["tpiv_stereo_reconstruct"][1]) == 27
    declared = re.search(r"int tpiv_stereo_reconstruct\((.*?)\);", hdr, re.S).group(1)
    assert declared.count(",") + 1 == 27
    # argument errors are decided on the host, before any launch (the pointers are never followed): 16 cells, 2 pairs
    call = _lib.lib.tpiv_stereo_reconstruct
    M1 = 1 << 24
    base = dict(u1=1 * M1, v1=2 * M1, u2=3 * M1, v2=4 * M1, su1=5 * M1, sv1=6 * M1, su2=7 * M1, sv2=8 * M1, skip=9 * M1,
                a1=10 * M1, b1=11 * M1, a2=12 * M1, b2=13 * M1, batch=2, cells=16, fill=0.0, U=14 * M1, V=15 * M1, W=16 * M1,
                res=17 * M1, sU=18 * M1, sV=19 * M1, sW=20 * M1, status=21 * M1, rms=22 * M1, count=23 * M1)

    def rc(**change):
        a = dict(base, **change)
        return call(*a.values(), None)
    for k in ("u1", "v1", "u2", "v2", "a1", "b1", "a2", "b2", "U", "V", "W", "res", "status", "rms", "count", "sU", "sV", "sW"):
        assert rc(**{k: None}) == _lib.EINVAL, k
    assert rc(batch=-1) == _lib.EINVAL and rc(cells=0) == _lib.EINVAL and rc(cells=-4) == _lib.EINVAL
    for k in ("su1", "sv1", "su2", "sv2"):                            # a partial set of sigmas
        assert rc(**{k: None}) == _lib.EINVAL, k
    none = dict(su1=None, sv1=None, su2=None, sv2=None)
    assert rc(batch=0, **none, sU=None, sV=None, sW=None, skip=None) == _lib.OK     # nothing to do, nothing launched
    assert rc(batch=0) == _lib.OK
    assert rc(batch=1 << 11, cells=1 << 20) == _lib.EINVAL and rc(batch=1, cells=1 << 31) == _lib.EINVAL     # a stack too large
    assert rc(batch=600000, cells=1) == _lib.EUNSUPPORTED
    # an output that overlaps an input (fields 256 bytes, planes 128, skip 16), or another output
    assert rc(U=base["u1"] + 248) == _lib.EINVAL and rc(W=base["a2"] + 120) == _lib.EINVAL
    assert rc(status=base["skip"] + 15) == _lib.EINVAL and rc(sW=base["sv2"] - 248) == _lib.EINVAL
    assert rc(rms=base["v2"] + 250) == _lib.EINVAL and rc(count=base["b1"] - 4) == _lib.EINVAL
    assert rc(V=base["U"] + 8) == _lib.EINVAL and rc(res=base["W"] - 248) == _lib.EINVAL
    assert rc(status=base["sU"] + 255) == _lib.EINVAL and rc(count=base["rms"] + 15) == _lib.EINVAL
    assert rc(count=base["rms"] + 16, batch=0) == _lib.OK


if __name__ == "__main__":
    print(f"model against lstsq: worst relative difference {lstsq_distance():.3e}")
