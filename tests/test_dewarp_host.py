"""Geometric rectification, the parts that need no GPU: the weight table, known answers of the numpy model the device
kernel is checked against (tests/dewarp_model.py) and its distance from unrounded float64 interpolation, the dewarp=
argument (engine.dewarp_arg), the map built from it (engine.dewarp_map), the fit from a dot target (engine.dewarp_fit),
the constructors that check the argument before any device is touched, and the new symbol in header, binding and library."""
import os
import re

import numpy as np
import pytest
import torch

import dewarp_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 72, 90


@pytest.fixture(scope="module")
def scene():
    s = M.scene(H, W)
    s.flags.writeable = False
    return s


@pytest.fixture(scope="module")
def rot():
    """(matrix, sx, sy, map) of the 7 degree rotation with perspective."""
    Hm = M.rotation_perspective(H, W)
    sx, sy = M.homography_coords(Hm, H, W)
    return Hm, sx, sy, M.quantize(sx, sy, H, W)


# ---------------------------------------------------------------------------------------------------------------------
# table
# ---------------------------------------------------------------------------------------------------------------------
def test_cubic_table():
    from torchpiv_amd.engine import dewarp_cubic_table
    T = M.cubic_table()
    assert T.dtype == np.int16 and T.shape == (256, 4)
    assert (T.astype(np.int64).sum(axis=1) == 1024).all()
    assert T[0].tolist() == [0, 1024, 0, 0]
    for f in range(1, 256):
        assert np.array_equal(T[f], T[256 - f][::-1]), f
    assert np.abs(T.astype(np.int64)).sum(axis=1).max() == 1280           # |acc| <= 255 * 1280^2 < 2^31
    assert 255 * 1280 ** 2 < 2 ** 31
    E = dewarp_cubic_table()
    assert E.dtype == np.int16 and np.array_equal(E, T)


# ---------------------------------------------------------------------------------------------------------------------
# model: known answers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_model_identity_and_integer_shift(scene, interp):
    x, y = M.grid(H, W)
    ident = M.quantize(x, y, H, W)
    assert not M.outside(ident).any()
    assert np.array_equal(M.dewarp(scene, ident, interp), scene)
    # source = output + (3, -2): the image moves by (-3, +2) and the rim that has no source carries fill
    m = M.quantize(x + 3, y - 2, H, W)
    got = M.dewarp(scene, m, interp, fill=9)
    want = np.full_like(scene, 9)
    want[:, 2:, :W - 3] = scene[:, :H - 2, 3:]
    assert np.array_equal(got, want)
    assert M.outside(m).sum() == 2 * W + 3 * (H - 2)


def test_model_outside_and_non_finite_deliver_fill(scene):
    from torchpiv_amd.engine import dewarp_outside
    x, y = M.grid(H, W)
    x, y = x.copy(), y.copy()
    x[3, 4], y[5, 6], x[7, 8], y[9, 10] = np.nan, np.inf, -np.inf, -0.01             # -0.01 * 256 + 0.5 < 0: outside
    x[11, 12], x[13, 14] = W - 1 + 0.002, W - 1 + 0.001                              # q = (W - 1) 256 + 1: outside; + 0: inside
    y[15, 16] = -0.001                                                                # floor(-0.256 + 0.5) = 0: inside
    m = M.quantize(x, y, H, W)
    out_px = np.zeros((H, W), bool)
    for rc in ((3, 4), (5, 6), (7, 8), (9, 10), (11, 12)):
        out_px[rc] = True
    assert np.array_equal(M.outside(m), out_px)
    assert (m[out_px] == -1).all() and (m[~out_px] >= 0).all()
    assert np.array_equal(dewarp_outside(m), out_px) and np.array_equal(dewarp_outside(torch.from_numpy(m)), out_px)
    want = scene.copy()
    want[:, out_px] = 200
    want[:, 13, 14], want[:, 15, 16] = scene[:, 13, W - 1], scene[:, 0, 16]         # the two that round onto the frame's edge
    for interp in ("linear", "cubic"):
        assert np.array_equal(M.dewarp(scene, m, interp, fill=200), want)


def test_model_offsets_form(scene, rot):
    flat = np.concatenate([np.zeros(5, np.uint8), scene[1].ravel(), scene[0].ravel()])
    off = [5 + H * W, 5, 5 + H * W]
    got = M.dewarp_offsets(flat, off, H, W, rot[3], "cubic", 3)
    assert np.array_equal(got, M.dewarp(scene[[0, 1, 0]], rot[3], "cubic", 3))


# ---------------------------------------------------------------------------------------------------------------------
# model against unrounded float64 interpolation
# ---------------------------------------------------------------------------------------------------------------------
def test_model_against_float64_interpolation(scene, rot):
    """Linear within 1.5 gray levels: the Q8 coordinate step moves a position by at most 1/512 px per axis, a bilinear
    surface of 8-bit samples has a slope of at most 255 per px and axis -- 255 * 2 / 512 -- plus 0.5 for the rounding.
    Cubic within 6: per axis the coordinate step times sum |w'| <= 3 and the other axis's sum |w| <= 1.25, 2 * 255 / 512 *
    3 * 1.25 = 3.7, plus the table rounding (four weights off by at most 1/2048 + the fix-up 1/1024 per axis, times 255
    * 1.25: below 1) and 0.5.  Seen: 1.19 and 1.32."""
    _, sx, sy, m = rot
    inside = ~M.outside(m)
    assert inside.sum() > 0.9 * H * W
    rows, cols = np.nonzero(~inside)
    assert rows.min() == 0 and rows.max() == H - 1 and cols.min() == 0 and cols.max() == W - 1      # outside on all four sides
    below, above = 0, 0
    for k in range(2):
        for interp, bound in (("linear", 1.5), ("cubic", 6.0)):
            ref = M.dewarp_float(scene[k], sx, sy, interp)
            got = M.dewarp(scene[k], m, interp).astype(np.float64)
            ok = inside & np.isfinite(ref)
            err = np.abs(got - np.clip(ref, 0, 255))[ok].max()
            print(f"frame {k} {interp}: max distance from float64 interpolation {err:.3f}")
            assert err <= bound, (k, interp, err)
        acc = M.accumulate(scene[k], m, "cubic")
        below += int((acc[inside] < 0).sum())
        above += int((((acc[inside] + (1 << 19)) >> 20) > 255).sum())
    assert below > 0 and above > 0, (below, above)             # the scene exercises the clamp on both sides


# ---------------------------------------------------------------------------------------------------------------------
# dewarp_arg, dewarp_map
# ---------------------------------------------------------------------------------------------------------------------
HM = M.rotation_perspective(H, W)
P3 = np.array([[44.0, 43.0, 1.5], [35.0, -1.0, 34.0]])
XY = M.grid(H, W)
GOOD = [{"homography": HM}, {"homography": HM.tolist(), "interp": "linear"}, {"homography": torch.from_numpy(HM), "fill": 255},
        {"poly": P3}, {"poly": np.zeros((2, 6)), "fill": np.int64(7)}, {"poly": np.zeros((2, 10), np.float32)},
        {"map": XY}, {"map": [XY[0].astype(np.float32), XY[1]], "interp": "cubic", "fill": 0}]
BAD = ["keystone", 3, HM, [HM], {}, {"interp": "cubic"}, {"homography": HM, "poly": P3}, {"homography": HM, "order": 2},
       {"homography": HM[:2]}, {"homography": np.zeros((3, 3))}, {"homography": HM * np.nan}, {"homography": "eye"},
       {"poly": np.zeros((2, 4))}, {"poly": np.zeros((3, 6))}, {"poly": np.zeros(6)}, {"poly": np.full((2, 3), np.inf)},
       {"map": XY[0]}, {"map": (XY[0], XY[1][:-1])}, {"map": (XY[0][0], XY[1][0])}, {"map": (XY[0], XY[1], XY[0])},
       {"homography": HM, "interp": "nearest"}, {"homography": HM, "interp": None}, {"homography": HM, "fill": 256},
       {"homography": HM, "fill": -1}, {"homography": HM, "fill": 1.5}, {"homography": HM, "fill": True}]


def test_dewarp_arg_accepts_and_normalises():
    from torchpiv_amd.engine import dewarp_arg
    assert dewarp_arg(None) is None
    for good in GOOD:
        got = dewarp_arg(good)
        assert len(got) == 3 and got["interp"] in ("cubic", "linear") and isinstance(got["fill"], int)
        form = [k for k in ("homography", "poly", "map") if k in got]
        assert len(form) == 1
        for a in (got[form[0]] if form[0] == "map" else [got[form[0]]]):
            assert isinstance(a, np.ndarray) and a.dtype == np.float64
        again = dewarp_arg(got)                                    # its own result passes
        assert again["interp"] == got["interp"] and again["fill"] == got["fill"]
    got = dewarp_arg({"homography": HM})
    assert (got["interp"], got["fill"]) == ("cubic", 0)


@pytest.mark.parametrize("k", range(len(BAD)))
def test_dewarp_arg_rejects(k):
    from torchpiv_amd.engine import dewarp_arg
    with pytest.raises(ValueError):
        dewarp_arg(BAD[k])


def test_dewarp_map_equals_the_models(rot):
    from torchpiv_amd.engine import dewarp_map, dewarp_outside
    m = dewarp_map({"homography": HM}, H, W)
    assert m.dtype == np.int32 and m.shape == (H, W, 2) and np.array_equal(m, rot[3])
    assert np.array_equal(dewarp_outside(m), M.outside(rot[3])) and M.outside(rot[3]).any()
    for K, (h, w) in ((3, (H, W)), (6, (33, 67)), (10, (9, 3))):
        rng = np.random.default_rng(K)
        P = np.zeros((2, K))
        P[0, :3], P[1, :3] = [(w - 1) / 2, (w - 1) / 2 * 1.04, 2.0], [(h - 1) / 2, -1.5, (h - 1) / 2 * 0.97]
        P[:, 3:] = rng.normal(0, 1.5, (2, K - 3))
        want = M.quantize(*M.poly_coords(P, h, w), h, w)
        assert np.array_equal(dewarp_map({"poly": P}, h, w), want), K
        assert 0 < M.outside(want).sum() < h * w, K
    # the term order: one coefficient at a time, against the polynomial written out
    x, y = M.grid(H, W)
    xn, yn = 2 * x / (W - 1) - 1, 2 * y / (H - 1) - 1
    terms = [1 + 0 * xn, xn, yn, xn ** 2, xn * yn, yn ** 2, xn ** 3, xn ** 2 * yn, xn * yn ** 2, yn ** 3]
    for k in range(10):
        P = np.zeros((2, 10))
        P[0, k], P[1, 0] = 40.0, 7.0
        want = M.quantize(40.0 * terms[k], np.full((H, W), 7.0), H, W)
        assert np.array_equal(dewarp_map({"poly": P}, H, W), want), k
    xs, ys = x * 0.9 + 2.25, y * 1.1 - 3.5
    xs[0, 0] = np.nan
    assert np.array_equal(dewarp_map({"map": (xs, ys)}, H, W), M.quantize(xs, ys, H, W))
    with pytest.raises(ValueError, match="shape"):
        dewarp_map({"map": (xs, ys)}, H, W + 1)


# ---------------------------------------------------------------------------------------------------------------------
# dewarp_fit
# ---------------------------------------------------------------------------------------------------------------------
def _dots(h, w):
    gx, gy = np.meshgrid(np.linspace(4, w - 5, 7), np.linspace(4, h - 5, 7))
    return np.column_stack([gx.ravel(), gy.ravel()])


def test_dewarp_fit_homography():
    from torchpiv_amd.engine import dewarp_coords, dewarp_fit
    h, w = 128, 160
    Hm = M.rotation_perspective(h, w, degrees=4.0, px=3e-4, py=2e-4)
    t = _dots(h, w)
    s = (Hm @ np.column_stack([t, np.ones(len(t))]).T).T
    s = s[:, :2] / s[:, 2:]
    fit = dewarp_fit(t, s)                                        # "homography" is the default kind
    assert sorted(fit) == ["homography"] and fit["homography"].shape == (3, 3)
    sx, sy = dewarp_coords(fit, h, w)
    tx, ty = M.homography_coords(Hm, h, w)
    assert max(np.abs(sx - tx).max(), np.abs(sy - ty).max()) < 1e-6
    with pytest.raises(ValueError, match="at least 4"):
        dewarp_fit(t[:3], s[:3], "homography")
    with pytest.raises(ValueError):
        dewarp_fit(np.column_stack([np.arange(6.0), np.arange(6.0)]), s[:6], "homography")        # collinear


def test_dewarp_fit_polynomial():
    from torchpiv_amd.engine import dewarp_coords, dewarp_fit
    h, w = 128, 160
    rng = np.random.default_rng(3)
    P = np.zeros((2, 10))
    P[0, :3], P[1, :3] = [(w - 1) / 2, (w - 1) / 2, 1.0], [(h - 1) / 2, -2.0, (h - 1) / 2]
    P[:, 3:] = rng.normal(0, 2.0, (2, 7))
    t = _dots(h, w)
    xn, yn = M.normalised(t[:, 0], t[:, 1], h, w)
    A = np.stack(M.poly_terms(xn, yn, 10), axis=1)
    s = A @ P.T
    fit = dewarp_fit(t, s, "poly3", shape=(h, w))
    assert sorted(fit) == ["poly"] and fit["poly"].shape == (2, 10)
    sx, sy = dewarp_coords(fit, h, w)
    tx, ty = M.poly_coords(P, h, w)
    assert max(np.abs(sx - tx).max(), np.abs(sy - ty).max()) < 1e-6
    for kind, K in (("poly1", 3), ("poly2", 6)):                  # a lower order fits its own truth
        fit = dewarp_fit(t, A[:, :K] @ P[:, :K].T, kind, shape=(h, w))
        assert fit["poly"].shape == (2, K) and np.abs(fit["poly"] - P[:, :K]).max() < 1e-8
    for kind, K in (("poly1", 3), ("poly2", 6), ("poly3", 10)):
        with pytest.raises(ValueError, match=f"at least {K}"):
            dewarp_fit(t[:K - 1], s[:K - 1], kind, shape=(h, w))
    with pytest.raises(ValueError, match="shape"):
        dewarp_fit(t, s, "poly2")
    with pytest.raises(ValueError):
        dewarp_fit(t, s, "spline")
    with pytest.raises(ValueError):
        dewarp_fit(t, s[:-1])


# ---------------------------------------------------------------------------------------------------------------------
# API surface
# ---------------------------------------------------------------------------------------------------------------------
def test_constructors_check_dewarp_before_any_device(tmp_path):
    """A bad dewarp= raises ValueError in OfflinePIV, run_folder and ResidentPIV on a machine without a GPU; a good one on
    an empty folder gives an empty run.  A "map" of another shape than the frames raises where mask= does."""
    import torchpiv_amd as T
    from torchpiv_amd import runner
    f = torch.zeros(2, H, W, dtype=torch.uint8)
    for bad in (BAD[0], BAD[4], BAD[6], BAD[7], BAD[9], BAD[12], BAD[16], BAD[20], BAD[22]):
        with pytest.raises(ValueError):
            T.OfflinePIV(str(tmp_path), "cpu", "bmp", 32, 16, dewarp=bad)
        with pytest.raises(ValueError):
            runner.run_folder(str(tmp_path), "cpu", "bmp", 32, 16, dewarp=bad)
        with pytest.raises(ValueError):
            T.ResidentPIV(f, f, 32, 16, dewarp=bad)
    for good in (GOOD[0], GOOD[3], GOOD[6]):
        piv = T.OfflinePIV(str(tmp_path), "cpu", "bmp", 32, 16, dewarp=good)
        assert len(piv) == 0 and list(piv()) == [] and piv.dewarp_outside() is None and piv._dw_frames is None
        assert runner.run_folder(str(tmp_path), "cpu", "bmp", 32, 16, dewarp=good) == (None, 0)
    assert T.OfflinePIV(str(tmp_path), "cpu", "bmp", 32, 16).dewarp_outside() is None
    other = M.grid(H, W - 2)
    with pytest.raises(ValueError, match="shape"):
        T.ResidentPIV(f, f, 32, 16, dewarp={"map": other})
    from PIL import Image
    for name in ("image0_a.bmp", "image0_b.bmp"):
        Image.fromarray(np.zeros((H, W), np.uint8), "L").save(tmp_path / name)
    with pytest.raises(ValueError, match="shape"):
        T.OfflinePIV(str(tmp_path), "cpu", "bmp", 32, 16, dewarp={"map": other})
    with pytest.raises(ValueError, match="shape"):
        runner.run_folder(str(tmp_path), "cpu", "bmp", 32, 16, dewarp={"map": other})


def test_dewarp_symbol_in_header_binding_and_library():
    from torchpiv_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "torchpiv_hip.h")).read()
    assert re.search(r"\bint\s+tpiv_dewarp\s*\(", hdr)
    assert "tpiv_dewarp" in _lib.SIGNATURES and hasattr(_lib.lib, "tpiv_dewarp") and len(_lib.SIGNATURES["tpiv_dewarp"][1]) == 11
    assert _lib.DEWARP_INTERPS == {"linear": 0, "cubic": 1}
    assert re.search(r"#define\s+TPIV_DEWARP_LINEAR\s+0\b", hdr) and re.search(r"#define\s+TPIV_DEWARP_CUBIC\s+1\b", hdr)
