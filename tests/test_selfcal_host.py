"""Stereo self-calibration, the parts that need no GPU: the numpy model of the triangulation (tests/selfcal_model.py) on
analytic disparities of a tilted sheet, engine.stereo_correct / stereo_plane / stereo_cells against the exact pinhole and
np.linalg.lstsq, trimming, the status codes and their precedence, the NaN written, the fixed-order sums against math.fsum,
the refusals of StereoPIV.self_calibrate and of disparity()'s grid keywords, and the new symbol in the header, the binding
and the library.

Bounds: float64 rounding at a 500 mm stand-off is ~1e-13 mm (observed: points 2e-13, projections 6e-14 px); the bounds
below leave the margin for other geometries that the feature's definition names."""
import math
import os
import re

import numpy as np
import pytest

import selfcal_model as S
import stereo_model as M
from torchpiv_amd.engine import stereo_cells, stereo_correct, stereo_plane, stereo_triangulate   # no feature, no tests

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_BITS = 0x7ff8000000000000


def _analytic(X, Y, Z, P=None):
    """(Xc, Yc, dx, dy) in mm of sheet points (X, Y, Z): the two rectified positions' midpoint and difference (2 - 1)."""
    P1, P2 = M.cameras() if P is None else P
    r = []
    for Pc in (P1, P2):
        px, py = M.rectified(Pc, M.SCALE, M.ORIGIN, X, Y, Z)
        r.append((M.ORIGIN[0] + M.SCALE * px, M.ORIGIN[1] - M.SCALE * py))
    return (r[0][0] + r[1][0]) / 2, (r[0][1] + r[1][1]) / 2, r[1][0] - r[0][0], r[1][1] - r[0][1]


def _centres(P=None):
    P1, P2 = M.cameras() if P is None else P
    return M.centre(P1), M.centre(P2)


def _grid63():
    from oracle import piv_oracle as O
    x, y = O.coordinates((M.H, M.W), S.WS, S.OV)
    X, Y = S.cells(x, y)
    assert X.shape == (7, 9)
    return x, y, X, Y


# ---- the triangulation on analytic disparities ----------------------------------------------------------------------------------

def test_analytic_disparities_return_the_sheet():
    rng = np.random.default_rng(11)
    X, Y = rng.uniform(-8, 8, 500), rng.uniform(-6, 6, 500)
    Z = S.sheet(X, Y)
    Xc, Yc, dx, dy = _analytic(X, Y, Z)
    assert abs(np.median(dx) - 0.639) < 0.03                       # 6.4 rectified pixels: the misregistration of the two views
    C1, C2 = _centres()
    centre = (float(Xc.mean()), float(Yc.mean()), 0.0)
    got = S.triangulate(dx, dy, Xc, Yc, C1, C2, centre=centre)
    err = max(np.abs(got["Mx"] - X).max(), np.abs(got["My"] - Y).max(), np.abs(got["Mz"] - Z).max())
    print(f"analytic: points within {err:.2e} mm, gap <= {got['gap'].max():.2e} mm")
    assert (got["status"] == 0).all() and got["count"] == 500
    assert err < 1e-9 and got["gap"].max() < 1e-9
    for fit in (S.plane, stereo_plane):
        c0, c1, c2, rms = fit(got["count"], got["sums"], centre)
        assert max(abs(c0 - S.SHEET[0]), abs(c1 - S.SHEET[1]), abs(c2 - S.SHEET[2])) < 1e-10 and rms < 1e-9, fit


def test_correct_puts_the_sheet_at_zero_and_keeps_the_projections():
    rng = np.random.default_rng(12)
    X, Y = rng.uniform(-8, 8, 200), rng.uniform(-6, 6, 200)
    old = np.stack([X, Y, S.sheet(X, Y), np.ones(200)])
    for P in M.cameras():
        P_new, T = stereo_correct(P, S.SHEET)
        R = T[:3, :3]
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1.0) < 1e-14
        assert np.array_equal(T[3], (0.0, 0.0, 0.0, 1.0)) and np.array_equal(T[:3, 3], (0.0, 0.0, S.SHEET[0]))
        n = np.array([-S.SHEET[1], -S.SHEET[2], 1.0])
        assert np.abs(R[:, 2] - n / np.linalg.norm(n)).max() < 1e-15 and abs(R[1, 0]) > 0 and abs(R[:, 0] @ R[:, 2]) < 1e-15
        ex = np.array([1.0, 0, 0]) - R[0, 2] * R[:, 2]
        assert np.abs(R[:, 0] - ex / np.linalg.norm(ex)).max() < 1e-15                # the old X axis, projected into the plane
        new = np.linalg.inv(T) @ old
        assert np.abs(new[2]).max() < 1e-10                                            # the sheet is z = 0 in the new frame
        a, b = M.project(P_new, new[0], new[1], new[2]), M.project(P, X, Y, old[2])
        assert max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max()) < 1e-9
        Pm, Tm = S.correct(P, S.SHEET)                                                 # the model builds the frame another way
        assert np.abs(Tm - T).max() < 1e-15 and np.abs(Pm - P_new).max() < 1e-9
        again, T2 = stereo_correct(P_new, (0.0, 0.0, 0.0))
        assert np.array_equal(T2, np.eye(4)) and np.abs(again - P_new).max() <= 1e-12 * np.abs(P_new).max()
    for bad in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)):
        with pytest.raises(ValueError, match="finite"):
            stereo_correct(M.cameras()[0], bad)
    with pytest.raises(ValueError, match="in front of the sheet"):
        stereo_correct(M.cameras()[0], (600.0, 0.0, 0.0))                              # a sheet behind the camera
    with pytest.raises(ValueError, match="three numbers"):
        stereo_correct(M.cameras()[0], (0.0, 0.0))


def test_cells_flip_like_the_delivered_fields():
    x, y, X, Y = _grid63()
    gx, gy = stereo_cells(x, y, M.SCALE, M.ORIGIN)
    assert np.array_equal(gx, X) and np.array_equal(gy, Y) and gx.flags.c_contiguous and gy.flags.c_contiguous
    assert gy[0, 0] < gy[-1, 0] and gx[0, 0] < gx[0, -1]          # delivered rows run upwards in Y
    with pytest.raises(ValueError, match="one shape"):
        stereo_cells(x, y[:3], M.SCALE, M.ORIGIN)
    with pytest.raises(ValueError, match="scale"):
        stereo_cells(x, y, 0.0, M.ORIGIN)


def test_plane_agrees_with_lstsq_and_refuses_what_is_no_plane():
    _, _, X, Y = _grid63()
    rng = np.random.default_rng(13)
    Z = S.sheet(X, Y) + rng.normal(0, 0.01, X.shape)
    centre = (float(X.mean()), float(Y.mean()), 0.25)
    x, y, z = X.ravel() - centre[0], Y.ravel() - centre[1], Z.ravel() - centre[2]
    sums = [math.fsum(q) for q in (x, y, z, x * x, x * y, y * y, x * z, y * z, z * z)]
    want, res = np.linalg.lstsq(np.column_stack([np.ones(63), X.ravel(), Y.ravel()]), Z.ravel(), rcond=None)[:2]
    for fit in (stereo_plane, S.plane):
        got = fit(63, sums, centre)
        rel = max(abs(g - w) / abs(w) for g, w in zip(got[:3], want))
        assert rel < 1e-10 and abs(got[3] - math.sqrt(res[0] / 63)) < 1e-10 * got[3], (fit, rel)
        with pytest.raises(ValueError):
            fit(2, [math.fsum(q[:2]) for q in (x, y, z, x * x, x * y, y * y, x * z, y * z, z * z)], centre)
        t = np.linspace(-1, 1, 9)                                   # nine cells on one line
        lx, ly, lz = 3 * t, -2 * t, 0.1 * t
        with pytest.raises(ValueError):
            fit(9, [math.fsum(q) for q in (lx, ly, lz, lx * lx, lx * ly, ly * ly, lx * lz, ly * lz, lz * lz)], (0, 0, 0))
    with pytest.raises(ValueError, match="finite"):
        stereo_plane(63, [np.nan] * 9)


def test_trimming_drops_exactly_the_planted_cells():
    _, _, X, Y = _grid63()
    Xc, Yc, dx, dy = _analytic(X, Y, S.sheet(X, Y))
    bad = [(1, 2), (2, 6), (3, 4), (5, 1), (5, 7)]
    for k, rc in enumerate(bad):
        dx[rc] += (3 if k % 2 == 0 else -3) * M.SCALE              # 3 px off
    C1, C2 = _centres()
    centre = (float(Xc.mean()), float(Yc.mean()), 0.0)
    first = S.triangulate(dx, dy, Xc, Yc, C1, C2, centre=centre)
    assert first["count"] == 63
    c0, c1, c2, rms = S.plane(63, first["sums"], centre)
    second = S.triangulate(dx, dy, Xc, Yc, C1, C2, plane=(c0, c1, c2), tol=3.0 * rms, centre=centre)
    assert sorted(map(tuple, np.argwhere(second["status"] == 5))) == bad and second["count"] == 58
    assert set(np.unique(second["status"])) == {0, 5} and np.isfinite(second["Mz"]).all()      # status 5 keeps its point
    skip = np.zeros(X.shape, np.uint8)
    for rc in bad:
        skip[rc] = 1
    clean = S.triangulate(dx, dy, Xc, Yc, C1, C2, skip=skip, centre=centre)
    for fit in (S.plane, stereo_plane):
        a, b = fit(58, second["sums"], centre), fit(58, clean["sums"], centre)
        assert np.array_equal(second["sums"], clean["sums"]) and a == b
        assert max(abs(a[0] - S.SHEET[0]), abs(a[1] - S.SHEET[1]), abs(a[2] - S.SHEET[2])) < 1e-10


# ---- status, NaN, sums ---------------------------------------------------------------------------------------------------------

def test_status_precedence_and_the_nan_written():
    C1, C2 = np.array([100.0, 0.0, 400.0]), np.array([-100.0, 0.0, 400.0])
    X = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, np.nan])
    Y = np.zeros(8)
    z = 40.0                                                        # a point at height z shows dx = 200 z / (400 - z)
    d = 200.0 * z / (400.0 - z)
    #     0: fine  1: skipped  2: dx NaN  3: parallel  4: gap  5: off the plane  6: skipped AND NaN  7: no cell position
    dx = np.array([d, d, np.nan, -200.0, d, d + 3.0, np.inf, d])
    dy = np.array([0.0, 0.0, 0.0, 0.0, 2.0, 0.0, np.nan, 0.0])
    skip = np.array([0, 1, 0, 0, 0, 0, 255, 0], np.uint8)
    got = S.triangulate(dx, dy, X, Y, C1, C2, skip=skip, gap_max=0.5, plane=(z, 0.0, 0.0), tol=0.25)
    assert got["status"].tolist() == [0, 1, 2, 3, 4, 5, 1, 3] and got["count"] == 1
    assert abs(got["Mz"][0] - z) < 1e-12 and abs(got["Mx"][0]) < 1e-12 and got["gap"][0] < 1e-12
    assert got["gap"][4] > 0.5 and abs(got["Mz"][5] - z) > 0.25
    for name in ("Mx", "My", "Mz", "gap"):
        bits = got[name].view(np.int64)
        assert (bits[[1, 2, 3, 6, 7]] == NAN_BITS).all() and np.isfinite(got[name][[0, 4, 5]]).all(), name
    # infinite limits switch their tests off; a non-finite centre is status 3 everywhere but at the skipped cells, before
    # the data are looked at
    free = S.triangulate(dx, dy, X, Y, C1, C2, skip=skip, plane=(z, 0.0, 0.0))
    assert free["status"].tolist() == [0, 1, 2, 3, 0, 0, 1, 3] and free["count"] == 3
    for k in range(6):
        C = np.concatenate([C1, C2])
        C[k] = (np.nan, np.inf, -np.inf)[k % 3]
        lost = S.triangulate(dx, dy, X, Y, C[:3], C[3:], skip=skip)
        assert lost["status"].tolist() == [3, 1, 3, 3, 3, 3, 1, 3] and lost["count"] == 0 and (lost["sums"] == 0.0).all()
    # with the batch axis: the cells' skip and positions hold for every item
    two = S.triangulate(np.stack([dx, dx[::-1]]), np.stack([dy, dy[::-1]]), X, Y, C1, C2, skip=skip)
    assert two["status"].shape == (2, 8) and two["status"][0].tolist() == free["status"].tolist()
    assert two["status"][1, 1] == 1 and two["status"][1, 6] == 1 and two["count"].shape == (2,) and two["sums"].shape == (2, 9)


@pytest.mark.parametrize("cells", [1, 63, 1025, 2050])
def test_fixed_order_sums_against_fsum(cells):
    rng = np.random.default_rng(cells)
    X, Y = rng.uniform(-8, 8, cells), rng.uniform(-6, 6, cells)
    Xc, Yc, dx, dy = _analytic(X, Y, S.sheet(X, Y) + rng.normal(0, 0.02, cells))
    C1, C2 = _centres()
    skip = (rng.random(cells) < 0.2).astype(np.uint8) if cells > 1 else None
    centre = (-20.0, -15.0, -1.0)                                   # every term positive: the relative error means something
    got = S.triangulate(dx, dy, Xc, Yc, C1, C2, skip=skip, centre=centre)
    ok = got["status"] == 0
    assert got["count"] == ok.sum() and (cells == 1 or 0 < ok.sum() < cells)
    x, y, z = got["Mx"][ok] - centre[0], got["My"][ok] - centre[1], got["Mz"][ok] - centre[2]
    for k, q in enumerate((x, y, z, x * x, x * y, y * y, x * z, y * z, z * z)):
        want = math.fsum(q)
        assert want > 0 and abs(got["sums"][k] - want) <= 1e-12 * want, (k, got["sums"][k], want)
    assert S.fixed_sum(np.arange(5000.0), np.ones(5000, bool)) == 5000 * 4999 / 2


# ---- the class's refusals (no GPU is touched before them) ----------------------------------------------------------------------

def test_self_calibrate_and_disparity_refuse_before_any_gpu_call():
    import types
    import torchpiv_amd as T
    piv = object.__new__(T.StereoPIV)                               # no camera object, no frame: whatever went on would raise
    for kw in ({"iterations": 0}, {"iterations": 1.5}, {"iterations": True}, {"trim": 0.0}, {"trim": -1.0}, {"trim": np.nan},
               {"tol": -1e-3}, {"tol": np.inf}, {"tol": np.nan}, {"gap_max": -0.1}, {"gap_max": np.inf}, {"gap_max": "1"},
               {"min_cells": 2}, {"wind_size": 0}, {"wind_size": 32.0}, {"overlap": -1}, {"multipass": 0}, {"multipass": True}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            piv.self_calibrate(**kw)
    for kw in ({"wind_size": 0}, {"wind_size": "32"}, {"overlap": -16}, {"multipass": 0}, {"overlap": 1.0}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            piv.disparity(**kw)
    piv._resident = False                                           # a from_folders object
    for call in (piv.self_calibrate, piv.disparity, lambda: piv.disparity(wind_size=64, overlap=32)):
        with pytest.raises(NotImplementedError, match="resident frames only"):
            call()
    piv._resident = True
    piv._cams = (types.SimpleNamespace(_depth={"lo": 0, "hi": 4095}),) * 2
    for call in (piv.self_calibrate, piv.disparity):
        with pytest.raises(NotImplementedError, match="8-bit frames only"):
            call()
    assert "left to the caller" not in (T.StereoPIV.disparity.__doc__ + T.StereoPIV.__doc__)


def test_triangulate_refuses_host_tensors_and_wrong_arguments():
    import torch
    t = torch.zeros(2, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stereo_triangulate(t, t, t, t, (0, 0, 1), (1, 0, 1))
    with pytest.raises(TypeError):
        stereo_triangulate(t.numpy(), t, t, t, (0, 0, 1), (1, 0, 1))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

def test_symbol_in_header_binding_and_library():
    import ctypes as C
    from torchpiv_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "torchpiv_hip.h")).read()
    kern = open(os.path.join(ROOT, "torchpiv_amd", "csrc", "piv_kernels.h")).read()
    assert re.search(r"\bint\s+tpiv_stereo_triangulate\s*\(", hdr) and "launch_stereo_triangulate" in kern
    assert "tpiv_stereo_triangulate" in _lib.SIGNATURES and hasattr(_lib.lib, "tpiv_stereo_triangulate")
    assert len(_lib.SIGNATURES["tpiv_stereo_triangulate"][1]) == 20
    declared = re.search(r"int tpiv_stereo_triangulate\((.*?)\);", hdr, re.S).group(1)
    assert declared.count(",") + 1 == 20 and _lib.ABI_VERSION == 2
    # argument errors are decided on the host, before any launch (the device pointers are never followed): 16 cells, 2 items
    call = _lib.lib.tpiv_stereo_triangulate
    M1 = 1 << 24
    three = (C.c_double * 3)(0.0, 0.0, 0.0)
    base = dict(dx=1 * M1, dy=2 * M1, X=3 * M1, Y=4 * M1, skip=5 * M1, batch=2, cells=16,
                cams=(C.c_double * 6)(-1.0, 0.0, 5.0, 1.0, 0.0, 5.0), gap_max=1.0, plane=three, tol=1.0, centre=three,
                Mx=6 * M1, My=7 * M1, Mz=8 * M1, gap=9 * M1, status=10 * M1, count=11 * M1, sums=12 * M1)

    def rc(**change):
        a = dict(base, **change)
        return call(*a.values(), None)
    for k in ("dx", "dy", "X", "Y", "cams", "plane", "centre", "status", "count", "sums", "Mx", "My", "Mz", "gap"):
        assert rc(**{k: None}) == _lib.EINVAL, k                    # (one point output missing: a partial set)
    assert b"all four or not at all" in _lib.lib.tpiv_last_error()
    assert rc(batch=-1) == _lib.EINVAL and rc(cells=0) == _lib.EINVAL and rc(cells=-4) == _lib.EINVAL
    for k in ("gap_max", "tol"):
        for v in (-1.0, -0.0 - 1e-300, float("nan")):
            assert rc(**{k: v}) == _lib.EINVAL and k.encode() in _lib.lib.tpiv_last_error(), (k, v)
    none = dict(Mx=None, My=None, Mz=None, gap=None)
    assert rc(batch=0) == _lib.OK and rc(batch=0, **none, skip=None) == _lib.OK            # nothing to do, nothing launched
    assert rc(batch=0, gap_max=float("inf"), tol=float("inf")) == _lib.OK and rc(batch=0, gap_max=0.0, tol=0.0) == _lib.OK
    assert rc(batch=1 << 11, cells=1 << 20) == _lib.EINVAL and b"too large" in _lib.lib.tpiv_last_error()
    assert rc(batch=1, cells=1 << 31) == _lib.EINVAL and rc(batch=600000, cells=1) == _lib.EUNSUPPORTED
    # an output that overlaps an input (fields 256 bytes, cell planes 128, skip 16, sums 144, count 8), or another output
    assert rc(Mx=base["dx"] + 248) == _lib.EINVAL and b"aliases an input" in _lib.lib.tpiv_last_error()
    assert rc(gap=base["Y"] + 120) == _lib.EINVAL and rc(status=base["skip"] + 15) == _lib.EINVAL
    assert rc(sums=base["dy"] - 136) == _lib.EINVAL and rc(count=base["X"] - 4) == _lib.EINVAL
    assert rc(My=base["Mx"] + 8) == _lib.EINVAL and b"two outputs overlap" in _lib.lib.tpiv_last_error()
    assert rc(status=base["gap"] + 255) == _lib.EINVAL and rc(count=base["sums"] + 143) == _lib.EINVAL
    assert rc(count=base["sums"] + 144, batch=0) == _lib.OK


# ---- the gates' figures ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_cpu_path_converges_and_its_figures_are_the_recorded_ones(seed):
    """The conditions behind the GPU gates: the CPU path converges within four rounds (in three), every cell is valid in
    every measurement, and what it leaves stays within the recorded worst case."""
    rounds, converged, height, d, _ = S.cpu_path(seed)
    print(f"seed {seed}: {len(rounds)} rounds, sheet height left {height:.6f} mm, median |d| left {d:.6f} mm")
    assert converged and len(rounds) == 3 and all(r[6] == 63 for r in rounds) and all(r[2] >= 62 for r in rounds)
    assert abs(rounds[0][0][0] - 0.489) < 1e-3                       # round 1 stops 2 % short of 0.5
    assert height <= S.HEIGHT_LEFT + 5e-7 and d <= S.D_LEFT + 5e-7
    assert seed != 2 or (abs(height - S.HEIGHT_LEFT) < 5e-7 and abs(d - S.D_LEFT) < 5e-7)       # the worst seed sets both
