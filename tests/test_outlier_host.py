"""Normalized median test, the parts that need no GPU: known answers of the numpy model the device kernel is checked
against (tests/outlier_model.py), the outlier= argument checked in the constructors before any device is touched, the
new symbols in the header and the binding, and the false-flag share of the model on a clean flow (the cap that
tests/test_gpu_outlier.py applies to the fields of real frames)."""
import os
import re

import numpy as np
import pytest

from outlier_model import median_test, replaced

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_uniform_field_with_one_spike():
    u = np.full((7, 9), 2.5)
    v = np.full((7, 9), -1.25)
    u[3, 4] = 11.0
    inv = np.zeros((7, 9), np.uint8)
    st, mu, mv = median_test(u, v, inv)
    want = np.zeros((7, 9), np.uint8)
    want[3, 4] = 1
    assert np.array_equal(st, want)
    assert mu[3, 4] == 2.5 and mv[3, 4] == -1.25
    # the spike's neighbours see one deviating value among eight (five, three): the median stays the uniform value
    assert np.array_equal(_bits(mu), _bits(np.full((7, 9), 2.5))) and np.array_equal(_bits(mv), _bits(v))
    ru, rv = replaced(u, v, st, mu, mv)
    assert np.array_equal(ru, np.full((7, 9), 2.5)) and np.array_equal(rv, v)


def test_corners_and_edges_have_three_and_five_neighbours():
    # u = column index: a corner's neighbours are {0, 1, 1} resp. an edge's {0, 0, 1, 2, 2} -- odd k, the middle one
    u = np.tile(np.arange(4.0), (3, 1))
    v = np.zeros((3, 4))
    inv = np.zeros((3, 4), np.uint8)
    st, mu, _ = median_test(u, v, inv)
    assert mu[0, 0] == 1.0            # k = 3: sorted (0, 1, 1) -> s[1]
    assert mu[0, 1] == 1.0            # k = 5: sorted (0, 0, 1, 2, 2) -> s[2]
    assert mu[1, 1] == 1.0            # k = 8: sorted (0,0,0,1,2,2,2,... ) -> (s[3] + s[4]) / 2
    assert mu[1, 0] == 1.0            # k = 5 on the left edge: (0, 0, 1, 1, 1) -> s[2]
    # corner (0, 0): |0 - 1| = 1 against 2 * (median(|0-1|, |1-1|, |1-1|) + 0.1) = 0.2: flagged at the defaults
    assert st[0, 0] == 1
    # ... and not with min_neighbours = 4: three neighbours are too few, the medians are the cell's own values
    st4, mu4, mv4 = median_test(u, v, inv, min_neighbours=4)
    assert st4[0, 0] == 0 and mu4[0, 0] == u[0, 0] and mv4[0, 0] == v[0, 0]
    assert st4[0, 1] == median_test(u, v, inv)[0][0, 1]           # an edge (k = 5) is still tested
    # an even k on purpose: a 2 x 2 grid has k = 3 everywhere; a 2 x 3 grid's middle cells k = 5, a 1 x 3 row's k = 2
    st, mu, _ = median_test(np.array([[1.0, 5.0, 2.0]]), np.zeros((1, 3)), np.zeros((1, 3), np.uint8), min_neighbours=2)
    assert mu[0, 1] == 1.5 and mu[0, 0] == 1.0 and st[0, 0] == 0  # ends: k = 1 < 2, untouched


def test_invalid_neighbours_are_excluded_and_the_centre_mask_plays_no_part():
    u = np.full((3, 3), 1.0)
    v = np.full((3, 3), 1.0)
    u[0, 0] = u[0, 1] = u[0, 2] = 100.0                          # three wild neighbours of the centre ...
    inv = np.zeros((3, 3), np.uint8)
    inv[0, :] = 1                                                 # ... that the peak-ratio test has already thrown out
    st, mu, _ = median_test(u, v, inv)
    assert mu[1, 1] == 1.0 and (st[1, 1] & 1) == 0               # k = 5, all ones
    assert np.array_equal(st >> 1, inv)                           # bit 1 carries the input mask
    # the same field with the centre itself invalid: same decision, same medians (its own mask bit plays no part)
    inv2 = inv.copy()
    inv2[1, 1] = 1
    st2, mu2, mv2 = median_test(u, v, inv2)
    assert (st2[1, 1] & 1) == (st[1, 1] & 1) and mu2[1, 1] == mu[1, 1] and st2[1, 1] >> 1 == 1
    # an invalid cell is tested too: row 0 lies 99 off its valid neighbours' median
    assert (st[0, 1] & 1) == 1 and mu[0, 1] == 1.0
    # all invalid: k = 0 everywhere, nothing flagged, medians = own values
    st3, mu3, mv3 = median_test(u, v, np.ones((3, 3), np.uint8))
    assert np.array_equal(st3, np.full((3, 3), 2, np.uint8)) and np.array_equal(mu3, u) and np.array_equal(mv3, v)


def test_all_equal_neighbourhood_eps_decides():
    u = np.full((3, 3), 4.0)
    v = np.zeros((3, 3))
    inv = np.zeros((3, 3), np.uint8)
    for centre, eps, want in ((4.15, 0.1, 0), (4.25, 0.1, 1), (4.25, 0.2, 0), (4.0 + 2 ** -20, 0.0, 1), (4.0, 0.0, 0)):
        u[1, 1] = centre
        st, _, _ = median_test(u, v, inv, threshold=2.0, eps=eps)
        assert st[1, 1] == want, (centre, eps)
    # exactly on the bound is not an outlier (strict >): 4.5 - 4 = 0.5 = 2 * (0 + 0.25), all exact in binary
    u[1, 1] = 4.5
    assert median_test(u, v, inv, threshold=2.0, eps=0.25)[0][1, 1] == 0


def test_linear_shear_flags_nothing_at_threshold_two():
    """synth's "shear" flow (u = 5 y / H - 1, v = 0.4) sampled at 8 px spacing in a 512 px frame: 0.078 px per cell.
    Interior and side-edge cells have their neighbours symmetric around them: the median is the cell's own value.  On the
    top / bottom edge and in the corners the cell is one step g off its neighbours' median with a median residual of 0:
    flagged only where g > threshold * eps = 0.2 px per cell, which this shear is not (a shear of 0.3 px per cell is)."""
    yc = (np.arange(40) * 8.0 + 8.0)[:, None] * np.ones((1, 12))
    u = 5.0 * (yc / 512.0) - 1.0
    v = np.full_like(u, 0.4)
    inv = np.zeros(u.shape, np.uint8)
    st, _, _ = median_test(u, v, inv, threshold=2.0, eps=0.1)
    assert not st.any()
    st3, _, _ = median_test(0.3 * np.arange(40.0)[:, None] * np.ones((1, 12)), v, inv, threshold=2.0, eps=0.1)
    assert st3[1:-1].sum() == 0 and st3[0].all() and st3[-1].all()


def test_minus_zero_sorts_before_plus_zero():
    # k = 3 at a corner with neighbours (+0.0, -0.0, 1.0): sorted (-0.0, +0.0, 1.0) -> the median is +0.0;
    # with neighbours (-0.0, +0.0, -1.0): sorted (-1.0, -0.0, +0.0) -> the median is -0.0
    u = np.array([[5.0, 0.0], [-0.0, 1.0]])
    st, mu, _ = median_test(u, np.zeros((2, 2)), np.zeros((2, 2), np.uint8))
    assert _bits(mu[0, 0]) == _bits(0.0)
    u = np.array([[5.0, -0.0], [0.0, -1.0]])
    st, mu, _ = median_test(u, np.zeros((2, 2)), np.zeros((2, 2), np.uint8))
    assert _bits(mu[0, 0]) == _bits(-0.0)


FALSE_FLAG_CAP = 0.01        # share of clean-flow cells the test may flag (tests/test_gpu_outlier.py applies the same cap)


def test_model_false_flag_share_on_a_clean_flow():
    """The model on the ground truth of the flow tests/test_gpu_outlier.py runs on frames -- synth's "uniform" flow,
    (2.3, -1.6) px, on the 31 x 31 grid of 16 px windows at 8 px spacing in a 256 px frame -- plus independent Gaussian
    noise per component at the level the delivered fields carry against the true flow.  That level is measured by
    test_gpu_outlier.py on its own frames (clean_rms in its docstring) and asserted there to stay below the 0.07 px this
    test covers; the float32 / float64 differences the parity tests gate, 1e-6 px, play no part.  At threshold 2, eps 0.1
    a cell is flagged beyond 2 * (median residual ~ 0.7 sigma + 0.1) of its neighbours' median: 5 sigma at 0.05 px.
    Model alone, three seeds each: 0 of 961 cells at 0.03 and 0.05 px rms, 0.1 ... 0.2 % at 0.07 px -- under the cap of
    1 % -- and over it from 0.1 px on (1.7 %; 7 % at 0.15 px), where eps should be raised with the noise."""
    n = 31
    u = np.full((n, n), 2.3)
    v = np.full((n, n), -1.6)
    inv = np.zeros((n, n), np.uint8)
    for sigma, seed in ((0.05, 17), (0.07, 17), (0.07, 18), (0.07, 19)):
        rng = np.random.default_rng(seed)
        st, _, _ = median_test(u + rng.normal(0, sigma, u.shape), v + rng.normal(0, sigma, v.shape), inv)
        share = (st & 1).mean()
        print(f"noise {sigma} px rms: flagged share {share:.4f}")
        assert share < FALSE_FLAG_CAP, (sigma, share)


def test_border_cells_of_a_steep_gradient_are_flagged():
    """What the one-sided neighbourhood of a border cell means: synth's "wavy" flow at 8 px spacing in a
    512 px frame changes by 4 * 2 pi / 512 * 8 = 0.39 px per cell across the top and bottom rows -- more than
    threshold * eps = 0.2 -- so those rows are flagged, and nothing in the interior, where the neighbours surround the
    cell.  min_neighbours = 6 exempts edges and corners (k = 5 and 3)."""
    import math
    n = 63
    yc, xc = np.mgrid[0:n, 0:n] * 8.0 + 8.0
    u = 4.0 * np.sin(2 * math.pi * yc / 512) + 1.3
    v = 3.0 * np.cos(2 * math.pi * xc / 512) - 0.7
    inv = np.zeros((n, n), np.uint8)
    st = median_test(u, v, inv)[0]
    assert not st[1:-1, 1:-1].any() and st[0].all() and st[-1].all()
    assert not median_test(u, v, inv, min_neighbours=6)[0].any()


# ---------------------------------------------------------------------------------------------------------------------
# the keyword, checked before any GPU call
# ---------------------------------------------------------------------------------------------------------------------
BAD = ["mean", "Median", 2.0, ["median"], {"thresh": 2.0}, {"threshold": 0.0}, {"threshold": -1.0}, {"eps": -0.1},
       {"min_neighbours": 0}, {"min_neighbours": 9}, {"min_neighbours": 3.5}, {"threshold": "high"},
       {"threshold": float("nan")}, {"eps": float("inf")}, {"min_neighbours": True}]
GOOD = [None, "median", {}, {"threshold": 3.0}, {"eps": 0.0}, {"min_neighbours": 1}, {"min_neighbours": 8},
        {"threshold": 1.5, "eps": 0.2, "min_neighbours": 5}]


def test_outlier_argument_is_checked_before_the_gpu(tmp_path):
    from torchpiv_amd import backend as T
    from torchpiv_amd import engine, runner
    for bad in BAD:
        with pytest.raises(ValueError):
            T.OfflinePIV(str(tmp_path), "cpu", "bmp", 64, 32, outlier=bad)
        with pytest.raises(ValueError):
            runner.run_folder(str(tmp_path), "cpu", "bmp", 64, 32, outlier=bad)
        with pytest.raises(ValueError):                           # engine.Plan checks it ahead of its own device check
            engine.Plan(64, 64, 32, 16, outlier=bad)
    for good in GOOD:
        piv = T.OfflinePIV(str(tmp_path), "cpu", "bmp", 64, 32, outlier=good)
        assert len(piv) == 0 and list(piv()) == []
        assert runner.run_folder(str(tmp_path), "cpu", "bmp", 64, 32, outlier=good) == (None, 0)
    assert engine.outlier_arg("median") == {"threshold": 2.0, "eps": 0.1, "min_neighbours": 3}
    assert engine.outlier_arg({"eps": 0.25}) == {"threshold": 2.0, "eps": 0.25, "min_neighbours": 3}
    assert engine.outlier_arg(None) is None


def test_resident_outlier_argument_is_checked_before_the_gpu():
    import torch
    from torchpiv_amd import backend as T
    f = torch.zeros(2, 64, 64, dtype=torch.uint8)
    with pytest.raises(ValueError):
        T.ResidentPIV(f, f, 32, 16, outlier="mean")
    with pytest.raises(ValueError):
        T.ResidentPIV(f, f, 32, 16, outlier={"min_neighbours": 12})


def test_outlier_symbols_in_header_and_binding():
    """The three new entry points are declared in the header, bound in _lib.SIGNATURES and exported by the library (the
    import of _lib resolves every bound name); the ABI version stays 2."""
    from torchpiv_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "torchpiv_hip.h")).read()
    for name in ("tpiv_median_test", "tpiv_plan_set_outlier", "tpiv_plan_pass_outliers"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert len(_lib.SIGNATURES["tpiv_median_test"][1]) == 13
    assert _lib.ABI_VERSION == 2 and "#define TPIV_VERSION 2" in hdr
    # argument errors of the function-level seam are decided on the host, before any launch
    for args in ((1, 0, 4, 2.0, 0.1, 3), (1, 4, 0, 2.0, 0.1, 3), (1, 4, 4, 0.0, 0.1, 3), (1, 4, 4, 2.0, -1.0, 3),
                 (1, 4, 4, 2.0, 0.1, 0), (1, 4, 4, 2.0, 0.1, 9), (-1, 4, 4, 2.0, 0.1, 3)):
        b, nr, nc, thr, eps, mn = args
        assert _lib.lib.tpiv_median_test(4096, 8192, 12288, b, nr, nc, thr, eps, mn, 16384, None, None, None) == _lib.EINVAL
    assert _lib.lib.tpiv_median_test(None, 8192, 12288, 1, 4, 4, 2.0, 0.1, 3, 16384, None, None, None) == _lib.EINVAL
    # an output that overlaps an input, or another output
    assert _lib.lib.tpiv_median_test(4096, 8192, 12288, 1, 4, 4, 2.0, 0.1, 3, 12288 + 15, None, None, None) == _lib.EINVAL
    assert _lib.lib.tpiv_median_test(4096, 8192, 12288, 1, 4, 4, 2.0, 0.1, 3, 16384, 4096 + 120, None, None) == _lib.EINVAL
    assert _lib.lib.tpiv_median_test(4096, 8192, 12288, 1, 4, 4, 2.0, 0.1, 3, 16384, 20480, 20480, None) == _lib.EINVAL
    assert _lib.lib.tpiv_plan_set_outlier(None, 1, 2.0, 0.1, 3) == _lib.EINVAL
