"""Iterative image deformation, the parts that need no GPU: the numpy model the device kernels are checked against
(tests/deform_model.py) on cases whose answers are written down here, the deform= argument, the new symbols in the header
and the binding, and the scheme's accuracy on the model alone: three rounds around the CPU oracle's first pass against the
oracle's plain two-pass CWS field on a flow with gradients."""
import inspect
import os
import re

import numpy as np
import pytest

import deform_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- nodes ----------------------------------------------------------------------------------------------------------
def test_nodes_single_valid_cell():
    u = np.zeros((3, 4))
    v = np.zeros((3, 4))
    inv = np.ones((3, 4), dtype=np.uint8)
    u[1, 1], v[1, 1], inv[1, 1] = 2.0, -1.0, 0
    nd = M.nodes(u, v, inv, smooth=False)
    want = np.zeros((3, 4, 2), dtype=np.int16)
    want[0:3, 0:3] = (256, -128)        # the cell and its 8 neighbours (each has it as the only valid neighbour)
    assert nd.dtype == np.int16 and np.array_equal(nd, want)
    # smoothing reads the substituted values with edge replicate: column 3 holds zeros
    sm = M.nodes(u, v, inv, smooth=True)
    assert sm[1, 1].tolist() == [256, -128] and sm[1, 2].tolist() == [192, -96]     # 4 of the 16 weights fall on column 3
    e = np.pad(want.astype(np.int64), ((1, 1), (1, 1), (0, 0)), mode="edge")
    k = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]])
    for r in range(3):
        for c in range(4):
            acc = (k[:, :, None] * e[r:r + 3, c:c + 3]).sum(axis=(0, 1))
            assert sm[r, c].tolist() == ((acc + 8) >> 4).tolist()


def test_nodes_all_invalid_give_zeros():
    u = np.full((4, 5), 3.7)
    inv = np.ones((4, 5), dtype=np.uint8)
    for smooth in (False, True):
        assert not M.nodes(u, -u, inv, smooth).any()
    # non-finite cells are invalid cells
    bad = np.full((2, 2), np.nan)
    assert not M.nodes(bad, bad, np.zeros((2, 2), dtype=np.uint8), True).any()


def test_nodes_rounding_ties_clamp_and_floor():
    w = np.array([[0.5 / 128, 1.5 / 128, 2.5 / 128, -0.5 / 128, -1.5 / 128, 200.0, -200.0, 1e300]])
    z = np.zeros_like(w)
    nd = M.nodes(w, z, np.zeros(w.shape, dtype=np.uint8), smooth=False)
    assert nd[0, :, 0].tolist() == [0, 2, 2, 0, -2, 16383, -16383, 16383]       # ties to even; the clamp
    assert not nd[..., 1].any()
    # substitution: floor((2 s + k) / (2 k)) is the mean rounded half up, also below zero
    u = np.array([[1 / 128, 0.0, 2 / 128]])           # s = 3, k = 2 -> 2 (1.5 rounds up)
    inv = np.array([[0, 1, 0]], dtype=np.uint8)
    assert M.nodes(u, -u, inv, False)[0, 1].tolist() == [2, -1]                   # -1.5 rounds up to -1
    # a NaN in one component makes the whole cell invalid
    u2, v2 = np.array([[1.0, np.inf, 3.0]]), np.array([[1.0, 1.0, 1.0]])
    assert M.nodes(u2, v2, np.zeros((1, 3), dtype=np.uint8), False)[0, 1].tolist() == [256, 128]


def test_nodes_one_row_grid_and_batch():
    rng = np.random.default_rng(3)
    u, v = rng.normal(0, 3, (2, 1, 5)), rng.normal(0, 3, (2, 1, 5))
    inv = (rng.random((2, 1, 5)) < 0.3).astype(np.uint8)
    nd = M.nodes(u, v, inv, True)
    assert nd.shape == (2, 1, 5, 2)
    for k in range(2):
        assert np.array_equal(nd[k], M.nodes(u[k], v[k], inv[k], True))
    # 1 x 1: nothing to substitute from, nothing to smooth with
    assert M.nodes(np.array([[1.0]]), np.array([[-2.0]]), np.zeros((1, 1), dtype=np.uint8), True).tolist() == [[[128, -256]]]
    assert M.nodes(np.array([[1.0]]), np.array([[-2.0]]), np.ones((1, 1), dtype=np.uint8), True).tolist() == [[[0, 0]]]


# ---- dense shift and warp -------------------------------------------------------------------------------------------
def test_axis_weights_are_bilinear_between_the_window_centres():
    ws, st, n, size = 16, 8, 4, 44
    r, w = M.axis(size, n, ws, st)
    centres = np.arange(n) * st + (ws - 1) / 2.0         # 7.5, 15.5, 23.5, 31.5
    assert r[:8].tolist() == [0] * 8 and w[:8].tolist() == [0] * 8            # constant in front of the first centre
    assert r[-12:].tolist() == [n - 2] * 12 and w[-12:].tolist() == [256] * 12
    for y in range(8, 32):
        pos = r[y] + w[y] / 256.0
        assert abs(pos - (y - centres[0]) / st) <= 1 / 512 + 1e-12
    assert M.axis(20, 1, 16, 8)[0].tolist() == [0] * 20 and not M.axis(20, 1, 16, 8)[1].any()


def test_zero_field_is_the_identity_and_uniform_field_a_shifted_copy():
    a, b = M.scene(0, 45, 61)
    ws, ov = 12, 5
    nr, nc = M.field_shape(45, 61, ws, ov)
    zero = np.zeros((nr, nc, 2), dtype=np.int16)
    for interp in ("linear", "cubic"):
        wa, wb = M.warp(a, b, zero, ws, ov, interp)
        assert np.array_equal(wa, a) and np.array_equal(wb, b)
    # half shift (+2, -1) px everywhere: wa[y][x] = a[y + 1][x - 2], wb[y][x] = b[y - 1][x + 2], edges replicated
    nd = np.empty((nr, nc, 2), dtype=np.int16)
    nd[..., 0], nd[..., 1] = 512, -256
    y, x = np.mgrid[0:45, 0:61]
    for interp in ("linear", "cubic"):
        wa, wb = M.warp(a, b, nd, ws, ov, interp)
        assert np.array_equal(wa, a[np.clip(y + 1, 0, 44), np.clip(x - 2, 0, 60)])
        assert np.array_equal(wb, b[np.clip(y - 1, 0, 44), np.clip(x + 2, 0, 60)])
    # one window in the frame: one node, a constant field
    one = np.array([[[256, 256]]], dtype=np.int16)
    wa, _ = M.warp(a[:12, :12], b[:12, :12], one, 12, 5, "cubic")
    yy, xx = np.mgrid[0:12, 0:12]
    assert np.array_equal(wa, a[:12, :12][np.clip(yy - 1, 0, 11), np.clip(xx - 1, 0, 11)])


def test_dense_shift_reproduces_the_node_at_a_window_centre():
    rng = np.random.default_rng(5)
    ws, ov, H, W = 13, 5, 70, 93          # an odd window: the centre r st + 6 is a pixel
    nr, nc = M.field_shape(H, W, ws, ov)
    nd = rng.integers(-2000, 2000, (nr, nc, 2)).astype(np.int16)
    hx, hy = M.dense(nd, H, W, ws, ov)
    for r in range(nr):
        for c in range(nc):
            assert (hx[r * 8 + 6, c * 8 + 6], hy[r * 8 + 6, c * 8 + 6]) == tuple(nd[r, c])
    # half way between two centres: the mean of the two nodes, rounded half up
    assert hx[6, 10] == (int(nd[0, 0, 0]) + int(nd[0, 1, 0]) + 1) >> 1
    assert hx.min() >= nd[..., 0].min() and hx.max() <= nd[..., 0].max()       # a convex combination, rounded to nearest
    assert hy.min() >= nd[..., 1].min() and hy.max() <= nd[..., 1].max()


def test_combine_is_one_rounding():
    nd = np.array([[[3, -5]]], dtype=np.int16)
    u, v, inv = M.combine(nd, np.array([[0.1]]), np.array([[0.2]]), np.array([[1]], dtype=np.uint8))
    assert u[0, 0] == 3 / 128 + 0.1 and v[0, 0] == -5 / 128 + 0.2 and inv.dtype == np.uint8 and inv[0, 0] == 1


# ---- the argument and the symbols -----------------------------------------------------------------------------------
def test_deform_arg_forms_and_refusals():
    from torchpiv_amd import engine
    full = {"iterations": 3, "interp": "cubic", "smooth": True}
    assert engine.DEFORM_DEFAULTS == full
    assert engine.deform_arg(None) is None and engine.deform_arg(0) is None and engine.deform_arg({"iterations": 0}) is None
    assert engine.deform_arg(3) == full and engine.deform_arg({}) == full and engine.deform_arg(np.int64(3)) == full
    assert engine.deform_arg({}) is not engine.DEFORM_DEFAULTS
    assert engine.deform_arg(8)["iterations"] == 8
    assert engine.deform_arg({"iterations": 1, "interp": "linear", "smooth": False}) == \
        {"iterations": 1, "interp": "linear", "smooth": False}
    for bad in (True, "3", 3.0, -1, 9, [3], {"iterations": 9}, {"iterations": 2.0}, {"iterations": True},
                {"interp": "nearest"}, {"interp": None}, {"smooth": 1}, {"smooth": None}, {"rounds": 3}, {"iterations": 3, 1: 2}):
        with pytest.raises(ValueError, match="deform"):
            engine.deform_arg(bad)


def test_constructors_check_the_argument_before_any_device(tmp_path):
    import torch

    import torchpiv_amd as T
    from torchpiv_amd import runner
    with pytest.raises(ValueError, match="deform"):
        T.OfflinePIV(str(tmp_path), "cpu", "bmp", 32, 16, deform="3")
    z = torch.zeros(1, 64, 64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="deform"):
        T.ResidentPIV(z, z, 32, 16, deform={"iterations": 9})
    with pytest.raises(ValueError, match="deform"):
        runner.run_folder(str(tmp_path), "cpu", "bmp", 32, 16, deform={"interp": "nearest"})
    piv = T.OfflinePIV(str(tmp_path), "cpu", "bmp", 32, 16, deform=2)
    assert piv._deform == {"iterations": 2, "interp": "cubic", "smooth": True}
    assert T.OfflinePIV(str(tmp_path), "cpu", "bmp", 32, 16)._deform is None
    for fn in (T.OfflinePIV.__init__, T.ResidentPIV.__init__, runner.run_folder):
        assert inspect.signature(fn).parameters["deform"].default is None


def test_new_symbols_in_header_binding_and_library():
    from torchpiv_amd import _lib
    header = open(os.path.join(ROOT, "include", "torchpiv_hip.h")).read()
    for name in ("tpiv_deform_nodes", "tpiv_deform_warp", "tpiv_deform_combine", "tpiv_plan_set_deform",
                 "tpiv_plan_deform_stage", "tpiv_plan_deform_ms"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name) is not None
    assert len(_lib.SIGNATURES["tpiv_deform_warp"][1]) == 14
    assert _lib.lib.tpiv_version() == 2


# ---- accuracy of the scheme on the model alone ----------------------------------------------------------------------
def test_three_rounds_halve_the_error_of_plain_cws_on_a_flow_with_gradients():
    """256 x 256, the scene of deform_model (peak gradient 0.196 px / px), seed 0; the oracle's first pass at 32/16 and CWS
    pass at 16/8, then three rounds of the model (cubic, smoothed) around the oracle's first pass at 16/8.  RMS vector error
    against the constructed flow over the interior cells valid in both runs: the model's must be at most half the plain
    field's, with at least 95 % of the interior cells counted.  Measured with this model: printed below and recorded in
    profiles/deform/measurements.json."""
    from oracle import piv_oracle as O
    H = W = 256
    a, b = M.scene(0, H, W)
    u, v, x, y, val = O.pass1(a, b, 32, 16, validate=True)
    u, v, x, y, val = O.ITER["CWS"](a.shape, 16, 8)(a, b, x, y, u, v, val)

    def first_pass(wa, wb):
        du, dv, _, _, dval = O.pass1(wa, wb, 16, 8, validate=True)
        return du, dv, dval

    u3, v3, inv3 = M.rounds(a, b, u, v, np.asarray(val).astype(np.uint8), 16, 8, 3, first_pass)
    tu, tv = M.truth(H, W, 16, 8)
    ok = (~np.asarray(val).astype(bool)) & (inv3 == 0)
    plain, share = M.rms_interior(u, v, tu, tv, ok)
    deformed, _ = M.rms_interior(u3, v3, tu, tv, ok)
    print(f"deform model accuracy: plain CWS {plain:.4f} px, 3 rounds {deformed:.4f} px, ratio {deformed / plain:.3f}, "
          f"share of interior cells {share:.4f}")
    assert share >= 0.95, share
    assert deformed <= 0.5 * plain, (deformed, plain)
