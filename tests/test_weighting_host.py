"""Weighted interrogation windows (weighting="gaussian" / "uniform") on the CPU: every form and refusal of the keyword, the
new symbols, the tables, the float64 model of tests/weighting_model.py against the oracle ("uniform" is the top-hat window)
and against its own definition (empty windows), and what the Gaussian weight buys on the scene of tests/deform_model.py --
all without a GPU.

TPIV_WEIGHTING_REPORT=<file>: the figures are appended there as JSON lines (profiles/weighting/measurements.json keeps a
run's)."""
import functools
import inspect
import json
import os
import re

import numpy as np
import pytest

from oracle import piv_oracle as O
import deform_model as DM
import ensemble_model as EM
import weighting_model as WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.environ.get("TPIV_WEIGHTING_REPORT")
GATE_PX = 1e-3


def report(**kw):
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(json.dumps(kw) + "\n")


# ---- arguments and refusals -----------------------------------------------------------------------------------------
def test_every_form_of_the_keyword():
    from torchpiv_amd import engine
    g = {"kind": "gaussian", "sx": 0.4, "sy": 0.4}
    assert engine.weighting_arg(None) is None
    assert engine.weighting_arg("gaussian") == g
    assert engine.weighting_arg({}) == g and engine.weighting_arg({"kind": "gaussian"}) == g
    assert engine.weighting_arg(g) == g                                  # its own result
    assert engine.weighting_arg("uniform") == {"kind": "uniform", "sx": 0.0, "sy": 0.0}
    assert engine.weighting_arg(engine.weighting_arg("uniform")) == engine.weighting_arg("uniform")
    assert engine.weighting_arg({"sigma": 1}) == {"kind": "gaussian", "sx": 1.0, "sy": 1.0}
    assert engine.weighting_arg({"kind": "gaussian", "sigma": (0.3, 0.6)}) == {"kind": "gaussian", "sx": 0.3, "sy": 0.6}
    assert engine.weighting_arg({"sigma": 0.2})["sx"] == 0.2 and engine.weighting_arg({"sigma": [4, 4.0]})["sy"] == 4.0
    for bad in ("gauss", "Gaussian", "tophat", 1, 0.4, ("gaussian",), {"kind": "hann"}, {"kind": None}, {"sigma": 0.19},
                {"sigma": 4.1}, {"sigma": (0.4, 5.0)}, {"sigma": (0.4, 0.4, 0.4)}, {"sigma": "wide"}, {"sigma": True},
                {"sigma": None}, {"sigma": float("nan")}, {"sigma": -0.4}, {"radius": 3}, {"kind": "uniform", "sigma": 0.4},
                {"diameter": 2.0}):
        with pytest.raises(ValueError):
            engine.weighting_arg(bad)


def test_refusals_without_a_gpu():
    import torch
    from torchpiv_amd import backend, engine, runner
    for ws, n_pass in ((8, 1), (128, 1), (48, 1), (32, 3)):            # 32 -> 16 -> 8: a chain that reaches 8
        sizes = [w for w, _ in engine.pass_sizes(ws, ws // 2, n_pass, 2.0)]
        with pytest.raises(NotImplementedError, match=str([s for s in sizes if s not in (16, 32, 64)][0])):
            engine.weighting_check(sizes)
        with pytest.raises(NotImplementedError):
            engine.Plan(256, 256, ws, ws // 2, n_pass=n_pass, weighting="gaussian")
    engine.weighting_check([64, 32, 16], "CWS")
    with pytest.raises(NotImplementedError, match="CWS_Fast"):
        engine.weighting_check([32], "CWS_Fast")
    with pytest.raises(ValueError, match="uncertainty"):
        engine.Plan(160, 160, 32, 16, weighting="gaussian", uncertainty="cs")
    with pytest.raises(ValueError, match="ensemble"):
        engine.Plan(160, 160, 32, 16, weighting="uniform", ensemble=True)
    with pytest.raises(ValueError, match="correlation"):
        engine.Plan(160, 160, 32, 16, weighting="gaussian", correlation="rpc")
    with pytest.raises(ValueError):
        engine.Plan(160, 160, 32, 16, weighting="hann")
    with pytest.raises(ValueError):
        engine.Plan(160, 160, 32, 16, weighting={"sigma": 9.0})
    # the host classes check in the constructor, before any GPU call (CPU tensors: the GPU is asked for last)
    z = torch.zeros(2, 96, 96, dtype=torch.uint8)
    with pytest.raises(ValueError):
        backend.ResidentPIV(z, z, 32, 16, weighting="hann")
    with pytest.raises(ValueError):
        backend.ResidentPIV(z, z, 32, 16, weighting={"sigma": 0.1})
    with pytest.raises(NotImplementedError, match="8"):
        backend.ResidentPIV(z, z, 16, 8, multipass=2, weighting="gaussian")
    with pytest.raises(ValueError, match="uncertainty"):
        backend.ResidentPIV(z, z, 32, 16, weighting="gaussian", uncertainty="cs")
    with pytest.raises(ValueError, match="correlation"):
        backend.ResidentPIV(z, z, 32, 16, weighting="gaussian", correlation="phase")
    with pytest.raises(ValueError):
        backend.OfflinePIV("no/such/folder", "cuda:0", "bmp", 32, 16, weighting="hann")
    with pytest.raises(NotImplementedError, match="48"):
        backend.OfflinePIV("no/such/folder", "cuda:0", "bmp", 48, 24, weighting="uniform")
    with pytest.raises(ValueError):
        runner.run_folder("no/such/folder", "cuda:0", "bmp", 32, 16, weighting={"kind": "gaussian", "diameter": 1})
    # on the host classes and run_folder the keyword stands behind correlation=
    for fn in (backend.OfflinePIV.__init__, backend.ResidentPIV.__init__, runner.run_folder):
        names = list(inspect.signature(fn).parameters)
        assert names.index("weighting") == names.index("correlation") + 1
    for fn in (engine.Plan.__init__, engine.debug_pass):
        assert "weighting" in inspect.signature(fn).parameters
    assert callable(engine.Plan.set_weighting)


def test_new_symbols_in_header_binding_and_library():
    from torchpiv_amd import _lib
    header = open(os.path.join(ROOT, "include", "torchpiv_hip.h")).read()
    for name in ("tpiv_plan_set_weighting", "tpiv_debug_pass_weighted"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name) is not None
    m = re.search(r"enum\s*\{\s*TPIV_WEIGHT_NONE\s*=\s*0\s*,\s*TPIV_WEIGHT_UNIFORM\s*=\s*1\s*,\s*TPIV_WEIGHT_GAUSSIAN\s*=\s*2\s*\}", header)
    assert m
    assert (_lib.WEIGHT_NONE, _lib.WEIGHT_UNIFORM, _lib.WEIGHT_GAUSSIAN) == (0, 1, 2)
    assert _lib.WEIGHTINGS == {"uniform": 1, "gaussian": 2}
    # the two entries take the argument lists the header gives them: count the parameters
    for name in ("tpiv_plan_set_weighting", "tpiv_debug_pass_weighted"):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "xcorr_win" in open(os.path.join(ROOT, "torchpiv_amd", "csrc", "Makefile")).read()


def test_tables_are_float64_exp_rounded_once():
    from torchpiv_amd import engine
    par = engine.weighting_arg({"sigma": (0.3, 0.6)})
    tab = engine.weighting_tables(par, [64, 32])
    assert tab.dtype == np.float32 and tab.size == 2 * 64 + 2 * 32
    assert np.array_equal(tab[:64], WM.table(64, 0.6)) and np.array_equal(tab[64:128], WM.table(64, 0.3))     # g_y, then g_x
    assert np.array_equal(tab[128:160], WM.table(32, 0.6)) and np.array_equal(tab[160:], WM.table(32, 0.3))
    for ws in (16, 32, 64):
        for s in (0.2, 0.4, 1.0, 4.0):
            g = engine.weighting_tables(engine.weighting_arg({"sigma": s}), [ws])[:ws]
            i = np.arange(ws, dtype=np.float64)
            want = np.float32(np.exp(-(((2 * i - (ws - 1)) / ws) ** 2) / (2 * s * s)))
            assert np.array_equal(g, want)
            assert np.array_equal(g, g[::-1])                           # symmetric about the window centre
            assert (g > 0).all() and (g <= 1).all() and np.isfinite(g).all()
            assert g.argmax() in (ws // 2 - 1, ws // 2)
    ones = engine.weighting_tables(engine.weighting_arg("uniform"), [16, 32])
    assert np.array_equal(ones, np.ones(96, np.float32))
    W = WM.weight(32, {"sigma": (0.3, 0.6)})
    assert W.dtype == np.float32 and np.array_equal(W, (WM.table(32, 0.6)[:, None] * WM.table(32, 0.3)[None, :]))
    assert not np.array_equal(W, W.T)


def test_a_swap_of_the_two_tables_shows_in_the_map():
    """sigma = (0.3, 0.6): the map formed with g_x and g_y exchanged differs from the right one by thousands of times what
    a float32 evaluation differs by, so the map gate of tests/test_gpu_weighting.py sees a swap."""
    a, b = EM.scene(3, 96, 96, density=0.03)
    wa, wb = WM.windows(0, a, b, 32, 16)
    W = WM.weight(32, {"sigma": (0.3, 0.6)})
    C, _ = WM.weighted_map(wa, wb, W, True)
    C32, _ = WM.weighted_map(wa, wb, W, True, f32=True)
    Cs, _ = WM.weighted_map(wa, wb, np.ascontiguousarray(W.T), True)
    scale = WM.shift_scale(wa, wb, W, True)[:, None, None]
    assert (np.abs(Cs - C) / scale).max() > 1000 * (np.abs(C32 - C) / scale).max()


# ---- "uniform" is the top-hat window ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def particle_pair(seed, H=160, W=176):
    return EM.scene(seed, H, W, density=0.03)


@pytest.mark.parametrize("ws,ov", [(64, 32), (32, 16), (32, 24), (16, 8)])
def test_uniform_first_pass_is_the_oracles(ws, ov):
    for seed in (0, 1):
        a, b = particle_pair(seed)
        ou, ov_, _, _, oinv = O.pass1(a, b, ws, ov, validate=True)
        u, v, inv = WM.pass1(a, b, ws, ov, "uniform")
        assert np.array_equal(inv, oinv.astype(bool))
        worst = max(np.abs(u - ou).max(), np.abs(v - ov_).max())
        assert worst <= GATE_PX, (ws, ov, seed, worst)


@pytest.mark.parametrize("mode", ["CWS", "DWS"])
@pytest.mark.parametrize("ws,ov", [(64, 32), (32, 16)])
def test_uniform_shifted_pass_is_the_oracles(mode, ws, ov):
    """The oracle's float32 shifted pass behind its own first pass against the model's "uniform" pass at the same
    predictor: 1e-3 px, identical validity."""
    for seed in (0, 1):
        a, b = particle_pair(seed)
        u1, v1, x, y, inv1 = O.pass1(a, b, ws, ov, validate=True)
        wf, of = ws // 2, ov // 2
        it = O.ITER[mode](a.shape, wf, of)
        ou, ov_, _, _, oinv = it(a, b, x, y, u1.copy(), v1.copy(), inv1.copy())
        u0, v0, u2, v2 = EM.predictor(mode, a.shape, ws, ov, wf, of, u1, v1, inv1)
        u, v, inv = WM.iterate(mode, a, b, wf, of, u0, v0, u2, v2, "uniform")
        assert np.array_equal(inv, oinv.astype(bool)), (mode, ws, seed)
        worst = max(np.abs(u - ou).max(), np.abs(v - ov_).max())
        assert worst <= GATE_PX, (mode, ws, seed, worst)


# ---- empty windows --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", ["gaussian", "uniform", {"sigma": (0.3, 0.6)}], ids=str)
def test_constant_zero_and_masked_windows_are_empty_by_exact_equality(weighting):
    """A zero window, a constant one at grey level 90 and a window whose pixels a mask has zeroed are empty in float32 and
    in float64 by exact equality, in the first pass and in a shifted one; the live window beside them is not."""
    ws = 32
    rng = np.random.default_rng(5)
    live = rng.integers(0, 256, (ws, ws)).astype(np.float64)
    wa = np.stack([live, np.zeros((ws, ws)), np.full((ws, ws), 90.0), live * 0.0, live])
    wb = np.stack([live, live, live, live, np.full((ws, ws), 90.0)])
    W = WM.weight(ws, weighting)
    for f32 in (False, True):
        for first in (True, False):
            x, e = WM.weighted_windows(wa, W, first, f32)
            assert list(e.numpy()) == [False, True, True, True, False]
            assert not x[1:4].numpy().any()
            C, empty = WM.weighted_map(wa, wb, W, first, f32)
            assert np.isfinite(C).all() and list(empty) == [False, True, True, True, True]
            assert not C[1:].any()
            du, dv, inv = WM.peaks(C, empty, 0 if first else "CWS", 5, 1)
            if first:
                assert not inv[1:].any() and not du[1:].any() and not dv[1:].any()      # dead: u = v = 0, valid
            else:
                assert inv[1:].all() and not inv[0]                                      # the zero map's peak ratio


def test_without_the_plain_mean_a_constant_window_is_rounding_noise():
    """What step 2 is for: the W-weighted mean of a constant window at grey level 90, formed in float32 without removing the
    plain mean first, is not 90 -- the remainder has an energy of the size of the rounding, and its peak ratio is arbitrary.
    With step 2 the remainder is exactly 0."""
    for ws in (16, 32, 64):
        W = WM.weight(ws, "gaussian")
        w = np.full((ws, ws), 90.0, dtype=np.float32)
        # (float32 sums in sequence, as a chain of fused multiply-adds forms them: np.cumsum does not re-associate)
        num = np.cumsum((W * w).ravel(), dtype=np.float32)[-1]
        den = np.cumsum(W.ravel(), dtype=np.float32)[-1]
        direct = W * (w - np.float32(num / den))
        assert float((direct * direct).sum()) > 0.0, ws
        x, e = WM.weighted_windows(w[None], W, False, f32=True)
        assert bool(e[0]) and not x.numpy().any()


def test_weighted_signal_has_no_dc():
    """Step 3: sum x = 0, so the map has no W * W pedestal -- its mean over the cells is 0."""
    a, b = particle_pair(0)
    wa, wb = WM.windows(0, a, b, 32, 16)
    W = WM.weight(32, "gaussian")
    x, _ = WM.weighted_windows(wa, W, True)
    assert np.abs(x.numpy().sum(axis=(1, 2))).max() <= 1e-12 * np.abs(x.numpy()).sum(axis=(1, 2)).max()
    C, _ = WM.weighted_map(wa, wb, W, True)
    assert np.abs(C.mean(axis=(1, 2))).max() <= 1e-12 * np.abs(C).max()


# ---- what it buys ---------------------------------------------------------------------------------------------------
H = W_ = 256
WS, OV = 32, 24


@functools.lru_cache(maxsize=None)
def scored(seed, weighting, rounds):
    a, b = DM.scene(seed, H, W_)
    u, v, inv = WM.pass1(a, b, WS, OV, weighting)
    if rounds:
        u, v, inv = WM.deform_rounds(a, b, u, v, inv, WS, OV, rounds, weighting, "cubic", True)
    tu, tv = DM.truth(H, W_, WS, OV)
    return DM.rms_interior(u, v, tu, tv, ~np.asarray(inv).astype(bool))


@pytest.mark.parametrize("seed", [0, 1])
def test_gaussian_first_pass_has_at_most_0p6_of_the_uniform_rms(seed):
    (g, gs), (t, ts) = scored(seed, "gaussian", 0), scored(seed, "uniform", 0)
    print(f"  seed {seed}: 32/24 first pass RMS uniform {t:.3f} px ({ts:.1%} of the interior cells valid), gaussian 0.4 "
          f"{g:.3f} px ({gs:.1%}), ratio {g / t:.2f}")
    report(section="model first pass 32/24", seed=seed, uniform_rms_px=t, gaussian_rms_px=g, ratio=g / t,
           uniform_valid=ts, gaussian_valid=gs)
    assert gs >= 0.95 and ts >= 0.95
    assert g <= 0.6 * t, (seed, g, t)


@pytest.mark.parametrize("seed", [0, 1])
def test_gaussian_after_three_rounds_has_at_most_0p7_of_the_uniform_rms(seed):
    (g, gs), (t, ts) = scored(seed, "gaussian", 3), scored(seed, "uniform", 3)
    print(f"  seed {seed}: 32/24 + 3 rounds (cubic, smooth) RMS uniform {t:.3f} px ({ts:.1%} valid), gaussian 0.4 {g:.3f} px "
          f"({gs:.1%}), ratio {g / t:.2f}")
    report(section="model 32/24 + 3 rounds", seed=seed, uniform_rms_px=t, gaussian_rms_px=g, ratio=g / t,
           uniform_valid=ts, gaussian_valid=gs)
    assert gs >= 0.95 and ts >= 0.95
    assert g <= 0.7 * t, (seed, g, t)
