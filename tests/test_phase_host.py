"""The spectrally filtered passes (correlation="phase" / "rpc") on the CPU: the float64 model of tests/phase_model.py against
its own definition (pure shifts, the floor), what the filter buys on frames with a shared static pattern, and every form and
refusal of the correlation= argument -- all without a GPU."""
import functools

import numpy as np
import pytest

from oracle import piv_oracle as O
import ensemble_model as EM
import phase_model as PM

SEEDS = (0, 1, 2)
H = W = 256
RPC = "rpc"          # diameter 2.8


# ---- pure circular shift --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ws", [16, 32, 64])
@pytest.mark.parametrize("d", [(0.0, 0.0), (2.8, 2.8), (2.0, 4.0)], ids=str)
def test_pure_circular_shift(ws, d):
    """A window pair that is a pure circular shift by integer (sx, sy): C is the inverse transform of W moved to the shift,
    its peak sum W sits at the shift, to 1e-9 relative.  (Up to the DC bin: the windows are mean-free, so Q(0, 0) = 0 where
    W(0, 0) = 1 -- every cell of C is lower by exactly 1, which C - min C does not see.)  The exact statement needs a window
    with no bin below the floor: an impulse, whose spectrum has magnitude 1 everywhere; on a random window only the place
    of the peak is asserted."""
    rng = np.random.default_rng(ws)
    imp = np.zeros((1, ws, ws))
    imp[0, 3, 5] = 200.0
    rnd = rng.integers(0, 256, (1, ws, ws)).astype(np.float64)
    dx, dy = d
    Winv = np.fft.fftshift(np.fft.ifft2(PM.weight(ws, dx, dy).astype(np.float64)).real * ws * ws)
    top = PM.peak_scale(ws, dx, dy)
    assert abs(Winv[ws // 2, ws // 2] - top) <= 1e-12 * top
    for sx, sy in ((0, 0), (3, -2), (-5, 1), (ws // 2 - 1, -(ws // 2) + 1)):
        for wa, exact in ((imp, True), (rnd, False)):
            wb = np.roll(wa, (sy, sx), axis=(1, 2))
            C, empty = PM.filtered_map(wa, wb, dx, dy)
            assert not empty.any()
            my, mx = np.unravel_index(np.argmax(C[0]), C[0].shape)
            assert (my - ws // 2, mx - ws // 2) == (sy, sx)
            if exact:
                want = np.roll(Winv, (sy, sx), axis=(0, 1))
                assert np.abs((C[0] + 1.0) - want).max() <= 1e-9 * top
                assert abs((C[0, my, mx] + 1.0) - top) <= 1e-9 * top


def test_anisotropic_weight_widens_one_axis_only():
    """(d_x, d_y) = (2, 4): by the definition g_y is built from d_y and multiplies ky, the larger diameter damps the ky
    spectrum more, so the map is wider along y than along x -- and (4, 2) the other way round, by the same amounts: a swap
    of the two frequency axes shows."""
    ws = 32
    wa = np.zeros((1, ws, ws))
    wa[0, 7, 9] = 200.0              # an impulse: no bin below the floor, the map is the inverse transform of W itself

    def widths(dx, dy):
        C, _ = PM.filtered_map(wa, wa, dx, dy)
        c = C[0] - C[0].min()
        m = ws // 2
        return c[m, m + 1] / c[m, m], c[m + 1, m] / c[m, m]       # first neighbour along x, along y
    x24, y24 = widths(2.0, 4.0)
    x42, y42 = widths(4.0, 2.0)
    assert y24 > x24 and x42 > y42
    assert abs(x24 - y42) < 1e-12 and abs(y24 - x42) < 1e-12


# ---- the floor ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ws", [16, 32, 64])
def test_floor_makes_float32_agree_on_periodic_windows(ws):
    """Noise-free stripes of period 16 (exact zeros in most bins): the complex64 evaluation gives the validity and the
    arg-max of the float64 one, and stays within 1e-6 of the peak scale."""
    Hs = Ws = 4 * ws
    s = PM.stripes(Hs, Ws, period=16, level=60.0)
    a, _ = EM.scene(3, Hs, Ws, density={16: 0.06, 32: 0.03, 64: 0.015}[ws], noise=0.0, offset=0.0)
    for fa, fb in ((s, np.roll(s, 2, axis=1)), (s + a, np.roll(s + a, (1, 3), axis=(0, 1)))):
        fa, fb = np.clip(fa, 0, 255).astype(np.uint8), np.clip(fb, 0, 255).astype(np.uint8)
        wa, wb = PM.windows(0, fa, fb, ws, ws // 2)
        for d in ((0.0, 0.0), (2.8, 2.8)):
            C64, e64 = PM.filtered_map(wa, wb, *d)
            C32, e32 = PM.filtered_map(wa, wb, *d, f32=True)
            assert np.isfinite(C32).all() and np.array_equal(e64, e32)
            n = len(C64)
            f64 = PM.peaks(C64, e64, 0, n, 1)
            f32 = PM.peaks(C32, e32, 0, n, 1)
            assert np.array_equal(f64[2], f32[2])
            assert np.array_equal(C64.reshape(n, -1).argmax(axis=1), C32.reshape(n, -1).argmax(axis=1))
            assert np.abs(C32 - C64).max() <= 1e-6 * PM.peak_scale(ws, *d)


def test_empty_windows_give_the_zero_map_and_no_nan():
    ws = 32
    rng = np.random.default_rng(1)
    wa = rng.integers(0, 256, (3, ws, ws)).astype(np.float64)
    wb = wa.copy()
    wa[0] = 0.0
    wb[1] = 77.0
    for f32 in (False, True):
        C, empty = PM.filtered_map(wa, wb, 2.8, 2.8, f32=f32)
        assert np.isfinite(C).all() and list(empty) == [True, True, False]
        assert not C[0].any() and not C[1].any()
        du, dv, inv = PM.peaks(C, empty, 0, 3, 1)
        assert not inv[:2].any() and not du[:2].any() and not dv[:2].any()            # first pass: dead, u = v = 0, valid
        du, dv, inv = PM.peaks(C, empty, "CWS", 3, 1)
        assert inv[:2].all() and not inv[2]                                          # shifted pass: the peak ratio says invalid


# ---- what it buys ---------------------------------------------------------------------------------------------------
CHAINS = {                      # name: (ws, ov, n_pass, mode, density)
    "64/32": (64, 32, 1, "CWS", 0.015),
    "32/16": (32, 16, 1, "CWS", 0.03),
    "64/32->32/16 CWS": (64, 32, 2, "CWS", 0.03),
    "64/32->32/16 DWS": (64, 32, 2, "DWS", 0.03),
    "32/16->16/8 CWS": (32, 16, 2, "CWS", 0.06),
}


@functools.lru_cache(maxsize=None)
def scored(name, seed, correlation):
    ws, ov, n_pass, mode, density = CHAINS[name]
    a, b = PM.striped_scene(seed, H, W, density=density)
    u, v, inv = PM.chain(a, b, ws, ov, n_pass, mode, correlation)[-1]
    wl, ol = ws >> (n_pass - 1), ov >> (n_pass - 1)
    return PM.score(u, v, inv, H, W, wl, ol)


@pytest.mark.parametrize("name", list(CHAINS))
def test_rpc_leaves_no_invalid_vector_on_striped_frames(name):
    for seed in SEEDS:
        n_inv, n_far, rms = scored(name, seed, RPC)
        print(f"  {name:18s} seed {seed}: rpc {n_inv} invalid, {n_far} more than 1 px off, RMS {rms:.3f} px")
        assert n_inv == 0 and n_far == 0, (name, seed, n_inv, n_far)


def test_plain_correlation_loses_vectors_to_the_stripes():
    for seed in SEEDS:
        n64 = scored("64/32", seed, None)[0]
        n32 = scored("32/16", seed, None)[0]
        print(f"  seed {seed}: plain 64/32 {n64} of 49 invalid, 32/16 {n32} of 225")
        assert n64 >= 28 and n32 >= 24, (seed, n64, n32)


def test_rpc_chain_is_four_times_closer_than_the_plain_one():
    name = "64/32->32/16 CWS"
    for seed in SEEDS:
        plain, rpc = scored(name, seed, None)[2], scored(name, seed, RPC)[2]
        print(f"  seed {seed}: {name} RMS plain {plain:.3f} px, rpc {rpc:.3f} px, ratio {rpc / plain:.2f}")
        assert rpc <= 0.25 * plain, (seed, rpc, plain)


# ---- arguments and refusals -----------------------------------------------------------------------------------------
def test_every_form_of_the_keyword():
    from torchpiv_amd import engine
    assert engine.correlation_arg(None) is None
    assert engine.correlation_arg("phase") == {"kind": "phase", "dx": 0.0, "dy": 0.0, "floor": 2.0 ** -10}
    assert engine.correlation_arg("rpc") == {"kind": "rpc", "dx": 2.8, "dy": 2.8, "floor": 2.0 ** -10}
    assert engine.correlation_arg({"kind": "rpc"}) == engine.correlation_arg("rpc")
    assert engine.correlation_arg({}) == engine.correlation_arg("rpc")
    assert engine.correlation_arg({"kind": "rpc", "diameter": 3}) == {"kind": "rpc", "dx": 3.0, "dy": 3.0, "floor": 2.0 ** -10}
    assert engine.correlation_arg({"diameter": (2.0, 4.0), "floor": 2.0 ** -8}) == \
        {"kind": "rpc", "dx": 2.0, "dy": 4.0, "floor": 2.0 ** -8}
    assert engine.correlation_arg({"kind": "phase", "floor": 2.0 ** -4})["floor"] == 2.0 ** -4
    assert engine.correlation_arg({"diameter": 0})["dx"] == 0.0 and engine.correlation_arg({"diameter": 16})["dy"] == 16.0
    for bad in ("spof", "RPC", 1, 2.8, ("rpc",), {"kind": "gauss"}, {"kind": None}, {"diameter": -0.1}, {"diameter": 16.5},
                {"diameter": (1.0, 17.0)}, {"diameter": (1.0, 2.0, 3.0)}, {"diameter": "wide"}, {"diameter": True},
                {"floor": 2.0 ** -21}, {"floor": 0.1}, {"floor": None}, {"floor": float("nan")}, {"radius": 3},
                {"kind": "phase", "diameter": 2.0}, {"diameter": float("nan")}):
        with pytest.raises(ValueError):
            engine.correlation_arg(bad)


def test_tables_are_float64_exp_rounded_once():
    from torchpiv_amd import engine
    par = engine.correlation_arg({"diameter": (2.0, 4.0)})
    tab = engine.correlation_tables(par, [64, 32])
    assert tab.dtype == np.float32 and tab.size == 2 * 33 + 2 * 17
    assert np.array_equal(tab[:33], PM.table(64, 4.0)) and np.array_equal(tab[33:66], PM.table(64, 2.0))       # g_y, then g_x
    assert np.array_equal(tab[66:83], PM.table(32, 4.0)) and np.array_equal(tab[83:], PM.table(32, 2.0))
    ones = engine.correlation_tables(engine.correlation_arg("phase"), [16])
    assert np.array_equal(ones, np.ones(18, np.float32))


def test_refusals_without_a_gpu():
    import torch
    from torchpiv_amd import backend, engine, runner
    for ws, n_pass in ((8, 1), (128, 1), (24, 1), (32, 3)):            # 32 -> 16 -> 8: a chain that reaches 8
        sizes = [w for w, _ in engine.pass_sizes(ws, ws // 2, n_pass, 2.0)]
        with pytest.raises(NotImplementedError, match=str([s for s in sizes if s not in (16, 32, 64)][0])):
            engine.correlation_check(sizes)
        with pytest.raises(NotImplementedError):
            engine.Plan(256, 256, ws, ws // 2, n_pass=n_pass, correlation="rpc")
    engine.correlation_check([64, 32, 16], "CWS")
    with pytest.raises(NotImplementedError, match="CWS_Fast"):
        engine.correlation_check([32], "CWS_Fast")
    with pytest.raises(ValueError, match="uncertainty"):
        engine.Plan(160, 160, 32, 16, correlation="rpc", uncertainty="cs")
    with pytest.raises(ValueError, match="deform"):
        engine.Plan(160, 160, 32, 16, correlation="phase", deform=1)
    with pytest.raises(ValueError, match="ensemble"):
        engine.Plan(160, 160, 32, 16, correlation="rpc", ensemble=True)
    with pytest.raises(ValueError):
        engine.Plan(160, 160, 32, 16, correlation="spof")
    with pytest.raises(ValueError):
        engine.Plan(160, 160, 32, 16, correlation={"floor": 1.0})
    # the host classes check in the constructor, before any GPU call (CPU tensors: the GPU is asked for last)
    z = torch.zeros(2, 96, 96, dtype=torch.uint8)
    with pytest.raises(ValueError):
        backend.ResidentPIV(z, z, 32, 16, correlation="spof")
    with pytest.raises(ValueError):
        backend.ResidentPIV(z, z, 32, 16, correlation={"diameter": 20})
    with pytest.raises(NotImplementedError, match="8"):
        backend.ResidentPIV(z, z, 16, 8, multipass=2, correlation="rpc")
    with pytest.raises(ValueError, match="uncertainty"):
        backend.ResidentPIV(z, z, 32, 16, correlation="rpc", uncertainty="cs")
    with pytest.raises(ValueError, match="deform"):
        backend.ResidentPIV(z, z, 32, 16, correlation="rpc", deform=2)
    with pytest.raises(ValueError):
        backend.OfflinePIV("no/such/folder", "cuda:0", "bmp", 32, 16, correlation="spof")
    with pytest.raises(NotImplementedError, match="24"):
        backend.OfflinePIV("no/such/folder", "cuda:0", "bmp", 24, 12, correlation="phase")
    with pytest.raises(ValueError):
        runner.run_folder("no/such/folder", "cuda:0", "bmp", 32, 16, correlation={"kind": "rpc", "sigma": 1})
    import inspect
    for fn in (engine.Plan.__init__, engine.debug_pass):
        assert list(inspect.signature(fn).parameters)[-1] == "correlation"
    # (the host classes and run_folder keep equalize, prefilter as their last two keywords: tests/test_equalize_host.py)
    for fn in (backend.OfflinePIV.__init__, backend.ResidentPIV.__init__, runner.run_folder):
        names = list(inspect.signature(fn).parameters)
        assert names.index("correlation") == names.index("deform") + 1
