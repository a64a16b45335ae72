"""The paired half inverse of the float32 tile kernels (TPIV_HALF_INV, xcorr_tile.hpp; numpy model in
tests/test_half_inverse_model.py) on the device: the 64 x 64 and 32 x 32 kernels' correlation maps against a float64 map
inside the float32 band, on random, particle and adversarial windows, for pass 1 and the shifted (CWS) instances, and the
default "exact" first pass against the float64 kernels on full 2048 x 2048 frames."""
import os

import numpy as np
import pytest
import torch

from oracle import piv_oracle as O
from test_exact_scheme import band_coef, e_plus

pytestmark = pytest.mark.gpu

TOL_F64 = 1e-11
GAMMA = band_coef(64) / (2 * (1 + 1 / 16))          # Gamma(64) of DESIGN.md 3.4b; Gamma(32) is smaller


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def map64(a, b):
    """float64 circular cross-correlation in the kernels' fftshift layout, minimum at 0."""
    W = a.shape[-1]
    c = np.fft.irfft2(np.conj(np.fft.rfft2(a)) * np.fft.rfft2(b), s=(W, W))
    c = np.fft.fftshift(c, axes=(-2, -1))
    return c - c.min(axis=(-2, -1), keepdims=True)


def err_ratio(got, want, scale):
    """half the spread of (got - want) per window (a common offset changes no decision) over scale."""
    e = (got.astype(np.float64) - want).reshape(len(got), -1)
    return 0.5 * (e.max(axis=1) - e.min(axis=1)) / scale


@pytest.mark.parametrize("ws", [32, 64])
def test_pass1_maps_inside_the_band(eng, ws):
    """Pass 1 ("fast" float32 kernel): mean-normalised windows; the map stays inside Gamma E+ / 8 (the margin the adversarial
    GPU test asks for) on random bytes, synthetic particle images and (64 x 64) the hill-climbed adversarial windows."""
    from torchpiv_amd import synth
    rng = np.random.default_rng(ws)
    sets = [rng.integers(0, 256, (6, 2, ws, ws)).astype(np.uint8)]
    a, b = synth.make_pair(4 * ws, 4 * ws, 70 + ws, kind="wavy", noise=2.0)
    aa, bb = O.windows(a.numpy(), ws, 0), O.windows(b.numpy(), ws, 0)
    sets.append(np.stack([aa, bb], axis=1))
    if ws == 64:
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_adversarial.npz"))
        sets += [g[f"w{i}"] for i in range(len(g["names"]))]
    worst = 0.0
    for P in sets:
        P = P[[(p[0].sum() > 0 and p[1].sum() > 0) for p in P]]
        a_, b_ = np.ascontiguousarray(P[:, 0]), np.ascontiguousarray(P[:, 1])
        _, _, _, _, corr = eng.debug_pass(0, dev(a_), dev(b_), ws, 0, precision="fast")
        got = corr.cpu().numpy().reshape(-1, ws, ws)
        af, bf = a_.astype(np.float64), b_.astype(np.float64)
        want = map64(af / af.mean(axis=(1, 2), keepdims=True) - 1, bf / bf.mean(axis=(1, 2), keepdims=True) - 1)
        ratio = err_ratio(got, want, np.array([e_plus(x, y) for x, y in zip(a_, b_)]))
        worst = max(worst, float(ratio.max()))
    print(f"  ws {ws}: worst |map32 - map| / E+ {worst:.2e} against Gamma / 8 = {GAMMA / 8:.2e}")
    assert 0 < worst < GAMMA / 8, (ws, worst)


@pytest.mark.parametrize("ws,precision", [(32, "fast"), (32, "reference"), (64, "fast")])
def test_shifted_pass_maps_inside_the_band(eng, ws, precision):
    """Shifted (CWS) passes: the map of the staged windows the kernel reports, against a float64 map of the same windows.
    These kernels transform the raw samples (the "fast" order removes the mean in the DC bin after the row transform), so
    the rounding scales with the windows' energy (|a|^2 + |b|^2) / 2 instead of E+."""
    from torchpiv_amd import synth
    H, W, ov = 6 * ws, 8 * ws, ws // 2
    a, b = synth.make_pair(H, W, 90 + ws, kind="wavy", noise=3.0)
    nr, nc = O.field_shape((H, W), ws, ov)
    rng = np.random.default_rng(5 + ws)
    vx = torch.from_numpy(rng.uniform(-3, 3, (1, nr, nc))).cuda()
    vy = torch.from_numpy(rng.uniform(-3, 3, (1, nr, nc))).cuda()
    _, _, _, win, corr = eng.debug_pass("CWS", a.cuda(), b.cuda(), ws, ov, vx, vy, precision=precision)
    wa = win[0, :, 0].cpu().numpy().astype(np.float64)
    wb = win[0, :, 1].cpu().numpy().astype(np.float64)
    got = corr[0].cpu().numpy()
    want = map64(wa - wa.mean(axis=(1, 2), keepdims=True), wb - wb.mean(axis=(1, 2), keepdims=True))
    energy = 0.5 * ((wa ** 2).sum(axis=(1, 2)) + (wb ** 2).sum(axis=(1, 2)))
    keep = energy > 0
    ratio = err_ratio(got[keep], want[keep], energy[keep])
    print(f"  ws {ws} {precision}: worst |map32 - map| / energy {ratio.max():.2e}")
    assert ratio.max() < GAMMA, (ws, precision, float(ratio.max()))


@pytest.mark.parametrize("ws", [32, 64])
def test_exact_first_pass_on_full_frames(eng, ws):
    """precision "exact" (the float32 locating kernel with the paired inverse + exact integer sums) against the float64 kernel
    on two full 2048 x 2048 pairs: the same fields to 1e-11 px and identical validity masks."""
    from torchpiv_amd import synth
    A, B = synth.make_batch(2, 2048, 2048, device="cuda", noise=2.0, first_index=300 + ws)
    ue, ve, ie = eng.pass1(A, B, ws, ws // 2, precision="exact")
    uf, vf, i_f = eng.pass1(A, B, ws, ws // 2, precision="f64")
    torch.cuda.synchronize()
    d = max(float((ue - uf).abs().max()), float((ve - vf).abs().max()))
    assert d < TOL_F64 and torch.equal(ie, i_f), (ws, d, int((ie != i_f).sum()))
