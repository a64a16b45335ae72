"""numpy model of the paired half inverse of the tile kernels (TPIV_HALF_INV, xcorr_tile.hpp).

After the forward column transform lane r of a window holds spectrum column r.  The lanes of columns c and -c (partner
lane (W - r) mod W) share one column's worth of information, since P(-ky, -kx) = conj P(ky, kx):
  * every lane forms its own cross-spectrum products for ky = 0 .. W/2 only, from its own Z(ky) and the partner's Z(-ky);
  * it takes the partner's P(W/2 - k), whose conjugate is its own P(k + W/2), and runs ONE radix-2 decimation-in-frequency
    level over ky:  lanes 1 .. W/2-1 keep  P(k) + P(k + W/2)  (rows 2m of their column), lanes W/2+1 .. W-1 keep
    w^k (P(k) - P(k + W/2))  (rows 2m + 1 of column -c = the conjugate of column c's), w = exp(2 pi i / W);
  * lanes 0 and W/2 are their own partners; their columns are real, so they take the c2r form
    (P(k) + conj P(W/2 - k)) + i w^k (P(k) - conj P(W/2 - k))  and their W/2-point result is t(2m) + i t(2m + 1);
  * one W/2-point inverse transform per lane, the half transposition puts the odd rows of column c (conjugated back) and
    the real columns 0 and W/2 in place, and the c2r row transform finishes the map.
The model follows the kernel's arithmetic (cross-spectrum formula, the float32 twiddle literals, one rounding per
operation) and is checked against numpy's float64 irfft2, exactly in float64 and inside the proven bound in float32.
"""
import os

import numpy as np
import pytest

from test_exact_scheme import band_coef, e_plus


def cross(zk, zm):
    """4 conj(A) B of the packed bins z_k = a + ib, z_-k = c + id (the kernel's formula, in the inputs' precision)."""
    a, b, c, d = zk.real, zk.imag, zm.real, zm.imag
    return ((a * d + b * c) * 2) + 1j * ((c * c - a * a) + (d * d - b * b))


def paired_map(xa, xb, dt):
    """The circular cross-correlation map (n, W, W) [y, x] of the (already normalised) windows xa, xb through the paired
    half inverse, in precision dt (float32: every step rounds to float32)."""
    ct = np.complex64 if dt == np.float32 else np.complex128
    n, W, _ = xa.shape
    M = W // 2
    z = (xa.astype(dt) * dt(0.5 / W)) + 1j * (xb.astype(dt) * dt(0.5 / W))      # the kernel's 0.5 / W on both inputs
    Z = np.fft.fft2(z.astype(ct))                                              # [ky, kx]
    lanes = np.arange(W)
    partner = (W - lanes) % W
    ky = np.arange(M + 1)
    zk = Z[:, ky][:, :, lanes]                         # own Z(ky, c), ky = 0 .. W/2
    zm = Z[:, (-ky) % W][:, :, partner]                # the partner's Z(-ky, -c)
    P = cross(zk, zm).astype(ct)                       # (n, W/2 + 1, lane)
    k = np.arange(M)
    R = P[:, M - k][:, :, partner]                     # the partner's P(W/2 - k) = conj P(k + W/2)
    s = P[:, :M] + np.conj(R)
    d = P[:, :M] - np.conj(R)
    w = np.exp(2j * np.pi * k / W).astype(ct)          # correctly rounded literals in float32
    T = w[None, :, None] * d
    odd = lanes > M
    self_ = ((lanes == 0) | (lanes == M)).astype(dt)
    h = np.where(odd[None, None, :], T, s + self_[None, None, :] * (1j * T))
    out = (np.fft.ifft(h, axis=1) * dt(M)).astype(ct)  # unnormalised W/2-point inverse: (n, m, lane)
    # half transposition: row y, columns 0 .. W/2
    t = np.zeros((n, W, M + 1), ct)
    c = np.arange(1, M)
    t[:, 0::2, 1:M] = out[:, :, c]
    t[:, 1::2, 1:M] = np.conj(out[:, :, W - c])
    for c0 in (0, M):
        t[:, 0::2, c0] = out[:, :, c0].real
        t[:, 1::2, c0] = out[:, :, c0].imag
    return np.fft.irfft(t, n=W, axis=2) * dt(W)


def reference_map(xa, xb):
    return np.fft.irfft2(np.conj(np.fft.rfft2(xa)) * np.fft.rfft2(xb), s=xa.shape[1:])


@pytest.mark.parametrize("W", [16, 32, 64])
def test_paired_half_inverse_is_the_inverse_transform(W):
    """float64: the lane pairs, the half products, the DIF split, the conjugated odd rows and the c2r form of columns 0
    and W/2 give the same map as numpy's irfft2 to float64 rounding."""
    rng = np.random.default_rng(W)
    xa = rng.standard_normal((6, W, W))
    xb = rng.standard_normal((6, W, W))
    xb[1] = np.roll(xa[1], (3, -5), axis=(0, 1))            # a sharp peak
    xa[2] = 1.0                                              # a constant window: zero map apart from the DC bin
    got = paired_map(xa, xb, np.float64)
    want = reference_map(xa, xb)
    scale = np.abs(want).max(axis=(1, 2), keepdims=True) + 1e-300
    assert (np.abs(got - want) / scale).max() < 1e-13


@pytest.mark.parametrize("W", [16, 32, 64])
def test_each_lane_role_alone(W):
    """A spectrum that lives in one column pair only exercises one lane role at a time (column c and -c, and the two
    self-mirrored columns 0 and W/2 separately)."""
    M = W // 2
    rng = np.random.default_rng(100 + W)
    for c in (0, 1, M - 1, M):
        xa = np.zeros((1, W, W))
        xb = np.zeros((1, W, W))
        xx = np.arange(W)
        for arr in (xa, xb):
            col = rng.standard_normal(W)
            arr[0] = col[:, None] * np.cos(2 * np.pi * c * xx / W + rng.uniform(0, 2 * np.pi))[None, :]
        got = paired_map(xa, xb, np.float64)
        want = reference_map(xa, xb)
        assert np.abs(got - want).max() <= 1e-13 * (np.abs(want).max() + 1e-300), (W, c)


def test_float32_paired_map_inside_the_proven_bound():
    """float32: |map32 - map| <= Gamma E+ with the same eighth of Gamma to spare the GPU test asks of the
    kernel, on the adversarial windows of tests/golden/g12_adversarial.npz (hill-climbed on the full-form kernel's error)
    and on random ones: one radix-2 level plus a W/2-point transform is log2 W levels, the twiddles are correctly rounded
    literals, and the self-mirrored columns take the c2r form the row transform already uses."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_adversarial.npz"))
    gamma = band_coef(64) / (2 * (1 + 1 / 16))
    rng = np.random.default_rng(11)
    fams = [g[f"w{i}"] for i in range(len(g["names"]))] + [rng.integers(0, 256, (4, 2, 64, 64)).astype(np.uint8)]
    worst = 0.0
    for P in fams:
        keep = [(a, b) for a, b in P if a.sum() > 0 and b.sum() > 0]
        a = np.stack([p[0] for p in keep])
        b = np.stack([p[1] for p in keep])
        af, bf = a.astype(np.float32), b.astype(np.float32)
        ma = af.mean(axis=(1, 2), keepdims=True, dtype=np.float32)
        mb = bf.mean(axis=(1, 2), keepdims=True, dtype=np.float32)
        c32 = paired_map((af - ma) / ma, (bf - mb) / mb, np.float32).astype(np.float64)
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        c64 = reference_map(a64 / a64.mean(axis=(1, 2), keepdims=True) - 1, b64 / b64.mean(axis=(1, 2), keepdims=True) - 1)
        e = (c32 - c64).reshape(len(a), -1)
        ratio = 0.5 * (e.max(axis=1) - e.min(axis=1)) / np.array([e_plus(x, y) for x, y in zip(a, b)])
        worst = max(worst, float(ratio.max()))
    assert 0 < worst < gamma / 8, (worst, gamma)
