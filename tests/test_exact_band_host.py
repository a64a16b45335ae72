"""The constants of the "exact" first pass's decision band (piv_kernels.h "The band"), on the host.

(1) The Python mirror of Gamma(ws, kind) in tests/test_exact_scheme.py is the C++ exact_gamma_u / exact_band_coef the
launcher uses, for every even window size 8 ... 128 and each of the three kinds of transform.
(2) The per-transform error claims Gamma is built from hold for the codelets the locating kernels run: the normwise relative
error of one 1-D transform stays below F u -- F = eta log2 n for the radix-2/4 codelets of fft_inreg.hpp (complex, both
directions, and the real inverse c2r_inreg), F = 64 for the two-factor mixed-radix codelets of fft_mixed.hpp -- on a few
hundred random and structured lines per size.  (The GPU side, tests/test_gpu_exact_band.py, checks the whole map.)
"""
import os
import subprocess

import numpy as np
import pytest

from test_exact_scheme import ETA, KINDS, U32, band_coef, gamma_u, kind_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "torchpiv_amd", "csrc")
SIZES = list(range(8, 129, 2))
MIXED = [n for n in SIZES if kind_of(n) == "mixed"]
RADIX2 = [8, 16, 32, 64, 128]


def test_kinds_cover_every_exact_size():
    kinds = {n: kind_of(n) for n in SIZES}
    assert [n for n in SIZES if kinds[n] == "radix2"] == RADIX2
    assert MIXED == [10, 12, 14, 18, 20, 24, 28, 30, 36, 40, 42, 48, 56]
    assert sum(k == "plain" for k in kinds.values()) == 43


def test_gamma_mirror_equals_the_launcher_constants(tmp_path):
    src = tmp_path / "g.cpp"
    src.write_text(r"""
#include "piv_kernels.h"
#include <cstdio>
int main() {
  for (int ws = 8; ws <= 128; ws += 2)
    for (int k = 0; k < 3; ++k)
      printf("%d %d %.17g %.9g\n", ws, k, tpiv::exact_gamma_u(ws, k), (double)tpiv::exact_band_coef(ws, k));
}
""")
    exe = tmp_path / "g"
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, str(src),
                    "-o", str(exe)], check=True)
    rows = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    rows = [r.split() for r in rows if r]
    assert len(rows) == len(SIZES) * 3
    for ws_, k_, g_, b_ in rows:
        ws, k = int(ws_), int(k_)
        g = gamma_u(ws, KINDS[k])
        assert float(g_) == g, (ws, KINDS[k], float(g_), g)
        assert np.float32(float(b_)) == np.float32(2.0 * g * (1 + 1 / 16) * U32), (ws, KINDS[k])
    for ws in RADIX2:                                  # band_coef (the callers of the radix-2-only form) is the same number
        assert abs(band_coef(ws) - 2.0 * gamma_u(ws, "radix2") * (1 + 1 / 16) * U32) < 1e-15 * band_coef(ws)


HARNESS = r"""
#include "fft_mixed.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace tpiv;
// stdin: count lines of n complex float32 (n / 2 + 1 bins for c2r); stdout: the transforms, natural order (c2r: n reals)
template <int N, int DIR> void mixed(int count) {
  for (int l = 0; l < count; ++l) {
    cf x[N];
    if (fread(x, sizeof(cf), N, stdin) != (size_t)N) exit(2);
    fmx::fft_mixed<N, DIR>(x);
    for (int k = 0; k < N; ++k) fwrite(&x[fmx::mixed_pos(k, N)], sizeof(cf), 1, stdout);
  }
}
template <int N, int DIR> void radix2(int count) {
  for (int l = 0; l < count; ++l) {
    cf x[N];
    if (fread(x, sizeof(cf), N, stdin) != (size_t)N) exit(2);
    fft_inreg<N, DIR>(x);
    for (int k = 0; k < N; ++k) fwrite(&x[fft_pos(k, N)], sizeof(cf), 1, stdout);
  }
}
template <int N> void c2r(int count) {
  for (int l = 0; l < count; ++l) {
    cf y[N / 2 + 1], h[N / 2];
    if (fread(y, sizeof(cf), N / 2 + 1, stdin) != (size_t)(N / 2 + 1)) exit(2);
    c2r_inreg<N>(y, h);
    for (int m = 0; m < N / 2; ++m) fwrite(&h[fft_pos(m, N / 2)], sizeof(cf), 1, stdout);
  }
}
int main(int argc, char** argv) {
  const char k = argv[1][0];
  const int n = atoi(argv[2]), dir = atoi(argv[3]), count = atoi(argv[4]);
#define M(NN) if (k == 'm' && n == NN) { if (dir > 0) mixed<NN, 1>(count); else mixed<NN, -1>(count); return 0; }
#define R(NN) if (k == 'r' && n == NN) { if (dir > 0) radix2<NN, 1>(count); else radix2<NN, -1>(count); return 0; } \
              if (k == 'c' && n == NN) { c2r<NN>(count); return 0; }
  SIZES
  return 1;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("codelets")
    sizes = " ".join(f"M({n})" for n in MIXED) + " " + " ".join(f"R({n})" for n in RADIX2)
    src = d / "h.cpp"
    src.write_text(HARNESS.replace("SIZES", sizes))
    exe = d / "h"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


def lines(n, seed):
    """A few hundred float32 complex lines of length n: random and structured (what the locating kernels transform: packed
    a' + i b' of mean-normalised windows, and spectra), as complex128 holding the float32 values exactly."""
    rng = np.random.default_rng(seed)
    j = np.arange(n)
    out = [rng.normal(size=(64, n)) + 1j * rng.normal(size=(64, n)),
           rng.uniform(-1, 1, (32, n)) * 1e3 + 1j * rng.uniform(-1, 1, (32, n)) * 1e-3]          # unequal parts
    by = rng.integers(0, 256, (64, 2, n)).astype(np.float64) + 1.0
    by = by / by.mean(axis=2, keepdims=True) - 1                                                  # a / mean(a) - 1
    out.append(by[:, 0] + 1j * by[:, 1])
    lo = rng.integers(100, 104, (32, 2, n)).astype(np.float64)
    lo = lo / lo.mean(axis=2, keepdims=True) - 1
    out.append(lo[:, 0] + 1j * lo[:, 1])
    k = np.arange(n)[:, None]
    out.append(np.exp(2j * np.pi * k * j[None] / n))                                              # one bin each
    out.append(np.cos(2 * np.pi * k * j[None] / n) + 1j * np.sin(2 * np.pi * (k + 1) * j[None] / n + 0.3))
    imp = np.zeros((n, n), complex)
    imp[j, j] = 1.0 + 0.5j                                                                        # one sample each
    out.append(imp)
    out.append(np.ones((1, n)) + 0j)
    out.append(((-1.0) ** j)[None] + 1j * (j[None] % 3 - 1.0))
    out.append(np.where(rng.random((32, n)) < 0.05, 254.0, 1.0) + 1j * np.where(rng.random((32, n)) < 0.95, 254.0, 1.0))
    x = np.concatenate(out).astype(np.complex64)
    return x.astype(np.complex128)


def run(exe, kind, n, d, x):
    cnt = len(x)
    buf = np.ascontiguousarray(x.astype(np.complex64)).tobytes()
    out = subprocess.run([exe, kind, str(n), str(d), str(cnt)], input=buf, capture_output=True, check=True).stdout
    return np.frombuffer(out, np.complex64).astype(np.complex128).reshape(cnt, -1)


def normwise(got, want):
    nw = np.linalg.norm(want, axis=1)
    keep = nw > 0
    return (np.linalg.norm(got - want, axis=1)[keep] / nw[keep]).max()


@pytest.mark.parametrize("n", MIXED)
def test_mixed_radix_codelet_error_below_64_u(harness, n):
    """fft_mixed.hpp, forward and inverse: normwise relative error <= 64 u (the F = I of EXACT_FFT_MIXED)."""
    x = lines(n, n)
    worst = 0.0
    for d in (1, -1):
        got = run(harness, "m", n, d, x)
        want = np.fft.fft(x, axis=1) if d > 0 else np.fft.ifft(x, axis=1) * n
        worst = max(worst, normwise(got, want) / U32)
    print(f"  mixed {n}: worst normwise error {worst:.1f} u against F = 64 u")
    assert 0 < worst <= 64, (n, worst)


@pytest.mark.parametrize("n", RADIX2)
def test_radix2_codelet_error_below_eta_log2n_u(harness, n):
    """fft_inreg.hpp, forward and inverse complex transforms and the real inverse c2r_inreg (the tile kernels' last
    transform): normwise relative error <= eta log2 n u (the F = I of EXACT_FFT_RADIX2)."""
    F = ETA * np.log2(n)
    x = lines(n, 1000 + n)
    worst = 0.0
    for d in (1, -1):
        got = run(harness, "r", n, d, x)
        want = np.fft.fft(x, axis=1) if d > 0 else np.fft.ifft(x, axis=1) * n
        worst = max(worst, normwise(got, want) / U32)
    # c2r: a Hermitian half spectrum in (imaginary parts of the DC and Nyquist bins ignored), n reals out
    y = np.fft.rfft(x.real, axis=1)
    y = y.astype(np.complex64).astype(np.complex128)
    y[:, 0] = y[:, 0].real
    y[:, -1] = y[:, -1].real
    h = run(harness, "c", n, 0, y)
    got = np.empty((len(y), n))
    got[:, 0::2], got[:, 1::2] = h.real, h.imag
    worst_c2r = normwise(got, np.fft.irfft(y, n, axis=1) * n) / U32
    print(f"  radix-2 {n}: worst normwise error {worst:.1f} u (complex), {worst_c2r:.1f} u (c2r) against F = {F:.1f} u")
    assert 0 < worst <= F and 0 < worst_c2r <= F, (n, worst, worst_c2r, F)
