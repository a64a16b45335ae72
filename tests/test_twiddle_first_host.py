"""The twiddle-first (decimation-in-time) codelets of fft_inreg.hpp on the host, against numpy float64.

fft_twf<N, DIR> folds each twiddle product into the butterfly's additions (a + w b as two nested fma per component,
a - w b = 2a - (a + w b) as one) and leaves bin k in register fft_pos(k, N), where the shipped decimation-in-frequency form
fft_dif leaves it: the consumers (cross-spectrum, transpositions, c2r) index through FFT_POS and do not know which form ran.

Inputs, for N = 4 ... 128, both directions, both twiddle sources, and c2r_inreg<8 ... 64>:
  * an impulse at every input position: bin k of impulse j is exp(-+2 pi i j k / N), so a wrong twiddle index or a result
    in the wrong register is an O(1) error in that bin;
  * constant and alternating rows, 200 random rows;
  * the rows of the adversarial windows tests/golden/g12_adversarial.npz as the locating kernel transforms them
    (a / mean(a) - 1 + i (b / mean(b) - 1)).
Gate: normwise error <= log2 N * 6.66 u, the F = I of exact_gamma_u -- the bound the exact first pass's
band is built on; both forms stay in the header, so they must also agree with each other within it.
(Worst seen: 3.3 u at N = 128 against 46.6 u, 2.3 u at N = 64 against 40 u; profiles/twiddle_first/README.md.)
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "torchpiv_amd", "csrc")
U32 = 2.0 ** -24
ETA = 6.66
SIZES = (4, 8, 16, 32, 64, 128)
C2R_SIZES = (8, 16, 32, 64)

HARNESS = r"""
#include "fft_inreg.hpp"
#include <cstdio>
#include <cstdlib>
using namespace tpiv;
// stdin: count lines of n complex float32 (n / 2 + 1 bins for c2r); stdout: the transforms in natural order
// kind: 't' twiddle-first, literals; 'T' twiddle-first, TwRegs; 's' shipped form, literals; 'c' / 'C' c2r through the
// twiddle-first / the shipped transform
template <int N, int DIR> void cplx(char kind, int count) {
  for (int l = 0; l < count; ++l) {
    cf x[N];
    if (fread(x, sizeof(cf), N, stdin) != (size_t)N) exit(2);
    if (kind == 't') fft_twf<N, DIR>(x, TwLiteral{});
    else if (kind == 's') fft_dif<N, DIR>(x, TwLiteral{});
    else { TwRegs<N> tw; tw.init(); fft_twf<N, DIR>(x, tw); }
    for (int k = 0; k < N; ++k) fwrite(&x[fft_pos(k, N)], sizeof(cf), 1, stdout);
  }
}
template <int N> void c2r(char kind, int count) {
  for (int l = 0; l < count; ++l) {
    cf y[N / 2 + 1], h[N / 2];
    if (fread(y, sizeof(cf), N / 2 + 1, stdin) != (size_t)(N / 2 + 1)) exit(2);
    if (kind == 'c') c2r_inreg<N, true>(y, h); else c2r_inreg<N, false>(y, h);
    for (int m = 0; m < N / 2; ++m) fwrite(&h[fft_pos(m, N / 2)], sizeof(cf), 1, stdout);
  }
}
int main(int argc, char** argv) {
  const char k = argv[1][0];
  const int n = atoi(argv[2]), dir = atoi(argv[3]), count = atoi(argv[4]);
#define R(NN) if ((k == 't' || k == 'T' || k == 's') && n == NN) { if (dir > 0) cplx<NN, 1>(k, count); else cplx<NN, -1>(k, count); return 0; }
#define C(NN) if ((k == 'c' || k == 'C') && n == NN) { c2r<NN>(k, count); return 0; }
  R(4) R(8) R(16) R(32) R(64) R(128)
  C(8) C(16) C(32) C(64)
  return 1;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("twiddle_first")
    src = d / "h.cpp"
    src.write_text(HARNESS)
    exe = d / "h"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def adversarial_rows():
    """The rows of every adversarial window, normalised as the kernel's input stage does: (n_rows, 64) complex."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "g12_adversarial.npz"))
    rows = []
    for i in range(len(g["names"])):
        P = g[f"w{i}"].astype(np.float64)
        P = P[(P[:, 0].sum(axis=(1, 2)) > 0) & (P[:, 1].sum(axis=(1, 2)) > 0)]
        m = P.mean(axis=(2, 3), keepdims=True)
        Q = P / m - 1.0
        rows.append((Q[:, 0] + 1j * Q[:, 1]).reshape(-1, 64))
    return np.concatenate(rows)


def lines(n, seed, adv):
    rng = np.random.default_rng(seed)
    j = np.arange(n)
    imp = np.zeros((n, n), complex)
    imp[j, j] = 1.0
    imp2 = np.zeros((n, n), complex)
    imp2[j, j] = 0.75 - 0.5j
    flat = adv.reshape(-1)
    flat = flat[:(len(flat) // n) * n].reshape(-1, n)               # n = 128: two rows per line; n < 64: pieces of a row
    x = np.concatenate([imp, imp2, np.ones((1, n)) * (1 + 1j), ((-1.0) ** j)[None] * (1 - 2j),
                        rng.normal(size=(200, n)) + 1j * rng.normal(size=(200, n)), flat])
    return x.astype(np.complex64).astype(np.complex128)


def run(exe, kind, n, d, x):
    cnt = len(x)
    buf = np.ascontiguousarray(x.astype(np.complex64)).tobytes()
    out = subprocess.run([exe, kind, str(n), str(d), str(cnt)], input=buf, capture_output=True, check=True).stdout
    return np.frombuffer(out, np.complex64).astype(np.complex128).reshape(cnt, -1)


def normwise(got, want):
    nw = np.linalg.norm(want, axis=1)
    keep = nw > 0
    return (np.linalg.norm(got - want, axis=1)[keep] / nw[keep]).max()


@pytest.mark.parametrize("n", SIZES)
def test_twiddle_first_codelet_against_float64(harness, adversarial_rows, n):
    F = ETA * np.log2(n)
    x = lines(n, 7000 + n, adversarial_rows)
    for d in (1, -1):
        want = np.fft.fft(x, axis=1) if d > 0 else np.fft.ifft(x, axis=1) * n
        shipped = run(harness, "s", n, d, x)
        e_s = normwise(shipped, want) / U32
        for kind in ("t", "T"):
            got = run(harness, kind, n, d, x)
            # the impulses first, bin by bin: every bin of an impulse has modulus |amplitude|
            amp = np.abs(x[:2 * n].sum(axis=1))[:, None]
            bin_err = (np.abs(got[:2 * n] - want[:2 * n]) / amp).max() / U32
            e = normwise(got, want) / U32
            e_ab = normwise(got, shipped) / U32
            print(f"  N = {n:3d} dir {d:+d} {'literals' if kind == 't' else 'TwRegs  '}: twiddle-first {e:.2f} u, shipped {e_s:.2f} u, "
                  f"between the forms {e_ab:.2f} u, worst impulse bin {bin_err:.2f} u; gate {F:.1f} u")
            assert bin_err <= F, (n, d, kind, bin_err)
            assert 0 < e <= F and e_s <= F, (n, d, kind, e, e_s, F)
            assert e_ab <= F, (n, d, kind, e_ab, F)


@pytest.mark.parametrize("n", C2R_SIZES)
def test_c2r_through_twiddle_first_against_float64(harness, adversarial_rows, n):
    F = ETA * np.log2(n)
    x = lines(n, 9000 + n, adversarial_rows)
    y = np.fft.rfft(x.real, axis=1).astype(np.complex64).astype(np.complex128)
    y[:, 0] = y[:, 0].real
    y[:, -1] = y[:, -1].real
    j = np.arange(n // 2 + 1)
    imp = np.zeros((n // 2 + 1, n // 2 + 1), complex)                 # one bin each (DC and Nyquist real)
    imp[j, j] = np.where((j == 0) | (j == n // 2), 1.0, 0.75 - 0.5j)
    y = np.concatenate([imp, y])
    want = np.fft.irfft(y, n, axis=1) * n
    res = {}
    for kind in ("c", "C"):
        h = run(harness, kind, n, 0, y)
        got = np.empty((len(y), n))
        got[:, 0::2], got[:, 1::2] = h.real, h.imag
        res[kind] = got
    e, e_s, e_ab = (normwise(res["c"], want) / U32, normwise(res["C"], want) / U32, normwise(res["c"], res["C"]) / U32)
    print(f"  c2r N = {n:3d}: twiddle-first {e:.2f} u, shipped {e_s:.2f} u, between the forms {e_ab:.2f} u; gate {F:.1f} u")
    assert 0 < e <= F and e_s <= F and e_ab <= F, (n, e, e_s, e_ab, F)
