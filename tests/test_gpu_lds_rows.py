"""The lane-contiguous first transposition of the planar 32 x 32 and 64 x 64 tile kernels (transpose_tile<.., ROWS>,
csrc/xcorr_tile.hpp): row k of the LDS tile holds element k of all 64 lanes (pitch 68 dwords), stored with two blocks of
16 `ds_write_addtid_b32` per plane-phase and read back as 8 `ds_read_b128` per lane.  What can go wrong there moves a
sample to another row or column of the spectrum: a store block that starts at the wrong row (the blocks meet at
k = 15 | 16), a 16-byte read whose four values land in the wrong registers (k = 3 | 4), a wrong half offset (k = 31 | 32,
the other lane half's columns in the second phase of 64 x 64, the other WINDOW of the wavefront at 32 x 32).  So the inputs
are windows with one bright pixel on a dim random background, on the diagonal at exactly those indices and next to it,
each with a known displacement; at 32 x 32 horizontally adjacent windows -- the two windows of one wavefront -- have
different displacements, so exchanging them shows.

Built like tests/test_gpu_noswap64.py (see there for why the background is dim and not black): the case windows are the
middle row of a 3 x (n + 2) grid of windows at overlap 0, the windows around them hold particle images and are compared
too.  test_oracle_peaks_are_unambiguous (no GPU) holds every case window to a valid, untied, well-conditioned peak at the
known displacement in the oracle alone, so no case window is excused below.  Gates: TOL_PX for the float32 passes, 1e-9 px
and identical masks for "exact"."""
import functools

import numpy as np
import pytest
import torch

from oracle import piv_oracle as O
from test_gpu_noswap64 import particles
from test_gpu_parity import TOL_PX, constant_windows, fp32_noise_excuse, near_tie_windows

DIAG = {64: [0, 3, 4, 15, 16, 31, 32, 35, 47, 48, 63], 32: [0, 3, 4, 15, 16, 19, 31]}
OFF = {64: [(15, 16), (16, 15), (31, 32), (32, 31)], 32: [(15, 16), (16, 15)]}
SEED = {64: 6864, 32: 6833}      # (of the backgrounds; chosen on the oracle alone: test_oracle_peaks_are_unambiguous)
MAGS = [(3, 2), (2, 3), (1, 2), (2, 1), (3, 1), (1, 3), (2, 2)]       # |dy|, |dx|, cycled: neighbours differ


def pixels(ws):
    """[((row, column), (dy, dx))]: the displacement points into the window."""
    pos = [(d, d) for d in DIAG[ws]] + OFF[ws]
    out = []
    for n, (py, px) in enumerate(pos):
        my, mx = MAGS[n % len(MAGS)]
        out.append(((py, px), (my if py < ws // 2 else -my, mx if px < ws // 2 else -mx)))
    return out


@functools.lru_cache(maxsize=None)
def frames(ws):
    """The case windows as the middle row of a 3 x (n + 2) grid of ws x ws windows (overlap 0) of particle images."""
    pix = pixels(ws)
    n = len(pix)
    rng = np.random.default_rng(SEED[ws])
    H, W = 3 * ws, (n + 2) * ws
    a, b = particles(rng, H, W, H * W // 60, (1.3, -0.7))
    A = np.clip(np.rint(a + rng.normal(6, 1.5, a.shape)), 0, 255).astype(np.uint8)
    B = np.clip(np.rint(b + rng.normal(6, 1.5, b.shape)), 0, 255).astype(np.uint8)
    for i, ((py, px), (dy, dx)) in enumerate(pix):
        wa, wb = rng.integers(0, 16, (ws, ws)), rng.integers(0, 16, (ws, ws))
        wa[py, px] = 255
        wb[py + dy, px + dx] = 255
        A[ws:2 * ws, (i + 1) * ws:(i + 2) * ws] = wa
        B[ws:2 * ws, (i + 1) * ws:(i + 2) * ws] = wb
    is_case = np.zeros((3, n + 2), bool)
    is_case[1, 1:n + 1] = True
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B, [s for _, s in pix], is_case


def predictor(ws, mode):
    """Half shifts of a shifted pass, as in test_gpu_noswap64: small, so that the case windows keep their content."""
    n = len(pixels(ws))
    nr, nc = 3, n + 2
    rng = np.random.default_rng(6900 + ws + len(mode))
    if mode == "DWS":
        u2, v2 = rng.integers(-1, 2, (nr, nc)).astype(np.float64), rng.integers(-1, 2, (nr, nc)).astype(np.float64)
        u2[1, 1:n + 1] = 0.0
        v2[1, 1:n + 1] = 0.0
    else:
        u2, v2 = rng.uniform(-0.9, 0.9, (nr, nc)), rng.uniform(-0.9, 0.9, (nr, nc))
        u2[1, 1:n + 1] *= 0.15
        v2[1, 1:n + 1] *= 0.15
    return u2, v2


@functools.lru_cache(maxsize=None)
def shifted_oracle(ws, mode):
    """The oracle's shifted pass from predictor(ws, mode): u = 2 u2 + du where valid, 0 where not (what debug_pass returns
    with a zero predictor u0); also the staged windows and the bare peak offsets."""
    A, B, _, _ = frames(ws)
    u2, v2 = predictor(ws, mode)
    nr, nc = O.field_shape(A.shape, ws, 0)
    idx = O.window_index(A.shape, ws, 0)
    if mode == "CWS":
        su, sv = (t.astype(np.float32).reshape(-1)[:, None, None] for t in (u2, v2))
        aa, bb = O.shift_cws(A, idx, -su, -sv), O.shift_cws(B, idx, su, sv)
    else:
        su, sv = (t.astype(np.int64).reshape(-1)[:, None, None] for t in (u2, v2))
        aa, bb = O.shift_dws(A, idx, -su, -sv), O.shift_dws(B, idx, su, sv)
    corr = O.xcorr_fft(aa, bb)
    corr = corr - corr.min(axis=(-2, -1), keepdims=True)
    du, dv, val = O.corr_to_disp(corr, nr, nc, True)
    return np.where(val, 0.0, 2 * u2 + du), np.where(val, 0.0, 2 * v2 + dv), val, aa, bb, du, dv


@functools.lru_cache(maxsize=None)
def pass1_oracle(ws):
    A, B, _, _ = frames(ws)
    u, v, _, _, mask = O.pass1(A, B, ws, 0, validate=True)
    return u, v, mask


@pytest.mark.parametrize("ws", [64, 32])
def test_oracle_peaks_are_unambiguous(ws):
    """No GPU: every case window has a valid, untied, well-conditioned peak at its known displacement in the oracle -- in
    pass 1 and in both shifted passes under the predictors used below -- and horizontally adjacent case windows have
    different displacements.  So the GPU tests excuse no case window."""
    A, B, shifts, is_case = frames(ws)
    nr, nc = is_case.shape
    assert all(s != t for s, t in zip(shifts, shifts[1:]))
    u, v, mask = pass1_oracle(ws)
    assert not mask[is_case].any()
    want = np.array(shifts, dtype=np.float64)
    assert np.abs(u[is_case] - want[:, 1]).max() < 0.5 and np.abs(v[is_case] - want[:, 0]).max() < 0.5, (u[is_case], v[is_case])
    assert not near_tie_windows(A, B, ws, 0)[is_case].any()
    aa, bb = O.windows(A, ws, 0), O.windows(B, ws, 0)
    na = aa / aa.mean(axis=(-2, -1), dtype=np.float64, keepdims=True)
    nb = bb / bb.mean(axis=(-2, -1), dtype=np.float64, keepdims=True)
    assert not fp32_noise_excuse(na - 1, nb - 1, nr, nc, fit_tol=0.5e-3)[is_case].any()
    for mode in ("DWS", "CWS"):
        u2, v2 = predictor(ws, mode)
        _, _, val, aa, bb, du, dv = shifted_oracle(ws, mode)
        assert not val[is_case].any(), mode
        res_u, res_v = want[:, 1] - 2 * u2[is_case], want[:, 0] - 2 * v2[is_case]
        # (within one pixel: the bilinear shift smears a single pixel and pulls its fit towards the integer; a misplaced
        #  sample moves the peak by whole rows or columns, and a neighbour's displacement differs by one pixel or more)
        assert np.abs(du[is_case] - res_u).max() < 1.0 and np.abs(dv[is_case] - res_v).max() < 1.0, (mode, du[is_case], res_u)
        assert not fp32_noise_excuse(aa, bb, nr, nc, fit_tol=0.5e-3)[is_case].any(), mode
        assert not constant_windows(aa, bb, nr, nc)[is_case].any(), mode


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the cached frames are read-only)


def compare(ws, u, v, inv, ru, rv, rinv, excused, tol, what):
    is_case = frames(ws)[3]
    u, v, inv = u.cpu().numpy(), v.cpu().numpy(), inv.cpu().numpy().astype(bool)
    err = np.maximum(np.abs(u - ru), np.abs(v - rv))
    print(f"  {ws} x {ws} {what}: case windows max |d| {err[is_case].max():.2e} px; all windows {err[~excused].max():.2e} px, "
          f"{int(excused.sum())} excused (0 of them case windows), flags differing {int((inv != rinv).sum())}")
    assert not excused[is_case].any(), what
    assert excused.mean() <= 0.1, (what, int(excused.sum()))
    bad = ((err > tol) | (inv != rinv)) & ~excused
    names = [pixels(ws)[c - 1][0] for r, c in np.argwhere(bad & is_case)]
    assert not bad.any(), (ws, what, np.argwhere(bad).tolist(), err[bad].tolist(), names)


@pytest.mark.gpu
@pytest.mark.parametrize("ws", [64, 32])
def test_pass1_fast(eng, ws):
    A, B, _, _ = frames(ws)
    u, v, inv = eng.pass1(dev(A), dev(B), ws, 0, precision="fast")
    ru, rv, rm = pass1_oracle(ws)
    compare(ws, u[0], v[0], inv[0], ru, rv, rm, near_tie_windows(A, B, ws, 0), TOL_PX, "pass 1 fast")


@pytest.mark.gpu
@pytest.mark.parametrize("ws", [64, 32])
def test_pass1_exact(eng, ws):
    """The candidate (locating) pass + exact integer sums: 1e-9 px and identical masks, every window."""
    A, B, _, is_case = frames(ws)
    u, v, inv = eng.pass1(dev(A), dev(B), ws, 0, precision="exact")
    ru, rv, rm = pass1_oracle(ws)
    compare(ws, u[0], v[0], inv[0], ru, rv, rm, np.zeros_like(is_case), 1e-9, "pass 1 exact")


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fast", "reference"])
@pytest.mark.parametrize("mode", ["DWS", "CWS"])
@pytest.mark.parametrize("ws", [64, 32])
def test_shifted_pass(eng, ws, mode, precision):
    """DWS and CWS through debug_pass, in the fast and the reference operation order (64 x 64 CWS "fast": the wide-load
    instance and its list launch)."""
    A, B, _, is_case = frames(ws)
    nr, nc = is_case.shape
    u2, v2 = predictor(ws, mode)
    u, v, inv, _, _ = eng.debug_pass(mode, dev(A), dev(B), ws, 0, dev(u2)[None], dev(v2)[None], precision=precision)
    ru, rv, rval, aa, bb, _, _ = shifted_oracle(ws, mode)
    excused = fp32_noise_excuse(aa, bb, nr, nc, fit_tol=0.5e-3) | constant_windows(aa, bb, nr, nc)
    compare(ws, u[0], v[0], inv[0], ru, rv, rval, excused, TOL_PX, f"{mode} {precision}")
