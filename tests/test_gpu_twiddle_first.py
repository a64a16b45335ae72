"""The twiddle-first FFT codelets (fft_twf, csrc/fft_inreg.hpp) inside the 64 x 64 and 32 x 32 tile kernels.

The codelet computes each level's twiddle products in front of the butterfly and must leave bin k in register
FFT_POS<k, N>, where every consumer (cross-spectrum, both transpositions, the half inverse, c2r) expects it.  A result in
the wrong register, a wrong twiddle index or a wrong sign of the +-i rotation moves the correlation peak by whole pixels,
so the inputs are windows with a known displacement whose content sits where such mistakes show:
  * one bright pixel on a dim random background at (row, column) (0, 0), (1, 0), (0, 1), (WS/4, WS/4 + 1),
    (WS/2 - 1, WS/2), (WS - 1, WS - 1): its spectrum is one pure phase ramp, every bin counts;
  * particle images confined to one quadrant (each of the four);
  * energy only in odd rows, only in odd columns (the first radix level's odd sub-transforms alone carry the signal).
(Dim backgrounds instead of black ones for the reason given in tests/test_gpu_noswap64.py: on black, the fit's neighbours
sit AT the map minimum and the three-point fit amplifies any rounding.)

The case windows are the middle row of a 3 x (n + 2) grid of windows at overlap 0; the windows around them hold ordinary
particle images and are compared too.  WS = 64 and 32, through the first pass ("fast": the tile kernel; "exact": the
locating kernel + integer refinement), a DWS and a CWS shifted pass (tpiv_debug_pass at that window size: the 64 x 64 CWS
instances are what a 64 -> 64 second pass runs, the 32 x 32 CWS instance what the 64 -> 32 second pass of the headline
plan runs).  16 x 16 keeps the shipped codelet and is not run here.

Tolerances: the project's own (tests/test_gpu_parity.py) -- TOL_PX = 1e-3 px for the float32 passes, 1e-9 px and
identical masks for "exact".  No case window is excused: test_oracle_peaks_are_unambiguous (no GPU) holds each one to
"valid in the oracle, peak at the known displacement, not a near tie, outside the float32 noise band"."""
import functools

import numpy as np
import pytest
import torch

from oracle import piv_oracle as O
from test_gpu_parity import TOL_PX, constant_windows, fp32_noise_excuse, near_tie_windows

SIZES = (64, 32)
REGIONS = ["q00", "q01", "q10", "q11", "odd_rows", "odd_cols"]
REGION_SHIFTS = [(2, -1), (-1, 2), (1, 2), (-2, -1), (2, 1), (1, 2)]


def pixels(ws):
    """((row, column), (dy, dx)): the pixel of frame a and where it went in frame b (inside the window)."""
    return [((0, 0), (3, 2)), ((1, 0), (2, 3)), ((0, 1), (3, 1)), ((ws // 4, ws // 4 + 1), (-2, 3)),
            ((ws // 2 - 1, ws // 2), (2, -3)), ((ws - 1, ws - 1), (-3, -2))]


def case_names(ws):
    return [f"pixel{p[0]}_{p[1]}" for p, _ in pixels(ws)] + REGIONS


def particles(rng, h, w, n, shift, sigma=1.3, margin=2.0):
    """Two images of n Gaussian particles, the second displaced by shift = (dy, dx)."""
    py, px, amp = rng.uniform(margin, h - margin, n), rng.uniform(margin, w - margin, n), rng.uniform(120, 250, n)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for oy, ox in ((0.0, 0.0), shift):
        img = np.zeros((h, w))
        for y, x, a in zip(py + oy, px + ox, amp):
            img += a * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2 * sigma ** 2))
        out.append(img)
    return out


def region_mask(name, ws):
    m = np.zeros((ws, ws), bool)
    if name == "odd_rows":
        m[1::2, :] = True
    elif name == "odd_cols":
        m[:, 1::2] = True
    else:
        qy, qx = int(name[1]), int(name[2])
        h = ws // 2
        m[h * qy:h * qy + h, h * qx:h * qx + h] = True
    return m


def case_windows(ws):
    rng = np.random.default_rng(7100 + ws)
    wins, shifts = [], []
    for (py, px), (dy, dx) in pixels(ws):
        # (0 ... 15 grey levels at 64 x 64; 0 ... 7 at 32 x 32, where the background's share of the map is four times larger
        #  and a bilinear shift of the corner pixel would otherwise fail the oracle's peak-ratio test)
        a = rng.integers(0, 16 if ws == 64 else 8, (ws, ws))
        b = rng.integers(0, 16 if ws == 64 else 8, (ws, ws))
        a[py, px] = 255
        b[py + dy, px + dx] = 255
        wins.append(np.stack([a, b]))
        shifts.append((dy, dx))
    for name, (dy, dx) in zip(REGIONS, REGION_SHIFTS):
        m = region_mask(name, ws)
        if name.startswith("q"):
            # the particles live inside the quadrant in both frames (4 px from its edges: the content moves, the region does
            # not cut it), a dozen of them even in a 16 x 16 quadrant
            h = ws // 2
            qa, qb = particles(rng, h, h, 12 if ws == 32 else 20, (dy, dx), margin=4.0)
            a, b = np.zeros((ws, ws)), np.zeros((ws, ws))
            a[m], b[m] = qa.reshape(-1), qb.reshape(-1)
        else:
            a, b = particles(rng, ws, ws, 64 if ws == 64 else 40, (dy, dx))
        # (odd rows / columns: a window that is black in every even row is AT its map minimum at every odd row lag, the
        #  fit's neighbours -- there the even ones keep the dim background, < 1 % of the energy)
        out = rng.integers(0, 4, (2, ws, ws)) if name.startswith("odd") else np.zeros((2, ws, ws))
        a = np.where(m, a + rng.integers(0, 4, (ws, ws)), out[0])
        b = np.where(m, b + rng.integers(0, 4, (ws, ws)), out[1])
        wins.append(np.stack([a, b]))
        shifts.append((dy, dx))
    return np.clip(np.rint(np.stack(wins)), 0, 255).astype(np.uint8), shifts


@functools.lru_cache(maxsize=None)
def frames(ws):
    wins, shifts = case_windows(ws)
    n = len(wins)
    H, W = 3 * ws, (n + 2) * ws
    rng = np.random.default_rng(7200 + ws)
    a, b = particles(rng, H, W, H * W // 60, (1.3, -0.7))
    A = np.clip(np.rint(a + rng.normal(6, 1.5, a.shape)), 0, 255).astype(np.uint8)
    B = np.clip(np.rint(b + rng.normal(6, 1.5, b.shape)), 0, 255).astype(np.uint8)
    for i, w in enumerate(wins):
        A[ws:2 * ws, (i + 1) * ws:(i + 2) * ws] = w[0]
        B[ws:2 * ws, (i + 1) * ws:(i + 2) * ws] = w[1]
    is_case = np.zeros((3, n + 2), bool)
    is_case[1, 1:n + 1] = True
    return A, B, shifts, is_case


@functools.lru_cache(maxsize=None)
def pass1_oracle(ws):
    A, B, _, _ = frames(ws)
    ru, rv, _, _, rm = O.pass1(A, B, ws, 0, validate=True)
    return ru, rv, rm, near_tie_windows(A, B, ws, 0)


def predictor(mode, ws, nr, nc):
    """Half shifts of a shifted pass: small (the case windows keep their content), integers for DWS, fractional for CWS with
    some integral row coordinates (the per-pixel path of the CWS kernels) among them."""
    rng = np.random.default_rng(7300 + ws + len(mode))
    npix = len(pixels(ws))
    if mode == "DWS":
        u2, v2 = rng.integers(-1, 2, (nr, nc)).astype(np.float64), rng.integers(-1, 2, (nr, nc)).astype(np.float64)
        u2[1, 1:npix + 1] = 0.0                 # (a whole-pixel shift would push the pixels at the window edge out of it)
        v2[1, 1:npix + 1] = 0.0
    else:
        u2, v2 = rng.uniform(-0.9, 0.9, (nr, nc)), rng.uniform(-0.9, 0.9, (nr, nc))
        u2[1, 1:npix + 1] *= 0.15               # (a bilinear shift spreads a single pixel over four: kept small)
        v2[1, 1:npix + 1] *= 0.15
        v2[1, 2::4] = np.rint(v2[1, 2::4])
        u2[1, npix] = -abs(u2[1, npix])         # (the sign that keeps the pixel in the last column inside the shifted window)
    return u2, v2


@functools.lru_cache(maxsize=None)
def shifted_oracle(ws, mode):
    """The oracle's shifted pass from the predictor above: staged windows, float32 correlation, peak analysis; u = 2 u2 + du
    where valid, 0 where not (what tpiv_debug_pass returns with a zero predictor u0)."""
    A, B, _, is_case = frames(ws)
    nr, nc = is_case.shape
    u2, v2 = predictor(mode, ws, nr, nc)
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
    excused = fp32_noise_excuse(aa, bb, nr, nc, fit_tol=0.5e-3) | constant_windows(aa, bb, nr, nc)
    return u2, v2, np.where(val, 0.0, 2 * u2 + du), np.where(val, 0.0, 2 * v2 + dv), val, du, dv, excused


@pytest.mark.parametrize("ws", SIZES)
def test_oracle_peaks_are_unambiguous(ws):
    """No GPU: every case window has a valid, well-conditioned peak at its known displacement in the oracle -- in pass 1
    and in both shifted passes under the predictors used below -- so the GPU tests excuse none of them."""
    A, B, shifts, is_case = frames(ws)
    nr, nc = is_case.shape
    u, v, mask, tie = pass1_oracle(ws)
    assert not mask[is_case].any(), [c for c, m in zip(case_names(ws), mask[is_case]) if m]
    want = np.array(shifts, dtype=np.float64)
    assert np.abs(u[is_case] - want[:, 1]).max() < 0.5 and np.abs(v[is_case] - want[:, 0]).max() < 0.5, (u[is_case], v[is_case])
    assert not tie[is_case].any()
    aa, bb = O.windows(A, ws, 0), O.windows(B, ws, 0)
    with np.errstate(all="ignore"):
        na = aa / aa.mean(axis=(-2, -1), dtype=np.float64, keepdims=True)
        nb = bb / bb.mean(axis=(-2, -1), dtype=np.float64, keepdims=True)
    shaky = fp32_noise_excuse(na - 1, nb - 1, nr, nc, fit_tol=0.5e-3)
    assert not shaky[is_case].any(), [c for c, m in zip(case_names(ws), shaky[is_case]) if m]
    for mode in ("DWS", "CWS"):
        u2, v2, _, _, val, du, dv, excused = shifted_oracle(ws, mode)
        assert not val[is_case].any(), mode
        res_u, res_v = want[:, 1] - 2 * u2[is_case], want[:, 0] - 2 * v2[is_case]
        # (within one pixel: the bilinear shift smears a single pixel and pulls its fit towards the integer)
        assert np.abs(du[is_case] - res_u).max() < 1.0 and np.abs(dv[is_case] - res_v).max() < 1.0, (mode, du[is_case], res_u)
        assert not excused[is_case].any(), (mode, [c for c, m in zip(case_names(ws), excused[is_case]) if m])


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def compare(ws, u, v, inv, ru, rv, rinv, excused, is_case, tol, what):
    u, v, inv = u.cpu().numpy(), v.cpu().numpy(), inv.cpu().numpy().astype(bool)
    err = np.maximum(np.abs(u - ru), np.abs(v - rv))
    print(f"  {ws} x {ws} {what}: case windows max |d| {err[is_case].max():.2e} px; all windows {err[~excused].max():.2e} px, "
          f"{int(excused.sum())} excused (none of them a case window), flags differing {int((inv != rinv).sum())}")
    assert not excused[is_case].any(), what
    assert excused.mean() <= 0.1, (what, int(excused.sum()))
    bad = ((err > tol) | (inv != rinv)) & ~excused
    names = case_names(ws)
    assert not bad.any(), (what, np.argwhere(bad).tolist(), err[bad].tolist(), [names[c - 1] for r, c in np.argwhere(bad & is_case)])


@pytest.mark.gpu
@pytest.mark.parametrize("ws", SIZES)
def test_pass1_fast(eng, ws):
    A, B, _, is_case = frames(ws)
    u, v, inv = eng.pass1(dev(A), dev(B), ws, 0, precision="fast")
    ru, rv, rm, tie = pass1_oracle(ws)
    compare(ws, u[0], v[0], inv[0], ru, rv, rm, tie, is_case, TOL_PX, "pass 1 fast")


@pytest.mark.gpu
@pytest.mark.parametrize("ws", SIZES)
def test_pass1_exact(eng, ws):
    """The locating pass + exact integer sums: 1e-9 px and identical masks, every window."""
    A, B, _, is_case = frames(ws)
    u, v, inv = eng.pass1(dev(A), dev(B), ws, 0, precision="exact")
    ru, rv, rm, _ = pass1_oracle(ws)
    compare(ws, u[0], v[0], inv[0], ru, rv, rm, np.zeros_like(is_case), is_case, 1e-9, "pass 1 exact")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["DWS", "CWS"])
@pytest.mark.parametrize("ws", SIZES)
def test_shifted_pass(eng, ws, mode):
    A, B, _, is_case = frames(ws)
    u2, v2, ru, rv, rval, _, _, excused = shifted_oracle(ws, mode)
    u, v, inv, _, _ = eng.debug_pass(mode, dev(A), dev(B), ws, 0, dev(u2)[None], dev(v2)[None], precision="fast")
    compare(ws, u[0], v[0], inv[0], ru, rv, rval, excused, is_case, TOL_PX, f"{mode} fast")
