"""The swap-free first transposition of the 64 x 64 tile kernels (TPIV_NOSWAP64, csrc/xcorr_tile.hpp): rows 32 ... 63 enter
the row transform with their odd samples negated, every lane reads the other lane half's tile in the second phase, and
the rotation by 32 rows that leaves in columns 32 ... 63 comes back as a sign of the odd cross-spectrum bins.  A wrong tile,
a missed sign or a rotated row moves the correlation peak by whole pixels (typically by 32), so the inputs here are
windows whose content sits where those mistakes show: energy only in rows 32 ... 63, only in rows 0 ... 31, only in odd
columns, only in one quadrant (each of the four), and one bright pixel at (0, 0), (31, 31), (32, 32), (63, 63), (31, 32)
(row, column), each with a known displacement.

The bright pixel stands on a dim random background (0 ... 15 grey levels) and the particles of the other cases on one of
0 ... 3: on a black background every cell but the peak is AT the map minimum, and the three-point log fit of
corr - min + 1e-7 then amplifies any rounding -- the float64 oracle's included -- into tenths of a pixel; that would test
the fit's conditioning, not the transposition.  test_oracle_peaks_are_unambiguous (no GPU) holds every case window to:
valid in the oracle, peak at the known displacement, not a near tie, and outside the float32 noise band of the existing
parity gates (arg-max, peak ratio, fit) -- so no case is skipped or excused below.

Fields against the CPU oracle at the tolerances the project gates on (BASELINE.json north_star, tests/test_gpu_parity.py):
1e-3 px for the "fast" first pass and the shifted passes, 1e-9 px and identical masks for the "exact" first pass.  The
case windows lie in the middle row of a 3 x (n + 2) grid of windows; the windows around them hold ordinary particle
images and are compared too (the border ones take the per-pixel staging path of the shifted passes, which has to apply
the same input sign)."""
import numpy as np
import pytest
import torch

from oracle import piv_oracle as O
from test_gpu_parity import TOL_PX, constant_windows, fp32_noise_excuse, near_tie_windows

WS = 64
PIXELS = [((0, 0), (3, 2)), ((31, 31), (-2, 3)), ((32, 32), (2, -3)), ((63, 63), (-3, -2)), ((31, 32), (1, 1))]
REGIONS = ["rows_hi", "rows_lo", "odd_cols", "q00", "q01", "q10", "q11"]
SHIFTS = [(2, -1), (-1, 2), (1, 2), (-2, -1), (1, -2), (-1, 1), (1, 2)]
CASES = [f"pixel{p[0]}_{p[1]}" for p, _ in PIXELS] + REGIONS


def particles(rng, h, w, n, shift, sigma=1.3):
    """Two uint8 images of n Gaussian particles, the second displaced by shift = (dy, dx)."""
    py, px, amp = rng.uniform(3, h - 3, n), rng.uniform(3, w - 3, n), rng.uniform(120, 250, n)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for oy, ox in ((0.0, 0.0), shift):
        img = np.zeros((h, w))
        for y, x, a in zip(py + oy, px + ox, amp):
            img += a * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2 * sigma ** 2))
        out.append(img)
    return out


def region_mask(name):
    m = np.zeros((WS, WS), bool)
    if name == "rows_hi":
        m[32:, :] = True
    elif name == "rows_lo":
        m[:32, :] = True
    elif name == "odd_cols":
        m[:, 1::2] = True
    else:
        qy, qx = int(name[1]), int(name[2])
        m[32 * qy:32 * qy + 32, 32 * qx:32 * qx + 32] = True
    return m


def case_windows():
    """[n, 2, 64, 64] uint8 and the displacement (dy, dx) of frame b against frame a, per case."""
    rng = np.random.default_rng(640)
    wins, shifts = [], []
    for (py, px), (dy, dx) in PIXELS:
        a = rng.integers(0, 16, (WS, WS))
        b = rng.integers(0, 16, (WS, WS))
        a[py, px] = 255
        b[py + dy, px + dx] = 255
        wins.append(np.stack([a, b]))
        shifts.append((dy, dx))
    for name, (dy, dx) in zip(REGIONS, SHIFTS):
        m = region_mask(name)
        # the particles live inside the region in both frames: it is the content that moves, not the region
        a, b = particles(rng, WS, WS, 60, (dy, dx))
        # (odd_cols: the map of a window that is black in every even column is AT its minimum at every odd column lag --
        #  the fit's left and right neighbours -- so there the even columns keep the dim background: < 1 % of the energy)
        out = rng.integers(0, 4, (2, WS, WS)) if name == "odd_cols" else np.zeros((2, WS, WS))
        a = np.where(m, a + rng.integers(0, 4, (WS, WS)), out[0])
        b = np.where(m, b + rng.integers(0, 4, (WS, WS)), out[1])
        wins.append(np.stack([a, b]))
        shifts.append((dy, dx))
    return np.clip(np.rint(np.stack(wins)), 0, 255).astype(np.uint8), shifts


def frames():
    """The case windows as the middle row of a 3 x (n + 2) grid of 64 x 64 windows (overlap 0) of particle images."""
    wins, shifts = case_windows()
    n = len(wins)
    H, W = 3 * WS, (n + 2) * WS
    rng = np.random.default_rng(641)
    a, b = particles(rng, H, W, H * W // 60, (1.3, -0.7))
    A = np.clip(np.rint(a + rng.normal(6, 1.5, a.shape)), 0, 255).astype(np.uint8)
    B = np.clip(np.rint(b + rng.normal(6, 1.5, b.shape)), 0, 255).astype(np.uint8)
    for i, w in enumerate(wins):
        A[WS:2 * WS, (i + 1) * WS:(i + 2) * WS] = w[0]
        B[WS:2 * WS, (i + 1) * WS:(i + 2) * WS] = w[1]
    is_case = np.zeros((3, n + 2), bool)
    is_case[1, 1:n + 1] = True
    return A, B, shifts, is_case


def predictor(mode, nr, nc):
    """Half shifts of a shifted pass: small (the case windows keep their content), integers for DWS, fractional for CWS with
    some integral row coordinates (the per-pixel path of the 64 x 64 CWS kernels) among them."""
    rng = np.random.default_rng(642 + len(mode))
    if mode == "DWS":
        u2, v2 = rng.integers(-1, 2, (nr, nc)).astype(np.float64), rng.integers(-1, 2, (nr, nc)).astype(np.float64)
        u2[1, 1:len(PIXELS) + 1] = 0.0          # (a whole-pixel shift would push the pixels at the window edge out of it)
        v2[1, 1:len(PIXELS) + 1] = 0.0
    else:
        u2, v2 = rng.uniform(-0.9, 0.9, (nr, nc)), rng.uniform(-0.9, 0.9, (nr, nc))
        u2[1, 1:len(PIXELS) + 1] *= 0.15        # (a bilinear shift spreads a single pixel over four: kept small)
        v2[1, 1:len(PIXELS) + 1] *= 0.15
        v2[1, 2::4] = np.rint(v2[1, 2::4])
    return u2, v2


def shifted_oracle(A, B, mode, u2, v2):
    """The oracle's shifted pass from a given half-shift field: staged windows, float32 correlation (B:249-257), peak
    analysis; u = 2 u2 + du where valid, 0 where not (what tpiv_debug_pass returns with a zero predictor u0)."""
    nr, nc = O.field_shape(A.shape, WS, 0)
    idx = O.window_index(A.shape, WS, 0)
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


def test_oracle_peaks_are_unambiguous():
    """No GPU: every case window has a valid, well-conditioned peak at its known displacement in the oracle -- in pass 1
    and in both shifted passes under the predictors used below -- so the GPU tests excuse none of them."""
    A, B, shifts, is_case = frames()
    nr, nc = is_case.shape
    u, v, _, _, mask = O.pass1(A, B, WS, 0, validate=True)
    assert not mask[is_case].any()
    want = np.array(shifts, dtype=np.float64)
    assert np.abs(u[is_case] - want[:, 1]).max() < 0.5 and np.abs(v[is_case] - want[:, 0]).max() < 0.5, (u[is_case], v[is_case])
    assert not near_tie_windows(A, B, WS, 0)[is_case].any()
    aa, bb = O.windows(A, WS, 0), O.windows(B, WS, 0)
    with np.errstate(all="ignore"):
        na = aa / aa.mean(axis=(-2, -1), dtype=np.float64, keepdims=True)
        nb = bb / bb.mean(axis=(-2, -1), dtype=np.float64, keepdims=True)
    assert not fp32_noise_excuse(na - 1, nb - 1, nr, nc, fit_tol=0.5e-3)[is_case].any()
    for mode in ("DWS", "CWS"):
        u2, v2 = predictor(mode, nr, nc)
        _, _, val, aa, bb, du, dv = shifted_oracle(A, B, mode, u2, v2)
        assert not val[is_case].any(), mode
        res_u, res_v = want[:, 1] - 2 * u2[is_case], want[:, 0] - 2 * v2[is_case]
        # (within one pixel: the bilinear shift smears a single pixel and pulls its fit towards the integer; a wrong tile is 32 off)
        assert np.abs(du[is_case] - res_u).max() < 1.0 and np.abs(dv[is_case] - res_v).max() < 1.0, (mode, du[is_case], res_u)
        assert not fp32_noise_excuse(aa, bb, nr, nc, fit_tol=0.5e-3)[is_case].any(), mode


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def compare(u, v, inv, ru, rv, rinv, excused, is_case, tol, what):
    u, v, inv = u.cpu().numpy(), v.cpu().numpy(), inv.cpu().numpy().astype(bool)
    err = np.maximum(np.abs(u - ru), np.abs(v - rv))
    print(f"  {what}: case windows max |d| {err[is_case].max():.2e} px; all windows {err[~excused].max():.2e} px, "
          f"{int(excused.sum())} excused (none of them a case window), flags differing {int((inv != rinv).sum())}")
    assert not excused[is_case].any(), what
    assert excused.mean() <= 0.1, (what, int(excused.sum()))
    bad = ((err > tol) | (inv != rinv)) & ~excused
    assert not bad.any(), (what, np.argwhere(bad).tolist(), err[bad].tolist(), [CASES[c - 1] for r, c in np.argwhere(bad & is_case)])


@pytest.mark.gpu
def test_pass1_fast(eng):
    A, B, _, is_case = frames()
    u, v, inv = eng.pass1(dev(A), dev(B), WS, 0, precision="fast")
    ru, rv, _, _, rm = O.pass1(A, B, WS, 0, validate=True)
    compare(u[0], v[0], inv[0], ru, rv, rm, near_tie_windows(A, B, WS, 0), is_case, TOL_PX, "pass 1 fast")


@pytest.mark.gpu
def test_pass1_exact(eng):
    """The locating pass + exact integer sums: 1e-9 px and identical masks, every window."""
    A, B, _, is_case = frames()
    u, v, inv = eng.pass1(dev(A), dev(B), WS, 0, precision="exact")
    ru, rv, _, _, rm = O.pass1(A, B, WS, 0, validate=True)
    compare(u[0], v[0], inv[0], ru, rv, rm, np.zeros_like(is_case), is_case, 1e-9, "pass 1 exact")


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fast", "reference"])
@pytest.mark.parametrize("mode", ["DWS", "CWS"])
def test_shifted_pass(eng, mode, precision):
    """64 x 64 DWS and CWS ("fast": the three-wavefront instances, for CWS the wide-load instance and its list launch;
    "reference": the reference-order instances, for CWS the complex-tile kernel)."""
    A, B, _, is_case = frames()
    nr, nc = is_case.shape
    u2, v2 = predictor(mode, nr, nc)
    u, v, inv, _, _ = eng.debug_pass(mode, dev(A), dev(B), WS, 0, dev(u2)[None], dev(v2)[None], precision=precision)
    ru, rv, rval, aa, bb, _, _ = shifted_oracle(A, B, mode, u2, v2)
    excused = fp32_noise_excuse(aa, bb, nr, nc, fit_tol=0.5e-3) | constant_windows(aa, bb, nr, nc)
    compare(u[0], v[0], inv[0], ru, rv, rval, excused, is_case, TOL_PX, f"{mode} {precision}")
