"""The reference's float64 first pass, evaluated exactly, with the error band of a float64 transform carried through it.
Shared by tests/test_gpu_f64_pass1.py (GPU cases and the CPU checks of its case table) and tests/f64_pass1_probe.py.
Not a test module itself.

Even window sizes.  The inputs are uint8, so the circular correlation sums S(d) = sum_p a[p] b[p + d] are integers
below 2^31: a float64 transform of the raw bytes, rounded to the nearest integer, IS S (the rounding distance is asserted
below 0.01; it is about 1e-5), and the reference's map cell is (S - S_min) n^4 / (sum a sum b) + 1e-7 in float64, as
tests/test_exact_scheme.py::exact_window and tests/test_gpu_exact_band.py::exact_reference form it.

Odd window sizes.  The reference calls irfft2 without `s` (B:255): the (n + 1) / 2 spectrum columns of rfft2 are read as
the half spectrum of a row of n - 1 samples, so the map is n rows x (n - 1) columns, not a correlation of integers any
more.  It is built here with numpy's longdouble transform (u = 2^-64, 2000 x finer than float64).

The band.  A float64 kernel's map is the exact one plus a common offset plus e, |e| <= beta = Gamma(ws, kind) 2^-53 E0
(piv_kernels.h "The band"; E0 below, the energy of what these kernels transform, where the float32
locating pass has E+); after both maps subtract their own minimum a cell is within
delta = 2 beta + 8 * 2^-53 * (largest cell) of the reference's (the second term: the three roundings of
(c - min) * scale + 1e-7 on either side).  delta goes through the log-Gaussian fit by the interval arithmetic of
tests/test_gpu_shifted_maps.py (fit_bound), which bounds |du|, |dv| per window; a window is excused only where a discrete
decision -- arg-max margin, peak ratio against val_ratio, the fit's denominator -- lies inside delta.
"""
import numpy as np

from oracle import piv_oracle as O
from test_exact_scheme import exact_sum, gamma_u
from test_gpu_shifted_maps import fit_bound, neighbours

U64 = 2.0 ** -53
ROUND_DIST = 0.01          # the rounded float64 transform must stay this close to the integers it stands for


def window_stats(a, b):
    """-> sum a, sum b (int64), E0, dead (a zero sum), const (a window without variation: constant map).
    E0 is the energy of what the float64 kernels transform.  They keep the DC pedestal in, as the reference does (B:513-514
    divides by the mean and subtracts nothing), so the rounding error of their transforms scales with the whole
    normalised window a_n = a / mean(a), |a_n|^2 = n^2 + |a'|^2, not with the mean-free a' of the float32 locating pass
    (E+).  The generic kernel transforms a_n + i b_n: E0 = (|a_n|^2 + |b_n|^2) / 2.  The tile and split kernels transform
    the raw bytes and scale the map by n^4 / (sum a sum b): E0 = n^4 (|a|^2 + |b|^2) / (2 sum a sum b).  The larger of
    the two serves every kernel (they are equal where sum a = sum b)."""
    n = a.shape[0]
    ai, bi = a.reshape(n, -1).astype(np.int64), b.reshape(n, -1).astype(np.int64)
    sa, sb = ai.sum(axis=1), bi.sum(axis=1)
    dead = (sa == 0) | (sb == 0)
    nn = float(ai.shape[1])
    qa, qb = (ai * ai).sum(axis=1).astype(np.float64), (bi * bi).sum(axis=1).astype(np.float64)
    fa, fb = sa.astype(np.float64), sb.astype(np.float64)
    with np.errstate(all="ignore"):
        e_norm = 0.5 * nn * nn * (qa / fa ** 2 + qb / fb ** 2)
        e_raw = 0.5 * nn * nn * (qa + qb) / (fa * fb)
    flat = (ai.max(axis=1) == ai.min(axis=1)) | (bi.max(axis=1) == bi.min(axis=1))
    e0 = np.where(dead, 0.0, np.nan_to_num(np.maximum(e_norm, e_raw)))
    return sa, sb, e0, dead, flat & ~dead


def e_plus(a, b):
    """E+ = (|a'|^2 + |b'|^2) / 2, a' = a / mean(a) - 1: the scale of a transform of the MEAN-FREE windows (the float32
    locating pass; tests/test_exact_scheme.py::e_plus for a stack of windows).  Live windows only."""
    n = a.shape[0]
    nn = float(a.shape[-1] * a.shape[-2])
    af, bf = a.reshape(n, -1).astype(np.float64), b.reshape(n, -1).astype(np.float64)
    return 0.5 * nn * (nn * (af ** 2).sum(axis=1) / af.sum(axis=1) ** 2 + nn * (bf ** 2).sum(axis=1) / bf.sum(axis=1) ** 2 - 2.0)


def exact_maps(a, b):
    """Even sizes: [n, W, W] map cells (S - S_min) n^4 / (sum a sum b), fftshift layout, without the 1e-7; dead windows get
    zeros.  Asserts the rounding distance of the transform and spot-checks cells against exact_sum."""
    n, W = a.shape[0], a.shape[-1]
    af, bf = a.astype(np.float64), b.astype(np.float64)
    Sf = np.fft.irfft2(np.conj(np.fft.rfft2(af)) * np.fft.rfft2(bf), s=(W, W))
    S = np.rint(Sf)
    dist = float(np.abs(Sf - S).max()) if n else 0.0
    assert dist < ROUND_DIST, dist
    S = np.fft.fftshift(S, axes=(1, 2)).astype(np.int64)
    rng = np.random.default_rng(n * 1000 + W)
    for i in rng.integers(0, n, min(n, 3)):
        for q in rng.integers(0, W * W, 2):
            assert exact_sum(a[i], b[i], int(q)) == S[i].reshape(-1)[q], (i, q)
    sa, sb, _, dead, _ = window_stats(a, b)
    with np.errstate(all="ignore"):
        scale = float(W) ** 4 / (sa.astype(np.float64) * sb.astype(np.float64))
    scale = np.where(dead, 0.0, scale)
    c = (S - S.min(axis=(1, 2), keepdims=True)).astype(np.float64) * scale[:, None, None]
    return c, dist


def odd_maps(a, b):
    """Odd sizes: the reference's n x (n - 1) map of a / mean(a), b / mean(b) (B:513-514, B:249-257, B:518) in longdouble,
    returned as float64 (one rounding, inside delta's second term); dead windows get zeros."""
    ld = np.longdouble
    n = a.shape[0]
    _, _, _, dead, _ = window_stats(a, b)
    al, bl = a.astype(ld), b.astype(ld)
    with np.errstate(all="ignore"):
        al = al / al.mean(axis=(1, 2), keepdims=True)
        bl = bl / bl.mean(axis=(1, 2), keepdims=True)
    al[dead], bl[dead] = 0, 0
    A, B = np.fft.rfft2(al), np.fft.rfft2(bl)
    assert A.dtype == np.complex256, A.dtype                  # (numpy >= 2: the transform runs in the input's precision)
    c = np.fft.fftshift(np.fft.irfft2(np.conj(A) * B), axes=(1, 2))
    assert c.shape == (n, a.shape[-1], a.shape[-1] - 1), c.shape
    c = c - c.min(axis=(1, 2), keepdims=True)
    return c.astype(np.float64)


def reference_maps(a, b):
    return odd_maps(a, b) if a.shape[-1] % 2 else exact_maps(a, b)[0]


def fit_bound_flat(c, m, i1, i2, delta):
    """fit_bound, with the one case it cannot know settled: both neighbours clamped onto the arg-max itself (B:389-392)
    makes nominator and denominator exact zeros of equal cells -- NaN, then 0 by nan_to_num (B:418-419) whatever the map's
    rounding, so the bound is 0."""
    out = fit_bound(c, m, i1, i2, delta)
    return np.where((i1 == m) & (i2 == m), 0.0, out)


def reference_fields(c0, ep, ws, kind, val_ratio, val_win, gate=1.0):
    """c0 [n, d, k]: the reference's map without the 1e-7.  -> dict: u, v, invalid (the reference's first pass on it), bu, bv
    (bounds of |du|, |dv| under the band), delta, near (the three discrete decisions inside the band)."""
    n, d, k = c0.shape
    rows = np.arange(n)
    c = c0.reshape(n, -1) + O.EPS
    beta = gate * gamma_u(ws, kind) * U64 * ep
    delta = 2.0 * beta + 8.0 * U64 * c.max(axis=1)
    u, v, _ = O.corr_to_disp(c0, n, 1, False)
    u, v = u[:, 0], v[:, 0]
    m = np.argmax(c, axis=1)
    srt = np.sort(c, axis=1)
    near_argmax = (srt[:, -1] - srt[:, -2]) <= 2 * delta
    # second peak as the reference's pass 1 sees it: its float64 map is zeroed IN PLACE (B:382 aliases it), so a map that
    # lies wholly inside the exclusion zone gives c[m2] = 0 and an infinite ratio (xcorr_generic.hip says the same)
    work = c.copy()
    m2 = O.second_peak(work, m, val_win, k, d)
    cm, c2 = c[rows, m], work[rows, m2]
    with np.errstate(all="ignore"):
        invalid = (cm / c2) < val_ratio
        r_lo = np.where(c2 > 0, (cm - delta) / (c2 + delta), np.inf)
        r_hi = np.where(c2 - delta > 0, (cm + delta) / (c2 - delta), np.inf)
    near_ratio = (r_lo <= val_ratio) & (r_hi >= val_ratio)
    left, right, top, bot = neighbours(m, k, d)
    bu = fit_bound_flat(c, m, left, right, delta)
    bv = fit_bound_flat(c, m, top, bot, delta)
    return {"u": u, "v": v, "invalid": invalid, "bu": bu, "bv": bv, "delta": delta, "m": m,
            "near": {"argmax": near_argmax, "ratio": near_ratio, "fit": ~np.isfinite(bu) | ~np.isfinite(bv)}}


def fit_slack(ws):
    """What the float64 evaluation of the fit itself may differ by, on either side: five logs to an ulp each (|log c| <= 17
    for cells between 1e-7 and 1e7), a division, and the sum with the integer part, which is below ws / 2 + 1."""
    return 64.0 * U64 * (ws / 2 + 1)
