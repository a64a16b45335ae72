"""Every float32 correlation kernel a shifted pass (DWS, CWS, CWS_Fast) or a "fast" first pass dispatches to, against a
float64 computation of the SAME staged windows (the ones tpiv_debug_pass reports), per window, at two levels:

* map: half the spread of (map32 - map64) -- a common offset changes no decision -- over the error scale S of the
  arithmetic the instance performs, below Gamma(ws, kind) u (tests/test_exact_scheme.py: gamma_u);
* field: the kernel's u, v, invalid against O.corr_to_disp on the float64 map.  Each window's cells lie within 2 h of the
  float64 map, h the window's own measured spread (which the map level holds below Gamma S).  That band, carried through the
  log-Gaussian fit by interval arithmetic, bounds |du|, |dv|; a window may be excused only where a discrete decision (arg-max
  margin, peak ratio against val_ratio, the fit's denominator) lies inside it, and at most 2 % of a case's windows may be.
  So the field level checks the peak stage and the combine on the kernel's own map; the transform error is the map level's.

Gamma by transform kind (gamma_u: Gamma = 2 (2 F + 1) + 5 + 2 I, F / I the forward / inverse per-transform constants):
* radix2 -- the tile kernels, the 128 x 128 first pass, and the w8 lane-per-window kernel: the same radix-2/4 codelets of
  fft_inreg.hpp (FFTStage, eta = 6.66 u per level, lg n levels per 1-D transform); the w8 kernel runs fft_inreg<8> on rows
  and columns of one window in registers, so F = I = 3 eta as for the 8 x 8 tile.  The OCC-2 64 x 64 CWS kernel's list-mode
  launch runs the full 64-point inverse codelet (no paired half inverse): I = 6 eta, the inverse Gamma was first derived
  for; the paired half inverse keeps Gamma unchanged.
* mixed -- fft_mixed.hpp codelets and radix_pass (run-time form), 64 u per transform (tests/test_exact_band_host.py).
* plain -- xcorr_generic_kernel's O(n^2) DFTs, for every n (44, 128 as a shifted pass, 130 ... 256): each output is a
  sequential sum of n complex products with float32 twiddles (error <= u each), so its error is at most (n + 3) u times
  sum |x_j| <= (n + 3) sqrt(n) u |x| (Cauchy-Schwarz); the inverse's I = n + 3 likewise.  No step depends on n <= 128.

The inventory is the library's own: a Python mirror of xcorr_kernel_name (piv_launch.hip) is checked against
Plan.kernel_name at every size on the device, and the case table must hold a case for every distinct name the mirror
yields (test_every_kernel_name_has_a_case runs without a GPU).

The mutant library tools/diag/libtorchpiv_hip_mutant_tw.so (TPIV_MUTANT_TWIDDLE, fft_inreg.hpp: w_N^1 of every codelet
scaled by 1 + 1e-4; the plain DFT's table entry w_N^1 by 1 + 1e-2, see xcorr_generic.hip) must fail the map check at every
instance it was compiled into (all but the first pass's xcorr_big128_kernel) -- in one child process,
tests/shifted_maps_probe.py.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from oracle import piv_oracle as O
from test_exact_scheme import gamma_u, mixed_factors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUTANT_TW = os.path.join(ROOT, "tools", "diag", "libtorchpiv_hip_mutant_tw.so")

U32 = 2.0 ** -24
PASS1, DWS, CWS, CWSF = 0, 1, 2, 3
MODE_KEYS = {PASS1: 0, DWS: "DWS", CWS: "CWS", CWSF: "CWS_Fast"}
REGISTER_SIZES = [12, 14, 18, 20, 24, 28, 30, 36, 40, 42, 48, 56]       # TPIV_CT_REGISTER_SIZES, csrc/xcorr_generic.hip
VAL_RATIO, VAL_WIN = 1.2, 3                                              # what tpiv_debug_pass runs with
SHIFT_SIZES = range(2, 257)                                              # shifted passes (check_window: 2 ... 256)
PASS1_SIZES = range(8, 129)                                              # "fast" first pass
# Odd sizes are in the dispatch space but not in the map check: the generic kernel reproduces the reference's ws x (ws - 1)
# irfft2 map for them and writes no debug map (xcorr_generic.hip: `!odd`).  Their kernel, xcorr_generic_kernel<mode, float>,
# is the one of the even sizes without a two-factor split, which the case table covers (44, 128).  Their FIRST pass (the
# float64 generic kernel, at every precision but "fast") is checked at the field level against a longdouble map in
# tests/test_gpu_f64_pass1.py.
ODD_EXCLUDED = "odd window sizes: no debug map (xcorr_generic.hip `!odd`); their kernel is covered at even sizes"
EXCUSE_CAP = 0.02          # share of a case's non-constant windows that may be excused by a decision inside the band


def ct_usable(ws):
    """xcorr_generic.hip ct_usable(ws, 0): even, 4 ... 96, n = n1 n2 with 2 <= n1 <= n2 <= 8 (the LDS limit holds at 96)."""
    return ws % 2 == 0 and 4 <= ws <= 96 and mixed_factors(ws) is not None


def kernel_name(ws, mode, precision):
    """xcorr_kernel_name (piv_launch.hip) for the float32 kernels: shifted passes at any precision ("reference" selects the
    reference-order instances <..., false> of the tile sizes; "fast", "f64" and "exact" the fast order), pass 1 at "fast"."""
    tf = "false" if (precision == "reference" and mode != PASS1) else "true"
    if mode == CWSF:
        return "xcorr_generic_ct_kernel<3, 0>" if ct_usable(ws) else "xcorr_generic_kernel<3, float>"
    if ws == 8:
        return f"xcorr_w8_kernel<{mode}, {tf}>"
    if ws in (16, 32, 64):
        occ = 4 if ws == 16 else (3 if (ws == 32 or mode != CWS) else 2)
        return f"xcorr_tile_kernel<{ws}, {mode}, {occ}, {tf}>"
    if ws == 128 and mode == PASS1:
        return "xcorr_big128_kernel"
    if ct_usable(ws):
        return f"xcorr_generic_ct_kernel<{mode}, {ws if ws in REGISTER_SIZES else 0}>"
    return f"xcorr_generic_kernel<{mode}, float>"


def transform_kind(ws, mode):
    """The transform the instance runs, for Gamma: the tile kernels, the w8 kernel and the 128x128 first pass radix-2/4
    codelets (fft_inreg.hpp); the second-generation generic kernel the mixed-radix ones (fft_mixed.hpp / radix_pass); every
    other size -- among them 128 and 130 ... 256 as shifted passes -- the plain O(n^2) DFTs of xcorr_generic_kernel."""
    if mode != CWSF and (ws in (8, 16, 32, 64) or (ws == 128 and mode == PASS1)):
        return "radix2"
    return "mixed" if ct_usable(ws) else "plain"


def dispatch_space():
    """(mode, ws, precision) of every float32 instance a shifted pass or a "fast" first pass can run, odd sizes excluded."""
    out = [(m, ws, prec) for m in (DWS, CWS) for prec in ("fast", "reference") for ws in SHIFT_SIZES if ws % 2 == 0]
    out += [(CWSF, ws, "fast") for ws in SHIFT_SIZES if ws % 2 == 0]
    out += [(PASS1, ws, "fast") for ws in PASS1_SIZES if ws % 2 == 0]
    return out


# the case table: (mode, ws, precision) -- one or more per distinct kernel name (test_every_kernel_name_has_a_case)
CASES = (
    [(m, ws, prec) for m in (DWS, CWS) for prec in ("fast", "reference") for ws in (8, 16, 32, 64)]
    + [(m, n, "fast") for m in (DWS, CWS) for n in REGISTER_SIZES]
    + [(m, ws, "fast") for m in (DWS, CWS) for ws in (10, 44, 128)]        # run-time ct form; plain DFT (44 = 4 x 11, 128)
    + [(CWSF, 32, "fast"), (CWSF, 44, "fast")]
    + [(PASS1, ws, "fast") for ws in (8, 16, 32, 64, 128, 10, 44)] + [(PASS1, n, "fast") for n in REGISTER_SIZES]
)


def case_id(c):
    return f"{MODE_KEYS[c[0]] or 'PASS1'}-{c[1]}-{c[2]}"


def test_every_kernel_name_has_a_case():
    """The case table covers every distinct kernel name of the dispatch space (a new instantiation fails here until a case
    is added); every case is itself in the space."""
    names = {}
    for c in dispatch_space():
        names.setdefault(kernel_name(c[1], c[0], c[2]), []).append(c)
    covered = {}
    for c in CASES:
        assert c in dispatch_space(), c
        covered.setdefault(kernel_name(c[1], c[0], c[2]), []).append(case_id(c))
    missing = sorted(set(names) - set(covered))
    print(f"  {len(names)} kernel names; odd sizes excluded ({ODD_EXCLUDED})")
    for n in sorted(names):
        print(f"    {n:44s} <- {', '.join(covered.get(n, ['-']))}")
    assert not missing, missing
    assert len(names) >= 60, len(names)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
def frame_geometry(ws):
    """A few windows in each direction (more for small windows), overlap ws / 2: border and interior windows both occur."""
    st = ws - ws // 2
    k = max(4, -(-96 // st))
    return ws + st * (k - 1), ws // 2


def families(H, W, ws, seed):
    """uint8 frame pairs [F, 2, H, W]: synthetic particles, synth `wavy`, uniform random bytes in 2 x 2 grains (b a shifted
    copy of a with 5 % of its pixels redrawn), the same texture as a bright background with low contrast (192 ... 208 grey levels),
    saturated blobs,
    half-black frames."""
    from torchpiv_amd import synth
    rng = np.random.default_rng(seed)
    pa, pb = (t.numpy() for t in synth.make_pair(H, W, seed, kind="shear", noise=2.0))
    wa, wb = (t.numpy() for t in synth.make_pair(H, W, seed + 1, kind="wavy", noise=3.0))
    # (2 x 2 pixels per random byte: white noise correlates to a one-cell spike whose fit neighbours sit at the map minimum,
    #  where the log of corr - min + 1e-7 leaves every band; a two-pixel grain gives the peak neighbours the fit can use)
    ra = np.repeat(np.repeat(rng.integers(0, 256, ((H + 1) // 2, (W + 1) // 2)), 2, axis=0), 2, axis=1)[:H, :W].astype(np.uint8)
    rb = np.roll(ra, (2, -3), axis=(0, 1))
    redraw = rng.random((H, W)) < 0.05
    rb = np.where(redraw, rng.integers(0, 256, (H, W)), rb).astype(np.uint8)
    bright = [(192 + (x.astype(np.int32) * 16 + 127) // 255).astype(np.uint8) for x in (ra, rb)]
    sat = [np.minimum(x.astype(np.int32) * 6, 255).astype(np.uint8) for x in (wa, wb)]
    half = [x.copy() for x in (pa, pb)]
    for x in half:
        x[:, : W // 2 + ws // 4] = 0
    fams = [("particles", pa, pb), ("wavy", wa, wb), ("random", ra, rb), ("bright", *bright), ("saturated", *sat),
            ("halfblack", *half)]
    return [f[0] for f in fams], np.stack([np.stack(f[1:]) for f in fams])


def predictors(mode, ws, F, nr, nc, seed):
    """{family: (u2, v2) [F, nr, nc]}: random fractional shifts up to +-9 px; exact integers and half-integers (CWS: integral
    row coordinates, which send 64 x 64 items to the per-pixel path); shifts that push border windows off the frame edge
    (each window moved away from the frame centre, so the border windows' samples leave the frame).  DWS: tpiv_debug_pass
    takes the half shift after the predictor's rint (B:782-785), so it gets integers in every family and no rint tie can
    be exercised through it (the ties belong to the predictor hand-off: tests/test_gpu_handoff.py,
    test_compact_and_four_field_hand_off, plants them; tests/test_handoff_model.py pins the rule)."""
    rng = np.random.default_rng(seed)
    integral = mode == DWS
    r = rng.uniform(-9, 9, (2, F, nr, nc))
    h = rng.integers(-12, 13, (2, F, nr, nc)) / 2.0
    mag = min(9.0, ws / 4 + 2) + (0 if integral else 0.375)
    gy, gx = np.meshgrid(np.arange(nr) - (nr - 1) / 2, np.arange(nc) - (nc - 1) / 2, indexing="ij")
    out = np.stack([np.broadcast_to(np.sign(gx) * mag, (F, nr, nc)), np.broadcast_to(np.sign(gy) * mag, (F, nr, nc))])
    fams = {"random": r, "integral": h, "outward": out}
    if integral:
        fams = {k: np.rint(v) for k, v in fams.items()}
    return {k: (np.ascontiguousarray(v[0]), np.ascontiguousarray(v[1])) for k, v in fams.items()}


def leaves_frame(H, W, ws, ov, u2, v2):
    """Windows of a CWS pass whose samples (either frame, bilinear support included) leave the frame."""
    nr, nc = O.field_shape((H, W), ws, ov)
    st = ws - ov
    x0 = (np.arange(nc) * st)[None, None, :]
    y0 = (np.arange(nr) * st)[None, :, None]
    lo_x, hi_x = x0 - np.abs(u2) - 1, x0 + ws - 1 + np.abs(u2) + 1
    lo_y, hi_y = y0 - np.abs(v2) - 1, y0 + ws - 1 + np.abs(v2) + 1
    return (lo_x < 0) | (hi_x > W - 1) | (lo_y < 0) | (hi_y > H - 1)


# ---------------------------------------------------------------------------------------------------------------------
# float64 side
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


def scales(wa, wb, mode):
    """The error scale S of the arithmetic the instance performs, per window ("Shifted-pass maps").
    Pass 1 and CWS_Fast transform mean-normalised windows a' = a / mean(a) - 1: S = E+ = (|a'|^2 + |b'|^2) / 2.
    DWS / CWS transform the raw samples; the mean leaves them in front of the transform (reference order), after the row
    transform (fast order, tile kernels) or in the cross-spectrum's DC bin (fast order, w8): a forward transform's
    rounding scales with the raw norm |a| of what it transformed, and it meets the other window's spectrum, whose mean is
    gone, in the cross-spectrum.  So every error term of Gamma is a product |a| |b'|, |a'| |b| or |a'| |b'| (a' = a -
    mean(a)), and S = max(|a| |b'|, |a'| |b|) bounds all three -- it is at most the raw energy (|a|^2 + |b|^2) / 2 the
    earlier test used, and a bright, low-contrast window gets |a| / |a'| (about 40 at 200 +- 8) instead of its square."""
    ca = wa - wa.mean(axis=(1, 2), keepdims=True)
    cb = wb - wb.mean(axis=(1, 2), keepdims=True)
    ea, eb = (ca ** 2).sum(axis=(1, 2)), (cb ** 2).sum(axis=(1, 2))
    if mode in (PASS1, CWSF):
        with np.errstate(all="ignore"):
            ma, mb = wa.mean(axis=(1, 2)), wb.mean(axis=(1, 2))
            s = 0.5 * (ea / ma ** 2 + eb / mb ** 2)
        const = (ma == 0) | (mb == 0) | (ea == 0) | (eb == 0)
        return np.where(const, 0.0, s), const
    ra, rb = (wa ** 2).sum(axis=(1, 2)), (wb ** 2).sum(axis=(1, 2))
    s = np.maximum(np.sqrt(ra * eb), np.sqrt(ea * rb))
    return s, (ea == 0) | (eb == 0)


def neighbours(m, k, d):
    """B:385-392 flat-index neighbours with the reference's one-sided fix-ups (they follow from m alone)."""
    kd = k * d
    left, right, top, bot = m + 1, m - 1, m + k, m - k
    left = np.where(left >= kd - 1, m, left)
    right = np.where(right <= 0, m, right)
    top = np.where(top >= kd - 1, m, top)
    bot = np.where(bot <= 0, m, bot)
    return left, right, top, bot


def fit_bound(c, i_m, i_1, i_2, delta):
    """Worst |change| of (log c2 - log c1) / (2 (log c1 + log c2) - 4 log cm) (B:399-407) over cells each within delta of
    the given values (interval arithmetic on the logs: nominator and denominator bounded separately); inf where a cell's
    interval reaches 0 or the denominator's interval contains 0 (the fit itself is then a decision inside the band)."""
    rows = np.arange(len(c))
    cm, c1, c2 = c[rows, i_m], c[rows, i_1], c[rows, i_2]
    with np.errstate(all="ignore"):
        lo = [np.log(np.maximum(x - delta, 0.0)) for x in (cm, c1, c2)]
        hi = [np.log(x + delta) for x in (cm, c1, c2)]
        nom0 = np.log(c2) - np.log(c1)
        den0 = 2 * (np.log(c1) + np.log(c2)) - 4 * np.log(cm)
        nom = (lo[2] - hi[1], hi[2] - lo[1])
        den = (2 * (lo[1] + lo[2]) - 4 * hi[0], 2 * (hi[1] + hi[2]) - 4 * lo[0])
        f0 = nom0 / den0
        worst = np.max([np.abs(n / dd - f0) for n in nom for dd in den], axis=0)
    bad = ~np.isfinite(worst) | (den[0] <= 0) & (den[1] >= 0) | ~np.isfinite(f0)
    return np.where(bad, np.inf, worst)


def expected_fields(c64, beta):
    """corr_to_disp (val_ratio 1.2, val_win 3) on the float64 maps, plus per window: the bound of |du|, |dv| implied by a map
    error of at most delta = 2 beta per cell (beta the offset-free spread: the kernel's map is c64 + o + e with |e| <= beta,
    and after both maps subtract their own minimum, |o| <= beta more), and
    the discrete decisions that lie inside that band: arg-max margin, peak ratio against val_ratio, the fit itself."""
    n, ws, _ = c64.shape
    du, dv, inv = O.corr_to_disp(c64, n, 1, True, VAL_RATIO, VAL_WIN)
    du, dv, inv = du[:, 0], dv[:, 0], inv[:, 0]
    delta = 2.0 * beta
    c = c64.reshape(n, -1) + O.EPS
    m = np.argmax(c, axis=1)
    srt = np.sort(c, axis=1)
    near_argmax = (srt[:, -1] - srt[:, -2]) <= 2 * delta
    work = c.copy()
    m2 = O.second_peak(work, m, VAL_WIN, ws, ws)
    rows = np.arange(n)
    cm, c2 = c[rows, m], c[rows, m2]
    with np.errstate(all="ignore"):
        r_lo = (cm - delta) / (c2 + delta)
        r_hi = np.where(c2 - delta > 0, (cm + delta) / (c2 - delta), np.inf)
    near_ratio = (r_lo <= VAL_RATIO) & (r_hi >= VAL_RATIO)
    left, right, top, bot = neighbours(m, ws, ws)
    bu = fit_bound(c, m, left, right, delta)
    bv = fit_bound(c, m, top, bot, delta)
    return du, dv, inv.astype(bool), bu, bv, {"argmax": near_argmax, "ratio": near_ratio,
                                              "fit": ~np.isfinite(bu) | ~np.isfinite(bv)}


# ---------------------------------------------------------------------------------------------------------------------
def run_case(eng, mode, ws, precision, seed=0):
    """One case: every window family x every predictor family through tpiv_debug_pass; returns a report (no assertions, so
    that the mutant probe can use it)."""
    H, ov = frame_geometry(ws)
    nr, nc = O.field_shape((H, H), ws, ov)
    fam_names, frames = families(H, H, ws, 1000 + 7 * ws + mode + seed)
    F = len(fam_names)
    A = torch.from_numpy(np.ascontiguousarray(frames[:, 0])).cuda()
    B = torch.from_numpy(np.ascontiguousarray(frames[:, 1])).cuda()
    kind = transform_kind(ws, mode)
    gam = gamma_u(ws, kind) * U32
    preds = {"none": None} if mode == PASS1 else predictors(mode, ws, F, nr, nc, 77 + ws + mode)
    rep = {"name": kernel_name(ws, mode, precision), "kind": kind, "gamma": gam, "map_worst": 0.0, "field_worst": 0.0,
           "field_median": 0.0, "excused": 0, "cap": 0, "windows": 0, "mismatch": [], "per_family_map": {},
           "leaving": 0}
    ratios, fields, n_nonconst, excused = [], [], 0, []
    for pname, pr in preds.items():
        if pr is None:
            u, v, inv, _, corr = eng.debug_pass(0, A, B, ws, ov, precision=precision)
            wa = np.stack([O.windows(f, ws, ov) for f in frames[:, 0]]).astype(np.float64).reshape(-1, ws, ws)
            wb = np.stack([O.windows(f, ws, ov) for f in frames[:, 1]]).astype(np.float64).reshape(-1, ws, ws)
            u2 = v2 = np.zeros((F, nr, nc))
        else:
            u2, v2 = pr
            tu, tv = torch.from_numpy(u2).cuda(), torch.from_numpy(v2).cuda()
            u, v, inv, win, corr = eng.debug_pass(MODE_KEYS[mode], A, B, ws, ov, tu, tv, precision=precision)
            w = win.cpu().numpy().astype(np.float64).reshape(-1, 2, ws, ws)
            wa, wb = w[:, 0], w[:, 1]
            if mode == CWS:
                rep["leaving"] += int(leaves_frame(H, H, ws, ov, u2, v2).sum())
        got = corr.cpu().numpy().reshape(-1, ws, ws)
        u, v = u.cpu().numpy().reshape(-1), v.cpu().numpy().reshape(-1)
        inv = inv.cpu().numpy().reshape(-1).astype(bool)
        S, const = scales(wa, wb, mode)
        if mode in (PASS1, CWSF):
            with np.errstate(all="ignore"):
                na = wa / wa.mean(axis=(1, 2), keepdims=True) - 1
                nb = wb / wb.mean(axis=(1, 2), keepdims=True) - 1
            want = map64(np.nan_to_num(na), np.nan_to_num(nb))
        else:
            want = map64(wa - wa.mean(axis=(1, 2), keepdims=True), wb - wb.mean(axis=(1, 2), keepdims=True))
        keep = ~const
        r = np.zeros(len(got))
        r[keep] = err_ratio(got[keep], want[keep], gam * S[keep])
        ratios.append(r[keep])
        fam_of = np.repeat(np.arange(F), nr * nc)
        for fi, fn in enumerate(fam_names):
            sel = keep & (fam_of == fi)
            if sel.any():
                key = f"{fn}/{pname}"
                rep["per_family_map"][key] = float(r[sel].max())
        # ---- fields
        h = np.zeros(len(got))
        h[keep] = r[keep] * gam * S[keep]         # the window's measured spread, <= Gamma S (the map level asserts it)
        du_e, dv_e, inv_e, bu, bv, near = expected_fields(want, h)
        u2f, v2f = u2.reshape(-1), v2.reshape(-1)
        if mode == CWSF:       # u = u0 + du unless masked (B:663-672); u0 = the given predictor, no invalid-zeroing here
            mu = ((du_e > u2f) & (np.rint(u2f) > 0)) | inv_e
            mv = ((dv_e > v2f) & (np.rint(v2f) > 0)) | inv_e
            near_mask = ((np.abs(du_e - u2f) <= bu) & (np.rint(u2f) > 0)) | ((np.abs(dv_e - v2f) <= bv) & (np.rint(v2f) > 0))
            ue, ve = np.where(mu, u2f, u2f + du_e), np.where(mv, v2f, v2f + dv_e)
            gu, gv = u, v
        else:
            near_mask = np.zeros(len(u), bool)
            ue, ve = du_e, dv_e
            if mode == PASS1:
                gu, gv = u, v
            else:               # valid: u = 2 u2 + du; invalid: 0 (u0 = 0)
                gu, gv = u - 2 * u2f, v - 2 * v2f
        exc = keep & (near["argmax"] | near["ratio"] | near["fit"] | near_mask)
        chk = keep & ~exc
        n_nonconst += int(keep.sum())
        for i in np.flatnonzero(exc):
            why = [k for k in ("argmax", "ratio", "fit") if near[k][i]] + (["mask"] if near_mask[i] else [])
            excused.append(f"{fam_names[fam_of[i]]}/{pname}#{i % (nr * nc)}:{'+'.join(why)}")
        flip = chk & (inv != inv_e)
        for i in np.flatnonzero(flip)[:5]:
            rep["mismatch"].append(f"{fam_names[fam_of[i]]}/{pname}#{i % (nr * nc)}: invalid {inv[i]} vs {inv_e[i]}")
        both = chk & ~inv_e & ~flip if mode != CWSF else chk & ~flip
        slack = 1e-9       # float64 evaluation of the fit on both sides, and u - 2 u2
        fu = np.abs(gu - ue)[both] / (bu[both] + slack)
        fv = np.abs(gv - ve)[both] / (bv[both] + slack)
        fields.append(np.maximum(fu, fv))
        for i in np.flatnonzero(both)[np.maximum(fu, fv) >= 1][:5]:
            rep["mismatch"].append(f"{fam_names[fam_of[i]]}/{pname}#{i % (nr * nc)}: u {gu[i]:.9f} vs {ue[i]:.9f} "
                                   f"(bound {bu[i]:.2e}), v {gv[i]:.9f} vs {ve[i]:.9f} (bound {bv[i]:.2e})")
    r = np.concatenate(ratios)
    f = np.concatenate(fields)
    rep["map_worst"] = float(r.max())
    rep["map_median"] = float(np.median(r))
    rep["field_worst"] = float(f.max()) if f.size else 0.0
    rep["field_median"] = float(np.median(f)) if f.size else 0.0
    rep["windows"] = n_nonconst
    rep["excused"] = len(excused)
    rep["excused_list"] = excused[:12]
    rep["cap"] = max(1, int(EXCUSE_CAP * n_nonconst))
    return rep


def case_failures(rep):
    """What the shipped library must satisfy: map inside the band; fields inside their bounds with identical validity
    outside the excused windows; at most the capped number excused."""
    out = []
    if not rep["map_worst"] < 1:
        out.append(f"map {rep['map_worst']:.3g} x bound")
    if not rep["field_worst"] < 1 or rep["mismatch"]:
        out.append(f"field {rep['field_worst']:.3g} x bound; {rep['mismatch'][:3]}")
    if rep["excused"] > rep["cap"]:
        out.append(f"excused {rep['excused']} > cap {rep['cap']}: {rep['excused_list']}")
    return out


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


@pytest.mark.gpu
def test_the_mirror_is_the_librarys(eng):
    """kernel_name above against Plan.kernel_name: pass 2 of a 2-pass plan (multipass_scale 1: the same window size) for
    every size 2 ... 256, DWS and CWS, at "fast" (the fast order, also run by "f64" and "exact") and "reference"; pass 1 of
    the "fast" plans for 8 ... 128."""
    checked = 0
    for ws in SHIFT_SIZES:
        for mode in (DWS, CWS):
            for prec in ("fast", "reference", "exact"):
                H = 3 * ws + 2          # (4 coarse points per axis: the spline predictor's minimum)
                plan = eng.Plan(H, H, ws, ws // 2, n_pass=2, mode=MODE_KEYS[mode], pass_scale=1.0, max_batch=1,
                                precision=prec)
                assert plan.geometry[1][0] == ws
                assert plan.kernel_name(1) == kernel_name(ws, mode, prec), (ws, mode, prec, plan.kernel_name(1))
                if prec == "fast" and ws in PASS1_SIZES:
                    assert plan.kernel_name(0) == kernel_name(ws, PASS1, prec), (ws, plan.kernel_name(0))
                plan.close()
                checked += 1
    print(f"  {checked} plans: kernel names as the mirror says")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_shifted_maps_and_fields(eng, case):
    mode, ws, precision = case
    t0 = time.time()
    rep = run_case(eng, mode, ws, precision)
    print(f"  {case_id(case):22s} {rep['name']:40s} map {rep['map_worst']:.3f} (median {rep['map_median']:.3f}) "
          f"field {rep['field_worst']:.3f} (median {rep['field_median']:.2e}) excused {rep['excused']}/{rep['cap']} "
          f"of {rep['windows']}  {time.time() - t0:.1f} s")
    if rep["excused"]:
        print("    excused:", rep["excused_list"])
    if mode == CWS and ws == 64 and precision == "fast":
        # both launches of the 64 x 64 CWS pass run: the fast-path kernel sets aside the items whose samples leave the frame
        # (and those at integral row coordinates) for the per-pixel kernel in list mode -- the outward family's border
        # windows are such items by construction
        assert rep["leaving"] > 0, rep
    fails = case_failures(rep)
    assert not fails, (case_id(case), fails)


@pytest.mark.gpu
def test_mutant_twiddle_is_caught():
    """The twiddle mutant (w_N^1 x (1 + 1e-4) in every codelet of the units of the float32 kernels) in ONE child process:
    the map check fails at every instance compiled with it."""
    if not os.path.exists(MUTANT_TW):         # normally built by `make` (build()); a bare checkout builds it here
        subprocess.run(["make", "-C", os.path.join(ROOT, "torchpiv_amd", "csrc"), "-j", "8", "mutant_tw"], check=True,
                       timeout=1800)
    env = dict(os.environ, TPIV_LIB=MUTANT_TW)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shifted_maps_probe.py")], env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("PROBE ")][-1]
    out = json.loads(line[len("PROBE "):])
    assert out["lib"] == MUTANT_TW
    field_caught = caught = 0
    for cid, rep in out["cases"].items():
        print(f"  mutant {cid:22s} {rep['name']:40s} map {rep['map_worst']:.2f} x bound, field {rep['field_worst']:.2f}, "
              f"mismatches {rep['n_mismatch']}")
        if rep["name"] != "xcorr_big128_kernel":          # (xcorr_ws128.hip is not compiled with the switch)
            assert rep["map_worst"] > 1, (cid, rep)
            caught += 1
        field_caught += rep["field_worst"] > 1 or rep["n_mismatch"] > 0
    # (the field level takes its band from the window's own map error, so it checks the peak stage on the kernel's map: a
    #  transform error moves map and band together and is the map level's to catch -- reported, not asserted)
    print(f"  map check caught {caught} of {caught} mutated instances; field level flagged {field_caught}")
