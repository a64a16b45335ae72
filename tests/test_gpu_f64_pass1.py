"""The float64 first-pass kernels -- the referee of about ten other GPU tests -- against the reference's pass 1 evaluated on
EXACT integer correlation sums (even sizes) or a longdouble map (odd sizes): tests/pass1_reference.py.

Inventory.  kernel_name below mirrors xcorr_kernel_name (piv_launch.hip) for pass 1 at "f64", and at "exact" for the sizes
exact_size() rejects (odd ones, 2 ... 6, 130 ... 256), over every window size check_window accepts; it is checked against
Plan.kernel_name on the device, and the case table must hold a case for every distinct name plus every list form (LIST_FORMS:
they have no name of their own in xcorr_kernel_name).

Gate A (proven).  Every cell of a float64 kernel's map lies within Gamma(ws, kind) 2^-53 E0 of the exact one (DESIGN.md
3.4c: radix2 for the tile and split kernels, plain for xcorr_generic_kernel<0, double>; E0 is the energy of the windows WITH
their DC pedestal, which these kernels transform -- pass1_reference.window_stats -- where the float32 locating pass has E+).  That band, carried through the
log-Gaussian fit by interval arithmetic, bounds |du|, |dv| per window; the kernel's field must lie inside it and its validity
flag must equal the reference's.  A window is excused only where a discrete decision lies inside the band; the excused set
is a function of the exact map alone, is computed without a GPU (test_excused_share_of_every_case), and holds at most 1 % of
a case's non-constant windows.  Dead windows (a zero sum) must give u = v = 0, valid; constant ones are counted apart.

Gate B (tight), per window and axis: |err| <= margin * max(W * bound, 4 ulp(max(|field|, 1))), where W is the worst
error / bound ratio of the CPU oracle's float64 pass (O.pass1, numpy / MKL transform) over the case's windows, bound the
window's own gate-A bound, and margin = 4 gamma_u(ws, kind) / gamma_u(ws, radix2).  The floor, four ulps of the window's own
field value, is there only so that an oracle that happens to be exact does not make the gate impossible; it decides for
0 ... 33 % of a case's window axes (those whose own bound is smallest) and the oracle for the rest.  Measured ratios of both:
profiles/f64_pass1/ratios.txt and DESIGN.md 4.

The window families whose exact map is tied by construction (band_windows leaves them out) run in cases of their own
(f64-*-tied): windows whose two largest exact cells are equal are counted apart there, like constant ones; every window, tied,
constant or excused, must still give a finite displacement inside the window, constant windows the reference's validity flag
where that decision lies outside the band, and the remaining windows pass both gates.

List forms run only behind the locating pass of precision "exact": a child process (tests/f64_pass1_probe.py) sets
TPIV_EXACT_BAND_SCALE so large that every live window is undecided, and Plan.exact_fallbacks() must report at least 99 % of
the non-dead windows.  The mutant tools/diag/libtorchpiv_hip_mutant_tw64.so (TPIV_MUTANT_TWIDDLE_F64: w_N^1 of the float64
codelets scaled by 1 + 1.9e-13, entry 1 of the plain DFT's double table by 1 + 1.9e-11) must fail gate A or B at every
instance, full and list form, in one child process.

Wall time of the whole file on one MI355X: 17 s for its 52 GPU tests (the CPU tests of this file: 20 s).
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
from test_exact_scheme import gamma_u, synthetic_pair
import pass1_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "f64_pass1_probe.py")
MUTANT_TW64 = os.path.join(ROOT, "tools", "diag", "libtorchpiv_hip_mutant_tw64.so")
EXCUSE_CAP = 0.01                  # pass 1: share of a case's non-constant windows a decision inside the band may excuse
BAND_SCALE_ALL = "1e6"             # TPIV_EXACT_BAND_SCALE of the forced-list child: every live window undecided
SIZES = [ws for ws in range(2, 257) if ws % 2 == 0 or ws >= 3]
TILE_WPW = {8: 8, 16: 4, 32: 2}    # F64TileGeo<WS>::WPW = 64 / WS (xcorr_f64.hip)
ODD_SIZES = (3, 5, 9, 33, 63, 65, 127, 129, 255)


def exact_size(ws):
    """piv_launch.hip exact_size / xcorr_exact.hip exact_refine_size: every even size from 8 to 128."""
    return ws % 2 == 0 and 8 <= ws <= 128


def kernel_name(ws, precision):
    """xcorr_kernel_name (piv_launch.hip) for pass 1 where a float64 kernel runs it; None where "exact" runs its scheme."""
    if precision == "exact" and exact_size(ws):
        return None
    if ws in (64, 128):
        return f"xcorr_f64_split_kernel<{ws}>"
    if ws in (8, 16, 32):
        return f"xcorr_f64_tile_kernel<{ws}>"
    return "xcorr_generic_kernel<0, double>"


def kind_of_f64(ws):
    """The transform for Gamma: radix-2/4 codelets in the tile and split kernels, the plain O(n^2) DFT elsewhere."""
    return "radix2" if ws in (8, 16, 32, 64, 128) else "plain"


def margin_b(ws):
    return 4.0 * gamma_u(ws, kind_of_f64(ws)) / gamma_u(ws, "radix2")


# The list forms: the float64 pass over PassParams::fb_list behind the locating pass of precision "exact" (launch_xcorr,
# `p.precision == 3`).  xcorr_kernel_name reports the locating kernel there, so these are listed by hand.
LIST_FORMS = {
    "xcorr_f64_tile_list_kernel<8>": 8,            # launch_xcorr_f64_list, case 8
    "xcorr_f64_tile_list_kernel<16>": 16,          # ... case 16
    "xcorr_f64_tile_list_kernel<32>": 32,          # ... case 32
    "xcorr_f64_list_kernel<64>": 64,               # ... case 64
    "xcorr_f64_split_kernel<128> (list)": 128,     # ... case 128: the one 128 x 128 instance, its run-time list branch
    "xcorr_generic_kernel<0, double> (list)": 22,  # launch_xcorr_generic with fb_list set: every other even size 10 ... 126
}


def list_form(ws):
    for name, w in LIST_FORMS.items():
        if w == ws:
            return name
    return "xcorr_generic_kernel<0, double> (list)"


def dispatch_space():
    return [("f64", ws) for ws in SIZES] + [("exact", ws) for ws in SIZES if not exact_size(ws)]


# ---------------------------------------------------------------------------------------------------------------------
# inputs: every builder returns uint8 frames A, B [batch, H, W]
def tile_windows(wa, wb, ws, cols):
    """Windows side by side, `cols` per frame row, raster order (overlap 0); the last row is padded with dead windows."""
    rows = -(-len(wa) // cols)
    A = np.zeros((1, rows * ws, cols * ws), np.uint8)
    B = np.zeros_like(A)
    for i, (a, b) in enumerate(zip(wa, wb)):
        r, c = divmod(i, cols)
        A[0, r * ws:(r + 1) * ws, c * ws:(c + 1) * ws] = a
        B[0, r * ws:(r + 1) * ws, c * ws:(c + 1) * ws] = b
    return A, B


def family_frames(ws, seed=0, k=None):
    """The six frame families of tests/test_gpu_shifted_maps.py (particles, wavy, random grains, bright low contrast,
    saturated, half black), a batch of six pairs, overlap ws / 2."""
    import test_gpu_shifted_maps as T
    H, _ = T.frame_geometry(ws)
    if k is not None:
        H = ws + (ws - ws // 2) * (k - 1)
    _, fr = T.families(H, H, ws, 500 + 3 * ws + seed)
    if kind_of_f64(ws) == "plain" and ws >= 60:
        # (16 windows per pair there, and the plain DFT's Gamma is 50 x the codelets': the four windows that straddle the
        #  edge of the half-black frame have map cells at the minimum next to the peak, whose logarithm leaves that band --
        #  4 of 92 windows excused where the cap allows none; the smaller sizes keep the family)
        fr = fr[:5]
    return np.ascontiguousarray(fr[:, 0]), np.ascontiguousarray(fr[:, 1])


def band_windows(ws, n=16):
    """tools/research/exact_band.py's window families WITHOUT those whose exact map is tied by construction -- a constant
    or exactly periodic map (the sinusoids, checkerboard against stripes, a ramp that is constant along y), or sums over so
    few distinct products that the largest ones coincide (two grey levels; five dark pixels in a saturated window: every
    shift at which no dark pixels meet gives the same sum; 3 x 3 particles on a true zero or without noise, and four grey levels, at 8 x 8).  Every decision of
    such a window is a true tie, which is what the excuse is for, and a case made of them could not stay under the cap.
    Left: particles at four noise levels, uniform and low-contrast noise, one bright pixel on a pedestal, particles on a
    true-zero background; plus the hill-climbed windows of the fixtures g12 (64) / g13 (other sizes), which bring the
    saturated blocks and impulses."""
    return _band_select(ws, n, tied=False)


TIED_FAMILIES = ("orthogonal sinusoids", "same sinusoid, other phase", "checkerboard vs stripes", "ramp vs noise",
                 "two levels 200/201", "saturated, five dark pixels")
TIED_BELOW_16 = ("particles on a true-zero background", "particles noise 0", "low-contrast noise 100..103")
TIED_FIXTURES = ("checker", "two levels")


def _band_select(ws, n, tied):
    sys.path.insert(0, os.path.join(ROOT, "tools", "research"))
    import exact_band
    out = TIED_FAMILIES + (TIED_BELOW_16 if ws < 16 else ())
    fam = exact_band.families(n=n, seed=ws, W=ws, size=max(512, 4 * ws))
    wa = [x for k_, (a, _) in fam.items() if (k_ in out) == tied for x in a]
    wb = [x for k_, (_, b) in fam.items() if (k_ in out) == tied for x in b]
    if ws == 64:
        g = np.load(os.path.join(ROOT, "tests", "golden", "g12_adversarial.npz"))
        named = [(str(nm), g[f"w{i}"]) for i, nm in enumerate(g["names"])]
    else:
        g = np.load(os.path.join(ROOT, "tests", "golden", "g13_adversarial_sizes.npz"))
        named = [(str(nm), g[f"w{i}"]) for i, (s_, nm) in enumerate(zip(g["sizes"], g["names"])) if int(s_) == ws]
    for nm, P in named:
        if any(t in nm for t in TIED_FIXTURES) == tied:
            wa += list(P[:, 0])
            wb += list(P[:, 1])
    return wa, wb


def tied_windows(ws, n=8):
    """What band_windows leaves out -- the families whose exact map is tied by construction -- plus three constant windows
    (both flat, frame a flat, frame b flat).  They run in cases of their own, with the exactly tied windows counted apart."""
    wa, wb = _band_select(ws, n, tied=True)
    rng = np.random.default_rng(ws)
    flat, noisy = np.full((ws, ws), 77, np.uint8), rng.integers(0, 256, (ws, ws)).astype(np.uint8)
    return wa + [flat, flat, noisy], wb + [np.full((ws, ws), 91, np.uint8), noisy, flat]


def cell_windows(ws, seed):
    """The arg-max on every border row and column and on each clamp (tests/test_gpu_exact_neighbourhood.py builds them)."""
    import test_gpu_exact_neighbourhood as NB
    rng = np.random.default_rng(seed)
    wa, wb = [], []
    for q in NB.target_cells(ws):
        a, b = NB.window_pair(ws, q, rng)
        wa.append(a)
        wb.append(b)
    return wa, wb


def particle_frames(batch, H, W, seed, noise=2.0, density=None):
    fr = [synthetic_pair(H, W, seed + i, shift=(1.3 + 0.7 * i, -2.1 + 0.4 * i), n=density and int(density * H * W), noise=noise)
          for i in range(batch)]
    return np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr])


def noise_frames(batch, H, W, seed):
    """Uniform random bytes with a common shift: for the sizes 2 ... 5, where particle frames tie too often (4 ... 16 map
    cells of small integer sums); sums of products of random bytes tie with probability about 1e-5 per pair of cells."""
    rng = np.random.default_rng(seed)
    A = rng.integers(0, 256, (batch, H + 2, W + 2))
    return A[:, 1:-1, 1:-1].astype(np.uint8), np.clip(A[:, 2:, :-2] + rng.integers(-9, 10, (batch, H, W)), 0, 255).astype(np.uint8)


def run_(frames, ov, val_win=3, val_ratio=1.2):
    return {"frames": frames, "ov": ov, "val_win": val_win, "val_ratio": val_ratio}


def tail_runs(ws, seed):
    """Grid tails: N = 1, a single row, a single column, batch 3 with a frame that is a multiple of nothing and an odd
    overlap, overlap ws - 1 (stride 1), window counts that are no multiple of the windows per wavefront."""
    fr = noise_frames if ws < 6 else (lambda b, H, W, s: particle_frames(b, H, W, s, noise=3.0))
    odd_ov = max(1, ws // 2 - 1) | 1 if ws > 2 else 1
    odd_ov = min(odd_ov, ws - 1)
    return [run_(lambda: fr(1, ws, ws, seed), 0),
            run_(lambda: fr(1, ws, 5 * ws + 3, seed + 1), 0),
            run_(lambda: fr(1, 5 * ws + 1, ws, seed + 2), min(1, ws - 1)),
            run_(lambda: fr(3, 3 * ws + 5, 4 * ws - odd_ov + 3, seed + 3), odd_ov),
            run_(lambda: fr(2, ws + 6, ws + 4, seed + 6), ws - 1)]


def chunk_runs(ws, seed):
    """The work split over eight XCD chunks, chunk = (items + 7) / 8: item counts 1 ... 9, 15, 17 -- a single row of that
    many windows (tile kernels: WPW windows per item, the last item partly idle)."""
    wpw = TILE_WPW.get(ws, 1)
    fr = lambda n, s: particle_frames(1, ws, ws * n, s, noise=3.0)
    return [run_((lambda n=it * wpw - (wpw > 1), s=seed + it: fr(n, s)), 0) for it in (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 17)]


def val_runs(ws, seed):
    """val_win 1 ... 5 (the power-of-two kernels accept 2 val_win < ws) x val_ratio 1.05 / 1.2 / 3.0 on one pair."""
    fr = particle_frames(2, 4 * ws + 3, 5 * ws, seed, noise=4.0)
    return [run_((lambda: fr), ws // 2, wv, vr) for wv in range(1, 6) if 2 * wv < ws or ws not in (8, 16, 32, 64, 128)
            for vr in (1.05, 1.2, 3.0)]


def frames_for(ws, seed):
    """The main frames of a size: families for >= 6, random bytes below (see noise_frames)."""
    if ws < 6:
        return lambda: noise_frames(4, 24 * ws, 24 * ws, seed)
    return lambda: family_frames(ws, seed)


def make_case(cid, ws, precision, runs, forced_list=False, tied_apart=False):
    return {"id": cid, "ws": ws, "precision": precision, "runs": runs, "forced_list": forced_list, "tied_apart": tied_apart}


def build_cases():
    cases = []
    for ws in (8, 16, 32, 64, 128):
        cases.append(make_case(f"f64-{ws}-families", ws, "f64", [run_(frames_for(ws, 1), ws // 2)]))
        cases.append(make_case(f"f64-{ws}-band", ws, "f64", [run_((lambda ws=ws: tile_windows(*band_windows(ws), ws, 7)), 0),
                                                            run_((lambda ws=ws: tile_windows(*cell_windows(ws, 40 + ws), ws, 7)), 0)]))
        cases.append(make_case(f"f64-{ws}-tails", ws, "f64", tail_runs(ws, 60 + ws) + chunk_runs(ws, 80 + ws)))
    for ws in (8, 16, 32, 64, 128, 12):          # the window families tied by construction, tied windows counted apart
        cases.append(make_case(f"f64-{ws}-tied", ws, "f64", [run_((lambda ws=ws: tile_windows(*tied_windows(ws), ws, 7)), 0)],
                               tied_apart=True))
    for ws in (16, 64, 12):
        cases.append(make_case(f"f64-{ws}-validation", ws, "f64", val_runs(ws, 90 + ws)))
    # xcorr_generic_kernel<0, double>: even sizes without a kernel of their own, 130 ... 256, and every odd size
    for ws in (2, 4, 6, 10, 24, 100, 130, 256):
        cases.append(make_case(f"f64-{ws}-families", ws, "f64", [run_(frames_for(ws, 2), ws // 2)]))
    for ws in ODD_SIZES:
        prec = "exact" if ws in (5, 33, 129) else "f64"          # (the same kernel either way: odd sizes have no exact scheme)
        cases.append(make_case(f"{prec}-{ws}-families", ws, prec, [run_(frames_for(ws, 3), ws // 2)]))
    cases.append(make_case("exact-132-families", 132, "exact", [run_(frames_for(132, 4), 66)]))
    cases.append(make_case("f64-12-cells", 12, "f64", [run_((lambda: tile_windows(*cell_windows(12, 52), 12, 7)), 0)]))
    cases.append(make_case("f64-7-tails", 7, "f64", tail_runs(7, 67) + chunk_runs(7, 87)))
    cases.append(make_case("f64-2-tails", 2, "f64", tail_runs(2, 62)))
    # list forms, forced (child process with TPIV_EXACT_BAND_SCALE): families; a list of one; lists that are no multiple
    # of WPW and whose neighbouring entries belong to different pairs (batch 3, five windows each); the XCD chunks
    for ws in (8, 16, 32, 64, 128, 22, 12):
        runs = [run_(frames_for(ws, 5), ws // 2),
                run_((lambda ws=ws: particle_frames(1, ws, ws, 70 + ws, noise=3.0)), 0),
                run_((lambda ws=ws: particle_frames(3, ws, 5 * ws + 1, 71 + ws, noise=3.0)), 0)]
        if ws in (8, 64):
            runs += chunk_runs(ws, 100 + ws)
        cases.append(make_case(f"list-{ws}-forced", ws, "exact", runs, forced_list=True))
    return cases


CASES = build_cases()
# at the normal band: the hill-climbed windows of the adversarial fixtures and the band families, where the list is short
SPARSE_LIST_CASES = [make_case(f"list-{ws}-sparse", ws, "exact", [run_((lambda ws=ws: tile_windows(*band_windows(ws), ws, 7)), 0)])
                     for ws in (16, 64, 128, 22)]
BY_ID = {c["id"]: c for c in CASES + SPARSE_LIST_CASES}


def case_kernel(case):
    return list_form(case["ws"]) if case["id"].startswith("list-") else kernel_name(case["ws"], case["precision"])


# ---------------------------------------------------------------------------------------------------------------------
def run_reference(run, ws, tied_apart=False):
    """Everything of one run that needs no GPU: windows, exact maps, the reference's fields, bounds and the excused set.
    tied_apart (the cases of window families whose exact map is tied by construction): windows whose two largest exact cells
    are EQUAL are counted apart, as constant windows are -- the reference's own arg-max there is the first of equals."""
    A, B = run["frames"]()
    ov = run["ov"]
    wa = np.concatenate([O.windows(f, ws, ov) for f in A])
    wb = np.concatenate([O.windows(f, ws, ov) for f in B])
    sa, sb, ep, dead, const = R.window_stats(wa, wb)
    maps = R.reference_maps(wa, wb)
    ref = R.reference_fields(maps, ep, ws, kind_of_f64(ws), run["val_ratio"], run["val_win"])
    top = np.sort(maps.reshape(len(maps), -1), axis=1)[:, -2:]
    tied = ~dead & ~const & (top[:, 0] == top[:, 1]) & bool(tied_apart)
    live = ~dead & ~const & ~tied
    near = ref["near"]
    exc = live & (near["argmax"] | near["ratio"] | near["fit"])
    return {"A": A, "B": B, "wa": wa, "wb": wb, "ref": ref, "dead": dead, "const": const, "live": live, "excused": exc,
            "tied": tied}


def oracle_fields(A, B, ws, ov, val_ratio):
    out = [O.pass1(a, b, ws, ov, validate=True, validation_ratio=val_ratio) for a, b in zip(A, B)]
    return np.concatenate([o[0].reshape(-1) for o in out]), np.concatenate([o[1].reshape(-1) for o in out])


def device_fields(eng, case, run, A, B):
    """-> u, v, invalid [windows] of the library, and (forced list) the number of windows that took the float64 list."""
    ws = case["ws"]
    a, b = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    n_fb = None
    if case["id"].startswith("list-"):
        plan = eng.Plan(A.shape[1], A.shape[2], ws, run["ov"], n_pass=1, val_ratio=run["val_ratio"], val_win=run["val_win"],
                        max_batch=A.shape[0], precision="exact")
        u, v, inv = (t.clone() for t in plan.run(a, b))
        n_fb = plan.exact_fallbacks()
        plan.close()
    else:
        u, v, inv = eng.pass1(a, b, ws, run["ov"], run["val_ratio"], run["val_win"], precision=case["precision"])
    torch.cuda.synchronize()
    return (u.cpu().numpy().reshape(-1), v.cpu().numpy().reshape(-1), inv.cpu().numpy().reshape(-1).astype(bool), n_fb)


def ulp4(x):
    """Four ulps of a field value (of 1 where it is smaller): gate B's floor, per window and axis."""
    return 4.0 * np.spacing(np.maximum(np.abs(x), 1.0))


def run_case(eng, case):
    """One case on the device: a report, no assertions (the mutant probe uses it too)."""
    ws = case["ws"]
    slack = R.fit_slack(ws)
    rep = {"id": case["id"], "name": case_kernel(case), "ws": ws, "windows": 0, "live": 0, "dead": 0, "const": 0, "tied": 0,
           "excused": 0, "gate_a": 0.0, "oracle": 0.0, "floor_share": 0.0, "mismatch": [], "listed": 0, "flags": 0,
           "const_report": []}
    kept = []                                   # per run: (kernel errors, oracle errors, bounds + slack, reference fields) of the checked windows
    for ri, run in enumerate(case["runs"]):
        cpu = run_reference(run, ws, case.get("tied_apart", False))
        ref, live, dead, const = cpu["ref"], cpu["live"], cpu["dead"], cpu["const"]
        u, v, inv, n_fb = device_fields(eng, case, run, cpu["A"], cpu["B"])
        chk = live & ~cpu["excused"]
        rep["windows"] += len(u)
        rep["live"] += int(live.sum())
        rep["dead"] += int(dead.sum())
        rep["const"] += int(const.sum())
        rep["tied"] += int(cpu["tied"].sum())
        rep["excused"] += int(cpu["excused"].sum())
        if n_fb is not None:
            rep["listed"] += int(n_fb)
        # every window, excused, tied and constant ones too: a finite field inside the window
        wild = ~(np.isfinite(u) & np.isfinite(v)) | (np.abs(u) > ws / 2 + 1) | (np.abs(v) > ws / 2 + 1)
        for i in np.flatnonzero(wild)[:3]:
            rep["mismatch"].append(f"run {ri} window {i}: u {u[i]} v {v[i]} is no displacement inside the window")
        # dead windows: sum 0 gives an all-NaN map in the reference and u = v = 0, valid
        bad_dead = dead & ((u != 0) | (v != 0) | inv)
        for i in np.flatnonzero(bad_dead)[:3]:
            rep["mismatch"].append(f"run {ri} dead window {i}: u {u[i]} v {v[i]} invalid {inv[i]}")
        # constant windows: every cell of the exact map is the 1e-7, so the arg-max and the fit are decided by rounding
        # noise alone, in any float64 transform, the reference's own included (its (0, 0) there is 0 / 0 of exactly equal
        # cells) -- no field value to hold the kernel to.  The validity flag is decided: peak and second peak are both
        # 1e-7 +- delta, ratio 1 < val_ratio, invalid -- wherever that decision lies outside the band and the map is larger
        # than the exclusion zone
        cflag = const & ~ref["near"]["ratio"] & ref["invalid"] & (ws >= 16)
        for i in np.flatnonzero(cflag & ~inv)[:3]:
            rep["mismatch"].append(f"run {ri} constant window {i}: valid, the reference's ratio is 1")
        for i in np.flatnonzero(const)[:4]:
            rep["const_report"].append(f"u {u[i]:.3g} v {v[i]:.3g} invalid {bool(inv[i])} (flag asserted: {bool(cflag[i])})")
        flip = chk & (inv != ref["invalid"])
        rep["flags"] += int(flip.sum())
        for i in np.flatnonzero(flip)[:3]:
            rep["mismatch"].append(f"run {ri} window {i}: invalid {inv[i]} vs {ref['invalid'][i]}")
        ou, ov_ = oracle_fields(cpu["A"], cpu["B"], ws, run["ov"], run["val_ratio"])
        if chk.any():
            den = np.stack([ref["bu"][chk] + slack, ref["bv"][chk] + slack])
            ke = np.stack([np.abs(u - ref["u"])[chk], np.abs(v - ref["v"])[chk]])
            oe = np.stack([np.abs(ou - ref["u"])[chk], np.abs(ov_ - ref["v"])[chk]])
            kept.append((ke, oe, den, np.stack([ref["u"][chk], ref["v"][chk]])))
            ka = (ke / den).max(axis=0)
            rep["gate_a"] = max(rep["gate_a"], float(ka.max()))
            rep["oracle"] = max(rep["oracle"], float((oe / den).max()))
            idx = np.flatnonzero(chk)
            for j in np.flatnonzero(ka >= 1)[:3]:
                i = idx[j]
                rep["mismatch"].append(f"run {ri} window {i}: u {u[i]!r} vs {ref['u'][i]!r} (bound {ref['bu'][i]:.2e}), "
                                       f"v {v[i]!r} vs {ref['v'][i]!r} (bound {ref['bv'][i]:.2e})")
    # gate B, per window and axis: |err| <= margin * max(the oracle's worst ratio of this case x the window's own bound,
    # four ulps of the window's own field value)
    rep["margin"] = margin_b(ws)
    rep["gate_b"] = 0.0
    n_floor = n_all = 0
    for ke, oe, den, fld in kept:
        allowed = np.maximum(rep["oracle"] * den, ulp4(fld))
        rep["gate_b"] = max(rep["gate_b"], float((ke / (rep["margin"] * allowed)).max()))
        n_floor += int((ulp4(fld) > rep["oracle"] * den).sum())
        n_all += ke.size
    rep["floor_share"] = n_floor / max(1, n_all)
    return rep


def case_failures(rep, case):
    out = []
    if not rep["gate_a"] < 1 or rep["mismatch"]:
        out.append(f"gate A: {rep['gate_a']:.3g} x bound, {rep['flags']} flags; {rep['mismatch'][:3]}")
    if not rep["gate_b"] <= 1:
        out.append(f"gate B: {rep['gate_b']:.3g} (kernel {rep['gate_a']:.3g}, oracle {rep['oracle']:.3g}, margin {rep['margin']:.3g})")
    if rep["excused"] > EXCUSE_CAP * rep["live"]:
        out.append(f"excused {rep['excused']} of {rep['live']}")
    not_dead = rep["windows"] - rep["dead"]
    if case["forced_list"] and rep["listed"] < 0.99 * not_dead:
        out.append(f"only {rep['listed']} of {not_dead} non-dead windows took the float64 list")
    if case["id"].endswith("-sparse") and not 0 < rep["listed"] <= not_dead // 2:
        out.append(f"{rep['listed']} of {not_dead} windows listed: the case is meant for a short, sparse list")
    return out


def report_line(rep):
    return (f"{rep['id']:22s} {rep['name']:40s} windows {rep['windows']:5d} live {rep['live']:5d} excused {rep['excused']:3d} "
            f"dead {rep['dead']:3d} const {rep['const']:3d} tied {rep['tied']:3d} listed {rep['listed']:5d} | kernel/bound "
            f"{rep['gate_a']:.3e} oracle/bound {rep['oracle']:.3e} margin {rep['margin']:.1f} B {rep['gate_b']:.3f} "
            f"(floor decides {100 * rep['floor_share']:.0f} %)")


# ---------------------------------------------------------------------------------------------------------------------
# CPU
def test_every_float64_instance_has_a_case():
    """Every distinct kernel name of the dispatch space and every list form has a case; every case is in the space."""
    names = {kernel_name(ws, p) for p, ws in dispatch_space()}
    assert names == {"xcorr_f64_tile_kernel<8>", "xcorr_f64_tile_kernel<16>", "xcorr_f64_tile_kernel<32>",
                     "xcorr_f64_split_kernel<64>", "xcorr_f64_split_kernel<128>", "xcorr_generic_kernel<0, double>"}
    covered = {}
    for c in CASES + SPARSE_LIST_CASES:
        if c["id"].startswith("list-"):
            assert exact_size(c["ws"]) and c["precision"] == "exact", c["id"]
        else:
            assert (c["precision"], c["ws"]) in dispatch_space(), c["id"]
        covered.setdefault(case_kernel(c), []).append(c["id"])
    for n in sorted(names | set(LIST_FORMS)):
        print(f"    {n:44s} <- {', '.join(covered.get(n, ['-']))}")
    assert not (names | set(LIST_FORMS)) - set(covered)
    odd = {c["ws"] for c in CASES if c["ws"] % 2}
    assert odd >= set(ODD_SIZES), odd
    assert len({c["id"] for c in CASES + SPARSE_LIST_CASES}) == len(CASES) + len(SPARSE_LIST_CASES)


@pytest.mark.parametrize("ws", [2, 3, 4, 5, 6, 8])
def test_tie_share_of_the_small_sizes(ws):
    """Why the sizes 2 ... 5 run on random bytes: the share of live windows whose two largest exact sums are equal, on the
    particle frames the other sizes use and on noise_frames; the latter stays under the cap."""
    def share(A, B):
        wa, wb = O.windows(A, ws, ws // 2), O.windows(B, ws, ws // 2)
        _, _, _, dead, const = R.window_stats(wa, wb)
        c = R.reference_maps(wa, wb).reshape(len(wa), -1)
        s = np.sort(c, axis=1)
        live = ~dead & ~const
        return float(((s[:, -1] == s[:, -2]) & live).sum() / max(1, live.sum()))
    pa, pb = synthetic_pair(128, 128, 1)
    na, nb = noise_frames(1, 128, 128, 1)
    sp, sn = share(pa, pb), share(na[0], nb[0])
    print(f"  ws {ws}: tied arg-max on particle frames {sp:.4f}, on random bytes {sn:.4f}")
    if ws % 2 == 0:
        assert sn <= EXCUSE_CAP, (ws, sn)


@pytest.mark.parametrize("case", CASES + SPARSE_LIST_CASES, ids=lambda c: c["id"])
def test_excused_share_of_every_case(case):
    """The excused set is a function of the exact map and the band alone: at most 1 % of a case's non-constant windows, and
    every case checks something."""
    live = exc = dead = const = tied = 0
    why = {"argmax": 0, "ratio": 0, "fit": 0}
    for run in case["runs"]:
        cpu = run_reference(run, case["ws"], case["tied_apart"])
        tied += int(cpu["tied"].sum())
        live += int(cpu["live"].sum())
        exc += int(cpu["excused"].sum())
        dead += int(cpu["dead"].sum())
        const += int(cpu["const"].sum())
        for k in why:
            why[k] += int((cpu["live"] & cpu["ref"]["near"][k]).sum())
    print(f"  {case['id']:22s} live {live:5d} excused {exc:3d} ({why}) dead {dead} const {const} tied {tied}")
    assert live > 0 and exc <= EXCUSE_CAP * live, (case["id"], exc, live, why)


@pytest.mark.parametrize("ws", [3, 9, 33, 65])
def test_odd_reference_is_the_oracles(ws):
    """The longdouble n x (n - 1) map against the CPU oracle's float64 pass 1 on the same windows: same validity flags and
    fields within the windows' own bounds outside the excused set."""
    run = run_(frames_for(ws, 3), ws // 2)
    cpu = run_reference(run, ws)
    ref, chk = cpu["ref"], cpu["live"] & ~cpu["excused"]
    ou, ov_ = oracle_fields(cpu["A"], cpu["B"], ws, run["ov"], run["val_ratio"])
    slack = R.fit_slack(ws)
    r = np.maximum(np.abs(ou - ref["u"])[chk] / (ref["bu"][chk] + slack), np.abs(ov_ - ref["v"])[chk] / (ref["bv"][chk] + slack))
    print(f"  ws {ws}: {int(chk.sum())} windows, oracle / bound {r.max():.3e}, max |d| {np.abs(ou - ref['u'])[chk].max():.2e} px")
    assert chk.sum() > 50 and r.max() < 1, (ws, r.max())


@pytest.mark.parametrize("ws", [9, 32])
def test_a_mean_free_band_does_not_hold_a_float64_transform_with_the_pedestal_in(ws):
    """Why gate A scales with E0 and not with the E+ of the float32 locating pass: on the bright,
    low-contrast family the CPU oracle's own float64 pass leaves a band of Gamma 2^-53 E+, and stays far inside the E0 one."""
    A, B = family_frames(ws, 3)
    wa, wb = O.windows(A[3], ws, ws // 2), O.windows(B[3], ws, ws // 2)
    _, _, e0, dead, const = R.window_stats(wa, wb)
    assert not dead.any() and not const.any()
    ou, ov_ = oracle_fields(A[3:4], B[3:4], ws, ws // 2, 1.2)
    maps = R.reference_maps(wa, wb)
    worst = {}
    for name, scale in (("E+", R.e_plus(wa, wb)), ("E0", e0)):
        ref = R.reference_fields(maps, scale, ws, kind_of_f64(ws), 1.2, 3)
        chk = ~(ref["near"]["argmax"] | ref["near"]["ratio"] | ref["near"]["fit"])
        worst[name] = float(np.maximum(np.abs(ou - ref["u"])[chk] / (ref["bu"][chk] + R.fit_slack(ws)),
                                       np.abs(ov_ - ref["v"])[chk] / (ref["bv"][chk] + R.fit_slack(ws))).max())
    print(f"  ws {ws}: oracle / bound {worst['E+']:.2f} with E+, {worst['E0']:.2e} with E0; E0 / E+ {np.median(e0 / R.e_plus(wa, wb)):.0f}")
    assert worst["E+"] > 1 > 10 * worst["E0"], worst


# ---------------------------------------------------------------------------------------------------------------------
# GPU
@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


@pytest.mark.gpu
def test_the_mirror_is_the_librarys(eng):
    checked = 0
    for prec, ws in dispatch_space():
        plan = eng.Plan(ws + 1, ws + 2, ws, 0, n_pass=1, max_batch=1, precision=prec)
        assert plan.kernel_name(0) == kernel_name(ws, prec), (ws, prec, plan.kernel_name(0))
        plan.close()
        checked += 1
    for ws in SIZES:                 # where "exact" runs its scheme, the float64 kernels serve through the list forms
        if exact_size(ws):
            plan = eng.Plan(ws, ws, ws, 0, n_pass=1, max_batch=1, precision="exact")
            assert "cand" in plan.kernel_name(0), (ws, plan.kernel_name(0))
            plan.close()
    print(f"  {checked} plans: kernel names as the mirror says")


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if not c["forced_list"]] + SPARSE_LIST_CASES, ids=lambda c: c["id"])
def test_f64_pass1_gates(eng, case):
    t0 = time.time()
    rep = run_case(eng, case)
    print(f"  {report_line(rep)}  {time.time() - t0:.1f} s")
    if rep["const_report"]:
        print("    constant windows on the device:", "; ".join(rep["const_report"]))
    fails = case_failures(rep, case)
    assert not fails, (case["id"], fails)


def probe(env_extra, ids, timeout=1500):
    env = dict(os.environ, **env_extra)
    try:
        r = subprocess.run([sys.executable, PROBE, *ids], env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:      # a hung child: nothing more is started on the device in this session
        pytest.exit(f"{PROBE} did not end within {timeout} s: {str(e.stderr)[-2000:]}", returncode=3)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        # the child died on the device: nothing more is started on it in this session
        pytest.exit(f"{PROBE} ended with status {r.returncode}: {r.stderr[-2000:]}", returncode=3)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("PROBE ")][-1]
    return json.loads(line[len("PROBE "):])


@pytest.mark.gpu
def test_list_forms_forced():
    """Every list form behind a locating pass that decides nothing: one child process (the band scale is read once)."""
    ids = [c["id"] for c in CASES if c["forced_list"]]
    out = probe({"TPIV_EXACT_BAND_SCALE": BAND_SCALE_ALL}, ids)
    bad = []
    for cid in ids:
        rep = out["cases"][cid]
        print(f"  {report_line(rep)}")
        fails = case_failures(rep, BY_ID[cid])
        if fails:
            bad.append((cid, fails))
    assert not bad, bad
    assert {out["cases"][c]["name"] for c in ids} >= set(LIST_FORMS)


# one case per instance, full and list form, for the mutant
MUTANT_CASES = ([f"f64-{ws}-families" for ws in (8, 16, 32, 64, 128, 24, 9)] + ["exact-33-families"]
                + [f"list-{ws}-forced" for ws in (8, 16, 32, 64, 128, 22)])


@pytest.mark.gpu
def test_mutant_twiddle_f64_is_caught():
    """tools/diag/libtorchpiv_hip_mutant_tw64.so in ONE child process: gate A or B fails at every float64 instance."""
    if not os.path.exists(MUTANT_TW64):       # normally built by `make` (build()); a bare checkout builds it here
        subprocess.run(["make", "-C", os.path.join(ROOT, "torchpiv_amd", "csrc"), "-j", "8", "mutant_tw64"], check=True,
                       timeout=1800)
    out = probe({"TPIV_LIB": MUTANT_TW64, "TPIV_EXACT_BAND_SCALE": BAND_SCALE_ALL}, MUTANT_CASES)
    assert out["lib"] == MUTANT_TW64
    survived, seen = [], set()
    for cid in MUTANT_CASES:
        rep = out["cases"][cid]
        seen.add(rep["name"])
        fails = [f for f in case_failures(rep, BY_ID[cid]) if f.startswith("gate")]
        print(f"  mutant {report_line(rep)} -> {'caught' if fails else 'SURVIVED'}")
        if not fails:
            survived.append(cid)
    assert not survived, survived
    assert seen >= set(LIST_FORMS) | {kernel_name(ws, "f64") for ws in SIZES}
