"""The decision band of precision="exact" at every window size it covers (every even size 8 ... 128).

The exact first pass is right whenever the float32 map its locating kernel decides on stays within Gamma(ws, kind) E+ of the
exact map, up to a common offset (piv_kernels.h "The band"); Gamma depends on the kind of transform the size
runs: radix-2 (tile kernels, 128x128), two-factor mixed radix (fft_mixed.hpp / radix_pass) or the plain O(n^2) DFT of the
first-generation generic kernel.  Here, per size:
  * the launcher dispatches the kind tests/test_exact_scheme.py::kind_of assumes,
  * the locating kernel's own map (engine.debug_pass(0, ..., precision="exact")) stays below Gamma / 4 on particle,
    noise and hand-built windows (tools/research/exact_band.py's families) and on the hill-climbed windows of
    tests/golden/g13_adversarial_sizes.npz (tools/research/exact_adversarial.py on the MI355X),
  * precision "exact" gives the float64 kernels' fields (1e-11 px) and validity masks on particle frames at a random
    overlap, and their masks on those windows -- with fields within 1e-11 px too, except where the float64 kernel's own
    rounding is amplified further by the log fit (hand-built windows: cells next to the peak at or near the map minimum);
    there the exact pass must give the exact-sum result (1e-12 px).
"""
import os
import sys

import numpy as np
import pytest
import torch

from test_exact_scheme import U32, e_plus, gamma_u, kind_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = list(range(8, 129, 2))
TOL_F64 = 1e-11
N_FAM = 16                 # window pairs per family and size


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def families(ws):
    sys.path.insert(0, os.path.join(ROOT, "tools", "research"))
    import exact_band
    return exact_band.families(n=N_FAM, seed=ws, W=ws, size=512)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def band_ratio(eng, a, b):
    """-> worst |map32 - map| / E+ (up to the common offset) of the locating kernel over the pairs (a[i], b[i]), one window
    each; pairs with a dead window or no variation (E+ = 0) are left out."""
    ws = a.shape[-1]
    keep = (a.reshape(len(a), -1).sum(1) > 0) & (b.reshape(len(b), -1).sum(1) > 0)
    a, b = a[keep], b[keep]
    ep = np.array([e_plus(x, y) for x, y in zip(a, b)])
    a, b, ep = a[ep > 0], b[ep > 0], ep[ep > 0]
    if len(a) == 0:
        return 0.0
    _, _, _, _, corr = eng.debug_pass(0, dev(a), dev(b), ws, 0, precision="exact")
    c32 = corr.cpu().numpy().reshape(-1, ws, ws).astype(np.float64)
    af, bf = a.astype(np.float64), b.astype(np.float64)
    an = af / af.mean(axis=(1, 2), keepdims=True) - 1
    bn = bf / bf.mean(axis=(1, 2), keepdims=True) - 1
    c64 = np.fft.fftshift(np.fft.irfft2(np.conj(np.fft.rfft2(an)) * np.fft.rfft2(bn), s=(ws, ws)), axes=(1, 2))
    e = (c32 - c64).reshape(len(a), -1)
    return float((0.5 * (e.max(axis=1) - e.min(axis=1)) / ep).max())


def exact_vs_f64(eng, A, B, ws, ov):
    """-> (max |exact - f64| px, differing mask cells, windows through the float64 transform, fields of both)."""
    plan = eng.Plan(A.shape[1], A.shape[2], ws, ov, n_pass=1, max_batch=A.shape[0], precision="exact")
    ue, ve, ie = (t.clone() for t in plan.run(A, B))
    n_fb = plan.exact_fallbacks()
    plan.close()
    uf, vf, i_f = eng.pass1(A, B, ws, ov, precision="f64")
    d = max(float((ue - uf).abs().max()), float((ve - vf).abs().max()))
    f = [t.cpu().numpy().reshape(-1) for t in (ue, ve, uf, vf)]
    return d, int((ie != i_f).sum()), n_fb, f


def exact_reference(a, b):
    """-> u, v [n] of the reference's pass 1 (B:383-411, B:518) evaluated on the EXACT integer correlation sums of the window
    pairs (a[i], b[i]): S = sum_p a[p] b[p + d] through a float64 transform, rounded to the integers it approximates (|S| < 2^31,
    transform error < 1e-5); value of a cell (S - S_min) n^4 / (sum a sum b) + 1e-7 in float64, as
    tests/test_exact_scheme.py::exact_window forms it."""
    n, W = a.shape[0], a.shape[-1]
    af, bf = a.astype(np.float64), b.astype(np.float64)
    S = np.rint(np.fft.irfft2(np.conj(np.fft.rfft2(af)) * np.fft.rfft2(bf), s=(W, W)))
    S = np.fft.fftshift(S, axes=(1, 2)).reshape(n, -1).astype(np.int64)
    u, v = np.zeros(n), np.zeros(n)
    KD = W * W
    for i in range(n):
        sa, sb = int(a[i].sum(dtype=np.int64)), int(b[i].sum(dtype=np.int64))
        if sa == 0 or sb == 0:
            continue
        s = S[i]
        m = int(np.argmax(s))
        left, right, top, bot = m + 1, m - 1, m + W, m - W
        left = m if left >= KD - 1 else left
        right = m if right <= 0 else right
        top = m if top >= KD - 1 else top
        bot = m if bot <= 0 else bot
        smin = int(s.min())
        scale = float(W) ** 4 / (float(sa) * float(sb))
        val = lambda q: (int(s[q]) - smin) * scale + 1e-7
        with np.errstate(all="ignore"):
            lm, ll, lr, lt, lb = (np.log(val(q)) for q in (m, left, right, top, bot))
            u[i] = np.nan_to_num(m % W + (lr - ll) / (2 * (ll + lr) - 4 * lm) - W // 2)
            v[i] = np.nan_to_num(m // W + (lb - lt) / (2 * (lb + lt) - 4 * lm) - W // 2)
    return u, v


def check_windows(eng, a, b):
    """precision "exact" against "f64" on one window per frame: identical masks, and fields within 1e-11 px -- or, where the
    float64 kernel's own rounding, amplified by the log fit next to a near-minimum cell, moves its result further than that,
    the exact pass within 1e-12 px of the exact-sum reference (exact_reference).  -> (ok, summary)"""
    ws = a.shape[-1]
    d, nm, n_fb, (ue, ve, uf, vf) = exact_vs_f64(eng, dev(a), dev(b), ws, 0)
    far = (np.abs(ue - uf) >= TOL_F64) | (np.abs(ve - vf) >= TOL_F64)
    dr = 0.0
    if far.any():
        ur, vr = exact_reference(a[far], b[far])
        dr = max(float(np.abs(ue[far] - ur).max()), float(np.abs(ve[far] - vr).max()))
    ok = nm == 0 and dr < 1e-12
    return ok, (f"max |exact - f64| {d:.1e} px, {int(far.sum())} beyond 1e-11 px (there max |exact - exact sums| {dr:.1e} px), "
                f"{nm} masks differing, {n_fb} of {len(a)} through float64")


def test_dispatch_matches_the_kind_of_every_size(eng):
    want = {"radix2": ("xcorr_tile_cand_kernel<", "xcorr_big128_cand_kernel"),
            "mixed": ("xcorr_generic_ct_kernel<0, ",),
            "plain": ("xcorr_generic_kernel<0, float> (cand)",)}
    for ws in SIZES:
        plan = eng.Plan(ws, ws, ws, 0, n_pass=1, max_batch=1, precision="exact")
        name = plan.kernel_name(0)
        plan.close()
        assert name.startswith(want[kind_of(ws)]) and "cand" in name, (ws, kind_of(ws), name)


def test_locating_map_inside_the_band_at_every_size(eng):
    """Every size: the locating kernel's map against a float64 map of the mean-normalised windows, worst err / E+ below
    Gamma(ws, kind) / 4 (and above 0: the hook reports the kernel's map, not the float64 one)."""
    rows = []
    for ws in SIZES:
        fam = families(ws)
        a = np.concatenate([x for x, _ in fam.values()])
        b = np.concatenate([y for _, y in fam.values()])
        worst = band_ratio(eng, a, b)
        g = gamma_u(ws, kind_of(ws)) * U32
        rows.append((ws, worst, g))
        print(f"  ws {ws:3d} {kind_of(ws):6s}: worst err / E+ {worst:.2e}  Gamma {g:.2e}  Gamma / worst {g / max(worst, 1e-30):7.1f}")
    bad = [(ws, w, g) for ws, w, g in rows if not 0 < w < g / 4]
    assert not bad, bad


def test_exact_equals_f64_at_every_size(eng):
    """Every size: the structured families (one window per frame) and two particle frames at a random overlap -- the same
    fields to 1e-11 px and identical validity masks."""
    from torchpiv_amd import synth
    rng = np.random.default_rng(2026)
    bad = []
    for ws in SIZES:
        fam = families(ws)
        a = np.concatenate([x for x, _ in fam.values()])
        b = np.concatenate([y for _, y in fam.values()])
        ok, msg = check_windows(eng, a, b)
        ov = int(rng.integers(0, ws))
        H = 3 * ws + int(rng.integers(0, ws))
        A, B = synth.make_batch(2, H, H + 7, device="cuda", noise=2.0, first_index=ws)
        d2, nm2, n_fb2, _ = exact_vs_f64(eng, A, B, ws, ov)
        print(f"  ws {ws:3d}: families {msg}; frames {H}x{H + 7} ov {ov}: {d2:.1e} px, {nm2} masks differing, "
              f"{n_fb2} through float64")
        if not (ok and d2 < TOL_F64 and nm2 == 0):
            bad.append((ws, msg, ov, d2, nm2))
    assert not bad, bad


def test_adversarial_windows_of_other_sizes(eng):
    """tests/golden/g13_adversarial_sizes.npz: the worst windows tools/research/exact_adversarial.py found per family at
    8, 16, 32, 128 (radix-2), 10, 24, 48, 56 (mixed), 22, 72, 96, 126 (plain DFT): inside Gamma / 4, and exact == f64."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "g13_adversarial_sizes.npz"))
    worst = {}
    for i, (ws, name) in enumerate(zip(g["sizes"], g["names"])):
        ws = int(ws)
        P = g[f"w{i}"]
        a, b = np.ascontiguousarray(P[:, 0]), np.ascontiguousarray(P[:, 1])
        r = band_ratio(eng, a, b)
        worst[ws] = max(worst.get(ws, 0.0), r)
        assert r < gamma_u(ws, kind_of(ws)) * U32 / 4, (ws, str(name), r)
        ok, msg = check_windows(eng, a, b)
        assert ok, (ws, str(name), msg)
    assert sorted(worst) == [8, 10, 16, 22, 24, 32, 48, 56, 72, 96, 126, 128]
    for ws, w in sorted(worst.items()):
        print(f"  ws {ws:3d} {kind_of(ws):6s}: worst err / E+ {w:.2e} against Gamma {gamma_u(ws, kind_of(ws)) * U32:.2e}")
