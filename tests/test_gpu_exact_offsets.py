"""The exact first pass on the device, on the inputs of profiles/exact_offsets/: (1) the two 2 x 2 blocks of windows whose
recorded "offsets" were one-pixel changes of the frames (tests/golden/g14_exact_first_pass_offsets.npz), stored and with that
pixel one grey level higher, at "exact" and "f64" against the oracle on the same pixels; (2) the same bits from three runs of
one plan whose undecided list -- filled through an atomic counter in whatever order the wavefronts arrive -- holds 84 windows
that are undecidable by construction, and the oracle's fields on the ordinary windows beside them; (3) synth's renderer gives
the same float32 image, and make_batch the same frames, in every call.  The CPU side of (1) and the construction of (2):
tests/test_exact_offsets_host.py.
"""
import numpy as np
import pytest
import torch

import exact_offsets_cases as X
from oracle import piv_oracle as O

pytestmark = pytest.mark.gpu

TOL_F64 = 1e-11          # px, tests/test_gpu_exact.py's gate of the exact sums against a float64 transform


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(fields):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().copy() for t in fields)


def same_bytes(x, y):
    return all(p.dtype == q.dtype and p.shape == q.shape and p.tobytes() == q.tobytes() for p, q in zip(x, y))


def oracle(A, B, ws):
    out = [O.pass1(a, b, ws, ws // 2, validate=True) for a, b in zip(A, B)]
    return np.stack([r[0] for r in out]), np.stack([r[1] for r in out]), np.stack([r[4] for r in out]).astype(bool)


def test_g14_windows_stored_and_incremented(eng):
    g = X.load_g14()
    A, B = X.g14_mosaics(g)                            # block 0 stored, incremented, block 1 stored, incremented
    u0, v0, m0 = oracle(A, B, X.WS)
    assert u0.shape == (4, 2, 2)
    got = {}
    for precision in ("exact", "f64"):
        runs = [host(eng.pass1(dev(A), dev(B), X.WS, X.OV, precision=precision)) for _ in range(3)]
        assert same_bytes(runs[0], runs[1]) and same_bytes(runs[0], runs[2]), precision
        u, v, inv = got[precision] = runs[0]
        d = max(np.abs(u - u0).max(), np.abs(v - v0).max())
        print(f"  g14 mosaics, {precision}: 16 vectors against the oracle on the same pixels {d:.1e} px")
        assert d < TOL_F64, (precision, d)
        assert np.array_equal(inv.astype(bool), m0), precision
    ue, ve, ie = got["exact"]
    uf, vf, i_f = got["f64"]
    d = max(np.abs(ue - uf).max(), np.abs(ve - vf).max())
    print(f"  g14 mosaics, exact against f64: {d:.1e} px")
    assert d < TOL_F64 and np.array_equal(ie, i_f)
    # the recorded fields, and the "offset" itself: one grey level of one pixel moves every vector of its block
    for block, (k0, _, _, _, _, tag) in enumerate(X.INCREMENTS):
        ks = slice(k0, k0 + 4)
        for j, t in enumerate(("f64", tag)):
            assert np.abs(ue[2 * block + j].reshape(-1) - g["u_" + t][ks]).max() < TOL_F64
            assert np.abs(ve[2 * block + j].reshape(-1) - g["v_" + t][ks]).max() < TOL_F64
        off = np.maximum(np.abs(ue[2 * block + 1] - ue[2 * block]), np.abs(ve[2 * block + 1] - ve[2 * block]))
        print(f"  block {block}: stored against incremented {off.min():.1e} .. {off.max():.1e} px")
        assert (off > 0).all() and off.max() < 5e-5


@pytest.mark.parametrize("size,ws", [(256, 64), (128, 32)])
def test_three_runs_give_the_same_bits_with_a_filled_undecided_list(eng, size, ws):
    from test_gpu_parity import near_tie_windows, pass1_constant
    A, B, tied = X.tied_frames(size, ws, 600)
    n_tied, n_other = 4 * int(tied.sum()), 4 * int((~tied).sum())
    assert (n_tied, n_other) == (84, 112)
    excused = np.stack([pass1_constant(a, b, ws, ws // 2) | near_tie_windows(a, b, ws, ws // 2, rel=64 * 2.0 ** -52) for a, b in zip(A, B)])
    assert np.array_equal(excused, np.broadcast_to(tied, excused.shape))      # no ordinary window is excused: a condition
    u0, v0, m0 = oracle(A, B, ws)
    Ad, Bd = dev(A), dev(B)
    plan = eng.Plan(size, size, ws, ws // 2, n_pass=1, precision="exact", max_batch=4)
    runs, fallbacks = [], []
    for _ in range(3):
        runs.append(host(plan.run(Ad, Bd)))
        fallbacks.append(plan.exact_fallbacks())
    plan.close()
    print(f"  {size}^2 at {ws}/{ws // 2}: undecided windows {fallbacks} of {n_tied + n_other} ({n_tied} tied by construction)")
    assert min(fallbacks) >= n_tied and len(set(fallbacks)) == 1, fallbacks
    assert same_bytes(runs[0], runs[1]) and same_bytes(runs[0], runs[2])
    u, v, inv = runs[0]
    assert u.shape == u0.shape
    other = np.broadcast_to(~tied, u.shape)
    d = max(np.abs(u - u0)[other].max(), np.abs(v - v0)[other].max())
    print(f"  ordinary windows against the oracle: {d:.1e} px, {int((inv.astype(bool) != m0)[other].sum())} flags differing")
    assert d < TOL_F64 and np.array_equal(inv.astype(bool)[other], m0[other])
    # the tied windows: a tie's winner belongs to the last-bit rounding of each kernel instance -- printed, not asserted
    pf = eng.Plan(size, size, ws, ws // 2, n_pass=1, precision="f64", max_batch=4)
    uf, vf, i_f = host(pf.run(Ad, Bd))
    pf.close()
    t = np.broadcast_to(tied, u.shape)
    df = np.maximum(np.abs(u - uf), np.abs(v - vf))
    print(f"  tied windows, exact against f64: {int((df[t] > TOL_F64).sum())} of {n_tied} beyond {TOL_F64} px (max {df[t].max():.3g} px), "
          f"{int((inv != i_f)[t].sum())} flags differing; ordinary windows: max {df[other].max():.1e} px")
    assert df[other].max() < TOL_F64 and np.array_equal(inv[other], i_f[other])


def test_render_gives_the_same_float32_image_twice():
    """The float32 image BEFORE it is rounded to grey levels: wherever two particles share a pixel, a changed order of the
    sum moves its last bits, so this sees every change of order -- the uint8 frames see one only where a sum lies near .5
    (the unguarded renderer: profiles/exact_offsets/README.md)."""
    from torchpiv_amd import synth
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    H = W = 1024
    g = torch.Generator(device="cpu").manual_seed(synth.BASE_SEED)
    n = int(0.03 * (H + 20) * (W + 20))
    px = (torch.rand(n, generator=g, dtype=torch.float64) * (W + 20) - 10).float().cuda()
    py = (torch.rand(n, generator=g, dtype=torch.float64) * (H + 20) - 10).float().cuda()
    amp = ((0.5 + 0.5 * torch.rand(n, generator=g, dtype=torch.float64)).float() * 200.0).cuda()
    before = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    i0 = synth._render(px, py, amp, H, W, 1.0, "cuda")
    i1 = synth._render(px, py, amp, H, W, 1.0, "cuda")
    assert (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()) == before
    assert i0.dtype == torch.float32 and i0.shape == (H, W) and float(i0.max()) > 100.0
    n_diff = int((i0.view(torch.int32) != i1.view(torch.int32)).sum())
    print(f"  float32 pixels differing between two renders: {n_diff} of {H * W}")
    assert n_diff == 0


def test_make_batch_gives_the_same_frames_twice():
    from torchpiv_amd import synth
    A0, B0 = synth.make_batch(2, 1024, 1024, noise=2.0, device="cuda")
    A1, B1 = synth.make_batch(2, 1024, 1024, noise=2.0, device="cuda")
    assert A0.dtype == torch.uint8 and A0.is_cuda and int(A0.max()) > 100
    assert torch.equal(A0, A1) and torch.equal(B0, B1)
