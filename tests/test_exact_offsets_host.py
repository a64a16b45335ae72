"""The "offsets" of the exact first pass recorded in profiles/twiddle_first/bits.txt are one-pixel changes of the frames
(profiles/exact_offsets/): tests/golden/g14_exact_first_pass_offsets.npz against the oracle and the numpy model of the scheme,
and the guard in synth._render that makes a render the same in every run.  tests/test_gpu_exact_offsets.py runs the same
inputs on the device.
"""
import numpy as np
import pytest
import torch

import exact_offsets_cases as X
from oracle import piv_oracle as O
from test_exact_scheme import exact_window

TOL_F64 = 1e-11          # px, tests/test_gpu_exact.py's gate of the exact sums against a float64 transform (measured here: 1.1e-14)


@pytest.fixture(scope="module")
def g14():
    return X.load_g14()


def oracle_windows(a, b):
    """The oracle's first pass on every 64 x 64 window alone -> u, v, invalid [n]."""
    out = [O.pass1(x, y, X.WS, X.OV, validate=True) for x, y in zip(a, b)]
    assert all(r[0].shape == (1, 1) for r in out)
    return (np.array([r[0][0, 0] for r in out]), np.array([r[1][0, 0] for r in out]), np.array([bool(r[4][0, 0]) for r in out]))


def test_g14_stored_pixels_give_the_float64_record(g14):
    u, v, inv = oracle_windows(g14["a"], g14["b"])
    d = max(np.abs(u - g14["u_f64"]).max(), np.abs(v - g14["v_f64"]).max())
    print(f"  stored pixels against u_f64 / v_f64: {d:.1e} px")
    assert d < TOL_F64 and not inv.any()
    # the records that were NOT off equal the float64 record: the parent's in block 0, this build's in block 1
    for tag, ks in (("parent", slice(0, 4)), ("this", slice(4, 8))):
        assert np.abs(g14["u_" + tag][ks] - g14["u_f64"][ks]).max() < TOL_F64 and np.abs(g14["v_" + tag][ks] - g14["v_f64"][ks]).max() < TOL_F64


@pytest.mark.parametrize("block", [0, 1])
def test_g14_one_pixel_one_grey_level_gives_the_off_record(g14, block):
    k0, frame, row, col, value, tag = X.INCREMENTS[block]
    a, b, where = X.incremented_windows(g14, block)
    # one frame pixel lies in exactly four windows at 50 % overlap, at positions that differ by the window step
    (y0, x0) = where[0]
    assert where == [(y0, x0), (y0, x0 - X.STEP), (y0 - X.STEP, x0), (y0 - X.STEP, x0 - X.STEP)]
    pairs = {int(g14["pair_row_col"][k0 + k][0]) for k in range(4)}
    r0, c0 = (int(x) for x in g14["pair_row_col"][k0][1:])
    assert len(pairs) == 1 and [tuple(int(x) for x in g14["pair_row_col"][k0 + k][1:]) for k in range(4)] == \
        [(r0, c0), (r0, c0 + 1), (r0 + 1, c0), (r0 + 1, c0 + 1)]
    assert (X.STEP * r0 + y0, X.STEP * c0 + x0) == (row, col)
    for r, c in ((r0 - 1, c0), (r0, c0 - 1), (r0 + 2, c0), (r0, c0 + 2)):      # ... and in no window around the block
        assert not (X.STEP * r <= row < X.STEP * r + X.WS and X.STEP * c <= col < X.STEP * c + X.WS)
    changed = (a != g14["a"][k0:k0 + 4]).sum(axis=(1, 2)) + (b != g14["b"][k0:k0 + 4]).sum(axis=(1, 2))
    assert changed.tolist() == [1, 1, 1, 1]
    u, v, inv = oracle_windows(a, b)
    ks = slice(k0, k0 + 4)
    d = max(np.abs(u - g14["u_" + tag][ks]).max(), np.abs(v - g14["v_" + tag][ks]).max())
    off = np.maximum(np.abs(u - g14["u_f64"][ks]), np.abs(v - g14["v_f64"][ks]))
    print(f"  block {block}: frame {frame} ({row}, {col}) {value} -> {value + 1}: against the {tag} record {d:.1e} px; "
          f"against the stored pixels {off.min():.1e} .. {off.max():.1e} px")
    assert d < TOL_F64 and not inv.any()
    assert 5e-7 < off.min() and off.max() < 5e-5         # the recorded offsets: 7e-7 ... 3.4e-5 px


def test_g14_mosaics_through_the_first_pass(g14):
    """The four windows of a block reassembled into the 96 x 96 piece of their frame (the overlaps agree, stored and
    incremented) give the same four vectors through pass 1 at 64/32 as each window alone."""
    A, B = X.g14_mosaics(g14)
    assert A.shape == B.shape == (4, 96, 96)
    for block, (k0, _, _, _, _, tag) in enumerate(X.INCREMENTS):
        ks = slice(k0, k0 + 4)
        for j, (ur, vr) in enumerate(((g14["u_f64"][ks], g14["v_f64"][ks]), (g14["u_" + tag][ks], g14["v_" + tag][ks]))):
            u, v, _, _, inv = O.pass1(A[2 * block + j], B[2 * block + j], X.WS, X.OV, validate=True)
            assert u.shape == (2, 2)
            assert np.abs(u.reshape(-1) - ur).max() < TOL_F64 and np.abs(v.reshape(-1) - vr).max() < TOL_F64
            assert not inv.any()
        assert (A[2 * block] != A[2 * block + 1]).sum() + (B[2 * block] != B[2 * block + 1]).sum() == 1


def test_g14_model_of_the_scheme_decides_every_window(g14):
    """None of the sixteen windows goes near the float64 fallback: the numpy statement of the exact scheme decides them all
    and agrees with the oracle on the same pixels."""
    sets = [(g14["a"], g14["b"])]
    for block in (0, 1):
        sets.append(X.incremented_windows(g14, block)[:2])
    worst = 0.0
    for a, b in sets:
        u, v, inv = oracle_windows(a, b)
        for k, (x, y) in enumerate(zip(a, b)):
            r = exact_window(x, y)
            assert r is not None, k
            worst = max(worst, abs(r[0] - u[k]), abs(r[1] - v[k]))
            assert r[2] == inv[k]
    print(f"  model against the oracle, 16 windows: {worst:.1e} px")
    assert worst < 1e-13


@pytest.mark.parametrize("size,ws", [(256, 64), (128, 32)])
def test_tied_frames_are_undecidable_where_they_repeat_and_ordinary_elsewhere(size, ws):
    """What tests/test_gpu_exact_offsets.py's run-to-run test stands on: in the periodic part every window has S(d) =
    S(d + ws/2) exactly -- the float64 gates' excuse set holds exactly those windows, and the model of the scheme decides
    none of them and every other one (the model on the first pair, the excuse set on all four)."""
    from test_gpu_parity import near_tie_windows, pass1_constant
    A, B, tied = X.tied_frames(size, ws, 600)
    assert tied.shape == (7, 7) and tied.sum() == 21 and tied[:, :3].all()
    for k in range(4):
        excused = pass1_constant(A[k], B[k], ws, ws // 2) | near_tie_windows(A[k], B[k], ws, ws // 2, rel=64 * 2.0 ** -52)
        assert np.array_equal(excused, tied), k
    aw, bw = O.windows(A[0], ws, ws // 2), O.windows(B[0], ws, ws // 2)
    for i, (a, b) in enumerate(zip(aw, bw)):
        q = (ws // 2 + 2) * ws + 3                       # any cell of the map's left half: the sum at d equals the sum at d + period
        if tied.reshape(-1)[i]:
            from test_exact_scheme import exact_sum
            assert exact_sum(a, b, q) == exact_sum(a, b, q + ws // 2)
        assert (exact_window(a, b) is None) == bool(tied.reshape(-1)[i]), i


class _Seen(Exception):
    pass


@pytest.mark.parametrize("raises", [False, True])
@pytest.mark.parametrize("det,warn_only", [(False, False), (True, False), (True, True)])
def test_render_sums_under_deterministic_algorithms_and_restores_the_flags(monkeypatch, det, warn_only, raises):
    from torchpiv_amd import synth
    seen = []
    real = torch.Tensor.index_add_

    def index_add_(self, *args, **kw):
        seen.append((torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()))
        if raises and len(seen) == 3:
            raise _Seen()
        return real(self, *args, **kw)

    monkeypatch.setattr(torch.Tensor, "index_add_", index_add_)
    before = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    torch.use_deterministic_algorithms(det, warn_only=warn_only)
    try:
        if raises:
            with pytest.raises(_Seen):
                synth.make_pair(64, 64, 3, noise=1.0)
        else:
            a, b = synth.make_pair(64, 64, 3, noise=1.0)
            assert len(seen) == 2 * 49 and a.dtype == torch.uint8 and a.shape == (64, 64)
        assert seen and all(s == (True, False) for s in seen)          # on, and as an error, not as a warning
        assert (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()) == (det, warn_only)
    finally:
        torch.use_deterministic_algorithms(before[0], warn_only=before[1])


def test_render_is_what_it_was_on_the_cpu():
    """Two calls give the same pair, and an outer switch changes nothing: the CPU sums in one order either way."""
    from torchpiv_amd import synth
    a0, b0 = synth.make_pair(96, 128, 7, noise=2.0)
    a1, b1 = synth.make_pair(96, 128, 7, noise=2.0)
    assert torch.equal(a0, a1) and torch.equal(b0, b1)
    torch_det = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        a2, b2 = synth.make_pair(96, 128, 7, noise=2.0)
    finally:
        torch.use_deterministic_algorithms(torch_det)
    assert torch.equal(a0, a2) and torch.equal(b0, b2)
