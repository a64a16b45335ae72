"""tests/handoff_model.py -- the yardstick of tests/test_gpu_handoff.py -- against the oracle's own passes (bit for bit) and
against hand-written known answers that pin every rule of the hand-off and the combine: the tie rule of rint, the side of
the halving the zeroing sits on, the strict comparison, the sign of the fallback, the independence of the two masks."""
import numpy as np
import pytest

from handoff_model import clause, combine, handoff
from oracle import piv_oracle as O

F = np.float64


def _oracle_case(mode):
    from torchpiv_amd import synth
    H, W, ws, ov = 128, 160, 32, 16
    # (sparse and noisy, so that the pass itself finds invalid vectors and cells the clause masks, in both modes)
    a, b = synth.make_pair(H, W, 78, kind="vortex", noise=10.0, density=0.01)
    an, bn = a.numpy(), b.numpy()
    u, v, x, y, val = O.pass1(an, bn, ws, ov, validate=True)
    val[2, 3] = True                      # make sure the invalid branch is exercised
    cls = O.IterCWSFast if mode == "CWS_Fast" else O.ITER[mode]
    it = cls(an.shape, ws // 2, ov // 2)
    out = it(an, bn, x, y, u.copy(), v.copy(), val.copy(), debug=True)
    u_raw, v_raw = it._predict(x, y, u.copy(), v.copy(), val.copy())
    mask = O.spline_predict(y, x, val, it.slice_y, it.slice_x) >= .5
    return out, u_raw, v_raw, mask


@pytest.mark.parametrize("mode", ["DWS", "CWS", "CWS_Fast"])
def test_model_reproduces_the_oracles_pass(mode):
    out, u_raw, v_raw, mask = _oracle_case(mode)
    ru, rv, _, _, rval, rdu, rdv, ru0, rv0 = out[:9]
    ru2, rv2 = (None, None) if mode == "CWS_Fast" else out[9:11]
    assert mask.any() and not mask.all() and rval.any()
    u0, v0, u2, v2 = handoff(mode, u_raw, v_raw, mask)
    assert np.array_equal(u0, ru0) and np.array_equal(v0, rv0)
    if mode == "CWS_Fast":
        assert u2 is None and v2 is None
    else:
        assert np.array_equal(u2, ru2) and np.array_equal(v2, rv2)
    mu, mv = clause(rdu, ru0), clause(rdv, rv0)
    print(f"  {mode}: {int(mask.sum())} masked predictor cells, {int(rval.sum())} invalid, clause u {int(mu.sum())} v {int(mv.sum())}")
    assert mu.any() and mv.any() and (mu != mv).any()
    u, v = combine(mode, rdu, rdv, rval, ru0, rv0, ru2, rv2)
    assert np.array_equal(u, ru) and np.array_equal(v, rv)
    assert not np.isnan(u).any() and not np.isnan(v).any()


def test_rint_ties_go_to_even():
    raw = np.array([1, -1, 3, -3, 5, -5], dtype=F)
    z = np.zeros(6, np.uint8)
    u0, v0, u2, v2 = handoff("DWS", raw, raw[::-1].copy(), z)
    want = np.array([0, -0.0, 2, -2, 2, -2], dtype=F)
    assert np.array_equal(u2, want) and np.array_equal(np.signbit(u2), np.signbit(want))
    assert np.array_equal(v2, want[::-1])
    assert np.array_equal(u0, raw)
    # the largest double below 0.5 does not round up, 1e-17 and -1e-17 give zeros of their sign
    t = handoff("DWS", np.array([2 * 0.49999999999999994, 1e-17, -1e-17]), np.zeros(3), np.zeros(3, np.uint8))[2]
    assert np.array_equal(t, [0.0, 0.0, -0.0]) and np.array_equal(np.signbit(t), [False, False, True])


def test_clause_needs_a_fallback_that_rounds_above_zero():
    for du in (-3.0, 0.0, 0.6, 7.0, np.inf):            # rint(0.5) = 0: never masked, whatever du
        assert not clause(F(du), F(0.5))
        u, _ = combine("CWS", F(du), F(0), None, F(0.5), F(0), F(0.25), F(0))
        assert u == F(0.5) + F(du)
    assert clause(F(7.0), F(0.5000000000000001))         # rint = 1
    for u0 in (-0.0, -0.5, -1.5, -3.0, -64.0):           # negative fallback: never masked
        assert not clause(F(100.0), F(u0))
    assert not clause(F(1.0), F(0.0))


def test_the_comparison_is_strict():
    u0 = F(1.5)
    assert not clause(F(1.5), u0)
    assert clause(np.nextafter(F(1.5), F(2)), u0)
    assert not clause(np.nextafter(F(1.5), F(1)), u0)
    for mode, u2 in (("CWS", F(0.75)), ("DWS", F(1.0)), ("CWS_Fast", None)):
        base = u0 if mode == "CWS_Fast" else 2 * u2
        u, v = combine(mode, F(1.5), F(0), None, u0, F(0), u2, F(0))
        assert u == base + F(1.5) and v == 0
        up = np.nextafter(F(1.5), F(2))
        u, v = combine(mode, up, F(0), None, u0, F(0), u2, F(0))
        assert u == u0 and v == 0


def test_invalid_sends_both_components_to_the_fallback():
    du, dv = np.array([0.25, 0.25]), np.array([-0.5, -0.5])
    u0, v0 = np.array([3.0, 3.0]), np.array([-2.0, -2.0])
    u, v = combine("CWS", du, dv, np.array([0, 1], np.uint8), u0, v0, u0 / 2, v0 / 2)
    assert np.array_equal(u, [3.25, 3.0]) and np.array_equal(v, [-2.5, -2.0])
    u, v = combine("CWS_Fast", du, dv, np.array([True, False]), u0, v0, None, None)
    assert np.array_equal(u, [3.0, 3.25]) and np.array_equal(v, [-2.0, -2.5])


def test_the_mask_byte_cws_keeps_the_half_shift_dws_does_not():
    raw_u, raw_v = np.array([3.0, 3.0]), np.array([-5.0, -5.0])
    m = np.array([0, 1], np.uint8)
    u0, v0, u2, v2 = handoff("CWS", raw_u, raw_v, m)
    assert np.array_equal(u2, [1.5, 1.5]) and np.array_equal(v2, [-2.5, -2.5])          # halves before the zeroing
    assert np.array_equal(u0, [3.0, 0.0]) and np.array_equal(v0, [-5.0, 0.0])
    du, dv = np.array([0.25, 0.25]), np.array([0.125, 0.125])
    u, v = combine("CWS", du, dv, None, u0, v0, u2, v2)
    # the masked cell keeps its half shift in the result (2 * 1.5 + du): its zero fallback never triggers the clause
    assert np.array_equal(u, [3.25, 3.25]) and np.array_equal(v, [-4.875, -4.875])
    u0, v0, u2, v2 = handoff("DWS", raw_u, raw_v, m)
    assert np.array_equal(u2, [2.0, 0.0]) and np.array_equal(v2, [-2.0, 0.0])           # rint of the halves after it
    u, v = combine("DWS", du, dv, None, u0, v0, u2, v2)
    assert np.array_equal(u, [4.25, 0.25]) and np.array_equal(v, [-3.875, 0.125])
    u0, v0, u2, v2 = handoff("CWS_Fast", raw_u, raw_v, m)
    assert u2 is None and v2 is None and np.array_equal(u0, [3.0, 0.0]) and np.array_equal(v0, [-5.0, 0.0])


def test_the_two_masks_are_independent():
    # u: du > u0 and rint(u0) > 0 -> fallback; v: dv <= v0 -> kept (and the other way round in the second cell)
    du, dv = np.array([2.0, 0.5]), np.array([0.5, 2.0])
    u0, v0 = np.array([1.25, 1.25]), np.array([1.25, 1.25])
    u2, v2 = u0 / 2, v0 / 2
    u, v = combine("CWS", du, dv, np.zeros(2, np.uint8), u0, v0, u2, v2)
    assert np.array_equal(u, [1.25, 1.75]) and np.array_equal(v, [1.75, 1.25])
    assert np.array_equal(clause(du, u0), [True, False]) and np.array_equal(clause(dv, v0), [False, True])


def test_inputs_are_left_alone_and_modes_are_checked():
    raw = np.array([1.0, 2.0])
    keep = raw.copy()
    handoff("CWS", raw, raw, np.array([1, 0], np.uint8))
    handoff("DWS", raw, raw, np.array([1, 0], np.uint8))
    assert np.array_equal(raw, keep)
    with pytest.raises(KeyError):
        handoff("cws", raw, raw, np.zeros(2))
    with pytest.raises(KeyError):
        combine("PASS1", raw, raw, None, raw, raw, raw, raw)


@pytest.mark.parametrize("mode", ["DWS", "CWS"])
def test_planted_cases_populate_every_class_on_the_reference(mode):
    """The inputs of tests/test_gpu_handoff.py with the oracle's own staging, correlation and peak analysis: the reference
    alone puts cells into every class the GPU cases must exercise, at every window size; the planted table holds every
    entry under both mask values; no planted magnitude lies below float32's normal range."""
    import handoff_cases as HC
    mag = np.abs(HC.TABLE)
    assert ((mag == 0) | ((mag >= 1e-30) & (mag <= 64))).all()
    for ws in HC.SIZES:
        assert HC.table_coverage(ws)
        u_raw, v_raw, mask = HC.planted(ws)
        assert 0.2 <= mask.mean() <= 0.3
        du, dv, inv = HC.oracle_raw(mode, ws)
        cov = HC.coverage(mode, du, dv, inv, u_raw, v_raw, mask)
        print(f"  {mode} {ws}: {cov}")
        assert all(n >= 1 for n in cov.values()), (mode, ws, cov)
        # the model reproduces the oracle's combine on these inputs too (IterPass._finish, operation by operation)
        u0, v0, u2, v2 = handoff(mode, u_raw, v_raw, mask)
        u, v = combine(mode, du, dv, inv, u0, v0, u2, v2)
        ru, rv = 2 * u2 + du, 2 * v2 + dv
        mu, mv = (du > u0) * (np.rint(u0) > 0), (dv > v0) * (np.rint(v0) > 0)
        mu[inv], mv[inv] = True, True
        ru[mu], rv[mv] = u0[mu], v0[mv]
        assert np.array_equal(u, ru) and np.array_equal(v, rv)
