"""Ensemble correlation on the CPU: the float64 model of tests/ensemble_model.py against the oracle (one pair: the oracle's
own pass) and on the sparse scene (what summing maps buys over averaging fields), and the refusals that need no GPU."""
import numpy as np
import pytest

from oracle import piv_oracle as O
import ensemble_model as EM

H = W = 160
GATE = 1e-3          # px: the project's gate for float32 passes (BASELINE.json, north_star); the oracle's shifted passes are float32


@pytest.fixture(scope="module")
def rec():
    return EM.recording(32, H, W)


def test_one_pair_is_the_oracles_first_pass(rec):
    """n = 1, pass 1: the model's map IS the oracle's (float64, same functions), so the fields agree to rounding."""
    A, B = rec
    for ws, ov in ((32, 16), (16, 8), (64, 32)):
        u, v, inv = EM.ensemble_pass1(A[:1], B[:1], ws, ov)
        ou, ov_, _, _, oval = O.pass1(A[0], B[0], ws, ov, validate=True)
        assert (inv == oval).all(), (ws, ov)
        assert np.abs(u - ou).max() < 1e-9 and np.abs(v - ov_).max() < 1e-9, (ws, ov)


@pytest.mark.parametrize("mode", ["CWS", "DWS"])
def test_one_pair_is_the_oracles_shifted_pass(rec, mode):
    """n = 1, 32/16 -> 16/8: the model's shifted pass (float64 maps of the oracle's staged windows) against IterCWS / IterDWS
    (float32 maps, as the reference's): same validity, fields inside the float32 gate; predictor and half shift identical."""
    A, B = rec
    a, b = A[0], B[0]
    u, v, x, y, val = O.pass1(a, b, 32, 16, validate=True)
    it = O.ITER[mode](a.shape, 16, 8)
    ou, ov_, _, _, oval, _, _, u0, v0, u2, v2 = it(a, b, x, y, u.copy(), v.copy(), val.copy(), debug=True)
    m0, n0, m2, n2 = EM.predictor(mode, a.shape, 32, 16, 16, 8, u, v, val)
    for got, want in ((m0, u0), (n0, v0), (m2, u2), (n2, v2)):
        assert np.array_equal(got, want)
    mu, mv, minv = EM.ensemble_iter(mode, A[:1], B[:1], 16, 8, m0, n0, m2, n2)
    # a window may sit within float32 map error of the ratio threshold or of an arg-max tie in the ORACLE's float32 map:
    # such windows are named, not compared (the model is float64; sparse 16 x 16 single-pair maps have many near-ties)
    S, _, _ = EM.summed(mode, A[:1], B[:1], 16, 8, m2, n2)
    M = S - S.min(axis=(1, 2), keepdims=True) + O.EPS
    flat = np.sort(M.reshape(len(M), -1), axis=1)
    tie = ((flat[:, -1] - flat[:, -2]) <= 1e-4 * flat[:, -1]).reshape(minv.shape)
    same = (minv == oval)
    assert same[~tie].mean() > 0.99, same[~tie].mean()
    ok = same & ~tie & ~minv
    assert np.abs(mu - ou)[ok].max() < GATE and np.abs(mv - ov_)[ok].max() < GATE


def test_summing_maps_beats_averaging_fields(rec):
    """The sparse scene at 32/16, 32 pairs: every ensemble vector valid; RMS error against the constructed flow at most
    half that of the mean of the valid single-pair fields (measured here: ratio 0.30)."""
    A, B = rec
    tu, tv = EM.truth(H, W, 32, 16)
    u, v, inv = EM.ensemble_pass1(A, B, 32, 16)
    assert not inv.any()
    ens = EM.rms(u, v, tu, tv)
    su, sv, cnt, bad = np.zeros_like(tu), np.zeros_like(tv), np.zeros_like(tu), 0
    for a, b in zip(A, B):
        pu, pv, _, _, pval = O.pass1(a, b, 32, 16, validate=True)
        su += np.where(pval, 0.0, pu)
        sv += np.where(pval, 0.0, pv)
        cnt += ~pval
        bad += int(pval.sum())
    assert (cnt > 0).all()
    avg = EM.rms(su / cnt, sv / cnt, tu, tv)
    print(f"  32/16, 32 pairs: ensemble RMS {ens:.3f} px (worst {np.hypot(u - tu, v - tv).max():.3f}), mean of valid "
          f"single-pair fields {avg:.3f} px, ratio {ens / avg:.2f}; {bad / (32 * tu.size):.1%} of single-pair vectors invalid")
    assert ens <= 0.5 * avg, (ens, avg)
    assert ens < 0.2, ens


def test_chain_refines(rec):
    """32/16 -> 16/8 with the ensemble field as the shared predictor: every vector valid, RMS below the one-pass 16/8."""
    A, B = rec
    tu, tv = EM.truth(H, W, 16, 8)
    for mode in ("CWS", "DWS"):
        u, v, inv = EM.chain(A, B, 32, 16, 2, mode)[-1]
        one = EM.ensemble_pass1(A, B, 16, 8)
        e2, e1 = EM.rms(u, v, tu, tv, ~inv), EM.rms(one[0], one[1], tu, tv, ~one[2])
        print(f"  {mode}: chain 32/16 -> 16/8 RMS {e2:.3f} px ({inv.mean():.1%} invalid), one pass at 16/8 {e1:.3f} px")
        assert inv.mean() < 0.02 and e2 < e1, (mode, e2, e1)


def test_zero_windows_contribute_the_zero_map():
    """A window whose pixel sum is 0 in either frame adds the zero map: no NaN, and a window that is zero in every pair
    has a constant mean map -- invalid, u = v = 0."""
    A, B = EM.recording(3, 96, 96)
    A, B = A.copy(), B.copy()
    A[:, :32, :32] = 0                     # window (0, 0) of every pair
    B[1, 32:64, 32:64] = 0                 # window (2, 2) of pair 1 only
    S, P, _ = EM.summed(0, A, B, 32, 16)
    assert np.isfinite(S).all()
    assert not S[0].any() and P[0] == 0
    nc = 5
    full, _, _ = EM.summed(0, A[[0, 2]], B[[0, 2]], 32, 16)
    assert np.array_equal(S[2 * nc + 2], full[2 * nc + 2])          # the skipped contribution
    u, v, inv = EM.peaks(S, 3, 5, 5)
    assert inv[0, 0] and u[0, 0] == 0 and v[0, 0] == 0


# ---- refusals that need no GPU --------------------------------------------------------------------------------------
def test_refusals_without_a_gpu():
    from torchpiv_amd import backend, engine
    for ws, n_pass in ((8, 1), (128, 1), (24, 1), (32, 3)):            # 32 -> 16 -> 8: a chain that reaches 8
        sizes = [w for w, _ in engine.pass_sizes(ws, ws // 2, n_pass, 2.0)]
        with pytest.raises(NotImplementedError, match=str([s for s in sizes if s not in (16, 32, 64)][0])):
            engine.ensemble_check(sizes)
        with pytest.raises(NotImplementedError):
            engine.Plan(256, 256, ws, ws // 2, n_pass=n_pass, ensemble=True)
    engine.ensemble_check([64, 32, 16])
    with pytest.raises(ValueError, match="uncertainty"):
        engine.Plan(160, 160, 32, 16, ensemble=True, uncertainty="cs")
    with pytest.raises(ValueError, match="deform"):
        engine.Plan(160, 160, 32, 16, ensemble=True, deform=1)
    with pytest.raises(KeyError):
        engine.ensemble_mode("CWS_Fast")
    assert engine.pass_sizes(64, 32, 3, 2.0) == [(64, 32), (32, 16), (16, 8)]
    for cls in (backend.OfflinePIV, backend.ResidentPIV):
        assert callable(getattr(cls, "ensemble"))
