"""The predictor hand-off and the combine of every shifted-pass kernel, bit for bit.

Every pass after the first ends in the same decisions: the predictor becomes a window shift (DWS rint(u0 / 2) after the
invalid-zeroing, CWS u0 / 2 before it) and finalize_kernel combines u = 2 u2 + du, replaced by the fallback u0 where
(du > u0) && rint(u0) > 0 or where the peak ratio fails -- per component.  The library has two forms of the hand-off: the
four fields u0, v0, u2, v2 of tpiv_iter, and the compact form of tpiv_plan_run (raw predictor + mask byte; the zeroing, the
halving and the rint formed where pred_half_shift / pred_half_shift_cws_f32 / pred_fallback read them, one item ahead of
the work).  Here the compact form gets CHOSEN inputs (tests/handoff_cases.py: every rint tie, both zeros, values on either
side of every comparison, each under both mask values) through tpiv_debug_iter_compact, and

  (a) both forms give the same u, v, invalid, du, dv, bit for bit (same kernels, same numbers);
  (b) the float64 model of tests/handoff_model.py, fed with the GPU's own du, dv, invalid, gives the GPU's u, v bit for bit;
  (c) CWS_Fast, which has the four-field form only: (b);
  (d) every case counts the cells of each class of the combine it exercised, and none may be empty;
  (e) the strict comparison: a four-field call with u0 = du planted (du does not depend on u0 there), so that du == u0 holds
      exactly in every valid cell;

and on natural fields every pass p >= 1 of a whole plan equals the seam fed with the plan's own predictor -- the only check
without a tolerance that the mask_out branch of predict_cols_mfma_kernel meets.  No tolerance and no excuse set anywhere:
the one class in which the two forms may differ by design (|u| below float32's normal range, where float(u / 2) and
float(u) * 0.5f round differently) is not planted (magnitudes are 0 or in [1e-30, 64]).

profiles/handoff/README.md: the coverage counts per case, and which assertion catches which one-line mutant of the readers."""
import numpy as np
import pytest
import torch

import handoff_cases as HC
from handoff_model import clause, combine, handoff

pytestmark = pytest.mark.gpu

MODE_ID = {"DWS": 1, "CWS": 2}
ORDERS = ("reference", "exact")          # the reference's operation order / the fast one: different template instances
CASES = [(ws, mode, order) for ws in HC.SIZES for mode in ("DWS", "CWS") for order in ORDERS]


def expected_kernel(ws, mode, order):
    m, tf = MODE_ID[mode], "false" if order == "reference" else "true"
    if ws == 8:
        return f"xcorr_w8_kernel<{m}, {tf}>"                         # one window per lane
    if ws in (16, 32, 64):                                           # tile kernels; 64 CWS at the fast order: two launches
        occ = 4 if ws == 16 else (3 if (ws == 32 or mode != "CWS") else 2)
        return f"xcorr_tile_kernel<{ws}, {m}, {occ}, {tf}>"
    if ws == 28:
        return f"xcorr_generic_ct_kernel<{m}, 28>"                   # compile-time generic
    if ws == 10:
        return f"xcorr_generic_ct_kernel<{m}, 0>"                    # run-time Cooley-Tukey form
    return f"xcorr_generic_kernel<{m}, float>"                       # 22, 15 (odd: the ws x (ws - 1) map), shifted 128


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def test_every_case_runs_the_kernel_it_names(eng):
    """The families of the case table, by the library's own dispatch (a throwaway two-pass plan whose second pass has the
    case's window size)."""
    assert sorted({expected_kernel(*c) for c in CASES}) == sorted(
        [f"xcorr_w8_kernel<{m}, {tf}>" for m in (1, 2) for tf in ("true", "false")]
        + [f"xcorr_tile_kernel<{ws}, {m}, {4 if ws == 16 else (3 if ws == 32 or m == 1 else 2)}, {tf}>"
           for ws in (16, 32, 64) for m in (1, 2) for tf in ("true", "false")]
        + [f"xcorr_generic_ct_kernel<{m}, {n}>" for m in (1, 2) for n in (28, 0)]
        + [f"xcorr_generic_kernel<{m}, float>" for m in (1, 2)])
    for ws, mode, order in CASES:
        plan = eng.Plan(6 * ws, 6 * ws, 2 * ws, 2 * (ws // 2), n_pass=2, mode=mode, max_batch=1, precision=order)
        assert plan.geometry[1][:2] == (ws, ws // 2), (ws, plan.geometry)
        assert plan.kernel_name(1) == expected_kernel(ws, mode, order), (ws, mode, order, plan.kernel_name(1))
        plan.close()


def report(tag, names, got, want, u_raw, v_raw, mask):
    """The first differing cells of a failed comparison: index, planted values, mask byte, both results."""
    lines = []
    for name, g, w in zip(names, got, want):
        g, w = host(g) if isinstance(g, torch.Tensor) else g, host(w) if isinstance(w, torch.Tensor) else w
        bad = np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w)))) if g.dtype.kind == "f" else np.argwhere(g != w)
        for i in bad[:8]:
            i = tuple(i)
            lines.append(f"{tag} {name}{list(i)}: planted u {u_raw[i]!r} v {v_raw[i]!r} mask {mask[i]}: {g[i]!r} != {w[i]!r}")
        if len(bad):
            lines.append(f"{tag} {name}: {len(bad)} cells differ")
    return "\n".join(lines)


def check_combine(tag, mode, out, fields, u_raw, v_raw, mask):
    """(b): the model on the GPU's own du, dv, invalid against the GPU's u, v."""
    u, v, inv, du, dv = (host(t) for t in out)
    mu, mv = combine(mode, du, dv, inv, *fields)
    ok = np.array_equal(mu, u) and np.array_equal(mv, v)
    assert ok, "\n" + report(tag + " combine", ("u", "v"), (u, v), (mu, mv), u_raw, v_raw, mask)
    assert set(np.unique(inv)) <= {0, 1}


def assert_classes(tag, cov):
    print(f"  {tag}: " + ", ".join(f"{k} {n}" for k, n in cov.items()))
    for k, n in cov.items():
        assert n >= 1, (tag, "class not exercised", k, cov)


@pytest.mark.parametrize("ws,mode,order", CASES, ids=[f"{c[1]}-{c[0]}-{c[2]}" for c in CASES])
def test_compact_and_four_field_hand_off(eng, ws, mode, order):
    H, W, ov, nr, nc = HC.geometry(ws)
    A, B = (dev(t) for t in HC.frames(ws))
    u_raw, v_raw, mask = HC.planted(ws)
    assert HC.table_coverage(ws)
    fields = handoff(mode, u_raw, v_raw, mask)
    tag = f"{mode} {ws} {order}"
    compact = eng.iterate_compact(mode, A, B, ws, ov, dev(u_raw), dev(v_raw), dev(mask), want_raw=True, precision=order)
    four = eng.iterate(mode, A, B, ws, ov, *(dev(f) for f in fields), want_raw=True, precision=order)
    names = ("u", "v", "invalid", "du", "dv")
    same = all(torch.equal(c, f) for c, f in zip(compact, four))                  # (a)
    assert same, "\n" + report(tag + " compact != four-field", names, compact, four, u_raw, v_raw, mask)
    check_combine(tag + " compact", mode, compact, fields, u_raw, v_raw, mask)    # (b), either form
    check_combine(tag + " four-field", mode, four, fields, u_raw, v_raw, mask)
    _, _, inv, du, dv = (host(t) for t in compact)                                # (d)
    assert_classes(tag, HC.coverage(mode, du, dv, inv, u_raw, v_raw, mask))


@pytest.mark.parametrize("ws", HC.FAST_SIZES)
def test_cws_fast_combine(eng, ws):
    """(c): CWS_Fast takes u0, v0 alone (u = u0 + du); the planted table after the zeroing."""
    H, W, ov, nr, nc = HC.geometry(ws)
    A, B = (dev(t) for t in HC.frames(ws))
    u_raw, v_raw, mask = HC.planted(ws)
    fields = handoff("CWS_Fast", u_raw, v_raw, mask)
    out = eng.iterate("CWS_Fast", A, B, ws, ov, dev(fields[0]), dev(fields[1]), None, None, want_raw=True)
    check_combine(f"CWS_Fast {ws}", "CWS_Fast", out, fields, u_raw, v_raw, mask)
    _, _, inv, du, dv = (host(t) for t in out)
    assert_classes(f"CWS_Fast {ws}", HC.coverage("CWS_Fast", du, dv, inv, u_raw, v_raw, mask))


@pytest.mark.parametrize("mode", ["DWS", "CWS"])
def test_equality_keeps_the_pass_result(eng, mode):
    """(e): du > u0 is strict.  Real correlation never lands on du == u0, so equality is planted: in the four-field form
    the shift comes from u2, v2 alone, hence du, dv do not depend on u0, v0 -- a second call with u0 = du, v0 = dv returns
    the same du, dv bit for bit, and every valid cell sits exactly on the comparison.  There the pass's own value 2 u2 + du
    must survive (a `>=` would put the fallback du in its place wherever u2 != 0 and rint(du) > 0)."""
    ws = 32
    H, W, ov, nr, nc = HC.geometry(ws)
    A, B = (dev(t) for t in HC.frames(ws))
    u_raw, v_raw, mask = HC.planted(ws)
    u0, v0, u2, v2 = handoff(mode, u_raw, v_raw, mask)
    first = eng.iterate(mode, A, B, ws, ov, dev(u0), dev(v0), dev(u2), dev(v2), want_raw=True)
    du, dv = host(first[3]), host(first[4])
    again = eng.iterate(mode, A, B, ws, ov, first[3], first[4], dev(u2), dev(v2), want_raw=True)
    assert torch.equal(again[3], first[3]) and torch.equal(again[4], first[4]) and torch.equal(again[2], first[2])
    inv = host(again[2]) != 0
    u, v = host(again[0]), host(again[1])
    mu, mv = combine(mode, du, dv, inv, du, dv, u2, v2)
    assert not clause(du, du).any()
    tell_u = ~inv & (np.rint(du) > 0) & (u2 != 0)          # cells in which a non-strict comparison changes the result
    tell_v = ~inv & (np.rint(dv) > 0) & (v2 != 0)
    print(f"  {mode}: du == u0 in all {du.size} cells; a non-strict comparison would change u in {int(tell_u.sum())}, "
          f"v in {int(tell_v.sum())} of them")
    assert tell_u.sum() >= 1 and tell_v.sum() >= 1
    assert np.array_equal(u, mu) and np.array_equal(v, mv), "\n" + report(f"{mode} equality", ("u", "v"), (u, v), (mu, mv),
                                                                          u_raw, v_raw, mask)
    assert np.array_equal(u[tell_u], (2 * u2 + du)[tell_u]) and np.array_equal(v[tell_v], (2 * v2 + dv)[tell_v])


def test_cws_fast_equality_in_one_step(eng):
    """The same through CWS_Fast, whose du depends on u0 through the resampling: planting u0 = du of a first call moves du,
    so one step does not reach equality (measured: profiles/handoff/README.md); the step is checked by the model all the same
    and the number of cells that did land on du == u0 is printed, not asserted."""
    ws = 32
    H, W, ov, nr, nc = HC.geometry(ws)
    A, B = (dev(t) for t in HC.frames(ws))
    u_raw, v_raw, mask = HC.planted(ws)
    u0, v0, _, _ = handoff("CWS_Fast", u_raw, v_raw, mask)
    first = eng.iterate("CWS_Fast", A, B, ws, ov, dev(u0), dev(v0), None, None, want_raw=True)
    du1, dv1 = host(first[3]), host(first[4])
    again = eng.iterate("CWS_Fast", A, B, ws, ov, first[3], first[4], None, None, want_raw=True)
    check_combine("CWS_Fast 32 second step", "CWS_Fast", again, (du1, dv1, None, None), u_raw, v_raw, mask)
    print(f"  CWS_Fast: cells with du == u0 after one step: u {int((host(again[3]) == du1).sum())}, "
          f"v {int((host(again[4]) == dv1).sum())} of {du1.size}")


# the chains of the plan test: first-pass (ws, ov), passes, frame.  Frames of the size of the multipass goldens; 256 -> 128
# on the smallest frame the plan accepts (the spline predictor needs four coarse windows per axis: 256 + 3 * 128 = 640)
CHAINS = [((64, 32), 4, (264, 328)), ((40, 20), 3, (150, 190)), ((88, 44), 3, (230, 270)), ((256, 128), 2, (640, 640))]


@pytest.mark.parametrize("precision", ["exact", "reference"])
@pytest.mark.parametrize("mode", ["DWS", "CWS"])
@pytest.mark.parametrize("chain", CHAINS, ids=[f"{c[0][0]}x{c[1]}" for c in CHAINS])
def test_plan_pass_equals_seam_fed_with_the_plans_predictor(eng, chain, mode, precision):
    """Every pass p >= 1 of a plan run (compact hand-off, written by the mask_out branch of the banded matrix-core
    predictor) against tpiv_iter fed with the four fields the same predictor writes through its other store branch from the
    plan's own pass p - 1: the same accumulators, the same kernels, so u, v and invalid are equal bit for bit."""
    from torchpiv_amd import synth
    (ws, ov), n_pass, (H, W) = chain
    # (sparse and noisy, so that every pass leaves invalid vectors and the next predictor's mask byte is set somewhere)
    pairs = [synth.make_pair(H, W, 300 + ws + i, kind=k, noise=8.0, density=0.012) for i, k in enumerate(("vortex", "wavy"))]
    a = torch.stack([p[0] for p in pairs]).cuda()
    b = torch.stack([p[1] for p in pairs]).cuda()
    plan = eng.Plan(H, W, ws, ov, n_pass=n_pass, mode=mode, max_batch=2, precision=precision)
    assert [g[:2] for g in plan.geometry] == [(ws >> p, ov >> p) for p in range(n_pass)]
    last = plan.run(a, b)
    fields = [plan.pass_fields(p, 2) if p < n_pass - 1 else last for p in range(n_pass)]
    for p in range(1, n_pass):
        w, o = plan.geometry[p][:2]
        four = plan.debug_predict(p, *fields[p - 1])
        seam = eng.iterate(mode, a, b, w, o, *four, precision=precision)
        n_mask = int((four[0] == 0).sum())
        for k, name in enumerate(("u", "v", "invalid")):
            same = torch.equal(seam[k], fields[p][k])
            if not same:
                g, s = host(fields[p][k]), host(seam[k])
                bad = np.argwhere(g != s)
                msg = [f"pass {p} (ws {w}) {name}: {len(bad)} of {g.size} cells differ"]
                for i in bad[:8]:
                    i = tuple(i)
                    msg.append(f"  {list(i)}: plan {g[i]!r} seam {s[i]!r}; u0 {host(four[0])[i]!r} v0 {host(four[1])[i]!r} "
                               f"u2 {host(four[2])[i]!r} v2 {host(four[3])[i]!r}")
                assert same, "\n".join(msg)
        print(f"  {mode} {precision} pass {p} (ws {w}, {plan.kernel_name(p)}): {fields[p][0].numel()} cells equal; "
              f"{n_mask} with a zero fallback, {int(fields[p][2].sum())} invalid")
    plan.close()
