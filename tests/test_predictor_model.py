"""tests/predictor_model.py -- the yardstick of tests/test_gpu_predictor_edges.py -- on the host alone: the case table reaches
what it says it reaches (by the grid arithmetic of launch_predict_mfma), the numpy model of the banded kernels passes the
checker on every case, every one-line mutant of that model fails it on a named case, and the reference masks leave the share of
undecided cells the decision rule is meant for."""
import numpy as np
import pytest

import predictor_model as PM

IDS = [c["id"] for c in PM.CASES]
# the case (and mask) that has to catch each mutant; the launch is sized for the case's largest batch, the first pairs computed
CAUGHT_BY = {
    "a": [("trips_17", "none"), ("both_walk", "r30"), ("cols_walk", "none")],
    "b": [("band_tail", "none"), ("exact32", "r30")],
    "c": [("rows_walk", "none"), ("cols_walk", "r30"), ("band_both", "none")],
    "d": [("cols_walk", "none"), ("both_walk", "r30")],
    "e": [("rows_walk", "all"), ("band_tail", "r30")],
}


def small_batch(case):
    fine = PM.passes(case)[-1]
    return min(PM.max_batch(case), 8 if fine[2] * fine[3] < 10000 else 3)


def run_model(case, p, kind, mode, mutant=None, n=None):
    n = n or small_batch(case)
    Ay, Ax = PM.operators(case, p)
    u, v = PM.fields(case, p, n)
    m = PM.mask(case, p, kind, n)
    ref = PM.reference(mode, Ay, Ax, u, v, m)
    outs = PM.banded_model(mode, Ay, Ax, u, v, m, launch_batch=PM.max_batch(case), mutant=mutant)
    return PM.check(mode, ref, outs), ref


def test_the_table_has_the_grids_it_promises():
    for c in PM.CASES:
        g = PM.passes(c)
        p = c["seq"][0]
        assert ((g[p - 1][2], g[p - 1][3]), (g[p][2], g[p][3])) == PM.GRIDS[c["id"]], (c["id"], [q[2:4] for q in g])
    assert len(set(IDS)) == len(IDS)


def test_every_case_labelled_as_walking_walks():
    """Fails when `slices` of launch_predict_mfma is retuned without revisiting the table."""
    for c in PM.CASES:
        for p in set(c["seq"]):
            g = PM.passes(c)
            for batch, kernel, stride in c["walks"]:
                L = PM.launch_shape(batch, g[p - 1][2], g[p - 1][3], g[p][2], g[p][3])
                assert L[kernel + "_walk"], (c["id"], batch, kernel, L)
                got = L["rows_grid"][0] if kernel == "rows" else L["cols_grid"][1]
                assert got == stride, (c["id"], batch, kernel, L)
    shape = {c["id"]: PM.launch_shape(max(c["batches"]), *PM.GRIDS[c["id"]][0], *PM.GRIDS[c["id"]][1]) for c in PM.CASES}
    assert (shape["rows_walk"]["nbc"], shape["cols_walk"]["nby"], shape["band_tail"]["nbc"]) == (3, 5, 5)
    assert shape["cols_walk"]["rows_early_exit"] and PM.GRIDS["cols_walk"][1][0] % 32 == 3
    assert PM.GRIDS["band_tail"][0][1] % 32 == 1 and PM.GRIDS["band_both"][0][1] % 32 == 0
    assert shape["exact32"]["nrfp"] == PM.GRIDS["exact32"][1][0] and PM.GRIDS["exact32"][1][1] % 32 == 1
    # no small batch walks: there the same kernels take one tile per wavefront
    for cid, batch in (("rows_walk", 3), ("cols_walk", 1), ("both_walk", 2)):
        L = PM.launch_shape(batch, *PM.GRIDS[cid][0], *PM.GRIDS[cid][1])
        assert not L["rows_walk"] and not L["cols_walk"], (cid, L)


def test_trip_counts_and_bands():
    trips, banded = set(), {}
    for c in PM.CASES:
        for p in set(c["seq"]):
            bd = PM.build_banded(*PM.operators(c, p))
            assert bd["KY"] % 8 == 0 and bd["KX"] % 8 == 0 and bd["leak"] <= PM.LEAK
            if c["id"].startswith("trips_"):
                trips |= {bd["KY"] // 8, bd["KX"] // 8}
            banded[c["id"]] = bd["bands"]
    assert trips == set(range(1, 10)), trips
    assert banded["trips_64"] == (False, False) and banded["trips_65"] == (False, False)
    assert banded["trips_66"] == (True, True) and banded["band_both"] == (True, True)
    assert banded["band_tail"] == (False, True) and banded["both_walk"] == (False, False)
    bd = PM.build_banded(*PM.operators(PM.CASE["band_tail"], 1))
    assert len(set(bd["k0x32"])) > 2                      # the band start drifts from block to block
    assert bd["k0x32"][-1] + bd["KX"] > 129               # ... and the last block's K runs past the matrix: loads read as 0


@pytest.mark.parametrize("cid", IDS)
def test_the_model_passes_the_checker(cid):
    c = PM.CASE[cid]
    for p in sorted(set(c["seq"])):
        n = small_batch(c)
        Ay, Ax = PM.operators(c, p)
        u, v = PM.fields(c, p, n)
        for kind in PM.MASKS:
            m = PM.mask(c, p, kind, n)
            ref = PM.reference("CWS", Ay, Ax, u, v, m)
            raw = PM.banded_raw(Ay, Ax, u, v, m, launch_batch=PM.max_batch(c))
            for mode in ("CWS", "DWS"):
                st = PM.check(mode, ref, PM.finish(mode, *raw))
                assert st, (cid, p, kind, mode, st.failures[:3])
                assert st.ratio < 0.5, (cid, p, kind, mode, st.ratio)       # the float64 host product: well inside the bound


def test_a_stale_work_buffer_does_not_reach_the_model():
    """p = 2, p = 1, p = 2 through one flat T1: the second p = 2 equals the first bit for bit."""
    c = PM.CASE["stale_T1"]
    g = PM.passes(c)
    n = 3
    T1 = np.full(n * 3 * max(g[p - 1][3] * ((g[p][2] + 31) // 32 * 32) for p in (1, 2)), np.nan)
    outs = []
    for p in c["seq"]:
        Ay, Ax = PM.operators(c, p)
        u, v = PM.fields(c, p, n)
        m = PM.mask(c, p, "r30", n)
        outs.append(PM.banded_model("CWS", Ay, Ax, u, v, m, T1=T1))
        assert PM.check("CWS", PM.reference("CWS", Ay, Ax, u, v, m), outs[-1])
    assert all(np.array_equal(a, b) for a, b in zip(outs[0], outs[2]))


@pytest.mark.parametrize("mutant", sorted(PM.MUTANTS))
def test_every_mutant_is_caught_by_a_named_case(mutant):
    for cid, kind in CAUGHT_BY[mutant]:
        c = PM.CASE[cid]
        p = c["seq"][0]
        seen = []
        for mode in ("CWS", "DWS"):
            st, _ = run_model(c, p, kind, mode, mutant=mutant)
            seen.append(len(st.failures))
            assert not st, f"mutant ({mutant}) {PM.MUTANTS[mutant]}: not seen by {cid} / {kind} / {mode}"
        print(f"  mutant ({mutant}) {PM.MUTANTS[mutant]}: caught by {cid} with mask {kind!r} ({seen[0]} / {seen[1]} rules broken in CWS / DWS)")


def test_a_dropped_last_trip_shows_at_every_odd_trip_count():
    """Mutant (a) over the trips family: caught wherever either trip count is odd, invisible where both are even."""
    for n in PM.TRIP_SIZES:
        c = PM.CASE[f"trips_{n}"]
        bd = PM.build_banded(*PM.operators(c, 1))
        odd = (bd["KY"] // 8) % 2 == 1 or (bd["KX"] // 8) % 2 == 1
        st, _ = run_model(c, 1, "none", "CWS", mutant="a", n=2)
        assert bool(st) == (not odd), (n, bd["KY"], bd["KX"], st.failures[:1])


def test_the_walk_mutant_needs_the_walk():
    """Mutant (c) is invisible at the batches that do not walk -- which is why the table has the large ones."""
    c = PM.CASE["rows_walk"]
    Ay, Ax = PM.operators(c, 1)
    u, v = PM.fields(c, 1, 3)
    m = PM.mask(c, 1, "r30", 3)
    ref = PM.reference("DWS", Ay, Ax, u, v, m)
    assert PM.check("DWS", ref, PM.banded_model("DWS", Ay, Ax, u, v, m, launch_batch=3, mutant="c"))
    assert not PM.check("DWS", ref, PM.banded_model("DWS", Ay, Ax, u, v, m, launch_batch=200, mutant="c"))


def test_the_checker_refuses_half_outcomes_and_wrong_halves():
    c = PM.CASE["exact32"]
    Ay, Ax = PM.operators(c, 1)
    u, v = PM.fields(c, 1, 2)
    m = PM.mask(c, 1, "half", 2)
    ref = PM.reference("CWS", Ay, Ax, u, v, m)
    und = PM.undecided(ref[2])
    assert und.any()
    i = tuple(np.argwhere(und)[0])
    for mode in ("CWS", "DWS"):
        good = PM.banded_model(mode, Ay, Ax, u, v, m)
        assert PM.check(mode, ref, good)
        raw = PM.finish(mode, ref[0].ref, ref[1].ref, np.zeros_like(ref[2].ref))
        for flip in (True, False):                         # either outcome of an undecided cell passes, when whole
            o = [a.copy() for a in good]
            src = PM.finish(mode, ref[0].ref, ref[1].ref, np.full_like(ref[2].ref, float(flip)))
            for a, s in zip(o, src):
                a[i] = s[i]
            assert PM.check(mode, ref, o), (mode, flip)
        o = [a.copy() for a in good]                       # ... but not u masked and v not
        o[0][i], o[1][i] = 0.0, raw[1][i]
        assert not PM.check(mode, ref, o)
        o = [a.copy() for a in good]                       # a decided cell with the other outcome
        j = tuple(np.argwhere(~und & (ref[2].ref < 0.5))[0])
        o[0][j] = o[1][j] = 0.0
        assert not PM.check(mode, ref, o)
        o = [a.copy() for a in good]                       # one ulp in u2
        o[2][j] = np.nextafter(o[2][j], np.inf)
        assert not PM.check(mode, ref, o)
        o = [a.copy() for a in good]                       # an error of four bounds in u0
        o[0][j] += 4 * ref[0].bound[j]
        o[2][j] = o[0][j] / 2 if mode == "CWS" else np.rint(o[0][j] / 2)
        assert not PM.check(mode, ref, o)
        o = [a.copy() for a in good]
        o[1][j] = np.nan
        assert not PM.check(mode, ref, o)


def test_undecided_cells_of_the_reference_masks():
    """From the reference alone: random masks leave few undecided cells (the rule is no blanket excuse), the half-plane mask
    leaves some in every case of the table (the tie branch runs; `trips` is one case of many sizes)."""
    cap = {"r05": 0.02, "r30": 0.05}
    half = {}
    for c in PM.CASES:
        for p in sorted(set(c["seq"])):
            n = small_batch(c)
            Ay, Ax = PM.operators(c, p)
            share = {}
            for kind in ("r05", "r30", "half"):
                M = PM.Field(Ay, Ax, PM.mask(c, p, kind, n).astype(np.float64))
                share[kind] = float(PM.undecided(M).mean())
            print(f"  {c['id']} p{p}: undecided r05 {share['r05']:.4%} r30 {share['r30']:.4%} half {share['half']:.4%}")
            for kind, top in cap.items():
                assert share[kind] <= top, (c["id"], p, kind, share[kind])
            row = "trips" if c["id"].startswith("trips_") else c["id"]
            half[row] = max(half.get(row, 0.0), share["half"])
    assert all(s > 0 for s in half.values()), half
