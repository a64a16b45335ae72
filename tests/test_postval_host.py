"""The device part of the post-validation without a GPU: the committed rule table against its generator, the numpy model
of the kernels (tests/postval_model.py) against SciPy on every scene, the conditions under which the scenes cover all 40
rules, how sharp the scenes are against a mutated table, and the two host pieces of the same path: the fill-worker pool
shared by several generators and the diamond short cut's sign of zero."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

import postval_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -52


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_committed_rule_table_is_what_the_generator_makes():
    """csrc/postval_rules.inc = tools/research/fill_rules.rules(5/2): count, order, vertex offsets, weights as fractions,
    blocker lists, PV_MAX_BLOCK."""
    sys.path.insert(0, os.path.join(ROOT, "tools", "research"))
    try:
        import fill_rules
    finally:
        sys.path.pop(0)
    want = fill_rules.rules(Fraction(5, 2))
    T = P.parse_rules()
    assert T.n_rules == len(want) == len(T.verts) == 40
    assert T.max_block == max(len(block) for _, _, block, _ in want)
    for k, (tri, w, block, r2) in enumerate(want):
        assert T.verts[k] == tuple(tuple(int(x) for x in p) for p in tri), k
        assert T.wfrac[k] == tuple(w) and sum(T.wfrac[k]) == 1, k
        assert T.w[k] == tuple(float(x.numerator) / float(x.denominator) for x in w), k
        assert T.blockers[k] == tuple(block), k
        assert r2 <= Fraction(5, 2)
    # the struct holds signed chars and nb of them: nothing in the table may outgrow that
    assert all(-128 <= x <= 127 for vs in T.verts + T.blockers for p in vs for x in p)


@pytest.mark.parametrize("name", P.SCENE_NAMES)
def test_model_agrees_with_scipy_on_every_filled_cell(name):
    """Every cell the model fills (straight runs and rules) holds SciPy's Delaunay-linear value to SCIPY_GATE * 2^-52 * M;
    Qhull refuses no scene field, and only the deliberately dropped pairs of the mixed batch are dropped."""
    s = P.scenes()[name]
    worst = n_cells = 0
    for b, (res, sc) in enumerate(zip(P.scene_model(name), P.scene_scipy(name))):
        if sc is None:
            assert name == "mixed batch" and s.tags[b][0] in ("no hole", "all invalid", "30 % holes"), (name, b, s.tags[b])
            continue
        assert s.tags[b][0] not in ("no hole", "all invalid", "30 % holes"), (name, b)
        cells, vals = sc
        assert vals is not None, (name, b, "Qhull refused the ring")
        if not len(cells):
            continue
        r, c = cells[:, 0], cells[:, 1]
        for f, col, M in zip((res.u, res.v), (0, 1), P.ring_magnitude(res)):
            assert np.isfinite(vals[:, col]).all(), (name, b)
            ratio = float((np.abs(f[r, c] - vals[:, col]) / (ULP * M)).max())
            worst = max(worst, ratio)
            assert ratio <= P.SCIPY_GATE, (name, b, ratio)
        n_cells += len(cells)
    print(f"  {name}: {n_cells} filled cells, worst |model - SciPy| / (2^-52 M) = {worst:.3f} (gate {P.SCIPY_GATE:.2f})")
    assert n_cells > 0


def test_scenes_cover_every_rule():
    """Conditions on the inputs, by the model alone: rule k fills the origin of own field k; all 40 fire in tiled; with one
    blocker valid rule k never fills the origin; every rule fills its origin in at least one border placement; the pairs of
    the mixed batch are dropped / need the host as they are meant to."""
    n = P.rules().n_rules
    S = P.scenes()
    for name in ("own", "zeros own"):
        for res, tag in zip(P.scene_model(name), S[name].tags):
            assert res.rule[tag[2]] == tag[1], (name, tag)
            assert res.counts[0] in (3, 4, 9), (name, tag, res.counts)
        assert P.fired(P.scene_model(name)) == set(range(n))
    for name in ("tiled", "zeros tiled"):
        res, origins = P.scene_model(name)[0], S[name].tags[0][1]
        assert [int(res.rule[o]) for o in origins] == list(range(n)), name
        assert 4 * res.counts[1] < res.cls.size and res.cls.size > 8 * 256, (name, res.counts)
    assert len(S["blockers"].tags) == 276
    for res, tag in zip(P.scene_model("blockers"), S["blockers"].tags):
        assert res.rule[tag[2]] != tag[1], tag
    assert len(S["borders"].tags) == 480
    hits = [tag[1] for res, tag in zip(P.scene_model("borders"), S["borders"].tags) if res.rule[tag[2]] == tag[1]]
    assert set(hits) == set(range(n)), sorted(set(range(n)) - set(hits))
    want = {"rule": "complete or host", "no hole": "dropped", "all invalid": "dropped", "30 % holes": "dropped",
            "isolated hole": "host"}
    for res, tag in zip(P.scene_model("mixed batch"), S["mixed batch"].tags):
        cells = res.cls.size
        state = "dropped" if P.dropped(res.counts, cells) else "host" if P.needs_host(res.counts, cells) else "complete"
        assert state in want[tag[0]], (tag, res.counts)
        if tag[0] == "rule":
            assert res.rule[tag[2]] == tag[1], tag
        if tag[0] == "isolated hole":
            assert res.counts == (1, 4, 1, 0), (tag, res.counts)
    assert len(S["clustered"].tags) == 64 and sum(t[2] for t in S["clustered"].tags) == 32
    for name in S:
        print(f"  {name}: {S[name].inv.shape[0]} pairs, rules fired {len(P.fired(P.scene_model(name)))} of {n}"
              + (f", origin hits {len(hits)}" if name == "borders" else ""))


def _differs(table, name, b):
    """The mutated table changes a class or a value (bits) of pair b of the scene."""
    s, ref = P.scenes()[name], P.scene_model(name)[b]
    got = P.model(s.u[b], s.v[b], s.inv[b], table=table)
    return not (np.array_equal(got.cls, ref.cls) and np.array_equal(_bits(got.u), _bits(ref.u))
                and np.array_equal(_bits(got.v), _bits(ref.v)))


def _caught(table, k, first=()):
    """Some pair of the scenes tells the mutant of rule k from the table: the pairs named in `first`, rule k's own field,
    its blocker and border fields, every other own field, the tiled field (in that order; the first hit ends the search)."""
    S = P.scenes()
    order = list(first) + [("own", k)]
    order += [(name, b) for name in ("blockers", "borders") for b, tag in enumerate(S[name].tags) if tag[1] == k]
    order += [("own", b) for b in range(P.rules().n_rules) if b != k] + [("tiled", 0)]
    return any(_differs(table, name, b) for name, b in order)


def test_scenes_tell_a_mutated_table_from_the_committed_one():
    """Sharpness of the scenes: for every rule, two unequal weights swapped, every vertex moved by one cell in each of the
    four directions, every single blocker deleted -- the model with the mutated table against the model with the committed
    one.  Every weight and vertex mutant changes a class or a value.  A blocker deletion can only show where the freed
    cell is a ring cell and rule k is the first to match: the ones no scene shows are those whose origin, with that
    blocker valid, is already taken by the straight-run fill or by an earlier rule."""
    T = P.rules()
    S = P.scenes()
    n_w = n_v = 0
    for k in range(T.n_rules):
        w = T.w[k]
        pairs = [(i, j) for i in range(3) for j in range(i + 1, 3) if w[i] != w[j]]
        if pairs:                                   # (rules 0-3 weigh 1/3 three times: nothing to swap)
            i, j = pairs[0]
            m = list(w)
            m[i], m[j] = m[j], m[i]
            assert _caught(P.mutate(T, k, w=tuple(m)), k), ("weights", k)
            n_w += 1
        for i in range(3):
            for d in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                moved = (T.verts[k][i][0] + d[0], T.verts[k][i][1] + d[1])
                if moved == (0, 0) or moved in T.verts[k]:
                    continue
                vs = tuple(moved if q == i else p for q, p in enumerate(T.verts[k]))
                assert _caught(P.mutate(T, k, verts=vs), k), ("vertex", k, i, d)
                n_v += 1
    assert n_w == 36 and n_v >= 3 * 3 * T.n_rules
    rows, n_caught = [], 0
    by_tag = {(tag[1], tag[3]): b for b, tag in enumerate(S["blockers"].tags)}
    for k in range(T.n_rules):
        caught, straight, earlier = 0, 0, 0
        for bl in T.blockers[k]:
            b = by_tag[(k, bl)]
            if _caught(P.mutate(T, k, blockers=tuple(x for x in T.blockers[k] if x != bl)), k, first=[("blockers", b)]):
                caught += 1
                continue
            res, o = P.scene_model("blockers")[b], S["blockers"].tags[b][2]
            took = int(res.rule[o])
            assert res.cls[o] == P.PV_FILLED and took < k, (k, bl, int(res.cls[o]), took)
            straight += took < 0
            earlier += took >= 0
        rows.append((k, len(T.blockers[k]), caught, straight, earlier))
        n_caught += caught
    print(f"  {n_w} weight mutants and {n_v} vertex mutants caught; blocker deletions caught {n_caught} of 276")
    print("  rule  blockers  caught  origin filled by a straight run  origin taken by an earlier rule")
    for row in rows:
        print("  %4d  %8d  %6d  %31d  %30d" % row)
    assert sum(r[1] for r in rows) == 276 and n_caught > 0


def _jobs(rng, n, nh):
    out = []
    for _ in range(n):
        hole = np.zeros((12, 12), bool)
        idx = rng.choice(100, nh, replace=False)
        hole[1 + idx // 10, 1 + idx % 10] = True
        pts = np.argwhere(~hole)
        out.append((pts, rng.normal(size=(pts.shape[0], 2)), np.argwhere(hole)))
    return out


def test_fill_workers_keep_the_tickets_of_two_owners_apart():
    """Two pipelines on one pool, advanced alternately (what two batched() generators of one OfflinePIV do): submit a1, a2;
    collect a1; submit b1, b2; collect b1; submit a3; collect a2 ... -- every collect(forget_older=True) returns its own
    answers, an owner's abandoned tickets are forgotten when it collects a later one, the other owner's stay; the answers
    of an owner that no longer exists go at the next collect."""
    from torchpiv_amd._qhull import FillWorkers, PipelineOwner, qhull_fill
    rng = np.random.default_rng(5)
    batch = {name: _jobs(rng, n, nh) for name, n, nh in (("a1", 3, 3), ("a2", 4, 4), ("a3", 2, 5), ("a4", 3, 3), ("a5", 1, 4),
                                                        ("a6", 2, 3), ("b1", 5, 3), ("b2", 2, 6), ("b3", 3, 4), ("b4", 1, 3),
                                                        ("c1", 2, 3))}
    owners = {"a": PipelineOwner(), "b": PipelineOwner(), "c": PipelineOwner()}
    fw = FillWorkers(2)
    t = {}

    def submit(name):
        t[name] = fw.submit(batch[name], owner=owners[name[0]])

    def collect(name):
        got = fw.collect(t[name], forget_older=True, owner=owners[name[0]])
        assert len(got) == len(batch[name]), name
        for g_, j in zip(got, batch[name]):
            assert np.array_equal(_bits(g_), _bits(qhull_fill(*j))), name

    try:
        for step in ("+a1", "+a2", "-a1", "+b1", "+b2", "-b1", "+a3", "-a2", "+b3", "-b2", "-a3"):
            (submit if step[0] == "+" else collect)(step[1:])
        # owner A abandons a4 and a5 (a generator closed with batches in flight), then collects a later ticket: both are
        # forgotten, b3 -- older than all of them -- is still there for its owner
        for step in ("+a4", "+a5", "+a6", "-a6"):
            (submit if step[0] == "+" else collect)(step[1:])
        assert t["a4"] not in fw._ready and t["a5"] not in fw._ready and t["b3"] in fw._ready
        with pytest.raises(KeyError):
            fw.collect(t["b3"], owner=owners["a"])             # not a's to collect
        collect("b3")
        # a pipeline that went away with a batch in flight: its answers are read off the pipes on the way to b4 and dropped
        submit("c1")
        del owners["c"]
        submit("b4")
        collect("b4")
        assert not fw._order and not fw._ready and not fw._parts and not fw._owner
    finally:
        fw.terminate()
    assert all(not p.is_alive() for p in fw.procs)


def test_diamond_short_cut_keeps_the_sign_of_zero_of_the_general_path():
    """qhull_fill(diamonds=True) against diamonds=False and against the literal LinearNDInterpolator call, as uint64 views,
    on fields of isolated holes whose ring values are mostly -0.0 / +0.0 and rounded numbers: the general path accumulates
    from +0.0, so two -0.0 ends give +0.0 there, and the short cut must say the same."""
    from scipy.spatial import Delaunay
    from torchpiv_amd import _qhull
    rng = np.random.default_rng(91)
    pool = np.array([-0.0] * 6 + [0.0, 1.0, -1.0, 2.5])
    n_fields = n_zero_pairs = 0
    for trial in range(200):
        nr, nc = (int(x) for x in rng.integers(8, 40, 2))
        hole = np.zeros((nr, nc), bool)
        for _ in range(int(rng.integers(1, 30))):
            r, c = int(rng.integers(1, nr - 1)), int(rng.integers(1, nc - 1))
            if hole[r - 1:r + 2, c].any() or hole[r, c - 1:c + 2].any():
                continue
            hole[r, c] = True
        d = hole.copy()
        d[1:] |= hole[:-1]
        d[:-1] |= hole[1:]
        d[:, 1:] |= hole[:, :-1]
        d[:, :-1] |= hole[:, 1:]
        pts, tg = np.argwhere(d & ~hole), np.argwhere(hole)
        vals = rng.choice(pool, size=(len(pts), 2))
        short = _qhull._diamond_fill(Delaunay(pts), pts, vals, tg)
        assert short is not None, trial                                          # the short cut is the path taken
        fast = _qhull.qhull_fill(pts, vals, tg)
        slow = _qhull.qhull_fill(pts, vals, tg, diamonds=False)
        ref = _qhull.qhull_fill_reference(pts, vals, tg)
        assert np.array_equal(_bits(fast), _bits(short)), trial
        assert np.array_equal(_bits(fast), _bits(slow)), (trial, np.argwhere(_bits(fast) != _bits(slow))[:5].tolist())
        assert np.array_equal(_bits(fast), _bits(ref)), trial
        assert not np.signbit(fast[fast == 0]).any(), trial
        n_fields += 1
        # the case is in play: some hole of this field lies between two -0.0 (all four neighbours -0.0)
        field = np.zeros((nr, nc))
        field[pts[:, 0], pts[:, 1]] = vals[:, 0]
        r, c = tg[:, 0], tg[:, 1]
        n_zero_pairs += int((np.signbit(field[r - 1, c]) & np.signbit(field[r + 1, c]) & (field[r - 1, c] == 0)
                             & (field[r + 1, c] == 0) & np.signbit(field[r, c - 1]) & np.signbit(field[r, c + 1])
                             & (field[r, c - 1] == 0) & (field[r, c + 1] == 0)).any())
    print(f"  {n_fields} fields bit-identical, {n_zero_pairs} of them with a hole between -0.0 ends on both diagonals")
    assert n_fields == 200 and n_zero_pairs >= 20
