"""tpiv_postval's triangulation-free fills on the device against the numpy model of tests/postval_model.py, which reads
the committed rule table: scenes that fire every one of the 40 rules of postval_rules.inc (alone, with one blocker
valid, next to the border, tiled over more than one block, in a batch with dropped and host-bound pairs, on zeros of
either sign, on random clustered holes), the packed lists of tpiv_postval_compact for the same batches, and two
generators of one ResidentPIV advanced alternately over a shared pool of fill workers."""
import itertools

import numpy as np
import pytest
import torch

import postval_model as P

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -52
N_RULES = 40


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _postval(eng, s):
    """ONE tpiv_postval call on the scene's stacked batch.  Returns the device tensors (U, V, cls, counts)."""
    U = torch.from_numpy(np.array(s.u)).cuda()
    V = torch.from_numpy(np.array(s.v)).cuda()
    M = torch.from_numpy(s.inv.astype(np.uint8)).cuda()
    cls, counts = eng.postval(U, V, M)
    torch.cuda.synchronize()
    return U, V, cls, counts


@pytest.mark.parametrize("name", P.SCENE_NAMES)
def test_device_fills_equal_the_model(eng, name):
    """Per pair: classes byte for byte, the four counts, every cell that is no hole after the border step bit for bit
    (border interpolation, untouched cells), cells left AMBIGUOUS / GENERAL with their input bits, straight-run fills bit
    for bit ((a + b) * 0.5: one addition and an exact halving leave nothing to contract -- -0.0 included), rule fills
    within RULE_BOUND * 2^-52 * M of the model (derived: postval_model.RULE_BOUND) and within that plus the host test's
    measured gate of SciPy (zeros compared by value).  The coverage is read off the model's rule map again."""
    s = P.scenes()[name]
    models, refs = P.scene_model(name), P.scene_scipy(name)
    U, V, cls, counts = (t.cpu().numpy() for t in _postval(eng, s))
    n_rule = n_straight = 0
    worst_m = worst_s = 0.0
    for b, res in enumerate(models):
        what = (name, b, s.tags[b])
        assert np.array_equal(cls[b], res.cls), (what, np.argwhere(cls[b] != res.cls)[:5].tolist())
        assert tuple(int(x) for x in counts[b]) == res.counts, (what, counts[b].tolist(), res.counts)
        left = (res.cls == P.PV_AMBIGUOUS) | (res.cls == P.PV_GENERAL) | (res.cls == P.PV_HOLE)
        straight = (res.cls == P.PV_FILLED) & (res.rule < 0)
        by_rule = res.rule >= 0
        for got, inp, want in ((U[b], s.u[b], res.u), (V[b], s.v[b], res.v)):
            assert np.array_equal(_bits(got[~res.holes]), _bits(want[~res.holes])), what
            assert np.array_equal(_bits(got[left]), _bits(inp[left])), what
            assert np.array_equal(_bits(got[straight]), _bits(want[straight])), what
        n_straight += int(straight.sum())
        if not by_rule.any():
            continue
        n_rule += int(by_rule.sum())
        for got, want, M in zip((U[b], V[b]), (res.u, res.v), P.ring_magnitude(res)):
            d = float(np.abs(got[by_rule] - want[by_rule]).max()) / (ULP * M)
            worst_m = max(worst_m, d)
            assert d <= P.RULE_BOUND, (what, d)
    # against the referee, on every cell the device filled (the straight runs carry the model's bits: the host gate alone)
    for b, (res, sc) in enumerate(zip(models, refs)):
        if sc is None or not len(sc[0]):
            continue
        cells, vals = sc
        assert vals is not None, (name, b)
        r, c = cells[:, 0], cells[:, 1]
        bound = np.where(res.rule[r, c] >= 0, P.RULE_BOUND, 0.0) + P.SCIPY_GATE
        for got, col, M in zip((U[b], V[b]), (0, 1), P.ring_magnitude(res)):
            d = np.abs(got[r, c] - vals[:, col]) / (ULP * M)
            worst_s = max(worst_s, float(d.max()))
            assert (d <= bound).all(), (name, b, s.tags[b], float(d.max()))
    hit = P.fired(models)
    print(f"  {name}: {len(models)} pairs, {n_straight} straight-run fills bit for bit, {n_rule} rule fills by {len(hit)} rules: "
          f"worst |device - model| {worst_m:.2f}, |device - SciPy| {worst_s:.2f} (x 2^-52 M)")
    if name in ("own", "zeros own", "tiled", "zeros tiled", "mixed batch", "borders"):
        assert hit == set(range(N_RULES)), (name, sorted(set(range(N_RULES)) - hit))
    if name in ("own", "zeros own", "mixed batch"):
        own = [(res, tag) for res, tag in zip(models, s.tags) if tag[0] == "rule"]
        assert len(own) == N_RULES and all(res.rule[tag[2]] == tag[1] for res, tag in own), name
    if name in ("tiled", "zeros tiled"):
        assert [int(models[0].rule[o]) for o in s.tags[0][1]] == list(range(N_RULES)), name
    if name == "borders":
        assert len({tag[1] for res, tag in zip(models, s.tags) if res.rule[tag[2]] == tag[1]}) == N_RULES
    if name == "blockers":
        assert len(models) == 276 and not any(res.rule[tag[2]] == tag[1] for res, tag in zip(models, s.tags))
    if name.startswith("zeros"):
        # the sign of zero is in play: some straight-run fill of the scene is -0.0
        assert any(np.signbit(f[(f == 0) & (res.cls == P.PV_FILLED) & (res.rule < 0)]).any()
                   for res in models for f in (res.u, res.v)), name
    assert n_rule > 0 and n_straight > 0


@pytest.mark.parametrize("name", ["tiled", "mixed batch"])
def test_compact_lists_of_the_scenes(eng, name):
    """tpiv_postval_compact behind the same batches: room in the lists for exactly the pairs the model says need the host
    (kept, with an AMBIGUOUS or GENERAL cell left), their ring cells, ring values and hole cells in np.argwhere order."""
    s = P.scenes()[name]
    models = P.scene_model(name)
    U, V, cls, counts = _postval(eng, s)
    off, rc, uv, hc = (t.cpu().numpy() for t in eng.postval_compact(U, V, cls, counts))
    B, cells = len(models), s.inv[0].size
    n_need = 0
    for b, res in enumerate(models):
        r0, r1, h0, h1 = off[0, b], off[0, b + 1], off[1, b], off[1, b + 1]
        if not P.needs_host(res.counts, cells):
            assert r0 == r1 and h0 == h1, (name, b, s.tags[b])
            continue
        n_need += 1
        ring, hole = res.cls == P.PV_RING, (res.cls >= P.PV_HOLE) & (res.cls <= P.PV_GENERAL)
        assert np.array_equal(rc[r0:r1], np.argwhere(ring)), (name, b)
        assert np.array_equal(hc[h0:h1], np.argwhere(hole)), (name, b)
        assert np.array_equal(_bits(uv[r0:r1, 0]), _bits(res.u[ring])), (name, b)
        assert np.array_equal(_bits(uv[r0:r1, 1]), _bits(res.v[ring])), (name, b)
    assert off[0, 0] == 0 and off[1, 0] == 0 and n_need == sum(P.needs_host(m.counts, cells) for m in models) > 0
    if name == "mixed batch":
        kinds = {tag[0] for res, tag in zip(models, s.tags) if not P.needs_host(res.counts, cells)}
        assert {"no hole", "all invalid", "30 % holes", "rule"} <= kinds and n_need < B


def test_two_generators_of_one_object_share_the_fill_workers(eng):
    """fill_workers = 2 and two batched() generators of one ResidentPIV (the even and the odd pairs) advanced alternately:
    both pipelines have tickets in the shared pool at the same time, and each must get its own answers back -- the
    tuples are, array for array, those of the two generators run one after the other."""
    import torchpiv_amd as T
    from torchpiv_amd import synth
    n = 32                                              # four launches of four pairs per generator: tickets of both in flight
    A, Bf = synth.make_batch(n, 256, 320, first_index=40, noise=2.0, device="cuda")
    for i in range(n):
        for (y, x) in ((60, 70), (150, 200), (200, 90)):
            A[i, y:y + 40, x:x + 40 + 8 * (i % 6)] = 0
            Bf[i, y:y + 40, x:x + 40 + 8 * (i % 6)] = 0
    even, odd = list(range(0, n, 2)), list(range(1, n, 2))
    piv = T.ResidentPIV(A, Bf, 32, 16, multipass=2, multipass_mode="CWS")
    piv.fill_workers = 2
    try:
        def keep(r):
            return tuple(np.array(t) for t in r)
        want = [[keep(r) for r in piv.batched(4, indices=idx)] for idx in (even, odd)]
        assert piv.stats["host_fallback"] >= n // 2 and min(len(w) for w in want) >= 12, (dict(piv.stats), [len(w) for w in want])
        got = [[], []]
        for ra, rb in itertools.zip_longest(piv.batched(4, indices=even), piv.batched(4, indices=odd)):
            for k, r in enumerate((ra, rb)):
                if r is not None:
                    got[k].append(keep(r))
        for k in range(2):
            assert len(got[k]) == len(want[k]), (k, len(got[k]), len(want[k]))
            for g_, w_ in zip(got[k], want[k]):
                assert len(g_) == len(w_) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(g_, w_)), (k, g_[0])
        assert not piv._pool._order and not piv._pool._ready
    finally:
        piv.close()
