"""A numpy model of the device part of the post-validation (torchpiv_amd/csrc/postval.hip: postval_border_kernel,
postval_classify_kernel, postval_rules_kernel) that READS THE COMMITTED RULE TABLE (csrc/postval_rules.inc), SciPy's
LinearNDInterpolator as the referee, and the scenes on which the host and the GPU tests compare the three.

The model follows the kernels step by step -- same classes, same counts, same order of the rules, the same float64
expressions evaluated left to right -- so that everything but the rule sums (which the device may contract to FMA) is
comparable bit for bit.  Nothing here imports torch or the package."""
import os
import re
from collections import namedtuple
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES_INC = os.path.join(ROOT, "torchpiv_amd", "csrc", "postval_rules.inc")

# cell classes: the byte values of postval.hip
PV_VALID, PV_HOLE, PV_FILLED, PV_AMBIGUOUS, PV_GENERAL, PV_RING = 0, 1, 2, 3, 4, 5

# verts[k]: three (row, column) offsets; wfrac[k]: the weights as Fractions; w[k]: the float64 quotients the compiler
# makes of `a.0 / b.0`; blockers[k]: the first nb offsets of the padded list
Rules = namedtuple("Rules", "n_rules max_block verts wfrac w blockers")
Result = namedtuple("Result", "cls counts u v rule holes")

_PAIR = r"\{\s*(-?\d+)\s*,\s*(-?\d+)\s*\}"
_ROW = re.compile(r"^\s*\{\{(?P<v>(?:\s*%s\s*,?){3})\}\s*,\s*\{(?P<w>[^}]*)\}\s*,\s*(?P<nb>\d+)\s*,\s*\{(?P<b>(?:\s*%s\s*,?)*)\}\}\s*,"
                  % (_PAIR, _PAIR))


def parse_rules(path=RULES_INC):
    """The table of postval_rules.inc in file order."""
    with open(path) as f:
        text = f.read()
    head = re.search(r"constexpr int PV_N_RULES = (\d+), PV_MAX_BLOCK = (\d+);", text)
    n_rules, max_block = int(head.group(1)), int(head.group(2))
    verts, wfrac, w, blockers = [], [], [], []
    for line in text.splitlines():
        m = _ROW.match(line)
        if m is None:
            continue
        vs = [(int(a), int(b)) for a, b in re.findall(_PAIR, m.group("v"))]
        fr, fl = [], []
        for expr in m.group("w").split(","):
            q = re.fullmatch(r"\s*(\d+)\.0\s*/\s*(\d+)\.0\s*", expr)
            fr.append(Fraction(int(q.group(1)), int(q.group(2))))
            fl.append(float(q.group(1)) / float(q.group(2)))
        nb = int(m.group("nb"))
        bs = [(int(a), int(b)) for a, b in re.findall(_PAIR, m.group("b"))]
        assert len(vs) == 3 and len(fr) == 3 and len(bs) == max_block and nb <= max_block, line
        verts.append(tuple(vs))
        wfrac.append(tuple(fr))
        w.append(tuple(fl))
        blockers.append(tuple(bs[:nb]))
    assert len(verts) == n_rules, (len(verts), n_rules)
    return Rules(n_rules, max_block, tuple(verts), tuple(wfrac), tuple(w), tuple(blockers))


_RULES = None


def rules():
    global _RULES
    if _RULES is None:
        _RULES = parse_rules()
    return _RULES


def _neighbour_holes(hole):
    """hN, hS, hW, hE: the neighbour exists and is a hole (out of the field: no)."""
    z = np.zeros_like(hole)
    hN, hS, hW, hE = z.copy(), z.copy(), z.copy(), z.copy()
    hN[1:] = hole[:-1]
    hS[:-1] = hole[1:]
    hW[:, 1:] = hole[:, :-1]
    hE[:, :-1] = hole[:, 1:]
    return hN, hS, hW, hE


def model(u, v, invalid, table=None):
    """One pair through the three kernels.  Returns Result: cls (uint8, postval.hip's byte values), counts = (holes,
    ring, ambiguous, general left after the rules), the filled u and v (cells nobody fills keep their input bits), rule
    (int: which rule filled the cell, -1 elsewhere) and holes (bool: the cells that are holes after the border step)."""
    T = rules() if table is None else table
    u = np.array(u, dtype=np.float64)
    v = np.array(v, dtype=np.float64)
    hole = np.asarray(invalid).astype(bool).copy()
    nr, nc = hole.shape
    # ---- postval_border_kernel: first row, last row, first column, last column; later edges see the earlier ones' cells
    if hole.any():
        for sl in ((0, slice(None)), (nr - 1, slice(None)), (slice(None), 0), (slice(None), nc - 1)):
            h = hole[sl]                                   # (views: the edits land in the fields)
            if h.all() or not h.any():
                continue
            idx = np.arange(h.size)
            for f in (u, v):
                line = f[sl]
                line[h] = np.interp(idx[h], idx[~h], line[~h])
            h[:] = False
    holes = hole.copy()
    # ---- postval_classify_kernel
    hN, hS, hW, hE = _neighbour_holes(hole)
    cls = np.zeros((nr, nc), dtype=np.uint8)
    ring = ~hole & (hN | hS | hW | hE)
    cls[ring] = PV_RING
    rows, cols = np.indices((nr, nc))
    vN, vS, vW, vE = (rows > 0) & ~hN, (rows < nr - 1) & ~hS, (cols > 0) & ~hW, (cols < nc - 1) & ~hE
    amb = hole & vN & vS & vW & vE
    ns = hole & ~amb & vN & vS
    we = hole & ~amb & ~ns & vW & vE
    gen = hole & ~amb & ~ns & ~we
    cls[amb] = PV_AMBIGUOUS
    cls[ns | we] = PV_FILLED
    cls[gen] = PV_GENERAL
    for f in (u, v):
        r, c = np.nonzero(ns)
        f[r, c] = (f[r - 1, c] + f[r + 1, c]) * 0.5
        r, c = np.nonzero(we)
        f[r, c] = (f[r, c - 1] + f[r, c + 1]) * 0.5
    # ---- postval_rules_kernel: first match wins; ring() is false outside the field
    rule = np.full((nr, nc), -1, dtype=np.int32)

    def is_ring(r, c):
        return 0 <= r < nr and 0 <= c < nc and ring[r, c]

    for r, c in np.argwhere(gen):
        for k in range(T.n_rules):
            vs = T.verts[k]
            if not all(is_ring(r + dr, c + dc) for dr, dc in vs):
                continue
            if any(is_ring(r + dr, c + dc) for dr, dc in T.blockers[k]):
                continue
            w0, w1, w2 = (np.float64(x) for x in T.w[k])
            for f in (u, v):
                x0, x1, x2 = (f[r + dr, c + dc] for dr, dc in vs)
                f[r, c] = w0 * x0 + w1 * x1 + w2 * x2
            cls[r, c] = PV_FILLED
            rule[r, c] = k
            break
    counts = (int(hole.sum()), int(ring.sum()), int(amb.sum()), int((cls == PV_GENERAL).sum()))
    return Result(cls, counts, u, v, rule, holes)


def dropped(counts, cells):
    """The census's drop decisions: nothing to interpolate from, or the ring holds a quarter of the cells or more."""
    return counts[1] == 0 or 4 * counts[1] >= cells


def needs_host(counts, cells):
    return not dropped(counts, cells) and counts[2] + counts[3] > 0


def scipy_fill(field, ring, cells):
    """The referee: LinearNDInterpolator over np.argwhere(ring) with the field's values there, evaluated at `cells`
    ([m, 2] integer: the hole cells asked for).  None when Qhull refuses the points."""
    from scipy.interpolate import LinearNDInterpolator
    pts = np.argwhere(ring)
    try:
        return LinearNDInterpolator(pts, field[ring])(np.asarray(cells, dtype=np.float64))
    except Exception:          # noqa: BLE001 -- the reference's bare except: the pair is dropped
        return None


# ---------------------------------------------------------------------------------------------------------------------
# scenes: stacks of pairs [B, nr, nc] with u and v drawn from different random fields.  `tags[b]` says what pair b is:
# ("rule", k, origin) and the like, see the builders.
Scene = namedtuple("Scene", "name u v inv tags")


def _values(rng, shape, zeros=False):
    if zeros:
        return rng.choice(np.array([-0.0, 0.0, -1.0, 1.0, 2.0]), size=shape)
    return rng.standard_normal(shape) * 4 + 2


def _stack(name, masks, tags, seed, zeros=False):
    rng = np.random.default_rng(seed)
    inv = np.stack(masks)
    return Scene(name, _values(rng, inv.shape, zeros), _values(rng, inv.shape, zeros), inv, tuple(tags))


def _pattern(shape, origin, k, leave=None):
    """Holes at the origin and at rule k's blocker cells (those inside the field), but for the blocker `leave`."""
    m = np.zeros(shape, dtype=bool)
    m[origin] = True
    for b in rules().blockers[k]:
        r, c = origin[0] + b[0], origin[1] + b[1]
        if b != leave and 0 <= r < shape[0] and 0 <= c < shape[1]:
            m[r, c] = True
    return m


def scene_own(zeros=False):
    """For every rule k an 11 x 11 field, holes at (5, 5) and at rule k's blocker cells."""
    n = rules().n_rules
    return _stack("zeros own" if zeros else "own", [_pattern((11, 11), (5, 5), k) for k in range(n)],
                  [("rule", k, (5, 5)) for k in range(n)], 101 + zeros, zeros)


def scene_blockers():
    """The same with one blocker left valid, for every (rule, blocker): that cell is then a ring cell inside the disc."""
    T = rules()
    kb = [(k, b) for k in range(T.n_rules) for b in T.blockers[k]]
    return _stack("blockers", [_pattern((11, 11), (5, 5), k, leave=b) for k, b in kb],
                  [("blocker", k, (5, 5), b) for k, b in kb], 103)


BORDER_ORIGINS = ((1, 5), (2, 5), (7, 5), (6, 5), (4, 1), (4, 2), (4, 10), (4, 9), (1, 1), (7, 10), (2, 2), (6, 9))


def scene_borders():
    """9 x 12 fields with the origin one and two cells from each edge and in two corners: blockers and vertices fall on
    the interpolated border or outside the field."""
    ko = [(k, o) for k in range(rules().n_rules) for o in BORDER_ORIGINS]
    return _stack("borders", [_pattern((9, 12), o, k) for k, o in ko], [("rule", k, o) for k, o in ko], 104)


def scene_tiled(zeros=False):
    """All own patterns as 7 x 7 tiles (8 rows of 5) inside one 58 x 37 field: 2146 cells, more than one block."""
    m = np.zeros((58, 37), dtype=bool)
    origins = []
    for k in range(rules().n_rules):
        o = (1 + 7 * (k // 5) + 3, 1 + 7 * (k % 5) + 3)
        m |= _pattern(m.shape, o, k)
        origins.append(o)
    return _stack("zeros tiled" if zeros else "tiled", [m], [("tiled", tuple(origins))], 105 + zeros, zeros)


def scene_mixed():
    """Own fields interleaved with pairs that are dropped (no hole, all invalid, 30 % holes) and with pairs that need the
    host (one isolated hole: AMBIGUOUS) -- a pair's counts must not leak into its neighbours'."""
    rng = np.random.default_rng(107)
    masks, tags = [], []
    for k in range(rules().n_rules):
        masks.append(_pattern((11, 11), (5, 5), k))
        tags.append(("rule", k, (5, 5)))
        kind = k % 4
        m = np.zeros((11, 11), dtype=bool)
        if kind == 1:
            m[:] = True
        elif kind == 2:
            m = rng.random((11, 11)) < 0.3
        elif kind == 3:
            m[int(rng.integers(2, 9)), int(rng.integers(2, 9))] = True
        masks.append(m)
        tags.append((("no hole", "all invalid", "30 % holes", "isolated hole")[kind],))
    return _stack("mixed batch", masks, tags, 108)


def scene_clustered():
    """64 random 11 x 11 fields, densities 0.1 - 0.3, clustered by roll-and-or like the masks of
    test_postval_device_vs_host; the odd ones keep their border holes, the even ones have a clean border.  Candidates
    the census would drop (a condition on the mask alone) are drawn again."""
    rng = np.random.default_rng(109)
    masks, tags = [], []
    zero = np.zeros((11, 11))
    while len(masks) < 64:
        k = len(masks)
        dens = float(rng.choice([0.1, 0.15, 0.2, 0.25, 0.3]))
        m = rng.random((11, 11)) < dens
        m |= np.roll(m, 1, axis=k % 2) & (rng.random((11, 11)) < 0.5)
        if k % 2 == 0:
            m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = False
        if dropped(model(zero, zero, m).counts, m.size):
            continue
        masks.append(m)
        tags.append(("clustered", dens, k % 2 == 1))
    return _stack("clustered", masks, tags, 110)


SCENE_NAMES = ("own", "blockers", "borders", "tiled", "mixed batch", "zeros own", "zeros tiled", "clustered")
_SCENES = None


def scenes():
    """Every scene, built once (the arrays are shared: nobody writes into them)."""
    global _SCENES
    if _SCENES is None:
        built = [scene_own(), scene_blockers(), scene_borders(), scene_tiled(), scene_mixed(), scene_own(zeros=True),
                 scene_tiled(zeros=True), scene_clustered()]
        for s in built:
            for a in (s.u, s.v, s.inv):
                a.flags.writeable = False
        _SCENES = {s.name: s for s in built}
        assert tuple(_SCENES) == SCENE_NAMES
    return _SCENES


_MODELS = {}


def scene_model(name):
    """[model(pair) for every pair of the scene], computed once."""
    if name not in _MODELS:
        s = scenes()[name]
        _MODELS[name] = [model(s.u[b], s.v[b], s.inv[b]) for b in range(s.inv.shape[0])]
    return _MODELS[name]


# |model - SciPy| <= SCIPY_GATE * 2^-52 * M on every cell the model fills (M: the pair's largest ring value in magnitude,
# per component).  SciPy's error is not derived here: the worst ratio over all scenes was MEASURED as 1.02 (the borders
# scene; profiles/postval_rules/README.md) and the gate is four times that figure -- room for SciPy builds whose LAPACK
# rounds the 2 x 2 barycentric transforms differently.
SCIPY_MEASURED = 1.02
SCIPY_GATE = 4 * SCIPY_MEASURED
# |device - model| <= RULE_BOUND * 2^-52 * M on a rule fill: both evaluate w0 x0 + w1 x1 + w2 x2 with the same rounded
# weights, the model with five roundings (three products, two sums), the device with five or, contracted to FMA, fewer;
# every intermediate is at most M in magnitude up to rounding, so each side is within 5 * 2^-53 * M of the exact sum.
RULE_BOUND = 5.0

_SCIPY = {}


def scene_scipy(name):
    """Per pair of the scene: None for a pair the census drops, else (cells [m, 2], SciPy's values [m, 2] for u and v) at
    the cells the model fills -- values None when Qhull refuses the ring.  Computed once."""
    if name not in _SCIPY:
        out = []
        for res in scene_model(name):
            if dropped(res.counts, res.cls.size):
                out.append(None)
                continue
            cells = np.argwhere(res.cls == PV_FILLED)
            out.append((cells, scipy_fill(np.stack([res.u, res.v], axis=-1), res.cls == PV_RING, cells)))
        _SCIPY[name] = out
    return _SCIPY[name]


def ring_magnitude(res):
    """(largest |u|, largest |v|) over the ring cells of a model result: the M of the tests' bounds, per component."""
    ring = res.cls == PV_RING
    return float(np.abs(res.u[ring]).max()), float(np.abs(res.v[ring]).max())


def fired(results):
    """The set of rules that filled a cell somewhere in these model results."""
    out = set()
    for r in results:
        out |= set(int(k) for k in np.unique(r.rule) if k >= 0)
    return out


def mutate(table, k, verts=None, w=None, blockers=None):
    """The table with rule k's vertices, float weights or blockers replaced."""
    def put(seq, new):
        return seq if new is None else tuple(new if i == k else x for i, x in enumerate(seq))
    return table._replace(verts=put(table.verts, verts), w=put(table.w, w), blockers=put(table.blockers, blockers))
