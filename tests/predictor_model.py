"""The spline predictor between the passes -- out = Ay . Z . Ax^T for Z = u, v and the invalid bytes, then the hand-off
(tests/handoff_model.py) -- as a host yardstick for the banded matrix-core kernels of torchpiv_amd/csrc/predict_mfma.hip and
for the dense kernel behind engine.predict.  Plain numpy; the GPU tests import it.

reference      float64 (and, for three pairs, long double) products with the host operators of engine.spline_matrix, which
               tests/test_host_logic.py pins to FITPACK.
bound          DERIVED, not measured.  Each output cell is two chained dot products of at most nrc + 8 and ncc + 8 terms
               (K is the operator or the band rounded up to 8; the zero padding adds no error), so with u = 2**-53
                   |err| <= (nrc + ncc + 16) u S,          S = |Ay| |Z| |Ax|^T  (elementwise absolute values)
               to first order.  build_banded may drop operator entries up to 1e-17: with Ay = By + Ey, |Ey| <= 1e-17,
                   |Ay Z Ax^T - By Z Bx^T| <= 1e-17 (1 |Z| |Ax|^T + |Ay| |Z| 1^T + 1e-17 1 |Z| 1^T) =: 1e-17 S_full.
               The float64 reference obeys the same bound, so a kernel is compared with it at twice the bound per cell and
               with the long double pairs at once the bound.
check          the decision rule of the mask threshold (`>= 0.5`): cells whose reference mask lies further from 0.5 than its
               tolerance are decided and must show that outcome; in the others either outcome passes, but whole: both
               components zero, or both the raw predictor.  u2, v2 are checked on the kernel's own u0, v0 (CWS: u0 / 2 bit for
               bit where the kernel did not mask, raw / 2 within tolerance where it did; DWS: rint(u0 / 2) exactly).
banded_model   build_banded (c_api.cpp) and the data flow of the two kernels in numpy: band starts, K x 32 weight tiles, k0 per
               block of 32, the transposed T1 of pitch nrfp in one flat buffer, buffer loads that return 0 past their range,
               tiles walked with the stride of the grid.  MUTANTS are one-line faults of that data flow; the case table has to
               make every one of them fail the checker (tests/test_predictor_model.py).
CASES          the shapes the CPU and the GPU tests share, with what each has to reach."""
import functools

import numpy as np

F = np.float64
LD = np.longdouble
U = 2.0 ** -53
LEAK = 1e-17                 # build_banded refuses an operator that leaves more than this outside the band (c_api.cpp)
PRED_BW = 65                 # c_api.cpp, PRED_BW
MASKS = ("none", "all", "r05", "r30", "half", "blocks")
MUTANTS = {
    "a": "the last trip is skipped when the trip count is odd",
    "b": "k0 of the last block is off by one",
    "c": "a walked tile after the first reuses the first tile's prefetched operands",
    "d": "the batch stride of T1 uses nrf instead of nrfp",
    "e": "mask bytes of columns >= 32 are read at the u field's offset scale (o * 8 in place of o)",
}


# ---------------------------------------------------------------------------------------------------------- case table
def _case(id, H, W, batches, reaches, ws=16, ov=8, n_pass=2, pass_scale=2.0, seq=None, walks=()):
    return dict(id=id, H=H, W=W, ws=ws, ov=ov, n_pass=n_pass, pass_scale=pass_scale, batches=tuple(batches),
                seq=tuple(seq or (n_pass - 1,)), walks=tuple(walks), reaches=reaches)


# trips: n x n -> (2n + 1) x (2n + 1); K = roundup8(n) below 65 points, so the trip counts K / 8 are 1..9.  (49 is not in
# the issue's list: without it no n gives seven trips.)
TRIP_SIZES = (4, 8, 9, 16, 17, 24, 25, 33, 40, 41, 49, 57, 64, 65, 66, 72)

# walks: (batch, "rows" | "cols", stride) -- the wavefronts of that kernel take several tiles at that batch
CASES = [
    _case("rows_walk", 40, 528, (1, 3, 200, 512), "min rows; nbc = 3; batch 512 walks all three tiles, batch 200 with stride 2",
          walks=((512, "rows", 1), (200, "rows", 2))),
    _case("cols_walk", 528, 40, (1, 512), "nby = 5, nrf % 32 = 3; early-exit wavefronts in the row kernel; column kernel walks 5",
          walks=((512, "cols", 1),)),
    _case("band_tail", 40, 1040, (200,), "truncated band with k0 drift; ncc % 32 = 1; row walk 0,2,4 / 1,3",
          walks=((200, "rows", 2),)),
    _case("both_walk", 296, 296, (2, 300), "K = 40 (5 trips); both kernels walk", walks=((300, "rows", 1), (300, "cols", 1))),
    _case("band_both", 776, 776, (96,), "bands on both axes; ncc a multiple of 32; both walk with stride 2",
          walks=((96, "rows", 2), (96, "cols", 2))),
    _case("exact32", 132, 136, (5,), "nrfp == nrf; ncf % 32 = 1"),
    _case("scale15", 420, 420, (4,), "fine points not at midpoints", ws=24, ov=12, pass_scale=1.5),
] + [
    _case(f"trips_{n}", 16 + 8 * (n - 1), 16 + 8 * (n - 1), (3,), "trip counts 1..9; the 64/65/66 band boundary; clamped end rows")
    for n in TRIP_SIZES
] + [
    _case("stale_T1", 296, 296, (7,), "p = 2, then p = 1, then p = 2 on one plan", ws=32, ov=16, n_pass=3, seq=(2, 1, 2)),
]
CASE = {c["id"]: c for c in CASES}
# coarse -> fine grids the table promises (rows, columns), checked against the library's geometry by the CPU test
GRIDS = {"rows_walk": ((4, 65), (9, 131)), "cols_walk": ((65, 4), (131, 9)), "band_tail": ((4, 129), (9, 259)),
         "both_walk": ((36, 36), (73, 73)), "band_both": ((96, 96), (193, 193)), "exact32": ((15, 16), (32, 33)),
         "scale15": ((34, 34), (51, 51)), "stale_T1": ((36, 36), (73, 73))}
GRIDS.update({f"trips_{n}": ((n, n), (2 * n + 1, 2 * n + 1)) for n in TRIP_SIZES})


def max_batch(case):
    return max(case["batches"])


@functools.lru_cache(maxsize=None)
def _passes(cid):
    from torchpiv_amd import engine
    c = CASE[cid]
    out, w, o = [], c["ws"], c["ov"]
    for p in range(c["n_pass"]):
        if p:
            w, o = int(np.floor(w / c["pass_scale"])), int(np.floor(o / c["pass_scale"]))      # tpiv_plan_create's geometry loop
        nr, nc = engine.field_shape(c["H"], c["W"], w, o)
        x, y = engine.coordinates_1d(c["H"], c["W"], w, o)
        out.append((w, o, nr, nc, x, y))
    return out


def passes(case):
    """[(ws, ov, n_rows, n_cols, x, y)] of the case's plan, from the library's host geometry."""
    return _passes(case["id"])


@functools.lru_cache(maxsize=None)
def _operators(cid, p):
    from torchpiv_amd import engine
    g = _passes(cid)
    return engine.spline_matrix(g[p - 1][5], g[p][5]), engine.spline_matrix(g[p - 1][4], g[p][4])


def operators(case, p):
    """(Ay, Ax) of the predictor in front of pass p: host float64, [fine, coarse]."""
    return _operators(case["id"], p)


# -------------------------------------------------------------------------------------------------------------- inputs
def seed_of(case):
    return 7000 + [c["id"] for c in CASES].index(case["id"])


PLANTED = (64.0, -64.0, 1e-30, -1e-30)


@functools.lru_cache(maxsize=None)
def _fields(cid, p, n):
    g = _passes(cid)[p - 1]
    nrc, ncc = g[2], g[3]
    u, v = np.empty((n, nrc, ncc)), np.empty((n, nrc, ncc))
    for i in range(n):
        rng = np.random.default_rng([seed_of(CASE[cid]), p, i])
        u[i] = rng.normal(0.0, 5.0, (nrc, ncc))
        v[i] = rng.normal(0.0, 5.0, (nrc, ncc))
        at = rng.choice(nrc * ncc, size=2 * len(PLANTED), replace=False)
        u[i].flat[at[:len(PLANTED)]] = PLANTED
        v[i].flat[at[len(PLANTED):]] = PLANTED
    u.setflags(write=False)
    v.setflags(write=False)
    return u, v


def fields(case, p, n):
    """u, v [n, nrc, ncc] of the coarse pass p - 1: N(0, 5^2) with +-64 and +-1e-30 planted; pair i depends on (seed, p, i)
    alone, so a smaller batch is a prefix of a larger one."""
    return _fields(case["id"], p, n)


@functools.lru_cache(maxsize=None)
def _mask(cid, p, kind, n):
    g = _passes(cid)[p - 1]
    nrc, ncc = g[2], g[3]
    m = np.zeros((n, nrc, ncc), np.uint8)
    for i in range(n):
        rng = np.random.default_rng([seed_of(CASE[cid]), p, i, MASKS.index(kind)])
        if kind == "all":
            m[i] = 1
        elif kind in ("r05", "r30"):
            m[i] = rng.random((nrc, ncc)) < (0.05 if kind == "r05" else 0.30)
        elif kind == "half":
            m[i, :, :ncc // 2] = 1
        elif kind == "blocks":
            for _ in range(2):
                h, w = max(1, nrc // 3), max(1, ncc // 3)
                r, c = rng.integers(0, nrc - h + 1), rng.integers(0, ncc - w + 1)
                m[i, r:r + h, c:c + w] = 1
        elif kind != "none":
            raise KeyError(kind)
    m.setflags(write=False)
    return m


def mask(case, p, kind, n):
    """invalid bytes [n, nrc, ncc] of one of MASKS."""
    return _mask(case["id"], p, kind, n)


# ----------------------------------------------------------------------------------------------------------- reference
def _triple(Ay, Z, Ax):
    return np.matmul(np.matmul(Ay, Z), Ax.T)


def _bound(Ay, Ax, Z):
    """The derived error bound of one field, per cell (module docstring)."""
    aAy, aAx, aZ = np.abs(Ay), np.abs(Ax), np.abs(Z)
    nrc, ncc = Z.shape[-2:]
    S = _triple(aAy, aZ, aAx)
    full = (np.matmul(aZ, aAx.T).sum(axis=-2, keepdims=True) + np.matmul(aAy, aZ).sum(axis=-1, keepdims=True)
            + LEAK * aZ.sum(axis=(-2, -1), keepdims=True))
    return (nrc + ncc + 16) * U * S + LEAK * full


def ld_pairs(n):
    return sorted({0, n // 2, n - 1})


class Field:
    """One field's reference: float64 value and bound [n, nrf, ncf]; long double values for the pairs of ld_pairs(n)."""

    def __init__(self, Ay, Ax, Z):
        Z = np.asarray(Z, dtype=F)
        self.ref = _triple(Ay, Z, Ax)
        self.bound = _bound(Ay, Ax, Z)
        Ayl, Axl = Ay.astype(LD), Ax.astype(LD)
        self.ld = {i: _triple(Ayl, Z[i].astype(LD), Axl) for i in ld_pairs(Z.shape[0])}


def reference(mode, Ay, Ax, u, v, inv):
    """(u, v, mask) as Field: Ay @ Z @ Ax.T in float64 for Z = u, v and the mask bytes as doubles.  `mode` does not enter the
    products (it enters the hand-off, which check() applies to the kernel's own values)."""
    if mode not in ("CWS", "DWS"):
        raise KeyError(mode)
    return Field(Ay, Ax, u), Field(Ay, Ax, v), Field(Ay, Ax, np.asarray(inv, dtype=F))


class Stats:
    def __init__(self):
        self.failures = []
        self.ratio = 0.0            # largest |err| / bound over the cells whose raw predictor is visible
        self.cells = 0
        self.undecided = 0
        self.undecided_masked = 0   # of those, the kernel masked

    def __bool__(self):
        return not self.failures


def undecided(M, factor=2.0):
    """Cells in which the reference mask alone does not decide the threshold."""
    return ~(np.abs(M.ref - 0.5) > factor * M.bound)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int64)


def _rules(mode, st, tag, ru, rv, bu, bv, m, bm, factor, outs):
    u0, v0, u2, v2 = outs
    tu, tv, tm = factor * bu, factor * bv, factor * bm
    masked = m - 0.5 > tm
    clear = 0.5 - m > tm
    und = ~(masked | clear)
    zero = (u0 == 0) & (v0 == 0)
    eu, ev = np.abs(u0 - ru), np.abs(v0 - rv)
    near = (eu <= tu) & (ev <= tv)

    def fail(name, bad):
        if bad.any():
            i = tuple(int(t) for t in np.argwhere(bad)[0])
            st.failures.append(f"{tag}{name}: {int(bad.sum())} cells, first {i}: u0 {u0[i]!r} v0 {v0[i]!r} u2 {u2[i]!r} v2 {v2[i]!r}; "
                               f"raw {float(ru[i])!r} {float(rv[i])!r} mask {float(m[i])!r}; tol {float(tu[i]):.3e} "
                               f"{float(tv[i]):.3e} {float(tm[i]):.3e}")

    fail("decided masked, not zero", masked & ~zero)
    fail("decided clear, not the raw predictor", clear & ~near)
    fail("undecided, neither outcome whole", und & ~(zero | near))
    two = F(2)
    if mode == "CWS":
        kept = ~zero                                    # the kernel did not mask (or the raw predictor is exactly zero)
        fail("u2 != u0 / 2 bit for bit", kept & (_bits(u2) != _bits(u0 / two)))
        fail("v2 != v0 / 2 bit for bit", kept & (_bits(v2) != _bits(v0 / two)))
        fail("u2 of a masked cell not raw / 2", zero & ~(np.abs(u2 - ru / 2) <= tu / 2))
        fail("v2 of a masked cell not raw / 2", zero & ~(np.abs(v2 - rv / 2) <= tv / 2))
        seen = [np.abs(2 * u2 - ru) / bu, np.abs(2 * v2 - rv) / bv]
    else:
        fail("u2 != rint(u0 / 2)", ~(u2 == np.rint(u0 / two)))
        fail("v2 != rint(v0 / 2)", ~(v2 == np.rint(v0 / two)))
        seen = [np.where(zero, 0, eu / bu), np.where(zero, 0, ev / bv)]
    with np.errstate(invalid="ignore"):
        r = float(max(np.nan_to_num(np.asarray(s, dtype=F), nan=np.inf).max() for s in seen))
    st.ratio = max(st.ratio, r)
    return und, zero


def check(mode, ref, outs, first=0):
    """The decision rule on the kernel's (u0, v0, u2, v2) [b, nrf, ncf], which are the pairs first .. first + b of `ref`
    (reference()'s triple).  Returns Stats; .failures is empty where every rule holds."""
    if mode not in ("CWS", "DWS"):
        raise KeyError(mode)
    Ru, Rv, Rm = ref
    outs = [np.asarray(o, dtype=F) for o in outs]
    b = outs[0].shape[0]
    sl = slice(first, first + b)
    st = Stats()
    for o in outs:
        if o.shape != Ru.ref[sl].shape:
            st.failures.append(f"shape {o.shape} != {Ru.ref[sl].shape}")
            return st
    with np.errstate(invalid="ignore", divide="ignore"):
        und, zero = _rules(mode, st, "", Ru.ref[sl], Rv.ref[sl], Ru.bound[sl], Rv.bound[sl], Rm.ref[sl], Rm.bound[sl], 2.0, outs)
        st.cells, st.undecided, st.undecided_masked = und.size, int(und.sum()), int((und & zero).sum())
        keep = st.ratio
        for i in Ru.ld:
            if first <= i < first + b:
                k = i - first
                _rules(mode, st, f"long double pair {i}: ", Ru.ld[i], Rv.ld[i], Ru.bound[i], Rv.bound[i], Rm.ld[i], Rm.bound[i],
                       1.0, [o[k] for o in outs])
        st.ratio = max(keep, st.ratio)
    return st


# ----------------------------------------------------------------------------------------------------- the numpy model
def band_start(row, bw):
    """c_api.cpp, band_start."""
    nc = row.size
    c = int(np.argmax(np.abs(row)))                    # the first largest entry, like the `>` of the loop
    return min(max(c - bw // 2, 0), nc - bw)


def _starts(op, bw):
    """c_api.cpp, build_banded, `starts`: band starts, monotone in the fine index; the largest entry left outside."""
    st, leak = [], 0.0
    for f in range(op.shape[0]):
        s = band_start(op[f], bw)
        if f and s < st[-1]:
            s = st[-1]
        st.append(s)
        out = np.abs(np.concatenate([op[f, :s], op[f, s + bw:]]))
        if out.size:
            leak = max(leak, float(out.max()))
    return st, leak


def _tiles32(op, st, bw):
    """c_api.cpp, build_banded, `tiles32`: K, the [nb, K, 32] weight tiles, k0 per block."""
    nf = op.shape[0]
    nb = (nf + 31) // 32
    k0 = [st[32 * b] for b in range(nb)]
    K = max(st[min(32 * b + 31, nf - 1)] + bw - st[32 * b] for b in range(nb))
    K = (K + 7) // 8 * 8
    tile = np.zeros((nb, K, 32))
    for f in range(nf):
        for j in range(st[f], st[f] + bw):
            tile[f // 32, j - k0[f // 32], f % 32] = op[f, j]
    return K, tile, k0


def build_banded(Ay, Ax):
    """c_api.cpp, build_banded."""
    bwy, bwx = min(Ay.shape[1], PRED_BW), min(Ax.shape[1], PRED_BW)
    sy, ly = _starts(Ay, bwy)
    sx, lx = _starts(Ax, bwx)
    KY, Wy32, k0y = _tiles32(Ay, sy, bwy)
    KX, Ax32, k0x = _tiles32(Ax, sx, bwx)
    return dict(KY=KY, KX=KX, Wy32=Wy32, Ax32=Ax32, k0y32=k0y, k0x32=k0x, leak=max(ly, lx), bands=(bwy < Ay.shape[1], bwx < Ax.shape[1]))


def launch_shape(batch, nrc, ncc, nrf, ncf):
    """The grids of launch_predict_mfma (predict_mfma.hip:226-241) and what they mean for the walk."""
    nby, nbx, nbc = (nrf + 31) // 32, (ncf + 31) // 32, (ncc + 31) // 32           # :227

    def slices(walked, others):                                                    # :232-235
        n = 512 // (others if others > 0 else 1)
        return 1 if n < 1 else min(n, walked)

    gy, gx = (nby + 3) // 4, (nbx + 3) // 4                                        # :236
    rows = (slices(nbc, gy * batch), gy, batch)                                    # :237
    cols = (gx, slices(nby, gx * batch), batch)                                    # :240
    return dict(nby=nby, nbx=nbx, nbc=nbc, nrfp=nby * 32, rows_grid=rows, cols_grid=cols,
                rows_walk=nbc > rows[0], cols_walk=nby > cols[1],                  # :126, :177: a second tile for wavefront 0
                rows_early_exit=4 * gy > nby, cols_early_exit=4 * gx > nbx)       # :98, :152


def _gather(flat, base, off, limit):
    """A raw buffer load: element `off` of the range of `limit` elements at `base`; 0 past the range."""
    ok = off < limit
    return np.where(ok, flat[..., base + np.where(ok, off, 0)], 0.0)


def banded_raw(Ay, Ax, u, v, inv, launch_batch=None, mutant=None, T1=None):
    """The three accumulators (u, v, mask) [B, nrf, ncf] the column kernel holds before its store phase.  launch_batch: the
    batch the grids are sized for (the pairs are independent: the first B of them are computed).  T1: the plan's flat work
    buffer, to be reused between calls; a fresh one is filled with NaN, so a cell the row kernel does not write shows."""
    if mutant is not None and mutant not in MUTANTS:
        raise KeyError(mutant)
    B, nrc, ncc = u.shape
    nrf, ncf = Ay.shape[0], Ax.shape[0]
    bd = build_banded(Ay, Ax)
    assert bd["leak"] <= LEAK
    L = launch_shape(launch_batch or B, nrc, ncc, nrf, ncf)
    nrfp, KY, KX = L["nrfp"], bd["KY"], bd["KX"]
    plane, zn = ncc * nrfp, nrc * ncc
    if T1 is None:
        T1 = np.full(B * 3 * plane, np.nan)
    assert T1.size >= B * 3 * plane
    Z = [np.asarray(z, dtype=F).reshape(B, zn) for z in (u, v, inv)]
    Tv = T1[:B * 3 * plane].reshape(B, 3, ncc, nrfp)

    def k_eff(K):
        return K - 8 if mutant == "a" and (K // 8) % 2 else K

    # rows: grid (x slices, ceil(nby / 4), batch); wavefront w of a workgroup = fine block 4 y + w (:97)
    sx, gy, _ = L["rows_grid"]
    k, j = np.arange(KY)[:, None], np.arange(32)[None, :]
    for rb in range(4 * gy):
        if rb * 32 >= nrf:                                                        # :98
            continue
        k0 = bd["k0y32"][rb] + (1 if mutant == "b" and rb == L["nby"] - 1 else 0)
        W = bd["Wy32"][rb]
        for x in range(sx):
            first = None
            for n, cb in enumerate(range(x, L["nbc"], sx)):                       # :126
                cc0 = cb * 32
                o = (k0 + k) * ncc + cc0 + j                                      # :107, :116; rows >= nrc: past the range
                om = np.where(cc0 + j >= 32, o * 8, o) if mutant == "e" else o
                X = [_gather(Z[0], 0, o, zn), _gather(Z[1], 0, o, zn), _gather(Z[2], 0, om, zn)]     # [B, KY, 32]
                if first is None:
                    first = X
                elif mutant == "c":
                    X = [np.concatenate([f0[:, :8], xf[:, 8:]], axis=1) for f0, xf in zip(first, X)]
                ke = k_eff(KY)
                cc1 = min(cc0 + 32, ncc)                                          # :136
                for f in range(3):
                    acc = np.einsum("bkc,kr->bcr", X[f][:, :ke], W[:ke])          # T1t[cc][rf], :139-141
                    Tv[:, f, cc0:cc1, rb * 32:rb * 32 + 32] = acc[:, :cc1 - cc0]
    # columns: grid (ceil(nbx / 4), y slices, batch); wavefront = block of 32 fine columns (:151)
    gx, sy, _ = L["cols_grid"]
    out = np.full((B, 3, nrf, ncf), np.nan)
    k, i = np.arange(KX)[:, None], np.arange(32)[None, :]
    bstride = 3 * ncc * (nrf if mutant == "d" else nrfp)                          # :156
    for g in range(4 * gx):
        if g * 32 >= ncf:                                                         # :152
            continue
        k0 = bd["k0x32"][g] + (1 if mutant == "b" and g == L["nbx"] - 1 else 0)
        W = bd["Ax32"][g]
        cf1 = min(g * 32 + 32, ncf)                                               # :185
        for y in range(sy):
            first = None
            for n, rbk in enumerate(range(y, nrfp >> 5, sy)):                     # :177
                rf0 = rbk * 32
                to = (k0 + k) * nrfp + rf0 + i                                    # :160, :168; rows >= ncc: past the range
                X = np.stack([np.stack([_gather(T1, b * bstride + f * plane, to, plane) for f in range(3)]) for b in range(B)])
                if first is None:
                    first = X
                elif mutant == "c":
                    X = np.concatenate([first[:, :, :8], X[:, :, 8:]], axis=2)
                ke = k_eff(KX)
                acc = np.einsum("bfki,kj->bfij", X[:, :, :ke], W[:ke])
                rf1 = min(rf0 + 32, nrf)                                          # :191
                out[:, :, rf0:rf1, g * 32:cf1] = acc[:, :, :rf1 - rf0, :cf1 - g * 32]
    return out[:, 0], out[:, 1], out[:, 2]


def finish(mode, pu, pv, pm):
    """The store phase of the column kernel (predict_mfma.hip:192-218): (u0, v0, u2, v2)."""
    from handoff_model import handoff
    return handoff(mode, pu, pv, pm >= 0.5)


def banded_model(mode, Ay, Ax, u, v, inv, launch_batch=None, mutant=None, T1=None):
    """(u0, v0, u2, v2) of the banded predictor as the kernels compute it, in numpy float64."""
    return finish(mode, *banded_raw(Ay, Ax, u, v, inv, launch_batch=launch_batch, mutant=mutant, T1=T1))
