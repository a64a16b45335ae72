"""The local least-squares fit of include/torchpiv_hip.h (tpiv_field_fit) and the quantities of engine.derive in plain numpy
float64, operation by operation -- the yardstick of the device kernel (the reference has no such operator).

Per cell (R, C): S = the data cells (skip byte 0, u and v finite) at offsets |i|, |j| <= radius inside the grid; the basis
1, i, j, i*i, i*j, j*j on the integer offsets (i: columns, j: rows); moments in integers; right-hand sides b[q] = b[q] +
w * phi_q, one product and one add per data cell in row-major order; LDL^T without pivoting with the pivot test d[k] > 2^-30 *
M[k][k]; back substitution; the ladder quadratic -> linear (the shared leading block) -> mean -> nothing.  numpy's
elementwise float64 operations are single IEEE operations, so every array expression below is one operation per cell, the
cells side by side; a cell that takes no part in a step keeps its value through np.where, as the device's select does.
"""
import numpy as np

EXP = ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2))       # (power of i, power of j) of the basis functions
PIVOT_TOL = 2.0 ** -30
QUANTITIES = ("dudx", "dudy", "dvdx", "dvdy", "vorticity", "divergence", "shear", "q", "swirl", "u_smooth", "v_smooth")


def _shifted(a, j, i, fill):
    """b[..., r, c] = a[..., r + j, c + i], `fill` outside the grid."""
    R, C = a.shape[-2:]
    out = np.full(a.shape, fill, dtype=a.dtype)
    rs, re = max(0, -j), min(R, R - j)
    cs, ce = max(0, -i), min(C, C - i)
    if rs < re and cs < ce:
        out[..., rs:re, cs:ce] = a[..., rs + j:re + j, cs + i:ce + i]
    return out


def data_cells(u, v, skip=None):
    ok = np.isfinite(u) & np.isfinite(v)
    return ok if skip is None else ok & (np.asarray(skip) == 0)


def field_fit(u, v, skip=None, radius=2, order=2, want_pivots=False):
    """u, v float64 [batch, R, C] or [R, C]; skip uint8 / bool of that shape or None.  Returns (fit [6, ...], count uint8,
    order int8); want_pivots adds (d [n, ...], M_kk [n, ...]), the pivots and the original diagonal."""
    u = np.asarray(u, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    ok = data_cells(u, v, skip)
    n = 6 if order == 2 else 3
    deg = 2 * order
    shape = u.shape
    mom = {(a, b): np.zeros(shape, np.int32) for a in range(deg + 1) for b in range(deg + 1 - a)}
    bu = [np.zeros(shape) for _ in range(n)]
    bv = [np.zeros(shape) for _ in range(n)]
    with np.errstate(all="ignore"):
        for j in range(-radius, radius + 1):
            for i in range(-radius, radius + 1):
                m = _shifted(ok, j, i, False)
                wu, wv = _shifted(u, j, i, np.nan), _shifted(v, j, i, np.nan)
                for (a, b) in mom:
                    mom[a, b] += np.where(m, np.int32(i ** a * j ** b), np.int32(0))
                for q, (a, b) in enumerate(EXP[:n]):
                    f = np.float64(i ** a * j ** b)
                    bu[q] = np.where(m, bu[q] + wu * f, bu[q])
                    bv[q] = np.where(m, bv[q] + wv * f, bv[q])
        count = mom[0, 0]
        sum_u, sum_v = bu[0], bv[0]
        A = [[mom[EXP[q][0] + EXP[s][0], EXP[q][1] + EXP[s][1]].astype(np.float64) if s <= q else None for s in range(n)]
             for q in range(n)]
        m0 = [A[q][q] for q in range(n)]
        L = [[None] * n for _ in range(n)]
        d = [None] * n
        acc = np.ones(shape, bool)
        accs = []
        for k in range(n):
            d[k] = A[k][k]
            acc = acc & (d[k] > np.float64(PIVOT_TOL) * m0[k])
            accs.append(acc)
            for q in range(k + 1, n):
                l = A[q][k] / d[k]
                for s in range(k + 1, q + 1):
                    A[q][s] = A[q][s] - l * A[s][k]
                bu[q] = bu[q] - l * bu[k]
                bv[q] = bv[q] - l * bv[k]
                L[q][k] = l
        yu = [bu[k] / d[k] for k in range(n)]
        yv = [bv[k] / d[k] for k in range(n)]

        def back(y, m):
            c = [None] * m
            for k in range(m - 1, -1, -1):
                t = y[k]
                for q in range(k + 1, m):
                    t = t - L[q][k] * c[q]
                c[k] = t
            return c
        lin_u, lin_v = back(yu, 3), back(yv, 3)
        acc3 = accs[2]
        fitted = np.where(acc3, 1, np.where(count >= 1, 0, -1)).astype(np.int8)
        cu, cv = lin_u, lin_v
        if order == 2:
            acc6 = accs[5]
            qu, qv = back(yu, 6), back(yv, 6)
            cu = [np.where(acc6, qu[k], lin_u[k]) for k in range(3)]
            cv = [np.where(acc6, qv[k], lin_v[k]) for k in range(3)]
            fitted = np.where(acc6, np.int8(2), fitted).astype(np.int8)
        cnt = count.astype(np.float64)
        mean_u, mean_v = sum_u / cnt, sum_v / cnt
    low, none = fitted <= 0, fitted < 0
    nan = np.float64(np.nan)
    fit = np.empty((6,) + shape)
    for base, c, mean in ((0, cu, mean_u), (3, cv, mean_v)):
        fit[base] = np.where(none, nan, np.where(low, mean, c[0]))
        fit[base + 1] = np.where(low, nan, c[1])
        fit[base + 2] = np.where(low, nan, c[2])
    if want_pivots:
        return fit, count.astype(np.uint8), fitted, (np.stack(d), np.stack(m0))
    return fit, count.astype(np.uint8), fitted


def moment_matrix(valid, radius, n=6):
    """The exact integer normal matrix (n x n, int64) of one (2 radius + 1)^2 validity pattern (bool, row-major)."""
    valid = np.asarray(valid, bool).reshape(2 * radius + 1, 2 * radius + 1)
    jj, ii = np.nonzero(valid)
    ii, jj = ii.astype(np.int64) - radius, jj.astype(np.int64) - radius
    P = np.stack([ii ** a * jj ** b for a, b in EXP[:n]], axis=1) if ii.size else np.zeros((0, n), np.int64)
    return P.T @ P


def ladder(valid, radius, order):
    """The order the ladder picks for one validity pattern, from the rank of the exact integer moment matrices."""
    M = moment_matrix(valid, radius)
    if order == 2 and np.linalg.matrix_rank(M.astype(np.float64)) == 6:
        return 2
    if np.linalg.matrix_rank(M[:3, :3].astype(np.float64)) == 3:
        return 1
    return 0 if np.asarray(valid).any() else -1


def derive(fit, hx, hy, quantities=QUANTITIES):
    """{name: float64 array} from the planes U, Ux, Uy, V, Vx, Vy; hx, hy: the signed grid steps in millimetres.  Every
    expression left to right as written, one numpy operation each."""
    U, Ux, Uy, V, Vx, Vy = (np.asarray(f, dtype=np.float64) for f in fit)
    sx, sy = np.float64(hx) / np.float64(1000), np.float64(hy) / np.float64(1000)
    with np.errstate(all="ignore"):
        dudx, dudy, dvdx, dvdy = Ux / sx, Uy / sy, Vx / sx, Vy / sy
        out = {"dudx": dudx, "dudy": dudy, "dvdx": dvdx, "dvdy": dvdy, "u_smooth": U, "v_smooth": V,
               "vorticity": dvdx - dudy, "divergence": dudx + dvdy, "shear": dvdx + dudy,
               "q": np.float64(-0.5) * (dudx * dudx + np.float64(2) * dudy * dvdx + dvdy * dvdy)}
        s = dudx + dvdy
        disc = dudx * dvdy - dudy * dvdx - np.float64(0.25) * (s * s)
        out["swirl"] = np.sqrt(np.where(disc < 0, np.float64(0), disc))     # (a NaN discriminant stays NaN)
    return {k: out[k] for k in quantities}
