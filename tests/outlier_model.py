"""The normalized median test (Westerweel & Scarano, Exp. Fluids 39, 2005) as include/torchpiv_hip.h defines it for
tpiv_median_test, in plain numpy float64 -- the yardstick of the device kernel (the reference has no such test).

Per cell: N = the up to eight cells around it inside the grid with invalid == 0, k = |N|; the cell's own mask byte
plays no part.  k < min_neighbours: not flagged, medians = the cell's own values.  Otherwise per component w:
    s = the k neighbour values sorted (the order of <, -0.0 before +0.0: ties leave no choice of bit pattern);
    med = s[(k-1)/2] for odd k, (s[k/2-1] + s[k/2]) * 0.5 for even k;
    rmed = the same pick from the sorted residuals |w_i - med|;
    out_w = |w_centre - med| > threshold * (rmed + eps).
Every operation is one IEEE float64 operation in the order written, so a device that does the same gives the same bits.
Explicit sorts and picks -- not np.median / np.nanmedian, whose order of operations is their own.
"""
import numpy as np

_LOW63 = np.int64(0x7fffffffffffffff)


def _sorted_values(w):
    """The values of the 1-D float64 array w in ascending order with -0.0 before +0.0: sorted as the signed integers
    whose order is that of the doubles (negative doubles: the low 63 bits inverted), then mapped back."""
    b = np.ascontiguousarray(w, dtype=np.float64).view(np.int64)
    key = np.sort(b ^ ((b >> np.int64(63)) & _LOW63), kind="stable")
    return (key ^ ((key >> np.int64(63)) & _LOW63)).view(np.float64)


def _pick(s):
    k = s.size
    if k % 2:
        return s[(k - 1) // 2]
    return (s[k // 2 - 1] + s[k // 2]) * np.float64(0.5)


def median_test(u, v, invalid, threshold=2.0, eps=0.1, min_neighbours=3):
    """u, v float64 and invalid uint8 / bool, [batch, R, C] or [R, C].  Returns (status uint8, med_u, med_v float64) of the
    same shape: status bit 0 = flagged, bit 1 = invalid on input."""
    u = np.asarray(u, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    inv = np.asarray(invalid) != 0
    if u.ndim == 2:
        s, mu, mv = median_test(u[None], v[None], inv[None], threshold, eps, min_neighbours)
        return s[0], mu[0], mv[0]
    thr, eps = np.float64(threshold), np.float64(eps)
    B, R, C = u.shape
    status = (inv.astype(np.uint8) << 1).astype(np.uint8)
    med = [u.copy(), v.copy()]
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            for r in range(R):
                for c in range(C):
                    nb = [(r + dr, c + dc) for dr in (-1, 0, 1) for dc in (-1, 0, 1)
                          if (dr or dc) and 0 <= r + dr < R and 0 <= c + dc < C and not inv[b, r + dr, c + dc]]
                    if len(nb) < min_neighbours:
                        continue
                    rr, cc = np.array(nb).T
                    flag = False
                    for w, m in ((u, med[0]), (v, med[1])):
                        s = _sorted_values(w[b, rr, cc])
                        mid = _pick(s)
                        rmed = _pick(_sorted_values(np.abs(s - mid)))
                        m[b, r, c] = mid
                        flag |= bool(np.abs(w[b, r, c] - mid) > thr * (rmed + eps))
                    status[b, r, c] |= np.uint8(flag)
    return status, med[0], med[1]


def replaced(u, v, status, med_u, med_v):
    """What a plan leaves of a pass before the last: flagged cells at their medians, every other cell as it was."""
    f = (np.asarray(status) & 1) != 0
    return np.where(f, med_u, u), np.where(f, med_v, v)
