"""Numpy model of the stereo self-calibration: the triangulation of a disparity field between two cameras' lines of sight
with its status codes and fixed-order sums (include/torchpiv_hip.h: tpiv_stereo_triangulate -- every operation in the
header's order, one float64 operation each), the least-squares plane through the points, the cameras expressed in the
frame of that plane, the whole loop (trimming and stopping rule included) and its scene: tests/stereo_model.py's cameras
and renderer looking at a thin tilted sheet that does not lie where the calibration says.  Nothing here shares a line with
torchpiv_amd.engine or with the device code.

The figures of the gates (HEIGHT_LEFT, D_LEFT below; tests/test_gpu_selfcal.py has the gates) come from the CPU path on the
scene's frames -- tests/dewarp_model.py's rectification, tests/ensemble_model.py's chain, calibrate() here -- for the seeds
0, 1, 2: python tests/selfcal_model.py prints them."""
import numpy as np

import stereo_model as SM

NAN = np.float64(np.nan)
LANES = 1024


# ---- the triangulation ----------------------------------------------------------------------------------------------------
def fixed_sum(q, ok):
    """The sum of q[ok] in the device's order: lane t of 1024 sums the cells t, t + 1024, ... in ascending order from +0.0,
    then acc[t] = acc[t] + acc[t + s] for s = 512, 256, ..., 1."""
    q, ok = np.asarray(q, dtype=np.float64).reshape(-1), np.asarray(ok, dtype=bool).reshape(-1)
    acc = np.zeros(LANES)
    with np.errstate(all="ignore"):
        for lo in range(0, q.size, LANES):
            part, use = q[lo:lo + LANES], ok[lo:lo + LANES]
            acc[:part.size] = np.where(use, acc[:part.size] + part, acc[:part.size])
        s = LANES // 2
        while s >= 1:
            acc[:s] = acc[:s] + acc[s:2 * s]
            s //= 2
    return acc[0]


def triangulate(dx, dy, X, Y, C1, C2, skip=None, gap_max=np.inf, plane=None, tol=np.inf, centre=(0.0, 0.0, 0.0)):
    """{Mx, My, Mz, gap, status, count, sums} of disparities [batch, cells...] (or without the batch axis) at the cells X, Y
    [cells...]; the header's operations in the header's order."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    flat = np.ndim(dx) == X.ndim
    dx, dy = (np.asarray(q, dtype=np.float64) for q in (dx, dy))
    if flat:
        dx, dy = dx[None], dy[None]
    B = dx.shape[0]
    X, Y = X[None], Y[None]
    C1, C2 = np.asarray(C1, dtype=np.float64), np.asarray(C2, dtype=np.float64)
    c0, c1, c2 = (np.float64(q) for q in ((0.0, 0.0, 0.0) if plane is None else plane))
    Xm, Ym, Zm = (np.float64(q) for q in centre)
    zero = np.float64(0.0)
    with np.errstate(all="ignore"):
        hx = dx * 0.5
        hy = dy * 0.5
        d1 = [(X - hx) - C1[0], (Y - hy) - C1[1], zero - C1[2]]
        d2 = [(X + hx) - C2[0], (Y + hy) - C2[1], zero - C2[2]]
        w = [C1[0] - C2[0], C1[1] - C2[1], C1[2] - C2[2]]

        def dot(p, q):
            return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]
        a, b, c, d, e = dot(d1, d1), dot(d1, d2), dot(d2, d2), dot(d1, w), dot(d2, w)
        den = a * c - b * b
        s = (b * e - c * d) / den
        t = (a * e - b * d) / den
        p1 = [C1[k] + s * d1[k] for k in range(3)]
        p2 = [C2[k] + t * d2[k] for k in range(3)]
        M = [(p1[k] + p2[k]) * 0.5 for k in range(3)]
        g = [p1[k] - p2[k] for k in range(3)]
        gap = np.sqrt(dot(g, g))
        r = M[2] - ((c0 + c1 * M[0]) + c2 * M[1])
        skipped = np.zeros(X.shape, bool) if skip is None else (np.asarray(skip)[None] != 0)
        centres = bool(np.isfinite(C1).all() and np.isfinite(C2).all())
        data = np.isfinite(dx) & np.isfinite(dy)
        lines = np.isfinite(den) & (den > 0.0)
        status = np.where(skipped, 1, np.where(not centres, 3, np.where(~data, 2, np.where(~lines, 3, np.where(
            gap > np.float64(gap_max), 4, np.where(np.abs(r) > np.float64(tol), 5, 0))))))
        status = np.broadcast_to(status, dx.shape).astype(np.uint8)
        blank = (status >= 1) & (status <= 3)
        out = {"status": status, "gap": np.where(blank, NAN, np.broadcast_to(gap, dx.shape))}
        for k, name in enumerate(("Mx", "My", "Mz")):
            out[name] = np.where(blank, NAN, np.broadcast_to(M[k], dx.shape))
        ok = status == 0
        x = np.broadcast_to(M[0] - Xm, dx.shape)
        y = np.broadcast_to(M[1] - Ym, dx.shape)
        z = np.broadcast_to(M[2] - Zm, dx.shape)
        terms = (x, y, z, x * x, x * y, y * y, x * z, y * z, z * z)
        out["count"] = ok.reshape(B, -1).sum(axis=1).astype(np.int32)
        out["sums"] = np.array([[fixed_sum(q[i], ok[i]) for q in terms] for i in range(B)]).reshape(B, 9)
    if flat:
        out = {k: q[0] for k, q in out.items()}
    return out


# ---- the plane and the corrected cameras ----------------------------------------------------------------------------------
def plane(count, sums, centre=(0.0, 0.0, 0.0)):
    """(c0, c1, c2, rms) of Z = c0 + c1 X + c2 Y from the centred sums: the 3 x 3 normal equations of (1, x, y) against z in
    the centred coordinates, solved whole; ValueError for fewer than 3 points or a singular system."""
    n = int(count)
    sx, sy, sz, sxx, sxy, syy, sxz, syz, szz = (float(q) for q in np.asarray(sums).reshape(9))
    if n < 3:
        raise ValueError("fewer than 3 points")
    A = np.array([[n, sx, sy], [sx, sxx, sxy], [sy, sxy, syy]])
    spread = np.linalg.eigvalsh(np.array([[sxx - sx * sx / n, sxy - sx * sy / n], [sxy - sx * sy / n, syy - sy * sy / n]]))
    if not spread[0] > 1e-12 * spread[1]:                      # the scatter of (x, y) has one direction only
        raise ValueError("points on one line")
    k = np.linalg.solve(A, np.array([sz, sxz, syz]))
    ss = szz - k @ np.array([sz, sxz, syz])
    return (centre[2] + k[0] - k[1] * centre[0] - k[2] * centre[1], k[1], k[2], float(np.sqrt(max(ss, 0.0) / n)))


def correct(P, pl):
    """(P_new, T): T takes the new world frame -- z along the plane's normal, x the old X axis projected into the plane, the
    origin at (0, 0, c0) -- to the old one; P_new = P T."""
    c0, c1, c2 = pl
    nz = np.array([-c1, -c2, 1.0]) / np.sqrt(c1 * c1 + c2 * c2 + 1.0)
    ey = np.cross(nz, np.array([1.0, 0.0, 0.0]))               # n x X = n x (X's in-plane part): the y axis comes first here
    ey = ey / np.linalg.norm(ey)
    ex = np.cross(ey, nz)
    T = np.zeros((4, 4))
    T[:3, :3] = np.column_stack([ex, ey, nz])
    T[:, 3] = (0.0, 0.0, c0, 1.0)
    return P @ T, T


def calibrate(measure, P, X, Y, free, iterations=4, tol=0.05 * SM.SCALE, trim=3.0):
    """The loop of StereoPIV.self_calibrate: measure(P1, P2) -> (dx, dy, skip) on the cells X, Y (free: the non-excluded
    ones).  Returns (P, T, rounds, converged), rounds = [(plane, rms, count, height, median gap, median |d|)]."""
    T, rounds, converged = np.eye(4), [], False
    centre = (float(X.mean()), float(Y.mean()), 0.0)
    for _ in range(iterations):
        dx, dy, skip = measure(*P)
        C1, C2 = SM.centre(P[0]), SM.centre(P[1])
        first = triangulate(dx, dy, X, Y, C1, C2, skip=skip, centre=centre)
        count = int(first["count"])
        c0, c1, c2, rms = plane(count, first["sums"], centre)
        for _ in range(2):
            rec = triangulate(dx, dy, X, Y, C1, C2, skip=skip, plane=(c0, c1, c2), tol=trim * rms, centre=centre)
            if int(rec["count"]) == count:
                break
            count = int(rec["count"])
            c0, c1, c2, rms = plane(count, rec["sums"], centre)
        height = float(np.abs(c0 + c1 * X + c2 * Y)[free].max())
        rounds.append(((c0, c1, c2), rms, count, height, float(np.median(first["gap"][first["status"] == 0])),
                       float(np.median(np.hypot(dx, dy)[free])), int(first["count"])))
        (P1, T1), (P2, _) = correct(P[0], (c0, c1, c2)), correct(P[1], (c0, c1, c2))
        P, T = (P1, P2), T @ T1
        if height <= tol:
            converged = True
            break
    return P, T, rounds, converged


# ---- the scene --------------------------------------------------------------------------------------------------------------
SHEET = (0.5, 0.02, -0.015)                              # z = 0.5 + 0.02 X - 0.015 Y mm: where the light sheet really lies
THICKNESS, PAIRS = 0.1, 6
WS, OV = 32, 16


def sheet(X, Y):
    return SHEET[0] + SHEET[1] * np.asarray(X, float) + SHEET[2] * np.asarray(Y, float)


def scene(seed=0, pairs=PAIRS, frame_b=False):
    """(A1, A2): uint8 [pairs, H, W], frame a of both cameras (stereo_model's cameras and renderer): about 1700 particles
    per pair, uniform over a region that covers both fields of view and over the sheet's thickness about sheet(X, Y).
    frame_b: (A1, B1, A2, B2) -- the same frames a, and frames b that show the particles moved by stereo_model's flow(), with
    stereo_model's hole in each camera (weak noise from a generator of its own, so the frames a do not depend on it)."""
    rng, noise = np.random.default_rng(seed), np.random.default_rng(1000 + seed)
    cams = SM.cameras()
    out = [np.empty((pairs, SM.H, SM.W), np.uint8) for _ in range(4 if frame_b else 2)]
    step = 2 if frame_b else 1
    for k in range(pairs):
        n = 1700
        X, Y = rng.uniform(-11.5, 11.5, n), rng.uniform(-8.5, 8.5, n)
        Z = sheet(X, Y) + rng.uniform(-0.5, 0.5, n) * THICKNESS
        amp = rng.uniform(100, 200, n)
        for c, P in enumerate(cams):
            out[step * c][k] = SM.render(*SM.project(P, X, Y, Z), amp)
            if frame_b:
                dX, dY, dZ = SM.flow(X, Y)
                out[2 * c + 1][k] = SM.render(*SM.project(P, X + dX, Y + dY, Z + dZ), amp)
                y0, y1, x0, x1 = SM.window_in_camera(P, *SM.HOLES[c])
                out[2 * c + 1][k][y0:y1, x0:x1] = noise.integers(0, 17, (y1 - y0, x1 - x0)).astype(np.uint8)
    return tuple(out)


def cells(x, y):
    """World positions of the cells of the delivered fields: x, y the window centres as get_coordinates returns them."""
    nr = x.shape[0]
    return SM.ORIGIN[0] + SM.SCALE * x, SM.ORIGIN[1] - SM.SCALE * y[nr - 1 - np.arange(nr)]


def sheet_height(T, X, Y, free):
    """max |z| over the free cells of the TRUE sheet's points above (X, Y), expressed in the frame T leads out of."""
    old = np.stack([X[free], Y[free], sheet(X[free], Y[free]), np.ones(int(free.sum()))])
    return float(np.abs((np.linalg.inv(T) @ old)[2]).max())


# the gates' figures: scene(seed) through the CPU path (module docstring) at 32/16, one pass, tol = 0.05 SCALE, trim = 3,
# iterations = 4; then one more disparity measurement with the corrected cameras
#   seed 0: three rounds, sheet height left 0.001685 mm, median |d| left 0.002723 mm; measured heights 0.688 -> 0.0104 -> 0.0019
#   seed 1: three rounds, sheet height left 0.000557 mm, median |d| left 0.002540 mm;                  0.688 -> 0.0117 -> 0.0019
#   seed 2: three rounds, sheet height left 0.002699 mm, median |d| left 0.002940 mm;                  0.685 -> 0.0118 -> 0.0022
# (round 1 stops 2 % short of c0 = 0.5: the passes' bias towards zero of a 6.4 px displacement, stereo_model's
# DISPARITY_DEVIATION.)  The conditions: every seed converges within iterations = 4 -- in three disparity measurements -- and
# every one of the 63 cells is valid in every measurement (63 status-0 cells before trimming, all rounds, all seeds).  The
# trim itself leaves out ONE cell in rounds 2 and 3 of seed 2 (|r| just above 3 rms with rms = 0.0019 mm: among 63 Gaussian
# residuals that happens in one round of six, whatever the plane), so the sheet stays as the feature's definition gives it.
# HEIGHT_LEFT, D_LEFT: the worst of the three seeds.
HEIGHT_LEFT = 0.002699
D_LEFT = 0.002940


def cpu_path(seed):
    """(rounds, converged, the true sheet's remaining max height in mm, the remaining median |d| in mm, cells used)."""
    import dewarp_model as D
    import ensemble_model as E
    from oracle import piv_oracle as O
    A1, A2 = scene(seed)
    xs, ys = O.coordinates((SM.H, SM.W), WS, OV)
    X, Y = cells(xs, ys)

    def measure(P1, P2):
        rect = [D.dewarp(A, D.quantize(*D.homography_coords(SM.homography(P, SM.SCALE, SM.ORIGIN), SM.H, SM.W), SM.H, SM.W))
                for A, P in ((A1, P1), (A2, P2))]
        u, v, inv = E.chain(rect[0], rect[1], WS, OV, 1, "CWS")[-1]
        return np.flip(u, axis=0) * SM.SCALE, -np.flip(v, axis=0) * SM.SCALE, np.flip(inv, axis=0).astype(np.uint8)
    free = np.ones(X.shape, bool)
    P, T, rounds, converged = calibrate(measure, SM.cameras(), X, Y, free)
    dx, dy, skip = measure(*P)
    return rounds, converged, sheet_height(T, X, Y, free), float(np.median(np.hypot(dx, dy)[skip == 0])), rounds[-1][2]


if __name__ == "__main__":
    for seed in (0, 1, 2):
        rounds, converged, height, d, used = cpu_path(seed)
        print(f"seed {seed}: converged {converged} after {len(rounds)} rounds, {used} cells, sheet height left {height:.6f} mm, "
              f"median |d| left {d:.6f} mm")
        for pl, rms, count, h, gap, dd, valid in rounds:
            print(f"    plane ({pl[0]:+.5f}, {pl[1]:+.6f}, {pl[2]:+.6f}) rms {rms:.5f} count {count} of {valid} height {h:.5f} "
                  f"gap {gap:.5f} |d| {dd:.5f}")
