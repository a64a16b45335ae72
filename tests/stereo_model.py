"""Numpy model of the stereoscopic reconstruction (torchpiv_amd/csrc/stereo.hip, include/torchpiv_hip.h:
tpiv_stereo_reconstruct) and of the camera geometry of engine.stereo_*: the pinhole, its centre, the backward homography,
the viewing tangents, the reconstruction with its status codes and per-pair summary -- every operation in the header's
order, one float64 operation each -- and a synthetic scene: two pinhole cameras at +35 and -30 degrees about the Y axis,
500 mm from a thin sheet of Gaussian particles that move by a prescribed (dX, dY, dZ)(X, Y) with dZ comparable to dX.
Nothing here shares a line with torchpiv_amd.engine or with the device code.

The physics figures of the scene (PHYSICS_RMS below; tests/test_gpu_stereo.py has the gate) come from the CPU path on the
scene's frames -- tests/dewarp_model.py's rectification, oracle/piv_oracle.py's passes and post-validation, reconstruct()
here -- for the seeds 0, 1, 2: see PHYSICS_RMS."""
import numpy as np

NAN = np.float64(np.nan)


# ---- geometry ---------------------------------------------------------------------------------------------------------
def pinhole(theta_deg, distance=500.0, focal_px=5000.0, centre_px=(79.5, 63.5)):
    """P [3, 4] of a pinhole that looks at the world origin from `distance` mm, turned by theta about the Y axis: image x
    to the right, image y down, (x, y, 1) ~ P (X, Y, Z, 1); P[2] . (X, Y, Z, 1) is the depth in mm."""
    t = np.deg2rad(theta_deg)
    C = distance * np.array([np.sin(t), 0.0, np.cos(t)])
    R = np.array([[np.cos(t), 0.0, -np.sin(t)], [0.0, -1.0, 0.0], [-np.sin(t), 0.0, -np.cos(t)]])
    K = np.array([[focal_px, 0.0, centre_px[0]], [0.0, focal_px, centre_px[1]], [0.0, 0.0, 1.0]])
    return K @ np.column_stack([R, -R @ C])


def project(P, X, Y, Z):
    """Camera pixels (x, y) of world points, the exact pinhole."""
    X, Y, Z = np.broadcast_arrays(np.asarray(X, float), np.asarray(Y, float), np.asarray(Z, float))
    h = P[:, 0, None] * X.ravel() + P[:, 1, None] * Y.ravel() + P[:, 2, None] * Z.ravel() + P[:, 3, None]
    return (h[0] / h[2]).reshape(X.shape), (h[1] / h[2]).reshape(X.shape)


def centre(P):
    return -np.linalg.inv(P[:, :3]) @ P[:, 3]


def homography(P, scale, origin=(0.0, 0.0)):
    """Rectified pixel (x, y, 1) -> camera pixel: pixel (x, y) is the world point (X0 + p x, Y0 - p y, 0)."""
    S = np.array([[scale, 0.0, origin[0]], [0.0, -scale, origin[1]], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    return P @ S


def rectified(P, scale, origin, X, Y, Z):
    """Where camera P's rectification puts the world point (X, Y, Z), in rectified pixels: the camera pixel taken back to
    the plane z = 0 along the line of sight."""
    C = centre(P)
    X, Y, Z = (np.asarray(q, float) for q in (X, Y, Z))
    s = C[2] / (C[2] - Z)                                  # the sight line from C through the point meets z = 0 here
    X0, Y0 = C[0] + (X - C[0]) * s, C[1] + (Y - C[1]) * s
    return (X0 - origin[0]) / scale, (origin[1] - Y0) / scale


def tangents(P, X, Y):
    C = centre(P)
    return (np.asarray(X, float) - C[0]) / C[2], (np.asarray(Y, float) - C[1]) / C[2]


def planes(P, x, y, scale, origin):
    """Tangent planes in the orientation of the delivered fields: cell [r, c] <- window centre (x[r, c], y[nr - 1 - r, c])."""
    nr = x.shape[0]
    yy = y[nr - 1 - np.arange(nr)]
    a, b = tangents(P, origin[0] + scale * x, origin[1] - scale * yy)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


# ---- the reconstruction -------------------------------------------------------------------------------------------------
def reconstruct(u1, v1, u2, v2, a1, b1, a2, b2, sigma=None, skip=None, fill=0.0):
    """{U, V, W, res, status, pair_rms, pair_count[, sU, sV, sW]} of fields [batch, cells...] (or without the batch axis)
    and tangent planes [cells...]; the header's operations in the header's order."""
    flat = np.ndim(u1) == np.ndim(a1)
    f = [np.asarray(q, dtype=np.float64) for q in (u1, v1, u2, v2)]
    if flat:
        f = [q[None] for q in f]
    u1, v1, u2, v2 = f
    a1, b1, a2, b2 = (np.asarray(q, dtype=np.float64)[None] for q in (a1, b1, a2, b2))
    B = u1.shape[0]
    with np.errstate(all="ignore"):
        du = u1 - u2
        dv = v1 - v2
        da = a1 - a2
        db = b1 - b2
        da2 = da * da
        db2 = db * db
        g = da2 + db2
        W = (da * du + db * dv) / g
        U = ((u1 + u2) - (a1 + a2) * W) * 0.5
        V = ((v1 + v2) - (b1 + b2) * W) * 0.5
        eu = du - da * W
        ev = dv - db * W
        res = np.sqrt((eu * eu + ev * ev) * 0.5)
        geo = np.isfinite(a1) & np.isfinite(b1) & np.isfinite(a2) & np.isfinite(b2) & (g != 0.0)
        data = np.isfinite(u1) & np.isfinite(v1) & np.isfinite(u2) & np.isfinite(v2)
        skipped = np.zeros(a1.shape, bool) if skip is None else (np.asarray(skip)[None] != 0)
        status = np.where(skipped, 1, np.where(~geo, 3, np.where(~data, 2, 0))).astype(np.uint8)
        status = np.broadcast_to(status, u1.shape).copy()
        ok = status == 0
        blank = np.where(status == 1, np.float64(fill), NAN)
        out = {"U": np.where(ok, U, blank), "V": np.where(ok, V, blank), "W": np.where(ok, W, blank),
               "res": np.where(ok, res, NAN), "status": status}
        if sigma is not None:
            s = [np.asarray(q, dtype=np.float64) for q in sigma]
            su1, sv1, su2, sv2 = (q[None] for q in s) if flat else s
            q1 = su1 * su1
            q2 = su2 * su2
            r1 = sv1 * sv1
            r2 = sv2 * sv2
            qs = q1 + q2
            rs = r1 + r2
            sW = np.sqrt((da2 * qs + db2 * rs) / (g * g))
            ma = (a1 + a2) * 0.5
            mb = (b1 + b2) * 0.5
            ka = ma * da / g
            kb = ma * db / g
            la = mb * db / g
            lb = mb * da / g
            cu1 = 0.5 - ka
            cu2 = 0.5 + ka
            cv1 = 0.5 - la
            cv2 = 0.5 + la
            sU = np.sqrt((cu1 * cu1) * q1 + (cu2 * cu2) * q2 + (kb * kb) * rs)
            sV = np.sqrt((cv1 * cv1) * r1 + (cv2 * cv2) * r2 + (lb * lb) * qs)
            oks = ok & np.isfinite(su1) & np.isfinite(sv1) & np.isfinite(su2) & np.isfinite(sv2)
            out.update(sU=np.where(oks, sU, NAN), sV=np.where(oks, sV, NAN), sW=np.where(oks, sW, NAN))
        count = ok.reshape(B, -1).sum(axis=1).astype(np.int32)
        r2sum = np.array([float(np.sum(np.square(out["res"][k][ok[k]]))) for k in range(B)])
        out["pair_count"] = count
        out["pair_rms"] = np.where(count > 0, np.sqrt(r2sum / np.maximum(count, 1)), NAN)
    if flat:
        out = {k: q[0] for k, q in out.items()}
    return out


def lstsq(u1, v1, u2, v2, a1, b1, a2, b2):
    """(U, V, W, res) of ONE cell from numpy.linalg.lstsq on the 4 x 3 system; res = the root of the summed squared residuals."""
    A = np.array([[1.0, 0.0, a1], [0.0, 1.0, b1], [1.0, 0.0, a2], [0.0, 1.0, b2]])
    y = np.array([u1, v1, u2, v2])
    x = np.linalg.lstsq(A, y, rcond=None)[0]
    return x[0], x[1], x[2], float(np.sqrt(((A @ x - y) ** 2).sum()))


# ---- the scene ----------------------------------------------------------------------------------------------------------
H, W = 128, 160
SCALE = 0.1                                              # mm per rectified pixel
ORIGIN = (-SCALE * (W - 1) / 2.0, SCALE * (H - 1) / 2.0)  # the frame centre is the world origin
ANGLES = (35.0, -30.0)
# rms errors of (U, V, W) in the delivered unit (scale / dt * 1000 with dt = 1: micrometres per frame) over the non-excluded
# cells of all six pairs, CPU path (module docstring), 32/16 one pass, seeds 0, 1, 2 -- and camera 1's own u against U
#   seed 0: 12.836  8.232  9.772   (6 pairs, 63 cells each; camera 1's u - U: 185.8)
#   seed 1: 12.180  8.733  9.406   (5 pairs: one is dropped by camera 2 for having no invalid vector; 184.9)
#   seed 2: 12.605  8.523 10.439   (6 pairs; 185.9)
# The mean errors, (-11.1, +6.5, -1.1) at seed 0, are the passes' own bias towards zero of a 3 px displacement in a 32 px
# top-hat window (-3.7 % of (3, -1.5) px); W is free of it to first order.  PHYSICS_RMS: the worst of the three per component.
PHYSICS_RMS = (12.836, 8.733, 10.439)
# the disparity check: scene(seed, z0=0.5, thickness=0.1, holes=False), frame a of camera 1 against frame a of camera 2, CPU
# path (dewarp_model's rectification, ensemble_model.chain at 32/16, one pass): the median dx over the 63 cells minus the
# median of (a2 - a1) z0 = 0.63878 mm is -0.01136, -0.01195, -0.01214 mm at the seeds 0, 1, 2 (the bias towards zero of a 6.4 px
# displacement; at z0 = -0.3 it is +0.0102 ... +0.0124), the median dy within 0.0005 mm of (b2 - b1) z0 = 0.000003
DISPARITY_Z0, DISPARITY_THICKNESS, DISPARITY_DEVIATION = 0.5, 0.1, 0.01214


def cameras():
    return pinhole(ANGLES[0]), pinhole(ANGLES[1])


def flow(X, Y):
    """The prescribed displacement (dX, dY, dZ) in mm of a particle at (X, Y): about (3, -1.5, 2.5) rectified pixels."""
    X, Y = np.asarray(X, float), np.asarray(Y, float)
    return 0.30 + 0.004 * Y, -0.15 + 0.003 * X, 0.25 + 0.005 * X + 0.0 * Y


def render(px, py, amp, sigma=1.0):
    img = np.zeros((H, W))
    cx, cy = np.rint(px).astype(int), np.rint(py).astype(int)
    for oy in range(-3, 4):
        for ox in range(-3, 4):
            xx, yy = cx + ox, cy + oy
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            w = amp * np.exp(-((xx - px) ** 2 + (yy - py) ** 2) / (2 * sigma * sigma))
            np.add.at(img, (yy[ok], xx[ok]), w[ok])
    return np.clip(np.rint(img + 8.0), 0, 255).astype(np.uint8)


def window_in_camera(P, row, col, ws=32, step=16):
    """(y0, y1, x0, x1): the camera pixels that hold window (row, col) of the rectified (ws, step) grid, one pixel of
    margin included."""
    Hm = homography(P, SCALE, ORIGIN)
    xs = np.array([col * step - 1.0, col * step + ws, col * step - 1.0, col * step + ws])
    ys = np.array([row * step - 1.0, row * step - 1.0, row * step + ws, row * step + ws])
    d = Hm[2, 0] * xs + Hm[2, 1] * ys + Hm[2, 2]
    cx, cy = (Hm[0, 0] * xs + Hm[0, 1] * ys + Hm[0, 2]) / d, (Hm[1, 0] * xs + Hm[1, 1] * ys + Hm[1, 2]) / d
    return (max(int(np.floor(cy.min())), 0), min(int(np.ceil(cy.max())) + 1, H),
            max(int(np.floor(cx.min())), 0), min(int(np.ceil(cx.max())) + 1, W))


HOLES = ((3, 3), (3, 5))                                 # the window of the 32/16 grid that each camera loses (row, col)


def scene(seed=0, pairs=6, z0=0.0, thickness=1.0, holes=True):
    """(A1, B1, A2, B2): uint8 [pairs, H, W] as the two cameras see them.  Per pair about 1500 particles uniform over a
    world region that covers both fields of view and over the sheet z0 +- thickness / 2; frame b shows them moved by
    flow().  holes: in every frame b the camera pixels of ONE window of the rectified 32/16 grid (HOLES) show weak noise
    instead of particles: that window fails the peak ratio, its neighbours keep half their particles and pass, so no
    pair is dropped for having no invalid vector (nor for too many)."""
    rng = np.random.default_rng(seed)
    cams = cameras()
    out = [np.empty((pairs, H, W), np.uint8) for _ in range(4)]
    for k in range(pairs):
        n = 1700
        X, Y = rng.uniform(-11.5, 11.5, n), rng.uniform(-8.5, 8.5, n)
        Z = z0 + rng.uniform(-0.5, 0.5, n) * thickness
        amp = rng.uniform(100, 200, n)
        dX, dY, dZ = flow(X, Y)
        for c, P in enumerate(cams):
            out[2 * c][k] = render(*project(P, X, Y, Z), amp)
            out[2 * c + 1][k] = render(*project(P, X + dX, Y + dY, Z + dZ), amp)
            if holes:
                y0, y1, x0, x1 = window_in_camera(P, *HOLES[c])
                out[2 * c + 1][k][y0:y1, x0:x1] = rng.integers(0, 17, (y1 - y0, x1 - x0)).astype(np.uint8)
    return tuple(out)


def truth(x, y):
    """(U, V, W) of the prescribed flow at the cells of the delivered fields, in mm: x, y the window-centre pixels as
    get_coordinates returns them."""
    nr = x.shape[0]
    yy = y[nr - 1 - np.arange(nr)]
    return flow(ORIGIN[0] + SCALE * x, ORIGIN[1] - SCALE * yy)
