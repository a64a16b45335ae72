"""The numpy model of tracks(): particle detection and matching exactly as include/torchpiv_hip.h defines them
(tpiv_particle_count / _detect / _match), operation for operation in float64, and a small renderer of particle images at known
positions.  The device must give the same bits (tests/test_gpu_tracks.py); the properties of the model itself are
tests/test_tracks_host.py's."""
import numpy as np

NAN_BITS = 0x7FF8000000000000
NAN = np.array([NAN_BITS], dtype=np.uint64).view(np.float64)[0]
MATCHED, NO_CANDIDATE, LOST_CLAIM, OUTSIDE, NO_PARTICLE = 0, 1, 2, 3, 255

BEFORE = ((-1, -1), (-1, 0), (-1, 1), (0, -1))      # the 8-neighbours that precede a pixel in raster order: I > them
BEHIND = ((0, 1), (1, -1), (1, 0), (1, 1))          # and those that follow: I >= them


def table():
    """ln(max(i, 1)), float64 [256]: the host table both the device and the model read."""
    return np.log(np.maximum(np.arange(256), 1).astype(np.float64))


def _subpixel(L, C, R):
    den = (L - 2.0 * C) + R
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den < 0.0, (L - R) / (2.0 * den), 0.0)


def detect(frames, level, mask=None, tab=None):
    """Particle images of frames uint8 [n, H, W]: a list per frame of (x float64, y float64, peak uint8) in raster order of
    the peak pixel, with row_start int32 [n, H + 1] and count int32 [n]."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 3
    n, H, W = frames.shape
    if H < 3 or W < 3:
        raise ValueError("frames of at least 3 x 3 pixels")
    tab = table() if tab is None else tab
    f = frames.astype(np.int32)
    I = f[:, 1:H - 1, 1:W - 1]
    ok = I >= level
    for dr, dc in BEFORE:
        ok &= I > f[:, 1 + dr:H - 1 + dr, 1 + dc:W - 1 + dc]
    for dr, dc in BEHIND:
        ok &= I >= f[:, 1 + dr:H - 1 + dr, 1 + dc:W - 1 + dc]
    if mask is not None:
        ok &= np.asarray(mask)[None, 1:H - 1, 1:W - 1] == 0
    lists, row_start = [], np.zeros((n, H + 1), dtype=np.int32)
    for k in range(n):
        r, c = np.nonzero(ok[k])                      # raster order
        r, c = r + 1, c + 1
        C = tab[f[k, r, c]]
        x = c.astype(np.float64) + _subpixel(tab[f[k, r, c - 1]], C, tab[f[k, r, c + 1]])
        y = r.astype(np.float64) + _subpixel(tab[f[k, r - 1, c]], C, tab[f[k, r + 1, c]])
        lists.append((x, y, frames[k, r, c]))
        row_start[k, 1:] = np.cumsum(np.bincount(r, minlength=H))
    return lists, row_start, row_start[:, H].copy()


def _bracket(c, x):
    k = int(np.searchsorted(c, x, side="right"))     # how many centres are <= x
    j0, j1 = max(k - 1, 0), min(k, len(c) - 1)
    t = (x - c[j0]) / (c[j1] - c[j0]) if j1 > j0 else np.float64(0.0)
    return j0, j1, t


def _bilinear(g, x0, x1, tx, y0, y1, ty):
    a = g[y0, x0] + tx * (g[y0, x1] - g[y0, x0])
    b = g[y1, x0] + tx * (g[y1, x1] - g[y1, x0])
    return a + ty * (b - a)


def predicted(x, y, up, vp, xc, yc):
    """Where the predictor puts the particle at (x, y): the bilinear interpolation between the window centres, constant
    outside them."""
    x0, x1, tx = _bracket(xc, x)
    y0, y1, ty = _bracket(yc, y)
    return x + _bilinear(up, x0, x1, tx, y0, y1, ty), y + _bilinear(vp, x0, x1, tx, y0, y1, ty)


def match(xa, ya, xb, yb, rsb, up, vp, xc, yc, radius, shape, all_pairs=False):
    """One pair: the stored lists of frame a (xa, ya) and of frame b (xb, yb, with frame b's row_start rsb), the predictor
    up, vp float64 [n_rows, n_cols] at the centres xc, yc.  Returns (match int32, status uint8, d2 float64, matched).
    all_pairs: the candidates from every particle of b instead of the rows the radius reaches."""
    H, W = shape
    xa, ya, xb, yb = (np.asarray(t, dtype=np.float64) for t in (xa, ya, xb, yb))
    up, vp, xc, yc = (np.asarray(t, dtype=np.float64) for t in (up, vp, xc, yc))
    na, nb = len(xa), len(xb)
    R = np.float64(radius)
    R2 = R * R
    fwd = np.full(na, -1, dtype=np.int32)
    status = np.zeros(na, dtype=np.uint8)
    d2 = np.full(na, NAN, dtype=np.float64)
    for i in range(na):
        px, py = predicted(xa[i], ya[i], up, vp, xc, yc)
        if not (px >= 0.0 and px <= float(W - 1) and py >= 0.0 and py <= float(H - 1)):
            status[i] = OUTSIDE
            continue
        if all_pairs:
            cand = range(nb)
        else:
            rlo = int(max(np.ceil(py - R - 0.5), 0.0))
            rhi = int(min(np.floor(py + R + 0.5), float(H - 1)))
            cand = range(min(int(rsb[rlo]), nb), min(int(rsb[rhi + 1]), nb))
        best, best_d2 = -1, NAN
        for j in cand:
            dx, dy = px - xb[j], py - yb[j]
            dd = dx * dx + dy * dy
            if dd <= R2 and (best < 0 or dd < best_d2):
                best, best_d2 = j, dd
        fwd[i], d2[i] = best, best_d2
        if best < 0:
            status[i] = NO_CANDIDATE
    out = np.full(na, -1, dtype=np.int32)
    for j in np.unique(fwd[fwd >= 0]):
        claim = np.flatnonzero(fwd == j)
        win = claim[np.lexsort((claim, d2[claim]))[0]]           # the smallest d2, of equal ones the lowest i
        out[win] = j
        status[claim[claim != win]] = LOST_CLAIM
    return out, status, d2, int((out >= 0).sum())


def padded(lists, capacity):
    """The lists of detect() as the device stores them: x, y float64 [n, capacity], peak uint8 [n, capacity] (zeros behind a
    list's end; the device leaves those entries alone) and the stored length of each list."""
    n = len(lists)
    x, y, peak = np.zeros((n, capacity)), np.zeros((n, capacity)), np.zeros((n, capacity), dtype=np.uint8)
    stored = []
    for k, (lx, ly, lp) in enumerate(lists):
        m = min(len(lx), capacity)
        x[k, :m], y[k, :m], peak[k, :m] = lx[:m], ly[:m], lp[:m]
        stored.append(m)
    return x, y, peak, stored


def render(shape, px, py, sigma=1.0, amplitude=200.0):
    """uint8 [H, W]: Gaussian particle images of the given width and amplitude centred at (px, py) (image coordinates: x
    along the columns, y down the rows), summed, rounded and clipped."""
    H, W = shape
    Y, X = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.zeros(shape)
    for x0, y0 in zip(px, py):
        img += amplitude * np.exp(-((X - x0) ** 2 + (Y - y0) ** 2) / (2.0 * sigma * sigma))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


# the scene of the host test and of the end-to-end device tests
SCENE_SHAPE = (96, 160)
SCENE_LEVEL, SCENE_RADIUS = 40, 1.5


def scene_shift(x, y, shape=SCENE_SHAPE):
    """The displacement (u along x, v along y, image coordinates) of the scene at (x, y)."""
    H, W = shape
    return 2.3 + 0.02 * (y - H / 2), -1.6 + 0.015 * (x - W / 2)


def scene(seed=7, shape=SCENE_SHAPE, shift=scene_shift):
    """(frame a, frame b, xa, ya, xb, yb): particles on an 8 px lattice from 8 to H - 8 / W - 8, jittered by +-2 px, Gaussian
    images of sigma 1 and amplitude 200, frame b's displaced by `shift` at each particle's position."""
    H, W = shape
    rng = np.random.default_rng(seed)
    gy, gx = np.meshgrid(np.arange(8, H - 8, 8), np.arange(8, W - 8, 8), indexing="ij")
    xa = gx.ravel() + rng.uniform(-2, 2, gx.size)
    ya = gy.ravel() + rng.uniform(-2, 2, gy.size)
    du, dv = shift(xa, ya, shape) if shift is scene_shift else shift(xa, ya)
    xb, yb = xa + du, ya + dv
    return render(shape, xa, ya), render(shape, xb, yb), xa, ya, xb, yb


def window_centres(size, ws, ov):
    """The centres of the interrogation windows along an axis of `size` pixels, in image coordinates: window k covers the
    pixels k (ws - ov) .. k (ws - ov) + ws - 1."""
    n = (size - ws) // (ws - ov) + 1
    return np.arange(n) * float(ws - ov) + (ws - 1) / 2.0
