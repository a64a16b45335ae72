"""Numpy model of the iterative image deformation (torchpiv_amd/csrc/deform.hip, include/torchpiv_hip.h): the Q8 nodes of a
field, the dense half shift between them, the warp of both frames (the sampling is dewarp_model's), the combine, and the
chain of rounds around any first pass.  Also the scene of the accuracy checks: particles moved by a sinusoidal field whose
gradients a rigid window cannot follow.  Nothing here shares a line with torchpiv_amd.engine or with the device code."""
import math

import numpy as np

import dewarp_model as DM

NODE_MAX = 16383


def field_shape(H, W, ws, ov):
    return (H - ws) // (ws - ov) + 1, (W - ws) // (ws - ov) + 1


# ---- nodes ----------------------------------------------------------------------------------------------------------
def quantise(w):
    """clamp(rint(w * 128), -16383, 16383) as int64; the caller has removed non-finite values."""
    with np.errstate(over="ignore"):
        return np.clip(np.rint(np.asarray(w, dtype=np.float64) * 128.0), -NODE_MAX, NODE_MAX).astype(np.int64)


def nodes(u, v, invalid, smooth=True):
    """int16 [..., n_rows, n_cols, 2] (x first) from u, v float64 and invalid [..., n_rows, n_cols]."""
    u, v, invalid = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64), np.asarray(invalid)
    if u.ndim == 3:
        return np.stack([nodes(u[k], v[k], invalid[k], smooth) for k in range(u.shape[0])])
    nr, nc = u.shape
    ok = (invalid == 0) & np.isfinite(u) & np.isfinite(v)
    q = np.stack([quantise(np.where(ok, u, 0.0)), quantise(np.where(ok, v, 0.0))], axis=-1)
    q[~ok] = 0
    # the substitution reads the unsubstituted values: sums over the up to 8 valid neighbours in the grid
    qp = np.pad(q, ((1, 1), (1, 1), (0, 0)))
    kp = np.pad(ok.astype(np.int64), 1)
    s = np.zeros_like(q)
    k = np.zeros((nr, nc), dtype=np.int64)
    for dr in (0, 1, 2):
        for dc in (0, 1, 2):
            if (dr, dc) != (1, 1):
                s += qp[dr:dr + nr, dc:dc + nc]
                k += kp[dr:dr + nr, dc:dc + nc]
    kk = np.maximum(k, 1)[..., None]
    sub = np.where(k[..., None] > 0, (2 * s + kk) // (2 * kk), 0)           # numpy's // is the floor
    q = np.where(ok[..., None], q, sub)
    if smooth:
        e = np.pad(q, ((1, 1), (1, 1), (0, 0)), mode="edge")
        acc = np.zeros_like(q)
        for dr, wr in zip((0, 1, 2), (1, 2, 1)):
            for dc, wc in zip((0, 1, 2), (1, 2, 1)):
                acc += wr * wc * e[dr:dr + nr, dc:dc + nc]
        q = (acc + 8) >> 4
    return q.astype(np.int16)


# ---- dense half shift -----------------------------------------------------------------------------------------------
def axis(size, n, ws, st):
    """(r, w) of every pixel coordinate 0 .. size - 1 along an axis of n windows: node cell and Q8 weight 0 .. 256."""
    y = np.arange(size, dtype=np.int64)
    if n == 1:
        return np.zeros(size, dtype=np.int64), np.zeros(size, dtype=np.int64)
    a = 2 * y - (ws - 1)
    r = np.clip(a // (2 * st), 0, n - 2)
    t = np.clip(a - 2 * r * st, 0, 2 * st)
    return r, (256 * t + st) // (2 * st)


def dense(nd, H, W, ws, ov):
    """(hx, hy) int64 [H, W]: the half shift of every pixel from the nodes int16 [n_rows, n_cols, 2]."""
    nr, nc = nd.shape[:2]
    st = ws - ov
    r, wy = axis(H, nr, ws, st)
    c, wx = axis(W, nc, ws, st)
    r1, c1 = np.minimum(r + 1, nr - 1), np.minimum(c + 1, nc - 1)
    n = nd.astype(np.int64)
    wy, wx = wy[:, None, None], wx[None, :, None]
    top = (256 - wx) * n[r][:, c] + wx * n[r][:, c1]
    bot = (256 - wx) * n[r1][:, c] + wx * n[r1][:, c1]
    h = ((256 - wy) * top + wy * bot + 32768) >> 16
    return h[..., 0], h[..., 1]


def positions(nd, H, W, ws, ov):
    """The Q8 sampling maps (ma, mb), int32 [H, W, 2] each (x first): frame a at -h, frame b at +h, clamped to the frame."""
    hx, hy = dense(nd, H, W, ws, ov)
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    out = []
    for sign in (-1, 1):
        qx = np.clip((x << 8) + sign * hx, 0, (W - 1) << 8)
        qy = np.clip((y << 8) + sign * hy, 0, (H - 1) << 8)
        out.append(np.stack([qx, qy], axis=-1).astype(np.int32))
    return out


def warp(a, b, nd, ws, ov, interp="cubic"):
    """(wa, wb) uint8 like the frames [H, W] or [batch, H, W]; nd int16 [(batch,) n_rows, n_cols, 2]."""
    if a.ndim == 3:
        pairs = [warp(a[k], b[k], nd[k], ws, ov, interp) for k in range(a.shape[0])]
        return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    H, W = a.shape
    ma, mb = positions(nd, H, W, ws, ov)
    return DM.dewarp(a, ma, interp), DM.dewarp(b, mb, interp)


def combine(nd, du, dv, dval):
    """u = qx / 128 + du, v = qy / 128 + dv (the quotient is exact: one rounding), invalid = dval."""
    q = nd.astype(np.float64)
    return q[..., 0] * (1.0 / 128) + du, q[..., 1] * (1.0 / 128) + dv, np.asarray(dval).astype(np.uint8)


def rounds(a, b, u, v, invalid, ws, ov, n, pass1, interp="cubic", smooth=True):
    """n rounds on one pair: pass1(wa, wb) -> (du, dv, dval) is the first pass at (ws, ov)."""
    for _ in range(n):
        nd = nodes(u, v, invalid, smooth)
        wa, wb = warp(a, b, nd, ws, ov, interp)
        du, dv, dval = pass1(wa, wb)
        u, v, invalid = combine(nd, du, dv, dval)
    return u, v, invalid


# ---- the scene of the accuracy checks -------------------------------------------------------------------------------
PERIOD = 96.0


def flow(x, y):
    """The constructed displacement (dx, dy) at positions (x, y): peak gradient 3 * 2 pi / 96 = 0.196 px / px."""
    return 3.0 * np.sin(2 * math.pi * y / PERIOD), 1.5 * np.sin(2 * math.pi * x / PERIOD)


def scene(seed, H=256, W=256, density=0.04, sigma=1.0, noise=2.0, offset=8.0):
    """(a, b) uint8 [H, W]: particles at p rendered at p - d(p) / 2 in frame a and at p + d(p) / 2 in frame b."""
    import torch
    from torchpiv_amd import synth
    g = torch.Generator(device="cpu")
    g.manual_seed(977 + int(seed))
    pad = 10.0
    n = int(density * (H + 2 * pad) * (W + 2 * pad))
    px = torch.rand(n, generator=g, dtype=torch.float64) * (W + 2 * pad) - pad
    py = torch.rand(n, generator=g, dtype=torch.float64) * (H + 2 * pad) - pad
    amp = ((0.5 + 0.5 * torch.rand(n, generator=g, dtype=torch.float64)) * 200.0).float()
    na = torch.randn(H, W, generator=g) * noise
    nb = torch.randn(H, W, generator=g) * noise
    dx, dy = flow(px.numpy(), py.numpy())
    dx, dy = torch.from_numpy(dx), torch.from_numpy(dy)
    frames = []
    for sign, nz in ((-0.5, na), (0.5, nb)):
        img = synth._render((px + sign * dx).float(), (py + sign * dy).float(), amp, H, W, sigma, "cpu") + offset + nz
        frames.append(img.round().clamp_(0, 255).to(torch.uint8).numpy())
    return frames[0], frames[1]


def truth(H, W, ws, ov):
    """(du, dv) [n_rows, n_cols]: the constructed displacement at the window centres r st + (ws - 1) / 2."""
    nr, nc = field_shape(H, W, ws, ov)
    st = ws - ov
    yc = np.arange(nr) * st + (ws - 1) / 2.0
    xc = np.arange(nc) * st + (ws - 1) / 2.0
    X, Y = np.meshgrid(xc, yc)
    return flow(X, Y)


def rms_interior(u, v, tu, tv, ok):
    """RMS vector error over the interior cells (a one-cell rim left out) where ok; also the share of interior cells ok."""
    sel = np.zeros(u.shape, dtype=bool)
    sel[1:-1, 1:-1] = True
    use = sel & ok
    e2 = (u - tu) ** 2 + (v - tv) ** 2
    return float(np.sqrt(e2[use].mean())), float(use.sum() / sel.sum())
