"""Frames for the tests of the per-pair masks: a disc that moves 6 px per pair across synth's uniform flow, lit and textured
(a body in the light sheet) or dark (a shadow without particles), and the frames that try the segmentation kernel's tile
seams, rim and corners."""
import numpy as np

FLOW = (2.3, -1.6)                  # synth's "uniform" flow (u, v) in px
RADIUS = 30
N_PAIRS = 4
BRIGHT = {"kind": "bright", "size": 7, "level": 40, "grow": 2}
DARK = {"kind": "dark", "size": 21, "level": 14, "grow": 0}
THRESHOLD = 0.5


def disc(cx, cy, H=256, W=256, radius=RADIUS):
    y, x = np.mgrid[0:H, 0:W]
    return (x - cx) ** 2 + (y - cy) ** 2 <= radius ** 2


def centres(i):
    """(x, y) of the disc's centre in frame a and in frame b of pair i."""
    return (80 + 12 * i, 128), (86 + 12 * i, 128)


def body(i):
    """bool [256, 256]: the pixels the body covers in either frame of pair i."""
    ca, cb = centres(i)
    return disc(*ca) | disc(*cb)


def disc_pair(i, kind):
    """(a, b) uint8 numpy [256, 256] of pair i: synth's uniform pair 7 + i (noise 2.0) with the disc.  "bright":
    max(frame, texture) inside it, the texture rolled along x with the body; "dark": min(frame, 3) inside it."""
    from torchpiv_amd import synth
    a, b = (t.numpy().copy() for t in synth.make_pair(256, 256, 7 + i, kind="uniform", noise=2.0))
    ca, cb = centres(i)
    da, db = disc(*ca), disc(*cb)
    if kind == "bright":
        tex = np.random.default_rng(3).integers(60, 200, (256, 256)).astype(np.uint8)
        ta, tb = np.roll(tex, 12 * i, axis=1), np.roll(tex, 12 * i + 6, axis=1)
        a[da] = np.maximum(a[da], ta[da])
        b[db] = np.maximum(b[db], tb[db])
    else:
        a[da] = np.minimum(a[da], 3)
        b[db] = np.minimum(b[db], 3)
    return a, b


def disc_batch(kind, n=N_PAIRS):
    """(A, B) uint8 numpy [n, 256, 256] of the pairs 0 ... n - 1."""
    pairs = [disc_pair(i, kind) for i in range(n)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def bar_frames(H, W, size, level, kind, seed=0):
    """(a, b) uint8 [H, W]: sparse particles on a dark ground ("bright"; inverted for "dark") plus bars size - 1, size and
    size + 1 wide -- horizontal and vertical, laid across rows 63/64 and columns 127/128 where the frame reaches them, in
    the four corners and along the rim -- in frame a, and the same shifted by (1, 2) pixels in frame b.  Bar pixels are at
    `level` or just inside it, the ground just outside, so the comparison with the level is tried at its edge."""
    rng = np.random.default_rng(seed + 17 * H + W)
    k = size
    inside = (lambda n: rng.integers(level, min(level + 3, 255) + 1, n)) if kind == "bright" \
        else (lambda n: rng.integers(max(level - 3, 0), level + 1, n))
    outside = max(level - 1, 0) if kind == "bright" else min(level + 1, 255)

    def one(dy, dx):
        f = np.full((H, W), outside, np.int64)
        # particles: single pixels and 2 x 2 blobs that pass the level but are narrower than any size
        for _ in range(max(4, H * W // 200)):
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            f[y:y + 2, x:x + 1 + (y & 1)] = inside(1)[0]
        spots = [(0, 0), (0, W), (H, 0), (H, W), (H // 2, 0), (0, W // 2), (H, W // 2), (H // 2, W)]      # corners, rim
        if H > 64:
            spots += [(64, W // 3), (64 - k // 2, 2 * W // 3)]                                            # tile seam rows
        if W > 128:
            spots += [(H // 3, 128), (2 * H // 3, 128 - k // 2)]                                          # tile seam columns
        for j, (cy, cx) in enumerate(spots):
            w = k - 1 + j % 3                                       # k - 1, k, k + 1 in turn
            length = k + 3 + j
            y0, x0 = cy - w // 2 + dy, cx - length // 2 + dx
            if j % 2:                                               # every other bar stands upright
                y0, x0, hh, ww = cy - length // 2 + dy, cx - w // 2 + dx, length, w
            else:
                hh, ww = w, length
            ys, xs = slice(max(y0, 0), max(min(y0 + hh, H), 0)), slice(max(x0, 0), max(min(x0 + ww, W), 0))
            shape = f[ys, xs].shape
            f[ys, xs] = inside(shape[0] * shape[1]).reshape(shape)
        return f.astype(np.uint8)
    return one(0, 0), one(1, 2)


MH, MW = 128, 160
MOVING = {"kind": "bright", "size": 7, "level": 40, "grow": 1}


def moving_rim(H=MH, W=MW):
    """A static image to go with the moving block: the left rim of the frame, with bytes 1 and 255."""
    m = np.zeros((H, W), np.uint8)
    m[:, :10] = 1
    m[:5, :10] = 255
    return m


def moving_block_pairs(n=4, noise=6.0, density=0.015):
    """(A, B) uint8 tensors [n, MH, MW]: synth's wavy flow, noisy and sparse enough that every pass leaves a few invalid
    vectors (a pair without any is dropped by the reference's post-validation), with a lit textured block of 50 x 46
    pixels that stands 10 px further right in every pair and moves 4 px from frame a to frame b."""
    import torch
    from torchpiv_amd import synth
    pairs = [synth.make_pair(MH, MW, 40 + i, kind="wavy", noise=noise, density=density) for i in range(n)]
    A = torch.stack([p[0] for p in pairs]).clone()
    B = torch.stack([p[1] for p in pairs]).clone()
    tex = torch.from_numpy(np.random.default_rng(5).integers(60, 200, (MH, MW)).astype(np.uint8))
    for i in range(n):
        for F, x0 in ((A, 30 + 10 * i), (B, 34 + 10 * i)):
            F[i, 40:90, x0:x0 + 46] = torch.maximum(F[i, 40:90, x0:x0 + 46], tex[40:90, 30:76])
    return A, B
