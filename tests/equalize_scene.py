"""The scene of the equalize= on-frames figures, shared by the GPU test and by whoever recomputes the
figures with the CPU oracle: four 256 x 256 pairs of a uniform (2.3, -1.6) px flow whose illumination is multiplied by a
ramp across the frame, and the statistics taken against the run on the clean frames.  No GPU involved."""
import numpy as np

N, H, W = 4, 256, 256
FLOOR = 0.15                # the ramp's value at column 0; 1 at the last column
CHAIN = (32, 16, 2)         # 32/16 -> 16/8, CWS


def ramp_scene(floor=FLOOR):
    """(A, B, A_ramp, B_ramp): uint8 numpy [N, H, W] -- the clean pairs and the same pairs with every pixel multiplied by
    floor + (1 - floor) x / (W - 1) and rounded half up, in integers."""
    from torchpiv_amd import synth
    A, B = synth.make_batch(N, H, W, kind="uniform")
    A, B = A.numpy(), B.numpy()
    q = np.rint((floor + (1.0 - floor) * np.arange(W) / (W - 1)) * 4096).astype(np.int64)     # the ramp in 1/4096
    dim = [((F.astype(np.int64) * q[None, None, :] + 2048) >> 12).astype(np.uint8) for F in (A, B)]
    return A, B, dim[0], dim[1]


def stats(res, clean, x):
    """res, clean: per pair (u, v, invalid) of the raw last pass on the grid x (px, [rows, cols]).  Returns (bad, bright):
    the number of vectors that are invalid or more than 0.5 px from the clean run's, and the largest distance from the
    clean run's among the vectors of the bright half (x >= W / 2) that are valid in both."""
    bad, bright = 0, 0.0
    for (u, v, inv), (cu, cv, cinv) in zip(res, clean):
        d = np.hypot(u - cu, v - cv)
        bad += int((inv.astype(bool) | (d > 0.5)).sum())
        ok = (x >= W / 2) & ~inv.astype(bool) & ~cinv.astype(bool)
        assert ok.sum() > 50
        bright = max(bright, float(d[ok].max()))
    return bad, bright
