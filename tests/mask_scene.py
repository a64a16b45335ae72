"""Frames for the tests of the geometric mask: a static lit band across a uniform flow (the scene that motivates the
feature) and a small recording with a block and a frame edge masked."""
import numpy as np
import torch

FLOW = (2.3, -1.6)                  # synth's "uniform" flow (u, v) in px
BAND = (103, 147)                   # rows of the band


def band_scene(index=7, H=256, W=256):
    """(a, b, band a, band b, mask) as uint8 numpy arrays: synth's uniform pair `index`, the same with rows BAND of both
    frames replaced by max(frame, texture) -- a static texture, uniform random 60...199, the same for every pair -- and
    the mask image of the band."""
    from torchpiv_amd import synth
    a, b = (t.numpy() for t in synth.make_pair(H, W, index, kind="uniform"))
    tex = np.random.default_rng(3).integers(60, 200, (BAND[1] - BAND[0], W)).astype(np.uint8)
    wa, wb = a.copy(), b.copy()
    wa[BAND[0]:BAND[1]] = np.maximum(a[BAND[0]:BAND[1]], tex)
    wb[BAND[0]:BAND[1]] = np.maximum(b[BAND[0]:BAND[1]], tex)
    mask = np.zeros((H, W), np.uint8)
    mask[BAND[0]:BAND[1]] = 1
    return a, b, wa, wb, mask


def band_batch(n=4, first=7):
    """(A, B) uint8 tensors [n, 256, 256] of the band frames of pairs first ... first + n - 1, and the mask image."""
    scenes = [band_scene(first + i) for i in range(n)]
    A = torch.from_numpy(np.stack([s[2] for s in scenes]))
    B = torch.from_numpy(np.stack([s[3] for s in scenes]))
    return A, B, scenes[0][4]


SH, SW = 128, 160


def block_mask(H=SH, W=SW):
    """A block in the interior and the left rim of the frame, with bytes 1, 7 and 255: at 32/16 and at 16/8 some windows
    are excluded at threshold 0.5 and some are partly covered."""
    m = np.zeros((H, W), np.uint8)
    m[40:90, 50:110] = 7
    m[60:70, 60:80] = 255
    m[:, :12] = 1
    return m


def block_pairs(n=4, noise=6.0, density=0.015):
    """n pairs [n, SH, SW] of synth's wavy flow, noisy and sparse enough that every pass leaves a few invalid vectors
    (a pair without any is dropped by the reference's post-validation, B:300-304), with a lit static texture under the
    mask of block_mask()."""
    from torchpiv_amd import synth
    pairs = [synth.make_pair(SH, SW, 40 + i, kind="wavy", noise=noise, density=density) for i in range(n)]
    A = torch.stack([p[0] for p in pairs]).clone()
    B = torch.stack([p[1] for p in pairs]).clone()
    m = torch.from_numpy(block_mask() != 0)
    tex = torch.from_numpy(np.random.default_rng(5).integers(60, 200, (SH, SW)).astype(np.uint8))
    A[:, m] = torch.maximum(A[:, m], tex[m])
    B[:, m] = torch.maximum(B[:, m], tex[m])
    return A, B
