"""Inputs shared by tests/test_exact_offsets_host.py and tests/test_gpu_exact_offsets.py (profiles/exact_offsets/).

(1) tests/golden/g14_exact_first_pass_offsets.npz: two 2 x 2 blocks of neighbouring 64 x 64 windows (50 % overlap) of the
64-pair comparison of profiles/twiddle_first/bits.txt, with the first-pass vectors recorded for them.  The records that
were "off" are what the oracle gives for the same windows with ONE frame pixel one grey level higher: the frames were
rendered again for each run, and the unordered float32 sum of synth._render rounded that pixel the other way.
(2) frames whose left part repeats with a period of half a window: the windows inside it have exactly tied correlation
maxima, S(d) = S(d + period), so the exact first pass cannot decide them and fills its undecided list with them.
"""
import os

import numpy as np

WS, OV = 64, 32
STEP = WS - OV

# (block's first fixture window, frame that holds the pixel, frame row, frame column, stored value, recorded field with the increment)
INCREMENTS = (
    (0, "b", 1368, 1668, 40, "this"),       # pair 0, windows (41..42, 51..52)
    (4, "a", 318, 1141, 112, "parent"),     # pair 27, windows (8..9, 34..35)
)


def load_g14():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_exact_first_pass_offsets.npz")
    with np.load(path, allow_pickle=False) as g:
        return {k: g[k] for k in g.files}


def local_position(g, k, row, col):
    """(row, column) inside fixture window k of the frame pixel (row, col); the window starts at STEP * its grid position."""
    _, wr, wc = (int(x) for x in g["pair_row_col"][k])
    return row - STEP * wr, col - STEP * wc


def incremented_windows(g, block):
    """-> a, b uint8 [4, 64, 64] of the block's four windows with its frame pixel one grey level higher, and the four
    window-local positions of that pixel."""
    k0, frame, row, col, value, _ = INCREMENTS[block]
    a, b = g["a"][k0:k0 + 4].copy(), g["b"][k0:k0 + 4].copy()
    where = []
    for k in range(4):
        ly, lx = local_position(g, k0 + k, row, col)
        assert 0 <= ly < WS and 0 <= lx < WS, (k, ly, lx)
        target = a if frame == "a" else b
        assert target[k, ly, lx] == value, (k, ly, lx, int(target[k, ly, lx]))
        target[k, ly, lx] += 1
        where.append((ly, lx))
    return a, b, where


def mosaic(w):
    """Four windows [4, 64, 64] at grid positions (r, c), (r, c + 1), (r + 1, c), (r + 1, c + 1) -> the 96 x 96 image
    they cut out of their frame; every overlap must agree."""
    out = np.zeros((WS + STEP, WS + STEP), np.uint8)
    seen = np.zeros(out.shape, bool)
    for k, (r, c) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        ys, xs = slice(STEP * r, STEP * r + WS), slice(STEP * c, STEP * c + WS)
        assert np.array_equal(out[ys, xs][seen[ys, xs]], w[k][seen[ys, xs]]), f"window {k} disagrees with its neighbours on their overlap"
        out[ys, xs] = w[k]
        seen[ys, xs] = True
    assert seen.all()
    return out


def g14_mosaics(g):
    """-> A, B uint8 [4, 96, 96]: block 0 stored, block 0 incremented, block 1 stored, block 1 incremented."""
    A, B = [], []
    for block, (k0, *_rest) in enumerate(INCREMENTS):
        ai, bi, _ = incremented_windows(g, block)
        for a, b in ((g["a"][k0:k0 + 4], g["b"][k0:k0 + 4]), (ai, bi)):
            A.append(mosaic(a))
            B.append(mosaic(b))
    return np.stack(A), np.stack(B)


def tied_frames(size, ws, first_index):
    """Four pairs of synth's "wavy" kind at noise 2, rendered on the CPU; in both frames the left half (columns 0 .. size/2 - 1)
    is four copies of columns 0 .. ws/2 - 1.  -> A, B uint8 [4, size, size], tied bool [n_rows, n_cols]: the windows that
    lie inside the periodic part."""
    from torchpiv_amd import synth
    period = ws // 2
    assert size == 8 * period
    A, B = [], []
    for i in range(4):
        a, b = (f.numpy().copy() for f in synth.make_pair(size, size, first_index + i, kind="wavy", noise=2.0))
        for f in (a, b):
            f[:, :4 * period] = np.tile(f[:, :period], (1, 4))
        A.append(a)
        B.append(b)
    n = (size - ws) // period + 1
    tied = np.zeros((n, n), bool)
    tied[:, [c for c in range(n) if c * period + ws <= 4 * period]] = True
    return np.stack(A), np.stack(B), tied
