"""The 64x64 exact refinement rotates frame b IN REGISTERS (csrc/xcorr_exact.hip, rot_cells / rotate_row): lane y keeps
b[y][0..63] in 16 dwords; for a cell (dy, dx) the wavefront picks one of 16 statically indexed bodies by dx >> 2, shifts by
dx & 3 bytes, and reads frame-a row (y - dy) & 63 from an LDS tile.  A wrong register index in one body, a wrong byte shift
or a wrong row wrap shows in one (dx, dy) class only, so the classes are enumerated:

1. the SHARED neighbourhood (regular arg-max: one rotation to dx - 1 serves m - 1, m, m + 1; m +- W take the rows next to
   it): the arg-max on every fftshift column 0 ... 63 of map rows 0, 1, 31, 32, 62, 63 -- all 16 dword rotations x 4 byte
   shifts, the row wrap in both directions, the irregular columns 0 and 63 (these run the per-cell loop) and the clamps;
2. the PER-CELL loop: windows whose SECOND peak sits on a chosen cell, its column taking every value 0 ... 63, its row the
   map's first and last row, one on each side of the arg-max's row;
3. a mixed batch: regular, irregular, dead and flat windows in consecutive wavefronts, 37 windows (the eight runs of the
   launch have 5 windows each: an odd count, the last workgroup of a run is partial and the last run is cut short).

Construction and comparisons are those of tests/test_gpu_exact_neighbourhood.py: every window against the numpy statement
of the scheme (tests/test_exact_scheme.py) at 1e-13 px with the same flag, the field against the float64 kernel at
1e-11 px with identical masks, the integer part of (u, v) against the displacement that was put in.
"""
import functools

import numpy as np
import pytest
import torch

from test_exact_scheme import exact_window, f32_map
from test_gpu_exact_neighbourhood import TOL_F64, batch, run, tile, window_pair

W = 64
TOL_MODEL = 1e-13        # px, against the numpy statement of the scheme
ROT_ROWS = (0, 1, 31, 32, 62, 63)
SEED_ROT = 11            # (fixed: every one of the 384 windows is decided by the model with this seed)
M1 = (W // 2 + 3) * W + (W // 2 - 5)                 # per-cell test: the arg-max, displacement (dy, dx) = (3, -5)
SECOND_ROWS = (0, 63)                                # rows of the second peak: below and above M1's row 35, the map's borders
                                                     # (dy = -32 and +31: frame a's row index wraps in either direction)
SEED_SECOND = 5


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def rotation_batch():
    """-> cells, windows a, windows b, model results: the arg-max on every column of ROT_ROWS."""
    rng = np.random.default_rng(SEED_ROT)
    cells = [r * W + c for r in ROT_ROWS for c in range(W)]
    wins = [window_pair(W, q, rng) for q in cells]
    wa, wb = [w[0] for w in wins], [w[1] for w in wins]
    return cells, wa, wb, [exact_window(a, b) for a, b in zip(wa, wb)]


def two_peak_pair(q1, q2, rng):
    """(a, b): b = (a rolled by cell q1's displacement + half of a rolled by q2's) / 1.5 + noise: the map peaks at q1 and
    has its second peak at q2."""
    a, _ = window_pair(W, q1, rng)
    af = a.astype(np.float64)
    roll = lambda q: np.roll(af, (q // W - W // 2, q % W - W // 2), axis=(0, 1))
    b = np.clip(np.rint((roll(q1) + 0.5 * roll(q2)) / 1.5) + rng.integers(-2, 3, (W, W)), 0, 255)
    return a, b.astype(np.uint8)


def peaks(a, b, wv=3):
    """-> (arg-max, arg-max outside its exclusion zone) of the float32 map: B:346-358 zeroes clip(m + i + W j), |i|, |j| <= wv."""
    flat = f32_map(a, b).reshape(-1).copy()
    m = int(np.argmax(flat))
    i, j = np.meshgrid(np.arange(-wv, wv + 1), np.arange(-wv, wv + 1))
    flat[np.clip(m + i + W * j, 0, W * W - 1).reshape(-1)] = -np.inf
    return m, int(np.argmax(flat))


@functools.lru_cache(maxsize=None)
def second_peak_batch():
    """-> second-peak cells, windows a, windows b, model results, (arg-max, second peak) of the float32 map per window."""
    rng = np.random.default_rng(SEED_SECOND)
    cells = [r * W + c for c in range(W) for r in SECOND_ROWS]
    wins = [two_peak_pair(M1, q, rng) for q in cells]
    wa, wb = [w[0] for w in wins], [w[1] for w in wins]
    second = [peaks(a, b) for a, b in zip(wa, wb)]
    return cells, wa, wb, [exact_window(a, b) for a, b in zip(wa, wb)], second


def test_the_model_decides_every_rotation_window():
    """(CPU) all 384 windows of the shared-neighbourhood batch: the float32 map peaks at the chosen cell and the scheme
    decides the window, so that the GPU test compares the refinement's own values."""
    cells, wa, wb, model = rotation_batch()
    assert len(cells) == 384
    assert {(q % W - W // 2 - 1) & 63 for q in cells} == set(range(64))          # every rotation of the shared span
    assert all(r is not None for r in model), [cells[i] for i, r in enumerate(model) if r is None]
    off = [q for q, a, b in zip(cells, wa, wb) if int(np.argmax(f32_map(a, b))) != q]
    assert not off, off


def test_the_second_peaks_cover_every_column():
    """(CPU) per column 0 ... 63 at least one window that the model decides, with the map's arg-max on M1 and its second
    peak (the highest cell outside the exclusion zone) on the intended cell; at least 3/4 of all windows decided."""
    cells, wa, wb, model, second = second_peak_batch()
    good = [r is not None and s == (M1, q) for q, r, s in zip(cells, model, second)]
    covered = {q % W for q, g in zip(cells, good) if g}
    assert covered == set(range(W)), sorted(set(range(W)) - covered)
    rows = {q // W for q, g in zip(cells, good) if g}
    assert rows == set(SECOND_ROWS)
    assert sum(r is not None for r in model) >= (len(cells) * 3) // 4


def fallbacks(eng, A, B):
    """Windows of the frame pair that the exact first pass sends to the float64 transform."""
    plan = eng.Plan(A.shape[0], A.shape[1], W, 0, n_pass=1, max_batch=1, precision="exact")
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x[None])).cuda()
    plan.run(dev(A), dev(B))
    n = plan.exact_fallbacks()
    plan.close()
    return n


def compare(eng, A, B, cells, wa, wb, model, shift_of):
    """The three comparisons; -> number of windows held to the model.  shift_of(i): the (dy, dx) put into window i."""
    ue, ve, ie = run(eng, A, B, W, "exact")
    uf, vf, i_f = run(eng, A, B, W, "f64")
    d = max(np.abs(ue - uf).max(), np.abs(ve - vf).max())
    print(f"exact against f64: {d:.3e} px, masks differing: {int((ie != i_f).sum())}")
    assert d < TOL_F64
    assert np.array_equal(ie, i_f)
    n_model, worst = 0, 0.0
    for i, r in enumerate(model):
        if cells[i] < 0 or r is None:   # (dead / flat, or sent to the float64 transform: covered by the comparison above)
            continue
        n_model += 1
        worst = max(worst, abs(r[0] - ue[i]), abs(r[1] - ve[i]))
        assert abs(r[0] - ue[i]) < TOL_MODEL and abs(r[1] - ve[i]) < TOL_MODEL and bool(ie[i]) == r[2], (i, cells[i], r, ue[i], ve[i])
        dy, dx = shift_of(i)
        assert abs(ue[i] - dx) < 1.0 and abs(ve[i] - dy) < 1.0, (i, cells[i], ue[i], ve[i])
    print(f"against the model: {n_model} of {len(cells)} windows, worst {worst:.3e} px")
    return n_model


@pytest.mark.gpu
def test_every_rotation_of_the_shared_neighbourhood(eng):
    cells, wa, wb, model = rotation_batch()
    A, B = tile(wa, W), tile(wb, W)
    n = compare(eng, A, B, cells, wa, wb, model, lambda i: (cells[i] // W - W // 2, cells[i] % W - W // 2))
    assert n == len(cells) == 384
    assert fallbacks(eng, A, B) == 0     # the refinement itself produced every value


@pytest.mark.gpu
def test_every_rotation_of_the_per_cell_loop(eng):
    cells, wa, wb, model, _ = second_peak_batch()
    A, B = tile(wa, W), tile(wb, W)
    n = compare(eng, A, B, cells, wa, wb, model, lambda i: (M1 // W - W // 2, M1 % W - W // 2))
    assert n >= (len(cells) * 3) // 4, (n, len(cells))


@pytest.mark.gpu
def test_mixed_wavefronts_and_a_partial_last_workgroup(eng):
    """Regular and irregular arg-maxes alternate, a dead and a flat window in between; 37 windows in one column."""
    _, _, cells, wa, wb = batch(W, 23, mixed=True)
    cells, wa, wb = cells[:37], wa[:37], wb[:37]
    assert len(cells) == 37 and cells.count(-1) == 2
    A, B = np.concatenate(wa, axis=0), np.concatenate(wb, axis=0)
    model = [exact_window(a, b) if q >= 0 else None for q, a, b in zip(cells, wa, wb)]
    n = compare(eng, A, B, cells, wa, wb, model, lambda i: (cells[i] // W - W // 2, cells[i] % W - W // 2))
    assert n >= (len(cells) * 3) // 4, (n, len(cells))
