"""The exact refinement's two paths for the arg-max's neighbourhood (csrc/xcorr_exact.hip, xcorr_exact_refine_kernel<W>).

A wavefront whose windows all have a REGULAR arg-max m (fftshift column 1 ... W - 2, none of the four flat-index clamps of
B:385-392) evaluates m and its four neighbours from one shared span of frame b and the frame-a rows above and below; any
other wavefront evaluates every cell on its own.  Windows are built so that the arg-max lands on a chosen cell: frame b is
frame a rolled circularly by that cell's displacement (plus a little noise), windows side by side with no overlap.  The
cells cover fftshift columns 0, 1, W - 2, W - 1, map rows 0 and W - 1 (the circular row wrap) and each clamp.  Every window
is checked against the numpy statement of the scheme (tests/test_exact_scheme.py) and the whole field against the float64
kernel, as tests/test_gpu_exact.py does.
"""
import numpy as np
import pytest
import torch

from test_exact_scheme import exact_window, f32_map

TOL_F64 = 1e-11          # px, exact sums against a float64 transform (as in test_gpu_exact.py)
COLS = 8                 # windows per frame row


def target_cells(W):
    """Flat fftshift indices the arg-max is put on: the border columns and rows, every clamp, and a few regular cells."""
    KD = W * W
    lines = [0, 1, W // 2 - 3, W // 2, W - 2, W - 1]
    cells = {r * W + c for r in lines for c in lines}
    cells |= {KD - 2, KD - 1, 0, 1, KD - 1 - W, W, KD - W, W - 1}      # left / right / top / bottom clamps and their edges
    return sorted(cells)


def window_pair(W, q, rng):
    """(a, b): b is a rolled by the displacement of cell q, so that the circular correlation peaks at q."""
    dy, dx = q // W - W // 2, q % W - W // 2
    base = rng.integers(0, 256, (W, W)).astype(np.float64)
    blur = sum(np.roll(base, (i, j), axis=(0, 1)) for i in (-1, 0, 1) for j in (-1, 0, 1)) / 9.0
    a = np.clip(np.rint(2.0 * (blur - 128.0) + 128.0), 0, 255)
    b = np.clip(np.roll(a, (dy, dx), axis=(0, 1)) + rng.integers(-2, 3, (W, W)), 0, 255)
    return a.astype(np.uint8), b.astype(np.uint8)


def tile(wins, W):
    """Windows side by side, COLS per row, in raster order (consecutive windows share wavefronts at 32x32)."""
    rows = -(-len(wins) // COLS)
    F = np.zeros((rows * W, COLS * W), np.uint8)
    for i, w in enumerate(wins):
        r, c = divmod(i, COLS)
        F[r * W:(r + 1) * W, c * W:(c + 1) * W] = w
    return F


def regular(q, W):
    KD = W * W
    return 1 <= q % W <= W - 2 and q + 1 < KD - 1 and q - 1 > 0 and q + W < KD - 1 and q - W > 0


def batch(W, seed, mixed):
    """-> frames A, B and the intended arg-max per window (-1: a window that does not go: dead, or flat)."""
    rng = np.random.default_rng(seed)
    cells = target_cells(W)
    if mixed:                            # regular and irregular arg-maxes alternate, dead and flat windows in between
        reg = [q for q in cells if regular(q, W)]
        irr = [q for q in cells if not regular(q, W)]
        cells = [x for pair in zip(reg * 4, irr) for x in pair]
        cells[5] = cells[12] = -1
    wa, wb = [], []
    for k, q in enumerate(cells):
        if q >= 0:
            a, b = window_pair(W, q, rng)
        elif k == 5:
            a, b = np.zeros((W, W), np.uint8), rng.integers(0, 256, (W, W)).astype(np.uint8)     # dead frame-a window
        else:
            a, b = np.full((W, W), 77, np.uint8), np.full((W, W), 91, np.uint8)             # flat: constant map
        wa.append(a)
        wb.append(b)
    return tile(wa, W), tile(wb, W), cells, wa, wb


@pytest.mark.parametrize("W", [32, 64, 128])
def test_windows_put_the_arg_max_on_the_chosen_cell(W):
    """(CPU) the construction does what the GPU test relies on: the float32 map peaks at the chosen cell."""
    _, _, cells, wa, wb = batch(W, 1, mixed=False)
    for q, a, b in list(zip(cells, wa, wb))[:: max(1, len(cells) // 12)]:
        assert int(np.argmax(f32_map(a, b))) == q, (W, q)


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def run(eng, A, B, W, precision):
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x[None])).cuda()
    u, v, inv = eng.pass1(dev(A), dev(B), W, 0, precision=precision)
    torch.cuda.synchronize()
    return u[0].cpu().numpy().reshape(-1), v[0].cpu().numpy().reshape(-1), inv[0].cpu().numpy().reshape(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("mixed", [False, True], ids=["border_cells", "mixed_wavefronts"])
@pytest.mark.parametrize("W", [32, 64, 128])
def test_exact_neighbourhood_on_border_and_clamped_arg_maxes(eng, W, mixed):
    A, B, cells, wa, wb = batch(W, 7 + W, mixed)
    n = len(cells)
    ue, ve, ie = run(eng, A, B, W, "exact")
    uf, vf, i_f = run(eng, A, B, W, "f64")
    assert np.abs(ue - uf).max() < TOL_F64 and np.abs(ve - vf).max() < TOL_F64
    assert np.array_equal(ie, i_f)
    n_model = 0
    for i in range(n):
        if cells[i] < 0:
            continue
        r = exact_window(wa[i], wb[i])
        if r is None:                    # (the scheme sends it to the float64 transform: covered by the comparison above)
            continue
        n_model += 1
        assert abs(r[0] - ue[i]) < 1e-13 and abs(r[1] - ve[i]) < 1e-13 and bool(ie[i]) == r[2], (W, i, cells[i], r, ue[i], ve[i])
        # the arg-max is where it was put: the integer part of the displacement (dy, dx) of the chosen cell
        dy, dx = cells[i] // W - W // 2, cells[i] % W - W // 2
        assert abs(ue[i] - dx) < 1.0 and abs(ve[i] - dy) < 1.0, (W, i, cells[i], ue[i], ve[i])
    assert n_model >= (n * 3) // 4, (n_model, n)
