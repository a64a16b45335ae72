"""Single-pixel ensemble correlation on the CPU: the numpy model (tests/pixel_corr_model.py) against a literal triple-loop
evaluation of the definition in include/torchpiv_hip.h, the argument checks, the three symbols, and the model's accuracy on
the channel scene."""
import json
import math
import os

import numpy as np
import pytest

import pixel_corr_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("tpiv_pixel_corr_bytes", "tpiv_pixel_corr_add", "tpiv_pixel_corr_peaks")

# measured with this model on scene(seed=0): bins (1, 128), 32 pairs, radius 5, the 54 interior rows of the second bin column
MEASURED_RMS, MEASURED_MAX = 0.0050, 0.0129
CAP_RMS, CAP_MAX = 3 * MEASURED_RMS, 3 * MEASURED_MAX


def by_definition(A, B, n_pairs, ky, kx, R, sy, sx):
    """acc, the coefficient planes and the statuses border / flat straight from the definition: Python integers (no
    overflow to think about), one loop per sum."""
    n, H, W = A.shape
    D = 2 * R + 1
    nby, nbx = H // ky, W // kx
    a = [[[int(A[i, y, x]) for x in range(W)] for y in range(H)] for i in range(n)]
    b = [[[int(B[i, y, x]) for x in range(W)] for y in range(H)] for i in range(n)]

    def bat(i, y, x):
        return b[i][y][x] if 0 <= y < H and 0 <= x < W else 0

    acc = np.zeros((nby, nbx, D, D), np.int64)
    C = np.zeros((nby, nbx, D, D))
    status = np.zeros((nby, nbx), np.uint8)
    for r in range(nby):
        for c in range(nbx):
            pix = [(y, x) for y in range(r * ky, (r + 1) * ky) for x in range(c * kx, (c + 1) * kx)]
            border = flat = False
            va = sum(n_pairs * sum(a[i][y][x] ** 2 for i in range(n)) - sum(a[i][y][x] for i in range(n)) ** 2 for y, x in pix)
            nums, vbs = {}, {}
            for j in range(D):
                for i_ in range(D):
                    dy, dx = sy + j - R, sx + i_ - R
                    border |= any(not (0 <= y + dy < H and 0 <= x + dx < W) for y, x in pix)
                    s = sum(a[i][y][x] * bat(i, y + dy, x + dx) for i in range(n) for y, x in pix)
                    acc[r, c, j, i_] = s
                    nums[j, i_] = n_pairs * s - sum(sum(a[i][y][x] for i in range(n)) * sum(bat(i, y + dy, x + dx) for i in range(n))
                                                    for y, x in pix)
                    vbs[j, i_] = sum(n_pairs * sum(bat(i, y + dy, x + dx) ** 2 for i in range(n))
                                     - sum(bat(i, y + dy, x + dx) for i in range(n)) ** 2 for y, x in pix)
            flat = va == 0 or any(v == 0 for v in vbs.values())
            status[r, c] = 1 if border else (2 if flat else 0)
            if not border and not flat:
                for (j, i_), num in nums.items():
                    C[r, c, j, i_] = float(num) / math.sqrt(float(va) * float(vbs[j, i_]))
    return acc, C, status


def test_model_against_the_definition():
    rng = np.random.default_rng(5)
    H, W, n = 9, 11, 3
    A = rng.integers(0, 256, (n, H, W)).astype(np.uint8)
    B = rng.integers(0, 256, (n, H, W)).astype(np.uint8)
    A[:, 4, 4:6] = 7                                   # a flat bin of a at (2, 2) under 2 x 2 bins ...
    A[:, 5, 4:6] = 7
    for (ky, kx), R, (sy, sx) in (((1, 1), 3, (0, 0)), ((2, 2), 3, (0, 1)), ((1, 3), 3, (-1, 0)), ((3, 2), 4, (0, 0))):
        acc, mom = M.accumulate(A, B, (ky, kx), R, (sy, sx))
        want_acc, want_C, want_status = by_definition(A, B, n, ky, kx, R, sy, sx)
        assert np.array_equal(acc, want_acc), (ky, kx, R)
        out = M.peaks(acc, mom, n, (H, W), (ky, kx), R, (sy, sx))
        early = np.where(out["status"] > 2, 0, out["status"])
        assert np.array_equal(early, want_status), (ky, kx, R, out["status"], want_status)
        assert np.array_equal(out["corr"], want_C), (ky, kx, R)          # bit for bit: the same float64 operations
        assert np.array_equal(np.isnan(out["u"]), out["status"] != 0)
    # splitting the recording into calls changes nothing
    acc2, mom2 = M.accumulate(A[:1], B[:1], (2, 2), 3, (0, 1))
    acc2, mom2 = M.accumulate(A[1:], B[1:], (2, 2), 3, (0, 1), acc2, mom2)
    acc1, mom1 = M.accumulate(A, B, (2, 2), 3, (0, 1))
    assert np.array_equal(acc1, acc2) and np.array_equal(mom1, mom2)


def test_model_statuses_on_prescribed_planes():
    R, D = 3, 7
    yy, xx = np.mgrid[0:D, 0:D]
    C = 0.1 + 0.8 * np.exp(-((yy - 4.25) ** 2 + (xx - 2.4) ** 2) / 2.0)
    u, v, peak, ratio, st = M.peak_of(C, R, (2, -1))
    assert st == 0 and abs(u - (-1 + 2.4 - R)) < 0.05 and abs(v - (2 + 4.25 - R)) < 0.05 and peak == C[4, 2]
    C2 = C.copy()
    C2[0, 3] = 2.0
    assert M.peak_of(C2, R)[4] == M.STATUS["range"]
    C3 = np.full((D, D), 0.25)
    C3[2, 2] = C3[2, 5] = 0.75                         # two equal maxima: the first in raster order
    u, v, peak, ratio, st = M.peak_of(C3, R)
    assert st == 0 and (u, v) == (-1.0, -1.0) and ratio == 1.0
    C4 = np.full((D, D), 0.5)                          # a constant plane: arg-max (0, 0), on the ring
    assert M.peak_of(C4, R)[4] == M.STATUS["range"]
    C5 = np.full((D, D), 0.2)
    C5[3, 3] = C5[3, 4] = 0.9                          # the right neighbour equals the peak: half a pixel, still a fit
    u, v, peak, ratio, st = M.peak_of(C5, R)          # (a first arg-max has a smaller left and upper neighbour, so the
    assert st == 0 and abs(u - 0.5) < 1e-15 and v == 0.0   # fit's denominator is never 0: status 4 guards non-finite planes)


def test_single_pixel_arg():
    from torchpiv_amd import engine
    got = engine.single_pixel_arg(4, 1)
    assert got == {"radius": 4, "bin": (1, 1), "shift": (0, 0), "min_ratio": None}
    assert engine.single_pixel_arg(16, (1, 256), (-64, 64), 1.5, shape=(64, 256))["bin"] == (1, 256)
    assert engine.single_pixel_arg(np.int64(3), [16, 16])["bin"] == (16, 16)
    bad = [dict(radius=2), dict(radius=17), dict(radius=4.0), dict(radius=True), dict(bin=0), dict(bin=(1, 257)),
           dict(bin=(17, 16)), dict(bin=(1, 2, 3)), dict(bin=2.0), dict(bin=(1.0, 2)), dict(bin=None), dict(shift=(65, 0)),
           dict(shift=(0, -65)), dict(shift=(0.5, 0)), dict(shift=3), dict(min_ratio=0.5), dict(min_ratio=float("nan")),
           dict(min_ratio=float("inf")), dict(min_ratio="1.2"), dict(bin=(1, 128), shape=(64, 100)),
           dict(bin=(65, 1), shape=(64, 100))]
    for kw in bad:
        with pytest.raises(ValueError):
            engine.single_pixel_arg(**kw)
    assert engine.PIXEL_CORR_STATUS["ratio"] == 5 and engine.PIXEL_CORR_STATUS["masked"] == 6
    assert {k: v for k, v in engine.PIXEL_CORR_STATUS.items() if v < 5} == M.STATUS


def test_the_three_symbols_are_declared_bound_and_exported():
    from torchpiv_amd import _lib
    header = open(os.path.join(ROOT, "include", "torchpiv_hip.h")).read()
    for name in SYMBOLS:
        assert f" {name}(" in header, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib, name), name
    assert "#define TPIV_VERSION 2" in header and _lib.ABI_VERSION == 2
    # host-only: the byte query and its refusals
    f = _lib.lib.tpiv_pixel_corr_bytes
    assert f(37, 45, 2, 3, 8) == 18 * 15 * 17 * 17 * 8
    assert f(64, 264, 1, 128, 5) == 64 * 2 * 121 * 8
    for args in ((37, 45, 1, 1, 2), (37, 45, 1, 1, 17), (37, 45, 0, 1, 4), (37, 45, 1, 257, 4), (37, 45, 17, 16, 4),
                 (37, 45, 38, 1, 4), (37, 45, 1, 46, 4), (0, 45, 1, 1, 4)):
        assert f(*args) == 0, args


def test_model_accuracy_on_the_channel_scene():
    """u of the one-row bins against the constructed profile: bins (1, 128), 32 pairs, radius 5, the interior rows 5..58 of
    the second bin column (the first reaches the left edge: status border).  Measured here with seed 0: rms 0.0050 px, max
    0.0129 px (seeds 1..3: rms 0.0047..0.0061, max 0.0110..0.0172); the caps are 3 x the seed-0 values, 0.0150 and 0.0387 px.
    For orientation, without a gate: the first pass of the ensemble() model (tests/ensemble_model.py) at 16 / 8 on the same
    pairs: rms 0.22 px, max 0.42 px -- the gradient inside its windows, not the number of pairs."""
    A, B = M.scene()
    out = M.single_pixel(A, B, M.SCENE_BIN, M.SCENE_RADIUS)
    rows = M.interior_rows()
    assert (out["status"][:, 0] == M.STATUS["border"]).all()
    assert (out["status"][rows, 1] == 0).all() and (out["status"][:M.SCENE_RADIUS, 1] == M.STATUS["border"]).all()
    rms, worst = M.profile_error(out["u"][rows, 1], rows)
    v_rms = float(np.sqrt(np.mean(out["v"][rows, 1] ** 2)))
    import ensemble_model as E
    du, _, _ = E.ensemble_pass1(A, B, 16, 8)
    e = du - M.profile(np.arange(du.shape[0]) * 8 + 7.5)[:, None]
    print(f"  single pixel (1, 128) x 32 pairs: rms {rms:.4f} px, max {worst:.4f} px, v rms {v_rms:.4f} px; "
          f"ensemble 16/8 first pass: rms {math.sqrt(np.mean(e * e)):.3f} px, max {np.abs(e).max():.3f} px")
    assert rms <= CAP_RMS and worst <= CAP_MAX, (rms, worst)
    recorded = json.load(open(os.path.join(ROOT, "profiles", "single_pixel", "measurements.json")))["model_accuracy"]
    assert recorded["cap_rms_px"] == pytest.approx(CAP_RMS) and recorded["cap_max_px"] == pytest.approx(CAP_MAX)
