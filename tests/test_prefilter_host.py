"""Spatial pre-filters, the parts that need no GPU: known answers of the numpy model the device kernel is checked against
(tests/prefilter_model.py), the model against the definition read literally, the prefilter= argument checked in the
constructors before any device is touched, and the new symbol in the header and the binding."""
import os
import re

import numpy as np
import pytest

from prefilter_model import brute_force, counts, prefilter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lone_bright_pixel_on_a_pedestal():
    f = np.full((7, 9), 40, np.uint8)
    f[3, 4] = 200
    want = np.zeros((7, 9), np.uint8)
    want[3, 4] = 160
    assert np.array_equal(prefilter(f, "min", 3), want)
    assert np.array_equal(prefilter(f, "min", 63), want)
    # mean, size 3: S = 8 * 40 + 200 = 520 around the pixel and at its eight neighbours, m = (1040 + 9) // 18 = 58
    want[3, 4] = 142
    assert np.array_equal(prefilter(f, "mean", 3), want)
    # a background below the pedestal leaves a lower pedestal; one above it leaves the pixel alone
    bg = np.full((7, 9), 15, np.uint8)
    want[3, 4] = 160
    assert np.array_equal(prefilter(f, "min", 5, background=bg), want)
    bg[:] = 90
    want[3, 4] = 110
    assert np.array_equal(prefilter(f, "min", 5, background=bg), want)
    assert np.array_equal(prefilter(f, None, cap=255, background=bg), want)
    # a stack is filtered frame by frame
    assert np.array_equal(prefilter(np.stack([f, f[::-1]]), "min", 3, background=bg), np.stack([want, want[::-1]]))


def test_ramp():
    f = np.tile((10 * np.arange(9)).astype(np.uint8), (5, 1))
    # min, size 3: the neighbourhood's minimum is the column to the left (clipped: the pixel's own column at x = 0)
    want = np.full((5, 9), 10, np.uint8)
    want[:, 0] = 0
    assert np.array_equal(prefilter(f, "min", 3), want)
    # mean, size 3: the mean of a ramp is its centre inside; at x = 8 it is 75 (columns 7, 8), at x = 0 it is 5 > 0
    want = np.zeros((5, 9), np.uint8)
    want[:, 8] = 5
    assert np.array_equal(prefilter(f, "mean", 3), want)


def test_image_smaller_than_the_window():
    f = np.array([[10, 20], [30, 50]], np.uint8)
    assert np.array_equal(counts(2, 2, 31), np.full((2, 2), 4))
    assert np.array_equal(prefilter(f, "min", 63), [[0, 10], [20, 40]])
    # S = 110, c = 4: m = (220 + 4) // 8 = 28
    assert np.array_equal(prefilter(f, "mean", 63), [[0, 0], [2, 22]])


def test_mean_rounds_half_up():
    # c = 2, S = 7: 2S + c = 16 = 4 * 2c exactly -- the mean 3.5 becomes 4
    assert np.array_equal(prefilter(np.array([[3, 4]], np.uint8), "mean", 3), [[0, 0]])
    assert np.array_equal(prefilter(np.array([[3, 9]], np.uint8), "mean", 3), [[0, 3]])          # mean 6
    # c = 3: S = 8 -> (16 + 3) // 6 = 3 (2.67 up), S = 7 -> 17 // 6 = 2 (2.33 down); the ends have c = 2
    assert np.array_equal(prefilter(np.array([[1, 3, 4]], np.uint8), "mean", 3), [[0, 0, 0]])    # m = 2, 3, 4
    assert np.array_equal(prefilter(np.array([[1, 5, 1]], np.uint8), "mean", 3), [[0, 3, 0]])    # m = 3, 2, 3
    assert np.array_equal(prefilter(np.array([[4, 5, 1]], np.uint8), "mean", 3), [[0, 2, 0]])    # m = 5 (4.5 up), 3, 3
    assert np.array_equal(counts(1, 3, 1), [[2, 3, 2]])


def test_cap_comes_last():
    f = np.full((7, 9), 40, np.uint8)
    f[3, 4] = 200
    f[1, 1] = 90
    got = prefilter(f, "min", 3, cap=100)
    assert got[3, 4] == 100 and got[1, 1] == 50 and got.sum() == 150
    assert np.array_equal(prefilter(f, None, cap=60), np.minimum(f, 60))
    bg = np.full((7, 9), 30, np.uint8)
    assert np.array_equal(prefilter(f, None, cap=60, background=bg), np.minimum(f - 30, 60))
    assert prefilter(f, "mean", 3, cap=1).max() == 1


@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (9, 4), (13, 17)])
def test_model_against_the_definition(H, W):
    rng = np.random.default_rng(H * 100 + W)
    f = rng.integers(0, 256, (H, W)).astype(np.uint8)
    bg = rng.integers(0, 120, (H, W)).astype(np.uint8)
    for kind in ("min", "mean"):
        for size in (3, 5, 15, 63):
            for b in (None, bg):
                for cap in (None, 37):
                    assert np.array_equal(prefilter(f, kind, size, cap, b), brute_force(f, kind, size, cap, b)), \
                        (kind, size, cap, b is not None)
    assert np.array_equal(prefilter(f, None, cap=99, background=bg), brute_force(f, None, cap=99, background=bg))
    # saturated and empty frames
    for v in (0, 255):
        c = np.full((H, W), v, np.uint8)
        assert not prefilter(c, "min", 5).any() and not prefilter(c, "mean", 5).any()


BAD = ["min", "mean", 15, ("min", 15), {}, {"kind": None}, {"kind": None, "size": 15}, {"kind": "min"},
       {"kind": "median", "size": 5}, {"kind": "min", "size": 4}, {"kind": "min", "size": 1}, {"kind": "mean", "size": 65},
       {"kind": "min", "size": 5.0}, {"kind": "min", "size": True}, {"kind": "min", "size": 5, "cap": 0},
       {"kind": "min", "size": 5, "cap": 256}, {"cap": 1.5}, {"cap": -3}, {"kind": "min", "size": 5, "radius": 2},
       {"kind": 1, "size": 5}, {"size": 5}, {"kind": None, "size": 4, "cap": 9}]
GOOD = [({"kind": "min", "size": 15}, {"kind": "min", "size": 15, "cap": None}),
        ({"kind": "mean", "size": 3, "cap": 200}, {"kind": "mean", "size": 3, "cap": 200}),
        ({"kind": "mean", "size": np.int64(63), "cap": None}, {"kind": "mean", "size": 63, "cap": None}),
        ({"cap": 120}, {"kind": None, "size": None, "cap": 120}),
        ({"kind": None, "cap": np.uint8(255)}, {"kind": None, "size": None, "cap": 255}),
        ({"kind": None, "size": 7, "cap": 1}, {"kind": None, "size": None, "cap": 1})]


def test_prefilter_argument_is_checked_before_the_gpu(tmp_path):
    import torch
    from torchpiv_amd import backend as T
    from torchpiv_amd import engine, runner
    f = torch.zeros(2, 64, 64, dtype=torch.uint8)
    for bad in BAD:
        with pytest.raises(ValueError):
            engine.prefilter_arg(bad)
        with pytest.raises(ValueError):
            T.OfflinePIV(str(tmp_path), "cpu", "bmp", 64, 32, prefilter=bad)
        with pytest.raises(ValueError):
            runner.run_folder(str(tmp_path), "cpu", "bmp", 64, 32, prefilter=bad)
        with pytest.raises(ValueError):
            T.ResidentPIV(f, f, 32, 16, prefilter=bad)
    assert engine.prefilter_arg(None) is None
    for good, norm in GOOD:
        assert engine.prefilter_arg(good) == norm
        assert all(v is None or type(v) in (int, str) for v in engine.prefilter_arg(good).values())
        piv = T.OfflinePIV(str(tmp_path), "cpu", "bmp", 64, 32, prefilter=good)
        assert len(piv) == 0 and list(piv()) == []
        assert runner.run_folder(str(tmp_path), "cpu", "bmp", 64, 32, prefilter=good) == (None, 0)
    # the keyword comes after the existing ones
    import inspect
    for fn in (T.OfflinePIV.__init__, T.ResidentPIV.__init__, runner.run_folder):
        assert list(inspect.signature(fn).parameters)[-1] == "prefilter"


def test_prefilter_symbol_in_header_and_binding():
    """tpiv_prefilter is declared in the header with its three kinds, bound in _lib.SIGNATURES and exported by the library;
    the ABI version stays 2; argument errors are decided on the host, before any launch."""
    from torchpiv_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "torchpiv_hip.h")).read()
    assert re.search(r"\bint\s+tpiv_prefilter\s*\(", hdr)
    assert "tpiv_prefilter" in _lib.SIGNATURES and hasattr(_lib.lib, "tpiv_prefilter")
    assert len(_lib.SIGNATURES["tpiv_prefilter"][1]) == 10
    for name, val in (("NONE", 0), ("MIN", 1), ("MEAN", 2)):
        assert re.search(rf"\bTPIV_PREFILTER_{name}\s*=\s*{val}\b", hdr)
        assert getattr(_lib, f"PREFILTER_{name}") == val
    assert _lib.ABI_VERSION == 2 and "#define TPIV_VERSION 2" in hdr
    call = _lib.lib.tpiv_prefilter
    fr, out, n, H, W = 1 << 20, 1 << 22, 2, 32, 48
    for kind, size, cap in ((3, 5, 255), (-1, 5, 255), (1, 4, 255), (1, 1, 255), (2, 65, 255), (1, 5, 0), (0, 0, 256),
                            (2, 5, -1)):
        assert call(fr, n, H, W, None, kind, size, cap, out, None) == _lib.EINVAL, (kind, size, cap)
    for shape in ((-1, H, W), (n, 0, W), (n, H, 0)):
        assert call(fr, *shape, None, 1, 5, 255, out, None) == _lib.EINVAL
    assert call(None, n, H, W, None, 1, 5, 255, out, None) == _lib.EINVAL
    assert call(fr, n, H, W, None, 1, 5, 255, None, None) == _lib.EINVAL
    # out overlaps the frames: itself, shifted by a frame, by the last byte; or the background
    for o in (fr, fr + H * W, fr + n * H * W - 1, fr - n * H * W + 1):
        assert call(fr, n, H, W, None, 1, 5, 255, o, None) == _lib.EINVAL
        assert call(fr, n, H, W, None, 0, 0, 9, o, None) == _lib.EINVAL
    assert call(fr, n, H, W, out + 5, 2, 5, 255, out, None) == _lib.EINVAL
    with pytest.raises(ValueError, match="overlaps"):
        _lib.check(call(fr, n, H, W, None, 1, 5, 255, fr, None))
    assert call(fr, 0, H, W, None, 1, 5, 255, out, None) == _lib.OK          # no frames: nothing to do
