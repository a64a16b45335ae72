"""Tile-wise adaptive histogram equalization, the parts that need no GPU: the numpy model the device kernels are checked
against (tests/equalize_model.py) against the definition read literally and against the properties the definition
promises, the equalize= argument checked in the constructors before any device is touched, its place in the signatures,
and the new symbols in the header, the binding and the library."""
import inspect
import os
import re

import numpy as np
import pytest

import equalize_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dark(rng, shape):
    """A frame like a PIV image: most pixels in a few low bins, few bright ones."""
    return (rng.integers(0, 256, shape).astype(np.int64) ** 3 // (4 * 65536)).astype(np.uint8)


@pytest.mark.parametrize("H,W,tile", [(5, 7, 8), (13, 17, 8), (20, 33, 8), (9, 40, 16), (1, 1, 8), (30, 12, 8)])
def test_model_against_the_definition(H, W, tile):
    rng = np.random.default_rng(1000 * H + W)
    for f in (rng.integers(0, 256, (H, W)).astype(np.uint8), dark(rng, (H, W))):
        for clip_q8 in (256, 768, 4000, 65536):
            out, tabs = M.equalize(f, tile, clip_q8, return_luts=True)
            want, want_tabs, red = M.brute_force(f, tile, clip_q8)
            assert np.array_equal(out, want), (tile, clip_q8)
            assert np.array_equal(tabs[0], np.array(want_tabs, dtype=np.uint8))
            ey, ex = M.edges(H, tile), M.edges(W, tile)
            for ty in range(len(ey) - 1):
                for tx in range(len(ex) - 1):
                    t = f[ey[ty]:ey[ty + 1], ex[tx]:ex[tx + 1]]
                    lut = tabs[0, ty, tx].astype(int)
                    assert sum(red[ty][tx]) == t.size                           # sum h' = N
                    assert (np.diff(lut) >= 0).all()                            # monotone
                    assert not lut[:int(t.min()) + 1].any()                     # levels <= b0 map to 0
                    if t.min() == t.max():
                        assert not lut.any()                                    # a tile of one grey level maps to 0
                    else:
                        assert lut[int(t.max())] == 255 or clip_q8 < 65536      # without clipping the top level reaches 255


def test_redistribution_keeps_the_pixel_count():
    rng = np.random.default_rng(5)
    for N in (1, 64, 255, 256, 257, 4096, 146689):
        for _ in range(4):
            h = np.bincount(dark(rng, N), minlength=256)
            for clip_q8 in (256, 300, 768, 65535, 65536):
                lut, h2 = M.tile_lut(h, clip_q8)
                L = max(1, (clip_q8 * N) >> 16)
                E = int(np.maximum(h - L, 0).sum())
                assert h2.sum() == N and (h2 >= 0).all()
                assert (h2 - np.minimum(h, L) - E // 256).max() <= 1            # the remainder: at most one per bin
                assert (np.diff(lut.astype(int)) >= 0).all()
    # a remainder that is not zero: 99 of 100 pixels in one bin, L = 1 -> E = 98, r = 98, spread over 98 bins
    h = np.zeros(256, np.int64)
    h[7], h[200] = 99, 1
    lut, h2 = M.tile_lut(h, 256)
    assert h2.sum() == 100 and (h2 - np.minimum(h, 1)).sum() == 98 and (h2 - np.minimum(h, 1)).max() == 1


def test_constant_tiles_and_zero_background():
    for v in (0, 7, 255):
        assert not M.equalize(np.full((40, 50), v, np.uint8), 16, 768).any()
    # zeros stay zeros wherever every neighbour tile holds a zero
    rng = np.random.default_rng(3)
    f = dark(rng, (64, 96))
    f[rng.random(f.shape) < 0.3] = 0
    out = M.equalize(f, 16, 768)
    assert not out[f == 0].any() and out.max() > f.max()


def test_single_tile_without_clipping_is_plain_equalization():
    rng = np.random.default_rng(11)
    f = dark(rng, (40, 56)) + 3
    assert M.edges(40, 64) == [0, 40] and M.edges(56, 64) == [0, 56]
    out, tabs = M.equalize(f, 64, 65536, return_luts=True)
    # L = N: nothing is clipped, h' = h; the table is the cumulative histogram with the darkest level at 0, rounded
    h = np.bincount(f.ravel(), minlength=256)
    C = np.cumsum(h)
    b0 = int(f.min())
    d = f.size - C[b0]
    want = np.floor(255 * np.maximum(C - C[b0], 0) / d + 0.5).astype(np.uint8)
    assert np.array_equal(tabs[0, 0, 0], want)
    assert np.array_equal(out, want[f])
    assert out.min() == 0 and out.max() == 255


GRID = {  # n: edges at tile 16, 64, 256
    5: ([0, 5], [0, 5], [0, 5]),
    45: ([0, 15, 30, 45], [0, 45], [0, 45]),
    97: ([0, 16, 32, 48, 64, 80, 97], [0, 48, 97], [0, 97]),
    200: ([(i * 200) // 13 for i in range(14)], [0, 66, 133, 200], [0, 200]),
    264: ([(i * 264) // 17 for i in range(18)], [0, 66, 132, 198, 264], [0, 264]),
    300: ([(i * 300) // 19 for i in range(20)], [0, 60, 120, 180, 240, 300], [0, 300]),
}


@pytest.mark.parametrize("n", sorted(GRID))
def test_tile_grid(n):
    for tile, want in zip((16, 64, 256), GRID[n]):
        e = M.edges(n, tile)
        assert e == want, (n, tile)
        sizes = np.diff(e)
        assert sizes.max() - sizes.min() <= 1 and sizes.min() >= 1
        if len(e) > 2:
            assert 2 * tile <= 3 * sizes.min() and sizes.max() <= 2 * tile       # no sliver, none twice the aim
        i, w0, w1, D = M.axis_weights(n, tile)
        assert (w0 + w1 == D).all() and (w0 >= 0).all() and (w1 >= 0).all() and (np.diff(i) >= 0).all()
        if len(e) == 2:
            assert (D == 1).all() and (w0 == 1).all()
        else:
            c = np.array(e[:-1]) + np.array(e[1:])
            assert D.max() <= 640 and i.max() == len(e) - 3
            # in front of the first and behind the last centre one tile has all the weight; the blend is continuous
            assert (w1[2 * np.arange(n) + 1 <= c[0]] == 0).all() and (w0[2 * np.arange(n) + 1 >= c[-1]] == 0).all()


def test_intermediates_fit_32_bits_at_the_largest_tiles():
    # the largest tile (383 pixels along an axis: k == 1 at tile 256) and the widest blend (tiles of 320)
    assert M.edges(383, 256) == [0, 383] and M.edges(639, 256) == [0, 319, 639]
    f = np.zeros((383, 383), np.uint8)
    f[0, 0] = 255
    assert M.equalize(f, 256, 65536)[0, 0] == 255
    rng = np.random.default_rng(2)
    M.equalize(rng.integers(0, 256, (639, 639)).astype(np.uint8), 256, 768)   # (the model asserts its bounds)


BAD = ["CLAHE", "he", "", 64, 3.0, ("clahe",), ["clahe"], {}, True, {"tile": 7}, {"tile": 257}, {"tile": 64.0},
       {"tile": True}, {"tile": "64"}, {"tile": None}, {"clip": 0.99}, {"clip": 256.5}, {"clip": True}, {"clip": "3"},
       {"clip": None}, {"clip": float("nan")}, {"tile": 64, "clip": 3.0, "size": 5}, {"clip_q8": 768}, {"kind": "clahe"},
       {"tile": 64, "clip": -1}]
GOOD = [("clahe", {"tile": 64, "clip": 3.0, "clip_q8": 768}),
        ({"tile": 8}, {"tile": 8, "clip": 3.0, "clip_q8": 768}),
        ({"clip": 1}, {"tile": 64, "clip": 1.0, "clip_q8": 256}),
        ({"tile": np.int64(256), "clip": np.float32(256)}, {"tile": 256, "clip": 256.0, "clip_q8": 65536}),
        ({"tile": 100, "clip": 2.5}, {"tile": 100, "clip": 2.5, "clip_q8": 640}),
        ({"tile": 16, "clip": 1.001}, {"tile": 16, "clip": 1.001, "clip_q8": 256})]


def test_equalize_argument_is_checked_before_the_gpu(tmp_path):
    import torch
    from torchpiv_amd import backend as T
    from torchpiv_amd import engine, runner
    f = torch.zeros(2, 64, 64, dtype=torch.uint8)
    for bad in BAD:
        with pytest.raises(ValueError):
            engine.equalize_arg(bad)
        with pytest.raises(ValueError):
            T.OfflinePIV(str(tmp_path), "cpu", "bmp", 64, 32, equalize=bad)
        with pytest.raises(ValueError):
            runner.run_folder(str(tmp_path), "cpu", "bmp", 64, 32, equalize=bad)
        with pytest.raises(ValueError):
            T.ResidentPIV(f, f, 32, 16, equalize=bad)
    assert engine.equalize_arg(None) is None
    for good, norm in GOOD:
        got = engine.equalize_arg(good)
        assert got == norm and sorted(got) == ["clip", "clip_q8", "tile"]
        assert type(got["tile"]) is int and type(got["clip"]) is float and type(got["clip_q8"]) is int
        assert got["clip_q8"] == M.clip_q8_of(got["clip"])
        piv = T.OfflinePIV(str(tmp_path), "cpu", "bmp", 64, 32, equalize=good)
        assert len(piv) == 0 and list(piv()) == []
        assert runner.run_folder(str(tmp_path), "cpu", "bmp", 64, 32, equalize=good) == (None, 0)
        piv = T.OfflinePIV(str(tmp_path), "cpu", "bmp", 64, 32, equalize=good, prefilter={"cap": 200})
        assert len(piv) == 0
    # the tensor-level entry point has no CPU path
    with pytest.raises(RuntimeError):
        engine.equalize(f, 64, 3.0)
    for n, tile in ((200, 64), (264, 64), (5, 64), (97, 8), (1024, 64), (64, 256)):
        assert engine.equalize_grid(n, n, tile) == (len(M.edges(n, tile)) - 1,) * 2


def test_equalize_sits_directly_in_front_of_prefilter():
    from torchpiv_amd import backend as T
    from torchpiv_amd import runner
    for fn in (T.OfflinePIV.__init__, T.ResidentPIV.__init__, runner.run_folder):
        names = list(inspect.signature(fn).parameters)
        assert names[-2:] == ["equalize", "prefilter"], names
        assert inspect.signature(fn).parameters["equalize"].default is None


def test_equalize_symbols_in_header_binding_and_library():
    """tpiv_equalize and tpiv_equalize_work_bytes are declared in the header, bound in _lib.SIGNATURES and exported by the
    library; the ABI version stays 2; argument errors are decided on the host, before any launch."""
    import ctypes as C
    from torchpiv_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "torchpiv_hip.h")).read()
    assert re.search(r"\bint\s+tpiv_equalize\s*\(", hdr) and re.search(r"\bsize_t\s+tpiv_equalize_work_bytes\s*\(", hdr)
    for name, nargs in (("tpiv_equalize", 10), ("tpiv_equalize_work_bytes", 4)):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.SIGNATURES["tpiv_equalize_work_bytes"][0] is C.c_size_t
    assert _lib.ABI_VERSION == 2 and "#define TPIV_VERSION 2" in hdr and _lib.lib.tpiv_version() == 2
    wb = _lib.lib.tpiv_equalize_work_bytes
    assert wb(3, 200, 264, 64) == 3 * 3 * 4 * 256 and wb(1, 5, 300, 64) == 5 * 256 and wb(2, 97, 8, 8) == 2 * 12 * 256
    assert wb(2, 1024, 1024, 64) == 2 * 16 * 16 * 256 and wb(1, 64, 64, 256) == 256
    assert wb(1, 64, 64, 7) == 0 and wb(1, 64, 64, 257) == 0 and wb(0, 64, 64, 64) == 0 and wb(1, 0, 64, 64) == 0
    call = _lib.lib.tpiv_equalize
    fr, out, work, n, H, W = 1 << 20, 1 << 22, 1 << 24, 2, 32, 48
    need = wb(n, H, W, 16)
    assert need == 2 * 2 * 3 * 256
    for tile, clip_q8 in ((7, 768), (257, 768), (0, 768), (-64, 768), (64, 255), (64, 65537), (64, 0), (64, -768)):
        assert call(fr, n, H, W, tile, clip_q8, out, work, 1 << 20, None) == _lib.EINVAL, (tile, clip_q8)
    for shape in ((-1, H, W), (n, 0, W), (n, H, 0), (n, -H, W)):
        assert call(fr, *shape, 16, 768, out, work, 1 << 20, None) == _lib.EINVAL
    for args in ((None, out, work), (fr, None, work), (fr, out, None)):
        assert call(args[0], n, H, W, 16, 768, args[1], args[2], 1 << 20, None) == _lib.EINVAL
    # a workspace that is too small
    assert call(fr, n, H, W, 16, 768, out, work, need - 1, None) == _lib.EINVAL
    assert call(fr, n, H, W, 16, 768, out, work, 0, None) == _lib.EINVAL
    # out overlaps the frames in part: shifted by a frame, by a byte, by all but the last byte -- in place (out == frames)
    # is allowed and not tried here, it would launch
    for o in (fr + H * W, fr + 1, fr - 1, fr + n * H * W - 1, fr - n * H * W + 1):
        assert call(fr, n, H, W, 16, 768, o, work, need, None) == _lib.EINVAL
    with pytest.raises(ValueError, match="overlaps"):
        _lib.check(call(fr, n, H, W, 16, 768, fr + 1, work, need, None))
    # the workspace inside the frames or the output
    assert call(fr, n, H, W, 16, 768, out, fr + 5, need, None) == _lib.EINVAL
    assert call(fr, n, H, W, 16, 768, out, out + n * H * W - 1, need, None) == _lib.EINVAL
    assert call(fr, 0, H, W, 16, 768, out, work, 0, None) == _lib.OK            # no frames: nothing to do
