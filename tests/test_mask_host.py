"""Geometric mask, the parts that need no GPU: the mask= argument (engine.mask_arg) and the constructors that check it
before any device is touched, known answers of the numpy model the device kernels are checked against
(tests/mask_model.py), the new symbols in the header, the binding and the library, and the scene that motivates the
feature through the CPU oracle: a lit static band across a uniform flow."""
import os
import re

import numpy as np
import pytest
import torch

import mask_model as M
from mask_scene import FLOW, band_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

IMG = np.zeros((64, 64), np.uint8)
GOOD = [IMG, IMG.astype(bool), torch.from_numpy(IMG), torch.from_numpy(IMG).bool(), {"image": IMG},
        {"image": IMG, "threshold": 0}, {"image": IMG, "threshold": 1.0}, {"image": IMG, "threshold": np.float32(0.25)},
        {"image": IMG, "pixels": "keep"}, {"image": IMG, "pixels": "zero", "fill": float("nan")},
        {"image": IMG, "fill": -3}, {"image": IMG, "fill": np.float64(7.5), "threshold": 0.3}]
BAD = [IMG.astype(np.int32), IMG.astype(np.float32), IMG[0], IMG[None], torch.from_numpy(IMG).float(), "wall", 3, [IMG],
       {}, {"threshold": 0.5}, {"image": IMG, "limit": 3}, {"image": IMG, "threshold": -0.1},
       {"image": IMG, "threshold": 1.5}, {"image": IMG, "threshold": float("nan")}, {"image": IMG, "threshold": "0.5"},
       {"image": IMG, "threshold": True}, {"image": IMG, "pixels": "nan"}, {"image": IMG, "pixels": None},
       {"image": IMG, "fill": "nan"}, {"image": IMG, "fill": None}, {"image": IMG, "fill": True},
       {"image": np.zeros((0, 4), np.uint8)}]


def test_mask_arg_accepts_and_normalises():
    from torchpiv_amd.engine import MASK_DEFAULTS, mask_arg
    assert mask_arg(None) is None
    for good in GOOD:
        got = mask_arg(good)
        assert sorted(got) == ["fill", "image", "pixels", "threshold"]
        im = got["image"]
        assert isinstance(im, torch.Tensor) and im.dtype == torch.uint8 and tuple(im.shape) == (64, 64) and im.is_contiguous()
        assert isinstance(got["threshold"], float) and isinstance(got["fill"], float) and got["pixels"] in ("zero", "keep")
    got = mask_arg(IMG)
    assert (got["threshold"], got["pixels"], got["fill"]) == (0.5, "zero", 0.0) == tuple(MASK_DEFAULTS[k] for k in ("threshold", "pixels", "fill"))
    assert np.isnan(mask_arg({"image": IMG, "fill": float("nan")})["fill"])
    # non-zero means masked: a uint8 image keeps its bytes, a bool image becomes 0 / 1, a strided view is made contiguous
    img = np.zeros((6, 8), np.uint8)
    img[1, 2], img[3, 4], img[5, 7] = 1, 7, 255
    assert np.array_equal(mask_arg(img)["image"].numpy(), img)
    assert np.array_equal(mask_arg(img != 0)["image"].numpy(), (img != 0).astype(np.uint8))
    assert np.array_equal(mask_arg(np.asfortranarray(img))["image"].numpy(), img)
    assert np.array_equal(mask_arg(torch.from_numpy(img).t())["image"].numpy(), img.T)


@pytest.mark.parametrize("k", range(len(BAD)))
def test_mask_arg_rejects(k):
    from torchpiv_amd.engine import mask_arg
    with pytest.raises(ValueError):
        mask_arg(BAD[k])


def test_constructors_check_the_mask_before_any_device(tmp_path):
    """A bad mask raises ValueError in OfflinePIV, run_folder, ResidentPIV and engine.Plan on a machine without a GPU; a
    good one on an empty folder gives an empty run.  A mask of another shape than the frames raises too."""
    import torchpiv_amd as T
    from torchpiv_amd import engine, runner
    f = torch.zeros(2, 64, 64, dtype=torch.uint8)
    for bad in (BAD[0], BAD[2], BAD[5], BAD[10], BAD[11], BAD[16], BAD[18]):
        with pytest.raises(ValueError):
            T.OfflinePIV(str(tmp_path), "cpu", "bmp", 32, 16, mask=bad)
        with pytest.raises(ValueError):
            runner.run_folder(str(tmp_path), "cpu", "bmp", 32, 16, mask=bad)
        with pytest.raises(ValueError):
            T.ResidentPIV(f, f, 32, 16, mask=bad)
        with pytest.raises(ValueError):                           # engine.Plan checks it ahead of its own device check
            engine.Plan(64, 64, 32, 16, mask=bad)
    for good in (GOOD[0], GOOD[9]):
        piv = T.OfflinePIV(str(tmp_path), "cpu", "bmp", 32, 16, mask=good)
        assert len(piv) == 0 and list(piv()) == [] and piv.mask_grid() is None
        assert runner.run_folder(str(tmp_path), "cpu", "bmp", 32, 16, mask=good) == (None, 0)
    other = np.zeros((64, 48), np.uint8)
    with pytest.raises(ValueError, match="shape"):
        T.ResidentPIV(f, f, 32, 16, mask=other)
    with pytest.raises(ValueError, match="shape"):
        engine.Plan(64, 64, 32, 16, mask={"image": other, "fill": 1.0})
    # ... and for files: the shape of the first decodable pair
    from PIL import Image
    for name in ("image0_a.bmp", "image0_b.bmp"):
        Image.fromarray(np.zeros((64, 64), np.uint8), "L").save(tmp_path / name)
    with pytest.raises(ValueError, match="shape"):
        T.OfflinePIV(str(tmp_path), "cpu", "bmp", 32, 16, mask=other)
    with pytest.raises(ValueError, match="shape"):
        runner.run_folder(str(tmp_path), "cpu", "bmp", 32, 16, mask=other)


def test_model_all_ones_counts_the_whole_window():
    for (H, W), ws, ov in (((97, 131), 8, 0), ((97, 131), 33, 16), ((97, 131), 42, 21), ((64, 64), 64, 32)):
        c = M.coverage(np.full((H, W), 9, np.uint8), ws, ov)
        assert c.shape == tuple(M.field_shape(H, W, ws, ov)) and c.dtype == np.int32 and (c == ws * ws).all()
        assert not M.grid(c, ws, 1.0).any() and M.grid(c, ws, 0.5).all() and M.grid(c, ws, 0.0).all()
        z = M.coverage(np.zeros((H, W), np.uint8), ws, ov)
        assert (z == 0).all() and not M.grid(z, ws, 0.0).any()


def test_model_single_pixel_is_counted_by_the_windows_that_contain_it():
    H, W = 97, 131
    for ws, ov in ((8, 0), (8, 4), (16, 8), (33, 16), (42, 21)):
        step = ws - ov
        nr, nc = M.field_shape(H, W, ws, ov)
        for y, x in ((0, 0), (H - 1, W - 1), (40, 77), (ws - 1, step), (step, ws)):
            m = np.zeros((H, W), np.uint8)
            m[y, x] = 200
            want = np.zeros((nr, nc), np.int32)
            for i in range(nr):
                for j in range(nc):
                    want[i, j] = i * step <= y < i * step + ws and j * step <= x < j * step + ws
            got = M.coverage(m, ws, ov)
            assert np.array_equal(got, want), (ws, ov, y, x)
            if (y, x) == (40, 77):                 # an interior pixel: one window without overlap, four at half overlap
                assert got.sum() == (1 if ov == 0 else 4 if 2 * ov == ws else got.sum()) >= 1


def test_model_grid_limit_is_one_truncated_product():
    c = np.arange(0, 1100, dtype=np.int32).reshape(1, -1)
    assert np.array_equal(M.grid(c, 33, 0.5), c > 544)            # int(0.5 * 1089) = 544
    assert np.array_equal(M.grid(c, 32, 0.3), c > 307)            # int(307.2)
    assert np.array_equal(M.grid(c, 32, 1.0), c > 1024)


def test_model_apply_and_fields():
    rng = np.random.default_rng(0)
    f = rng.integers(0, 256, (3, 5, 7), dtype=np.uint8)
    m = rng.choice(np.array([0, 1, 7, 255], np.uint8), (5, 7))
    out = M.apply(f, m)
    assert out.dtype == np.uint8 and (out[:, m != 0] == 0).all() and np.array_equal(out[:, m == 0], f[:, m == 0])
    u = rng.normal(size=(2, 5, 7))
    u[0, 1, 1] = np.nan
    g = np.zeros((5, 7), bool)
    g[1, 1] = g[4, 6] = True
    uu, vv, ii, st = M.fields(u, -u, np.ones((2, 5, 7), np.uint8), g, 0, status=np.full((2, 5, 7), 1, np.uint8))
    assert (uu[:, g].view(np.uint64) == 0).all() and (vv[:, g].view(np.uint64) == 0).all()        # +0.0, bit for bit
    assert (ii[:, g] == 0).all() and (ii[:, ~g] == 1).all() and (st[:, g] == 2).all() and (st[:, ~g] == 1).all()
    assert np.array_equal(uu[:, ~g], u[:, ~g]) and np.isnan(u[0, 1, 1])                           # the input is not written


def test_mask_symbols_in_header_binding_and_library():
    """The five new entry points are declared in the header, bound in _lib.SIGNATURES and exported by the built library
    (getattr on the CDLL looks the symbol up)."""
    from torchpiv_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "torchpiv_hip.h")).read()
    for name, nargs in (("tpiv_apply_mask", 6), ("tpiv_mask_coverage", 7), ("tpiv_mask_fields", 10),
                        ("tpiv_plan_set_mask", 4), ("tpiv_plan_pass_mask", 3)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name) and len(_lib.SIGNATURES[name][1]) == nargs


# ---------------------------------------------------------------------------------------------------------------------
# the scene: a static lit band across a uniform flow, through the CPU oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_band_scene_through_the_oracle():
    """The table of the feature's motivation: mean distance from the flow per grid row of a 32/16 first pass, on the clean
    frames, with the band and with the band's pixels zeroed.  Asserted: the rows touching the band are 5...9 with 288, 800,
    1024, 608 and 96 masked pixels per window, the excluded rows at threshold 0.5 are 6, 7, 8, and zeroing brings the
    partly covered rows 5 and 9 at least 0.3 px nearer the flow."""
    from oracle import piv_oracle as O
    a, b, wa, wb, mask = band_scene()
    count = M.coverage(mask, 32, 16)
    assert count.shape == (15, 15) and (count == count[:, :1]).all()
    assert count[:, 0].tolist() == [0] * 5 + [288, 800, 1024, 608, 96] + [0] * 5
    excluded = M.grid(count, 32, 0.5)
    assert np.flatnonzero(excluded[:, 0]).tolist() == [6, 7, 8] and (excluded == excluded[:, :1]).all()

    def rows(fa, fb):
        u, v = O.pass1(fa, fb, 32, 16)[:2]
        return np.hypot(u - FLOW[0], v - FLOW[1]).mean(axis=1)
    clean, band, zeroed = rows(a, b), rows(wa, wb), rows(M.apply(wa, mask), M.apply(wb, mask))
    print("band scene, mean distance from the flow per row: clean", np.round(clean, 2), "band", np.round(band, 2),
          "zeroed", np.round(zeroed, 2))
    for r in (5, 9):
        assert band[r] - zeroed[r] >= 0.3, (r, band[r], zeroed[r])
    away = [r for r in range(15) if not 5 <= r <= 9]
    assert np.array_equal(band[away], clean[away]) and np.array_equal(zeroed[away], clean[away])
    assert (band[6:9] > 2.0).all() and (clean < 0.3).all()
