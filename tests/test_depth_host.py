"""Host side of depth= (no GPU): the argument check, the tone-map tables and the range rule against the numpy model
(tests/depth_model.py), and the uint16 decode next to the unchanged 8-bit one."""
import numpy as np
import pytest
import torch

import depth_model as M
from torchpiv_amd import engine
from torchpiv_amd import io as pio

RANGES = [(0, 65535), (0, 255), (0, 4080), (100, 101), (65534, 65535)]


def _random_ranges():
    rng = np.random.default_rng(20240607)
    out = []
    while len(out) < 200:
        lo, hi = sorted(int(x) for x in rng.integers(0, 65536, 2))
        if lo < hi:
            out.append((lo, hi))
    return out


# --------------------------------------------------------------------------------------------------------------------
# depth_arg
# --------------------------------------------------------------------------------------------------------------------
def test_depth_arg_accepts_and_normalises_every_documented_form():
    assert engine.depth_arg(None) is None
    assert engine.depth_arg({"lo": 0, "hi": 4095}) == {"lo": 0, "hi": 4095, "curve": "linear"}
    assert engine.depth_arg({"lo": np.int64(3), "hi": np.int32(9), "curve": "sqrt"}) == {"lo": 3, "hi": 9, "curve": "sqrt"}
    assert type(engine.depth_arg({"lo": np.int64(3), "hi": 9})["lo"]) is int
    auto = {"auto": True, "clip_low": 0.0, "clip_high": 1e-4, "sample": 32, "curve": "linear"}
    assert engine.depth_arg("auto") == auto
    assert engine.depth_arg({"auto": True}) == auto
    assert engine.depth_arg({"auto": True, "clip_low": 0.01, "clip_high": 0, "sample": 3, "curve": "sqrt"}) == \
        {"auto": True, "clip_low": 0.01, "clip_high": 0.0, "sample": 3, "curve": "sqrt"}
    table = (np.arange(65536) >> 8).astype(np.uint8)
    for given in (table, torch.from_numpy(table)):
        got = engine.depth_arg({"lut": given})
        assert sorted(got) == ["lut"] and isinstance(got["lut"], np.ndarray) and got["lut"].dtype == np.uint8
        assert np.array_equal(got["lut"], table)


@pytest.mark.parametrize("bad", [
    "linear", "Auto", 7, ["auto"], {},                                      # not a form at all / asks for nothing
    {"curve": "sqrt"},                                                     # a curve alone asks for nothing
    {"lo": 0, "hi": 10, "gamma": 2}, {"low": 0, "hi": 10},                # unknown keys
    {"lo": 0}, {"hi": 10},                                                 # half a range
    {"lo": 0, "hi": 10, "auto": True}, {"lo": 0, "hi": 10, "clip_low": 0.1}, {"lo": 0, "hi": 10, "sample": 4},   # mixed forms
    {"lut": np.zeros(65536, np.uint8), "curve": "sqrt"}, {"lut": np.zeros(65536, np.uint8), "lo": 0, "hi": 9},
    {"lut": np.zeros(65536, np.uint8), "auto": True},
    {"lo": True, "hi": 10}, {"lo": 0, "hi": True}, {"lo": 0.0, "hi": 10}, {"lo": 0, "hi": 10.0}, {"lo": "0", "hi": 10},
    {"lo": -1, "hi": 10}, {"lo": 0, "hi": 65536}, {"lo": 10, "hi": 10}, {"lo": 11, "hi": 10},
    {"lo": 0, "hi": 10, "curve": "log"}, {"lo": 0, "hi": 10, "curve": None}, {"auto": True, "curve": "gamma"},
    {"auto": False}, {"auto": 1}, {"auto": "yes"},
    {"auto": True, "clip_low": 0.5}, {"auto": True, "clip_high": 0.5}, {"auto": True, "clip_low": -1e-9},
    {"auto": True, "clip_high": True}, {"auto": True, "clip_low": "0.1"}, {"auto": True, "clip_high": float("nan")},
    {"auto": True, "sample": 0}, {"auto": True, "sample": 2.0}, {"auto": True, "sample": True},
    {"lut": np.zeros(65535, np.uint8)}, {"lut": np.zeros((256, 256), np.uint8)}, {"lut": np.zeros(65536, np.uint16)},
    {"lut": torch.zeros(65536, dtype=torch.int16)}, {"lut": list(range(10))}, {"lut": None},
], ids=repr)
def test_depth_arg_rejects(bad):
    with pytest.raises(ValueError, match="depth"):
        engine.depth_arg(bad)


def test_depth_arg_names_the_offender():
    with pytest.raises(ValueError, match="gamma"):
        engine.depth_arg({"lo": 0, "hi": 10, "gamma": 2})
    with pytest.raises(ValueError, match="auto"):
        engine.depth_arg({"lo": 0, "hi": 10, "auto": True})
    with pytest.raises(ValueError, match="clip_high"):
        engine.depth_arg({"auto": True, "clip_high": 0.7})
    with pytest.raises(ValueError, match="70000"):
        engine.depth_arg({"lo": 0, "hi": 70000})


# --------------------------------------------------------------------------------------------------------------------
# depth_lut
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", ["linear", "sqrt"])
def test_depth_lut_equals_model_and_is_a_tone_map(curve):
    for lo, hi in RANGES + _random_ranges():
        t = engine.depth_lut(lo, hi, curve)
        assert isinstance(t, np.ndarray) and t.dtype == np.uint8 and t.shape == (65536,)
        assert np.array_equal(t, M.lut(lo, hi, curve)), (lo, hi, curve)
        assert (np.diff(t.astype(np.int16)) >= 0).all(), (lo, hi, curve)            # monotone
        assert t[lo] == 0 and t[hi] == 255 and (t[:lo + 1] == 0).all() and (t[hi:] == 255).all(), (lo, hi, curve)


def test_depth_lut_linear_special_tables():
    assert np.array_equal(engine.depth_lut(0, 255)[:256], np.arange(256))         # the identity on 8-bit values
    assert np.array_equal(engine.depth_lut(0, 4080)[16 * np.arange(256)], np.arange(256))    # exactly v / 16 there
    assert np.array_equal(engine.depth_lut(0, 4080), engine.depth_lut(0, 4080, "linear"))
    for bad in ((5, 5), (-1, 3), (0, 65536), (True, 9)):
        with pytest.raises(ValueError):
            engine.depth_lut(*bad)
    with pytest.raises(ValueError):
        engine.depth_lut(0, 9, "cubic")


# --------------------------------------------------------------------------------------------------------------------
# depth_range
# --------------------------------------------------------------------------------------------------------------------
def _h(**bins):
    h = np.zeros(65536, np.int64)
    for k, c in bins.items():
        h[int(k[1:])] = c
    return h


def test_depth_range_equals_model_and_the_worked_cases():
    cases = []
    # an empty-tailed histogram: nothing above 4095, a step at 17
    h = np.zeros(65536, np.int64)
    h[17:4096] = 3
    cases += [(h, 0.0, 0.0, (17, 4095)), (h, 0.0, 1e-4, None), (h, 0.01, 0.01, None)]
    # single bins: the constant recording
    cases += [(_h(b0=50), 0.0, 1e-4, (0, 1)), (_h(b777=50), 0.0, 1e-4, (777, 778)), (_h(b65535=50), 0.0, 1e-4, (65534, 65535)),
              (_h(b65535=50), 0.3, 0.3, (65534, 65535)), (_h(b0=1), 0.0, 0.0, (0, 1))]
    # two bins, 10 samples at 100 and 990 at 5000 (N = 1000): floor(clip * N) against the 10
    two = _h(b100=10, b5000=990)
    cases += [(two, 0.0, 0.0, (100, 5000)),
              (two, 0.009, 0.0, (100, 5000)),       # 9 may be clipped: the 10 at 100 stay inside
              (two, 0.010, 0.0, (5000, 5001)),      # 10 may: the small bin falls below lo, and lo runs up to the next sample
              (two, 0.011, 0.0, (5000, 5001))]
    two_hi = _h(b100=990, b5000=10)
    cases += [(two_hi, 0.0, 0.0, (100, 5000)), (two_hi, 0.0, 0.009, (100, 5000)), (two_hi, 0.0, 0.010, (100, 101)),
              (two_hi, 0.0, 0.011, (100, 101)), (two_hi, 0.3, 0.3, (100, 101))]
    # a 12-bit-shaped histogram: dark pedestal, a tail of particle intensities up to 4095
    rng = np.random.default_rng(11)
    samples = np.concatenate([rng.normal(120, 15, 95000).clip(0, 4095), rng.uniform(150, 4095, 5000)]).astype(np.int64)
    h12 = np.bincount(samples, minlength=65536).astype(np.int64)
    cases += [(h12, 0.0, 1e-4, None), (h12, 1e-3, 1e-3, None), (h12, 0.0, 0.0, (int(samples.min()), int(samples.max()))),
              (h12, 0.49, 0.49, None)]
    for h, cl, ch, want in cases:
        got = engine.depth_range(h, cl, ch)
        assert got == M.range_(h, cl, ch), (cl, ch, got)
        if want is not None:
            assert got == want, (cl, ch, got, want)
        assert 0 <= got[0] < got[1] <= 65535 and all(type(x) is int for x in got)
    assert engine.depth_range(h12) == engine.depth_range(h12, 0.0, 1e-4)              # the defaults
    assert engine.depth_range(torch.from_numpy(h12).numpy().astype(np.uint64)) == engine.depth_range(h12)


def test_depth_range_refuses_an_empty_histogram_and_bad_arguments():
    with pytest.raises(ValueError, match="empty"):
        engine.depth_range(np.zeros(65536, np.int64))
    with pytest.raises(ValueError):
        engine.depth_range(np.ones(65535, np.int64))
    with pytest.raises(ValueError):
        engine.depth_range(np.ones(65536, np.float64))
    with pytest.raises(ValueError):
        engine.depth_range(np.ones(65536, np.int64), clip_low=0.5)
    with pytest.raises(ValueError):
        engine.depth_range(np.ones(65536, np.int64), clip_high=-0.1)


def test_depth_sample_spreads_over_the_recording():
    assert engine.depth_sample(4, 32).tolist() == [0, 1, 2, 3]
    assert engine.depth_sample(100, 1).tolist() == [0]
    assert engine.depth_sample(100, 3).tolist() == [0, 50, 99]
    for n, s in ((1000, 32), (33, 32), (7, 7)):
        want = np.unique(np.rint(np.linspace(0, n - 1, min(n, s))).astype(int))
        assert np.array_equal(engine.depth_sample(n, s), want)
    assert engine.depth_sample(0, 32).size == 0


# --------------------------------------------------------------------------------------------------------------------
# decode
# --------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def deep_image():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 65536, (37, 50)).astype(np.uint16)
    img[0, :4] = [0, 255, 256, 65535]
    return img


def test_imdecode_deep_keeps_16_bit_files_bit_for_bit(tmp_path, deep_image):
    from PIL import Image
    for name in ("f.png", "f.tif"):
        Image.fromarray(deep_image).save(tmp_path / name)
        with Image.open(tmp_path / name) as im:
            assert im.mode.startswith("I;16")
        got = pio.imdecode_deep(str(tmp_path / name))
        assert got.dtype == np.uint16 and got.dtype.isnative and got.flags.c_contiguous
        assert np.array_equal(got, deep_image)
        # the 8-bit decode of the same file is still the reference's value >> 8
        gray = pio.imdecode_gray(str(tmp_path / name))
        assert gray.dtype == np.uint8 and np.array_equal(gray, (deep_image >> 8).astype(np.uint8))
    # a 32-bit integer file goes through when its values fit 16 bits, and is refused when they do not
    Image.fromarray(deep_image.astype(np.int32), "I").save(tmp_path / "i32.tif")
    assert np.array_equal(pio.imdecode_deep(str(tmp_path / "i32.tif")), deep_image)
    wide = deep_image.astype(np.int32)
    wide[3, 3] = 65536
    Image.fromarray(wide, "I").save(tmp_path / "i32wide.tif")
    assert pio.imdecode_deep(str(tmp_path / "i32wide.tif")) is None


def test_imdecode_deep_widens_8_bit_files(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(4)
    g = rng.integers(0, 256, (20, 33)).astype(np.uint8)
    rgb = rng.integers(0, 256, (20, 33, 3)).astype(np.uint8)
    Image.fromarray(g, "L").save(tmp_path / "g.bmp")
    Image.fromarray(g, "L").save(tmp_path / "g.png")
    Image.fromarray(rgb, "RGB").save(tmp_path / "c.bmp")
    Image.fromarray(rgb, "RGB").save(tmp_path / "c.png")
    for name in ("g.bmp", "g.png", "c.bmp", "c.png"):
        deep, gray = pio.imdecode_deep(str(tmp_path / name)), pio.imdecode_gray(str(tmp_path / name))
        assert deep.dtype == np.uint16 and gray.dtype == np.uint8 and np.array_equal(deep, gray), name
    assert np.array_equal(pio.imdecode_deep(str(tmp_path / "g.bmp")), g)


def test_imdecode_deep_returns_none_for_an_unreadable_file(tmp_path):
    (tmp_path / "junk.png").write_bytes(b"this is not an image")
    assert pio.imdecode_deep(str(tmp_path / "junk.png")) is None
    assert pio.imdecode_deep(str(tmp_path / "missing.png")) is None


def test_dataset_and_staging_hand_out_uint16_under_deep(tmp_path, deep_image):
    from PIL import Image
    for k in range(4):
        Image.fromarray(np.roll(deep_image, k, axis=1)).save(tmp_path / f"im{k}.png")
    ds8 = pio.PIVDataset(str(tmp_path), "png", "pairs", transform=pio.ToTensor(dtype=torch.uint8))
    ds16 = pio.PIVDataset(str(tmp_path), "png", "pairs", transform=pio.ToTensor(dtype=torch.uint16), deep=True)
    a8, b8 = ds8[1]
    a16, b16 = ds16[1]
    assert a8.dtype == torch.uint8 and a16.dtype == torch.uint16 and len(ds8) == len(ds16) == 2
    assert np.array_equal(a16.numpy(), np.roll(deep_image, 2, axis=1)) and np.array_equal(b16.numpy(), np.roll(deep_image, 3, axis=1))
    assert np.array_equal(a8.numpy(), (np.roll(deep_image, 2, axis=1) >> 8).astype(np.uint8))
    # a staging slot under deep: headerless little-endian uint16 [H, W]; a slot must hold 2 * H * W bytes
    H, W = deep_image.shape
    cap = pio.slot_bytes(H, W, ds16.img_pairs[0], deep=True)
    assert cap >= 2 * H * W and cap % 4096 == 0
    slot = np.full(cap, 0xAB, np.uint8)
    lay = pio.stage_raw(str(tmp_path / "im2.png"), slot, H, W, deep=True)
    assert lay is not None and lay[0] == 0
    assert np.array_equal(slot[:2 * H * W].view("<u2").reshape(H, W), np.roll(deep_image, 2, axis=1))
    assert (slot[2 * H * W:] == 0xAB).all()
    assert pio.stage_raw(str(tmp_path / "im2.png"), slot[:2 * H * W - 1], H, W, deep=True) is None      # too small a slot
    assert pio.stage_raw(str(tmp_path / "im2.png"), slot, H, W + 1, deep=True) is None                   # another shape
