"""Per-pair masks, the parts that need no GPU: the dynamic_mask= argument (engine.dynamic_mask_arg) and the constructors
that check it, the place of the keyword in the three signatures, the new symbols in the header, the binding and the
library, the properties of the brute-force model of the segmentation (tests/dynmask_model.py), and the scenes that
motivate the feature through the CPU oracle's first pass."""
import inspect
import os

import numpy as np
import pytest
import torch

import dynmask_model as D
import dynmask_scene as S
import mask_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = {"kind": "bright", "size": 7, "level": 40}
IMG = np.zeros((64, 64), np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# the argument
# ---------------------------------------------------------------------------------------------------------------------
def test_dynamic_mask_arg_accepts_and_normalises():
    from torchpiv_amd.engine import MASK_DEFAULTS, dynamic_mask_arg
    assert dynamic_mask_arg(None) is None and dynamic_mask_arg(None, mask=IMG) is None
    got = dynamic_mask_arg(SEG)
    assert got == dict(SEG, grow=0, **MASK_DEFAULTS)
    got = dynamic_mask_arg({"kind": "dark", "size": np.int64(21), "level": np.uint8(14), "grow": 3, "threshold": 0.25,
                            "pixels": "keep", "fill": float("nan")})
    assert (got["kind"], got["size"], got["level"], got["grow"]) == ("dark", 21, 14, 3)
    assert all(type(got[k]) is int for k in ("size", "level", "grow"))
    assert got["threshold"] == 0.25 and got["pixels"] == "keep" and np.isnan(got["fill"])
    # the limits: size 3 and 63, level 0 and 255, size // 2 + grow == 31
    for ok in ({"size": 3, "grow": 30}, {"size": 63, "grow": 0}, {"size": 61, "grow": 1}, {"level": 0}, {"level": 255}):
        dynamic_mask_arg(dict(SEG, **ok))
    # with mask=, its three values apply -- as given and as mask_arg returned it
    from torchpiv_amd.engine import mask_arg
    for static in ({"image": IMG, "threshold": 0.1, "fill": 7.5, "pixels": "keep"},
                   mask_arg({"image": IMG, "threshold": 0.1, "fill": 7.5, "pixels": "keep"})):
        got = dynamic_mask_arg(SEG, mask=static)
        assert (got["threshold"], got["fill"], got["pixels"]) == (0.1, 7.5, "keep")
    # the stack form: uint8 or bool, numpy or tensor, any strides
    st = (np.arange(2 * 4 * 6).reshape(2, 4, 6) % 3).astype(np.uint8)
    for form in (st, st != 0, torch.from_numpy(st), np.asfortranarray(st)):
        got = dynamic_mask_arg({"stack": form, "fill": 1.0})
        assert got["stack"].dtype == torch.uint8 and got["stack"].is_contiguous() and "kind" not in got
        assert np.array_equal(got["stack"].numpy() != 0, st != 0) and got["fill"] == 1.0


BAD = {
    "string": "bright",
    "image": IMG,
    "empty": {},
    "unknown_key": dict(SEG, radius=3),
    "no_kind": {"size": 7, "level": 40},
    "no_size": {"kind": "bright", "level": 40},
    "no_level": {"kind": "bright", "size": 7},
    "kind": dict(SEG, kind="edge"),
    "kind_type": dict(SEG, kind=0),
    "size_even": dict(SEG, size=8),
    "size_small": dict(SEG, size=1),
    "size_large": dict(SEG, size=65),
    "size_float": dict(SEG, size=7.0),
    "size_bool": dict(SEG, size=True),
    "level_low": dict(SEG, level=-1),
    "level_high": dict(SEG, level=256),
    "level_float": dict(SEG, level=40.0),
    "grow_negative": dict(SEG, grow=-1),
    "grow_too_far": dict(SEG, size=7, grow=29),
    "grow_float": dict(SEG, grow=1.0),
    "threshold": dict(SEG, threshold=1.5),
    "pixels": dict(SEG, pixels="blank"),
    "fill": dict(SEG, fill="nan"),
    "stack_and_kind": {"stack": np.zeros((2, 4, 4), np.uint8), "kind": "bright"},
    "stack_dtype": {"stack": np.zeros((2, 4, 4), np.float32)},
    "stack_rank": {"stack": np.zeros((4, 4), np.uint8)},
    "stack_empty": {"stack": np.zeros((0, 4, 4), np.uint8)},
    "stack_type": {"stack": [[0]]},
}


@pytest.mark.parametrize("k", sorted(BAD))
def test_dynamic_mask_arg_rejects(k):
    from torchpiv_amd.engine import dynamic_mask_arg
    with pytest.raises(ValueError):
        dynamic_mask_arg(BAD[k])


def test_threshold_pixels_and_fill_live_with_mask_when_it_is_given():
    from torchpiv_amd.engine import dynamic_mask_arg
    for key, val in (("threshold", 0.5), ("pixels", "zero"), ("fill", 0.0)):
        with pytest.raises(ValueError):
            dynamic_mask_arg(dict(SEG, **{key: val}), mask=IMG)
        dynamic_mask_arg(dict(SEG, **{key: val}), mask=None)
    with pytest.raises(ValueError):
        dynamic_mask_arg({"stack": np.zeros((2, 4, 4), np.uint8)}, stack=False)
    with pytest.raises(ValueError):
        dynamic_mask_arg(SEG, mask=np.zeros((4, 4), np.float32))      # a bad mask= is still a bad mask=


def test_constructors_check_the_argument_before_any_device(tmp_path):
    """Every error is raised in the constructor on a machine without a GPU; a good argument on an empty folder gives an
    empty run.  The stack form is ResidentPIV's alone, and its shape is the frames'."""
    import torchpiv_amd as T
    from torchpiv_amd import runner
    f = torch.zeros(2, 64, 64, dtype=torch.uint8)
    stack = np.zeros((2, 64, 64), np.uint8)
    for bad in (BAD["size_even"], BAD["unknown_key"], BAD["string"], dict(SEG, fill="x")):
        with pytest.raises(ValueError):
            T.OfflinePIV(str(tmp_path), "cpu", "bmp", 32, 16, dynamic_mask=bad)
        with pytest.raises(ValueError):
            runner.run_folder(str(tmp_path), "cpu", "bmp", 32, 16, dynamic_mask=bad)
        with pytest.raises(ValueError):
            T.ResidentPIV(f, f, 32, 16, dynamic_mask=bad)
    for make in (lambda **kw: T.OfflinePIV(str(tmp_path), "cpu", "bmp", 32, 16, **kw),
                 lambda **kw: runner.run_folder(str(tmp_path), "cpu", "bmp", 32, 16, **kw),
                 lambda **kw: T.ResidentPIV(f, f, 32, 16, **kw)):
        with pytest.raises(ValueError):
            make(dynamic_mask=dict(SEG, fill=1.0), mask=IMG)
    for make in (lambda **kw: T.OfflinePIV(str(tmp_path), "cpu", "bmp", 32, 16, **kw),
                 lambda **kw: runner.run_folder(str(tmp_path), "cpu", "bmp", 32, 16, **kw)):
        with pytest.raises(ValueError):
            make(dynamic_mask={"stack": stack})
    for other in (np.zeros((3, 64, 64), np.uint8), np.zeros((2, 64, 32), np.uint8)):
        with pytest.raises(ValueError):
            T.ResidentPIV(f, f, 32, 16, dynamic_mask={"stack": other})
    piv = T.OfflinePIV(str(tmp_path), "cpu", "bmp", 32, 16, dynamic_mask=dict(SEG, fill=float("nan")), mask=None)
    assert len(piv) == 0 and list(piv()) == []
    assert runner.run_folder(str(tmp_path), "cpu", "bmp", 32, 16, dynamic_mask=SEG, mask=IMG) == (None, 0)
    with pytest.raises(ValueError):
        piv.ensemble()


def test_the_keyword_stands_behind_weighting_in_the_three_signatures():
    import torchpiv_amd as T
    from torchpiv_amd import engine, runner
    for fn in (T.OfflinePIV.__init__, T.ResidentPIV.__init__, runner.run_folder):
        names = list(inspect.signature(fn).parameters)
        k = names.index("dynamic_mask")
        assert names[k - 1] == "weighting" and names[k - 2] == "correlation", names
        assert names[-2:] == ["equalize", "prefilter"] and names[k + 1] == "equalize"
        assert inspect.signature(fn).parameters["dynamic_mask"].default is None
    # Plan and debug_pass get no new parameter
    assert list(inspect.signature(engine.Plan.__init__).parameters)[-1] == "correlation"
    assert list(inspect.signature(engine.debug_pass).parameters)[-1] == "correlation"
    assert "dynamic_mask" not in inspect.signature(engine.Plan.__init__).parameters


ENTRIES = (("tpiv_dynamic_mask", 13), ("tpiv_dynamic_mask_work_bytes", 3), ("tpiv_apply_mask_pairs", 6),
           ("tpiv_mask_coverage_pairs", 8), ("tpiv_mask_fields_pairs", 10), ("tpiv_plan_set_pair_masks", 2),
           ("tpiv_plan_run_masked", 10), ("tpiv_plan_pass_pair_mask", 3))


def test_symbols_in_header_binding_and_library():
    import re
    from torchpiv_amd import _lib
    with open(os.path.join(ROOT, "include", "torchpiv_hip.h")) as fh:
        header = fh.read()
    assert "#define TPIV_VERSION 2" in header and _lib.ABI_VERSION == 2
    for name, nargs in ENTRIES:
        decl = re.search(r"^(?:int|size_t) " + name + r"\(([^;]*?)\);", header, re.S | re.M)      # the declaration, not a comment
        assert decl is not None, name
        assert len([a for a in decl.group(1).split(",") if a.strip()]) == nargs, (name, decl.group(1))
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.DYNMASKS == {"bright": 0, "dark": 1}
    assert "TPIV_DYNMASK_BRIGHT = 0" in header and "TPIV_DYNMASK_DARK = 1" in header


def test_host_side_checks_of_the_library_need_no_device():
    """The workspace size, and the refusals that are decided before anything is launched."""
    from torchpiv_amd import _lib
    lib = _lib.lib
    assert lib.tpiv_dynamic_mask_work_bytes(3, 70, 200) == 3 * 70 * 200
    for bad in ((0, 70, 200), (-1, 70, 200), (3, 0, 200), (3, 70, 0)):
        assert lib.tpiv_dynamic_mask_work_bytes(*bad) == 0
    p = 4096                                                           # (never dereferenced: every call is refused)
    for kind, size, level, grow in ((2, 7, 40, 0), (-1, 7, 40, 0), (0, 8, 40, 0), (0, 1, 40, 0), (0, 65, 40, 0),
                                    (0, 7, -1, 0), (0, 7, 256, 0), (0, 7, 40, -1), (0, 7, 40, 29), (0, 63, 40, 1)):
        assert lib.tpiv_dynamic_mask(p, 2 * p, 1, 16, 16, kind, size, level, grow, None, 3 * p, 4 * p, None) == _lib.EINVAL
    for n, H, W in ((-1, 16, 16), (1, 0, 16), (1, 16, 0)):
        assert lib.tpiv_dynamic_mask(p, 2 * p, n, H, W, 0, 7, 40, 0, None, 3 * p, 4 * p, None) == _lib.EINVAL
    assert lib.tpiv_dynamic_mask(p, 2 * p, 1, 16, 16, 0, 7, 40, 0, None, None, 4 * p, None) == _lib.EINVAL      # null
    assert lib.tpiv_dynamic_mask(p, 2 * p, 1, 16, 16, 0, 7, 40, 0, None, p + 8, 4 * p, None) == _lib.EINVAL     # overlap
    assert lib.tpiv_dynamic_mask(p, 2 * p, 1, 16, 16, 0, 7, 40, 0, None, 3 * p, 3 * p, None) == _lib.EINVAL     # overlap
    assert lib.tpiv_dynamic_mask(None, None, 0, 16, 16, 0, 7, 40, 0, None, None, None, None) == _lib.OK          # n == 0
    assert lib.tpiv_apply_mask_pairs(p, -1, 256, 2 * p, 3 * p, None) == _lib.EINVAL
    assert lib.tpiv_apply_mask_pairs(p, 1, 256, 2 * p, p + 8, None) == _lib.EINVAL                               # partial
    assert lib.tpiv_apply_mask_pairs(p, 1, 256, 2 * p, 2 * p, None) == _lib.EINVAL                               # out == masks
    assert lib.tpiv_apply_mask_pairs(None, 0, 256, None, None, None) == _lib.OK
    assert lib.tpiv_mask_coverage_pairs(p, 1, 64, 64, 4, 0, 2 * p, None) == _lib.EUNSUPPORTED
    assert lib.tpiv_mask_fields_pairs(p, p, p, None, p, 1, 4, 4, 2, None) == _lib.EINVAL
    assert lib.tpiv_plan_set_pair_masks(None, 1) == _lib.EINVAL
    assert lib.tpiv_plan_run_masked(None, p, p, p, 0.5, 1, p, p, p, None) == _lib.EINVAL


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bright", "dark"])
@pytest.mark.parametrize("k", [3, 7, 21])
def test_a_bar_narrower_than_the_size_vanishes_and_one_as_wide_comes_back_whole(kind, k):
    level = 100
    fg, bgd = (level, level - 1) if kind == "bright" else (level, level + 1)
    for width, survives in ((k - 1, False), (k, True), (k + 1, True)):
        for upright in (False, True):
            g = np.full((80, 90), bgd, np.uint8)
            g[30:30 + width, 10:70] = fg
            if upright:
                g = g.T.copy()
            m = D.obj(g, kind, k, level, 0)
            assert m.any() == survives, (width, upright)
            if survives:
                assert np.array_equal(m, g == fg)                      # the opening gives the bar back at full width
                grown = D.obj(g, kind, k, level, 2)
                want = np.zeros_like(m)
                ys, xs = np.nonzero(m)
                want[max(ys.min() - 2, 0):ys.max() + 3, max(xs.min() - 2, 0):xs.max() + 3] = True
                assert np.array_equal(grown, want)


def test_clipped_borders_find_a_body_that_touches_the_rim():
    """The neighbourhood is clipped, not padded: a body narrower than the size but cut by the rim counts with the part of
    the square that exists, in the corner as along an edge."""
    g = np.zeros((40, 50), np.uint8)
    g[:4, :4] = 200                     # 4 x 4 in the corner: N_3 of pixel (0, 0) is its 4 x 4 part inside the image
    g[20:27, 46:] = 200                 # 7 rows, 4 columns at the right rim
    m = D.obj(g, "bright", 7, 100, 0)
    assert m[:4, :4].all() and m[20:27, 46:].all() and int(m.sum()) == 16 + 28
    g[20:27, 45] = 0
    g[20:27, 41:45] = 200               # the same body one column off the rim: narrower than 7, it vanishes
    g[20:27, 46:] = 0
    assert not D.obj(g, "bright", 7, 100, 0)[20:27].any()


@pytest.mark.parametrize("kind", ["bright", "dark"])
def test_the_model_equals_scipy_filters_with_nearest_edges(kind):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(11)
    g = rng.integers(0, 256, (45, 61)).astype(np.uint8)
    g[10:30, 15:50] = 250 if kind == "bright" else 2
    for size, level, grow in ((3, 128, 0), (7, 200 if kind == "bright" else 60, 3), (31, 100, 16)):
        r = size // 2
        if kind == "bright":
            c = ndi.minimum_filter(g, size=size, mode="nearest") >= level
        else:
            c = ndi.maximum_filter(g, size=size, mode="nearest") <= level
        want = ndi.maximum_filter(c.astype(np.uint8), size=2 * (r + grow) + 1, mode="constant", cval=0) != 0
        assert np.array_equal(D.core(g, kind, size, level), c)
        assert np.array_equal(D.obj(g, kind, size, level, grow), want)


def test_degenerate_levels_mask_everything():
    g = np.random.default_rng(2).integers(0, 256, (20, 33)).astype(np.uint8)
    assert D.pair_mask(g, g, "bright", 5, 0).all() and D.pair_mask(g, g, "dark", 5, 255).all()
    assert not D.pair_mask(g // 2, g // 2, "bright", 5, 255).any() and not D.pair_mask(g | 1, g | 1, "dark", 5, 0).any()
    # the static image is OR-ed in, any non-zero byte, and the result is bytes 0 / 1
    st = np.zeros((20, 33), np.uint8)
    st[3, 4], st[5, 6] = 1, 200
    m = D.pair_mask(g // 2, g // 2, "bright", 5, 255, static=st)
    assert m.dtype == np.uint8 and int(m.sum()) == 2 and m[3, 4] == 1 and m[5, 6] == 1


# ---------------------------------------------------------------------------------------------------------------------
# the scenes through the CPU oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,par", [("bright", S.BRIGHT), ("dark", S.DARK)])
def test_disc_scene_through_the_oracle(kind, par):
    """A disc of radius 30 moves 6 px per pair across synth's uniform flow; the oracle's 32/16 first pass on four pairs,
    without a mask and with the mask segmented from the frames (pixels zeroed, cells over threshold 0.5 excluded).
    Windows per pair more than 0.5 px off the flow, measured: lit disc 12, 12, 11, 11 of 225 without the mask and 0, 2, 0,
    0 of the non-excluded cells with it (largest distance 0.57 px); dark disc 6, 5, 5, 6 and 0, 2, 0, 0.  The mask misses 0
    (lit) and at most 47 = 1.5 % (dark) of the 3177 body pixels; at most 156 = 4.9 % mask pixels lie outside the body
    grown by r + grow.  Asserted: five times the masked count is at most the unmasked count, summed over the pairs; at
    most 2 % of the body missed; at most 10 % of the body's area outside the grown body."""
    from oracle import piv_oracle as O
    r = par["size"] // 2 + par["grow"]
    off, on, far = [], [], []
    for i in range(S.N_PAIRS):
        a, b = S.disc_pair(i, kind)
        m = D.pair_mask(a, b, **par)
        u, v = O.pass1(a, b, 32, 16)[:2]
        off.append(int((np.hypot(u - S.FLOW[0], v - S.FLOW[1]) > 0.5).sum()))
        excluded = M.grid(M.coverage(m, 32, 16), 32, S.THRESHOLD)
        u, v = O.pass1(M.apply(a, m), M.apply(b, m), 32, 16)[:2]
        e = np.hypot(u - S.FLOW[0], v - S.FLOW[1])[~excluded]
        on.append(int((e > 0.5).sum()))
        far.append(float(e.max()))
        bd = S.body(i)
        grown = D._clipped(bd.astype(np.uint8), r, np.maximum, np.uint8(0)) != 0
        missed, outside = int((bd & (m == 0)).sum()), int(((m != 0) & ~grown).sum())
        print(f"{kind} disc, pair {i}: body {int(bd.sum())} px, missed {missed}, mask pixels outside the grown body {outside}, "
              f"excluded cells {int(excluded.sum())}")
        assert int(bd.sum()) == 3177
        assert missed <= 0.02 * bd.sum() and outside <= 0.10 * bd.sum()
    print(f"{kind} disc, windows over 0.5 px off the flow per pair: no mask {off} of 225; segmented mask, non-excluded cells "
          f"{on} (largest distance {max(far):.2f} px)")
    assert sum(off) > 0 and 5 * sum(on) <= sum(off)
