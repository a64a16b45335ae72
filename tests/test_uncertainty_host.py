"""Correlation-statistics uncertainty, the parts that need no GPU: the numpy model the device kernel is checked against
(tests/uncertainty_model.py) on five anchor windows whose integers are written down here, the uncertainty= argument, the
new symbols in the header and the binding, and the estimator's calibration on the model alone: its rms against the actual
error of the CPU oracle's two-pass CWS fields on synthetic pairs."""
import os
import re

import numpy as np
import pytest

import uncertainty_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def anchor_scene():
    rng = np.random.default_rng(20261019)
    base = rng.integers(0, 256, (60, 64)).astype(np.float64)
    p = np.pad(base, 1, mode="edge")
    a = (sum(p[i:i + 60, j:j + 64] for i in range(3) for j in range(3)) // 9).astype(np.uint8)
    b = np.roll(a, (-2, 2), axis=(0, 1))
    b = np.clip(b.astype(np.int64) + rng.integers(-6, 7, b.shape), 0, 255).astype(np.uint8)
    return a, b


# (y0, x0, ws, u, v, R): C0, (S2, S00, var, n) of x, the same of y, sigma_u, sigma_v
ANCHORS = [
    ((16, 20, 16, 2.3, -1.6, 3), 1418824, (1880186, 1981200556, 25533066506, 24),
     (1998577, 2604474639, 58038952603, 24), 0.1025844582420518, 0.16924438902645186),
    ((0, 0, 16, 2.3, -1.6, 3), 2214985, (3509905, 5414251025, 28208694029, 11),
     (3362984, 6458642088, 58159370358, 23), 0.10234692950048385, 0.12913221321413723),
    ((44, 48, 16, -2.3, 1.6, 4), -80625, (-263770, 15346859898, 57408353626, 9),
     (-204365, 14300387007, 53322595671, 8), float("nan"), float("nan")),
    ((8, 8, 32, 2.0, -2.0, 0), 9609824, (12258996, 4439230576, 4439230576, 0),
     (12790032, 4266082880, 4266082880, 0), 0.006043132272516508, 0.006269367049298384),
    ((20, 24, 8, 1.99609375, -2.00390625, 2), 406032, (457472, 171235328, 380825088, 5),
     (400992, 212144128, 406452224, 4), 0.03713083123150357, 0.035591431550533195),
]


def test_anchor_scene_is_the_one_written_down():
    a, b = anchor_scene()
    assert int(a.sum()) == 479871 and int(b.sum()) == 479815


@pytest.mark.parametrize("anchor", ANCHORS, ids=[str(k[0]) for k in ANCHORS])
def test_model_on_the_anchor_windows(anchor):
    (y0, x0, ws, u, v, R), C0, cx, cy, want_su, want_sv = anchor
    a, b = anchor_scene()
    su, sv, stats = M.windows(a, b, [y0], [x0], [u], [v], ws, R)
    assert stats.dtype == np.int64
    want = [C0, cx[0], cx[1], cx[2], cy[0], cy[1], cy[2], cx[3] + 256 * cy[3]]
    assert stats[0].tolist() == want
    for got, w in ((su[0], want_su), (sv[0], want_sv)):
        if np.isnan(w):
            assert np.isnan(got)
        else:
            assert got > 0 and abs(got - w) <= 1e-12 * w, (got, w)


def test_model_half_shift_and_refusals_of_a_cell():
    h, ok = M.half_shift(np.array([0.0, -0.0, 2.0, 255 / 128, 1 / 256, 3 / 256, 200.0, -300.0, np.nan, np.inf]))
    assert h.tolist() == [0, 0, 256, 255, 0, 2, 25600, -32767, 0, 0]       # ties to even; the clamp
    assert ok.tolist() == [True] * 8 + [False, False]
    a, b = anchor_scene()
    su, sv, st = M.windows(a, b, [16] * 3, [20] * 3, [2.3, np.nan, 2.3], [-1.6, -1.6, np.inf], 16, 3)
    assert np.isfinite(su[0]) and np.isnan(su[1:]).all() and np.isnan(sv[1:]).all() and not st[1:].any()
    su, sv, st = M.windows(a, b, [16] * 2, [20] * 2, [2.3] * 2, [-1.6] * 2, 16, 3, invalid=[0, 7])
    assert np.isfinite(su[0]) and np.isnan(su[1]) and np.isnan(sv[1]) and not st[1].any() and st[0].any()
    assert len(M.lags(3)) == 24 and len(M.lags(4)) == 40 and M.lags(0) == []
    # the whole field in one call equals the windows one by one
    u = np.full((3, 4), 2.3)
    v = np.full((3, 4), -1.6)
    a2, b2 = np.ascontiguousarray(a[:32, :41]), np.ascontiguousarray(b[:32, :41])
    assert M.field_shape(32, 41, 16, 8) == (3, 4)
    fsu, fsv, fst = M.field(a2, b2, u, v, 16, 8, R=2)
    for r in range(3):
        for c in range(4):
            s1, s2, st1 = M.windows(a2, b2, [8 * r], [8 * c], [2.3], [-1.6], 16, 2)
            assert np.array_equal(fst[r, c], st1[0]) and np.array_equal([fsu[r, c], fsv[r, c]], [s1[0], s2[0]], equal_nan=True)


def test_uncertainty_arg_forms_and_refusals():
    from torchpiv_amd import engine
    assert engine.UNCERTAINTY_DEFAULTS == {"kind": "cs", "radius": 3}
    assert engine.uncertainty_arg(None) is None
    assert engine.uncertainty_arg("cs") == {"kind": "cs", "radius": 3}
    assert engine.uncertainty_arg({}) == {"kind": "cs", "radius": 3}
    assert engine.uncertainty_arg({"kind": "cs", "radius": 0}) == {"kind": "cs", "radius": 0}
    assert engine.uncertainty_arg({"radius": np.int64(4)}) == {"kind": "cs", "radius": 4}
    assert engine.uncertainty_arg("cs") is not engine.UNCERTAINTY_DEFAULTS
    for bad in ("mc", "CS", 3, True, ["cs"], {"radius": 5}, {"radius": -1}, {"radius": 2.0}, {"radius": True},
                {"radius": None}, {"kind": "mc"}, {"kind": None}, {"reach": 3}, {"radius": 3, 1: 2}):
        with pytest.raises(ValueError, match="uncertainty"):
            engine.uncertainty_arg(bad)


def test_constructors_check_the_argument_before_any_device(tmp_path):
    import torch

    import torchpiv_amd as T
    from torchpiv_amd import dist
    with pytest.raises(ValueError, match="uncertainty"):
        T.OfflinePIV(str(tmp_path), "cpu", "bmp", 32, 16, uncertainty="mc")
    z = torch.zeros(1, 64, 64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="uncertainty"):
        T.ResidentPIV(z, z, 32, 16, uncertainty={"radius": 9})
    # an empty folder constructs without a device; run_sharded refuses the option before it touches the process group
    piv = T.OfflinePIV(str(tmp_path), "cpu", "bmp", 32, 16, uncertainty={"radius": 2})
    assert piv._uncertainty == {"kind": "cs", "radius": 2}
    with pytest.raises(ValueError, match="uncertainty"):
        dist.run_sharded(piv)
    assert T.OfflinePIV(str(tmp_path), "cpu", "bmp", 32, 16)._uncertainty is None


def test_new_symbols_in_header_binding_and_library():
    from torchpiv_amd import _lib
    header = open(os.path.join(ROOT, "include", "torchpiv_hip.h")).read()
    for name in ("tpiv_uncertainty", "tpiv_plan_set_uncertainty", "tpiv_plan_uncertainty"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name) is not None
    assert len(_lib.SIGNATURES["tpiv_uncertainty"][1]) == 15


# ---------------------------------------------------------------------------------------------------------------------
# calibration of the model against the actual error of the oracle's fields
# ---------------------------------------------------------------------------------------------------------------------
def _oracle_fields(a, b):
    from oracle import piv_oracle as O
    u, v, x, y, val = O.pass1(a, b, 64, 32, validate=True)
    u, v, x, y, val = O.ITER["CWS"](a.shape, 32, 16)(a, b, x, y, u, v, val)
    return u, v, x, y


def _calibration(kind, idx):
    import torch

    from torchpiv_amd import synth
    H = W = 256
    a, b = (t.numpy() for t in synth.make_pair(H, W, idx, kind=kind, noise=4.0))
    u, v, x, y = _oracle_fields(a, b)
    X, Y = np.meshgrid(np.asarray(x, np.float64), np.asarray(y, np.float64)) if np.ndim(x) == 1 else (x, y)
    dx, dy = synth.flow_field(torch.from_numpy(X), torch.from_numpy(Y), H, W, kind)
    su, sv, _ = M.field(a, b, u, v, 32, 16, R=3)
    out = {}
    for name, got, true, s in (("u", u, dx.numpy(), su), ("v", v, dy.numpy(), sv)):
        err = got - true
        ok = (np.abs(err) < 1.0) & np.isfinite(s)
        rms_s = float(np.sqrt(np.mean(s[ok] ** 2)))
        out[name] = {"share": float(ok.mean()), "rms_sigma": rms_s, "std_error": float(np.std(err[ok])),
                     "rms_error": float(np.sqrt(np.mean(err[ok] ** 2)))}
    return out


@pytest.mark.parametrize("kind,idx", [("uniform", 0), ("uniform", 1), ("wavy", 0), ("wavy", 1)])
def test_model_sigma_tracks_the_error_of_the_oracle_fields(kind, idx):
    """256 x 256 synth pairs, noise 4, the oracle's pass 1 at 64/32 and CWS pass at 32/16, R = 3.  Over the cells with
    |error| < 1 px and finite sigma (at least 95 % of all): rms sigma / std(error) on the uniform flow, rms sigma /
    rms(error) on the wavy one (whose in-window gradients the rigid shift leaves as error), inside [0.6, 1.7] per
    component.  Measured with this model (profiles/uncertainty/measurements.json): uniform 0: 1.10 (u) / 0.87 (v),
    uniform 1: 1.04 / 0.85, wavy 0: 1.22 / 0.98, wavy 1: 0.98 / 0.91 (mean of the wavy pairs 1.10 / 0.94); every cell
    counted (share 1.0)."""
    fig = _calibration(kind, idx)
    print("uncertainty calibration", kind, idx, fig)
    for name in ("u", "v"):
        f = fig[name]
        assert f["share"] >= 0.95, (name, f)
        ratio = f["rms_sigma"] / (f["std_error"] if kind == "uniform" else f["rms_error"])
        assert 0.6 <= ratio <= 1.7, (name, ratio, f)
