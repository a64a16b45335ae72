"""derive=, the parts that need no GPU: the derive= argument and its slot in the signatures, the new symbol in the header,
the binding and the library, and the numpy model of the local least-squares fit (tests/derive_model.py) -- against
np.linalg.lstsq on the same neighbourhoods, its rank decisions against the rank of the exact integer moment matrices, its
reproduction of polynomial fields, and its vorticity error on a noisy vortex against central differences.

The two tolerances below are gates at 4 x the worst figure measured with this file (python tests/test_derive_host.py prints
them; profiles/derive/measurements.json has the record): the model and lstsq solve the same well-conditioned systems by
different eliminations, so their distance is rounding, not method."""
import inspect
import os
import re

import numpy as np
import pytest

import derive_model as M
from torchpiv_amd.options import DERIVE_QUANTITIES          # the model is the yardstick of this keyword: no keyword, no tests

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(r, o) for r in (1, 2, 3) for o in (1, 2)]

# measured: 6.19e-14 (model against lstsq, relative to the largest coefficient of the cell) and 5.66e-15 (polynomial fields,
# relative to the largest exact value of the planes)
LSTSQ_GATE = 4 * 6.19e-14
POLY_GATE = 4 * 5.66e-15


# ---- the keyword ---------------------------------------------------------------------------------------------------------

def test_derive_arg_accepts_and_refuses():
    from torchpiv_amd import engine, options
    assert options.derive_arg is engine.derive_arg
    assert engine.DERIVE_QUANTITIES == M.QUANTITIES
    full = {"radius": 2, "order": 2}
    assert engine.derive_arg(None) is None
    assert engine.derive_arg("vorticity") == dict(full, quantities=("vorticity",))
    assert engine.derive_arg(("q", "swirl")) == dict(full, quantities=("q", "swirl"))
    assert engine.derive_arg(["dudx", "u_smooth"]) == dict(full, quantities=("dudx", "u_smooth"))
    assert engine.derive_arg({"quantities": "shear"}) == dict(full, quantities=("shear",))
    assert engine.derive_arg({"quantities": ["q"], "radius": 3}) == {"quantities": ("q",), "radius": 3, "order": 2}
    assert engine.derive_arg({"quantities": ("q",), "radius": np.int64(1), "order": 1}) == \
        {"quantities": ("q",), "radius": 1, "order": 1}
    got = engine.derive_arg(engine.DERIVE_QUANTITIES)
    assert got["quantities"] == engine.DERIVE_QUANTITIES and engine.derive_arg(got) == got       # its own result passes
    for bad, text in (("curl", "unknown quantity 'curl'"), (("q", "q"), r"\['q'\] named more than once"),
                      ((), "a name, a tuple or list of names"), (5, "a name, a tuple or list of names"),
                      (True, "a name, a tuple or list of names"), (("q", 3), "unknown quantity 3"),
                      ({"radius": 2}, "the dict needs 'quantities'"), ({}, "the dict needs 'quantities'"),
                      ({"quantities": "q", "size": 2}, r"unknown key\(s\) \['size'\]"),
                      ({"quantities": "q", "radius": 0}, "radius must be 1, 2 or 3, got 0"),
                      ({"quantities": "q", "radius": 4}, "radius must be 1, 2 or 3, got 4"),
                      ({"quantities": "q", "radius": 2.0}, "radius must be 1, 2 or 3, got 2.0"),
                      ({"quantities": "q", "radius": True}, "radius must be 1, 2 or 3, got True"),
                      ({"quantities": "q", "order": 0}, "order must be 1 or 2, got 0"),
                      ({"quantities": "q", "order": 3}, "order must be 1 or 2, got 3"),
                      ({"quantities": "q", "order": True}, "order must be 1 or 2, got True"),
                      ({"quantities": {"q"}}, "a name, a tuple or list of names")):
        with pytest.raises(ValueError, match="derive: .*" + text):
            engine.derive_arg(bad)


def test_keyword_in_the_record_and_no_exclusion_row():
    from torchpiv_amd import options
    assert DERIVE_QUANTITIES == M.QUANTITIES
    assert "derive" in options.KEYWORDS and options.Options().derive is None
    assert options.KEYWORDS.index("derive") == options.KEYWORDS.index("uncertainty") + 1
    assert not any("derive" in (row[0], row[1]) for row in options.EXCLUSIONS)
    run = dict(wind_size=32, overlap=16, multipass=2, multipass_scale=2.0, multipass_mode="CWS")
    every = dict(uncertainty="cs", deform=2, outlier="median", derive="q")          # it combines with the other keywords
    assert options.parse_options(run, **every).derive == {"quantities": ("q",), "radius": 2, "order": 2}
    assert options.parse_options(run, weighting="gaussian", derive=("q", "swirl")).derive["quantities"] == ("q", "swirl")
    assert options.parse_options(run).derive is None
    with pytest.raises(ValueError, match="derive: unknown quantity"):
        options.parse_options(run, derive="rot")


def test_keyword_slot_and_default_in_the_three_signatures(tmp_path):
    import torch
    from torchpiv_amd import backend, engine, runner
    for fn in (backend.OfflinePIV.__init__, backend.ResidentPIV.__init__):
        names = list(inspect.signature(fn).parameters)
        assert names[names.index("uncertainty") + 1] == "derive", names
        assert names[-6:] == ["deform", "correlation", "weighting", "dynamic_mask", "equalize", "prefilter"], names
        assert names[-7] == "derive" and inspect.signature(fn).parameters["derive"].default is None
    names = list(inspect.signature(runner.run_folder).parameters)
    assert names[-2:] == ["equalize", "prefilter"] and names[names.index("derive") + 1] == "deform", names
    assert inspect.signature(runner.run_folder).parameters["derive"].default is None
    # Plan and debug_pass get no new parameter
    assert list(inspect.signature(engine.Plan.__init__).parameters)[-1] == "correlation"
    assert list(inspect.signature(engine.debug_pass).parameters)[-1] == "correlation"
    for fn in (engine.Plan.__init__, engine.debug_pass):
        assert "derive" not in inspect.signature(fn).parameters
    # checked before any device is touched
    f = torch.zeros(2, 64, 64, dtype=torch.uint8)
    for bad in ("curl", ("q", "q"), {"quantities": "q", "radius": 5}):
        with pytest.raises(ValueError, match="derive:"):
            backend.OfflinePIV(str(tmp_path), "cpu", "bmp", 64, 32, derive=bad)
        with pytest.raises(ValueError, match="derive:"):
            backend.ResidentPIV(f, f, 32, 16, derive=bad)
        with pytest.raises(ValueError, match="derive:"):
            runner.run_folder(str(tmp_path), "cpu", "bmp", 64, 32, derive=bad)
    piv = backend.OfflinePIV(str(tmp_path), "cpu", "bmp", 64, 32, derive=("vorticity", "q"))
    assert len(piv) == 0 and list(piv()) == [] and piv._derive["quantities"] == ("vorticity", "q")
    assert runner.run_folder(str(tmp_path), "cpu", "bmp", 64, 32, derive="q") == (None, 0)
    assert [runner.derive_key(k) for k in ("dudx", "vorticity", "swirl", "q", "u_smooth", "v_smooth")] == \
        ["dudx[1/s]", "vorticity[1/s]", "swirl[1/s]", "q[1/s^2]", "u_smooth[m/s]", "v_smooth[m/s]"]


def test_run_sharded_refuses_the_keyword(tmp_path):
    from torchpiv_amd import backend, dist
    piv = backend.OfflinePIV(str(tmp_path), "cpu", "bmp", 64, 32, derive="q")
    with pytest.raises(ValueError, match="derive= is not gathered"):
        dist.run_sharded(piv)


def test_symbol_in_header_binding_and_library():
    from torchpiv_amd import _lib, engine
    hdr = open(os.path.join(ROOT, "include", "torchpiv_hip.h")).read()
    kern = open(os.path.join(ROOT, "torchpiv_amd", "csrc", "piv_kernels.h")).read()
    assert re.search(r"\bint\s+tpiv_field_fit\s*\(", hdr)
    assert "launch_field_fit" in kern and "fieldfit" in open(os.path.join(ROOT, "torchpiv_amd", "csrc", "Makefile")).read()
    tile = re.search(r"FIELDFIT_TILE_COLS = (\d+), FIELDFIT_TILE_ROWS = (\d+)", kern)
    assert (int(tile.group(2)), int(tile.group(1))) == engine.FIELD_FIT_TILE
    assert "tpiv_field_fit" in _lib.SIGNATURES and hasattr(_lib.lib, "tpiv_field_fit")
    assert len(_lib.SIGNATURES["tpiv_field_fit"][1]) == 12
    assert _lib.ABI_VERSION == 2 and "#define TPIV_VERSION 2" in hdr
    # argument errors are decided on the host, before any launch (the pointers are never followed)
    u, v, s, fit, cnt, ordr = 4096, 8192, 12288, 1 << 20, 2 << 20, 3 << 20
    call = _lib.lib.tpiv_field_fit
    for b, nr, nc, rad, od in ((1, 0, 4, 2, 2), (1, 4, 0, 2, 2), (-1, 4, 4, 2, 2), (1, 4, 4, 0, 2), (1, 4, 4, 4, 2),
                               (1, 4, 4, 2, 0), (1, 4, 4, 2, 3), (1 << 11, 1 << 10, 1 << 10, 2, 2)):
        assert call(u, v, s, b, nr, nc, rad, od, fit, cnt, ordr, None) == _lib.EINVAL, (b, nr, nc, rad, od)
    for args in ((None, v, s, fit, cnt, ordr), (u, None, s, fit, cnt, ordr), (u, v, s, None, cnt, ordr),
                 (u, v, s, fit, None, ordr), (u, v, s, fit, cnt, None)):
        assert call(*args[:3], 1, 4, 4, 2, 2, *args[3:], None) == _lib.EINVAL
    # an output that overlaps an input, or another output (16 cells: u 128 bytes, fit 768 bytes)
    assert call(u, v, s, 1, 4, 4, 2, 2, u + 120, cnt, ordr, None) == _lib.EINVAL
    assert call(u, v, s, 1, 4, 4, 2, 2, fit, s + 15, ordr, None) == _lib.EINVAL
    assert call(u, v, s, 1, 4, 4, 2, 2, fit, cnt, v - 8, None) == _lib.EINVAL
    assert call(u, v, s, 1, 4, 4, 2, 2, fit, fit + 760, ordr, None) == _lib.EINVAL
    assert call(u, v, s, 1, 4, 4, 2, 2, fit, cnt, cnt + 15, None) == _lib.EINVAL
    assert call(u, v, None, 0, 4, 4, 2, 2, fit, cnt, ordr, None) == _lib.OK             # nothing to do, nothing launched


# ---- the model -------------------------------------------------------------------------------------------------------------

def _lstsq_cell(u, v, ok, r, c, radius, n):
    """(coefficients [2, n] by np.linalg.lstsq, rank) of one cell's neighbourhood."""
    R, C = u.shape
    rows, rhs = [], []
    for j in range(-radius, radius + 1):
        for i in range(-radius, radius + 1):
            if 0 <= r + j < R and 0 <= c + i < C and ok[r + j, c + i]:
                rows.append([float(i ** a * j ** b) for a, b in M.EXP[:n]])
                rhs.append((u[r + j, c + i], v[r + j, c + i]))
    sol, _, rank, _ = np.linalg.lstsq(np.array(rows), np.array(rhs), rcond=None)
    return sol.T, rank


def lstsq_distance():
    """The worst distance between the model's c0, c1, c2 and lstsq's over random fields and skip patterns at every (radius,
    order), relative to the cell's largest coefficient; cells whose order fell below the one asked for are compared at
    the order fitted."""
    rng = np.random.default_rng(20261)
    worst = 0.0
    for radius, order in CASES:
        for density in (0.0, 0.3, 0.6):
            u, v = rng.normal(0, 3, (2, 12, 13))
            skip = rng.random((12, 13)) < density
            fit, count, fitted = M.field_fit(u, v, skip.astype(np.uint8), radius, order)
            for r in range(12):
                for c in range(13):
                    if fitted[r, c] < 1:
                        continue
                    n = 6 if fitted[r, c] == 2 else 3
                    sol, rank = _lstsq_cell(u, v, ~skip, r, c, radius, n)
                    assert rank == n
                    for w, base in ((0, 0), (1, 3)):
                        got = fit[base:base + 3, r, c]
                        worst = max(worst, np.abs(got - sol[w, :3]).max() / np.abs(sol[w]).max())
    return worst


def test_model_agrees_with_lstsq():
    worst = lstsq_distance()
    print(f"model against lstsq: worst relative difference {worst:.3e} (gate {LSTSQ_GATE:.3e})")
    assert worst <= LSTSQ_GATE


def _model_order(valid, radius, order):
    """The order the model fits at the centre of each validity pattern [n, 2 radius + 1, 2 radius + 1]."""
    rng = np.random.default_rng(7)
    u, v = rng.normal(0, 1, (2,) + valid.shape)
    fit, count, fitted, (d, m0) = M.field_fit(u, v, (~valid).astype(np.uint8), radius, order, want_pivots=True)
    assert np.array_equal(count[:, radius, radius], valid.reshape(valid.shape[0], -1).sum(1))
    return fitted[:, radius, radius], d[:, :, radius, radius].T, m0[:, :, radius, radius].T      # pivots: [pattern, k]


def test_rank_decisions_all_512_patterns_at_radius_1():
    valid = ((np.arange(512)[:, None] >> np.arange(9)) & 1).astype(bool).reshape(512, 3, 3)
    for order in (1, 2):
        got, _, _ = _model_order(valid, 1, order)
        want = np.array([M.ladder(p, 1, order) for p in valid])
        assert np.array_equal(got, want), np.flatnonzero(got != want)
    assert (want == 1).sum() > 300 and (want == 0).sum() > 9 and (want == -1).sum() == 1       # (nine cells never reach order 2)


def _written_down(radius):
    """The singular patterns: a single row, a single column, a diagonal, five points (too few for order 2; in general
    position for order 1), one cell and none -- with the order the ladder gives each at order 2 / order 1."""
    w = 2 * radius + 1
    z = np.zeros((w, w), bool)
    row, col, diag, five, one = z.copy(), z.copy(), z.copy(), z.copy(), z.copy()
    row[radius] = True
    col[:, 0] = True
    diag[np.arange(w), np.arange(w)] = True
    five[0, 0] = five[0, w - 1] = five[w - 1, 0] = five[w - 1, w - 1] = five[radius, radius] = True
    one[w - 1, 0] = True
    return np.stack([row, col, diag, five, one, z]), (0, 0, 0, 1, 0, -1)


@pytest.mark.parametrize("radius", (2, 3))
def test_rank_decisions_random_and_written_down_patterns(radius):
    rng = np.random.default_rng(100 + radius)
    w = 2 * radius + 1
    density = rng.choice([0.1, 0.2, 0.35, 0.5, 0.8], size=(5000, 1, 1))
    valid = rng.random((5000, w, w)) < density
    singular, expect = _written_down(radius)
    valid = np.concatenate([singular, valid])
    gap_full, gap_def = np.inf, 0.0
    for order in (1, 2):
        got, d, m0 = _model_order(valid, radius, order)
        want = np.array([M.ladder(p, radius, order) for p in valid])
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
        assert tuple(got[:6]) == expect
        with np.errstate(all="ignore"):
            rel = d / m0
        n = d.shape[1]
        full = want == (2 if order == 2 else 1)
        gap_full = min(gap_full, rel[full].min())
        # the first rejected pivot of the patterns that fell back
        for k in np.flatnonzero(~full & (want >= 0)):
            first = next(q for q in range(n) if not rel[k, q] > M.PIVOT_TOL)
            gap_def = max(gap_def, abs(rel[k, first]))
        assert (want == 2).sum() > 1000 or order == 1
        assert (want < (2 if order == 2 else 1)).sum() > 100
    print(f"radius {radius}: smallest accepted relative pivot {gap_full:.3e}, largest rejected {gap_def:.3e}")
    assert gap_full > 1e3 * M.PIVOT_TOL and gap_def < 1e-3 * M.PIVOT_TOL         # the threshold sits well inside the gap


def test_full_neighbourhood_never_falls_back():
    rng = np.random.default_rng(3)
    u, v = rng.normal(0, 1, (2, 9, 11))
    for radius, order in CASES:
        fit, count, fitted = M.field_fit(u, v, None, radius, order)
        inner = (slice(radius, 9 - radius), slice(radius, 11 - radius))
        assert (fitted[inner] == order).all() and (count[inner] == (2 * radius + 1) ** 2).all()
        if (radius, order) == (1, 2):                     # two offsets along an axis carry no second derivative
            border = np.ones(fitted.shape, bool)
            border[inner] = False
            assert (fitted[border] == 1).all()
        else:                                             # the cut neighbourhoods of the border hold a full-rank set too
            assert (fitted == order).all()
        assert count[0, 0] == (radius + 1) ** 2 and np.isfinite(fit).all()


def _poly_field(order, shape=(11, 12)):
    """u, v of degree <= order with dyadic coefficients on integer cells, and their exact U, Ux, Uy, V, Vx, Vy."""
    r, c = np.meshgrid(np.arange(shape[0], dtype=np.float64), np.arange(shape[1], dtype=np.float64), indexing="ij")
    q = 1.0 if order == 2 else 0.0
    u = 1.5 - 0.75 * c + 0.5 * r + q * (0.25 * c * c - 0.125 * c * r + 0.0625 * r * r)
    v = -2.0 + 0.375 * c - 1.25 * r + q * (-0.5 * c * c + 0.25 * c * r + 0.125 * r * r)
    ux = -0.75 + q * (0.5 * c - 0.125 * r)
    uy = 0.5 + q * (-0.125 * c + 0.125 * r)
    vx = 0.375 + q * (-1.0 * c + 0.25 * r)
    vy = -1.25 + q * (0.25 * c + 0.25 * r)
    return u, v, np.stack([u, ux, uy, v, vx, vy])


def poly_distance():
    rng = np.random.default_rng(11)
    worst = 0.0
    for radius, order in CASES:
        u, v, exact = _poly_field(order)
        for density in (0.0, 0.25):
            skip = (rng.random(u.shape) < density).astype(np.uint8)
            fit, count, fitted = M.field_fit(u, v, skip, radius, order)
            ok = fitted == order                     # where the order asked for was fitted the polynomial is reproduced
            assert ok.mean() > (0.3 if (radius, order) == (1, 2) else 0.8)
            worst = max(worst, np.abs(fit - exact)[:, ok].max() / np.abs(exact).max())
    return worst


def test_polynomial_fields_are_reproduced():
    worst = poly_distance()
    print(f"polynomial fields: worst error {worst:.3e} of the largest exact value (gate {POLY_GATE:.3e})")
    assert worst <= POLY_GATE


def vortex_errors(seeds=(0, 1, 2)):
    """rms vorticity error of np.gradient(edge_order=2) and of the model at radius 2, order 2 and 1, on a Lamb-Oseen vortex
    (core radius 6 cells, peak swirl velocity about 2.9 px) on a 41 x 41 grid with 0.1 px white noise, over the seeds."""
    n, rc, gamma, sigma = 41, 6.0, 150.0, 0.1
    y, x = np.meshgrid(np.arange(n) - 20.0, np.arange(n) - 20.0, indexing="ij")
    r2 = x * x + y * y
    with np.errstate(all="ignore"):
        ut = np.where(r2 > 0, gamma / (2 * np.pi * r2) * (1 - np.exp(-r2 / rc ** 2)), gamma / (2 * np.pi * rc ** 2))
    u0, v0 = -ut * y, ut * x
    omega = gamma / (np.pi * rc ** 2) * np.exp(-r2 / rc ** 2)
    err = {"gradient": [], (2, 2): [], (2, 1): []}
    for seed in seeds:
        rng = np.random.default_rng(seed)
        u, v = u0 + rng.normal(0, sigma, u0.shape), v0 + rng.normal(0, sigma, v0.shape)
        w = np.gradient(v, axis=1, edge_order=2) - np.gradient(u, axis=0, edge_order=2)
        err["gradient"].append(np.sqrt(np.mean((w - omega) ** 2)))
        for radius, order in ((2, 2), (2, 1)):
            fit, _, _ = M.field_fit(u, v, None, radius, order)
            w = M.derive(fit, 1000.0, 1000.0, ("vorticity",))["vorticity"]        # steps of one cell: per cell spacing
            err[radius, order].append(np.sqrt(np.mean((w - omega) ** 2)))
    return {k: float(np.sqrt(np.mean(np.square(e)))) for k, e in err.items()}


def test_noisy_vortex_beats_central_differences():
    err = vortex_errors()
    print("rms vorticity error:", err)
    assert err[2, 2] < err["gradient"] and err[2, 1] < err["gradient"]


def test_derive_expressions_of_the_model():
    fit = np.array([2.0, 0.5, -0.25, -1.0, 0.125, 0.75]).reshape(6, 1, 1)
    d = M.derive(fit, 2000.0, -4000.0)                   # steps 2 m and -4 m
    dudx, dudy, dvdx, dvdy = 0.25, 0.0625, 0.0625, -0.1875
    want = {"dudx": dudx, "dudy": dudy, "dvdx": dvdx, "dvdy": dvdy, "vorticity": dvdx - dudy, "divergence": dudx + dvdy,
            "shear": dvdx + dudy, "q": -0.5 * (dudx * dudx + 2 * dudy * dvdx + dvdy * dvdy), "u_smooth": 2.0, "v_smooth": -1.0,
            "swirl": 0.0}
    assert list(d) == list(M.QUANTITIES)
    for k, w in want.items():
        assert d[k].shape == (1, 1) and d[k][0, 0] == w, k
    rot = M.derive(np.array([0.0, 0.0, -3.0, 0.0, 3.0, 0.0]).reshape(6, 1), 1000.0, 1000.0)     # solid-body rotation
    assert rot["swirl"][0] == 3.0 and rot["vorticity"][0] == 6.0 and rot["q"][0] == 9.0 and rot["divergence"][0] == 0.0


if __name__ == "__main__":
    print("lstsq distance", lstsq_distance())
    print("poly distance", poly_distance())
    print("vortex", vortex_errors())
