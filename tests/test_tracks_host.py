"""tracks() on the host: the properties of the numpy model of tests/tracks_model.py -- what it finds and how well on a
rendered scene with known particle positions, the tie rules of detection and matching, the inclusive radius, the
statuses -- and the argument checks of engine.tracks_arg.  The device is held to this model bit for bit in
tests/test_gpu_tracks.py."""
import numpy as np
import pytest

import tracks_model as M

H, W = M.SCENE_SHAPE


def _scene_predictor(offset=(0.4, -0.3)):
    xc, yc = M.window_centres(W, 32, 16), M.window_centres(H, 32, 16)
    XC, YC = np.meshgrid(xc, yc)
    up, vp = M.scene_shift(XC, YC)
    return up + offset[0], vp + offset[1], xc, yc


def test_scene_counts_and_errors():
    """96 x 160, 180 particles on a jittered 8 px lattice (seed 7), sigma 1, amplitude 200, level 40, predictor off by
    (0.4, -0.3) px, radius 1.5.  Measured with this model: 180 of 180 found in both frames, 180 matched; worst position
    error 0.0066 px (0.00665 in frame a, 0.00639 in frame b), worst displacement error 0.0085 px (0.00853).  The bounds are
    twice those values: the margin is for another numpy's exp / rint in the renderer, the detection itself is table-driven."""
    a, b, xa, ya, xb, yb = M.scene()
    lists, row_start, count = M.detect(np.stack([a, b]), M.SCENE_LEVEL)
    assert count.tolist() == [180, 180]
    assert row_start[:, 0].tolist() == [0, 0] and row_start[:, H].tolist() == [180, 180]
    (ax, ay, ap), (bx, by, bp) = lists
    assert ap.dtype == np.uint8 and ap.min() >= M.SCENE_LEVEL

    def nearest(lx, ly, tx, ty):
        d = np.hypot(lx[:, None] - tx[None], ly[:, None] - ty[None])
        return d.argmin(1), d.min(1)
    ka, ea = nearest(ax, ay, xa, ya)
    kb, eb = nearest(bx, by, xb, yb)
    assert sorted(ka) == list(range(180)) and sorted(kb) == list(range(180))       # every particle once
    print(f"position error: a {ea.max():.5f} px, b {eb.max():.5f} px")
    assert ea.max() < 2 * 0.0066 and eb.max() < 2 * 0.0066
    up, vp, xc, yc = _scene_predictor()
    m, status, d2, matched = M.match(ax, ay, bx, by, row_start[1], up, vp, xc, yc, M.SCENE_RADIUS, (H, W))
    assert matched == 180 and (status == M.MATCHED).all() and sorted(m) == list(range(180))
    assert (kb[m] == ka).all()                                                     # the pairs are the true pairs
    du, dv = M.scene_shift(xa[ka], ya[ka])
    err = np.hypot(bx[m] - ax - du, by[m] - ay - dv)
    print(f"displacement error: {err.max():.5f} px")
    assert err.max() < 2 * 0.0085
    # the rows the radius reaches hold every candidate: the same result from all pairs
    m2, status2, d22, matched2 = M.match(ax, ay, bx, by, row_start[1], up, vp, xc, yc, M.SCENE_RADIUS, (H, W), all_pairs=True)
    assert (m2 == m).all() and (status2 == status).all() and d22.tobytes() == d2.tobytes() and matched2 == matched


def test_detection_definition_and_ties():
    f = np.zeros((1, 9, 12), dtype=np.uint8)
    f[0, 0, :] = 255                                  # bright border pixels are never reported
    f[0, :, 0] = 255
    f[0, 8, 5] = 255
    f[0, 2:5, 3:7] = 90                               # a 3 x 4 plateau: its raster-first pixel alone
    f[0, 6, 9] = 50
    f[0, 6, 10] = 50                                  # two equal neighbours: the left one
    f[0, 7, 2] = 39                                   # below the level
    lists, row_start, count = M.detect(f, 40)
    x, y, peak = lists[0]
    assert count.tolist() == [2] and peak.tolist() == [90, 50]
    assert (x[0], y[0]) == (3.5, 2.5)                 # L = ln 1 = 0, C = R: the fit puts the corner of a plateau half a pixel in
    assert (x[1], y[1]) == (9.5, 6.0)
    assert row_start[0].tolist() == [0, 0, 0, 1, 1, 1, 1, 2, 2, 2]
    # a mask hides the plateau's winner and nothing takes its place; the level is inclusive
    mask = np.zeros((9, 12), dtype=np.uint8)
    mask[2, 3] = 7
    assert M.detect(f, 50, mask)[2].tolist() == [1] and M.detect(f, 51, mask)[2].tolist() == [0]
    # peaks in the first and last interior rows and columns
    g = np.zeros((1, 5, 6), dtype=np.uint8)
    g[0, 1, 1] = g[0, 1, 4] = g[0, 3, 1] = g[0, 3, 4] = 200
    lists, row_start, count = M.detect(g, 1)
    assert count.tolist() == [4] and row_start[0].tolist() == [0, 0, 2, 2, 4, 4]
    assert lists[0][0].tolist() == [1.0, 4.0, 1.0, 4.0] and lists[0][1].tolist() == [1.0, 1.0, 3.0, 3.0]
    with pytest.raises(ValueError):
        M.detect(np.zeros((1, 2, 5), dtype=np.uint8), 1)


def test_subpixel_offset_stays_within_half_a_pixel():
    tab = M.table()
    L, C, R = np.meshgrid(tab, tab, tab, indexing="ij")
    keep = (C >= L) & (C >= R)                          # what a peak pixel can see
    off = M._subpixel(L[keep], C[keep], R[keep])
    # exactly, |L - R| <= |den|.  den's two roundings are at most 1.5 ulp(2 ln 255) = 2.7e-15 against |den| >= ln(255 / 254) =
    # 3.9e-3 where R = C: 7e-13 of it, half of that on the offset
    assert np.isfinite(off).all() and np.abs(off).max() <= 0.5 + 4e-13


def _rows(ys, Hh):
    """row_start of a hand-made list in raster order."""
    r = np.floor(np.asarray(ys) + 0.5).astype(int)
    rs = np.zeros(Hh + 1, dtype=np.int32)
    rs[1:] = np.cumsum(np.bincount(r, minlength=Hh))
    return rs


ZERO = (np.zeros((1, 1)), np.zeros((1, 1)), [8.0], [8.0])        # a 1 x 1 predictor grid of zero displacement


def _match(a, b, radius=1.5, pred=ZERO, shape=(17, 17)):
    xa, ya = (np.array(t, dtype=np.float64) for t in zip(*a)) if a else (np.zeros(0), np.zeros(0))
    xb, yb = (np.array(t, dtype=np.float64) for t in zip(*b)) if b else (np.zeros(0), np.zeros(0))
    return M.match(xa, ya, xb, yb, _rows(yb, shape[0]), *pred, radius, shape)


def test_match_ties_radius_and_statuses():
    # two equidistant candidates: the lower j
    m, s, d2, n = _match([(8.0, 8.0)], [(7.0, 8.0), (9.0, 8.0)])
    assert (m.tolist(), s.tolist(), d2.tolist(), n) == ([0], [0], [1.0], 1)
    # two claimants of one b: the nearer wins, the other gets status 2 and keeps its d2
    m, s, d2, n = _match([(7.0, 8.0), (8.5, 8.0)], [(8.0, 8.0)])
    assert (m.tolist(), s.tolist(), d2.tolist(), n) == ([-1, 0], [2, 0], [1.0, 0.25], 1)
    # equally near claimants: the lower i
    m, s, d2, n = _match([(7.5, 8.0), (8.5, 8.0), (8.0, 8.5)], [(8.0, 8.0)])
    assert (m.tolist(), s.tolist(), n) == ([0, -1, -1], [0, 2, 2], 1)
    # a candidate at exactly R is one (the bound is inclusive); just beyond it is none
    m, s, d2, n = _match([(8.0, 8.0)], [(9.5, 8.0)])
    assert (m.tolist(), s.tolist(), d2.tolist()) == ([0], [0], [2.25])
    m, s, d2, n = _match([(8.0, 8.0)], [(9.5, 8.0)], radius=np.nextafter(1.5, 0))
    assert (m.tolist(), s.tolist(), n) == ([-1], [M.NO_CANDIDATE], 0) and np.isnan(d2[0])
    # a loser does not fall back to its second candidate
    m, s, d2, n = _match([(8.0, 8.0), (8.25, 8.0)], [(8.25, 8.0), (7.0, 8.0)])
    assert (m.tolist(), s.tolist()) == ([-1, 0], [2, 0])
    # predicted outside the frame: status 3, whatever lies near; the frame's edge itself is inside
    pred = (np.full((1, 1), 9.0), np.zeros((1, 1)), [8.0], [8.0])
    m, s, d2, n = _match([(8.0, 8.0), (7.0, 8.0)], [(16.0, 8.0)], pred=pred)
    assert (m.tolist(), s.tolist()) == ([-1, 0], [M.OUTSIDE, 0])
    nan = (np.full((1, 1), np.nan), np.zeros((1, 1)), [8.0], [8.0])
    assert _match([(8.0, 8.0)], [(8.0, 8.0)], pred=nan)[1].tolist() == [M.OUTSIDE]
    # empty lists
    assert _match([], [(8.0, 8.0)])[3] == 0 and _match([(8.0, 8.0)], [])[1].tolist() == [M.NO_CANDIDATE]


def test_predictor_interpolation_and_clamp():
    xc, yc = np.array([4.0, 8.0, 12.0]), np.array([2.0, 10.0])
    up = np.array([[0.0, 1.0, 3.0], [4.0, 5.0, 7.0]])
    vp = -up
    for (x, y), want in {(4.0, 2.0): 0.0, (6.0, 2.0): 0.5, (12.0, 10.0): 7.0, (10.0, 6.0): 4.0, (0.0, 0.0): 0.0,
                         (16.0, 16.0): 7.0, (8.0, 16.0): 5.0, (0.0, 6.0): 2.0}.items():
        px, py = M.predicted(np.float64(x), np.float64(y), up, vp, xc, yc)
        assert (px - x, py - y) == (want, -want), (x, y)
    one = (np.full((1, 1), 0.5), np.full((1, 1), -0.25), np.array([3.0]), np.array([3.0]))
    assert M.predicted(np.float64(10.0), np.float64(1.0), *one) == (10.5, 0.75)


def test_tracks_arg():
    from torchpiv_amd import engine
    assert engine.tracks_arg(40) == {"level": 40, "radius": 1.5}
    assert engine.tracks_arg(np.uint8(255), radius=8) == {"level": 255, "radius": 8.0}
    for bad in (None, 0, 256, -1, 40.0, "40", True):
        with pytest.raises(ValueError, match="level"):
            engine.tracks_arg(bad)
    for bad in (0, -1.0, 8.5, float("nan"), float("inf"), "1.5", None, True):
        with pytest.raises(ValueError, match="radius"):
            engine.tracks_arg(40, bad)
    assert engine.particle_table().tobytes() == M.table().tobytes()
    assert engine.PARTICLE_STATUS == {"matched": M.MATCHED, "no_candidate": M.NO_CANDIDATE, "lost_claim": M.LOST_CLAIM,
                                      "outside": M.OUTSIDE, "no_particle": M.NO_PARTICLE}
