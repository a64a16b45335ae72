"""tracks() on the device: tpiv_particle_count / _detect / _match (particles.hip) against the numpy model of
tests/tracks_model.py bit for bit -- positions as uint64 views, every integer output, row_start, counts --, the capacity
contract, the argument errors, and the generator of ResidentPIV / OfflinePIV against engine.particle_match(
engine.particle_detect(...)) of each tuple's own frames and field."""
import ctypes as C

import numpy as np
import pytest
import torch

import tracks_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# detection
# ---------------------------------------------------------------------------------------------------------------------
# one interior pixel; a row that crosses a 64-lane boundary (4 pixels per lane: also one that does not fill a step); an odd
# width (the byte-wise tail), the batch stride and more rows than a workgroup's four; a row of more than one 256-pixel step
# with more than 64 peaks in it at batch 2
SHAPES = [(1, 3, 3), (2, 5, 70), (3, 67, 131), (2, 130, 257)]
CONTENTS = ["mixed", "zero", "lattice", "checker", "noise"]


def _content(shape, kind, seed=0):
    n, H, W = shape
    rng = np.random.default_rng(seed + 17 * H + W)
    f = np.zeros(shape, dtype=np.uint8)
    if kind == "zero":
        return f
    if kind == "lattice":                             # a peak at every odd (row, column): the densest list there is
        f[:, 1::2, 1::2] = rng.integers(60, 256, f[:, 1::2, 1::2].shape)
        return f
    if kind == "checker":                             # equal diagonal neighbours: the strict half of the tie rule
        r, c = np.mgrid[0:H, 0:W]
        f[:, (r + c) % 2 == 0] = 200
        f[:, 1::4, 1::4] = 201
        return f
    if kind == "noise":
        return rng.integers(0, 256, shape).astype(np.uint8)
    # mixed: sparse spots with a halo, plateaus of equal pixels up to 4 x 4, saturated blocks, peaks in the first and last
    # interior rows and columns, bright border pixels
    for k in range(n):
        for _ in range(max(1, H * W // 40)):
            r, c = rng.integers(0, H), rng.integers(0, W)
            v = int(rng.integers(30, 256))
            f[k, max(r - 1, 0):r + 2, max(c - 1, 0):c + 2] = np.maximum(f[k, max(r - 1, 0):r + 2, max(c - 1, 0):c + 2], v // 3)
            f[k, r, c] = v
        for _ in range(max(1, H * W // 300)):
            r, c = rng.integers(0, H), rng.integers(0, W)
            h, w = rng.integers(1, 5, 2)
            f[k, r:r + h, c:c + w] = 255 if rng.random() < 0.5 else int(rng.integers(50, 255))
        f[k, 1, 1] = f[k, 1, W - 2] = f[k, H - 2, 1] = f[k, H - 2, W - 2] = 250
        f[k, 0, ::3] = 255
        f[k, H - 1, 1::3] = 255
        f[k, ::2, 0] = 255
        f[k, 1::2, W - 1] = 255
    return f


def _check_detect(eng, frames, level, mask=None, capacity=None):
    dev = torch.from_numpy(frames).cuda()
    mdev = None if mask is None else torch.from_numpy(mask).cuda()
    keep = dev.clone(), None if mdev is None else mdev.clone()
    p = eng.particle_detect(dev, level, mask=mdev, capacity=capacity)
    torch.cuda.synchronize()
    assert dev.equal(keep[0]) and (mdev is None or mdev.equal(keep[1]))          # the inputs are never written
    lists, row_start, count = M.detect(frames, level, mask)
    n, H, W = frames.shape
    x, y, peak, rs, cnt = (t.cpu().numpy() for t in p)
    assert x.dtype == np.float64 and y.dtype == np.float64 and peak.dtype == np.uint8
    assert rs.dtype == np.int32 and cnt.dtype == np.int32 and rs.shape == (n, H + 1) and cnt.shape == (n,)
    assert cnt.tobytes() == count.tobytes(), (cnt, count)
    assert rs.tobytes() == row_start.tobytes(), np.argwhere(rs != row_start)[:5]
    cap = int(count.max()) if capacity is None else capacity
    assert x.shape == y.shape == peak.shape == (n, cap)
    for k, (lx, ly, lp) in enumerate(lists):
        m = min(len(lx), cap)
        assert _bits(x[k, :m]).tobytes() == _bits(lx[:m]).tobytes(), (k, np.flatnonzero(_bits(x[k, :m]) != _bits(lx[:m]))[:5])
        assert _bits(y[k, :m]).tobytes() == _bits(ly[:m]).tobytes(), (k, np.flatnonzero(_bits(y[k, :m]) != _bits(ly[:m]))[:5])
        assert peak[k, :m].tobytes() == lp[:m].tobytes(), k
    return lists, row_start, count


@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=["3x3", "5x70", "67x131", "130x257"])
def test_detect_equals_the_model_bit_for_bit(eng, shape, kind):
    frames = _content(shape, kind)
    lists, row_start, count = _check_detect(eng, frames, 40)
    if kind == "zero":
        assert count.tolist() == [0] * shape[0] and not row_start.any()
    if kind == "lattice":
        assert count.tolist() == [((shape[1] - 1) // 2) * ((shape[2] - 1) // 2)] * shape[0]
        if shape[2] == 257:
            assert np.diff(row_start[0]).max() == 128                           # more than 64 peaks in one row
    for lx, ly, lp in lists:                          # no border pixel is reported, however bright
        assert len(lx) == 0 or (lx.min() >= 0.5 and lx.max() <= shape[2] - 1.5 and ly.min() >= 0.5 and ly.max() <= shape[1] - 1.5)


@pytest.mark.parametrize("level", [0, 1, 200, 255])
def test_detect_levels(eng, level):
    _check_detect(eng, _content((2, 21, 77), "mixed", seed=level), level)
    _check_detect(eng, _content((1, 9, 9), "noise", seed=level), level)


def test_detect_mask_hides_peaks(eng):
    shape = (3, 67, 131)
    frames = _content(shape, "mixed", seed=5)
    free = M.detect(frames, 40)[2]
    mask = np.zeros(shape[1:], dtype=np.uint8)
    mask[10:40, 20:90] = 1
    mask[::7, ::5] = 200                                # any non-zero byte masks
    lists, row_start, count = _check_detect(eng, frames, 40, mask=mask)
    assert (count < free).all() and (count > 0).all()
    for lx, ly, lp in lists:
        # (the peak pixel of a position: the offset lies in (-1/2, 1/2], the upper end up to rounding)
        assert not mask[np.ceil(ly - 0.5 - 1e-9).astype(int), np.ceil(lx - 0.5 - 1e-9).astype(int)].any()


def test_detect_capacity(eng):
    """A capacity below the count: the true count and row_start, the stored prefix equal to the model's; through the C ABI
    with a buffer longer than the capacity: nothing behind the capacity is written."""
    from torchpiv_amd import _lib
    shape = (2, 67, 131)
    frames = _content(shape, "lattice", seed=2)
    lists, row_start, count = _check_detect(eng, frames, 40, capacity=100)
    assert count.min() > 100
    _check_detect(eng, frames, 40, capacity=0)
    _check_detect(eng, frames, 40, capacity=int(count.max()) + 50)
    one = frames[:1]
    dev = torch.from_numpy(one).cuda()
    n, H, W = one.shape
    cap, pad = 37, 19
    rs = torch.empty(1, H + 1, dtype=torch.int32, device="cuda")
    cnt = torch.empty(1, dtype=torch.int32, device="cuda")
    x = torch.full((cap + pad,), -7.25, dtype=torch.float64, device="cuda")
    y = torch.full((cap + pad,), -7.25, dtype=torch.float64, device="cuda")
    peak = torch.full((cap + pad,), 77, dtype=torch.uint8, device="cuda")
    tab = torch.from_numpy(eng.particle_table()).cuda()
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib.tpiv_particle_count(dev.data_ptr(), 1, H, W, 40, None, rs.data_ptr(), cnt.data_ptr(), st))
    _lib.check(_lib.lib.tpiv_particle_detect(dev.data_ptr(), 1, H, W, 40, None, tab.data_ptr(), rs.data_ptr(), cap, x.data_ptr(),
                                             y.data_ptr(), peak.data_ptr(), st))
    torch.cuda.synchronize()
    assert int(cnt[0]) == int(count[0]) and rs.cpu().numpy().tobytes() == row_start[:1].tobytes()
    assert _bits(x[:cap].cpu().numpy()).tobytes() == _bits(lists[0][0][:cap]).tobytes()
    assert _bits(y[:cap].cpu().numpy()).tobytes() == _bits(lists[0][1][:cap]).tobytes()
    assert peak[:cap].cpu().numpy().tobytes() == lists[0][2][:cap].tobytes()
    assert (x[cap:] == -7.25).all() and (y[cap:] == -7.25).all() and (peak[cap:] == 77).all()


def test_detect_argument_errors(eng):
    from torchpiv_amd import _lib
    ok = torch.zeros(2, 8, 8, dtype=torch.uint8, device="cuda")
    for bad in (torch.zeros(1, 2, 8, dtype=torch.uint8, device="cuda"), torch.zeros(1, 8, 2, dtype=torch.uint8, device="cuda"),
                torch.zeros(2, 7, dtype=torch.uint8, device="cuda"), torch.zeros(8, dtype=torch.uint8, device="cuda")):
        with pytest.raises(ValueError):
            eng.particle_detect(bad, 40)
    with pytest.raises(TypeError):
        eng.particle_detect(ok.float(), 40)
    with pytest.raises(TypeError):
        eng.particle_detect(ok, 40, mask=torch.zeros(8, 8, dtype=torch.bool, device="cuda"))
    with pytest.raises(RuntimeError):
        eng.particle_detect(ok.cpu(), 40)
    for bad in (dict(level=256), dict(level=-1), dict(level=1.5), dict(level=40, capacity=-1), dict(level=40, capacity=2.0),
                dict(level=40, mask=torch.zeros(8, 9, dtype=torch.uint8, device="cuda"))):
        with pytest.raises(ValueError):
            eng.particle_detect(ok, **bad)
    p = eng.particle_detect(ok[0], 40)                # a 2-D input: outputs without the frame axis
    assert p.x.shape == (0,) and p.row_start.shape == (9,) and p.count.shape == () and int(p.count) == 0
    # the C ABI refuses before it launches
    rs = torch.empty(2, 9, dtype=torch.int32, device="cuda")
    cnt = torch.empty(2, dtype=torch.int32, device="cuda")
    lib = _lib.lib
    assert lib.tpiv_particle_count(ok.data_ptr(), 2, 2, 8, 40, None, rs.data_ptr(), cnt.data_ptr(), None) == _lib.EINVAL
    assert lib.tpiv_particle_count(ok.data_ptr(), 2, 8, 8, 256, None, rs.data_ptr(), cnt.data_ptr(), None) == _lib.EINVAL
    assert lib.tpiv_particle_count(None, 2, 8, 8, 40, None, rs.data_ptr(), cnt.data_ptr(), None) == _lib.EINVAL
    assert lib.tpiv_particle_count(ok.data_ptr(), 2, 8, 8, 40, None, None, cnt.data_ptr(), None) == _lib.EINVAL
    assert lib.tpiv_particle_count(ok.data_ptr(), 2, 8, 8, 40, None, ok.data_ptr(), cnt.data_ptr(), None) == _lib.EINVAL
    assert lib.tpiv_particle_detect(ok.data_ptr(), 2, 8, 8, 40, None, None, rs.data_ptr(), 4, None, None, None, None) == _lib.EINVAL
    assert lib.tpiv_particle_count(ok.data_ptr(), 0, 8, 8, 40, None, rs.data_ptr(), cnt.data_ptr(), None) == _lib.OK


# ---------------------------------------------------------------------------------------------------------------------
# matching
# ---------------------------------------------------------------------------------------------------------------------
def _raster(points):
    """Hand-made points (x, y) in raster order: by row floor(y + 1/2), then by x."""
    return sorted(points, key=lambda p: (np.floor(p[1] + 0.5), p[0]))


def _particles(eng, lists, H):
    """Particles of hand-made lists [(x, y), ...] per frame (raster order), padded to the longest, on the device."""
    n, cap = len(lists), max([len(pts) for pts in lists] + [0])
    x, y = np.zeros((n, cap)), np.zeros((n, cap))
    rs = np.zeros((n, H + 1), dtype=np.int32)
    for k, pts in enumerate(lists):
        assert pts == _raster(pts)
        if pts:
            x[k, :len(pts)], y[k, :len(pts)] = zip(*pts)
            rs[k, 1:] = np.cumsum(np.bincount(np.floor(y[k, :len(pts)] + 0.5).astype(int), minlength=H))
    dev = [torch.from_numpy(a).cuda() for a in (x, y, np.zeros((n, cap), dtype=np.uint8), rs, rs[:, H].copy())]
    return eng.Particles(*dev), x, y, rs


def _check_match(eng, a_lists, b_lists, up, vp, xc, yc, radius, shape):
    H, W = shape
    pa, xa, ya, rsa = _particles(eng, a_lists, H)
    pb, xb, yb, rsb = _particles(eng, b_lists, H)
    upd, vpd = torch.from_numpy(np.ascontiguousarray(up)).cuda(), torch.from_numpy(np.ascontiguousarray(vp)).cuda()
    keep = [t.clone() for t in tuple(pa) + tuple(pb) + (upd, vpd)]
    got = eng.particle_match(pa, pb, upd, vpd, xc, yc, radius, shape)
    torch.cuda.synchronize()
    for t, k in zip(tuple(pa) + tuple(pb) + (upd, vpd), keep):                  # the inputs are not written
        assert t.view(torch.uint8).equal(k.view(torch.uint8))
    match, status, d2, matched = (t.cpu().numpy() for t in got)
    n, cap = xa.shape
    assert match.dtype == np.int32 and status.dtype == np.uint8 and d2.dtype == np.float64 and matched.dtype == np.int32
    assert match.shape == status.shape == d2.shape == (n, cap) and matched.shape == (n,)
    want = []
    for k in range(n):
        na, nb = len(a_lists[k]), len(b_lists[k])
        m, s, dd, cnt = M.match(xa[k, :na], ya[k, :na], xb[k, :nb], yb[k, :nb], rsb[k], up[k], vp[k], xc, yc, radius, shape)
        assert match[k, :na].tolist() == m.tolist(), (k, match[k, :na], m)
        assert status[k, :na].tolist() == s.tolist(), (k, status[k, :na], s)
        assert _bits(d2[k, :na]).tobytes() == _bits(dd).tobytes(), (k, d2[k, :na], dd)
        assert int(matched[k]) == cnt
        assert (match[k, na:] == -1).all() and (status[k, na:] == M.NO_PARTICLE).all() and (_bits(d2[k, na:]) == M.NAN_BITS).all()
        want.append((m, s, dd, cnt))
    return want


def test_match_hand_made_cases(eng):
    """Dyadic coordinates, so every tie is exact; a 1 x 1 predictor grid; the cases share one call as a batch of pairs of
    unequal lengths."""
    H = W = 17
    cases = [
        ([], [(8.0, 8.0)], 0.0, 0.0),                                             # empty a
        ([(8.0, 8.0)], [], 0.0, 0.0),                                             # empty b
        ([], [], 0.0, 0.0),
        ([(3.0, 2.0), (9.0, 2.0), (4.0, 7.0), (12.0, 11.0)],                      # a uniform shift, one-to-one
         [(4.5, 1.0), (10.5, 1.0), (5.5, 6.0), (13.5, 10.0)], 1.25, -1.25),
        ([(7.0, 8.0), (8.5, 8.0)], [(8.0, 8.0)], 0.0, 0.0),                       # two claimants: the nearer wins
        ([(7.5, 8.0), (8.5, 8.0), (8.0, 8.5)], [(8.0, 8.0)], 0.0, 0.0),           # equally near: the lower i
        ([(8.0, 8.0)], [(7.0, 8.0), (9.0, 8.0)], 0.0, 0.0),                       # two equidistant candidates: the lower j
        ([(8.0, 8.0)], [(8.0, 7.0), (8.0, 9.0)], 0.0, 0.0),                       #   ... in two rows
        ([(8.0, 8.0)], [(9.5, 8.0)], 0.0, 0.0),                                   # a candidate at exactly R
        ([(8.0, 6.5)], [(8.0, 8.0)], 0.0, 0.0),                                   #   ... along the rows (row range edge)
        ([(8.0, 8.0)], [(9.75, 8.0)], 0.0, 0.0),                                  # just outside R: status 1
        ([(8.0, 8.0), (8.25, 8.0)], [(7.0, 8.0), (8.25, 8.0)], 0.0, 0.0),         # the loser takes no second candidate
        ([(15.0, 8.0), (14.5, 8.0), (8.0, 1.0)], [(16.0, 8.0)], 1.5, 0.0),        # predicted outside: status 3; the edge is in
        ([(1.0, 0.0), (15.0, 0.25), (2.0, 16.0), (9.0, 16.0)],                    # the first and last rows: the row clamp
         [(1.5, -0.25), (15.0, 0.0), (2.0, 15.0), (2.5, 16.0), (9.0, 16.25)], 0.0, 0.0),
    ]
    a_lists = [_raster(c[0]) for c in cases]
    b_lists = [_raster(c[1]) for c in cases]
    up = np.array([c[2] for c in cases]).reshape(-1, 1, 1)
    vp = np.array([c[3] for c in cases]).reshape(-1, 1, 1)
    want = _check_match(eng, a_lists, b_lists, up, vp, [8.0], [8.0], 1.5, (H, W))
    assert [w[3] for w in want] == [0, 0, 0, 4, 1, 1, 1, 1, 1, 1, 0, 1, 1, 4]
    assert want[4][1].tolist() == [2, 0] and want[5][0].tolist() == [0, -1, -1] and want[6][0].tolist() == [0]
    assert want[8][2].tolist() == [2.25] and want[10][1].tolist() == [1] and want[12][1].tolist() == [1, 0, 3]


@pytest.mark.parametrize("grid", [(1, 1), (1, 5), (5, 1), (3, 4)], ids=["1x1", "1x5", "5x1", "3x4"])
def test_match_random_lists_and_predictor_grids(eng, grid):
    """Three pairs of a few hundred particles at quarter-pixel positions -- many exact ties and contested candidates --
    under a predictor on every grid shape, with particles outside the centre grid: the verdicts do not depend on
    scheduling, so they are the model's in every run."""
    H, W = 40, 300                                     # a_lists of more than one 256-lane workgroup
    nr, nc = grid
    rng = np.random.default_rng(11 + 10 * nr + nc)
    xc = np.linspace(60.0, 240.0, nc) if nc > 1 else np.array([150.0])
    yc = np.linspace(10.0, 30.0, nr) if nr > 1 else np.array([20.0])
    a_lists, b_lists = [], []
    for k in range(3):
        for lists, count in ((a_lists, 700 - 150 * k), (b_lists, 650)):
            cells = rng.choice(H * W, count, replace=False)
            r, c = cells // W, cells % W
            pts = zip(c + rng.integers(-1, 2, count) / 4.0, r + rng.integers(-1, 2, count) / 4.0)
            lists.append(_raster([(float(x), float(y)) for x, y in pts]))
    up = rng.integers(-8, 9, (3, nr, nc)) / 4.0
    vp = rng.integers(-8, 9, (3, nr, nc)) / 4.0
    want = _check_match(eng, a_lists, b_lists, up, vp, xc, yc, 1.5, (H, W))
    seen = np.concatenate([w[1] for w in want])
    assert {0, 1, 2, 3} <= set(seen.tolist())          # every status occurs
    again = _check_match(eng, a_lists, b_lists, up, vp, xc, yc, 1.5, (H, W))
    assert all(x[0].tolist() == y[0].tolist() for x, y in zip(want, again))


def test_match_capped_lists(eng):
    """Lists stored with a capacity below their count: the particles behind it take no part, on either side."""
    frames = _content((2, 40, 60), "lattice", seed=4)
    dev = torch.from_numpy(frames).cuda()
    full = eng.particle_detect(dev, 40)
    capped = eng.particle_detect(dev, 40, capacity=150)
    assert int(full.count.min()) > 150
    H, W = frames.shape[1:]
    lists, row_start, count = M.detect(frames, 40)
    pa = eng.Particles(*(t[:1] for t in capped))
    pb = eng.Particles(*(t[1:] for t in capped))
    zero = torch.zeros(1, 1, 1, dtype=torch.float64, device="cuda")
    got = eng.particle_match(pa, pb, zero, zero, [30.0], [20.0], 1.0, (H, W))
    m, s, dd, cnt = M.match(lists[0][0][:150], lists[0][1][:150], lists[1][0][:150], lists[1][1][:150], row_start[1],
                            np.zeros((1, 1)), np.zeros((1, 1)), [30.0], [20.0], 1.0, (H, W))
    assert got.match[0].cpu().numpy().tolist() == m.tolist() and got.status[0].cpu().numpy().tolist() == s.tolist()
    assert _bits(got.d2[0].cpu().numpy()).tobytes() == _bits(dd).tobytes() and int(got.matched[0]) == cnt
    assert cnt > 0 and (m < 150).all()


def test_match_argument_errors(eng):
    from torchpiv_amd import _lib
    pa, *_ = _particles(eng, [[(8.0, 8.0)]], 17)
    pb, *_ = _particles(eng, [[(8.0, 8.0)]], 17)
    z = torch.zeros(1, 1, 1, dtype=torch.float64, device="cuda")
    ok = dict(pa=pa, pb=pb, up=z, vp=z, xc=[8.0], yc=[8.0], radius=1.5, shape=(17, 17))
    assert int(eng.particle_match(**ok).matched[0]) == 1
    for bad in (dict(radius=0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(radius="1"),
                dict(xc=[8.0, 9.0]), dict(yc=[]), dict(shape=(16, 17)), dict(up=z[0]), dict(vp=torch.zeros(1, 1, 2, dtype=torch.float64, device="cuda")),
                dict(up=torch.zeros(2, 1, 1, dtype=torch.float64, device="cuda"), vp=torch.zeros(2, 1, 1, dtype=torch.float64, device="cuda"))):
        with pytest.raises(ValueError):
            eng.particle_match(**dict(ok, **bad))
    z2 = torch.zeros(1, 1, 2, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="ascending"):
        eng.particle_match(**dict(ok, up=z2, vp=z2, xc=[8.0, 8.0]))
    for bad in (dict(up=z.float()), dict(pa=tuple(pa)), dict(pb=None)):
        with pytest.raises(TypeError):
            eng.particle_match(**dict(ok, **bad))
    with pytest.raises(RuntimeError):
        eng.particle_match(**dict(ok, up=z.cpu()))
    one = eng.particle_match(eng.Particles(*(t[0] for t in pa)), eng.Particles(*(t[0] for t in pb)), z[0], z[0], [8.0], [8.0], 1.5, (17, 17))
    assert one.match.shape == (1,) and one.matched.shape == () and int(one.matched) == 1
    # the C ABI refuses before it launches
    out = [torch.empty(1, dtype=dt, device="cuda") for dt in (torch.int32, torch.uint8, torch.float64, torch.int32)]
    work = torch.empty(2, dtype=torch.int64, device="cuda")
    cen = torch.tensor([8.0, 8.0], dtype=torch.float64, device="cuda")

    def call(radius=1.5, work_bytes=16, n_cols=1, rsa=pa.row_start.data_ptr(), match=out[0].data_ptr()):
        return _lib.lib.tpiv_particle_match(pa.x.data_ptr(), pa.y.data_ptr(), rsa, 1, pb.x.data_ptr(), pb.y.data_ptr(),
                                            pb.row_start.data_ptr(), 1, 1, 17, 17, z.data_ptr(), z.data_ptr(), 1, n_cols,
                                            cen.data_ptr(), cen[1:].data_ptr(), radius, match, out[1].data_ptr(),
                                            out[2].data_ptr(), out[3].data_ptr(), work.data_ptr(), C.c_size_t(work_bytes), None)
    assert call() == _lib.OK
    torch.cuda.synchronize()
    assert int(out[0][0]) == 0 and int(out[3][0]) == 1
    assert call(radius=0.0) == _lib.EINVAL and call(radius=float("nan")) == _lib.EINVAL
    assert call(work_bytes=15) == _lib.EINVAL and call(n_cols=0) == _lib.EINVAL and call(rsa=None) == _lib.EINVAL
    assert call(match=pa.x.data_ptr()) == _lib.EINVAL                            # an output aliases an input


# ---------------------------------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------------------------------
H, W = M.SCENE_SHAPE
KW = dict(multipass=2, multipass_mode="CWS")


def _scene_pair(seed, shift=M.scene_shift):
    """The host test's scene; a square of noise in frame b makes a few vectors of the last pass fail the peak ratio, so
    that the post-validation does not drop the pair for having no invalid vector."""
    a, b = M.scene(seed=seed, shift=shift)[:2]
    b = b.copy()
    b[40:54, 100:114] = np.random.default_rng(3).integers(0, 256, (14, 14)).astype(np.uint8)
    return a, b


@pytest.fixture(scope="module")
def scene_pairs():
    """Three pairs: the scene, the scene at another seed, the scene again."""
    pairs = [_scene_pair(7), _scene_pair(11), _scene_pair(7)]
    return (torch.from_numpy(np.stack([p[0] for p in pairs])), torch.from_numpy(np.stack([p[1] for p in pairs])))


def _expected_tracks(eng, piv, fa, fb, raw, mask=None):
    """Tracks from engine.particle_match(engine.particle_detect(...)) of one pair's prepared frames fa, fb (device, [H, W])
    and raw field (numpy u, v), and the same from the numpy model."""
    plan = piv._plan
    w, o = plan.geometry[-1][:2]
    nr, nc = raw[0].shape
    xc, yc = M.window_centres(W, w, o), M.window_centres(H, w, o)
    assert (len(yc), len(xc)) == (nr, nc)
    mdev = None if mask is None else torch.from_numpy(mask).cuda()
    pa, pb = eng.particle_detect(fa, 40, mask=mdev), eng.particle_detect(fb, 40, mask=mdev)
    up, vp = (torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in raw)
    m = eng.particle_match(pa, pb, up, vp, xc, yc, 1.5, (H, W))
    xa, ya, ka, xb, yb, kb, match, status, d2 = (t.cpu().numpy() for t in (pa.x, pa.y, pa.peak, pb.x, pb.y, pb.peak, m.match,
                                                                           m.status, m.d2))
    ia = np.flatnonzero(status == 0)
    ib = match[ia]
    s, dt = piv._scale, piv._dt
    dev = (xa[ia] * s, ya[ia] * s, (xb[ib] - xa[ia]) * s / dt * 1000, -(yb[ib] - ya[ia]) * s / dt * 1000, np.sqrt(d2[ia]),
           ka[ia], kb[ib], int(pa.count), int(pb.count), int(m.matched))
    frames = np.stack([fa.cpu().numpy(), fb.cpu().numpy()])
    lists, row_start, count = M.detect(frames, 40, mask)
    mm, ms, md, mc = M.match(lists[0][0], lists[0][1], lists[1][0], lists[1][1], row_start[1], raw[0], raw[1], xc, yc, 1.5, (H, W))
    ja = np.flatnonzero(ms == 0)
    jb = mm[ja]
    model = (lists[0][0][ja] * s, lists[0][1][ja] * s, (lists[1][0][jb] - lists[0][0][ja]) * s / dt * 1000,
             -(lists[1][1][jb] - lists[0][1][ja]) * s / dt * 1000, np.sqrt(md[ja]), lists[0][2][ja], lists[1][2][jb],
             int(count[0]), int(count[1]), mc)
    return dev, model


def _same_tracks(t, want):
    assert type(t).__name__ == "Tracks" and t._fields == ("x", "y", "u", "v", "residual", "peak_a", "peak_b", "count_a",
                                                          "count_b", "matched")
    for name, g, w in zip(t._fields, t, want):
        if isinstance(w, np.ndarray):
            assert isinstance(g, np.ndarray) and g.dtype == w.dtype and g.tobytes() == w.tobytes(), name
        else:
            assert g == w, name
    assert len(t.x) == t.matched


def _raw_fields(piv, A, B):
    """The raw filled fields of the pairs A, B through the object's own plan, as _one makes them (None: dropped)."""
    plan = piv._get_plan(H, W, max_batch=A.shape[0])
    u, v, inv = plan.run(A, B)
    return piv._post_validate_batch(u, v, inv, plan=plan, sigma=False)


def test_resident_tracks(eng, scene_pairs):
    import torchpiv_amd as T
    A, B = (t.cuda() for t in scene_pairs)
    piv = T.ResidentPIV(A, B, 32, 16, **KW)
    fields = {o[0]: o[1:] for o in piv.batched(3)}
    outs = list(piv.tracks(level=40, batch_size=3))
    assert [o[0] for o in outs] == sorted(fields) == [0, 1, 2] and all(len(o) == 6 for o in outs)
    raw = _raw_fields(piv, A, B)
    for i, x, y, u, v, t in outs:
        for g, w in zip((x, y, u, v), fields[i]):      # what batched() delivers for the pair
            assert isinstance(g, np.ndarray) and g.tobytes() == np.asarray(w).tobytes()
        fin = piv._finish(raw[i], *np.meshgrid(*eng.coordinates_1d(H, W, *piv._plan.geometry[-1][:2])), plan=piv._plan, derive=False)
        assert fin[2].tobytes() == u.tobytes() and fin[3].tobytes() == v.tobytes()      # raw[i] is this tuple's field
        dev, model = _expected_tracks(eng, piv, A[i], B[i], raw[i])
        _same_tracks(t, dev)
        _same_tracks(t, model)
        assert t.count_a == 180 and t.matched >= 150 and t.residual.max() <= 1.5
    assert outs[0][5].x.tobytes() == outs[2][5].x.tobytes() and outs[0][5].x.tobytes() != outs[1][5].x.tobytes()
    # another batch size, a subset in another order: the same tracks
    sub = list(piv.tracks(40, indices=[2, 0], batch_size=1))
    assert [o[0] for o in sub] == [2, 0] and sub[1][5].u.tobytes() == outs[0][5].u.tobytes()
    # scale and dt reach the tracks as they reach the fields
    scaled = T.ResidentPIV(A, B, 32, 16, scale=0.5, dt=4, **KW)
    for o, p in zip(scaled.tracks(40, batch_size=3), outs):
        assert o[5].x.tobytes() == (p[5].x * 0.5).tobytes() and o[5].residual.tobytes() == p[5].residual.tobytes()
        px = p[5].u / 1000
        assert np.allclose(o[5].u, px * 0.5 / 4 * 1000, rtol=1e-14, atol=0)
    scaled.close()
    piv.close()


def test_uniform_shift_pins_the_convention(eng):
    """Frame b = frame a moved 3 px toward larger columns and 2 px toward smaller rows (up in the image): u > 0 and v > 0,
    3 and 2 px per frame in the delivered units.  A raw field read with the wrong axis or sign would predict 4 to 6 px
    off: nothing would be matched within the radius."""
    import torchpiv_amd as T
    a, b = _scene_pair(7, shift=lambda x, y: (3.0 + 0 * x, -2.0 + 0 * y))
    A, B = torch.from_numpy(a[None]).cuda(), torch.from_numpy(b[None]).cuda()
    piv = T.ResidentPIV(A, B, 32, 16, **KW)
    outs = list(piv.tracks(level=40))
    piv.close()
    assert len(outs) == 1
    i, x, y, u, v, t = outs[0]
    assert t.count_a == 180 and t.matched >= 150
    assert (t.u > 0).all() and (t.v > 0).all()
    # within 0.05 px, away from the square of noise (where a noise peak inside the radius may stand in for the particle)
    bx, by = t.x + 3, t.y - 2
    away = ~((bx > 96) & (bx < 118) & (by > 36) & (by < 58))
    assert away.sum() >= 150 and np.abs(t.u[away] - 3000).max() < 50 and np.abs(t.v[away] - 2000).max() < 50
    assert np.median(u) > 0 and np.median(v) > 0                                # the delivered field's signs, the same
    assert t.x.min() > 0 and t.x.max() < W and t.y.min() > 0 and t.y.max() < H


def test_offline_tracks_equal_resident(eng, tmp_path):
    """Three small BMPs read as sequential pairs: the tracks ResidentPIV gives on the same frames."""
    import torchpiv_amd as T
    from PIL import Image
    a, b = _scene_pair(7)
    a2 = _scene_pair(11)[1]
    frames = [a, b, a2]
    for k, f in enumerate(frames):
        Image.fromarray(f, "L").save(tmp_path / f"image{k}.bmp")
    off = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", 32, 16, folder_mode="sequential", **KW)
    got = list(off.tracks(level=40, radius=2.0, batch_size=2))
    plain = {o[0]: o[1:] for o in off.batched(2)}
    off.close()
    A = torch.from_numpy(np.stack(frames[:2])).cuda()
    B = torch.from_numpy(np.stack(frames[1:])).cuda()
    res = T.ResidentPIV(A, B, 32, 16, **KW)
    want = list(res.tracks(level=40, radius=2.0, batch_size=2))
    res.close()
    assert [o[0] for o in got] == [o[0] for o in want] == sorted(plain) and len(got) >= 1
    for g, w in zip(got, want):
        for p, q in zip(g[1:5], w[1:5]):
            assert p.tobytes() == q.tobytes()
        for p, q in zip(g[1:5], plain[g[0]]):
            assert p.tobytes() == np.asarray(q).tobytes()
        _same_tracks(g[5], tuple(w[5]))


def test_tracks_options(eng, scene_pairs):
    import torchpiv_amd as T
    A, B = (t.cuda() for t in scene_pairs)
    # dynamic_mask= is refused, at the call
    dyn = T.ResidentPIV(A, B, 32, 16, dynamic_mask={"stack": torch.zeros(3, H, W, dtype=torch.uint8)}, **KW)
    with pytest.raises(ValueError, match="dynamic_mask"):
        dyn.tracks(level=40)
    dyn.close()
    piv = T.ResidentPIV(A, B, 32, 16, **KW)
    for bad in (dict(), dict(level=0), dict(level=40.0), dict(level=40, radius=0), dict(level=40, radius=9)):
        with pytest.raises((ValueError, TypeError)):
            piv.tracks(**bad)
    assert list(piv.tracks(40, indices=[])) == []
    free = {o[0]: o[5] for o in piv.tracks(40, batch_size=3)}
    piv.close()
    # mask= removes the particles under it: none is detected there, in either frame, and none of a track lies there
    img = torch.zeros(H, W, dtype=torch.uint8)
    img[:, :40] = 1
    masked = T.ResidentPIV(A, B, 32, 16, mask={"image": img, "fill": -5.0}, **KW)
    outs = list(masked.tracks(40, batch_size=3))
    fields = {o[0]: o[1:] for o in masked.batched(3)}
    assert outs and sorted(fields) == [o[0] for o in outs]
    for i, x, y, u, v, t in outs:
        assert u.tobytes() == np.asarray(fields[i][2]).tobytes() and (u == -5.0).any()
        assert t.count_a < free[i].count_a and t.count_b < free[i].count_b and t.matched > 50
        assert t.x.min() >= 39.5 and (t.x + t.u / 1000).min() >= 39.5
    masked.close()
    # uncertainty= and derive= add nothing to the tuples of tracks()
    more = T.ResidentPIV(A, B, 32, 16, uncertainty="cs", derive=("vorticity",), **KW)
    outs = list(more.tracks(40, batch_size=3))
    assert outs and all(len(o) == 6 for o in outs)
    _same_tracks(outs[0][5], tuple(free[outs[0][0]]))
    more.close()
    # deform= works through the plan
    deform = T.ResidentPIV(A, B, 32, 16, deform=1, **KW)
    outs = list(deform.tracks(40, batch_size=3))
    assert outs and all(o[5].matched >= 150 for o in outs)
    deform.close()
