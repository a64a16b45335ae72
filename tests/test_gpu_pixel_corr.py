"""Single-pixel ensemble correlation on the device against the numpy model (tests/pixel_corr_model.py): the accumulators bit
for bit, the peaks on the model's and on prescribed accumulators, ResidentPIV / OfflinePIV.single_pixel end to end, the
refusals and the memory contract of the three entry points.

The memory-contract cases are registered at import in tests/test_gpu_memory_contract.py's table (entry(...)), so that its
test_every_symbol_is_exercised_or_exempt sees the three symbols in a suite run, where every module is imported before any
test runs; this module runs them itself under the three (poison, guard) settings.  Selecting the old file alone does not
import this one and will report the three symbols as unexercised."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import guarded
import pixel_corr_model as M
import test_gpu_memory_contract as MC
from test_pixel_corr_host import CAP_MAX, CAP_RMS

pytestmark = pytest.mark.gpu

DEV = "cuda"
EINVAL = 1
H0, W0 = 37, 45
BINS = ((1, 1), (2, 3), (1, 45), (16, 16))
RADII = (3, 8, 16)
SHIFTS = ((0, 0), (2, -3), (-5, 4))
CALLS = ((1, 4), (4, 5), (5, 9), (9, 1))                 # two successive calls into one accumulator


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def dev(t):
    return torch.from_numpy(np.array(t)).to(DEV)      # (a copy: the source may be read-only)


def odd(t):
    """The uint8 array on the device, its first byte at an odd address."""
    t = torch.from_numpy(np.array(t))                # (a copy: the source may be read-only)
    buf = torch.empty(t.numel() + 1, dtype=torch.uint8, device=DEV)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    return view


@functools.lru_cache(maxsize=None)
def random_pairs():
    """(A, B) uint8 [14, 37, 45]: uniform over 0..255, pair 3 all 255 in both frames."""
    rng = np.random.default_rng(20240607)
    A = rng.integers(0, 256, (14, H0, W0)).astype(np.uint8)
    B = rng.integers(0, 256, (14, H0, W0)).astype(np.uint8)
    A[3] = 255
    B[3] = 255
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


@functools.lru_cache(maxsize=1)
def products(radius, shift, n):
    """(P int64 [D, D, H, W]: the per-pixel products of the first n pairs summed over the pairs, mom): the model's sums before
    the bins, shared by the four bin shapes."""
    A, B = random_pairs()
    acc, mom = M.accumulate(A[:n], B[:n], (1, 1), radius, shift)
    return np.ascontiguousarray(acc.transpose(2, 3, 0, 1)), mom


@pytest.mark.parametrize("shift", SHIFTS, ids=lambda s: f"s{s[0]}_{s[1]}")
@pytest.mark.parametrize("radius", RADII)
def test_accumulators_are_the_models_bits(eng, radius, shift):
    A, B = random_pairs()
    dA, dB = odd(A), odd(B)
    for n1, n2 in CALLS:
        P, mom = products(radius, shift, n1 + n2)
        for bin in BINS:
            acc_d, mom_d = eng.pixel_corr_add(dA[:n1], dB[:n1], bin, radius, shift)
            acc_d, mom_d = eng.pixel_corr_add(dA[n1:n1 + n2], dB[n1:n1 + n2], bin, radius, shift, acc=acc_d, mom=mom_d)
            want = M.bin_sums(P, bin).transpose(2, 3, 0, 1)
            got = acc_d.cpu().numpy()
            assert got.shape == want.shape and got.nbytes == eng.pixel_corr_bytes(H0, W0, bin, radius)
            bad = np.argwhere(got != want)
            assert not len(bad), (bin, radius, shift, (n1, n2), len(bad), bad[:4].tolist())
            assert np.array_equal(mom_d.cpu().numpy(), mom), (bin, radius, shift, (n1, n2))


def test_aligned_frames_take_the_dword_path_to_the_same_bits(eng):
    """W % 4 == 0 and 4-byte aligned stacks (the fast staging path), bins that start off a 4-pixel boundary, a batch beyond
    one library call's 256 pairs cut by the engine."""
    rng = np.random.default_rng(11)
    A = rng.integers(0, 256, (6, 21, 44)).astype(np.uint8)
    B = rng.integers(0, 256, (6, 21, 44)).astype(np.uint8)
    dA, dB = dev(A), dev(B)
    for bin, radius, shift in (((1, 1), 4, (0, 0)), ((2, 3), 5, (1, -2)), ((8, 8), 4, (0, 3)), ((3, 40), 3, (-1, 1))):
        acc_d, mom_d = eng.pixel_corr_add(dA, dB, bin, radius, shift)
        acc, mom = M.accumulate(A, B, bin, radius, shift)
        assert np.array_equal(acc_d.cpu().numpy(), acc) and np.array_equal(mom_d.cpu().numpy(), mom), (bin, radius, shift)
    n = 260
    A2 = np.ascontiguousarray(np.broadcast_to(A[:1], (n, 21, 44)))
    acc_d, mom_d = eng.pixel_corr_add(dev(A2), dev(A2), (1, 2), 3)
    acc, mom = M.accumulate(A[:1], A[:1], (1, 2), 3)
    assert np.array_equal(acc_d.cpu().numpy(), n * acc) and np.array_equal(mom_d.cpu().numpy(), n * mom)


# ---- peaks ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene():
    A, B = M.scene()
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


@functools.lru_cache(maxsize=None)
def scene_model(bin=M.SCENE_BIN, radius=M.SCENE_RADIUS, shift=(0, 0)):
    A, B = scene()
    acc, mom = M.accumulate(A, B, bin, radius, shift)
    return acc, mom, M.peaks(acc, mom, len(A), A.shape[1:], bin, radius, shift)


def ulps(a, b):
    """The distance of two float64 arrays in units in the last place (same-sign finite values; equal values count 0)."""
    ia, ib = np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64)
    d = np.abs(ia - ib)
    return np.where((a == b) | (np.isnan(a) & np.isnan(b)), 0, np.where(np.signbit(a) == np.signbit(b), d, np.iinfo(np.int64).max))


def check_against_model(got, want, label):
    """The gates of the issue: status identical, corr within 4 ulp, u and v within 1e-9 px, ratio within 1e-12 relative
    (peak is a cell of corr: 4 ulp); NaN exactly where the model has it."""
    status = got["status"]
    assert np.array_equal(status, want["status"]), (label, np.argwhere(status != want["status"])[:4].tolist())
    ok = want["status"] == 0
    worst_ulp = int(ulps(got["corr"], want["corr"]).max())
    print(f"  {label}: {int(ok.sum())} valid of {ok.size} bins, corr within {worst_ulp} ulp", end="")
    assert worst_ulp <= 4, (label, worst_ulp)
    for k in ("u", "v", "peak", "ratio"):
        assert np.array_equal(np.isnan(got[k]), ~ok), (label, k)
    if ok.any():
        du = max(np.abs(got["u"][ok] - want["u"][ok]).max(), np.abs(got["v"][ok] - want["v"][ok]).max())
        dr = np.abs(got["ratio"][ok] / want["ratio"][ok] - 1.0).max()
        print(f", u, v within {du:.2e} px, ratio within {dr:.2e}", end="")
        assert du <= 1e-9 and dr <= 1e-12, (label, du, dr)
        assert int(ulps(got["peak"][ok], want["peak"][ok]).max()) <= 4, label
    print()


def device_peaks(eng, acc, mom, n, shape, bin, radius, shift=(0, 0)):
    out = eng.pixel_corr_peaks(dev(acc), dev(mom), n, shape, bin, radius, shift,
                               planes=True)
    return {k: getattr(out, k).cpu().numpy() for k in out._fields}


@pytest.mark.parametrize("bin,radius,shift", [(M.SCENE_BIN, M.SCENE_RADIUS, (0, 0)), ((2, 64), 4, (0, 1)), ((4, 33), 3, (1, 2))],
                         ids=["rows", "2x64", "4x33"])
def test_peaks_on_the_models_accumulators(eng, bin, radius, shift):
    A, B = scene()
    acc, mom, want = scene_model(bin, radius, shift)
    got = device_peaks(eng, acc, mom, len(A), A.shape[1:], bin, radius, shift)
    check_against_model(got, want, f"scene {bin} R {radius} s {shift}")
    assert (want["status"] == 0).sum() >= 20


def test_status_flat(eng):
    rng = np.random.default_rng(3)
    n, H, W = 3, 20, 24
    const = np.full((n, H, W), 100, np.uint8)
    noise = rng.integers(0, 256, (n, H, W)).astype(np.uint8)
    part = noise.copy()
    part[:, 8:12, 10:14] = 9                       # b constant on a patch: vb = 0 for the bins that reach only into it
    for A, B in ((const, noise), (noise, const), (noise, part)):
        acc, mom = M.accumulate(A, B, (2, 2), 3)
        want = M.peaks(acc, mom, n, (H, W), (2, 2), 3)
        got = device_peaks(eng, acc, mom, n, (H, W), (2, 2), 3)
        check_against_model(got, want, "flat")
        inner = ~M.border_bins(H, W, (2, 2), 3)
        assert (want["status"][inner] == M.STATUS["flat"]).any()
        flat = got["status"] == M.STATUS["flat"]
        assert not got["corr"][flat].any() and not got["corr"][got["status"] == M.STATUS["border"]].any()
    assert (want["status"][inner] == 0).any()      # (the patch case keeps valid bins beside the flat ones)


def test_status_range(eng):
    """A true displacement of exactly R: the peak sits on the ring."""
    rng = np.random.default_rng(4)
    n, H, W, R = 4, 24, 40, 3
    A = rng.integers(0, 256, (n, H, W)).astype(np.uint8)
    B = np.roll(A, R, axis=2)
    acc_d, mom_d = eng.pixel_corr_add(dev(A), dev(B), (2, 4), R)
    acc, mom = M.accumulate(A, B, (2, 4), R)
    assert np.array_equal(acc_d.cpu().numpy(), acc)
    want = M.peaks(acc, mom, n, (H, W), (2, 4), R)
    got = device_peaks(eng, acc, mom, n, (H, W), (2, 4), R)
    check_against_model(got, want, "range")
    inner = ~M.border_bins(H, W, (2, 4), R)
    assert inner.any() and (got["status"][inner] == M.STATUS["range"]).all()
    assert got["corr"][inner].any()                # range keeps its plane
    # the same frames with the pre-shift on the displacement: valid, u = R
    acc, mom = M.accumulate(A, B, (2, 4), R, (0, R))
    got = device_peaks(eng, acc, mom, n, (H, W), (2, 4), R, (0, R))
    check_against_model(got, M.peaks(acc, mom, n, (H, W), (2, 4), R, (0, R)), "range, shifted")
    ok = got["status"] == 0
    assert ok.any() and np.abs(got["u"][ok] - R).max() <= 0.5 and np.abs(got["v"][ok]).max() <= 0.5     # (a one-cell peak)


@pytest.mark.parametrize("bin,radius,shift", [((1, 1), 3, (0, 0)), ((2, 3), 4, (2, -3)), ((5, 4), 3, (-5, 4)), ((16, 16), 3, (0, 0)),
                                              ((1, 45), 3, (0, 0)), ((37, 1), 3, (0, 0))])
def test_status_border_is_what_the_definition_names(eng, bin, radius, shift):
    A, B = random_pairs()
    acc, mom = M.accumulate(A[:3], B[:3], bin, radius, shift)
    got = device_peaks(eng, acc, mom, 3, (H0, W0), bin, radius, shift)
    want = M.border_bins(H0, W0, bin, radius, shift)
    assert np.array_equal(got["status"] == M.STATUS["border"], want), (bin, radius, shift)
    check_against_model(got, M.peaks(acc, mom, 3, (H0, W0), bin, radius, shift), f"border {bin}")
    # by hand for the first case: a single pixel is out of reach of an edge from R pixels in
    if bin == (1, 1):
        hand = np.ones((H0, W0), bool)
        hand[radius:H0 - radius, radius:W0 - radius] = False
        assert np.array_equal(want, hand)


def test_equal_maxima_take_the_first_in_raster_order(eng):
    """Prescribed accumulators: zero first moments and constant second moments make every denominator the same number, so
    C[d] = acc[d] x one constant and equal cells of acc are exactly equal coefficients."""
    H, W, R, n = 24, 24, 3, 5
    D = 2 * R + 1
    bin = (2, 2)
    mom = np.zeros((4, H, W), np.int64)
    mom[1] = 40000
    mom[3] = 40000
    acc = np.full((H // 2, W // 2, D, D), 1000, np.int64)
    acc[:, :, 2, 4] = acc[:, :, 4, 1] = acc[:, :, 2, 1] = 30000          # first in raster order: (2, 1)
    acc[5, 5, 1, 5] = 30000                                               # one bin: (1, 5) comes before
    acc[6, 6, 0, 3] = 30000                                               # one bin: a tie with a ring cell that comes first
    want = M.peaks(acc, mom, n, (H, W), bin, R)
    got = device_peaks(eng, acc, mom, n, (H, W), bin, R)
    check_against_model(got, want, "ties")
    ok = got["status"] == 0
    assert ok.sum() > 20 and got["status"][6, 6] == M.STATUS["range"]
    u, v = got["u"], got["v"]
    plain = ok.copy()
    plain[5, 5] = False
    assert np.all(np.rint(u[plain]) == 1 - R) and np.all(np.rint(v[plain]) == 2 - R)
    assert np.rint(u[5, 5]) == 5 - R and np.rint(v[5, 5]) == 1 - R
    assert got["ratio"][4, 4] == 1.0               # the second maximum lies outside the 5 x 5 of the first


# ---- end to end -----------------------------------------------------------------------------------------------------
def finished(want, scale, dt):
    """The model's dict as single_pixel delivers it: flipped rows, v's sign, scale / dt x 1000."""
    k = scale / dt * 1000
    out = {"u": np.flip(want["u"], axis=0) * k, "v": -np.flip(want["v"], axis=0) * k}
    for name in ("peak", "ratio", "status", "corr"):
        out[name] = np.flip(want[name], axis=0)
    return out


def test_host_classes(eng, tmp_path):
    from PIL import Image
    import torchpiv_amd.backend as T
    A, B = scene()
    n, (H, W) = len(A), A.shape[1:]
    acc, mom, want = scene_model()
    scale, dt = 0.5, 2
    k = scale / dt * 1000
    dA, dB = dev(A), dev(B)
    res = T.ResidentPIV(dA, dB, 32, 16, dt=dt, scale=scale)
    x, y, u, v, q = res.single_pixel(radius=M.SCENE_RADIUS, bin=M.SCENE_BIN, batch_size=12, planes=True)
    assert q.pairs == n and x.shape == u.shape == q.status.shape == (H, W // 128) and q.corr.shape == (H, 2, 11, 11)
    xs, ys = eng.pixel_corr_coordinates(H, W, M.SCENE_BIN)
    assert np.array_equal(x, np.meshgrid(xs, ys)[0] * scale) and np.array_equal(y, np.meshgrid(xs, ys)[1] * scale)
    assert xs.tolist() == [68.0, 196.0] and ys[:2].tolist() == [0.5, 1.5]      # get_coordinates' geometry, window = bin
    got = {"u": u / k, "v": v / k, "peak": q.peak, "ratio": q.ratio, "status": q.status, "corr": q.corr}
    fin = finished(want, 1.0, 1000.0)
    check_against_model(got, fin, "ResidentPIV.single_pixel")
    rows = M.interior_rows()
    rms, worst = M.profile_error(np.flip(u, axis=0)[rows, 1] / k, rows)
    print(f"  device, (1, 128) x {n} pairs against the profile: rms {rms:.4f} px, max {worst:.4f} px")
    assert rms <= CAP_RMS and worst <= CAP_MAX
    # files
    for i in range(n):
        Image.fromarray(A[i], "L").save(tmp_path / f"image{i:02d}_a.bmp")
        Image.fromarray(B[i], "L").save(tmp_path / f"image{i:02d}_b.bmp")
    off = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", 32, 16, dt=dt, scale=scale)
    o = off.single_pixel(radius=M.SCENE_RADIUS, bin=M.SCENE_BIN, batch_size=12, planes=True)
    for g, w in zip((x, y, u, v) + tuple(q), o[:4] + tuple(o[4])):
        assert np.asarray(g).tobytes() == np.asarray(w).tobytes()
    # indices and planes=False
    sub = res.single_pixel(radius=M.SCENE_RADIUS, bin=M.SCENE_BIN, indices=[0, 2, 5], batch_size=2)
    assert sub[4].pairs == 3 and sub[4].corr is None
    w3 = M.single_pixel(A[[0, 2, 5]], B[[0, 2, 5]], M.SCENE_BIN, M.SCENE_RADIUS)
    assert np.array_equal(sub[4].status, np.flip(w3["status"], axis=0))
    assert res.single_pixel(indices=[]) is None
    # min_ratio: valid bins below it become status 5 and NaN
    cut = float(np.median(want["ratio"][want["status"] == 0]))
    lo = res.single_pixel(radius=M.SCENE_RADIUS, bin=M.SCENE_BIN, min_ratio=cut)
    was_ok, low = fin["status"] == 0, got["ratio"] < cut
    assert (lo[4].status[was_ok & low] == 5).all() and (lo[4].status[was_ok & ~low] == 0).all() and (was_ok & low).any()
    assert np.isnan(lo[2][was_ok & low]).all() and np.array_equal(lo[4].status[~was_ok], fin["status"][~was_ok])
    # mask=: bins whose masked share exceeds the threshold get status 6 and the fill
    image = np.zeros((H, W), np.uint8)
    image[20:30, 128:228] = 1                      # 100 of 128 pixels of rows 20..29, second bin column: excluded at 0.5
    image[40:44, 128:168] = 1                      # 40 of 128: kept
    msk = T.ResidentPIV(dA, dB, 32, 16, dt=dt, scale=scale, mask={"image": image, "threshold": 0.5, "pixels": "keep",
                                                                   "fill": -7.0})
    mx = msk.single_pixel(radius=M.SCENE_RADIUS, bin=M.SCENE_BIN)
    st = np.flip(mx[4].status, axis=0)
    assert (st[20:30, 1] == 6).all() and (st[40:44, 1] == 0).all() and (st[20:30, 0] == 1).all() and (st == 6).sum() == 10
    assert (np.flip(mx[2], axis=0)[20:30, 1] == -7.0).all() and (np.flip(mx[3], axis=0)[20:30, 1] == -7.0).all()
    keep = st != 6
    assert np.array_equal(np.flip(mx[2], axis=0)[keep], np.flip(u, axis=0)[keep], equal_nan=True)     # "keep": frames untouched
    dyn = T.ResidentPIV(dA, dB, 32, 16, dynamic_mask={"kind": "bright", "size": 5, "level": 50})
    with pytest.raises(ValueError, match="dynamic_mask"):
        dyn.single_pixel()
    with pytest.raises(ValueError):
        res.single_pixel(radius=2)
    for obj in (res, off, msk, dyn):
        obj.close()


def test_memory_error_names_the_way_out(eng, monkeypatch):
    import torchpiv_amd.backend as T
    A, B = scene()
    res = T.ResidentPIV(dev(A[:2]), dev(B[:2]), 32, 16)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1 << 20, 1 << 30))
    with pytest.raises(MemoryError, match="larger bin or a smaller radius"):
        res.single_pixel(radius=16, bin=1)
    res.close()


# ---- refusals -------------------------------------------------------------------------------------------------------
def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def test_refusals_write_nothing(eng):
    """Every refusal of the header returns TPIV_EINVAL and leaves the accumulators, the outputs and the guards alone."""
    lib = eng.lib
    H, W, R, n = 12, 16, 3, 2
    D = 2 * R + 1
    arena = guarded.Arena(DEV, 0x5A, 0xA5, 1 << 24)
    rng = np.random.default_rng(8)
    a = arena.place(rng.integers(0, 256, (n, H, W)).astype(np.uint8), label="a")
    b = arena.place(rng.integers(0, 256, (n, H, W)).astype(np.uint8), label="b")
    acc = arena.empty((H, W, D, D), torch.int64, label="acc")
    mom = arena.empty((4, H, W), torch.int64, label="mom")
    outs = [arena.empty((H, W), torch.float64, label=k) for k in "uvpr"] + [arena.empty((H, W), torch.uint8, label="status"),
                                                                            arena.empty((H, W, D, D), torch.float64, label="corr")]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def add(batch=n, ky=1, kx=1, r=R, sy=0, sx=0, acc_p=None, mom_p=None, a_p=None):
        return lib.tpiv_pixel_corr_add(_p(a) if a_p is None else a_p, _p(b), batch, H, W, ky, kx, r, sy, sx,
                                       _p(acc) if acc_p is None else acc_p, _p(mom) if mom_p is None else mom_p, s)

    def peaks(n_pairs=n, ky=1, kx=1, r=R, sy=0, sx=0, acc_p=None, mom_p=None, u_p=None):
        return lib.tpiv_pixel_corr_peaks(_p(acc) if acc_p is None else acc_p, _p(mom) if mom_p is None else mom_p, n_pairs, H, W,
                                         ky, kx, r, sy, sx, _p(outs[0]) if u_p is None else u_p, _p(outs[1]), _p(outs[2]),
                                         _p(outs[3]), _p(outs[4]), _p(outs[5]), s)

    null = C.c_void_p(None)
    refused = [add(acc_p=null), add(mom_p=null), add(acc_p=_p(acc, 4)), add(mom_p=_p(mom, 4)), add(a_p=null), add(r=2),
               add(r=17), add(ky=0), add(kx=0), add(ky=-1), add(ky=2, kx=129), add(ky=H + 1), add(kx=W + 1), add(sy=65),
               add(sx=-65), add(batch=-1), add(batch=257),
               peaks(acc_p=null), peaks(mom_p=null), peaks(acc_p=_p(acc, 4)), peaks(mom_p=_p(mom, 4)), peaks(u_p=null),
               peaks(n_pairs=0), peaks(n_pairs=65537), peaks(r=2), peaks(r=17), peaks(ky=0), peaks(ky=2, kx=129), peaks(sy=-65),
               peaks(sx=65)]
    torch.cuda.synchronize()
    assert refused == [EINVAL] * len(refused), refused
    assert all(arena.holds_poison(t) for t in [acc, mom] + outs)
    arena.check()
    assert add(batch=0) == 0                       # succeeds and launches nothing
    torch.cuda.synchronize()
    assert arena.holds_poison(acc) and arena.holds_poison(mom)
    assert lib.tpiv_pixel_corr_bytes(H, W, 1, 1, R) == acc.numel() * 8
    with pytest.raises(ValueError):
        eng.pixel_corr_add(a, b, 1, R, acc=acc[:, :, :, :-1].contiguous())
    with pytest.raises(ValueError):
        eng.pixel_corr_peaks(torch.zeros_like(acc), torch.zeros_like(mom), 0, (H, W), 1, R)


# ---- memory contract ------------------------------------------------------------------------------------------------
CONTRACT = []


def _contract_entries():
    A, B = random_pairs()

    def b_add(n, with_acc, bin, radius):
        def build():
            d = {"frame_a": A[:n], "frame_b": B[:n]}
            if with_acc:
                r = np.random.default_rng(77)
                D = 2 * radius + 1
                d["acc"] = r.integers(0, 1 << 40, (H0 // bin[0], W0 // bin[1], D, D)).astype(np.int64)
                d["mom"] = r.integers(0, 1 << 30, (4, H0, W0)).astype(np.int64)
            return d
        return build

    def b_peaks(bin, radius, shift):
        def build():
            acc, mom = M.accumulate(A[:5], B[:5], bin, radius, shift)
            return {"acc": acc, "mom": mom}
        return build

    for bin, radius, shift in (((1, 1), 3, (0, 0)), ((2, 3), 8, (2, -3)), ((16, 16), 16, (-5, 4)), ((1, 45), 4, (0, 0))):
        tag = f"{bin[0]}x{bin[1]} R{radius}"
        for n, with_acc in ((5, False), (9, True)):
            label = f"pixel_corr_add {tag} {'into' if with_acc else 'fresh'}"
            MC.entry(label, b_add(n, with_acc, bin, radius),
                     lambda eng, i, mem, bin=bin, radius=radius, shift=shift: eng.pixel_corr_add(
                         i["frame_a"], i["frame_b"], bin, radius, shift, acc=i.get("acc"), mom=i.get("mom")),
                     family="pixel_corr")
            CONTRACT.append(label)
        for planes in (False, True):
            label = f"pixel_corr_peaks {tag} planes={planes}"
            MC.entry(label, b_peaks(bin, radius, shift),
                     lambda eng, i, mem, bin=bin, radius=radius, shift=shift, planes=planes: tuple(
                         t for t in eng.pixel_corr_peaks(i["acc"], i["mom"], 5, (H0, W0), bin, radius, shift, planes=planes)
                         if t is not None),
                     family="pixel_corr")
            CONTRACT.append(label)
    label = "pixel_corr_bytes"
    MC.entry(label, lambda: {"frame_a": A[:1]},
             lambda eng, i, mem: torch.tensor([eng.pixel_corr_bytes(H0, W0, b_, r_) for b_ in BINS for r_ in RADII] +
                                              [eng.pixel_corr_bytes(H0, W0, 1, 2), eng.pixel_corr_bytes(H0, W0, (17, 16), 3)]),
             family="pixel_corr")
    CONTRACT.append(label)


_contract_entries()
_BY_LABEL = {e.label: e for e in MC.ENTRIES}


@pytest.mark.parametrize("label", CONTRACT)
def test_memory_contract(eng, label):
    """Bounds, stale data and alignment for one table entry: every buffer the engine allocates comes from the guarded arena,
    the frames start at an odd address, the guard bands stay intact and the outputs are the unguarded call's bits under all
    three (poison, guard) settings."""
    e = _BY_LABEL[label]
    want = MC.run_plain(eng, e)
    runs = []
    for setting in guarded.SETTINGS:
        run, arena, out = MC.run_entry(eng, e, setting, offset=1)
        runs.append(run)
        assert len(run) == len(want)
        for k, (x, y) in enumerate(zip(run, want)):
            i = guarded.first_difference(x, y)
            assert i is None, f"{label}: output {k} differs from the unguarded call's at byte {i} under setting {setting}"
        del arena, out
    guarded.differing_output(runs, [f"{label}: output {k}" for k in range(len(want))])
    assert {"tpiv_pixel_corr_add", "tpiv_pixel_corr_peaks", "tpiv_pixel_corr_bytes"} & MC.CALLS
