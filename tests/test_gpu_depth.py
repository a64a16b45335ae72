"""Deep (16-bit) frames on the device (depth.hip) and through every host path: the tone-map and histogram kernels against
the numpy model (tests/depth_model.py) bit for bit, and depth= end to end -- uint16 frames whose map is exactly v / 16
give the fields of the uint8 run, bit for bit, while the 8-bit decode of the same files (value >> 8) does not."""
import numpy as np
import pytest
import torch

import depth_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def _dev(a):
    """numpy uint16 -> torch.uint16 on the device."""
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy()


def _shifted(t, nbytes):
    """A copy of the uint16 tensor t whose data starts `nbytes` (even) past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=torch.uint16, device=t.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[nbytes // 2:nbytes // 2 + t.numel()].view(t.shape)
    out.view(torch.int16).copy_(t.view(torch.int16))           # (copies through the signed view: no uint16 arithmetic needed)
    assert out.data_ptr() % 16 == nbytes
    return out


# (n, H, W): smaller than one 8-sample group (5 x 7 = 35 = 4 groups + 3); odd sizes and n; 24 x 48 a multiple of 8 with every
# frame 16-byte aligned; 256 x 256 one lane per group over several workgroups; 70 x 151: odd W, so frame 1 of the stack
# starts 2 bytes off any 4-byte boundary (its source takes the sample path while frame 0 takes the 16-byte path)
SHAPES = [(1, 5, 7), (3, 37, 50), (2, 24, 48), (1, 256, 256), (2, 70, 151)]


def _data(n, H, W):
    rng = np.random.default_rng(n * 1000 + H * 7 + W)
    dark = rng.integers(0, 200, (n, H, W))
    bright = rng.random((n, H, W)) >= 0.95
    dark[bright] = rng.integers(200, 4096, int(bright.sum()))
    out = {"random": rng.integers(0, 65536, (n, H, W)), "zeros": np.zeros((n, H, W)), "full": np.full((n, H, W), 65535),
           "dark12": dark}
    if (n, H, W) == (1, 256, 256):
        out["ramp"] = rng.permutation(65536).reshape(1, 256, 256)       # every value once: every table entry is read
        out["ramp_sorted"] = np.arange(65536).reshape(1, 256, 256)
    return {k: v.astype(np.uint16) for k, v in out.items()}


def _tables():
    rng = np.random.default_rng(99)
    return {"high_byte": (np.arange(65536) >> 8).astype(np.uint8),
            "linear_4095": M.lut(0, 4095, "linear"), "sqrt_4095": M.lut(0, 4095, "sqrt"),
            "linear_37_38": M.lut(37, 38, "linear"), "sqrt_37_38": M.lut(37, 38, "sqrt"),
            "random": rng.integers(0, 256, 65536).astype(np.uint8)}


TABLES = _tables()


@pytest.mark.parametrize("n,H,W", SHAPES)
def test_map_kernel_equals_model(eng, n, H, W):
    luts = {k: torch.from_numpy(v).cuda() for k, v in TABLES.items()}
    SENT = 0xA5
    for name, F_h in _data(n, H, W).items():
        F = _dev(F_h)
        Fs = _shifted(F, 2)
        keep, keep_s = F.view(torch.int16).clone(), Fs.view(torch.int16).clone()
        # the offsets form: the frames scattered in one flat buffer with odd gaps, in the order b0 a0 b1 a1 ..., read back
        # as the stacks a.., b.. (frame k of F plays a_k for even k ... the order below is what matters)
        gaps = [3 + 2 * k for k in range(n)]
        flat = torch.full((sum(gaps) + n * H * W + 5,), 0x1234, dtype=torch.int16, device="cuda").view(torch.uint16)
        offs, pos = [], 0
        for k in range(n):
            pos += gaps[k]
            offs.append(pos)
            flat.view(torch.int16)[pos:pos + H * W].copy_(F[k].reshape(-1).view(torch.int16))
            pos += H * W
        keep_flat = flat.view(torch.int16).clone()
        for tname, tab in TABLES.items():
            lut = luts[tname]
            want = M.map_(F_h, tab)
            tag = (name, tname)
            got = eng.depth_map(F, lut)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (n, H, W)
            assert np.array_equal(_host(got), want), tag
            assert np.array_equal(_host(eng.depth_map(Fs, lut)), want), tag                   # source 2 bytes off 16
            # a given out 1 byte past an 8-byte boundary inside a sentinel buffer: nothing outside [n, H, W] is written
            big = torch.full((n * H * W + 64,), SENT, dtype=torch.uint8, device="cuda")
            lead = 8 + (1 - big.data_ptr()) % 8
            out = big[lead:lead + n * H * W].view(n, H, W)
            assert out.data_ptr() % 8 == 1
            assert eng.depth_map(F, lut, out=out) is out
            big_h = _host(big)
            assert np.array_equal(big_h[lead:lead + n * H * W].reshape(n, H, W), want), tag
            assert (big_h[:lead] == SENT).all() and (big_h[lead + n * H * W:] == SENT).all(), tag
            assert np.array_equal(_host(eng.depth_map(F[n - 1], lut)), want[n - 1]), tag      # a single 2-D frame
            # offsets: as scattered, and in another order (b0 a0 b1 a1 -> a0 a1 b0 b1 is order[1::2] + order[0::2])
            got = eng.depth_map(flat, lut, offsets=torch.tensor(offs, dtype=torch.int64), shape=(H, W))
            assert np.array_equal(_host(got), want), tag
            order = list(range(1, n, 2)) + list(range(0, n, 2))
            got = eng.depth_map(flat, lut, offsets=np.array([offs[k] for k in order], dtype=np.int64), shape=(H, W))
            assert np.array_equal(_host(got), want[order]), tag
            got = eng.depth_map(flat, lut, offsets=torch.tensor(offs, dtype=torch.int64, device="cuda"), shape=(H, W))
            assert np.array_equal(_host(got), want), tag
        torch.cuda.synchronize()
        assert torch.equal(F.view(torch.int16), keep) and torch.equal(Fs.view(torch.int16), keep_s)      # never written
        assert torch.equal(flat.view(torch.int16), keep_flat)


def test_map_interleaved_slots_to_stacks(eng):
    """The staged layout of batched(): slots b0 a0 b1 a1 of `cap` samples each (frames at the start of a slot), one launch
    -> a0 a1 b0 b1."""
    H, W, cap = 24, 50, 24 * 50 + 848
    rng = np.random.default_rng(5)
    fr = rng.integers(0, 4096, (4, H, W)).astype(np.uint16)                # b0 a0 b1 a1
    slots = np.full((4, cap), 0xFFFF, np.uint16)
    slots[:, :H * W] = fr.reshape(4, -1)
    tab = M.lut(0, 4095)
    got = eng.depth_map(_dev(slots).view(-1), torch.from_numpy(tab).cuda(), offsets=np.array([1, 3, 0, 2], np.int64) * cap,
                        shape=(H, W))
    assert np.array_equal(_host(got), M.map_(fr[[1, 3, 0, 2]], tab))


@pytest.mark.parametrize("n,H,W", SHAPES)
def test_histogram_kernel_equals_bincount(eng, n, H, W):
    for name, F_h in _data(n, H, W).items():
        F = _dev(F_h)
        keep = F.view(torch.int16).clone()
        want = M.hist(F_h)
        got = eng.depth_histogram(F)
        assert got.dtype == torch.int64 and tuple(got.shape) == (65536,)
        assert np.array_equal(_host(got), want), name
        assert np.array_equal(_host(eng.depth_histogram(_shifted(F, 2))), want), name       # a head before the 16-byte groups
        assert np.array_equal(_host(eng.depth_histogram(_shifted(F, 14))), want), name
        assert np.array_equal(_host(eng.depth_histogram(F[n - 1])), M.hist(F_h[n - 1])), name
        torch.cuda.synchronize()
        assert torch.equal(F.view(torch.int16), keep)


def test_histogram_under_maximal_contention(eng):
    """(2, 300, 301): 90 300 samples per frame, 180 600 in all -- several chunks of the kernel's 65 528, each past nothing a
    16-bit private counter holds only because the chunk is capped; every sample on one bin, then on two alternating bins."""
    n, H, W = 2, 300, 301
    const = np.full((n, H, W), 1234, np.uint16)
    got = _host(eng.depth_histogram(_dev(const)))
    assert got[1234] == n * H * W == 180600 and got.sum() == n * H * W
    two = np.where(np.arange(n * H * W).reshape(n, H, W) % 2 == 0, 4094, 4095).astype(np.uint16)     # the halves of ONE dword
    assert np.array_equal(_host(eng.depth_histogram(_dev(two))), M.hist(two))
    far = np.where(np.arange(n * H * W).reshape(n, H, W) % 2 == 0, 0, 65535).astype(np.uint16)
    assert np.array_equal(_host(eng.depth_histogram(_dev(far))), M.hist(far))


def test_histogram_accumulates(eng):
    rng = np.random.default_rng(8)
    A = rng.integers(0, 4096, (3, 37, 50)).astype(np.uint16)
    B = rng.integers(0, 65536, (2, 37, 50)).astype(np.uint16)
    acc = eng.depth_histogram(_dev(A))
    assert eng.depth_histogram(_dev(B), acc) is acc
    assert np.array_equal(_host(acc), M.hist(np.concatenate([A, B])))
    # a starting accumulator near 2^32 keeps its high word: 64-bit adds
    start = np.zeros(65536, np.int64)
    start[7] = 2 ** 32 - 5
    start[4000] = 3 * 2 ** 32 + 11
    C = np.full((1, 10, 10), 7, np.uint16)
    C[0, 0, :3] = 4000
    got = _host(eng.depth_histogram(_dev(C), torch.from_numpy(start).cuda()))
    assert got[7] == 2 ** 32 - 5 + 97 and got[4000] == 3 * 2 ** 32 + 14 and got.sum() == start.sum() + 100


def test_argument_errors_launch_nothing(eng):
    F = _dev(np.arange(4 * 16 * 16, dtype=np.uint16).reshape(4, 16, 16))
    lut = torch.from_numpy(M.lut(0, 1023)).cuda()
    out = torch.full((4, 16, 16), 0x5A, dtype=torch.uint8, device="cuda")
    acc = torch.full((65536,), 77, dtype=torch.int64, device="cuda")
    bad_map = [
        dict(frames=F.view(torch.int16)), dict(frames=F.view(torch.uint8)),                          # dtype
        dict(frames=F[:, :, ::2]), dict(frames=F[:, ::2]),                                           # not contiguous
        dict(lut=lut.cpu()), dict(lut=lut[:65535]), dict(lut=lut.view(torch.int8)), dict(lut=lut.repeat(2)[::2]),
        dict(out=out[:3]), dict(out=out.view(torch.int8)), dict(out=out.cpu()),
        dict(offsets=torch.tensor([0], dtype=torch.int64)),                                          # offsets need a flat buffer
        dict(shape=(16, 16)),
        dict(frames=F.view(-1), offsets=torch.tensor([0, 3 * 256 + 1], dtype=torch.int64), shape=(16, 16), out=out[:2]),   # leaves the buffer
        dict(frames=F.view(-1), offsets=torch.tensor([-1], dtype=torch.int64), shape=(16, 16), out=out[:1]),
        dict(frames=F.view(-1), offsets=torch.tensor([0], dtype=torch.int32), shape=(16, 16), out=out[:1]),
        dict(frames=F.view(-1), offsets=torch.tensor([0], dtype=torch.int64), out=out[:1]),          # no shape
    ]
    for kw in bad_map:
        args = dict(frames=F, lut=lut, out=out)
        args.update(kw)
        with pytest.raises(ValueError):
            eng.depth_map(**args)
    # an out that overlaps the source or the table is refused
    raw = torch.zeros(4 * 256 * 2 + 1024 + 64, dtype=torch.uint8, device="cuda")
    src = raw[:4 * 256 * 2].view(torch.uint16).view(4, 16, 16)
    for o in (raw[:1024].view(4, 16, 16), raw[2047:2047 + 1024].view(4, 16, 16), raw[1000:2024].view(4, 16, 16)):
        with pytest.raises(ValueError, match="overlaps"):
            eng.depth_map(src, lut, out=o)
    two = torch.zeros(65536 + 1024, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="overlaps"):
        eng.depth_map(F, two[:65536], out=two[65535:65535 + 1024].view(4, 16, 16))
    for kw in (dict(frames=F.view(torch.int16)), dict(frames=F[:, :, ::2]), dict(acc=acc[:100]), dict(acc=acc.cpu()),
               dict(acc=acc.to(torch.int32)), dict(acc=torch.zeros(2 * 65536, dtype=torch.int64, device="cuda")[::2])):
        args = dict(frames=F, acc=acc)
        args.update(kw)
        with pytest.raises(ValueError):
            eng.depth_histogram(**args)
    torch.cuda.synchronize()
    assert (out == 0x5A).all() and (acc == 77).all() and (raw == 0).all()
    # n == 0 is a successful no-op
    assert tuple(eng.depth_map(F[:0], lut).shape) == (0, 16, 16)
    assert int(eng.depth_histogram(F[:0]).sum()) == 0


# --------------------------------------------------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------------------------------------------------
H0, W0, N0 = 160, 192, 4              # 64/32 needs four windows per axis for the spline predictor: (160 - 64) / 32 + 1 = 4
R16 = {"lo": 0, "hi": 4080}                     # v = 16 * g  ->  (g * 16 * 510 + 4080) // 8160 = g: exactly v / 16
CHAINS = [("CWS", 32, 16, 2), ("DWS", 64, 32, 2)]


@pytest.fixture(scope="module")
def frames():
    """Four wavy pairs as uint8 (F8), with at least one 0 and one 255 sample, and the same as 12-bit samples F16 = 16 * F8
    (minimum 0, maximum 4080)."""
    from torchpiv_amd import synth
    A, B = synth.make_batch(N0, H0, W0, kind="wavy", noise=1.5)
    A, B = A.clone(), B.clone()
    A[0, 0, 0], A[0, 0, 1] = 0, 255
    # a patch of noise in every frame b (sizes and places differ from pair to pair): its windows fail the peak-ratio test, so
    # every chain has holes to fill -- a pair without a single invalid vector is dropped, like in the reference
    g = torch.Generator().manual_seed(17)
    for i, (y0, x0, sz) in enumerate([(60, 70, 32), (30, 120, 24), (90, 40, 40), (100, 130, 16)]):
        B[i, y0:y0 + sz, x0:x0 + sz] = torch.randint(0, 256, (sz, sz), generator=g, dtype=torch.uint8)
    to16 = lambda F: torch.from_numpy((F.numpy().astype(np.int32) * 16).astype(np.uint16))      # noqa: E731
    return A, B, to16(A), to16(B)


def _fields(gen):
    out = {}
    for i, x, y, u, v in gen:
        out[i] = (np.asarray(u), np.asarray(v))
    return out


def _same(f1, f2):
    assert sorted(f1) == sorted(f2)
    for i in f1:
        assert np.array_equal(f1[i][0], f2[i][0], equal_nan=True) and np.array_equal(f1[i][1], f2[i][1], equal_nan=True), i


def _resident8(A, B, ws, ov, **kw):
    import torchpiv_amd as T
    piv = T.ResidentPIV(A.cuda(), B.cuda(), ws, ov, **kw)
    out = _fields(piv.batched(4))
    piv.close()
    return out


@pytest.mark.parametrize("mode,ws,ov,mp_", CHAINS)
@pytest.mark.parametrize("extra", [{}, {"background": "min"}, {"prefilter": {"kind": "min", "size": 15}}, {"outlier": "median"},
                                   {"background": "min", "prefilter": {"kind": "mean", "size": 7, "cap": 120}}],
                         ids=["plain", "background", "prefilter", "outlier", "background+prefilter"])
def test_resident_depth_equals_uint8_run(frames, mode, ws, ov, mp_, extra):
    import torchpiv_amd as T
    A, B, A16, B16 = frames
    kw = dict(multipass=mp_, multipass_mode=mode, **extra)
    want = _resident8(A, B, ws, ov, **kw)
    assert len(want) > 0
    Ad, Bd = A16.cuda(), B16.cuda()
    keep = Ad.view(torch.int16).clone(), Bd.view(torch.int16).clone()
    piv = T.ResidentPIV(Ad, Bd, ws, ov, depth=R16, **kw)
    assert piv.depth_range_ == (0, 4080)
    _same(_fields(piv.batched(4)), want)
    assert tuple(piv._depth_frames.shape) == (2, 4, H0, W0)                 # one reused buffer, not a copy of the recording
    sub = [3, 0, 2]                                                         # pairs out of order, a short last chunk
    _same(_fields(piv.batched(2, indices=sub)), {i: want[i] for i in sub if i in want})
    assert tuple(piv._depth_frames.shape) == (2, 4, H0, W0)
    res = list(piv())                                                       # __call__: one pair per launch
    assert len(res) == len(want)
    for i, (x, y, u, v) in zip(sorted(want), res):
        assert np.array_equal(u, want[i][0], equal_nan=True) and np.array_equal(v, want[i][1], equal_nan=True), i
    piv.close()
    torch.cuda.synchronize()
    assert torch.equal(Ad.view(torch.int16), keep[0]) and torch.equal(Bd.view(torch.int16), keep[1])


def test_resident_auto_range(frames):
    import torchpiv_amd as T
    from torchpiv_amd import engine
    A, B, A16, B16 = frames
    want = _resident8(A, B, 32, 16, multipass=2)
    piv = T.ResidentPIV(A16.cuda(), B16.cuda(), 32, 16, multipass=2, depth={"auto": True, "clip_low": 0, "clip_high": 0})
    assert piv.depth_range_ is None                                         # lazily, on first use
    _same(_fields(piv.batched(4)), want)
    assert piv.depth_range_ == (0, 4080)
    piv.close()
    # "min" background over mapped frames: the range prepass runs before the background prepass
    piv = T.ResidentPIV(A16.cuda(), B16.cuda(), 32, 16, multipass=2, background="min",
                        depth={"auto": True, "clip_low": 0, "clip_high": 0})
    _same(_fields(piv.batched(3)), _resident8(A, B, 32, 16, multipass=2, background="min"))
    assert piv.depth_range_ == (0, 4080)
    piv.close()
    # the default clips, and a sample smaller than the recording: the model's range of the model's histogram of those pairs
    for depth, pairs in (("auto", [0, 1, 2, 3]), ({"auto": True, "sample": 2, "clip_high": 0.01, "clip_low": 0.2}, [0, 3]),
                         ({"auto": True, "sample": 1}, [0])):
        par = engine.depth_arg(depth)
        piv = T.ResidentPIV(A16.cuda(), B16.cuda(), 32, 16, multipass=2, depth=depth)
        _fields(piv.batched(4))
        hist = M.hist(np.stack([A16.numpy()[pairs], B16.numpy()[pairs]]))
        assert piv.depth_range_ == M.range_(hist, par["clip_low"], par["clip_high"]), depth
        assert np.array_equal(piv._depth_lut.cpu().numpy(), M.lut(*piv.depth_range_)), depth
        piv.close()


def test_resident_dtype_rules(frames):
    import torchpiv_amd as T
    A, B, A16, B16 = frames
    with pytest.raises(ValueError, match="depth="):
        T.ResidentPIV(A16.cuda(), B16.cuda(), 32, 16)
    with pytest.raises(ValueError, match="uint16"):
        T.ResidentPIV(A.cuda(), B.cuda(), 32, 16, depth=R16)
    with pytest.raises(ValueError):
        T.ResidentPIV(A16.cuda(), B.cuda(), 32, 16, depth=R16)
    with pytest.raises(ValueError, match="depth"):
        T.ResidentPIV(A16.cuda(), B16.cuda(), 32, 16, depth={"lo": 5})
    lut_piv = T.ResidentPIV(A16.cuda(), B16.cuda(), 32, 16, depth={"lut": M.lut(0, 4080)})
    assert lut_piv.depth_range_ is None
    lut_piv.close()


def test_custom_table_reproduces_the_high_byte_rule(frames):
    """{"lut": v >> 8} on F16 is the reference's 16-bit rule through the new path: the uint8 run on F8 >> 4."""
    import torchpiv_amd as T
    A, B, A16, B16 = frames
    want = _resident8(A >> 4, B >> 4, 32, 16, multipass=2)
    piv = T.ResidentPIV(A16.cuda(), B16.cuda(), 32, 16, multipass=2, depth={"lut": (np.arange(65536) >> 8).astype(np.uint8)})
    _same(_fields(piv.batched(4)), want)
    assert piv.depth_range_ is None
    piv.close()


def _write_png16(path, A16, B16, broken=None):
    from PIL import Image
    for i in range(A16.shape[0]):
        Image.fromarray(A16[i].numpy()).save(path / f"image{i}_a.png")
        Image.fromarray(B16[i].numpy()).save(path / f"image{i}_b.png")
    if broken is not None:
        (path / f"image{broken}_b.png").write_bytes(b"not a png")


@pytest.mark.parametrize("mode,ws,ov,mp_", CHAINS)
def test_offline_depth_equals_resident(tmp_path, frames, mode, ws, ov, mp_):
    """16-bit PNGs through __call__ (batched and one pair at a time) and through batched(3) (a ragged last batch), alone
    and with background + pre-filter, against the uint8 resident run."""
    import torchpiv_amd as T
    A, B, A16, B16 = frames
    _write_png16(tmp_path, A16, B16)
    for extra in ({}, {"background": "min"}, {"background": "min", "prefilter": {"kind": "min", "size": 15}},
                  {"prefilter": {"kind": "mean", "size": 7, "cap": 120}}):
        kw = dict(multipass=mp_, multipass_mode=mode, **extra)
        want = _resident8(A, B, ws, ov, **kw)
        assert len(want) > 0
        piv = T.OfflinePIV(str(tmp_path), "cuda:0", "png", ws, ov, depth=R16, **kw)
        assert piv.depth_range_ == (0, 4080)
        _same(_fields(piv.batched(3)), want)
        assert tuple(piv._depth_frames.shape) == (6, H0, W0)
        _same(_fields(piv.batched(2, indices=[3, 0, 2])), {i: want[i] for i in (3, 0, 2) if i in want})
        piv.close()
        for call_batch in (32, 1):
            p2 = T.OfflinePIV(str(tmp_path), "cuda:0", "png", ws, ov, depth=R16, **kw)
            p2.call_batch = call_batch
            res = list(p2())
            assert len(res) == len(want)
            for i, (x, y, u, v) in zip(sorted(want), res):
                assert np.array_equal(u, want[i][0], equal_nan=True) and np.array_equal(v, want[i][1], equal_nan=True), i
            p2.close()


def test_offline_auto_and_broken_file_and_runner(tmp_path, frames):
    import torchpiv_amd as T
    from torchpiv_amd import runner
    A, B, A16, B16 = frames
    _write_png16(tmp_path, A16, B16, broken=1)
    want = _resident8(A, B, 32, 16, multipass=2)
    want.pop(1, None)
    assert len(want) > 0
    piv = T.OfflinePIV(str(tmp_path), "cuda:0", "png", 32, 16, multipass=2, depth=R16)
    got = _fields(piv.batched(3))
    _same(got, want)                                                        # exactly the broken pair is skipped
    piv.close()
    # "auto": the broken pair is left out of the sample too
    piv = T.OfflinePIV(str(tmp_path), "cuda:0", "png", 32, 16, multipass=2, depth={"auto": True, "clip_high": 0})
    _same(_fields(piv.batched(3)), want)
    assert piv.depth_range_ == (0, 4080)
    piv.close()
    piv = T.OfflinePIV(str(tmp_path), "cuda:0", "png", 32, 16, multipass=2, depth="auto")
    piv.call_batch = 1
    assert len(list(piv())) == len(want)
    ok = [0, 2, 3]
    assert piv.depth_range_ == M.range_(M.hist(np.stack([A16.numpy()[ok], B16.numpy()[ok]])), 0.0, 1e-4)
    piv.close()
    seen = {}
    runner.run_folder(str(tmp_path), "cuda:0", "png", 32, 16, multipass=2, depth=R16, batch_size=3,
                      on_pair=lambda i, out: seen.__setitem__(i, (out["Vx[m/s]"], out["Vy[m/s]"])))
    _same(seen, want)


def test_without_depth_the_files_lose_their_low_bits(tmp_path, frames):
    """The gap depth= closes: with depth=None the 16-bit files are decoded as value >> 8, i.e. the run sees F8 >> 4 (16
    grey levels) and does not reproduce the uint8 fields.  Measured on the device (profiles/depth/README.md): all 4 pairs
    kept, RMS difference to the full-depth fields 280 field units (0.28 px), largest 5975 (6.0 px).  Only the inequality is
    asserted."""
    import torchpiv_amd as T
    A, B, A16, B16 = frames
    _write_png16(tmp_path, A16, B16)
    full = _resident8(A, B, 32, 16, multipass=2)
    piv = T.OfflinePIV(str(tmp_path), "cuda:0", "png", 32, 16, multipass=2)
    got = _fields(piv.batched(4))
    piv.close()
    _same(got, _resident8(A >> 4, B >> 4, 32, 16, multipass=2))             # exactly the >> 8 rule, as before
    both = sorted(set(got) & set(full))
    differs = sorted(got) != sorted(full) or any(
        not (np.array_equal(got[i][0], full[i][0], equal_nan=True) and np.array_equal(got[i][1], full[i][1], equal_nan=True))
        for i in both)
    if both:
        d = np.concatenate([np.hypot(got[i][0] - full[i][0], got[i][1] - full[i][1]).ravel() for i in both])
        print(f"depth=None on 12-bit files: pairs kept {len(got)} of {len(full)}, RMS difference to the full-depth fields "
              f"{np.sqrt(np.nanmean(d ** 2)):.4f}, largest {np.nanmax(d):.4f} (field units)")
    assert differs
