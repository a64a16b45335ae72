"""Static background removal on the device (background.hip, the fused unpack of ingest.hip) and through every host path:
kernels against torch / numpy bit for bit, background="min" / given backgrounds against running on frames that were
subtracted beforehand (bit-identical fields), and the effect on a scene with a static textured band."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def _sub(f, bg):
    """max(f, bg) - bg in torch (int32, clamped)."""
    return (f.int() - bg.int()).clamp(min=0).to(torch.uint8)


def _misaligned(t):
    """A copy of t whose data starts one byte past a 16-byte boundary (the kernels' byte path)."""
    buf = torch.empty(t.numel() + 1, dtype=torch.uint8, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    return out


# (n, H, W): widths not multiples of 4 or 16 and odd H (byte path and tails), pixels % 16 == 0 (16-byte path), n = 1
# and n > 1, odd n (the subtraction's two-frames step)
SHAPES = [(1, 37, 50), (5, 33, 61), (4, 17, 13), (1, 64, 64), (9, 256, 320), (2, 40, 48)]


@pytest.mark.parametrize("n,H,W", SHAPES)
def test_frame_min_and_subtract_against_torch(eng, n, H, W):
    g = torch.Generator().manual_seed(n * 1000 + H * 7 + W)
    F = torch.randint(0, 256, (n, H, W), generator=g, dtype=torch.uint8).cuda()
    want_min = F.amin(0)
    assert torch.equal(eng.frame_min(F), want_min)
    # into a given accumulator, which already holds a minimum: min of both
    acc0 = torch.randint(0, 256, (H, W), generator=g, dtype=torch.uint8).cuda()
    acc = acc0.clone()
    assert eng.frame_min(F, acc) is acc
    assert torch.equal(acc, torch.minimum(acc0, want_min))
    # two accumulating calls == one call over all the frames
    G = torch.randint(0, 256, (n + 2, H, W), generator=g, dtype=torch.uint8).cuda()
    assert torch.equal(eng.frame_min(G, eng.frame_min(F)), torch.cat([F, G]).amin(0))
    # a 2-D frame is one frame
    assert torch.equal(eng.frame_min(F[0]), F[0])
    # the byte path on misaligned frames
    assert torch.equal(eng.frame_min(_misaligned(F)), want_min)
    bg = torch.randint(0, 256, (H, W), generator=g, dtype=torch.uint8).cuda()
    want = _sub(F, bg)
    assert torch.equal(eng.subtract_background(F, bg), want)
    assert torch.equal(eng.subtract_background(F[0], bg), want[0])
    assert torch.equal(eng.subtract_background(_misaligned(F), bg), want)
    assert torch.equal(eng.subtract_background(F, _misaligned(bg)), want)
    out = torch.full_like(F, 7)
    assert eng.subtract_background(F, bg, out=out) is out and torch.equal(out, want)
    # in place (out is frames), aligned and misaligned
    F2 = F.clone()
    eng.subtract_background(F2, bg, out=F2)
    assert torch.equal(F2, want)
    F3 = _misaligned(F)
    eng.subtract_background(F3, bg, out=F3)
    assert torch.equal(F3, want)
    # the background of a recording removes itself: min of F subtracted from F leaves a 0 in every pixel's stack
    assert int(eng.subtract_background(F, want_min).amin(0).max()) == 0
    torch.cuda.synchronize()


def test_subtract_background_refuses_a_partial_overlap(eng):
    F = torch.zeros(4, 16, 16, dtype=torch.uint8, device="cuda")
    bg = torch.zeros(16, 16, dtype=torch.uint8, device="cuda")
    buf = torch.zeros(5 * 256, dtype=torch.uint8, device="cuda")
    from torchpiv_amd._lib import check, lib
    with pytest.raises(ValueError):
        check(lib.tpiv_subtract_background(buf.data_ptr(), 4, 256, bg.data_ptr(), buf.data_ptr() + 256, 0))
    with pytest.raises(ValueError):
        eng.subtract_background(F, bg[:8])
    with pytest.raises(ValueError):
        eng.frame_min(F, torch.zeros(16, 15, dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("H,W", [(37, 50), (24, 48)])
def test_bmp_unpack_bg_equals_unpack_then_subtract(eng, tmp_path, H, W):
    """tpiv_bmp_unpack_bg == tpiv_bmp_unpack followed by a numpy subtraction, byte for byte: 8-bit grey-ramp and
    arbitrary palettes, 24- and 32-bit colour, bottom-up and top-down rows, padded rows (W = 50) and whole 4-pixel groups
    (W = 48), a host-decoded PNG staged as headerless pixels; desc[f][5] picks bg_a or bg_b."""
    import struct
    from PIL import Image
    from torchpiv_amd import io as pio
    rng = np.random.default_rng(H * W)
    files = []
    gray = rng.integers(0, 256, size=(H, W)).astype(np.uint8)
    Image.fromarray(gray, "L").save(tmp_path / "g8.bmp")
    files.append("g8.bmp")
    Image.fromarray(rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8), "RGB").save(tmp_path / "c24.bmp")
    files.append("c24.bmp")
    pal = Image.fromarray(gray, "L").convert("P", palette=Image.ADAPTIVE, colors=200)
    pal.putpalette(list(rng.integers(0, 256, size=768).astype(np.uint8)))
    pal.save(tmp_path / "p8.bmp")
    files.append("p8.bmp")
    bgra = rng.integers(0, 256, size=(H, W, 4)).astype(np.uint8)
    hdr = b"BM" + struct.pack("<IHHI", 54 + H * W * 4, 0, 0, 54) + struct.pack("<IiiHHIIiiII", 40, W, -H, 1, 32, 0, H * W * 4,
                                                                                2835, 2835, 0, 0)
    (tmp_path / "t32.bmp").write_bytes(hdr + bgra.tobytes())              # top-down 32 bit
    files.append("t32.bmp")
    Image.fromarray(rng.integers(0, 256, size=(H, W)).astype(np.uint8), "L").save(tmp_path / "g.png")
    files.append("g.png")
    cap = max((tmp_path / f).stat().st_size for f in files)
    cap = max(cap, H * W)
    stage = torch.zeros(2 * len(files), cap, dtype=torch.uint8).pin_memory()
    desc, luts = [], []
    for k in range(2 * len(files)):                   # every file twice: once against bg_a, once against bg_b
        f = files[k % len(files)]
        lay = pio.stage_raw(str(tmp_path / f), stage[k].numpy(), H, W)
        assert lay is not None, f
        desc.append([k * cap, lay[0], lay[1], lay[2], lay[3], k // len(files)])
        luts.append(lay[4])
    raw = stage.cuda().view(-1)
    desc_d = torch.tensor(desc, dtype=torch.int64).cuda()
    lut_d = torch.from_numpy(np.stack(luts)).cuda()
    bg2 = torch.from_numpy(rng.integers(0, 256, size=(2, H, W)).astype(np.uint8)).cuda()
    plain = eng.bmp_unpack(raw, desc_d, lut_d, H, W).cpu().numpy()
    fused = eng.bmp_unpack(raw, desc_d, lut_d, H, W, background=bg2).cpu().numpy()
    bg = bg2.cpu().numpy().astype(np.int32)
    for k in range(2 * len(files)):
        want = np.maximum(plain[k].astype(np.int32) - bg[k // len(files)], 0).astype(np.uint8)
        assert np.array_equal(fused[k], want), (files[k % len(files)], k)
    assert np.array_equal(plain[0], gray)
    # any non-zero slot value picks bg_b
    desc_d[:, 5] = 7
    fused7 = eng.bmp_unpack(raw, desc_d, lut_d, H, W, background=bg2).cpu().numpy()
    assert np.array_equal(fused7[:len(files)], fused[len(files):])
    with pytest.raises(ValueError):
        eng.bmp_unpack(raw, desc_d, lut_d, H, W, background=bg2[0])


# --------------------------------------------------------------------------------------------------------------------
# end to end: background= equals running on frames subtracted beforehand, bit for bit
# --------------------------------------------------------------------------------------------------------------------
H0, W0, N0 = 128, 160, 6


@pytest.fixture(scope="module")
def frames():
    from torchpiv_amd import synth
    A, B = synth.make_batch(N0, H0, W0, kind="wavy", noise=1.5)
    # a static band so that the minimum is more than the constant offset
    g = torch.Generator().manual_seed(5)
    band = torch.zeros(H0, W0, dtype=torch.int32)
    band[40:72] = torch.randint(0, 90, (32, W0), generator=g, dtype=torch.int32)
    A = (A.int() + band).clamp(max=255).to(torch.uint8)
    B = (B.int() + band).clamp(max=255).to(torch.uint8)
    return A, B


def _fields(gen):
    """{pair index: (u, v)} of a batched() / indexed run (numpy)."""
    out = {}
    for i, x, y, u, v in gen:
        out[i] = (np.asarray(u), np.asarray(v))
    return out


def _same(f1, f2):
    assert sorted(f1) == sorted(f2)
    for i in f1:
        assert np.array_equal(f1[i][0], f2[i][0], equal_nan=True) and np.array_equal(f1[i][1], f2[i][1], equal_nan=True), i


CHAINS = [("CWS", 32, 16, 2), ("DWS", 32, 16, 2)]


@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("mode,ws,ov,mp_", CHAINS)
def test_resident_background_equals_presubtracted_frames(frames, precision, mode, ws, ov, mp_):
    import torchpiv_amd as T
    A, B = (t.cuda() for t in frames)
    Ac, Bc = A.clone(), B.clone()
    kw = dict(multipass=mp_, multipass_mode=mode, precision=precision)
    As, Bs = _sub(A, A.amin(0)), _sub(B, B.amin(0))
    want = _fields(T.ResidentPIV(As, Bs, ws, ov, **kw).batched(4))
    assert len(want) > 0
    piv = T.ResidentPIV(A, B, ws, ov, background="min", **kw)
    bg_a, bg_b = piv.compute_background()
    assert torch.equal(bg_a, A.amin(0)) and torch.equal(bg_b, B.amin(0))
    _same(_fields(piv.batched(4)), want)
    assert piv._bg_frames.shape == (2, 4, H0, W0)
    # a subset of the pairs: the full run's rows (the background is the dataset's, not the subset's)
    sub = [4, 1, 3]
    got = _fields(piv.batched(2, indices=sub))
    _same(got, {i: want[i] for i in sub if i in want})
    # the background of a subset, given as a pair (bg_a, bg_b); one image for both frames
    ba, bb = piv.compute_background(indices=[0, 2])
    assert torch.equal(ba, A[[0, 2]].amin(0)) and torch.equal(bb, B[[0, 2]].amin(0))
    _same(_fields(T.ResidentPIV(A, B, ws, ov, background=(ba.cpu().numpy(), bb), **kw).batched(3)),
          _fields(T.ResidentPIV(_sub(A, ba), _sub(B, bb), ws, ov, **kw).batched(3)))
    one = (A.amin(0) // 2).cpu()
    _same(_fields(T.ResidentPIV(A, B, ws, ov, background=one, **kw).batched(6)),
          _fields(T.ResidentPIV(_sub(A, one.cuda()), _sub(B, one.cuda()), ws, ov, **kw).batched(6)))
    # the caller's frames are never written
    torch.cuda.synchronize()
    assert torch.equal(A, Ac) and torch.equal(B, Bc)
    piv.close()


def _write_folder(path, A, B):
    from PIL import Image
    for i in range(A.shape[0]):
        Image.fromarray(A[i].numpy(), "L").save(path / f"image{i}_a.bmp")
        Image.fromarray(B[i].numpy(), "L").save(path / f"image{i}_b.bmp")


@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("mode,ws,ov,mp_", CHAINS)
def test_offline_background_equals_presubtracted_frames(tmp_path, frames, precision, mode, ws, ov, mp_):
    """OfflinePIV over a BMP folder with background="min" / given: batched() (fused unpack), __call__ through
    batched() and through the one-pair path (subtraction after upload) all give the fields of ResidentPIV on frames
    subtracted in torch."""
    import torchpiv_amd as T
    A, B = frames
    _write_folder(tmp_path, A, B)
    kw = dict(multipass=mp_, multipass_mode=mode, precision=precision)
    As, Bs = _sub(A, A.amin(0)), _sub(B, B.amin(0))
    want = _fields(T.ResidentPIV(As.cuda(), Bs.cuda(), ws, ov, **kw).batched(4))
    piv = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", ws, ov, background="min", **kw)
    bg_a, bg_b = piv.compute_background()
    assert torch.equal(bg_a.cpu(), A.amin(0)) and torch.equal(bg_b.cpu(), B.amin(0))
    _same(_fields(piv.batched(4)), want)
    _same(_fields(piv.batched(2, indices=[5, 0, 2])), {i: want[i] for i in (5, 0, 2) if i in want})
    order = sorted(want)
    for call_batch in (32, 1):                    # through batched(), and the one-pair path
        p2 = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", ws, ov, background="min", **kw)
        p2.call_batch = call_batch
        res = list(p2())
        assert len(res) == len(order)
        for i, (x, y, u, v) in zip(order, res):
            assert np.array_equal(u, want[i][0], equal_nan=True) and np.array_equal(v, want[i][1], equal_nan=True)
        p2.close()
    # given (bg_a, bg_b)
    ga, gb = (A.amin(0) // 3), (B.amin(0) // 2)
    want_g = _fields(T.ResidentPIV(_sub(A, ga).cuda(), _sub(B, gb).cuda(), ws, ov, **kw).batched(4))
    pg = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", ws, ov, background=(ga.numpy(), gb), **kw)
    _same(_fields(pg.batched(3)), want_g)
    pg.call_batch = 1
    assert len(list(pg())) == len(want_g)
    # background=None: today's fields
    _same(_fields(T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", ws, ov, **kw).batched(4)),
          _fields(T.ResidentPIV(A.cuda(), B.cuda(), ws, ov, **kw).batched(4)))
    piv.close()
    pg.close()


def _folder_with_unstageable_pairs(tmp_path):
    """6 pairs of 96 x 128 BMPs of which pair 2 has a truncated a file (undecodable) and pair 4 another frame shape;
    (A, B, H, W, the good pairs)."""
    from PIL import Image
    from torchpiv_amd import synth
    H, W, good = 96, 128, [0, 1, 3, 5]
    A, B = synth.make_batch(6, H, W, kind="wavy", noise=1.5)
    g = torch.Generator().manual_seed(3)
    band = torch.zeros(H, W, dtype=torch.int32)
    band[8:30] = torch.randint(0, 90, (22, W), generator=g, dtype=torch.int32)
    A = (A.int() + band).clamp(max=255).to(torch.uint8)
    B = (B.int() + band).clamp(max=255).to(torch.uint8)
    A[:, 40:64, 50:74] = 0                       # dead windows: every pair holds invalid vectors to fill
    B[:, 40:64, 50:74] = 0
    _write_folder(tmp_path, A, B)
    blob = (tmp_path / "image2_a.bmp").read_bytes()
    (tmp_path / "image2_a.bmp").write_bytes(blob[:len(blob) // 2])
    for s_, F in (("a", A), ("b", B)):
        Image.fromarray(F[4, :80].numpy(), "L").save(tmp_path / f"image4_{s_}.bmp")
    return A, B, H, W, good


def test_file_staging_with_unstageable_pairs_and_a_stale_reader(tmp_path):
    """The file staging that batched() and compute_background() share, over 6 pairs of 96 x 128 BMPs of which pair 2 has
    a truncated a file (undecodable) and pair 4 another frame shape: the minimum leaves both out at any batch size; the
    fields of the good pairs are those of ResidentPIV on frames subtracted in torch; pair 4 reaches the one-pair path
    when its turn comes, where the dataset's background does not fit its shape (ValueError, after the pairs before it);
    a generator abandoned without close() leaves a live reader behind, which the next run -- of either kind -- stops."""
    import torchpiv_amd as T
    A, B, H, W, good = _folder_with_unstageable_pairs(tmp_path)
    kw = dict(multipass=2, multipass_mode="CWS")
    min_a, min_b = A[good].amin(0), B[good].amin(0)
    res = _fields(T.ResidentPIV(_sub(A[good], min_a).cuda(), _sub(B[good], min_b).cuda(), 32, 16, **kw).batched(4))
    want = {good[k]: f for k, f in res.items()}
    assert len(want) >= 2
    piv = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", 32, 16, background="min", **kw)
    assert len(piv) == 6 and piv.frame_shape() == (H, W)
    for bs in (2, 32):
        bg_a, bg_b = piv.compute_background(batch_size=bs)
        assert torch.equal(bg_a.cpu(), min_a) and torch.equal(bg_b.cpu(), min_b), bs
    e_a, e_b = piv.compute_background(indices=[])
    assert e_a.shape == (H, W) and int(e_a.min()) == 255 and int(e_b.min()) == 255
    every = [0, 1, 2, 3, 5]
    _same(_fields(piv.batched(4, indices=every)), want)
    # the whole folder: pair 4 takes the one-pair path, which refuses the background of another shape
    got = {}
    with pytest.raises(ValueError, match="background of shape"):
        for i, x, y, u, v in piv.batched(4):
            got[i] = (np.asarray(u), np.asarray(v))
    _same(got, {i: want[i] for i in want if i < 4})
    # abandoned generators, still referenced (their finally has not run: the reader is live)
    gen1 = piv.batched(2, indices=every)
    first = next(gen1)
    assert first[0] == min(want) and np.array_equal(first[3], want[first[0]][0], equal_nan=True)
    rd1 = piv._reader
    assert rd1._h is not None
    bg_a, bg_b = piv.compute_background()
    assert rd1._h is None                         # stopped by compute_background
    assert torch.equal(bg_a.cpu(), min_a) and torch.equal(bg_b.cpu(), min_b)
    gen2 = piv.batched(2, indices=every)
    next(gen2)
    rd2 = piv._reader
    assert rd2._h is not None
    _same(_fields(piv.batched(2, indices=every)), want)
    assert rd2._h is None and piv._reader._h is None
    gen1.close()
    gen2.close()
    piv.close()


def test_ensemble_and_tracks_over_unstageable_pairs_and_a_stale_reader(tmp_path):
    """The same folder under ensemble() and tracks(), which read through the staging of batched(): the pairs that cannot be
    staged are left out -- ensemble() over the whole folder is ensemble() over the good pairs, tracks() yields no id of
    the others --, and a tracks() generator abandoned after its first tuple leaves a live reader behind that the next
    batched() stops, to deliver what a fresh object delivers."""
    import torchpiv_amd as T
    _, _, H, W, good = _folder_with_unstageable_pairs(tmp_path)
    kw = dict(multipass=2, multipass_mode="CWS", background="min")
    piv = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", 32, 16, **kw)
    whole, picked = piv.ensemble(batch_size=2), piv.ensemble(indices=good, batch_size=4)
    assert whole is not None and len(whole) == 4
    assert all(np.array_equal(f, g, equal_nan=True) for f, g in zip(whole, picked))
    ids = [t[0] for t in piv.tracks(60, batch_size=2)]
    assert ids and set(ids) <= set(good) and ids == [t[0] for t in piv.tracks(60, indices=good, batch_size=4)]
    every = [0, 1, 2, 3, 5]
    gen = piv.tracks(60, batch_size=2)
    assert next(gen)[0] == ids[0]
    rd = piv._reader
    assert rd._h is not None                      # abandoned, still referenced: its finally has not run
    got = _fields(piv.batched(2, indices=every))
    assert rd._h is None and piv._reader._h is None
    fresh = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", 32, 16, **kw)
    want = _fields(fresh.batched(2, indices=every))
    assert len(want) >= 2
    _same(got, want)
    gen.close()
    fresh.close()
    piv.close()


def test_runner_passes_background(tmp_path, frames):
    from torchpiv_amd import runner
    A, B = frames
    _write_folder(tmp_path, A, B)
    seen = {}
    runner.run_folder(str(tmp_path), "cuda:0", "bmp", 32, 16, multipass=2, background="min",
                      on_pair=lambda i, out: seen.__setitem__(i, out["Vx[m/s]"]))
    import torchpiv_amd as T
    want = _fields(T.ResidentPIV(_sub(A, A.amin(0)).cuda(), _sub(B, B.amin(0)).cuda(), 32, 16, multipass=2).batched(4))
    assert sorted(seen) == sorted(want)
    assert all(np.array_equal(seen[i], want[i][0], equal_nan=True) for i in seen)


# --------------------------------------------------------------------------------------------------------------------
# the effect on a scene
# --------------------------------------------------------------------------------------------------------------------
SH, SW, SN, LO, HI = 192, 192, 16, 64, 128


def _scene():
    """16 clean pairs of a uniform flow (2.3, -1.6) px (synth), and the same with a static speckle band (rows 64-127,
    grey levels 0-160, identical in both frames, saturating at 255)."""
    from torchpiv_amd import synth
    A, B = synth.make_batch(SN, SH, SW, kind="uniform")
    g = torch.Generator().manual_seed(77)
    sp = torch.zeros(SH, SW, dtype=torch.int32)
    sp[LO:HI] = torch.randint(0, 161, (HI - LO, SW), generator=g, dtype=torch.int32)
    return A, B, (A.int() + sp).clamp(max=255).to(torch.uint8), (B.int() + sp).clamp(max=255).to(torch.uint8)


def test_min_background_removes_a_static_band():
    """Vectors inside the band (output rows whose 16 px windows of the 32/16 -> 16/8 CWS chain lie wholly in it),
    compared with the clean scene's over the pairs both runs yield, in px.

    Thresholds, from oracle.piv_oracle.offline_piv on the CPU (the reference's arithmetic) on the same frames, pair by
    pair (4 pairs of the clean run survive the reference's drop rule, 644 band vectors):
      band, no background:  median error 2.49 px, median |d| 0.29 px (clean: 2.78 px) -- locked towards 0;
      band, "min":          median error 0.027 px, mean 0.034 px, 90th percentile 0.069 px.
    Asserted with a margin of about 2.5x on the side that proves the effect and 4x on the other: without a background
    the median error exceeds 1.0 px and the median |d| stays below 1.0 px; with "min" the median error is below 0.1 px,
    the mean below 0.15 px and the median |d| within 0.1 px of the clean 2.78."""
    import torchpiv_amd as T
    A, B, Ab, Bb = (t.cuda() for t in _scene())
    kw = dict(multipass=2, multipass_mode="CWS", precision="exact")
    clean = _fields(T.ResidentPIV(A, B, 32, 16, **kw).batched(8))
    band = _fields(T.ResidentPIV(Ab, Bb, 32, 16, **kw).batched(8))
    sub = _fields(T.ResidentPIV(Ab, Bb, 32, 16, background="min", **kw).batched(8))
    from torchpiv_amd import backend
    _, y = backend.get_coordinates((SH, SW), 16, 8)
    yc = y[:, 0]
    rows = np.flatnonzero(((yc - 8 >= LO) & (yc + 8 <= HI))[::-1])          # u, v are flipped along the rows
    assert rows.size >= 5

    def stats(res):
        ks = [k for k in res if k in clean]
        assert len(ks) >= 3
        e = np.concatenate([np.hypot(res[k][0][rows] - clean[k][0][rows], res[k][1][rows] - clean[k][1][rows]).ravel()
                            for k in ks]) / 1000
        m = np.concatenate([np.hypot(res[k][0][rows], res[k][1][rows]).ravel() for k in ks]) / 1000
        return np.median(e), e.mean(), np.median(m)
    e_band, _, m_band = stats(band)
    e_sub, mean_sub, m_sub = stats(sub)
    m_clean = stats(clean)[2]
    print(f"band without background: median error {e_band:.3f} px, median |d| {m_band:.3f} px (clean {m_clean:.3f}); "
          f"with 'min': median error {e_sub:.4f} px, mean {mean_sub:.4f} px, median |d| {m_sub:.3f} px")
    assert e_band > 1.0 and m_band < 1.0
    assert e_sub < 0.1 and mean_sub < 0.15 and abs(m_sub - m_clean) < 0.1
