"""Tile-wise adaptive histogram equalization on the device (equalize.hip) and through every host path: the two kernels
against the numpy model (tests/equalize_model.py) bit for bit -- frames and tables --, equalize= against running on
frames that the model equalized beforehand (bit-identical fields and the same dropped pairs), the keyword left out, and
the effect on a scene whose illumination falls off across the frame."""
import numpy as np
import pytest
import torch

import equalize_model as M
import equalize_scene as S
from depth_model import lut as depth_lut_model
from prefilter_model import prefilter as prefilter_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def _misaligned(t):
    """A copy of t whose data starts one byte past a 16-byte boundary (the kernels' byte paths)."""
    buf = torch.empty(t.numel() + 1, dtype=torch.uint8, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    return out


# (n, H, W, tile) and what the stack is for
STACKS = [(3, 200, 264, 64),     # uneven 3 x 4 grid
          (2, 45, 333, 16),      # odd width, no 16-byte rows
          (1, 5, 300, 64),       # one tile row
          (1, 64, 64, 256),      # a single tile, no blend
          (2, 97, 8, 8),         # narrow
          (2, 1024, 1024, 64)]   # many tiles
CLIPS = [1.0, 3.0, 256]


def _contents(n, H, W, tile):
    """{name: uint8 numpy [n, H, W]}: particle frames, noise, all 0, all 255, one grey level plus a single other pixel, and
    frames whose tiles hold 99 % of their pixels in one bin (the histogram's contention path; the clipped excess of such
    a tile is no multiple of 256)."""
    from torchpiv_amd import synth
    rng = np.random.default_rng(n * 100000 + H * 1000 + W)
    out = {"particles": synth.make_batch(n, H, W, kind="uniform", noise=1.0)[0].numpy(),
           "noise": rng.integers(0, 256, (n, H, W)).astype(np.uint8),
           "zeros": np.zeros((n, H, W), np.uint8), "full": np.full((n, H, W), 255, np.uint8)}
    one = np.full((n, H, W), 40, np.uint8)
    one[:, H // 2, W // 3] = 41
    one[n - 1, H - 1, W - 1] = 9
    out["one level"] = one
    heavy = np.full((n, H, W), 3, np.uint8)
    other = rng.random((n, H, W)) < 0.01
    heavy[other] = rng.integers(0, 256, int(other.sum())).astype(np.uint8)
    out["99 % in one bin"] = heavy
    return out


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("n,H,W,tile", STACKS)
def test_kernels_equal_model(eng, n, H, W, tile, clip):
    clip_q8 = M.clip_q8_of(clip)
    for name, F_h in _contents(n, H, W, tile).items():
        want, want_t = M.equalize(F_h, tile, clip_q8, return_luts=True)
        want, want_t = torch.from_numpy(want), torch.from_numpy(want_t)
        F = torch.from_numpy(F_h).cuda()
        keep = F.clone()
        got, tabs = eng.equalize(F, tile, clip, return_luts=True)
        tag = (name, tile, clip)
        assert tabs.shape == want_t.shape and torch.equal(tabs.cpu(), want_t), tag       # the table kernel
        assert torch.equal(got.cpu(), want), tag                                         # the map kernel
        assert torch.equal(F, keep), tag                                                 # the input is not written
        if name in ("particles", "99 % in one bin"):
            # an odd-offset view as input and as output (byte paths of both kernels); a view that is not contiguous
            Fm = _misaligned(F)
            got, tabs = eng.equalize(Fm, tile, clip, return_luts=True, out=_misaligned(torch.full_like(F, 7)))
            assert torch.equal(tabs.cpu(), want_t) and torch.equal(got.cpu(), want), tag
            wide = torch.zeros(n, H, W + 3, dtype=torch.uint8, device="cuda")
            wide[:, :, 2:W + 2] = F
            assert torch.equal(eng.equalize(wide[:, :, 2:W + 2], tile, clip).cpu(), want), tag
            assert torch.equal(eng.equalize(F[n - 1], tile, clip).cpu(), want[n - 1]), tag     # a single 2-D frame
            # in place, with a workspace of the caller's
            work = torch.empty(want_t.numel() + 5, dtype=torch.uint8, device="cuda")
            G = F.clone()
            assert eng.equalize(G, tile, clip, out=G, work=work) is G
            assert torch.equal(G.cpu(), want), tag
            assert torch.equal(work[:want_t.numel()].cpu().view(want_t.shape), want_t), tag
            Gm = Fm.clone()
            eng.equalize(Gm, tile, clip, out=Gm)
            assert torch.equal(Gm.cpu(), want), tag


def test_partly_overlapping_out_is_refused_and_nothing_is_launched(eng):
    buf = torch.full((5 * 16 * 16 + 4 * 4 * 256,), 9, dtype=torch.uint8, device="cuda")
    F = buf[:4 * 256].view(4, 16, 16)
    keep = buf.clone()
    for out in (buf[256:5 * 256].view(4, 16, 16), buf[255:255 + 4 * 256].view(4, 16, 16), buf[1:1 + 4 * 256].view(4, 16, 16)):
        with pytest.raises(ValueError, match="overlaps"):
            eng.equalize(F, 8, 3.0, out=out)
    with pytest.raises(ValueError, match="overlaps"):                # the workspace (2 x 2 tiles a frame) reaches into the frames
        eng.equalize(F, 8, 3.0, work=buf[1000:])
    torch.cuda.synchronize()
    assert torch.equal(buf, keep)
    with pytest.raises(ValueError):
        eng.equalize(F, 7, 3.0)
    with pytest.raises(ValueError):
        eng.equalize(F, 8, 0.5)
    with pytest.raises(ValueError):
        eng.equalize(F, 8, 3.0, out=torch.zeros(4, 16, 15, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        eng.equalize(F, 8, 3.0, work=torch.zeros(4 * 4 * 256 - 1, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(buf, keep)


# --------------------------------------------------------------------------------------------------------------------
# end to end: equalize= equals running on frames equalized beforehand by the model, bit for bit
# --------------------------------------------------------------------------------------------------------------------
H0, W0, N0 = 256, 256, 4
WS, OV, MP = 32, 16, 2                       # 32/16 -> 16/8, CWS
EQ = {"tile": 48, "clip": 2.5}
PF = {"kind": "min", "size": 15, "cap": 200}
DEPTH = {"lo": 100, "hi": 3000}


@pytest.fixture(scope="module")
def frames():
    """Four wavy 256 x 256 pairs with a static band (so that a background has something to remove), brighter on one side."""
    from torchpiv_amd import synth
    A, B = synth.make_batch(N0, H0, W0, kind="wavy", noise=1.5)
    g = torch.Generator().manual_seed(7)
    band = torch.zeros(H0, W0, dtype=torch.int32)
    band[90:130] = torch.randint(0, 70, (40, W0), generator=g, dtype=torch.int32)
    gain = (0.3 + 0.7 * torch.arange(W0) / (W0 - 1))[None, None, :]
    A = ((A.float() * gain).int() + band).clamp(max=255).to(torch.uint8)
    B = ((B.float() * gain).int() + band).clamp(max=255).to(torch.uint8)
    return A, B


def _eq_t(F, eq=EQ):
    return torch.from_numpy(M.equalize(F.numpy(), eq["tile"], M.clip_q8_of(eq["clip"])))


def _chain_t(F, bg):
    """background, pre-filter and cap, equalize -- the three models in the order of the device."""
    return _eq_t(torch.from_numpy(prefilter_model(F.numpy(), PF["kind"], PF["size"], PF["cap"], bg.numpy())))


def _bits(a):
    a = np.ascontiguousarray(np.asarray(a))
    return a.view(np.int64) if a.dtype == np.float64 else a.view(np.uint8) if a.dtype == np.bool_ else a


def _fields(gen):
    """{pair index: (u, v)} of a batched() / indexed run (numpy; masked fields as data and mask); a dropped pair has no
    entry."""
    out = {}
    for i, x, y, u, v in gen:
        out[i] = tuple((np.ma.getdata(f), np.ma.getmaskarray(f)) for f in (u, v))
    return out


def _same(f1, f2):
    assert sorted(f1) == sorted(f2)
    for i in f1:
        for (d1, m1), (d2, m2) in zip(f1[i], f2[i]):
            assert np.array_equal(_bits(m1), _bits(m2)), i                   # masks and fields as integer views
            assert np.array_equal(_bits(d1)[~m1], _bits(d2)[~m2]), i


@pytest.fixture(scope="module")
def wanted(frames):
    """The fields of ResidentPIV on frames the models processed beforehand, per (precision, chain of filters); computed
    once and shared."""
    import torchpiv_amd as T
    A, B = frames
    ba, bb = A.amin(0), B.amin(0)
    pre = {"eq": (_eq_t(A), _eq_t(B)), "chain": (_chain_t(A, ba), _chain_t(B, bb))}
    out = {}
    for precision in ("exact", "fast"):
        for key, (Af, Bf) in pre.items():
            piv = T.ResidentPIV(Af.cuda(), Bf.cuda(), WS, OV, multipass=MP, multipass_mode="CWS", precision=precision)
            out[precision, key] = _fields(piv.batched(4))
            piv.close()
            assert len(out[precision, key]) > 0
    return out


CHAIN_KW = {"background": "min", "prefilter": PF}


@pytest.mark.parametrize("precision", ["exact", "fast"])
def test_resident_equalize_equals_equalized_frames(frames, wanted, precision):
    import torchpiv_amd as T
    A, B = frames
    Ad, Bd = A.cuda(), B.cuda()
    Ac, Bc = Ad.clone(), Bd.clone()
    kw = dict(multipass=MP, multipass_mode="CWS", precision=precision)
    want = wanted[precision, "eq"]
    piv = T.ResidentPIV(Ad, Bd, WS, OV, equalize=EQ, **kw)
    _same(_fields(piv.batched(4)), want)
    assert piv._bg_frames.shape == (2, 4, H0, W0) and piv._pf_frames is None          # one reused buffer
    work = piv._eq_work
    sub = [3, 0, 2]                                                                   # gathered pairs, a short last chunk
    _same(_fields(piv.batched(2, indices=sub)), {i: want[i] for i in sub if i in want})
    assert piv._eq_work is work                                                       # the workspace is kept
    piv.close()
    # background, pre-filter and cap, then equalize, in place on the one reused buffer
    piv = T.ResidentPIV(Ad, Bd, WS, OV, equalize=EQ, **CHAIN_KW, **kw)
    _same(_fields(piv.batched(4)), wanted[precision, "chain"])
    assert piv._bg_frames.shape == (2, 4, H0, W0) and piv._pf_frames is None
    piv.close()
    torch.cuda.synchronize()
    assert torch.equal(Ad, Ac) and torch.equal(Bd, Bc)                                # the caller's frames are never written


def test_resident_depth_then_equalize(frames):
    """uint16 stacks: tone map, then equalize in place on the tone map's buffer."""
    import torchpiv_amd as T
    A, B = frames
    A16 = (A.to(torch.int32) * 11 + 100).to(torch.uint16)
    B16 = (B.to(torch.int32) * 11 + 100).to(torch.uint16)
    table = torch.from_numpy(depth_lut_model(DEPTH["lo"], DEPTH["hi"]))
    A8, B8 = table[A16.long()], table[B16.long()]
    kw = dict(multipass=MP, multipass_mode="CWS")
    ref = T.ResidentPIV(_eq_t(A8).cuda(), _eq_t(B8).cuda(), WS, OV, **kw)
    want = _fields(ref.batched(4))
    ref.close()
    Ad, Bd = A16.cuda(), B16.cuda()
    Ac, Bc = Ad.clone(), Bd.clone()
    piv = T.ResidentPIV(Ad, Bd, WS, OV, depth=DEPTH, equalize=EQ, **kw)
    _same(_fields(piv.batched(4)), want)
    assert piv._bg_frames is None and piv._depth_frames.shape == (2, 4, H0, W0)
    piv.close()
    torch.cuda.synchronize()
    assert torch.equal(Ad, Ac) and torch.equal(Bd, Bc)


def _write_folder(path, A, B):
    from PIL import Image
    for i in range(A.shape[0]):
        Image.fromarray(A[i].numpy(), "L").save(path / f"image{i}_a.bmp")
        Image.fromarray(B[i].numpy(), "L").save(path / f"image{i}_b.bmp")


@pytest.mark.parametrize("precision", ["exact", "fast"])
def test_offline_equalize_equals_equalized_frames(tmp_path, frames, wanted, precision):
    """OfflinePIV over a BMP folder: batched(3) (one call over the unpacked stack, in place), __call__ through batched()
    and through the one-pair loop (call_batch = 1) give the fields of ResidentPIV on frames that the models processed."""
    import torchpiv_amd as T
    A, B = frames
    _write_folder(tmp_path, A, B)
    kw = dict(multipass=MP, multipass_mode="CWS", precision=precision)
    for key, extra in (("eq", {}), ("chain", CHAIN_KW)):
        want = wanted[precision, key]
        piv = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", WS, OV, equalize=EQ, **extra, **kw)
        _same(_fields(piv.batched(3)), want)
        assert (piv._pf_frames is None) == (not extra)
        piv.close()
        order = sorted(want)
        p2 = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", WS, OV, equalize=EQ, **extra, **kw)
        p2.call_batch = 1                                                             # the one-pair loop
        res = list(p2())
        p2.close()
        assert len(res) == len(order)
        for i, (x, y, u, v) in zip(order, res):
            _same({i: tuple((np.ma.getdata(f), np.ma.getmaskarray(f)) for f in (u, v))}, {i: want[i]})


def test_runner_passes_equalize(tmp_path, frames, wanted):
    import torchpiv_amd as T
    from torchpiv_amd import runner
    A, B = frames
    _write_folder(tmp_path, A, B)
    seen = {}
    runner.run_folder(str(tmp_path), "cuda:0", "bmp", WS, OV, multipass=MP, equalize=EQ, batch_size=3,
                      on_pair=lambda i, out: seen.__setitem__(i, out["Vx[m/s]"]))
    want = wanted["exact", "eq"]
    assert sorted(seen) == sorted(want)
    for i in seen:
        d, m = want[i][0]
        assert np.array_equal(_bits(np.ma.getmaskarray(seen[i])), _bits(m))
        assert np.array_equal(_bits(np.ma.getdata(seen[i]))[~m], _bits(d)[~m]), i
    # "clahe" is the dict of the defaults
    piv = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", WS, OV, multipass=MP, equalize="clahe")
    got = _fields(piv.batched(4))
    piv.close()
    ref = T.ResidentPIV(_eq_t(A, {"tile": 64, "clip": 3.0}).cuda(), _eq_t(B, {"tile": 64, "clip": 3.0}).cuda(), WS, OV,
                        multipass=MP)
    _same(got, _fields(ref.batched(4)))
    ref.close()


def test_off_means_off(tmp_path, frames):
    """equalize=None, and the keyword left out, give the fields of a run on the frames as they are, on all three entry
    points, with and without the other filters; no workspace is allocated."""
    import torchpiv_amd as T
    from torchpiv_amd import runner
    A, B = frames
    _write_folder(tmp_path, A, B)
    for extra in ({}, CHAIN_KW):
        kw = dict(multipass=MP, multipass_mode="CWS", **extra)
        r0 = T.ResidentPIV(A.cuda(), B.cuda(), WS, OV, **kw)
        r1 = T.ResidentPIV(A.cuda(), B.cuda(), WS, OV, equalize=None, **kw)
        base = _fields(r0.batched(4))
        assert len(base) > 0
        _same(_fields(r1.batched(4)), base)
        assert r1._eq_work is None and (r1._bg_frames is None) == (not extra)
        o0 = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", WS, OV, **kw)
        o1 = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", WS, OV, equalize=None, **kw)
        _same(_fields(o0.batched(3)), base)
        _same(_fields(o1.batched(3)), base)
        o1.call_batch = 1
        res = list(o1())                                                              # the one-pair loop
        assert len(res) == len(base)
        for i, (x, y, u, v) in zip(sorted(base), res):
            _same({i: tuple((np.ma.getdata(f), np.ma.getmaskarray(f)) for f in (u, v))}, {i: base[i]})
        assert o1._eq_work is None and o1._equalize is None
        for p in (r0, r1, o0, o1):
            p.close()
        seen = {}
        for ekw in ({}, {"equalize": None}):
            seen.clear()
            runner.run_folder(str(tmp_path), "cuda:0", "bmp", WS, OV, multipass=MP, batch_size=3, **extra, **ekw,
                              on_pair=lambda i, out: seen.__setitem__(i, out["Vx[m/s]"]))
            assert sorted(seen) == sorted(base)
            for i in seen:
                d, m = base[i][0]
                assert np.array_equal(_bits(np.ma.getdata(seen[i]))[~m], _bits(d)[~m]), i


# --------------------------------------------------------------------------------------------------------------------
# the effect on a scene
# --------------------------------------------------------------------------------------------------------------------
def test_clahe_recovers_vectors_under_an_illumination_ramp(eng):
    """Raw vectors of the last pass of the 32/16 -> 16/8 CWS chain ("exact") on tests/equalize_scene.py -- four 256 x 256
    pairs of a uniform (2.3, -1.6) px flow whose illumination falls linearly to 15 % at column 0 --, 4 x 31 x 31 = 3844 of
    them, against the same chain on the clean frames.  Bad = invalid, or more than 0.5 px from the clean run's vector.

    From oracle.piv_oracle on the CPU (the reference's arithmetic; pass1 and IterCWS per pair) with the numpy model as
    the filter, on the same frames (the clean run itself holds 3 invalid vectors):
      no filter:                          53 bad; bright half (x >= 128) within 0.6864 px of the clean run
      equalize "clahe" (tile 64, clip 3): 13 bad; bright half within 0.2246 px
    (with the ramp's floor at 5 % instead: 113 and 61 bad; "clahe" on the clean frames themselves: 4 bad, 0.1396 px -- the
    equalization moves sub-pixel fits by that much where nothing was wrong).
    Asserted with half the measured difference as margin: the equalized run has at least 20 bad vectors fewer than the
    unfiltered run, and its bright half stays within 0.2246 + 0.001 px of the clean run (the oracle's figure plus a
    thousand times the 1e-6 px between device and oracle).  The device's own figures are printed."""
    from torchpiv_amd import backend, engine
    A, B, Ar, Br = (torch.from_numpy(t) for t in S.ramp_scene())
    ws, ov, n_pass = S.CHAIN
    x, y = backend.get_coordinates((S.H, S.W), ws // 2, ov // 2)
    plan = engine.Plan(S.H, S.W, ws, ov, n_pass=n_pass, mode="CWS", max_batch=S.N, device="cuda:0", precision="exact")

    def run(a, b):
        u, v, inv = plan.run(a, b)
        torch.cuda.synchronize()
        u, v, inv = u.cpu().numpy(), v.cpu().numpy(), inv.cpu().numpy()
        return [(u[i], v[i], inv[i]) for i in range(S.N)]
    Ad, Bd = Ar.cuda(), Br.cuda()
    clean = run(A.cuda(), B.cuda())
    none = S.stats(run(Ad, Bd), clean, x)
    clahe = S.stats(run(eng.equalize(Ad, 64, 3.0), eng.equalize(Bd, 64, 3.0)), clean, x)
    plan.close()
    print(f"bad vectors of {S.N * x.size}: no filter {none[0]}, equalize 'clahe' {clahe[0]}; largest distance from the "
          f"clean run in the bright half: {none[1]:.4f} / {clahe[1]:.4f} px")
    assert none[0] - clahe[0] >= 20
    assert clahe[1] < 0.2246 + 1e-3
