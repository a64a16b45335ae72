"""Spatial pre-filters on the device (prefilter.hip) and through every host path: the kernel against the numpy model
(tests/prefilter_model.py) bit for bit, prefilter= against running on frames that the model filtered beforehand
(bit-identical fields and the same dropped pairs), and the effect on a scene whose background changes from frame to frame."""
import numpy as np
import pytest
import torch

from prefilter_model import prefilter as model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def _misaligned(t):
    """A copy of t whose data starts one byte past a 16-byte boundary (the kernels' byte path)."""
    buf = torch.empty(t.numel() + 1, dtype=torch.uint8, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    return out


# (n, H, W): smaller than any window and than a tile (5 x 7); odd sizes, W % 16 != 0 (byte path) and == 0 (16-byte path);
# n = 1, odd n, even n; 70 x 150 and 100 x 288 span two tiles of 64 rows and two / three tiles of 128 columns -- the kernel's
# tile is 128 x 64 (PREFILTER_TILE_COLS x PREFILTER_TILE_ROWS), so at size 63 the 31-pixel halo of every tile reaches
# across the tile borders at row 64 and columns 128 and 256, in the 16-byte path (W = 288) and in the byte path (W = 150)
SHAPES = [(1, 5, 7), (3, 37, 50), (2, 24, 48), (1, 70, 150), (2, 100, 288)]
FILTERS = [(kind, size) for kind in ("min", "mean") for size in (3, 15, 63)] + [(None, None)]


@pytest.mark.parametrize("n,H,W", SHAPES)
def test_kernel_equals_model(eng, n, H, W):
    g = torch.Generator().manual_seed(n * 1000 + H * 7 + W)
    bg_h = torch.randint(0, 140, (H, W), generator=g, dtype=torch.uint8)
    data = {"random": torch.randint(0, 256, (n, H, W), generator=g, dtype=torch.uint8),
            "zeros": torch.zeros(n, H, W, dtype=torch.uint8), "full": torch.full((n, H, W), 255, dtype=torch.uint8)}
    # a random frame with structure at the scale of the windows, so that minima and means differ from pixel to pixel
    data["random"][:, : H // 2] //= 3
    for name, F_h in data.items():
        F = F_h.cuda()
        Fm = _misaligned(F)
        keep = F.clone()
        for kind, size in FILTERS:
            for bg_h_ in (None, bg_h):
                caps = (None, 90) if kind is not None else (90, 255)
                for cap in caps:
                    want = torch.from_numpy(model(F_h.numpy(), kind, size, cap, None if bg_h_ is None else bg_h_.numpy()))
                    bg = None if bg_h_ is None else bg_h_.cuda()
                    tag = (name, kind, size, cap, bg is not None)
                    got = eng.prefilter(F, kind, size, cap=cap, background=bg)
                    assert torch.equal(got.cpu(), want), tag
                    assert torch.equal(eng.prefilter(Fm, kind, size, cap=cap, background=bg).cpu(), want), tag
                    if name == "random":
                        # a misaligned background / output, a given output, a single 2-D frame
                        out = _misaligned(torch.full_like(F, 7))
                        bgm = None if bg is None else _misaligned(bg)
                        assert eng.prefilter(F, kind, size, cap=cap, background=bgm, out=out) is out
                        assert torch.equal(out.cpu(), want), tag
                        assert torch.equal(eng.prefilter(F[n - 1], kind, size, cap=cap, background=bg).cpu(), want[n - 1]), tag
        torch.cuda.synchronize()
        assert torch.equal(F, keep) and torch.equal(Fm, keep)              # the input is never written


def test_overlapping_out_is_refused_and_nothing_is_launched(eng):
    buf = torch.full((5 * 16 * 16,), 9, dtype=torch.uint8, device="cuda")
    F = buf[:4 * 256].view(4, 16, 16)
    keep = buf.clone()
    for out in (F, buf[256:].view(4, 16, 16), buf[255:255 + 4 * 256].view(4, 16, 16)):
        for kind, size, cap in (("min", 3, None), ("mean", 5, 20), (None, None, 3)):
            with pytest.raises(ValueError, match="overlaps"):
                eng.prefilter(F, kind, size, cap=cap, out=out)
    torch.cuda.synchronize()
    assert torch.equal(buf, keep)
    with pytest.raises(ValueError):
        eng.prefilter(F, "min", 4)
    with pytest.raises(ValueError):
        eng.prefilter(F, "min", 3, background=torch.zeros(16, 15, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        eng.prefilter(F, "min", 3, out=torch.zeros(4, 16, 15, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        eng.prefilter(F, None, None)


# --------------------------------------------------------------------------------------------------------------------
# end to end: prefilter= equals running on frames filtered beforehand by the model, bit for bit
# --------------------------------------------------------------------------------------------------------------------
H0, W0, N0 = 128, 160, 6
CHAINS = [("CWS", 32, 16, 2), ("DWS", 32, 16, 2)]
PF = {"kind": "min", "size": 15}
PF2 = {"kind": "mean", "size": 7, "cap": 120}


@pytest.fixture(scope="module")
def frames():
    """Six wavy pairs with a static band (so that a background has something to remove) and a per-frame pedestal."""
    from torchpiv_amd import synth
    A, B = synth.make_batch(N0, H0, W0, kind="wavy", noise=1.5)
    g = torch.Generator().manual_seed(5)
    band = torch.zeros(H0, W0, dtype=torch.int32)
    band[40:72] = torch.randint(0, 90, (32, W0), generator=g, dtype=torch.int32)
    ped = torch.randint(0, 60, (2, N0, 1, 1), generator=g, dtype=torch.int32)
    A = (A.int() + band + ped[0]).clamp(max=255).to(torch.uint8)
    B = (B.int() + band + ped[1]).clamp(max=255).to(torch.uint8)
    return A, B


def _model_t(F, pf, bg=None):
    return torch.from_numpy(model(F.numpy(), pf["kind"], pf.get("size"), pf.get("cap"), None if bg is None else bg.numpy()))


def _fields(gen):
    """{pair index: (u, v)} of a batched() / indexed run (numpy); a dropped pair has no entry."""
    out = {}
    for i, x, y, u, v in gen:
        out[i] = (np.asarray(u), np.asarray(v))
    return out


def _same(f1, f2):
    assert sorted(f1) == sorted(f2)
    for i in f1:
        assert np.array_equal(f1[i][0], f2[i][0], equal_nan=True) and np.array_equal(f1[i][1], f2[i][1], equal_nan=True), i


@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("mode,ws,ov,mp_", CHAINS)
def test_resident_prefilter_equals_prefiltered_frames(frames, precision, mode, ws, ov, mp_):
    import torchpiv_amd as T
    A, B = frames
    Ad, Bd = A.cuda(), B.cuda()
    Ac, Bc = Ad.clone(), Bd.clone()
    kw = dict(multipass=mp_, multipass_mode=mode, precision=precision)
    want = _fields(T.ResidentPIV(_model_t(A, PF).cuda(), _model_t(B, PF).cuda(), ws, ov, **kw).batched(4))
    assert len(want) > 0
    piv = T.ResidentPIV(Ad, Bd, ws, ov, prefilter=PF, **kw)
    _same(_fields(piv.batched(4)), want)
    assert piv._bg_frames.shape == (2, 4, H0, W0) and piv._pf_frames is None       # one reused buffer
    sub = [4, 1, 3]                                                                # gathered pairs, a short last chunk
    _same(_fields(piv.batched(2, indices=sub)), {i: want[i] for i in sub if i in want})
    piv.close()
    # with background= at the same time: background, then filter, then cap -- in one launch into the same buffer
    ba, bb = A.amin(0), B.amin(0)
    want_bg = _fields(T.ResidentPIV(_model_t(A, PF2, ba).cuda(), _model_t(B, PF2, bb).cuda(), ws, ov, **kw).batched(4))
    piv = T.ResidentPIV(Ad, Bd, ws, ov, background="min", prefilter=PF2, **kw)
    _same(_fields(piv.batched(4)), want_bg)
    assert piv._bg_frames.shape == (2, 4, H0, W0) and piv._pf_frames is None
    piv.close()
    torch.cuda.synchronize()
    assert torch.equal(Ad, Ac) and torch.equal(Bd, Bc)                             # the caller's frames are never written


def _write_folder(path, A, B):
    from PIL import Image
    for i in range(A.shape[0]):
        Image.fromarray(A[i].numpy(), "L").save(path / f"image{i}_a.bmp")
        Image.fromarray(B[i].numpy(), "L").save(path / f"image{i}_b.bmp")


@pytest.mark.parametrize("precision,width", [("exact", W0), ("fast", W0), ("exact", 150)])
@pytest.mark.parametrize("mode,ws,ov,mp_", CHAINS)
def test_offline_prefilter_equals_prefiltered_frames(tmp_path, frames, precision, width, mode, ws, ov, mp_):
    """OfflinePIV over a BMP folder (width 150: rows that are no multiple of 16 bytes): batched() (one launch over the
    unpacked stack), __call__ through batched() and through the one-pair path (background fused into the filter launch)
    all give the fields of ResidentPIV on frames that the model filtered."""
    import torchpiv_amd as T
    A, B = (t[:, :, :width].contiguous() for t in frames)
    _write_folder(tmp_path, A, B)
    kw = dict(multipass=mp_, multipass_mode=mode, precision=precision)
    ba, bb = A.amin(0), B.amin(0)
    for pf, bkw, (Af, Bf) in ((PF, {}, (_model_t(A, PF), _model_t(B, PF))),
                              (PF2, {"background": "min"}, (_model_t(A, PF2, ba), _model_t(B, PF2, bb)))):
        want = _fields(T.ResidentPIV(Af.cuda(), Bf.cuda(), ws, ov, **kw).batched(4))
        assert len(want) > 0
        piv = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", ws, ov, prefilter=pf, **bkw, **kw)
        _same(_fields(piv.batched(4)), want)
        assert piv._pf_frames.shape == (8, H0, width)
        _same(_fields(piv.batched(2, indices=[5, 0, 2])), {i: want[i] for i in (5, 0, 2) if i in want})
        piv.close()
        order = sorted(want)
        for call_batch in (32, 1):                    # through batched(), and the one-pair path
            p2 = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", ws, ov, prefilter=pf, **bkw, **kw)
            p2.call_batch = call_batch
            res = list(p2())
            assert len(res) == len(order)
            for i, (x, y, u, v) in zip(order, res):
                assert np.array_equal(u, want[i][0], equal_nan=True) and np.array_equal(v, want[i][1], equal_nan=True)
            p2.close()


def test_runner_passes_prefilter(tmp_path, frames):
    import torchpiv_amd as T
    from torchpiv_amd import runner
    A, B = frames
    _write_folder(tmp_path, A, B)
    seen = {}
    runner.run_folder(str(tmp_path), "cuda:0", "bmp", 32, 16, multipass=2, prefilter=PF,
                      on_pair=lambda i, out: seen.__setitem__(i, out["Vx[m/s]"]))
    piv = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", 32, 16, multipass=2, prefilter=PF)
    want = _fields(piv.batched(4))
    piv.close()
    assert len(want) > 0 and sorted(seen) == sorted(want)
    assert all(np.array_equal(seen[i], want[i][0], equal_nan=True) for i in seen)
    _same(want, _fields(T.ResidentPIV(_model_t(A, PF).cuda(), _model_t(B, PF).cuda(), 32, 16, multipass=2).batched(4)))


def test_off_means_off(tmp_path, frames):
    """prefilter=None, and the keyword left out, give the fields of a run that knows no such keyword: ResidentPIV and
    OfflinePIV (batched and one-pair), with and without a background; no filter buffer is allocated."""
    import torchpiv_amd as T
    A, B = frames
    _write_folder(tmp_path, A, B)
    for bkw in ({}, {"background": "min"}):
        kw = dict(multipass=2, multipass_mode="CWS", **bkw)
        r0 = T.ResidentPIV(A.cuda(), B.cuda(), 32, 16, **kw)
        r1 = T.ResidentPIV(A.cuda(), B.cuda(), 32, 16, prefilter=None, **kw)
        base = _fields(r0.batched(4))
        _same(_fields(r1.batched(4)), base)
        assert r1._pf_frames is None and (r1._bg_frames is None) == (not bkw)
        o0 = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", 32, 16, **kw)
        o1 = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", 32, 16, prefilter=None, **kw)
        _same(_fields(o0.batched(4)), base)
        _same(_fields(o1.batched(4)), base)
        o1.call_batch = 1
        res = list(o1())                                       # the one-pair path
        assert len(res) == len(base)
        for i, (x, y, u, v) in zip(sorted(base), res):
            assert np.array_equal(u, base[i][0], equal_nan=True) and np.array_equal(v, base[i][1], equal_nan=True), i
        assert o1._pf_frames is None and o1._prefilter is None
        for p in (r0, r1, o0, o1):
            p.close()


# --------------------------------------------------------------------------------------------------------------------
# the effect on a scene
# --------------------------------------------------------------------------------------------------------------------
GN, GH, GW, GAMP, GSIG = 4, 256, 256, 230.0, 30.0


def _glow_scene():
    """Four pairs of a uniform flow (2.3, -1.6) px at half the particle amplitude (synth frames // 2), clean, and with a
    broad Gaussian glow (sigma 30 px, amplitude 138..230 grey levels) added to every frame, amplitude and centre drawn
    anew for each frame of each pair, saturating at 255.  Returns (A, B, A_glow, B_glow, centres [2, n, 2] as (y, x))."""
    from torchpiv_amd import synth
    A, B = synth.make_batch(GN, GH, GW, kind="uniform")
    A, B = A // 2, B // 2
    rng = np.random.default_rng(2024)
    yy, xx = np.mgrid[0:GH, 0:GW]
    out, centres = [], np.empty((2, GN, 2))
    for s, F in enumerate((A, B)):
        G = np.empty((GN, GH, GW), np.int64)
        for i in range(GN):
            amp = GAMP * (0.6 + 0.4 * rng.random())
            cy, cx = rng.uniform(0.3, 0.7) * GH, rng.uniform(0.3, 0.7) * GW
            centres[s, i] = cy, cx
            glow = np.rint(amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * GSIG * GSIG))).astype(np.int64)
            G[i] = np.minimum(F[i].numpy().astype(np.int64) + glow, 255)
        out.append(torch.from_numpy(G.astype(np.uint8)))
    return A, B, out[0], out[1], centres


def _glow_stats(res, clean, x, y, centres):
    """res, clean: per pair (u, v, invalid) of the raw last pass on the grid x, y (px).  Returns (bad, far_max): the
    number of vectors that are invalid or more than 0.5 px from the clean run's, and the largest distance from the clean
    run's among the vectors that are valid in both and more than 4 sigma from both glow centres of their pair."""
    bad, far_max = 0, 0.0
    for i, ((u, v, inv), (cu, cv, cinv)) in enumerate(zip(res, clean)):
        d = np.hypot(u - cu, v - cv)
        bad += int((inv.astype(bool) | (d > 0.5)).sum())
        far = np.ones(x.shape, bool)
        for s in range(2):
            far &= np.hypot(y - centres[s, i, 0], x - centres[s, i, 1]) > 4 * GSIG
        ok = far & ~inv.astype(bool) & ~cinv.astype(bool)
        assert ok.sum() > 50
        far_max = max(far_max, float(d[ok].max()))
    return bad, far_max


def test_min_filter_removes_a_glow_that_changes_from_frame_to_frame(eng):
    """Raw vectors of the last pass of the 32/16 -> 16/8 CWS chain ("exact") on the glow scene, 4 x 31 x 31 = 3844 of
    them, against the same chain on the clean frames.  Bad = invalid, or more than 0.5 px from the clean run's vector.

    From oracle.piv_oracle on the CPU (the reference's arithmetic; pass1 and IterCWS per pair) with the numpy model as
    the filter, on the same frames (the clean run itself holds 3 invalid vectors):
      no filter:                              201 bad (131 invalid)
      background "min" (minimum over 4 pairs): 193 bad (120 invalid) -- the glow differs in every frame, its minimum removes little
      prefilter {"kind": "min", "size": 15}:     5 bad (5 invalid)
    and, more than 4 sigma = 120 px from both glow centres of a pair, the filtered run's vectors lie within 0.0149 px of
    the clean run's (the filter also removes the frames' constant offset, which moves sub-pixel fits by that much).
    Asserted with half the measured differences as margins: the filtered run has at least 98 bad vectors fewer than the
    unfiltered run and at least 94 fewer than the run with the minimum background; away from the glow it stays within
    0.0149 + 0.001 px of the clean run (the oracle's figure plus a thousand times the 1e-6 px between device and oracle).
    The device's own figures: 201 / 193 / 5 bad vectors and 0.0149 px."""
    from torchpiv_amd import backend, engine
    A, B, Ag, Bg, centres = _glow_scene()
    x, y = backend.get_coordinates((GH, GW), 16, 8)
    plan = engine.Plan(GH, GW, 32, 16, n_pass=2, mode="CWS", max_batch=GN, device="cuda:0", precision="exact")

    def run(a, b):
        u, v, inv = plan.run(a, b)
        torch.cuda.synchronize()
        u, v, inv = u.cpu().numpy(), v.cpu().numpy(), inv.cpu().numpy()
        return [(u[i], v[i], inv[i]) for i in range(GN)]
    Ad, Bd = Ag.cuda(), Bg.cuda()
    clean = run(A.cuda(), B.cuda())
    none = _glow_stats(run(Ad, Bd), clean, x, y, centres)
    bgmin = _glow_stats(run(eng.subtract_background(Ad, Ad.amin(0)), eng.subtract_background(Bd, Bd.amin(0))),
                        clean, x, y, centres)
    filt = _glow_stats(run(eng.prefilter(Ad, "min", 15), eng.prefilter(Bd, "min", 15)), clean, x, y, centres)
    plan.close()
    print(f"bad vectors of {GN * x.size}: no filter {none[0]}, background 'min' {bgmin[0]}, min filter 15 {filt[0]}; "
          f"largest distance from the clean run away from the glow: {none[1]:.4f} / {bgmin[1]:.4f} / {filt[1]:.4f} px")
    assert none[0] - filt[0] >= 98 and bgmin[0] - filt[0] >= 94
    assert filt[1] < 0.0149 + 1e-3
