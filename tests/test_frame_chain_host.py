"""The ownership rule of the frame chain, without a GPU: OfflinePIV._filtered (background and pre-filter) and _finished
(equalize, then mask pixels) on CPU tensors, with the four engine calls replaced by stand-ins that apply the numpy models
and honour out; _scratch, the one reuse-if-big-enough rule of the reused frame buffers; and the prepared frame source over
resident stacks (_frame_batches): its chunks, views and copies.  A step may write in place only into memory the object
made -- never into a caller's tensor."""
import itertools

import numpy as np
import pytest
import torch

import equalize_model as EM
import mask_model as MM
import prefilter_model as PM

N, H, W = 3, 24, 30                             # neither axis a multiple of the equalize tile
PF = {"kind": "mean", "size": 5, "cap": 100}
EQ = {"tile": 8, "clip": 2.0}
CPU = torch.device("cpu")


def _mask():
    m = np.zeros((H, W), np.uint8)
    m[5:15, 8:20], m[7, 9] = 7, 255
    return m


def _into(result, out):
    if out is None:
        return torch.from_numpy(result)
    out.copy_(torch.from_numpy(result))
    return out


@pytest.fixture
def stand_ins(monkeypatch):
    """The engine's four frame steps on CPU tensors through the numpy models, with their signatures; returns the log of
    the calls."""
    from torchpiv_amd import backend
    log = []

    def prefilter(frames, kind, size=None, cap=None, background=None, out=None):
        log.append("prefilter")
        bg = None if background is None else background.numpy()
        return _into(PM.prefilter(frames.numpy(), kind, size, cap, background=bg), out)

    def subtract_background(frames, bg, out=None):
        log.append("subtract_background")
        return _into(np.maximum(frames.numpy(), bg.numpy()) - bg.numpy(), out)

    def equalize(frames, tile=64, clip=3.0, out=None, return_luts=False, work=None):
        log.append("equalize")
        assert not return_luts and work is not None and work.numel() >= frames.shape[0] * 3 * 4 * 256
        return _into(EM.equalize(frames.numpy(), tile, EM.clip_q8_of(clip)), out)

    def apply_mask(frames, mask, out=None):
        log.append("apply_mask")
        return _into(MM.apply(frames.numpy(), mask.numpy()), out)
    for f in (prefilter, subtract_background, equalize, apply_mask):
        monkeypatch.setattr(backend.engine, f.__name__, f)
    return log


def _object(prefilter=None, equalize=None, mask=None):
    from torchpiv_amd import backend, engine, options
    piv = backend.ResidentPIV.__new__(backend.ResidentPIV)
    run = dict(wind_size=32, overlap=16, multipass=1, multipass_mode="CWS", dt=1, scale=1.0, multipass_scale=2.0,
               precision="exact", validation_ratio=1.2, validation_window=3)
    piv._init_state(CPU, range(N), None, run, options.Options(prefilter=engine.prefilter_arg(prefilter),
                                                              equalize=engine.equalize_arg(equalize), mask=engine.mask_arg(mask)))
    return piv


def _frames(seed=0):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (N, H, W), dtype=np.uint8)
    return x, rng.integers(0, 90, (H, W), dtype=np.uint8)


def _aliases(a, b):
    return a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()


@pytest.mark.parametrize("with_bg,with_pf", list(itertools.product((False, True), repeat=2)))
def test_filtered(stand_ins, with_bg, with_pf):
    x_h, bg_h = _frames()
    piv = _object(prefilter=PF if with_pf else None)
    bg = torch.from_numpy(bg_h) if with_bg else None
    if with_pf:
        want, calls = PM.prefilter(x_h, PF["kind"], PF["size"], PF["cap"], background=bg_h if with_bg else None), ["prefilter"]
    elif with_bg:
        want, calls = np.maximum(x_h, bg_h) - bg_h, ["subtract_background"]
    else:
        want, calls = x_h, []
    for out in (None, torch.full((N, H, W), 0xAA, dtype=torch.uint8)):
        x = torch.from_numpy(x_h.copy())
        del stand_ins[:]
        y = piv._filtered(x, bg, out=out)
        assert stand_ins == calls
        assert np.array_equal(y.numpy(), want) and np.array_equal(x.numpy(), x_h)           # the input is never written
        if calls:
            assert not _aliases(y, x) and (out is None or y is out)
        else:
            assert y is x and (out is None or (out == 0xAA).all())


@pytest.mark.parametrize("owned", [False, True])
@pytest.mark.parametrize("with_bg,with_pf,with_eq,with_mask", list(itertools.product((False, True), repeat=4)))
def test_chain_and_ownership(stand_ins, with_bg, with_pf, with_eq, with_mask, owned):
    """_filtered, then _finished, for every on / off combination of the four steps: the models chained; owned=False never
    writes the input and hands out other memory (out where given); owned=True goes in place; nothing on: the input."""
    x_h, bg_h = _frames(1)
    m = _mask()
    piv = _object(prefilter=PF if with_pf else None, equalize=EQ if with_eq else None, mask=m if with_mask else None)
    bg = torch.from_numpy(bg_h) if with_bg else None
    mid = PM.prefilter(x_h, PF["kind"], PF["size"], PF["cap"], background=bg_h if with_bg else None) if with_pf else \
        (np.maximum(x_h, bg_h) - bg_h) if with_bg else x_h
    want = EM.equalize(mid, EQ["tile"], EM.clip_q8_of(EQ["clip"])) if with_eq else mid
    want = MM.apply(want, m) if with_mask else want
    for out in (None, torch.full((N, H, W), 0xAA, dtype=torch.uint8)):
        x = torch.from_numpy(x_h.copy())
        y = piv._filtered(x, bg)
        y_h = y.numpy().copy()
        del stand_ins[:]
        z = piv._finished(y, owned, out=out)
        assert stand_ins == ["equalize"] * with_eq + ["apply_mask"] * with_mask
        assert np.array_equal(z.numpy(), want)
        if y is not x or not owned:
            assert np.array_equal(x.numpy(), x_h)                           # (owned and y is x: x is the object's to write)
        if not (with_eq or with_mask):
            assert z is y
        elif owned:
            assert z is y and _aliases(z, y)                                # in place
        else:
            assert np.array_equal(y.numpy(), y_h) and not _aliases(z, y)    # the input stays, the result is other memory
            assert out is None or z is out
        if out is not None and (owned or not (with_eq or with_mask)):
            assert (out == 0xAA).all()                                      # out is for frames that are not owned only
    assert (piv._eq_work is not None) == with_eq


def test_scratch_reuses_what_is_big_enough():
    piv = _object()
    buf = piv._scratch("_bg_frames", (2, 4), H, W, CPU)
    assert buf is piv._bg_frames and tuple(buf.shape) == (2, 4, H, W) and buf.dtype == torch.uint8
    assert piv._scratch("_bg_frames", (2, 4), H, W, CPU) is buf
    assert piv._scratch("_bg_frames", (2, 3), H, W, CPU) is buf and piv._scratch("_bg_frames", (1, 1), H, W, CPU) is buf
    assert piv._depth_frames is None and piv._pf_frames is None             # one attribute per name
    bigger = piv._scratch("_bg_frames", (2, 5), H, W, CPU)                  # a larger lead
    assert bigger is not buf and bigger is piv._bg_frames and tuple(bigger.shape) == (2, 5, H, W)
    other = piv._scratch("_bg_frames", (2, 5), H, W + 2, CPU)               # another (H, W)
    assert other is not bigger and tuple(other.shape) == (2, 5, H, W + 2)
    assert piv._scratch("_bg_frames", (2, 5), W + 2, H, CPU) is not other
    flat = piv._scratch("_depth_frames", (8,), H, W, CPU)                   # another rank under one name: the file path's
    assert tuple(flat.shape) == (8, H, W) and piv._scratch("_depth_frames", (6,), H, W, CPU) is flat
    quad = piv._scratch("_depth_frames", (2, 4), H, W, CPU)                 # ... and the resident path's
    assert quad is not flat and tuple(quad.shape) == (2, 4, H, W) and piv._depth_frames is quad
    assert tuple(piv._scratch("_depth_frames", (8,), H, W, CPU).shape) == (8, H, W)
    meta = piv._scratch("_pf_frames", (4,), H, W, torch.device("meta"))     # another device
    assert piv._scratch("_pf_frames", (4,), H, W, torch.device("meta")) is meta
    assert piv._scratch("_pf_frames", (4,), H, W, CPU) is not meta and piv._pf_frames.device == CPU


# --------------------------------------------------------------------------------------------------------------------
# the prepared frame source over resident stacks (ResidentPIV._raw_batches under OfflinePIV._frame_batches)
# --------------------------------------------------------------------------------------------------------------------
RAGGED, GATHERED = ([0, 1, 2], [[0, 1], [2]]), ([2, 0, 1], [[2, 0], [1]])          # (idx, its chunks at batch size 2)


def _resident(seed, background=None, **steps):
    """A ResidentPIV over N random CPU pairs (and the pairs as numpy); background: a pair of images, as given by a caller."""
    rng = np.random.default_rng(seed)
    A_h, B_h = (rng.integers(0, 256, (N, H, W), dtype=np.uint8) for _ in range(2))
    piv = _object(**steps)
    piv._A, piv._B = torch.from_numpy(A_h.copy()), torch.from_numpy(B_h.copy())
    if background is not None:
        piv._bg_arg = tuple(torch.from_numpy(b_) for b_ in background)
    return piv, A_h, B_h


@pytest.mark.parametrize("idx,chunks", [RAGGED, GATHERED], ids=["ragged", "gathered"])
def test_resident_frame_batches_plain(stand_ins, idx, chunks):
    """No step on: the chunks idx[s:s + 2] with their ids, every pair staged, no masks, no step launched; a run of
    consecutive pairs is a view of the caller's stacks, anything else a gathered copy."""
    piv, A_h, B_h = _resident(2)
    got = list(piv._frame_batches(idx, 2, H, W, idx[0]))
    assert [raw.chunk for raw, _, _, _ in got] == chunks and stand_ins == []
    assert [raw.last for raw, _, _, _ in got] == [False, True]
    for raw, fa, fb, masks in got:
        c = raw.chunk
        assert raw.order == [(i, True) for i in c] and masks is None and raw.stack is None
        assert fa is raw.A and fb is raw.B and (raw.bg_a, raw.bg_b) == (None, None)
        assert np.array_equal(fa.numpy(), A_h[c]) and np.array_equal(fb.numpy(), B_h[c])
        consecutive = c == list(range(c[0], c[0] + len(c)))
        assert raw.owned == (not consecutive)
        assert _aliases(fa, piv._A) == consecutive and _aliases(fb, piv._B) == consecutive
        if consecutive:
            assert fa.data_ptr() == piv._A[c[0]].data_ptr() and fb.data_ptr() == piv._B[c[0]].data_ptr()
    assert piv._bg_frames is None and piv._depth_frames is None and piv._dw_frames is None


@pytest.mark.parametrize("idx,chunks", [RAGGED, GATHERED], ids=["ragged", "gathered"])
@pytest.mark.parametrize("with_bg,with_pf,with_eq,with_mask",
                         [c for c in itertools.product((False, True), repeat=4) if any(c)])
def test_resident_frame_batches_steps(stand_ins, with_bg, with_pf, with_eq, with_mask, idx, chunks):
    """Any step on: every batch equals the model chain of its pairs (frame a minus bg_a, frame b minus bg_b), in memory
    that is not the caller's, and the caller's stacks are never written."""
    rng = np.random.default_rng(5)
    bgs = tuple(rng.integers(0, 90, (H, W), dtype=np.uint8) for _ in range(2)) if with_bg else None
    m = _mask()
    piv, A_h, B_h = _resident(3, background=bgs, prefilter=PF if with_pf else None, equalize=EQ if with_eq else None,
                              mask=m if with_mask else None)
    want = []
    for f, bg in ((A_h, bgs[0] if with_bg else None), (B_h, bgs[1] if with_bg else None)):
        f = PM.prefilter(f, PF["kind"], PF["size"], PF["cap"], background=bg) if with_pf else \
            (np.maximum(f, bg) - bg) if with_bg else f
        f = EM.equalize(f, EQ["tile"], EM.clip_q8_of(EQ["clip"])) if with_eq else f
        want.append(MM.apply(f, m) if with_mask else f)
    seen = []
    for raw, fa, fb, masks in piv._frame_batches(idx, 2, H, W, idx[0]):       # (the buffers are reused: compare batch by batch)
        c = raw.chunk
        seen.append(c)
        assert masks is None and tuple(fa.shape) == tuple(fb.shape) == (len(c), H, W)
        assert np.array_equal(fa.numpy(), want[0][c]) and np.array_equal(fb.numpy(), want[1][c]), c
        assert not _aliases(fa, piv._A) and not _aliases(fb, piv._B)
        assert np.array_equal(piv._A.numpy(), A_h) and np.array_equal(piv._B.numpy(), B_h)
    assert seen == chunks
    per_stack = [k for k, on in (("prefilter", with_pf), ("subtract_background", with_bg and not with_pf),
                                 ("equalize", with_eq), ("apply_mask", with_mask)) if on]
    assert sorted(stand_ins) == sorted(per_stack * 2 * len(chunks))              # one launch per step, stack and batch
    assert tuple(piv._bg_frames.shape) == (2, 2, H, W)
