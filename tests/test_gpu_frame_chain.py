"""What enters the passes: the frames every path hands to engine.Plan.run -- ResidentPIV.batched over consecutive and over
gathered pairs, OfflinePIV.batched over files and the one-pair loop, tracks() of both classes -- and to
engine.Plan.ensemble_add (ensemble() of both classes), against the numpy models of the frame chain in chain
order (tone map, background, pre-filter and cap, equalize, mask pixels), bit for bit, for every combination of steps that
is a branch of its own in the backend.  The expectation comes from the models alone, never from a run of the library with
the steps off.  Also pinned: the caller's resident frames are never written, the plain consecutive resident path hands out
views of them, the reused buffers exist exactly when a path needs them, compute_background() of both classes is the
models' minimum, and the file path launches each step once per batch over both stacks."""
import numpy as np
import pytest
import torch

import depth_model as DM
import equalize_model as EM
import mask_model as MM
import prefilter_model as PM

pytestmark = pytest.mark.gpu

# 72 x 90: BMP rows are padded to 92 bytes, and neither axis is a multiple of the equalize tile
H, W, N = 72, 90, 4
WS, OV = 32, 16
R16 = {"lo": 0, "hi": 4080}                     # v = 16 g -> g exactly (tests/test_gpu_depth.py)
EQ = {"tile": 16, "clip": 2.0}
PF = {"kind": "mean", "size": 7, "cap": 120}


def _mask():
    """A block of 30 x 44 = 1320 of the 6480 pixels (a fifth), with bytes 1, 7 and 255."""
    m = np.zeros((H, W), np.uint8)
    m[20:50, 30:74] = 7
    m[30:40, 40:60] = 255
    m[20, 30:74] = 1
    return m


MASK = _mask()
SETS = {
    "plain": {},
    "equalize": {"equalize": EQ},
    "mask": {"mask": MASK},
    "background": {"background": "min"},
    "prefilter+equalize+mask": {"prefilter": PF, "equalize": EQ, "mask": MASK},
    "background+prefilter+equalize+mask": {"background": "min", "prefilter": PF, "equalize": EQ, "mask": MASK},
    "depth": {"depth": R16},
    "depth+background": {"depth": R16, "background": "min"},
    "depth+background+prefilter+equalize+mask": {"depth": R16, "background": "min", "prefilter": PF, "equalize": EQ,
                                                 "mask": MASK},
}
PATHS = ["resident", "resident_gathered", "files", "one_pair",
         "resident_ensemble", "files_ensemble", "resident_tracks", "files_tracks"]
LEVEL = 60                                      # tracks(): any level does, the frames are captured in front of the detection


@pytest.fixture(scope="module")
def frames():
    """Four wavy pairs over a static texture (so that the minimum over the pairs is no flat image), with a 0 and a 255
    sample, as uint8 numpy stacks [N, H, W] and the same as 12-bit samples (16 x, uint16)."""
    from torchpiv_amd import synth
    A, B = synth.make_batch(N, H, W, kind="wavy", noise=3.0)
    tex = torch.from_numpy(np.random.default_rng(11).integers(0, 48, (H, W)).astype(np.uint8))
    A, B = torch.maximum(A, tex).numpy().copy(), torch.maximum(B, tex).numpy().copy()
    A[0, 0, 0], A[0, 0, 1] = 0, 255
    return A, B, (A.astype(np.uint16) * 16), (B.astype(np.uint16) * 16)


@pytest.fixture(scope="module")
def folders(tmp_path_factory, frames):
    """The pairs as 8-bit BMP files and as 16-bit PNG files."""
    from PIL import Image
    A, B, A16, B16 = frames
    bmp, png = tmp_path_factory.mktemp("chain_bmp"), tmp_path_factory.mktemp("chain_png")
    for i in range(N):
        Image.fromarray(A[i], "L").save(bmp / f"image{i}_a.bmp")
        Image.fromarray(B[i], "L").save(bmp / f"image{i}_b.bmp")
        Image.fromarray(A16[i]).save(png / f"image{i}_a.png")
        Image.fromarray(B16[i]).save(png / f"image{i}_b.png")
    assert (bmp / "image0_a.bmp").stat().st_size >= 92 * H
    return str(bmp), str(png)


_EXPECTED = {}


def _expected(name, frames):
    """(a, b): the frames of all N pairs after the chain of option set `name`, from the numpy models alone; computed once
    per set and shared by the paths (read-only)."""
    if name not in _EXPECTED:
        opts = SETS[name]
        A, B, A16, B16 = frames
        out = []
        for f8, f16 in ((A, A16), (B, B16)):
            f = DM.map_(f16, DM.lut(R16["lo"], R16["hi"])) if "depth" in opts else f8
            bg = f.min(axis=0) if "background" in opts else None        # background="min": over every pair of the dataset
            if "prefilter" in opts:
                f = PM.prefilter(f, PF["kind"], PF["size"], PF["cap"], background=bg)
            elif bg is not None:
                f = np.maximum(f, bg) - bg
            if "equalize" in opts:
                f = EM.equalize(f, EQ["tile"], EM.clip_q8_of(EQ["clip"]))
            if "mask" in opts:
                f = MM.apply(f, MASK)
            f.flags.writeable = False
            out.append(f)
        _EXPECTED[name] = tuple(out)
    return _EXPECTED[name]


def test_the_models_chain_does_something(frames):
    """Every step of the largest set changes the frames, the tone map of the deep frames gives the uint8 ones, and the
    background is no flat image: an expectation that skipped a step would differ."""
    A, B, A16, B16 = frames
    assert np.array_equal(DM.map_(A16, DM.lut(0, 4080)), A)
    assert len(np.unique(A.min(axis=0))) > 8
    seen = [_expected(k, frames)[0] for k in ("plain", "background", "prefilter+equalize+mask",
                                              "background+prefilter+equalize+mask", "equalize", "mask")]
    for i in range(len(seen)):
        for j in range(i):
            assert not np.array_equal(seen[i], seen[j]), (i, j)
    assert np.array_equal(_expected("depth", frames)[0], seen[0])


@pytest.fixture
def launches(monkeypatch):
    """[(data_ptr of a, clone of a, clone of b)] of every engine.Plan.run and engine.Plan.ensemble_add from here on."""
    from torchpiv_amd import engine
    seen = []
    for name in ("run", "ensemble_add"):
        def capture(self, a, b, *args, _inner=getattr(engine.Plan, name), **kw):
            seen.append((a.data_ptr(), a.clone(), b.clone()))
            return _inner(self, a, b, *args, **kw)
        monkeypatch.setattr(engine.Plan, name, capture)
    return seen


def _allocated(path, opts):
    """The reused buffers that are not None after a run of `path` with `opts`."""
    deep, bg, pf = "depth" in opts, "background" in opts, "prefilter" in opts
    eq, mask = "equalize" in opts, "mask" in opts
    if path.startswith("resident"):
        # the tone map has a buffer of its own that equalize and mask go on in; else they need one for the caller's frames
        want = {"_depth_frames": deep, "_bg_frames": bg or pf or ((eq or mask) and not deep), "_pf_frames": False}
    elif path == "files":
        want = {"_depth_frames": deep, "_bg_frames": False, "_pf_frames": pf}
    else:       # the one-pair loop keeps no frame buffer; "min" over deep files runs the staged tone map once
        want = {"_depth_frames": deep and bg, "_bg_frames": False, "_pf_frames": False}
    want["_eq_work"] = eq
    return want


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(SETS))
def test_frames_that_enter_the_passes(frames, folders, launches, name, path):
    import torchpiv_amd as T
    opts = SETS[name]
    deep = "depth" in opts
    want_a, want_b = _expected(name, frames)
    kw = dict(multipass=1, **opts)
    keep = None
    consume = {"ensemble": lambda piv, **kw: piv.ensemble(**kw),
               "tracks": lambda piv, **kw: list(piv.tracks(LEVEL, **kw))}.get(path.split("_")[-1])
    if path.startswith("resident"):
        src = frames[2:] if deep else frames[:2]
        Ad, Bd = (torch.from_numpy(f).cuda() for f in src)
        bits = (lambda t: t.view(torch.int16)) if deep else (lambda t: t)
        keep = bits(Ad).clone(), bits(Bd).clone()
        piv = T.ResidentPIV(Ad, Bd, WS, OV, **kw)
        if path == "resident":
            list(piv.batched(3))
            chunks = [[0, 1, 2], [3]]                    # idx[s:s + bs]: a ragged last chunk
        elif consume is not None:                        # both in one object: consecutive pairs, then gathered ones
            consume(piv, batch_size=3)
            consume(piv, indices=[3, 0, 2], batch_size=2)
            chunks = [[0, 1, 2], [3], [3, 0], [2]]
        else:
            list(piv.batched(2, indices=[3, 0, 2]))
            chunks = [[3, 0], [2]]
    else:
        piv = T.OfflinePIV(folders[1] if deep else folders[0], "cuda:0", "png" if deep else "bmp", WS, OV, **kw)
        if path == "files":
            list(piv.batched(3))
            chunks = [[0, 1, 2], [3]]
        elif consume is not None:
            consume(piv, batch_size=3)
            chunks = [[0, 1, 2], [3]]
        else:
            piv.call_batch = 1
            list(piv())
            chunks = [[0], [1], [2], [3]]                # dataset order
    torch.cuda.synchronize()
    assert len(launches) == len(chunks), (len(launches), chunks)
    for k, (chunk, (_, a, b)) in enumerate(zip(chunks, launches)):
        a, b = a.cpu().numpy().reshape(-1, H, W), b.cpu().numpy().reshape(-1, H, W)
        assert a.dtype == np.uint8 and a.shape == b.shape == (len(chunk), H, W), (k, a.shape, b.shape)
        for got, want, which in ((a, want_a[chunk], "a"), (b, want_b[chunk], "b")):
            assert np.array_equal(got, want), (k, chunk, which, int((got != want).sum()), np.argwhere(got != want)[:5])
    if keep is not None:
        assert torch.equal(bits(Ad), keep[0]) and torch.equal(bits(Bd), keep[1])           # the caller's frames stay
        if name == "plain" and path == "resident":
            assert launches[0][0] == Ad.data_ptr()                                         # ... and are not copied
    got = {k: getattr(piv, k) is not None for k in ("_depth_frames", "_bg_frames", "_pf_frames", "_eq_work")}
    assert got == _allocated("files" if path.startswith("files") else path, opts)
    piv.close()


@pytest.mark.parametrize("indices", [None, [3, 0, 2]], ids=["all", "indices"])
@pytest.mark.parametrize("deep", [False, True], ids=["uint8", "depth"])
@pytest.mark.parametrize("path", ["resident", "files"])
def test_compute_background_is_the_models_minimum(frames, folders, path, deep, indices):
    """compute_background() folds the raw frame source: the minimum over the pairs asked for of the frames behind the
    tone map (R16 maps the deep frames onto the uint8 ones), two pairs per batch."""
    import torchpiv_amd as T
    pairs = list(range(N)) if indices is None else indices
    want_a, want_b = (f[pairs].min(axis=0) for f in _expected("depth" if deep else "plain", frames))
    kw = dict(multipass=1, depth=R16) if deep else dict(multipass=1)
    if path == "resident":
        Ad, Bd = (torch.from_numpy(f).cuda() for f in (frames[2:] if deep else frames[:2]))
        piv = T.ResidentPIV(Ad, Bd, WS, OV, **kw)
    else:
        piv = T.OfflinePIV(folders[1] if deep else folders[0], "cuda:0", "png" if deep else "bmp", WS, OV, **kw)
    bg_a, bg_b = piv.compute_background(indices=indices, batch_size=2)
    assert bg_a.dtype == torch.uint8 and tuple(bg_a.shape) == tuple(bg_b.shape) == (H, W)
    assert np.array_equal(bg_a.cpu().numpy(), want_a) and np.array_equal(bg_b.cpu().numpy(), want_b)
    piv.close()


@pytest.mark.parametrize("name,per_batch", [("prefilter+equalize+mask", (1, 1, 1)),
                                            ("depth+background+prefilter+equalize+mask", (2, 1, 1))])
def test_file_path_launches_each_step_once_per_batch(frames, folders, monkeypatch, name, per_batch):
    """Over files both stacks of a batch are one tensor: the pre-filter, equalize and the mask pixels run once over it --
    only a background that the unpack could not fuse (here: behind the tone map) makes the filter, which subtracts it,
    run per stack.  Two batches (3 + 1 pairs)."""
    import torchpiv_amd as T
    from torchpiv_amd import engine
    calls = {"prefilter": 0, "equalize": 0, "apply_mask": 0}
    for step in calls:
        def counted(*args, _inner=getattr(engine, step), _step=step, **kw):
            calls[_step] += 1
            return _inner(*args, **kw)
        monkeypatch.setattr(engine, step, counted)
    deep = "depth" in SETS[name]
    piv = T.OfflinePIV(folders[1] if deep else folders[0], "cuda:0", "png" if deep else "bmp", WS, OV, multipass=1, **SETS[name])
    list(piv.batched(3))
    assert calls == {step: 2 * k for step, k in zip(("prefilter", "equalize", "apply_mask"), per_batch)}
    piv.close()
