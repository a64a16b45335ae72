"""Geometric rectification on the device: engine.dewarp (tpiv_dewarp) against the numpy model of tests/dewarp_model.py bit
for bit -- shapes that reach the 4-byte and the byte form, frame counts on both sides of the kernel's frame chunk, both
interpolations, the offsets form, the refusals --, the frames that enter the passes on every path with dewarp= in the
chain, and a keystone scene whose uniform flow only the rectified run recovers."""
import numpy as np
import pytest
import torch

import depth_model as DM
import dewarp_model as M
import equalize_model as EM
import mask_model as MM
import prefilter_model as PM

pytestmark = pytest.mark.gpu

# (72, 90): rows of 90 bytes, W % 4 != 0 and rows that are not 4-byte aligned; (33, 67): odd both ways; (9, 3): W below one
# lane's four pixels; (16, 24): W % 4 == 0, the 4-byte form
SHAPES = [(72, 90), (33, 67), (9, 3), (16, 24)]
N_MAX = 9                                   # the kernel walks the frames in chunks of 8 (DEWARP_FRAME_CHUNK): 9 crosses it
COUNTS = (1, 3, 5, N_MAX)
MAPS = ["identity", "half_pixel", "rotation_perspective", "quarter_turn", "random"]


def _coords(name, H, W):
    x, y = M.grid(H, W)
    if name == "identity":
        return x, y
    if name == "half_pixel":
        return x + 0.5, y + 0.5
    if name == "rotation_perspective":
        return M.homography_coords(M.rotation_perspective(H, W), H, W)
    if name == "quarter_turn":              # neighbouring pixels of a row read a column: lanes far apart in memory
        cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
        return cx + (y - cy), cy - (x - cx)
    rng = np.random.default_rng(H * 1000 + W)
    xs, ys = rng.uniform(-1.5, W + 0.5, (H, W)), rng.uniform(-1.5, H + 0.5, (H, W))
    xs[:, W - 1], ys[H - 1, :] = W - 2 + 255 / 256, H - 2 + 255 / 256      # the last tap pair, and cubic's tap beyond it
    xs[0, 0], ys[0, 0] = 0.0, 0.0
    xs[0, 1], ys[0, 1] = W - 1, rng.uniform(0, H - 1)
    xs[1, 0], ys[1, 0] = W - 1, H - 1
    xs[1, 1], ys[1, 1] = np.nan, 1.0
    xs[2, 0], ys[2, 0] = W - 1 + 0.01, 0.0                                  # just outside
    return xs, ys


def _frames(H, W):
    """uint8 [N_MAX, H, W]: noise with 0 and 255 samples, the 0 / 255 checkerboard second."""
    rng = np.random.default_rng(H + W)
    f = rng.integers(0, 256, (N_MAX, H, W)).astype(np.uint8)
    f[:, 0, 0], f[:, -1, -1] = 0, 255
    f[1] = M.scene(H, W)[1]
    return f


_CASES = {}


def _case(shape, name):
    """(frames, map, {(interp, fill): model output of all N_MAX frames}) per shape and map, computed once, read-only."""
    key = (shape, name)
    if key not in _CASES:
        H, W = shape
        f, m = _frames(H, W), M.quantize(*_coords(name, H, W), H, W)
        want = {(i, fill): M.dewarp(f, m, i, fill) for i in ("linear", "cubic") for fill in (0, 9)}
        for a in (f, m, *want.values()):
            a.flags.writeable = False
        _CASES[key] = (f, m, want)
    return _CASES[key]


def test_the_maps_reach_their_branches():
    m = _case((72, 90), "rotation_perspective")[1]
    rows, cols = np.nonzero(M.outside(m))
    assert rows.min() == 0 and rows.max() == 71 and cols.min() == 0 and cols.max() == 89
    for shape in SHAPES:
        H, W = shape
        m = _case(shape, "random")[1]
        out = M.outside(m)
        assert out.any() and not out.all() and out[1, 1] and out[2, 0]
        assert tuple(m[0, 0]) == (0, 0) and m[0, 1, 0] == (W - 1) * 256 and tuple(m[1, 0]) == ((W - 1) * 256, (H - 1) * 256)
        assert (m[:, W - 1, 0][~out[:, W - 1]] & 255 == 255).all() and (m[H - 1, :, 1][~out[H - 1, :]] & 255 == 255).all()
        f, _, want = _case(shape, "half_pixel")
        assert not np.array_equal(want[("linear", 0)], want[("cubic", 0)])


@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("name", MAPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_dewarp_equals_the_model(shape, name, interp):
    from torchpiv_amd import engine
    H, W = shape
    f, m, want = _case(shape, name)
    fd = torch.from_numpy(f.copy()).cuda()
    md = engine.dewarp_upload(m, fd.device)
    for fill in (0, 9):
        for n in COUNTS:
            got = engine.dewarp(fd[:n], md, interp, fill)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (n, H, W)
            got = got.cpu().numpy()
            ref = want[(interp, fill)][:n]
            assert np.array_equal(got, ref), (n, fill, int((got != ref).sum()), np.argwhere(got != ref)[:5])
    one = engine.dewarp(fd[2], md, interp, 9)                               # [H, W] in, [H, W] out
    assert tuple(one.shape) == (H, W) and np.array_equal(one.cpu().numpy(), want[(interp, 9)][2])
    assert np.array_equal(fd.cpu().numpy(), f)                              # the source is not written


@pytest.mark.parametrize("shape", [(72, 90), (16, 24)])
def test_offsets_form(shape):
    """Frames addressed out of order and twice from a flat buffer, at offsets that are no multiple of four."""
    from torchpiv_amd import engine
    H, W = shape
    f, m, want = _case(shape, "rotation_perspective")
    lead = 3
    flat = np.concatenate([np.full(lead, 99, np.uint8), f.ravel()])
    order = [4, 0, 4, 8, 1, 7, 7, 2, 3, 5]                                  # ten: more than one frame chunk
    off = np.array([lead + k * H * W for k in order], dtype=np.int64)
    fd = torch.from_numpy(flat).cuda()
    md = engine.dewarp_upload(m, fd.device)
    for interp in ("linear", "cubic"):
        ref = want[(interp, 9)][order]
        assert np.array_equal(M.dewarp_offsets(flat, off, H, W, m, interp, 9), ref)
        for offsets in (off, off.tolist(), torch.from_numpy(off), torch.from_numpy(off).cuda()):
            got = engine.dewarp(fd, md, interp, 9, offsets=offsets, shape=(H, W))
            assert np.array_equal(got.cpu().numpy(), ref)
    assert np.array_equal(fd.cpu().numpy(), flat)
    for bad in ([-1], [flat.size - H * W + 1]):
        with pytest.raises(ValueError, match="leaves the buffer"):
            engine.dewarp(fd, md, offsets=bad, shape=(H, W))
    with pytest.raises(ValueError):
        engine.dewarp(fd, md, offsets=off)                                  # no shape
    with pytest.raises(ValueError):
        engine.dewarp(fd[lead:].view(N_MAX, H, W), md, shape=(H, W))        # shape without offsets


def test_refusals_launch_nothing():
    from torchpiv_amd import engine
    H, W = 9, 3
    f, m, want = _case((H, W), "half_pixel")
    fd = torch.from_numpy(f.copy()).cuda()
    md = engine.dewarp_upload(m, fd.device)
    keep = torch.full((N_MAX, H, W), 77, dtype=torch.uint8, device="cuda")

    def refused(*args, **kw):
        with pytest.raises(ValueError):
            engine.dewarp(*args, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(fd.cpu().numpy(), f) and bool((keep == 77).all())

    # out overlaps the source: itself, and a shifted view of the same memory
    big = torch.empty(2 * N_MAX * H * W, dtype=torch.uint8, device="cuda")
    src = big[:N_MAX * H * W].view(N_MAX, H, W).copy_(fd)
    refused(src, md, out=src)
    refused(src, md, out=big[H * W:(N_MAX + 1) * H * W].view(N_MAX, H, W))
    assert np.array_equal(src.cpu().numpy(), f)
    # out overlaps the map, out overlaps the table
    refused(fd[:8], md, out=md.view(torch.uint8).view(-1)[:8 * H * W].view(8, H, W))
    assert np.array_equal(md.cpu().numpy(), m)
    table = engine._dewarp_table(fd.device)
    refused(fd, md, out=table.view(torch.uint8).view(-1)[100:100 + N_MAX * H * W].view(N_MAX, H, W))
    assert np.array_equal(table.cpu().numpy(), M.cubic_table())
    # the map: another device, illegal entries (checked on the host, once per tensor and version), dtype, shape
    refused(fd, torch.from_numpy(m.copy()), out=keep)
    for entry in ((5, (H - 1) * 256 + 1), ((W - 1) * 256 + 1, 0), (-1, 5), (-7, -7), (2 ** 31 - 1, 0)):
        bad = m.copy()
        bad[4, 1] = entry
        refused(fd, torch.from_numpy(bad).cuda(), out=keep)
        with pytest.raises(ValueError, match="illegal map entry"):
            engine.dewarp_upload(bad, "cuda")
    written = md.clone()
    assert np.array_equal(engine.dewarp(fd, written, "linear").cpu().numpy(), want[("linear", 0)])      # checked here ...
    written[4, 1, 0] = -5                                                   # ... and again after a write
    refused(fd, written, out=keep)
    refused(fd, md.to(torch.int64), out=keep)
    refused(fd, md[:-1], out=keep)
    # the frames and out: dtype, shape, fill, interp
    refused(fd.to(torch.int16), md, out=keep)
    refused(fd, md, out=keep[:-1])
    refused(fd, md, out=keep.to(torch.int32))
    refused(fd, md, "nearest", out=keep)
    refused(fd, md, "cubic", 256, out=keep)
    assert np.array_equal(engine.dewarp(fd, md, out=keep).cpu().numpy(), want[("cubic", 0)])          # and the good call writes


# ---------------------------------------------------------------------------------------------------------------------
# the frames that enter the passes
# ---------------------------------------------------------------------------------------------------------------------
H, W, N = 72, 90, 4
WS, OV = 32, 16
R16 = {"lo": 0, "hi": 4080}                     # v = 16 g -> g exactly
EQ = {"tile": 16, "clip": 2.0}
PF = {"kind": "mean", "size": 7, "cap": 120}
HM = M.rotation_perspective(H, W, degrees=3.0, px=2e-4, py=-1e-4)
DW = {"homography": HM, "fill": 5}
DWL = {"homography": HM, "interp": "linear"}


def _mask():
    m = np.zeros((H, W), np.uint8)
    m[20:50, 30:74] = 7
    m[30:40, 40:60] = 255
    return m


MASK = _mask()
SETS = {
    "dewarp": {"dewarp": DW},
    "depth+dewarp": {"depth": R16, "dewarp": DWL},
    "dewarp+background+prefilter+equalize+mask": {"dewarp": DW, "background": "min", "prefilter": PF, "equalize": EQ,
                                                  "mask": MASK},
}
PATHS = ["resident", "resident_gathered", "files", "one_pair"]


@pytest.fixture(scope="module")
def frames():
    """Four wavy pairs over a static texture, with a 0 and a 255 sample, as uint8 numpy stacks [N, H, W] and the same as
    12-bit samples (16 x, uint16)."""
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
    bmp, png = tmp_path_factory.mktemp("dewarp_bmp"), tmp_path_factory.mktemp("dewarp_png")
    for i in range(N):
        Image.fromarray(A[i], "L").save(bmp / f"image{i}_a.bmp")
        Image.fromarray(B[i], "L").save(bmp / f"image{i}_b.bmp")
        Image.fromarray(A16[i]).save(png / f"image{i}_a.png")
        Image.fromarray(B16[i]).save(png / f"image{i}_b.png")
    return str(bmp), str(png)


_EXPECTED = {}


def _expected(name, frames):
    """(a, b): the frames of all N pairs after the chain of option set `name` -- tone map, dewarp, background, pre-filter
    and cap, equalize, mask -- from the numpy models alone; computed once per set and shared by the paths (read-only)."""
    if name not in _EXPECTED:
        opts = SETS[name]
        A, B, A16, B16 = frames
        dw = opts["dewarp"]
        m = M.quantize(*M.homography_coords(dw["homography"], H, W), H, W)
        out = []
        for f8, f16 in ((A, A16), (B, B16)):
            f = DM.map_(f16, DM.lut(R16["lo"], R16["hi"])) if "depth" in opts else f8
            f = M.dewarp(f, m, dw.get("interp", "cubic"), dw.get("fill", 0))
            bg = f.min(axis=0) if "background" in opts else None        # "min": over the rectified frames of every pair
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


def test_the_chain_of_models_depends_on_the_order(frames):
    """The rectified frames differ from the raw ones, carry the fill value, and a background taken before the
    rectification would give other frames: an expectation with the step missing or misplaced would differ."""
    A = frames[0]
    m = M.quantize(*M.homography_coords(HM, H, W), H, W)
    got = _expected("dewarp", frames)[0]
    assert M.outside(m).any() and (got[:, M.outside(m)] == 5).all() and not np.array_equal(got, A)
    late = M.dewarp(np.maximum(A, A.min(axis=0)) - A.min(axis=0), m, "cubic", 5)
    early = got - got.min(axis=0)
    assert not np.array_equal(late, early)


@pytest.fixture
def launches(monkeypatch):
    """[(data_ptr of a, clone of a, clone of b)] of every engine.Plan.run from here on."""
    from torchpiv_amd import engine
    seen = []
    run = engine.Plan.run

    def capture(self, a, b, *args, **kw):
        seen.append((a.data_ptr(), a.clone(), b.clone()))
        return run(self, a, b, *args, **kw)
    monkeypatch.setattr(engine.Plan, "run", capture)
    return seen


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(SETS))
def test_frames_that_enter_the_passes(frames, folders, launches, name, path):
    import torchpiv_amd as T
    opts = SETS[name]
    deep = "depth" in opts
    want_a, want_b = _expected(name, frames)
    kw = dict(multipass=1, **opts)
    keep = None
    if path.startswith("resident"):
        src = frames[2:] if deep else frames[:2]
        Ad, Bd = (torch.from_numpy(f).cuda() for f in src)
        bits = (lambda t: t.view(torch.int16)) if deep else (lambda t: t)
        keep = bits(Ad).clone(), bits(Bd).clone()
        piv = T.ResidentPIV(Ad, Bd, WS, OV, **kw)
        if path == "resident":
            list(piv.batched(3))
            chunks = [[0, 1, 2], [3]]
        else:
            list(piv.batched(2, indices=[3, 0, 2]))
            chunks = [[3, 0], [2]]
    else:
        piv = T.OfflinePIV(folders[1] if deep else folders[0], "cuda:0", "png" if deep else "bmp", WS, OV, **kw)
        if path == "files":
            list(piv.batched(3))
            chunks = [[0, 1, 2], [3]]
        else:
            piv.call_batch = 1
            list(piv())
            chunks = [[0], [1], [2], [3]]
    torch.cuda.synchronize()
    assert len(launches) == len(chunks), (len(launches), chunks)
    for k, (chunk, (_, a, b)) in enumerate(zip(chunks, launches)):
        a, b = a.cpu().numpy().reshape(-1, H, W), b.cpu().numpy().reshape(-1, H, W)
        assert a.dtype == np.uint8 and a.shape == b.shape == (len(chunk), H, W), (k, a.shape, b.shape)
        for got, want, which in ((a, want_a[chunk], "a"), (b, want_b[chunk], "b")):
            assert np.array_equal(got, want), (k, chunk, which, int((got != want).sum()), np.argwhere(got != want)[:5])
    if keep is not None:
        assert torch.equal(bits(Ad), keep[0]) and torch.equal(bits(Bd), keep[1])           # the caller's frames stay
    assert piv._dw_frames is not None and piv._dw_map is not None
    m = M.quantize(*M.homography_coords(HM, H, W), H, W)
    assert np.array_equal(piv._dw_map.cpu().numpy(), m) and np.array_equal(piv.dewarp_outside(), M.outside(m))
    piv.close()


def test_without_the_keyword_nothing_of_it_exists(frames, folders, launches):
    """No buffer, no map, and the consecutive resident path still hands out views of the caller's frames."""
    import torchpiv_amd as T
    Ad, Bd = (torch.from_numpy(f).cuda() for f in frames[:2])
    piv = T.ResidentPIV(Ad, Bd, WS, OV)
    list(piv.batched(3))
    assert piv._dw_frames is None and piv._dw_map is None and piv.dewarp_outside() is None
    assert launches[0][0] == Ad.data_ptr()
    piv.close()
    piv = T.OfflinePIV(folders[0], "cuda:0", "bmp", WS, OV)
    list(piv.batched(3))
    assert piv._dw_frames is None and piv._dw_map is None
    piv.close()


def test_a_map_of_another_shape_raises_where_a_mask_does(frames):
    import torchpiv_amd as T
    Ad, Bd = (torch.from_numpy(f).cuda() for f in frames[:2])
    with pytest.raises(ValueError, match="shape"):
        T.ResidentPIV(Ad, Bd, WS, OV, dewarp={"map": M.grid(H, W + 2)})


def test_runner_passes_dewarp(tmp_path):
    """run_folder(..., dewarp=) delivers the generator's fields.  128 x 160 pairs of synth's wavy flow, noisy and sparse
    enough that both passes leave a few invalid vectors (a pair without any is dropped by the reference's
    post-validation), so that every pair is kept, rectified or not."""
    import torchpiv_amd as T
    from PIL import Image
    from torchpiv_amd import runner, synth
    h, w = 128, 160
    for i in range(4):
        a, b = synth.make_pair(h, w, 40 + i, kind="wavy", noise=6.0, density=0.015)
        Image.fromarray(a.numpy(), "L").save(tmp_path / f"image{i}_a.bmp")
        Image.fromarray(b.numpy(), "L").save(tmp_path / f"image{i}_b.bmp")
    dw = {"homography": M.rotation_perspective(h, w, degrees=3.0, px=2e-4, py=-1e-4), "fill": 5}
    piv = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", WS, OV, multipass=2, dewarp=dw)
    want = {i: (u, v) for i, _, _, u, v in piv.batched(3)}
    piv.close()
    plain = T.OfflinePIV(str(tmp_path), "cuda:0", "bmp", WS, OV, multipass=2)
    other = {i: (u, v) for i, _, _, u, v in plain.batched(3)}
    plain.close()
    seen = {}
    runner.run_folder(str(tmp_path), "cuda:0", "bmp", WS, OV, multipass=2, dewarp=dw, batch_size=3,
                      on_pair=lambda i, out: seen.__setitem__(i, (out["Vx[m/s]"], out["Vy[m/s]"])))
    assert sorted(want) == [0, 1, 2, 3] == sorted(seen) == sorted(other)
    for i in want:
        assert np.array_equal(seen[i][0], want[i][0], equal_nan=True) and np.array_equal(seen[i][1], want[i][1], equal_nan=True)
        assert not np.array_equal(other[i][0], want[i][0], equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------------
# the physical check: a uniform flow seen through a keystone
# ---------------------------------------------------------------------------------------------------------------------
PH, PW = 128, 160
FLOW = (3.25, -1.5)                     # px in the rectified (world) frame, x and y (rows grow downwards)
# RMS error of the rectified run over the 48 windows inside the source, measured on one MI355X (profiles/dewarp/measurements.json):
# 0.1353 px, against 0.4102 px as recorded.  The CPU oracle on the numpy model's frames gives the same 0.1353 px, and 0.1339 and
# 0.1430 px for two other seeds: the spread is far inside the factor two of the assertion.
RMS_MEASURED = 0.1353


def keystone(H=PH, W=PW):
    """3 x 3, rectified pixel -> camera pixel: about the frame centre, x' = s xc / (1 + k xc), y' = s yc / (1 + k xc) with
    the magnification s / (1 + k xc) running from 1.1 at the left edge to 0.9 at the right one."""
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    k, s = 0.2 / (W - 1), 0.99
    T0 = np.array([[1, 0, -cx], [0, 1, -cy], [0, 0, 1.0]])
    K = np.array([[s, 0, 0], [0, s, 0], [k, 0, 1.0]])
    T1 = np.array([[1, 0, cx], [0, 1, cy], [0, 0, 1.0]])
    return T1 @ K @ T0


def _through(G, x, y):
    d = G[2, 0] * x + G[2, 1] * y + G[2, 2]
    return (G[0, 0] * x + G[0, 1] * y + G[0, 2]) / d, (G[1, 0] * x + G[1, 1] * y + G[1, 2]) / d


def _render(px, py, amp, H, W, sigma=1.0):
    img = np.zeros((H, W))
    cx, cy = np.rint(px).astype(int), np.rint(py).astype(int)
    for oy in range(-3, 4):
        for ox in range(-3, 4):
            xx, yy = cx + ox, cy + oy
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            w = amp * np.exp(-((xx - px) ** 2 + (yy - py) ** 2) / (2 * sigma * sigma))
            np.add.at(img, (yy[ok], xx[ok]), w[ok])
    return np.clip(np.rint(img + 8.0), 0, 255).astype(np.uint8)


def keystone_pair(seed=0):
    """(a, b, particles in frame a) -- uint8 [PH, PW] as the camera sees them: about 1000 Gaussian particles in the frame,
    at G(X) in frame a and at G(X + FLOW) in frame b, X uniform over a world region that covers the camera's field."""
    rng = np.random.default_rng(seed)
    G = keystone()
    n = 1780                                                    # over 200 x 178 world px: 0.05 per px, ~1000 in the frame
    X, Y = rng.uniform(-15, 185, n), rng.uniform(-25, 153, n)
    amp = rng.uniform(100, 200, n)
    xa, ya = _through(G, X, Y)
    a = _render(xa, ya, amp, PH, PW)
    b = _render(*_through(G, X + FLOW[0], Y + FLOW[1]), amp, PH, PW)
    return a, b, int(((xa >= 0) & (xa <= PW - 1) & (ya >= 0) & (ya <= PH - 1)).sum())


@pytest.fixture
def fields(monkeypatch):
    """[(u, v, invalid)] as numpy arrays of every engine.Plan.run from here on: the raw fields of a pass, before the
    post-validation decides about the pair."""
    from torchpiv_amd import engine
    seen = []
    run = engine.Plan.run

    def capture(self, a, b, *args, **kw):
        out = run(self, a, b, *args, **kw)
        seen.append(tuple(t.cpu().numpy().copy() for t in out[:3]))
        return out
    monkeypatch.setattr(engine.Plan, "run", capture)
    return seen


def test_keystone_flow_is_recovered(fields):
    """A uniform flow of FLOW px seen through a keystone of +-10 % magnification, 32/16, one pass.  As recorded, the
    field is off by more than 0.2 px at the outer columns of the grid: there the x magnification is 0.99 / 0.92^2 = 1.17
    and 0.99 / 1.08^2 = 0.85, i.e. 3.25 px come out as 3.80 and 2.76.  Rectified with the keystone as the backward map, the
    RMS error over the windows that lie inside the source is below half of the uncorrected one and within twice
    RMS_MEASURED.  The truth is the constructed flow, never another run of the library."""
    import torchpiv_amd as T
    a, b, count = keystone_pair()
    assert 900 < count < 1100
    Ad, Bd = torch.from_numpy(a)[None].cuda(), torch.from_numpy(b)[None].cuda()
    G = keystone()
    piv = T.ResidentPIV(Ad, Bd, WS, OV, multipass=1)
    list(piv.batched(1))
    piv.close()
    piv = T.ResidentPIV(Ad, Bd, WS, OV, multipass=1, dewarp={"homography": G})
    list(piv.batched(1))
    outside = piv.dewarp_outside()
    piv.close()
    assert len(fields) == 2
    (u0, v0, i0), (u1, v1, i1) = ((f[0] for f in run) for run in fields)
    nr, nc = u0.shape
    assert (nr, nc) == (7, 9)
    # the windows whose 32 x 32 pixels all have a source in the camera frame
    inside = np.array([[not outside[i * 16:i * 16 + 32, j * 16:j * 16 + 32].any() for j in range(nc)] for i in range(nr)])
    assert outside.any() and 40 <= inside.sum() < nr * nc
    e0 = np.hypot(u0 - FLOW[0], v0 - FLOW[1])
    e1 = np.hypot(u1 - FLOW[0], v1 - FLOW[1])
    rms0 = float(np.sqrt((e0[inside] ** 2).mean()))
    rms1 = float(np.sqrt((e1[inside] ** 2).mean()))
    print(f"keystone: RMS error as recorded {rms0:.4f} px, rectified {rms1:.4f} px over {int(inside.sum())} windows; "
          f"outer columns as recorded {e0[:, 0].min():.3f} .. {e0[:, 0].max():.3f} and {e0[:, -1].min():.3f} .. "
          f"{e0[:, -1].max():.3f} px; invalid {int(i0.sum())} / {int(i1[inside].sum())}")
    assert (e0[:, 0] > 0.2).all() and (e0[:, -1] > 0.2).all()
    assert rms1 < 0.5 * rms0
    assert rms1 <= 2 * RMS_MEASURED
