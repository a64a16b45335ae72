"""The memory contract of every entry point that takes device memory (include/torchpiv_hip.h, "Memory contract"): where a
kernel reads and writes, not what it computes.  No tolerance anywhere: every assertion is bit identity, guard integrity or
a status code.

Every table entry (ENTRIES) is run through tests/guarded.py:
  (a) bounds: inputs placed in an Arena, every tensor the engine allocates taken from it (guarded.patched), the guard bands
      on both sides of every buffer intact afterwards, the outputs bit for bit those of the same call on ordinary tensors;
  (b) stale data and reads out of bounds: the outputs bit-identical under the three (poison, guard) settings -- an output
      cell nobody wrote, a counter or list slot that was expected to hold zeros and a read outside an input that reaches a
      result all make them differ;
  (c) refusals: a work buffer one byte short, or NULL, is TPIV_EINVAL and leaves the outputs' poison and the guards alone.
The work buffer of the correlation seam is exactly tpiv_work_bytes() long with a guard directly behind it, for every
precision and mode: the positive half of that query's contract.

Frames of the seam: tests/handoff_cases.py's geometry and particle pairs (odd window counts, W three pixels past the grid,
batch 2, H * W odd so that pair 1 starts at an odd address: one column more where W is even, and one row more at the odd
window size 15, whose H is even), its planted predictor with +-(ws / 2 + 0.5), +-(W + 9.25) and
an integral value in the corner cells and one cell of every border, so that source rows and columns leave the frame on
every side.  An undefined part of an output is left out by a selector only where the header says so; the line is quoted
beside it."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest
import torch

import guarded
import handoff_cases as HC
from guarded import Arena, SETTINGS
from handoff_model import handoff
from test_gpu_handoff import expected_kernel

pytestmark = pytest.mark.gpu

DEV = "cuda"
MIB = 1 << 20
SEAM_SIZES = HC.SIZES + (44,)                    # + the plain O(n^2) kernel at an even size
PRECISIONS = ("fast", "reference", "f64", "exact")
CALLS = guarded.Calls()                          # every library symbol the module reached through a proxy
STATS = {}                                       # label -> (guarded buffers, guard bytes checked) of one run
RAN = set()


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


class Plain:
    """Ordinary tensors where a call allocates its own out= / work=: the reference run of (a)."""

    @staticmethod
    def empty(shape, dtype, offset=0, label=None):
        return torch.empty(shape, dtype=dtype, device=DEV)


def plain_inputs(inputs):
    return {k: (torch.from_numpy(np.array(v)).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in inputs.items()}


class Entry:
    def __init__(self, label, build, call, select=None, capacity=32 * MIB, family=None):
        self.label, self.build, self.call, self.select, self.capacity = label, build, call, select, capacity
        self.family = family or label.split(" ")[0]


ENTRIES = []


def entry(label, build, call, select=None, capacity=32 * MIB, family=None):
    ENTRIES.append(Entry(label, build, call, select, capacity, family))


def run_entry(eng, e, setting, offset=0):
    run, arena, out = guarded.run_one(DEV, setting, e.build, lambda inp, mem: e.call(eng, inp, mem), select=e.select,
                                      capacity=e.capacity() if callable(e.capacity) else e.capacity, engine=eng, calls=CALLS,
                                      offset=offset)
    STATS[e.label] = (len(arena.regions), arena.guard_bytes)
    RAN.add(e.label)
    return run, arena, out


def run_plain(eng, e):
    inputs = plain_inputs(e.build())
    out = e.call(eng, inputs, Plain)
    out = tuple(out) if isinstance(out, (tuple, list)) else (out,)
    sel = e.select(out, inputs) if e.select else out
    return [guarded.bits(t) for t in sel if t is not None]


# ---------------------------------------------------------------------------------------------------------------------
# the correlation seam

@functools.lru_cache(maxsize=None)
def seam_frames(ws):
    """(A, B) uint8 [2, H, W] of handoff_cases with H * W odd: one column more where W is even (and, at the odd window size,
    whose H is even, one row more); the grid stays."""
    A, B = HC.frames(ws)
    H0, W0, ov, nr, nc = HC.geometry(ws)
    H, W = seam_geometry(ws)[:2]
    if W > W0:
        A, B = (np.concatenate([t, t[:, :, W0 // 2:W0 // 2 + 1]], axis=2) for t in (A, B))
    if H > H0:
        A, B = (np.concatenate([t, t[:, H0 // 2:H0 // 2 + 1, :]], axis=1) for t in (A, B))
    assert A.shape == (2, H, W) and (H * W) % 2 == 1 and tuple(HC.O.field_shape((H, W), ws, ov)) == (nr, nc)
    assert 2 * nr * nc <= 300                    # "no case has more than a few hundred windows"
    A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


def seam_geometry(ws):
    H, W, ov, nr, nc = HC.geometry(ws)
    return H + (1 - H % 2), W + (1 - W % 2), ov, nr, nc


@functools.lru_cache(maxsize=None)
def seam_predictor(ws):
    """handoff_cases' planted raw predictor with the extremes in the four corners and one cell of every border."""
    H, W, ov, nr, nc = seam_geometry(ws)
    u, v, m = (t.copy() for t in HC.planted(ws))
    cells = [(0, 0), (0, nc - 1), (nr - 1, 0), (nr - 1, nc - 1), (0, nc // 2), (nr - 1, nc // 2), (nr // 2, 0), (nr // 2, nc - 1)]
    values = [ws / 2 + 0.5, -(ws / 2 + 0.5), W + 9.25, -(W + 9.25), 4.0]
    for p in range(2):
        for k, (r, c) in enumerate(cells):
            u[p, r, c] = values[(k + p) % 5]
            v[p, r, c] = values[(k + p + 2) % 5]
            m[p, r, c] = 0
    for t in (u, v, m):
        t.setflags(write=False)
    return u, v, m


def seam_capacity(ws, more=0):
    """Evaluated when the entry runs (the module imports without the library): the work buffer and its guard, the frames, a
    debug pass's windows and maps."""
    def capacity():
        from torchpiv_amd import _lib
        H, W, ov, nr, nc = seam_geometry(ws)
        return int(_lib.lib.tpiv_work_bytes(H, W, ws, ov, 2)) + 26 * MIB + more
    return capacity


def b_frames(ws):
    A, B = seam_frames(ws)
    return {"frame_a": A, "frame_b": B}


def b_fields(ws, mode):
    def build():
        u_raw, v_raw, mask = seam_predictor(ws)
        u0, v0, u2, v2 = handoff(mode, u_raw, v_raw, mask)
        d = dict(b_frames(ws), u0=u0, v0=v0)
        if u2 is not None:
            d.update(u2=u2, v2=v2)
        return d
    return build


def b_compact(ws):
    def build():
        u_raw, v_raw, mask = seam_predictor(ws)
        return dict(b_frames(ws), u_raw=u_raw, v_raw=v_raw, mask=mask)
    return build


def seam_entries():
    for ws in SEAM_SIZES:
        H, W, ov, nr, nc = seam_geometry(ws)
        cap = seam_capacity(ws)
        for prec in PRECISIONS:
            entry(f"pass1 {ws} {prec}", functools.partial(b_frames, ws),
                  lambda eng, i, mem, ws=ws, ov=ov, prec=prec: eng.pass1(i["frame_a"], i["frame_b"], ws, ov, precision=prec),
                  capacity=cap)
        for mode in ("DWS", "CWS"):
            for prec in ("fast", "reference"):
                entry(f"iterate {mode} {ws} {prec}", b_fields(ws, mode),
                      lambda eng, i, mem, ws=ws, ov=ov, mode=mode, prec=prec: eng.iterate(
                          mode, i["frame_a"], i["frame_b"], ws, ov, i["u0"], i["v0"], i["u2"], i["v2"], want_raw=True,
                          precision=prec), capacity=cap)
    for ws in HC.FAST_SIZES:
        H, W, ov, nr, nc = seam_geometry(ws)
        entry(f"iterate CWS_Fast {ws}", b_fields(ws, "CWS_Fast"),
              lambda eng, i, mem, ws=ws, ov=ov: eng.iterate("CWS_Fast", i["frame_a"], i["frame_b"], ws, ov, i["u0"], i["v0"],
                                                            None, None, want_raw=True), capacity=seam_capacity(ws))
    for ws in (16, 64, 28):
        H, W, ov, nr, nc = seam_geometry(ws)
        for mode in ("DWS", "CWS"):
            entry(f"iterate_compact {mode} {ws}", b_compact(ws),
                  lambda eng, i, mem, ws=ws, ov=ov, mode=mode: eng.iterate_compact(
                      mode, i["frame_a"], i["frame_b"], ws, ov, i["u_raw"], i["v_raw"], i["mask"], want_raw=True),
                  capacity=seam_capacity(ws))
    for ws in (16, 32, 64):
        H, W, ov, nr, nc = seam_geometry(ws)
        cap = seam_capacity(ws, 16 * MIB)

        def dbg(mode, ws=ws, ov=ov, **kw):
            if mode == 0:
                return lambda eng, i, mem: eng.debug_pass(0, i["frame_a"], i["frame_b"], ws, ov, **kw)
            return lambda eng, i, mem: eng.debug_pass(mode, i["frame_a"], i["frame_b"], ws, ov, i["u2"], i["v2"], **kw)
        entry(f"debug_pass {ws} pass1 exact", functools.partial(b_frames, ws), dbg(0, precision="exact"), capacity=cap)
        entry(f"debug_pass {ws} pass1 fast", functools.partial(b_frames, ws), dbg(0, precision="fast"), capacity=cap)
        entry(f"debug_pass {ws} CWS reference", b_fields(ws, "CWS"), dbg("CWS", precision="reference"), capacity=cap)
        entry(f"debug_pass {ws} pass1 weighting", functools.partial(b_frames, ws), dbg(0, weighting="gaussian"), capacity=cap)
        entry(f"debug_pass {ws} CWS weighting", b_fields(ws, "CWS"), dbg("CWS", weighting="gaussian"), capacity=cap)
        for kind in ("phase", "rpc"):
            entry(f"debug_pass {ws} pass1 {kind}", functools.partial(b_frames, ws), dbg(0, correlation=kind), capacity=cap)
            entry(f"debug_pass {ws} CWS {kind}", b_fields(ws, "CWS"), dbg("CWS", correlation=kind), capacity=cap)
    for ws, planar in [(8, False), (8, True), (8, 2), (16, False), (16, True), (32, False), (32, True), (64, False),
                       (64, True), (128, False)]:             # the pairs of test_gpu_parity.test_peak_logic_on_handmade_maps
        entry(f"debug_peaks {ws} planar={planar}",
              lambda ws=ws: {"maps": (np.random.default_rng(100 + ws).random((65, ws, ws)) * 10).astype(np.float32)},
              lambda eng, i, mem, planar=planar: eng.debug_peaks(i["maps"], planar=planar))
    for ws in (16, 32, 64):
        H, W, ov, nr, nc = seam_geometry(ws)
        cap = seam_capacity(ws)

        def b_acc(ws=ws, nr=nr, nc=nc, shifted=False):
            d = b_fields(ws, "CWS")() if shifted else b_frames(ws)
            for k in ("u0", "v0", "u2", "v2"):
                if k in d:
                    d[k] = np.ascontiguousarray(d[k][0])
            d["acc"] = (np.random.default_rng(7 * ws).random((nr * nc, ws, ws)) * 3 + 1).astype(np.float32)
            return d
        entry(f"ensemble_add {ws} pass1", b_acc,
              lambda eng, i, mem, ws=ws, ov=ov: eng.ensemble_add(0, i["frame_a"], i["frame_b"], ws, ov, acc=i["acc"]), capacity=cap)
        entry(f"ensemble_add {ws} CWS", functools.partial(b_acc, shifted=True),
              lambda eng, i, mem, ws=ws, ov=ov: eng.ensemble_add("CWS", i["frame_a"], i["frame_b"], ws, ov, acc=i["acc"],
                                                                 u2=i["u2"], v2=i["v2"]), capacity=cap)
        entry(f"ensemble_add {ws} fresh", functools.partial(b_frames, ws),
              lambda eng, i, mem, ws=ws, ov=ov: eng.ensemble_add(0, i["frame_a"], i["frame_b"], ws, ov), capacity=cap)
        entry(f"ensemble_peaks {ws} pass1", b_acc,
              lambda eng, i, mem, ws=ws, ov=ov, H=H, W=W: eng.ensemble_peaks(0, i["acc"], 5, H, W, ws, ov), capacity=cap)
        entry(f"ensemble_peaks {ws} CWS", functools.partial(b_acc, shifted=True),
              lambda eng, i, mem, ws=ws, ov=ov, H=H, W=W: eng.ensemble_peaks("CWS", i["acc"], 5, H, W, ws, ov, i["u0"], i["v0"],
                                                                             i["u2"], i["v2"], want_raw=True), capacity=cap)
    for ws in (16, 32):
        H, W, ov, nr, nc = seam_geometry(ws)

        def b_unc(ws=ws):
            u, v, m = seam_predictor(ws)
            return dict(b_frames(ws), u=u, v=v, invalid=m)
        entry(f"uncertainty {ws}", b_unc,
              lambda eng, i, mem, ws=ws, ov=ov: eng.uncertainty(i["frame_a"], i["frame_b"], i["u"], i["v"], ws, ov,
                                                                invalid=i["invalid"], want_stats=True))


# ---------------------------------------------------------------------------------------------------------------------
# every other engine function that allocates or accepts device memory

IMG = (37, 53)                                   # the "bytes_tail9" shape of test_gpu_mask.py
GRIDS = ((1, 1, 1), (3, 3, 4), (1, 18, 35))      # (batch, n_rows, n_cols): 18 x 35 crosses a 16 x 16 block


def rng_of(label):
    return np.random.default_rng(zlib.crc32(label.encode()))


def b_grid(label, B, nr, nc, nan=False):
    def build():
        r = rng_of(label)
        u, v = r.normal(0, 2, (B, nr, nc)), r.normal(0, 2, (B, nr, nc))
        inv = (r.random((B, nr, nc)) < 0.15).astype(np.uint8)
        if nan and nr * nc > 4:
            u[0, nr // 2, nc // 2] = np.nan
            v[-1, 0, nc - 1] = np.inf
        return {"u": u, "v": v, "inv": inv, "skip": (r.random((B, nr, nc)) < 0.1).astype(np.uint8),
                "grid": (r.random((nr, nc)) < 0.3).astype(np.uint8), "grids": (r.random((B, nr, nc)) < 0.3).astype(np.uint8),
                "status": np.full((B, nr, nc), 1, np.uint8)}
    return build


def b_img(label, n, dtype=np.uint8):
    def build():
        r = rng_of(label)
        hi = 256 if dtype == np.uint8 else 65536
        f = r.integers(0, hi, (n,) + IMG).astype(dtype)
        return {"frames": f, "frames_b": r.integers(0, hi, (n,) + IMG).astype(dtype),
                "bg": r.integers(0, 64, IMG).astype(np.uint8), "mask": (r.random(IMG) < 0.3).astype(np.uint8),
                "masks": (r.random((n,) + IMG) < 0.3).astype(np.uint8)}
    return build


def b_bmp(label, n, background):
    def build():
        r = rng_of(label)
        H, W = IMG
        files, desc, off = [], [], 0
        for f in range(n):
            bpp = (1, 3, 4)[f % 3]
            stride = (W * bpp + 3) // 4 * 4
            data = 54 + (1024 if bpp == 1 else 0)
            files.append(r.integers(0, 256, data + stride * H).astype(np.uint8))
            desc.append([off, data, stride, bpp, (f + 1) % 2, f % 2])
            off += files[-1].size
        d = {"raw": np.concatenate(files), "desc": np.array(desc, np.int64), "lut": r.integers(0, 256, (n, 256)).astype(np.uint8)}
        if background:
            d["bg2"] = r.integers(0, 64, (2,) + IMG).astype(np.uint8)
        return d
    return build


def sel_postval(out, inp):
    """tpiv_postval_compact, include/torchpiv_hip.h: "ring_rc_dev [total ring, 2] int32 (row, column), ring_uv_dev [total
    ring, 2] float64 (u, v), hole_rc_dev [total holes, 2] int32.  The caller sizes ring_* for batch * ceil(cells / 4)
    entries and hole_rc for batch * cells": the lists end at the totals in offsets."""
    u, v, cls, counts, offsets, ring_rc, ring_uv, hole_rc = out
    B = u.shape[0]
    nr_, nh = int(offsets[0, B]), int(offsets[1, B])
    return u, v, cls, counts, offsets, ring_rc[:nr_], ring_uv[:nr_], hole_rc[:nh]


def sel_particles(out, inp):
    """tpiv_particle_detect, include/torchpiv_hip.h: "entries at list index >= capacity are not written, nor are the entries
    of a frame behind its last particle image"."""
    x, y, peak, row_start, count = out[:5]
    keep = torch.arange(x.shape[1], device=x.device)[None, :] < count[:, None]
    return (x[keep], y[keep], peak[keep], row_start, count) + tuple(out[5:])


def other_entries():
    for B, nr, nc in GRIDS:
        g = f"{B}x{nr}x{nc}"
        entry(f"median_test {g}", b_grid("median" + g, B, nr, nc), lambda eng, i, mem: eng.median_test(i["u"], i["v"], i["inv"]))
        entry(f"median_test medians {g}", b_grid("medians" + g, B, nr, nc),
              lambda eng, i, mem: eng.median_test(i["u"], i["v"], i["inv"], want_medians=True))
        entry(f"field_fit {g}", b_grid("fit" + g, B, nr, nc, nan=True),
              lambda eng, i, mem: eng.field_fit(i["u"], i["v"], i["skip"], radius=2, order=2))
        entry(f"finish_fields {g}", b_grid("finish" + g, B, nr, nc), lambda eng, i, mem: eng.finish_fields(i["u"], i["v"], 0.05, 1e-3))
        entry(f"ensemble_moments {g}", b_grid("moments" + g, B, nr, nc), lambda eng, i, mem: eng.ensemble_moments(i["u"], i["v"]))
        entry(f"mask_fields {g}", b_grid("mf" + g, B, nr, nc),
              lambda eng, i, mem: eng.mask_fields(i["u"], i["v"], i["inv"], i["grid"], 1, status=i["status"]))
        entry(f"mask_fields_pairs {g}", b_grid("mfp" + g, B, nr, nc),
              lambda eng, i, mem: eng.mask_fields_pairs(i["u"], i["v"], i["inv"], i["grids"], 0, status=i["status"]))
        entry(f"deform_nodes {g}", b_grid("nodes" + g, B, nr, nc, nan=True),
              lambda eng, i, mem: eng.deform_nodes(i["u"], i["v"], i["inv"], smooth=True))

        def b_comb(B=B, nr=nr, nc=nc, g=g):
            d = b_grid("comb" + g, B, nr, nc)()
            d["nodes"] = rng_of("nodes" + g).integers(-2000, 2000, (B, nr, nc, 2)).astype(np.int16)
            return d
        entry(f"deform_combine {g}", b_comb, lambda eng, i, mem: eng.deform_combine(i["nodes"], i["u"], i["v"], i["inv"]))
        if nr >= 2 and nc >= 2:
            def postval(eng, i, mem):
                cls, counts = eng.postval(i["u"], i["v"], i["inv"])
                return (i["u"], i["v"], cls, counts) + tuple(eng.postval_compact(i["u"], i["v"], cls, counts))
            entry(f"postval postval_compact {g}", b_grid("postval" + g, B, nr, nc), postval, select=sel_postval)

        def b_stereo(B=B, nr=nr, nc=nc, g=g):
            r = rng_of("stereo" + g)
            d = {k: r.normal(0, 1, (B, nr, nc)) for k in ("u1", "v1", "u2", "v2", "su1", "sv1", "su2", "sv2")}
            d.update({k: r.normal(0, 0.3, (nr, nc)) for k in ("a1", "b1", "a2", "b2")})
            d["u1"].reshape(-1)[0] = np.nan
            d["skip"] = (r.random((nr, nc)) < 0.2).astype(np.uint8)
            d["X"], d["Y"] = r.normal(0, 20, (nr, nc)), r.normal(0, 20, (nr, nc))
            return d
        entry(f"stereo_reconstruct {g}", b_stereo,
              lambda eng, i, mem: eng.stereo_reconstruct(i["u1"], i["v1"], i["u2"], i["v2"], i["a1"], i["b1"], i["a2"], i["b2"],
                                                         skip=i["skip"], fill=float("nan")))
        entry(f"stereo_reconstruct sigma {g}", b_stereo,
              lambda eng, i, mem: eng.stereo_reconstruct(i["u1"], i["v1"], i["u2"], i["v2"], i["a1"], i["b1"], i["a2"], i["b2"],
                                                         sigma=(i["su1"], i["sv1"], i["su2"], i["sv2"])))
        entry(f"stereo_triangulate {g}", b_stereo,
              lambda eng, i, mem: eng.stereo_triangulate(i["u1"], i["v1"], i["X"], i["Y"], (-300.0, 0.0, 800.0), (300.0, 5.0, 790.0),
                                                         skip=i["skip"], gap_max=50.0, plane=(0.1, 0.0, 0.0), tol=500.0))

    # the predictor: coarse 32 / 16 -> fine 16 / 8 on 81 x 99 frames (4 x 5 -> 9 x 11 cells)
    for B in (1, 3):
        def b_predict(B=B):
            from torchpiv_amd import engine
            r = rng_of(f"predict{B}")
            xc, yc = engine.coordinates_1d(81, 99, 32, 16)
            xf, yf = engine.coordinates_1d(81, 99, 16, 8)
            return {"Ay": engine.spline_matrix(yc, yf), "Ax": engine.spline_matrix(xc, xf), "u": r.normal(0, 3, (B, 4, 5)),
                    "v": r.normal(0, 3, (B, 4, 5)), "inv": (r.random((B, 4, 5)) < 0.2).astype(np.uint8)}
        for mode in ("DWS", "CWS"):
            entry(f"predict {mode} batch {B}", b_predict,
                  lambda eng, i, mem, mode=mode: eng.predict(mode, i["Ay"], i["Ax"], i["u"], i["v"], i["inv"]))

    for n in (1, 3):
        entry(f"apply_mask n={n}", b_img(f"am{n}", n), lambda eng, i, mem: eng.apply_mask(i["frames"], i["mask"]))
        entry(f"apply_mask_pairs n={n}", b_img(f"amp{n}", n), lambda eng, i, mem: eng.apply_mask_pairs(i["frames"], i["masks"]))
        entry(f"mask_coverage_pairs n={n}", b_img(f"mcp{n}", n), lambda eng, i, mem: eng.mask_coverage_pairs(i["masks"], 8, 4))

        def dynmask(eng, i, mem, n=n):
            need = int(eng.lib.tpiv_dynamic_mask_work_bytes(n, *IMG))
            out, work = mem.empty((n,) + IMG, torch.uint8, label="out="), mem.empty(max(need, 16), torch.uint8, label="work=")
            return eng.dynamic_mask(i["frames"], i["frames_b"], "bright", 5, 128, grow=1, static=i["mask"], out=out, work=work)
        entry(f"dynamic_mask n={n}", b_img(f"dm{n}", n), dynmask)
        entry(f"dynamic_mask fresh n={n}", b_img(f"dmf{n}", n),
              lambda eng, i, mem: eng.dynamic_mask(i["frames"], i["frames_b"], "dark", 3, 100))
        entry(f"prefilter min n={n}", b_img(f"pmin{n}", n), lambda eng, i, mem: eng.prefilter(i["frames"], "min", size=5))
        entry(f"prefilter mean n={n}", b_img(f"pmean{n}", n),
              lambda eng, i, mem: eng.prefilter(i["frames"], "mean", size=7, cap=200, background=i["bg"]))

        def equalize(eng, i, mem, n=n):
            need = int(eng.lib.tpiv_equalize_work_bytes(n, IMG[0], IMG[1], 16))
            work = mem.empty(max(need, 16), torch.uint8, label="work=")
            return eng.equalize(i["frames"], tile=16, clip=3.0, work=work, return_luts=True)
        entry(f"equalize n={n}", b_img(f"eq{n}", n), equalize)
        entry(f"equalize fresh n={n}", b_img(f"eqf{n}", n), lambda eng, i, mem: eng.equalize(i["frames"], tile=16, clip=2.0))
        entry(f"frame_min n={n}", b_img(f"fm{n}", n), lambda eng, i, mem: eng.frame_min(i["frames"]))
        entry(f"frame_min acc n={n}", b_img(f"fma{n}", n), lambda eng, i, mem: eng.frame_min(i["frames"], acc=i["bg"]))
        entry(f"subtract_background n={n}", b_img(f"sb{n}", n), lambda eng, i, mem: eng.subtract_background(i["frames"], i["bg"]))
        entry(f"bmp_unpack n={n}", b_bmp(f"bmp{n}", n, False),
              lambda eng, i, mem: eng.bmp_unpack(i["raw"], i["desc"], i["lut"], *IMG))
        entry(f"bmp_unpack background n={n}", b_bmp(f"bmpbg{n}", n, True),
              lambda eng, i, mem: eng.bmp_unpack(i["raw"], i["desc"], i["lut"], *IMG, background=i["bg2"]))

        def b_deep(n=n):
            from torchpiv_amd import engine
            d = b_img(f"deep{n}", n, np.uint16)()
            d["lut"] = engine.depth_lut(1000, 60000, "sqrt")
            return d
        entry(f"depth_histogram n={n}", b_deep, lambda eng, i, mem: eng.depth_histogram(i["frames"]))
        entry(f"depth_map n={n}", b_deep, lambda eng, i, mem: eng.depth_map(i["frames"], i["lut"]))

        def b_dewarp(n=n):
            from torchpiv_amd import engine
            d = b_img(f"dewarp{n}", n)()
            M = np.array([[1.02, 0.05, -1.5], [-0.04, 0.98, 2.25], [1e-4, -2e-4, 1.0]])
            d["map"] = engine.dewarp_map({"homography": M}, *IMG)
            return d
        for interp in ("linear", "cubic"):
            entry(f"dewarp {interp} n={n}", b_dewarp,
                  lambda eng, i, mem, interp=interp: eng.dewarp(i["frames"], i["map"], interp=interp, fill=7))
        entry(f"particle_detect n={n}", b_img(f"pd{n}", n),
              lambda eng, i, mem: tuple(eng.particle_detect(i["frames"], 200, mask=i["mask"])), select=sel_particles)

        def match(eng, i, mem, n=n):
            pa = eng.particle_detect(i["frames"], 200)
            pb = eng.particle_detect(i["frames_b"], 190, mask=i["mask"])
            m = eng.particle_match(pa, pb, i["up"], i["vp"], [8.0, 26.0, 44.0], [6.0, 18.0, 30.0], 6.0, IMG)
            return tuple(pa) + tuple(pb) + tuple(m)

        def b_match(n=n):
            d = b_img(f"pm{n}", n)()
            r = rng_of(f"pmf{n}")
            d["up"], d["vp"] = r.normal(0, 4, (n, 3, 3)), r.normal(0, 4, (n, 3, 3))
            return d

        def sel_match(out, inp):
            return sel_particles(out[:5], inp) + sel_particles(out[5:10], inp) + tuple(out[10:])
        entry(f"particle_match n={n}", b_match, match, select=sel_match)
    entry("mask_coverage", b_img("mc", 1), lambda eng, i, mem: eng.mask_coverage(i["mask"], 8, 4))

    # deform_warp: grids 3 x 4 (16 / 8 windows) and 18 x 35 (8 / 4 windows), W three pixels past the grid
    for B, nr, nc, ws, ov in ((3, 3, 4, 16, 8), (1, 18, 35, 8, 4), (1, 1, 1, 16, 8)):
        H, W = ws + (nr - 1) * (ws - ov) + 1, ws + (nc - 1) * (ws - ov) + 3

        def b_warp(B=B, nr=nr, nc=nc, H=H, W=W):
            r = rng_of(f"warp{B}{nr}{nc}")
            return {"frame_a": r.integers(0, 256, (B, H, W)).astype(np.uint8), "frame_b": r.integers(0, 256, (B, H, W)).astype(np.uint8),
                    "nodes": r.integers(-1500, 1500, (B, nr, nc, 2)).astype(np.int16), "counter": np.zeros(2, np.int32)}
        for interp in ("linear", "cubic"):
            entry(f"deform_warp {interp} {B}x{nr}x{nc}", b_warp,
                  lambda eng, i, mem, ws=ws, ov=ov, interp=interp: eng.deform_warp(
                      i["frame_a"], i["frame_b"], i["nodes"], ws, ov, interp=interp, counter=i["counter"]) + (i["counter"],))

    # plan entry points that write caller memory
    PH, PW = 32 + 3 * 16 + 1, 32 + 4 * 16 + 3

    def b_plan():
        from torchpiv_amd import synth
        pairs = [synth.make_pair(PH, PW, 40 + k, kind="wavy", noise=1.0) for k in range(2)]
        r = rng_of("plan")
        return {"frame_a": np.stack([p[0].numpy() for p in pairs]), "frame_b": np.stack([p[1].numpy() for p in pairs]),
                "masks": (r.random((2, PH, PW)) < 0.2).astype(np.uint8), "u": r.normal(0, 3, (2, 4, 5)),
                "v": r.normal(0, 3, (2, 4, 5)), "inv": (r.random((2, 4, 5)) < 0.2).astype(np.uint8)}

    def with_plan(fn, **kw):
        def call(eng, i, mem):
            plan = eng.Plan(PH, PW, 32, 16, n_pass=2, mode="CWS", max_batch=2, device=DEV, **kw)
            try:
                out = fn(eng, plan, i)
                torch.cuda.synchronize()
                return out
            finally:
                plan.close()
        return call
    entry("plan run_masked", b_plan, with_plan(lambda eng, plan, i: plan.run_masked(i["frame_a"], i["frame_b"], i["masks"])))
    entry("plan run_ensemble", b_plan,
          with_plan(lambda eng, plan, i: plan.run_ensemble(lambda: iter([(i["frame_a"], i["frame_b"])])), ensemble=True))
    entry("plan debug_predict", b_plan, with_plan(lambda eng, plan, i: plan.debug_predict(1, i["u"], i["v"], i["inv"])))


seam_entries()
other_entries()
BY_LABEL = {e.label: e for e in ENTRIES}
assert len(BY_LABEL) == len(ENTRIES)


# ---------------------------------------------------------------------------------------------------------------------

def pass1_family(ws, prec):
    tile = ws in (8, 16, 32, 64)
    if prec == "exact" and ws % 2 == 0:
        if ws == 128:
            return "xcorr_big128_cand_kernel"
        if tile:
            return f"xcorr_tile_cand_kernel<{ws}>"
        return {28: "xcorr_generic_ct_kernel<0, 28> (cand)", 10: "xcorr_generic_ct_kernel<0, 0> (cand)"}.get(
            ws, "xcorr_generic_kernel<0, float> (cand)")
    if prec != "fast":
        return f"xcorr_f64_split_kernel<{ws}>" if ws in (64, 128) else (f"xcorr_f64_tile_kernel<{ws}>" if tile
                                                                         else "xcorr_generic_kernel<0, double>")
    if ws == 8:
        return "xcorr_w8_kernel<0, true>"
    if tile:
        return f"xcorr_tile_kernel<{ws}, 0, "
    if ws == 128:
        return "xcorr_big128_kernel"
    return {28: "xcorr_generic_ct_kernel<0, 28>", 10: "xcorr_generic_ct_kernel<0, 0>"}.get(ws, "xcorr_generic_kernel<0, float>")


def test_each_size_launches_the_family_it_is_listed_for(eng):
    """One size per kernel, by the library's own dispatch (Plan.kernel_name): the first pass at every precision, the
    shifted passes in both operation orders, the weighted and the spectral kernels."""
    seen = set()
    for ws in SEAM_SIZES:
        H, W, ov, nr, nc = seam_geometry(ws)
        for prec in PRECISIONS:
            plan = eng.Plan(H, W, ws, ov, n_pass=1, max_batch=1, precision=prec)
            name = plan.kernel_name(0)
            plan.close()
            assert name.startswith(pass1_family(ws, prec)), (ws, prec, name)
            seen.add(name)
        for mode in ("DWS", "CWS"):
            for prec, order in (("fast", "exact"), ("reference", "reference")):
                plan = eng.Plan(6 * ws, 6 * ws, 2 * ws, 2 * (ws // 2), n_pass=2, mode=mode, max_batch=1, precision=prec)
                want = expected_kernel(ws if ws != 44 else 22, mode, order)          # (44 = 4 x 11, like 22: the plain kernel)
                assert plan.geometry[1][:2] == (ws, ws // 2) and plan.kernel_name(1) == want, (ws, mode, prec, plan.kernel_name(1))
                seen.add(plan.kernel_name(1))
                plan.close()
    for ws in (16, 32, 64):
        H, W, ov, nr, nc = seam_geometry(ws)
        for kw, stem in (({"weighting": "gaussian"}, "xcorr_win_kernel<"), ({"correlation": "phase"}, "xcorr_spec_kernel<")):
            plan = eng.Plan(H, W, ws, ov, n_pass=1, max_batch=1, **kw)
            assert plan.kernel_name(0).startswith(f"{stem}{ws}, 0, "), (ws, kw, plan.kernel_name(0))
            plan.close()
    families = {n.split("<")[0].split(" ")[0] for n in seen}
    assert families >= {"xcorr_w8_kernel", "xcorr_tile_kernel", "xcorr_tile_cand_kernel", "xcorr_f64_tile_kernel",
                        "xcorr_f64_split_kernel", "xcorr_big128_kernel", "xcorr_big128_cand_kernel", "xcorr_generic_ct_kernel",
                        "xcorr_generic_kernel"}, families


def test_the_seam_frames_are_what_the_issue_asks_for():
    for ws in SEAM_SIZES:
        H, W, ov, nr, nc = seam_geometry(ws)
        A, B = seam_frames(ws)
        assert A.shape == (2, H, W) and (H * W) % 2 == 1 and (nr * nc) % 2 == 1 and (2 * nr * nc) % 64
        assert W - (ws + (nc - 1) * (ws - ov)) in (3, 4) and H - (ws + (nr - 1) * (ws - ov)) in (1, 2)
        u, v, m = seam_predictor(ws)
        for val in (ws / 2 + 0.5, -(ws / 2 + 0.5), W + 9.25, -(W + 9.25), 4.0):
            assert (u == val).any() and (v == val).any()
        border = np.ones((nr, nc), bool)
        border[1:-1, 1:-1] = False
        for w in (u, v):
            assert (np.abs(w[:, border]) > W).any() and not (np.abs(w[:, ~border]) > 64).any()
    assert max(2 * nr * nc for _, _, _, nr, nc in map(seam_geometry, SEAM_SIZES)) <= 300


@pytest.mark.parametrize("label", [e.label for e in ENTRIES])
def test_bounds_and_stale_data(eng, label):
    """(a) and (b) for one table entry."""
    e = BY_LABEL[label]
    want = run_plain(eng, e)
    runs = []
    for setting in SETTINGS:
        run, arena, out = run_entry(eng, e, setting)
        runs.append(run)
        assert len(run) == len(want), (label, len(run), len(want))
        for k, (x, y) in enumerate(zip(run, want)):                 # (a): what the call returns in ordinary tensors
            i = guarded.first_difference(x, y)
            assert i is None, f"{label}: output {k} differs from the unguarded call's at byte {i} under setting {setting}"
        del arena, out
    guarded.differing_output(runs, [f"{label}: output {k}" for k in range(len(want))])       # (b)
    n, g = STATS[label]
    print(f"  {label}: {n} guarded buffers, {g} guard bytes checked per setting")


# ---- (c) refusals

EINVAL = 1


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def refusal_cases():
    """(label, need(lib), call(lib, inputs, outputs, work pointer, work bytes), inputs, outputs, sized): sized = the entry
    point takes work_bytes and documents the size, so need - 1 is refused; every one refuses NULL."""
    cases = []
    ws = 16
    H, W, ov, nr, nc = seam_geometry(ws)
    N = nr * nc
    fields = b_fields(ws, "CWS")
    seam_need = lambda lib: int(lib.tpiv_work_bytes(H, W, ws, ov, 2))                                   # noqa: E731
    one_need = lambda lib: int(lib.tpiv_work_bytes(H, W, ws, ov, 1))                                    # noqa: E731
    uvi = lambda B=2: {"u": ((B, nr, nc), torch.float64), "v": ((B, nr, nc), torch.float64), "inv": ((B, nr, nc), torch.uint8)}  # noqa: E731
    dbg = dict(uvi(), win=((2, N, 2, ws, ws), torch.float32), corr=((2, N, ws, ws), torch.float32))
    cases.append(("tpiv_pass1", seam_need, lambda lib, i, o, w, n: lib.tpiv_pass1(
        _ptr(i["frame_a"]), _ptr(i["frame_b"]), 2, H, W, ws, ov, 1.2, 3, 3, _ptr(o["u"]), _ptr(o["v"]), _ptr(o["inv"]), w, n,
        _stream()), functools.partial(b_frames, ws), uvi(), False))
    cases.append(("tpiv_iter", seam_need, lambda lib, i, o, w, n: lib.tpiv_iter(
        2, _ptr(i["frame_a"]), _ptr(i["frame_b"]), 2, H, W, ws, ov, _ptr(i["u0"]), _ptr(i["v0"]), _ptr(i["u2"]), _ptr(i["v2"]),
        1.2, 3, 0, _ptr(o["u"]), _ptr(o["v"]), _ptr(o["inv"]), None, None, w, n, _stream()), fields, uvi(), False))
    cases.append(("tpiv_debug_iter_compact", seam_need, lambda lib, i, o, w, n: lib.tpiv_debug_iter_compact(
        2, _ptr(i["frame_a"]), _ptr(i["frame_b"]), 2, H, W, ws, ov, _ptr(i["u_raw"]), _ptr(i["v_raw"]), _ptr(i["mask"]), 1.2, 3,
        0, _ptr(o["u"]), _ptr(o["v"]), _ptr(o["inv"]), None, None, w, n, _stream()), b_compact(ws), uvi(), False))
    cases.append(("tpiv_debug_pass", seam_need, lambda lib, i, o, w, n: lib.tpiv_debug_pass(
        0, 0, _ptr(i["frame_a"]), _ptr(i["frame_b"]), 2, H, W, ws, ov, None, None, None, _ptr(o["u"]), _ptr(o["v"]),
        _ptr(o["inv"]), _ptr(o["win"]), _ptr(o["corr"]), w, n, _stream()), functools.partial(b_frames, ws), dbg, False))

    def b_tab(kind):
        def build():
            from torchpiv_amd import engine
            par = engine.weighting_arg("gaussian") if kind == "w" else engine.correlation_arg("rpc")
            tab = engine.weighting_tables(par, [ws]) if kind == "w" else engine.correlation_tables(par, [ws])
            return dict(b_frames(ws), tab=tab)
        return build
    cases.append(("tpiv_debug_pass_weighted", seam_need, lambda lib, i, o, w, n: lib.tpiv_debug_pass_weighted(
        0, _ptr(i["tab"]), _ptr(i["frame_a"]), _ptr(i["frame_b"]), 2, H, W, ws, ov, None, None, None, _ptr(o["u"]), _ptr(o["v"]),
        _ptr(o["inv"]), _ptr(o["win"]), _ptr(o["corr"]), w, n, _stream()), b_tab("w"), dbg, False))
    cases.append(("tpiv_debug_pass_spec", seam_need, lambda lib, i, o, w, n: lib.tpiv_debug_pass_spec(
        0, 2, 2.0 ** -10, _ptr(i["tab"]), _ptr(i["frame_a"]), _ptr(i["frame_b"]), 2, H, W, ws, ov, None, None, None, _ptr(o["u"]),
        _ptr(o["v"]), _ptr(o["inv"]), _ptr(o["win"]), _ptr(o["corr"]), w, n, _stream()), b_tab("s"), dbg, False))

    def b_acc():
        return dict(b_frames(ws), acc=np.full((N, ws, ws), 2.0, np.float32))
    cases.append(("tpiv_ensemble_add", one_need, lambda lib, i, o, w, n: lib.tpiv_ensemble_add(
        0, _ptr(i["frame_a"]), _ptr(i["frame_b"]), 2, H, W, ws, ov, None, None, _ptr(i["acc"]), w, n, _stream()), b_acc, {}, True))
    cases.append(("tpiv_ensemble_peaks", one_need, lambda lib, i, o, w, n: lib.tpiv_ensemble_peaks(
        0, _ptr(i["acc"]), 5, H, W, ws, ov, None, None, None, None, 1.2, 3, _ptr(o["u"]), _ptr(o["v"]), _ptr(o["inv"]), None, None,
        w, n, _stream()), b_acc, uvi(1), True))
    n_maps = 65
    cases.append(("tpiv_debug_peaks", lambda lib: n_maps * 32, lambda lib, i, o, w, n: lib.tpiv_debug_peaks(
        _ptr(i["maps"]), n_maps, 16, 0, 1.2, 3, _ptr(o["u"]), _ptr(o["v"]), _ptr(o["inv"]), w, n, _stream()),
        lambda: {"maps": (np.random.default_rng(3).random((n_maps, 16, 16)) * 10).astype(np.float32)},
        {"u": (n_maps, torch.float64), "v": (n_maps, torch.float64), "inv": (n_maps, torch.uint8)}, True))
    cases.append(("tpiv_equalize", lambda lib: int(lib.tpiv_equalize_work_bytes(3, IMG[0], IMG[1], 16)),
                  lambda lib, i, o, w, n: lib.tpiv_equalize(_ptr(i["frames"]), 3, IMG[0], IMG[1], 16, 768, _ptr(o["out"]), w, n,
                                                            _stream()), b_img("eqr", 3), {"out": ((3,) + IMG, torch.uint8)}, True))
    cases.append(("tpiv_dynamic_mask", lambda lib: int(lib.tpiv_dynamic_mask_work_bytes(3, *IMG)),
                  lambda lib, i, o, w, n: lib.tpiv_dynamic_mask(_ptr(i["frames"]), _ptr(i["frames_b"]), 3, IMG[0], IMG[1], 0, 5, 128,
                                                                1, None, _ptr(o["out"]), w, _stream()),
                  b_img("dmr", 3), {"out": ((3,) + IMG, torch.uint8)}, False))
    cap = 9

    def b_pm():
        r = rng_of("pmr")
        per_row = np.concatenate([[0], r.multinomial(cap, np.ones(IMG[0] - 2) / (IMG[0] - 2)), [0]])       # interior rows
        rs = np.concatenate([[0], np.cumsum(per_row)]).astype(np.int32)[None]
        y = np.repeat(np.arange(IMG[0]), per_row)[None] + r.uniform(-0.4, 0.4, (1, cap))
        return {"xa": r.uniform(1, 50, (1, cap)), "ya": y, "rsa": rs, "xb": r.uniform(1, 50, (1, cap)), "yb": y + 0.25, "rsb": rs.copy(),
                "up": r.normal(0, 1, (1, 2, 2)), "vp": r.normal(0, 1, (1, 2, 2)), "cen": np.array([10.0, 40.0, 8.0, 30.0])}
    cases.append(("tpiv_particle_match", lambda lib: 16 * cap, lambda lib, i, o, w, n: lib.tpiv_particle_match(
        _ptr(i["xa"]), _ptr(i["ya"]), _ptr(i["rsa"]), cap, _ptr(i["xb"]), _ptr(i["yb"]), _ptr(i["rsb"]), cap, 1, IMG[0], IMG[1],
        _ptr(i["up"]), _ptr(i["vp"]), 2, 2, _ptr(i["cen"]), C.c_void_p(i["cen"].data_ptr() + 16), 4.0, _ptr(o["match"]),
        _ptr(o["status"]), _ptr(o["d2"]), _ptr(o["matched"]), w, n, _stream()), b_pm,
        {"match": ((1, cap), torch.int32), "status": ((1, cap), torch.uint8), "d2": ((1, cap), torch.float64),
         "matched": (1, torch.int32)}, True))
    return cases


REFUSALS = refusal_cases()


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals_leave_memory_alone(eng, case):
    """(c): a work buffer one byte short (where the entry point takes its size and documents it) and a NULL one are
    TPIV_EINVAL; the outputs keep their poison, an accumulator its contents, the guards hold."""
    name, need_of, call, build, outputs, sized = case
    lib = guarded.LibProxy(eng.lib, CALLS)
    need = need_of(lib)
    assert need > 1
    for poison, guard in SETTINGS:
        arena = Arena(DEV, poison, guard, need + 32 * MIB)
        host = build()
        inp = guarded.place_inputs(arena, host)
        out = {k: arena.empty(shape, dtype, label=f"output {k}") for k, (shape, dtype) in outputs.items()}
        work = arena.empty(need, torch.uint8, label="work")
        tries = [(None, 0), (None, need)] + ([(_ptr(work), need - 1), (_ptr(work), 0)] if sized else [])
        for w, n in tries:
            rc = call(lib, inp, out, w, n)
            torch.cuda.synchronize()
            assert rc == EINVAL, (name, "work", "NULL" if w is None else "given", n, "of", need, "->", rc)
            assert eng.lib.tpiv_last_error()
        for k, t in out.items():
            assert arena.holds_poison(t), (name, k, "was written by a refused call")
        assert arena.holds_poison(work), (name, "the work buffer was written by a refused call")
        for k, v in host.items():
            if isinstance(v, np.ndarray):
                assert guarded.first_difference(guarded.bits(inp[k]), guarded.bits(torch.from_numpy(np.array(v)))) is None, (name, k)
        arena.check()
        # ... and the same buffers, exactly `need` bytes of work, are accepted
        rc = call(lib, inp, out, _ptr(work), need)
        torch.cuda.synchronize()
        assert rc == 0, (name, rc, eng.lib.tpiv_last_error())
        arena.check()


def test_short_work_tensors_are_refused_by_the_engine(eng):
    """engine.equalize / engine.dynamic_mask with their own work= one byte short: ValueError, nothing written."""
    arena = Arena(DEV, 0xFF, 0x00, 8 * MIB)
    inp = guarded.place_inputs(arena, b_img("short", 3)())
    out = arena.empty((3,) + IMG, torch.uint8)
    with guarded.patched(eng, arena, CALLS):
        for fn, need in ((lambda w: eng.equalize(inp["frames"], tile=16, out=out, work=w),
                          int(eng.lib.tpiv_equalize_work_bytes(3, IMG[0], IMG[1], 16))),
                         (lambda w: eng.dynamic_mask(inp["frames"], inp["frames_b"], "bright", 5, 128, out=out, work=w),
                          int(eng.lib.tpiv_dynamic_mask_work_bytes(3, *IMG)))):
            work = arena.empty(need - 1, torch.uint8)
            with pytest.raises(ValueError):
                fn(work)
            torch.cuda.synchronize()
            assert arena.holds_poison(work) and arena.holds_poison(out)
    arena.check()


# ---- alignment

FRAME_OFFSETS = (1, 2, 3, 15)
DEEP_OFFSETS = (2, 6, 14)
ALIGN_SEAM = [f"pass1 {ws} {p}" for ws in (16, 64, 28, 128) for p in ("exact", "fast")] + \
             [f"iterate CWS {ws} fast" for ws in (16, 64, 28, 128)]
ALIGN_SEAM_MORE = [f"debug_pass {ws} pass1 fast" for ws in (16, 64)] + ["ensemble_add 16 CWS", "ensemble_add 64 pass1",
                                                                       "uncertainty 16", "uncertainty 32",
                                                                       "deform_warp cubic 3x3x4", "deform_warp linear 1x18x35",
                                                                       "plan run_masked", "plan run_ensemble"]


@pytest.mark.parametrize("label", ALIGN_SEAM + ALIGN_SEAM_MORE)
def test_alignment_of_the_correlation_seam(eng, label):
    """Frames at byte offsets 1, 2, 3 and 15 past a 256-byte boundary: the header states no requirement, so the outputs are
    bit-identical to those of offset 0 (and the guards hold: a wide load that leaves the pair would read guard bytes, and
    the comparison under another setting in test_bounds_and_stale_data would see them)."""
    e = BY_LABEL[label]
    setting = SETTINGS[2]
    base, _, _ = run_entry(eng, e, setting, offset=0)
    for off in FRAME_OFFSETS:
        run, arena, _ = run_entry(eng, e, setting, offset=off)
        assert arena.regions[0][0].startswith("input frame") and (arena.regions[0][2] - arena._base) % 256 == off
        for k, (x, y) in enumerate(zip(run, base)):
            i = guarded.first_difference(x, y)
            assert i is None, f"{label}: output {k} at frame offset {off} differs from offset 0 at byte {i}"
    # the other two settings at the oddest offset: a read outside the misplaced frames that reaches a result
    runs = [run_entry(eng, e, s, offset=15)[0] for s in SETTINGS]
    guarded.differing_output(runs, [f"{label} at offset 15: output {k}" for k in range(len(base))])


IMAGES = ("frames", "frames_b", "raw", "bg", "bg2", "mask", "masks")          # every uint8 / uint16 image input of b_img, b_bmp


def _named_frames(e):
    """The entry with its uint8 / uint16 image inputs renamed so that run_one's offset applies to them."""
    def build():
        d = e.build()
        return {("frame_" + k if k in IMAGES else k): v for k, v in d.items()}

    def call(eng, i, mem):
        return e.call(eng, {(k[6:] if k.startswith("frame_") and k[6:] in IMAGES else k): v for k, v in i.items()}, mem)
    return Entry(e.label + " (offset)", build, call, e.select, e.capacity)


ALIGN_FRAMES = ["apply_mask n=3", "apply_mask_pairs n=3", "dynamic_mask n=3", "prefilter min n=3", "prefilter mean n=3",
                "equalize n=3", "frame_min n=3", "subtract_background n=3", "bmp_unpack n=3", "bmp_unpack background n=3",
                "dewarp linear n=3", "dewarp cubic n=3", "particle_detect n=3", "particle_match n=3", "mask_coverage",
                "mask_coverage_pairs n=3", "depth_histogram n=3", "depth_map n=3"]


@pytest.mark.parametrize("label", ALIGN_FRAMES)
def test_alignment_of_frame_readers(eng, label):
    """Every other entry point that reads uint8 frames (offsets 1, 2, 3, 15) or uint16 frames (2, 6, 14; tpiv_depth_map:
    "src_dev needs 2-byte alignment only"): the header asks for nothing more, the outputs are those of offset 0."""
    e = _named_frames(BY_LABEL[label])
    setting = SETTINGS[1]
    base, _, _ = run_entry(eng, e, setting, offset=0)
    for off in (DEEP_OFFSETS if label.startswith("depth") else FRAME_OFFSETS):
        run, arena, _ = run_entry(eng, e, setting, offset=off)
        assert (arena.regions[0][2] - arena._base) % 256 == off, arena.regions[0]
        for k, (x, y) in enumerate(zip(run, base)):
            i = guarded.first_difference(x, y)
            assert i is None, f"{label}: output {k} at frame offset {off} differs from offset 0 at byte {i}"


def test_alignment_the_header_requires(eng):
    """Where the header states a requirement the misaligned call is TPIV_EINVAL and writes nothing: tpiv_particle_match
    ("work_dev: ... 8-byte aligned"), tpiv_deform_warp ("nodes that are not 4-byte aligned"), tpiv_ensemble_add / _peaks
    ("acc_dev ... 16-byte aligned"; "a null or misaligned accumulator"), tpiv_dewarp ("a map that is not 4-byte aligned")."""
    lib = guarded.LibProxy(eng.lib, CALLS)
    arena = Arena(DEV, 0xFF, 0x00, 32 * MIB)
    name, need_of, call, build, outputs, _ = next(c for c in REFUSALS if c[0] == "tpiv_particle_match")
    inp = guarded.place_inputs(arena, build())
    out = {k: arena.empty(s, d) for k, (s, d) in outputs.items()}
    work = arena.empty(need_of(lib) + 8, torch.uint8)
    assert call(lib, inp, out, C.c_void_p(work.data_ptr() + 4), need_of(lib)) == EINVAL
    watch = list(out.values()) + [work]
    # nodes int16 at 2 bytes past a 4-byte boundary
    e = BY_LABEL["deform_warp cubic 3x3x4"]
    d = e.build()
    i = guarded.place_inputs(arena, {k: v for k, v in d.items() if k != "nodes"})
    nodes = arena.place(torch.from_numpy(d["nodes"]), offset=2)
    with guarded.patched(eng, arena, CALLS):
        n_before = len(arena.regions)
        with pytest.raises(ValueError):
            eng.deform_warp(i["frame_a"], i["frame_b"], nodes, 16, 8, interp="cubic")
        watch += [arena.buf[s:t] for _, _, s, t, _ in arena.regions[n_before:]]                 # wa, wb
    # accumulator float32 at 4 bytes past a 16-byte boundary
    ws = 16
    H, W, ov, nr, nc = seam_geometry(ws)
    fr = guarded.place_inputs(arena, b_frames(ws))
    acc = arena.empty((nr * nc, ws, ws), torch.float32, offset=4)
    assert acc.numel() * 4 == lib.tpiv_ensemble_bytes(H, W, ws, ov)
    with guarded.patched(eng, arena, CALLS):
        n_before = len(arena.regions)
        with pytest.raises(ValueError):
            eng.ensemble_add(0, fr["frame_a"], fr["frame_b"], ws, ov, acc=acc)
        with pytest.raises(ValueError):
            eng.ensemble_peaks(0, acc, 3, H, W, ws, ov)
        watch += [acc] + [arena.buf[s:t] for _, _, s, t, _ in arena.regions[n_before:]]         # work, u, v, invalid
    # map int32 at 2 bytes past a 4-byte boundary: no tensor can say that, so through the library
    e = BY_LABEL["dewarp cubic n=3"]
    d = e.build()
    frames = arena.place(torch.from_numpy(d["frames"]))
    raw_map = arena.place(torch.from_numpy(d["map"]).view(torch.uint8).reshape(-1), offset=2)
    table = torch.from_numpy(eng.dewarp_cubic_table()).to(DEV)
    outw = arena.empty((3,) + IMG, torch.uint8)
    assert lib.tpiv_dewarp(_ptr(frames), None, 3, IMG[0], IMG[1], _ptr(raw_map), _ptr(table), 1, 0, _ptr(outw), _stream()) == EINVAL
    watch.append(outw)
    torch.cuda.synchronize()
    assert all(arena.holds_poison(t) for t in watch)
    arena.check()


# ---- plan reuse

PLANS = {"CWS exact 64/32 -> 32/16": dict(n_pass=2, mode="CWS", precision="exact"),
         "DWS fast 64/32 -> 32/16": dict(n_pass=2, mode="DWS", precision="fast"),
         "CWS 64/32 -> 42/21 -> 28/14": dict(n_pass=3, mode="CWS", pass_scale=1.5)}
PLAN_H, PLAN_W = 64 + 4 * 32 + 1, 64 + 5 * 32 + 3


@functools.lru_cache(maxsize=None)
def plan_pairs():
    from torchpiv_amd import synth
    pairs = [synth.make_pair(PLAN_H, PLAN_W, 70 + k, kind=("wavy", "vortex")[k % 2], noise=1.0) for k in range(4)]
    a, b = np.stack([p[0].numpy() for p in pairs]), np.stack([p[1].numpy() for p in pairs])
    return (a[:3], b[:3]), (a[3:], b[3:])


@pytest.mark.parametrize("name", list(PLANS))
def test_plan_state_does_not_leak(eng, name):
    """A plan's workspace is the library's own, so it cannot be guarded; what it leaves behind can be tested: pairs A at
    max_batch = 3, then pairs B at batch 1 -- B's fields and the intermediate pass_fields are bit for bit a fresh plan's.
    Both results go through out= tensors of 4 rows from an arena: the rows beyond the batch keep their poison."""
    kw = PLANS[name]
    (a3, b3), (a1, b1) = plan_pairs()
    fresh = eng.Plan(PLAN_H, PLAN_W, 64, 32, max_batch=3, device=DEV, **kw)
    want = [guarded.bits(t) for t in fresh.run(*(torch.from_numpy(t).to(DEV) for t in (a1, b1)))]
    want_pf = [[guarded.bits(t) for t in fresh.pass_fields(p, 1)] for p in range(fresh.n_pass - 1)]
    fresh.close()
    for poison, guard in SETTINGS:
        arena = Arena(DEV, poison, guard, 32 * MIB)
        inp = guarded.place_inputs(arena, {"frame_a3": a3, "frame_b3": b3, "frame_a1": a1, "frame_b1": b1})
        with guarded.patched(eng, arena, CALLS):
            plan = eng.Plan(PLAN_H, PLAN_W, 64, 32, max_batch=3, device=DEV, **kw)
            nr, nc = plan.out_shape
            outs = []
            for k, batch in (("3", 3), ("1", 1)):
                out = (arena.empty((4, nr, nc), torch.float64), arena.empty((4, nr, nc), torch.float64),
                       arena.empty((4, nr, nc), torch.uint8))
                got = plan.run(inp["frame_a" + k], inp["frame_b" + k], out=out)
                torch.cuda.synchronize()
                assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
                for t in out:
                    assert arena.holds_poison(t[batch:]), (name, "rows beyond the batch were written", batch)
                outs.append(out)
            pf = [[guarded.bits(t) for t in plan.pass_fields(p, 1)] for p in range(plan.n_pass - 1)]
            plan.close()
        arena.check()
        for k, (t, w) in enumerate(zip(outs[1], want)):
            i = guarded.first_difference(guarded.bits(t[:1]), w)
            assert i is None, f"{name}: output {k} of the second run differs from a fresh plan's at byte {i}"
        for p, (got_p, want_p) in enumerate(zip(pf, want_pf)):
            for k, (x, y) in enumerate(zip(got_p, want_p)):
                i = guarded.first_difference(x, y)
                assert i is None, f"{name}: pass_fields({p}) field {k} of the second run differs from a fresh plan's at byte {i}"


# ---- coverage of the table

EXEMPT = {
    "tpiv_version": "host only: the ABI number",
    "tpiv_last_error": "host only: the message of the last failure (read through _lib.check, outside the proxy)",
    "tpiv_coordinates": "host only: geometry into host arrays",
    "tpiv_spline_matrix": "host only: the spline operator into a host array (it builds the inputs of the predict entries)",
    "tpiv_read_files": "reader: host files into host staging memory",
    "tpiv_reader_open": "reader: host files into host staging memory",
    "tpiv_reader_next": "reader: host files into host staging memory",
    "tpiv_reader_release": "reader: host files into host staging memory",
    "tpiv_reader_close": "reader: host files into host staging memory",
    "tpiv_plan_kernel_name": "plan getter: a name into a host buffer",
    "tpiv_plan_exact_fallbacks": "plan getter: one host number",
    "tpiv_plan_exact_timing": "plan getter: host numbers",
    "tpiv_plan_set_timing": "plan setter: a flag",
    "tpiv_plan_get_timing": "plan getter: host numbers",
    "tpiv_plan_deform_ms": "plan getter: one host number",
    "tpiv_plan_set_outlier": "plan setter: allocates plan-owned memory, moves none of the caller's",
    "tpiv_plan_pass_outliers": "plan getter: a pointer into plan-owned memory",
    "tpiv_plan_set_mask": "plan setter: reads the caller's image once into plan-owned grids, writes nothing of the caller's",
    "tpiv_plan_pass_mask": "plan getter: a pointer into plan-owned memory",
    "tpiv_plan_pass_pair_mask": "plan getter: a pointer into plan-owned memory",
    "tpiv_plan_set_uncertainty": "plan setter: allocates plan-owned memory",
    "tpiv_plan_uncertainty": "plan getter: pointers into plan-owned memory",
    "tpiv_plan_set_deform": "plan setter: copies the caller's table once into plan-owned memory",
    "tpiv_plan_deform_stage": "plan getter: pointers into plan-owned memory",
    "tpiv_plan_set_correlation": "plan setter: copies a host table into plan-owned memory",
    "tpiv_plan_set_weighting": "plan setter: copies a host table into plan-owned memory",
}


def test_every_symbol_is_exercised_or_exempt(eng, request):
    """The symbols the library proxy recorded over the whole table equal the declared ones minus EXEMPT: a new entry point
    fails here until it has a table entry or a reason.  (Entries, refusals and plans this session did not run yet -- the
    test was selected alone -- run here once.)"""
    from torchpiv_amd import _lib
    for e in ENTRIES:
        if e.label not in RAN:
            run_entry(eng, e, SETTINGS[0])
    if "tpiv_equalize_work_bytes" not in CALLS:
        for case in REFUSALS:
            test_refusals_leave_memory_alone(eng, case)
    if "tpiv_plan_pass_fields" not in CALLS:
        test_plan_state_does_not_leak(eng, next(iter(PLANS)))
    assert all(isinstance(r, str) and len(r) > 8 for r in EXEMPT.values())
    declared = set(_lib.SIGNATURES)
    assert set(EXEMPT) <= declared, sorted(set(EXEMPT) - declared)
    both = CALLS & set(EXEMPT)
    assert not both, f"exempt but exercised (drop the exemption): {sorted(both)}"
    missing = declared - set(EXEMPT) - CALLS
    assert not missing, f"neither exercised by a table entry nor exempt with a reason: {sorted(missing)}"
    assert CALLS <= declared, sorted(CALLS - declared)
    by_family = {}
    for e in ENTRIES:
        n, g = STATS[e.label]
        c = by_family.setdefault(e.family, [0, 0, 0])
        c[0], c[1], c[2] = c[0] + 1, c[1] + n, c[2] + g
    for fam, (cases, n, g) in by_family.items():
        print(f"  {fam}: {cases} cases, {n} guarded buffers, {g} guard bytes checked per setting")
