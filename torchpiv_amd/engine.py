"""Thin tensor-level wrappers over the C ABI: PyTorch-ROCm tensors in, tensors out.

PyTorch is used for device memory and streams only; all arithmetic of the hot path
happens in libtorchpiv_hip.so.  Every function requires CUDA(HIP) tensors and raises
otherwise -- there is no CPU fallback.
"""
from __future__ import annotations

import collections
import ctypes as C
import functools

import numpy as np
import torch

from . import _lib
from ._lib import ITER_MODES, MODES, PRECISIONS, check, lib
from .options import *  # noqa: F401,F403  (the keyword parsers, their constants and checks live there; engine.X keeps working)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _hip():
    """The HIP runtime itself, opened at its first use: for copies out of arrays that a plan owns (Plan._copy_out)."""
    return C.CDLL("libamdhip64.so")


def _need_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("torchpiv_amd: the HIP path needs tensors on a ROCm device "
                               "(there is no CPU fallback)")


def _frames(a: torch.Tensor, b: torch.Tensor):
    _need_cuda(a, b)
    if a.dtype != torch.uint8 or b.dtype != torch.uint8:
        raise TypeError("frames must be uint8")
    if a.shape != b.shape:
        raise ValueError("frame shapes differ")
    if a.dim() == 2:
        a, b = a[None], b[None]
    if a.dim() != 3:
        raise ValueError("frames must be [H, W] or [batch, H, W]")
    return a.contiguous(), b.contiguous()


def _work(H, W, ws, ov, batch, device):
    """Caller-provided work buffer of the function-level entry points (torch's caching allocator is
    stream-aware, so concurrent calls on different streams get different buffers)."""
    n = int(lib.tpiv_work_bytes(H, W, ws, ov, batch))
    buf = torch.empty(max(n, 16), dtype=torch.uint8, device=device)
    return buf, n


def _precision(precision):
    try:
        return PRECISIONS[precision]
    except KeyError:
        raise KeyError(f"precision must be one of {sorted(PRECISIONS)}, got {precision!r}") from None


def field_shape(H, W, ws, ov):
    """get_field_shape, PIVbackend.py:425-456."""
    nr, nc = C.c_int(), C.c_int()
    check(lib.tpiv_field_shape(H, W, ws, ov, C.byref(nr), C.byref(nc)))
    return nr.value, nc.value


def coordinates_1d(H, W, ws, ov):
    """Axis vectors of get_coordinates, PIVbackend.py:522-597."""
    nr, nc = field_shape(H, W, ws, ov)
    x = np.empty(nc, dtype=np.float64)
    y = np.empty(nr, dtype=np.float64)
    check(lib.tpiv_coordinates(H, W, ws, ov, x.ctypes.data_as(C.POINTER(C.c_double)),
                               y.ctypes.data_as(C.POINTER(C.c_double))))
    return x, y


def spline_matrix(xc: np.ndarray, xf: np.ndarray) -> np.ndarray:
    """1-D operator of the RectBivariateSpline predictor (host, float64)."""
    xc = np.ascontiguousarray(xc, dtype=np.float64)
    xf = np.ascontiguousarray(xf, dtype=np.float64)
    A = np.empty((xf.size, xc.size), dtype=np.float64)
    P = C.POINTER(C.c_double)
    check(lib.tpiv_spline_matrix(xc.size, xc.ctypes.data_as(P), xf.size, xf.ctypes.data_as(P),
                                 A.ctypes.data_as(P)))
    return A


def pass1(a, b, ws, ov, val_ratio=1.2, val_win=3, precision="exact"):
    """Device part of extended_search_area_piv(validate=True). Returns u, v (float64) and
    invalid (uint8), each [batch, n_rows, n_cols], on the frames' device.
    precision: "exact" (default, like OfflinePIV: exact integer correlation sums at the cells that reach the result, 64x64
    windows -- csrc/xcorr_exact.hip; other sizes run as "f64"), "f64" (float64 transforms as in PIVbackend.py:513-514), "reference"
    (the same kernel here) or "fast" (float32 transforms, about 1e-6 px from the reference; opt-in)."""
    a, b = _frames(a, b)
    B, H, W = a.shape
    prec = _precision(precision)
    nr, nc = field_shape(H, W, ws, ov)
    u = torch.empty(B, nr, nc, dtype=torch.float64, device=a.device)
    v = torch.empty_like(u)
    inv = torch.empty(B, nr, nc, dtype=torch.uint8, device=a.device)
    with torch.cuda.device(a.device):
        work, nbytes = _work(H, W, ws, ov, B, a.device)
        check(lib.tpiv_pass1(a.data_ptr(), b.data_ptr(), B, H, W, ws, ov, val_ratio, val_win, prec,
                             u.data_ptr(), v.data_ptr(), inv.data_ptr(), work.data_ptr(), nbytes, _stream()))
    return u, v, inv


def predict(mode, Ay, Ax, u_c, v_c, inv_c):
    """Spline predictor of one iteration: returns u0, v0 (zeroed where invalid), u2, v2."""
    _need_cuda(Ay, Ax, u_c, v_c, inv_c)
    B, nrc, ncc = u_c.shape
    nrf, ncf = Ay.shape[0], Ax.shape[0]
    dev = u_c.device
    work = torch.empty(B * 3 * nrc * ncf, dtype=torch.float64, device=dev)
    outs = [torch.empty(B, nrf, ncf, dtype=torch.float64, device=dev) for _ in range(4)]
    with torch.cuda.device(dev):
        check(lib.tpiv_predict(MODES[mode], B, nrc, ncc, nrf, ncf, Ay.data_ptr(), Ax.data_ptr(),
                               u_c.contiguous().data_ptr(), v_c.contiguous().data_ptr(),
                               inv_c.contiguous().data_ptr(), work.data_ptr(),
                               *[o.data_ptr() for o in outs], _stream()))
    return outs


def iterate(mode, a, b, ws, ov, u0, v0, u2, v2, val_ratio=1.2, val_win=3, want_raw=False, precision="exact"):
    """Device part of piv_iteration_{DWS,CWS}.__call__ after the predictor.  Shifted passes run in float32 like the
    reference's (B:249-257) at every precision; precision="reference" additionally keeps the reference's operation
    order in the CWS bilinear sampling (bit-identical staged windows), "exact" (default), "f64" and "fast" use the lerp form."""
    prec = _precision(precision)
    a, b = _frames(a, b)
    if mode == "CWS_Fast" and u2 is None:        # B:599-675: the shift is u0 / 2 inside the window; no u2 field
        u2, v2 = u0, v0
    _need_cuda(u0, v0, u2, v2)
    B, H, W = a.shape
    nr, nc = field_shape(H, W, ws, ov)
    dev = a.device
    u = torch.empty(B, nr, nc, dtype=torch.float64, device=dev)
    v = torch.empty_like(u)
    inv = torch.empty(B, nr, nc, dtype=torch.uint8, device=dev)
    du = torch.empty_like(u) if want_raw else None
    dv = torch.empty_like(u) if want_raw else None
    with torch.cuda.device(dev):
        work, nbytes = _work(H, W, ws, ov, B, dev)
        check(lib.tpiv_iter(ITER_MODES[mode], a.data_ptr(), b.data_ptr(), B, H, W, ws, ov,
                            u0.contiguous().data_ptr(), v0.contiguous().data_ptr(),
                            u2.contiguous().data_ptr(), v2.contiguous().data_ptr(),
                            val_ratio, val_win, prec, u.data_ptr(), v.data_ptr(), inv.data_ptr(),
                            du.data_ptr() if want_raw else None, dv.data_ptr() if want_raw else None,
                            work.data_ptr(), nbytes, _stream()))
    if want_raw:
        return u, v, inv, du, dv
    return u, v, inv


def iterate_compact(mode, a, b, ws, ov, u_raw, v_raw, mask, val_ratio=1.2, val_win=3, want_raw=False, precision="exact"):
    """Test hook: iterate() fed with the compact hand-off of Plan.run -- the raw predictor u_raw, v_raw (float64, before
    the invalid-zeroing) and its thresholded mask (uint8) -- instead of the four fields u0, v0, u2, v2: the zeroing, the
    halving and DWS's rint happen where the kernels read them.  mode "DWS" or "CWS"; same outputs as iterate()."""
    prec = _precision(precision)
    a, b = _frames(a, b)
    _need_cuda(u_raw, v_raw, mask)
    if mask.dtype != torch.uint8:
        raise TypeError("mask must be uint8")
    B, H, W = a.shape
    nr, nc = field_shape(H, W, ws, ov)
    for t in (u_raw, v_raw, mask):
        if tuple(t.shape) != (B, nr, nc):
            raise ValueError(f"predictor fields must be [{B}, {nr}, {nc}], got {tuple(t.shape)}")
    if u_raw.dtype != torch.float64 or v_raw.dtype != torch.float64:
        raise TypeError("u_raw, v_raw must be float64")
    u_raw, v_raw, mask = u_raw.contiguous(), v_raw.contiguous(), mask.contiguous()
    dev = a.device
    u = torch.empty(B, nr, nc, dtype=torch.float64, device=dev)
    v = torch.empty_like(u)
    inv = torch.empty(B, nr, nc, dtype=torch.uint8, device=dev)
    du = torch.empty_like(u) if want_raw else None
    dv = torch.empty_like(u) if want_raw else None
    with torch.cuda.device(dev):
        work, nbytes = _work(H, W, ws, ov, B, dev)
        check(lib.tpiv_debug_iter_compact(ITER_MODES[mode], a.data_ptr(), b.data_ptr(), B, H, W, ws, ov,
                                          u_raw.data_ptr(), v_raw.data_ptr(), mask.data_ptr(), val_ratio, val_win, prec,
                                          u.data_ptr(), v.data_ptr(), inv.data_ptr(),
                                          du.data_ptr() if want_raw else None, dv.data_ptr() if want_raw else None,
                                          work.data_ptr(), nbytes, _stream()))
    if want_raw:
        return u, v, inv, du, dv
    return u, v, inv


def debug_pass(mode, a, b, ws, ov, u2=None, v2=None, precision="reference", weighting=None, correlation=None):
    """Test hook: one pass plus the staged windows and the correlation maps (shifted passes at
    `precision`: "reference" = the reference's operation order, bit-identical windows).  Pass 1
    (mode 0) runs the float32 kernel, or with precision="exact" the exact first pass, whose maps
    are those of its float32 locating kernel -- the map every decision is taken on, also for the
    windows that then go to the float64 transform.  "CWS_Fast" takes u2, v2 as its predictor u0, v0 (the windows are
    resampled by -/+ u0 / 2 inside themselves); DWS / CWS return u = 2 u2 + du where valid, 0 where invalid.
    correlation (correlation_arg): the spectrally filtered pass instead (tpiv_debug_pass_spec; `precision` has no effect on
    it) -- the windows as staged, before the mean removal, and the filtered map the decisions are taken on.
    weighting (weighting_arg): the weighted pass instead (tpiv_debug_pass_weighted; `precision` has no effect on it) -- the
    windows as staged, before the weighting, and the map the decisions are taken on."""
    prec = _precision(precision)
    corr_par = correlation_arg(correlation)
    if corr_par is not None:
        correlation_check([ws], mode if isinstance(mode, str) else None)
    wt_par = weighting_arg(weighting)
    if wt_par is not None:
        weighting_check([ws], mode if isinstance(mode, str) else None, correlation=corr_par)
    a, b = _frames(a, b)
    B, H, W = a.shape
    nr, nc = field_shape(H, W, ws, ov)
    dev = a.device
    N = nr * nc
    u = torch.empty(B, nr, nc, dtype=torch.float64, device=dev)
    v = torch.empty_like(u)
    inv = torch.empty(B, nr, nc, dtype=torch.uint8, device=dev)
    win = torch.empty(B, N, 2, ws, ws, dtype=torch.float32, device=dev)
    corr = torch.empty(B, N, ws, ws, dtype=torch.float32, device=dev)
    m = 0 if mode in (0, None, "PASS1") else ITER_MODES[mode]
    zero = torch.zeros(B, nr, nc, dtype=torch.float64, device=dev) if m else None
    if wt_par is not None:
        tab = torch.from_numpy(weighting_tables(wt_par, [ws])).to(dev)
        with torch.cuda.device(dev):
            work, nbytes = _work(H, W, ws, ov, B, dev)
            check(lib.tpiv_debug_pass_weighted(m, tab.data_ptr(), a.data_ptr(), b.data_ptr(), B, H, W, ws, ov,
                                               u2.contiguous().data_ptr() if u2 is not None else None,
                                               v2.contiguous().data_ptr() if v2 is not None else None,
                                               zero.data_ptr() if zero is not None else None,
                                               u.data_ptr(), v.data_ptr(), inv.data_ptr(), win.data_ptr(),
                                               corr.data_ptr(), work.data_ptr(), nbytes, _stream()))
        return u, v, inv, win, corr
    if corr_par is not None:
        tab = torch.from_numpy(correlation_tables(corr_par, [ws])).to(dev)
        with torch.cuda.device(dev):
            work, nbytes = _work(H, W, ws, ov, B, dev)
            check(lib.tpiv_debug_pass_spec(m, _lib.CORRELATIONS[corr_par["kind"]], corr_par["floor"], tab.data_ptr(),
                                           a.data_ptr(), b.data_ptr(), B, H, W, ws, ov,
                                           u2.contiguous().data_ptr() if u2 is not None else None,
                                           v2.contiguous().data_ptr() if v2 is not None else None,
                                           zero.data_ptr() if zero is not None else None,
                                           u.data_ptr(), v.data_ptr(), inv.data_ptr(), win.data_ptr(),
                                           corr.data_ptr(), work.data_ptr(), nbytes, _stream()))
        return u, v, inv, win, corr
    with torch.cuda.device(dev):
        work, nbytes = _work(H, W, ws, ov, B, dev)
        check(lib.tpiv_debug_pass(m, prec, a.data_ptr(), b.data_ptr(), B, H, W, ws, ov,
                                  u2.contiguous().data_ptr() if u2 is not None else None,
                                  v2.contiguous().data_ptr() if v2 is not None else None,
                                  zero.data_ptr() if zero is not None else None,
                                  u.data_ptr(), v.data_ptr(), inv.data_ptr(), win.data_ptr(),
                                  corr.data_ptr(), work.data_ptr(), nbytes, _stream()))
    return u, v, inv, win, corr


def debug_peaks(maps: torch.Tensor, val_ratio=1.2, val_win=3, planar=False):
    """Test hook: the kernels' peak analysis on hand-made correlation maps [n, ws, ws], ws in
    8/16/32/64/128.  planar selects the LDS layout of the three-wavefront tile kernels."""
    _need_cuda(maps)
    maps = maps.contiguous().float()
    n, ws = maps.shape[0], maps.shape[-1]
    u = torch.empty(n, dtype=torch.float64, device=maps.device)
    v = torch.empty_like(u)
    inv = torch.empty(n, dtype=torch.uint8, device=maps.device)
    work = torch.empty(max(n * 32, 16), dtype=torch.uint8, device=maps.device)
    with torch.cuda.device(maps.device):
        check(lib.tpiv_debug_peaks(maps.data_ptr(), n, ws, int(planar), float(val_ratio), int(val_win),
                                   u.data_ptr(), v.data_ptr(), inv.data_ptr(), work.data_ptr(), n * 32, _stream()))
    return u, v, inv


ENSEMBLE_MODES = {0: 0, None: 0, "PASS1": 0, "DWS": _lib.MODE_DWS, "CWS": _lib.MODE_CWS}


def correlation_tables(par, sizes):
    """float32 [sum over the passes of 2 (ws/2 + 1)]: g_y[0 .. ws/2] then g_x[0 .. ws/2] per pass, g[j] =
    float32(exp(-(pi d / (2 ws))^2 j^2)) evaluated in float64 and rounded once."""
    out = []
    for ws in sizes:
        j = np.arange(ws // 2 + 1, dtype=np.float64)
        for d in (par["dy"], par["dx"]):
            out.append(np.exp(-(np.pi * d / (2.0 * ws)) ** 2 * j * j).astype(np.float32))
    return np.ascontiguousarray(np.concatenate(out))


def weighting_tables(par, sizes):
    """float32 [sum over the passes of 2 ws]: g_y[0 .. ws-1] then g_x[0 .. ws-1] per pass; "gaussian": g[i] =
    float32(exp(-t^2 / (2 sigma^2))), t = (2 i - (ws - 1)) / ws, evaluated in float64 and rounded once; "uniform": ones."""
    out = []
    for ws in sizes:
        t = (2.0 * np.arange(ws, dtype=np.float64) - (ws - 1)) / ws
        for s in (par["sy"], par["sx"]):
            out.append(np.ones(ws, np.float32) if par["kind"] == "uniform"
                       else np.exp(-t * t / (2.0 * s * s)).astype(np.float32))
    return np.ascontiguousarray(np.concatenate(out))


def ensemble_mode(mode):
    try:
        return ENSEMBLE_MODES[mode]
    except (KeyError, TypeError):
        raise KeyError(f"ensemble mode must be 0 / 'PASS1', 'DWS' or 'CWS', got {mode!r}") from None


def ensemble_bytes(H, W, ws, ov):
    """Bytes of the accumulator of (ws, ov) on H x W frames: n_rows * n_cols * ws * ws * 4 (0: not an ensemble geometry)."""
    return int(lib.tpiv_ensemble_bytes(int(H), int(W), int(ws), int(ov)))


def ensemble_add(mode, a, b, ws, ov, acc=None, u2=None, v2=None):
    """Adds the raw correlation maps of the pairs a, b uint8 [batch, H, W] to acc float32 [n_rows * n_cols, ws, ws]
    (fftshift layout; None: a fresh zeroed one) and returns acc (tpiv_ensemble_add).  mode 0 / "PASS1": first-pass maps;
    "DWS" / "CWS": the windows shifted by the half shift u2, v2 float64 [n_rows, n_cols] (or [1, n_rows, n_cols]) -- one
    shift per window for every pair.  ws in 16, 32, 64 (NotImplementedError otherwise).  Pairs are summed in float32 in
    ascending order without atomics: the same calls give the same bits."""
    m = ensemble_mode(mode)
    a, b = _frames(a, b)
    B, H, W = a.shape
    if ws not in ENSEMBLE_SIZES:
        raise NotImplementedError(f"ensemble correlation covers window sizes 16, 32 and 64 (got {ws})")
    nr, nc = field_shape(H, W, ws, ov)
    dev = a.device
    if acc is None:
        acc = torch.zeros(nr * nc, ws, ws, dtype=torch.float32, device=dev)
    else:
        _need_cuda(acc)
        if acc.dtype != torch.float32 or tuple(acc.shape) != (nr * nc, ws, ws) or not acc.is_contiguous() or acc.device != dev:
            raise ValueError(f"ensemble_add: acc must be a contiguous float32 [{nr * nc}, {ws}, {ws}] tensor on the frames' device")
    if m:
        if u2 is None or v2 is None:
            raise ValueError("ensemble_add: a shifted pass needs the half shift u2, v2")
        _need_cuda(u2, v2)
        u2, v2 = (t.reshape(nr, nc).contiguous() if t.numel() == nr * nc else t for t in (u2, v2))
        for t in (u2, v2):
            if t.dtype != torch.float64 or tuple(t.shape) != (nr, nc) or t.device != dev:
                raise ValueError(f"ensemble_add: u2, v2 must be float64 [{nr}, {nc}] on the frames' device")
    with torch.cuda.device(dev):
        work, nbytes = _work(H, W, ws, ov, 1, dev)
        check(lib.tpiv_ensemble_add(m, a.data_ptr(), b.data_ptr(), B, H, W, ws, ov, u2.data_ptr() if m else None,
                                    v2.data_ptr() if m else None, acc.data_ptr(), work.data_ptr(), nbytes, _stream()))
    return acc


def ensemble_peaks(mode, acc, n_pairs, H, W, ws, ov, u0=None, v0=None, u2=None, v2=None, val_ratio=1.2, val_win=3,
                   want_raw=False):
    """The field of an accumulator of n_pairs pairs (tpiv_ensemble_peaks): M = acc / n_pairs in float32 through the peak
    stage of every pass.  Returns u, v float64 and invalid uint8 [1, n_rows, n_cols]; a shifted mode takes the predictor
    fields u0, v0, u2, v2 of predict() / Plan.debug_predict for a batch of one and combines like iterate(); want_raw adds
    the raw displacement du, dv of a shifted pass."""
    m = ensemble_mode(mode)
    _need_cuda(acc, u0, v0, u2, v2)
    if ws not in ENSEMBLE_SIZES:
        raise NotImplementedError(f"ensemble correlation covers window sizes 16, 32 and 64 (got {ws})")
    nr, nc = field_shape(H, W, ws, ov)
    dev = acc.device
    if acc.dtype != torch.float32 or tuple(acc.shape) != (nr * nc, ws, ws) or not acc.is_contiguous():
        raise ValueError(f"ensemble_peaks: acc must be a contiguous float32 [{nr * nc}, {ws}, {ws}] tensor")
    pred = [None] * 4
    if m:
        if any(t is None for t in (u0, v0, u2, v2)):
            raise ValueError("ensemble_peaks: a shifted pass needs u0, v0, u2, v2")
        pred = [t.reshape(nr, nc).contiguous() if t.numel() == nr * nc else t for t in (u0, v0, u2, v2)]
        for t in pred:
            if t.dtype != torch.float64 or tuple(t.shape) != (nr, nc) or t.device != dev:
                raise ValueError(f"ensemble_peaks: predictor fields must be float64 [{nr}, {nc}] on the accumulator's device")
    u = torch.empty(1, nr, nc, dtype=torch.float64, device=dev)
    v = torch.empty_like(u)
    inv = torch.empty(1, nr, nc, dtype=torch.uint8, device=dev)
    raw = m and want_raw
    du = torch.empty_like(u) if raw else None
    dv = torch.empty_like(u) if raw else None
    with torch.cuda.device(dev):
        work, nbytes = _work(H, W, ws, ov, 1, dev)
        check(lib.tpiv_ensemble_peaks(m, acc.data_ptr(), int(n_pairs), H, W, ws, ov, *[t.data_ptr() if m else None for t in pred],
                                      float(val_ratio), int(val_win), u.data_ptr(), v.data_ptr(), inv.data_ptr(),
                                      du.data_ptr() if raw else None, dv.data_ptr() if raw else None, work.data_ptr(), nbytes,
                                      _stream()))
    return (u, v, inv, du, dv) if raw else (u, v, inv)


PIXEL_CORR_RADIUS = (3, 16)      # search radius R; the plane is D x D, D = 2 R + 1
PIXEL_CORR_BIN = 256             # pixels of a bin at most
PIXEL_CORR_SHIFT = 64            # |pre-shift| per axis at most
PIXEL_CORR_BATCH = 256           # pairs per tpiv_pixel_corr_add call (32-bit partial sums)
PIXEL_CORR_PAIRS = 65536         # pairs of a recording (the int64 numerators stay below 2^57)
PIXEL_CORR_STATUS = {"valid": 0, "border": 1, "flat": 2, "range": 3, "fit": 4, "ratio": 5, "masked": 6}

PixelCorr = collections.namedtuple("PixelCorr", "u v peak ratio status corr")


def single_pixel_arg(radius=4, bin=1, shift=(0, 0), min_ratio=None, shape=None):
    """The arguments of single-pixel ensemble correlation, checked (no GPU involved): radius, an integer in 3..16; bin, an
    integer k (k x k pixels) or a pair (k_y, k_x) of integers >= 1 with k_y * k_x <= 256; shift, a pair of integers
    (s_y, s_x) with |s| <= 64, the one pre-shift of every bin; min_ratio, None or a finite number >= 1; shape, None or the
    frame shape (H, W), which a bin must fit.  Returns {"radius", "bin": (k_y, k_x), "shift": (s_y, s_x), "min_ratio"}."""
    if not is_int(radius) or not PIXEL_CORR_RADIUS[0] <= radius <= PIXEL_CORR_RADIUS[1]:
        raise ValueError(f"single_pixel: radius must be an integer in {PIXEL_CORR_RADIUS[0]}..{PIXEL_CORR_RADIUS[1]}, got {radius!r}")
    ky_kx = (bin, bin) if is_int(bin) else bin
    if (not isinstance(ky_kx, (tuple, list)) or len(ky_kx) != 2 or not all(is_int(k) for k in ky_kx)
            or min(ky_kx) < 1 or ky_kx[0] * ky_kx[1] > PIXEL_CORR_BIN):
        raise ValueError(f"single_pixel: bin must be an integer or a pair (k_y, k_x) of integers >= 1 with k_y * k_x <= "
                         f"{PIXEL_CORR_BIN}, got {bin!r}")
    if (not isinstance(shift, (tuple, list)) or len(shift) != 2 or not all(is_int(s) for s in shift)
            or max(abs(int(s)) for s in shift) > PIXEL_CORR_SHIFT):
        raise ValueError(f"single_pixel: shift must be a pair (s_y, s_x) of integers with |s| <= {PIXEL_CORR_SHIFT}, got {shift!r}")
    if min_ratio is not None and (not is_real(min_ratio) or not np.isfinite(min_ratio) or min_ratio < 1):
        raise ValueError(f"single_pixel: min_ratio must be None or a finite number >= 1, got {min_ratio!r}")
    if shape is not None:
        H, W = int(shape[0]), int(shape[1])
        if ky_kx[0] > H or ky_kx[1] > W:
            raise ValueError(f"single_pixel: a bin of {tuple(ky_kx)} pixels does not fit frames of {(H, W)}")
    return {"radius": int(radius), "bin": (int(ky_kx[0]), int(ky_kx[1])), "shift": (int(shift[0]), int(shift[1])),
            "min_ratio": None if min_ratio is None else float(min_ratio)}


def pixel_corr_bytes(H, W, bin, radius):
    """Bytes of the accumulator acc int64 [n_by, n_bx, D, D] of bins `bin` at search radius `radius` on H x W frames
    (tpiv_pixel_corr_bytes; 0: a geometry the library refuses)."""
    ky, kx = (bin, bin) if is_int(bin) else bin
    return int(lib.tpiv_pixel_corr_bytes(int(H), int(W), int(ky), int(kx), int(radius)))


def pixel_corr_coordinates(H, W, bin):
    """(x [n_bx], y [n_by]): the bin centres in pixels -- the axis vectors of get_coordinates at window = bin, overlap 0,
    each axis with its own bin edge."""
    ky, kx = (bin, bin) if is_int(bin) else bin
    return coordinates_1d(W, W, kx, 0)[0], coordinates_1d(H, H, ky, 0)[1]


def _pixel_corr_acc(who, t, shape, dev):
    _need_cuda(t)
    if t.dtype != torch.int64 or tuple(t.shape) != shape or not t.is_contiguous() or (dev is not None and t.device != dev):
        raise ValueError(f"{who} must be a contiguous int64 {list(shape)} tensor on the device")


def pixel_corr_add(a, b, bin, radius, shift=(0, 0), acc=None, mom=None):
    """Adds the pairs a, b uint8 [batch, H, W] (or [H, W]) to the accumulators of single-pixel ensemble correlation and
    returns (acc, mom) (tpiv_pixel_corr_add): acc int64 [n_by, n_bx, D, D], the products a(p) b(p + shift + d) summed over
    the pixels of a bin and over the pairs; mom int64 [4, H, W], the per-pixel sums of a, a^2, b, b^2.  None: fresh zeroed
    ones.  Exact integer sums without atomics: any split of a recording into calls gives the same bits.  At most 256 pairs
    per library call: a larger batch goes in several."""
    par = single_pixel_arg(radius, bin, shift)
    a, b = _frames(a, b)
    B, H, W = (int(s) for s in a.shape)
    (ky, kx), R, (sy, sx) = par["bin"], par["radius"], par["shift"]
    single_pixel_arg(radius, bin, shift, shape=(H, W))
    D = 2 * R + 1
    dev = a.device
    if acc is None:
        acc = torch.zeros(H // ky, W // kx, D, D, dtype=torch.int64, device=dev)
    else:
        _pixel_corr_acc("pixel_corr_add: acc", acc, (H // ky, W // kx, D, D), dev)
    if mom is None:
        mom = torch.zeros(4, H, W, dtype=torch.int64, device=dev)
    else:
        _pixel_corr_acc("pixel_corr_add: mom", mom, (4, H, W), dev)
    with torch.cuda.device(dev):
        for k in range(0, B, PIXEL_CORR_BATCH):
            n = min(PIXEL_CORR_BATCH, B - k)
            check(lib.tpiv_pixel_corr_add(a[k:k + n].data_ptr(), b[k:k + n].data_ptr(), n, H, W, ky, kx, R, sy, sx,
                                          acc.data_ptr(), mom.data_ptr(), _stream()))
    return acc, mom


def pixel_corr_peaks(acc, mom, n_pairs, shape, bin, radius, shift=(0, 0), planes=False):
    """The field of the accumulators of n_pairs pairs (tpiv_pixel_corr_peaks): a PixelCorr record of u, v (pixels, the
    pre-shift included), peak (the correlation coefficient at the peak), ratio (peak to second peak) float64 and status
    uint8 [n_by, n_bx] (PIXEL_CORR_STATUS), and corr float64 [n_by, n_bx, D, D], the planes of coefficients (planes=True;
    else None).  A bin with a non-zero status carries NaN."""
    H, W = int(shape[0]), int(shape[1])
    par = single_pixel_arg(radius, bin, shift, shape=(H, W))
    (ky, kx), R, (sy, sx) = par["bin"], par["radius"], par["shift"]
    D = 2 * R + 1
    nby, nbx = H // ky, W // kx
    _pixel_corr_acc("pixel_corr_peaks: acc", acc, (nby, nbx, D, D), None)
    _pixel_corr_acc("pixel_corr_peaks: mom", mom, (4, H, W), acc.device)
    if not is_int(n_pairs) or not 1 <= n_pairs <= PIXEL_CORR_PAIRS:
        raise ValueError(f"pixel_corr_peaks: n_pairs must be an integer in 1..{PIXEL_CORR_PAIRS}, got {n_pairs!r}")
    dev = acc.device
    u = torch.empty(nby, nbx, dtype=torch.float64, device=dev)
    v = torch.empty_like(u)
    peak = torch.empty_like(u)
    ratio = torch.empty_like(u)
    status = torch.empty(nby, nbx, dtype=torch.uint8, device=dev)
    corr = torch.empty(nby, nbx, D, D, dtype=torch.float64, device=dev) if planes else None
    with torch.cuda.device(dev):
        check(lib.tpiv_pixel_corr_peaks(acc.data_ptr(), mom.data_ptr(), int(n_pairs), H, W, ky, kx, R, sy, sx, u.data_ptr(),
                                        v.data_ptr(), peak.data_ptr(), ratio.data_ptr(), status.data_ptr(),
                                        corr.data_ptr() if planes else None, _stream()))
    return PixelCorr(u, v, peak, ratio, status, corr)


def median_test(u, v, inv, threshold=2.0, eps=0.1, min_neighbours=3, want_medians=False):
    """Normalized median test (Westerweel & Scarano 2005; tpiv_median_test) on fields u, v float64 and the mask inv uint8,
    [batch, n_rows, n_cols] on the GPU.  Returns status uint8 (bit 0: flagged, bit 1: invalid on input), with
    want_medians also the neighbourhood medians (status, med_u, med_v).  The inputs are not written."""
    _need_cuda(u, v, inv)
    if u.dtype != torch.float64 or v.dtype != torch.float64 or inv.dtype != torch.uint8:
        raise TypeError("median_test: u, v float64 and invalid uint8")
    if u.dim() != 3 or u.shape != v.shape or u.shape != inv.shape:
        raise ValueError("median_test: [batch, n_rows, n_cols] tensors of one shape")
    par = outlier_arg({"threshold": threshold, "eps": eps, "min_neighbours": min_neighbours})
    u, v, inv = u.contiguous(), v.contiguous(), inv.contiguous()
    B, nr, nc = u.shape
    status = torch.empty(B, nr, nc, dtype=torch.uint8, device=u.device)
    mu = torch.empty_like(u) if want_medians else None
    mv = torch.empty_like(v) if want_medians else None
    with torch.cuda.device(u.device):
        check(lib.tpiv_median_test(u.data_ptr(), v.data_ptr(), inv.data_ptr(), B, nr, nc, par["threshold"], par["eps"],
                                   par["min_neighbours"], status.data_ptr(), mu.data_ptr() if want_medians else None,
                                   mv.data_ptr() if want_medians else None, _stream()))
    return (status, mu, mv) if want_medians else status


FIELD_FIT_TILE = (8, 64)         # rows, columns of the cells a workgroup of tpiv_field_fit covers (csrc/piv_kernels.h)


def field_fit(u, v, skip=None, radius=2, order=2):
    """Local least-squares polynomial fit (tpiv_field_fit) of fields u, v float64 [batch, n_rows, n_cols] (or [n_rows,
    n_cols]) on the GPU over the (2 radius + 1)^2 neighbourhood of every cell, radius 1..3, order 1 or 2; skip (uint8,
    optional, the same shape): non-zero = the cell is not data, as is a cell whose u or v is not finite.  Returns (fit,
    count, order): fit float64 [6, batch, n_rows, n_cols] = the planes U, Ux, Uy, V, Vx, Vy (the denoised vector and its
    slopes per cell spacing along the columns and the rows), count uint8 = the data cells used, order int8 = the order
    fitted (2, 1, 0: the mean, -1: nothing, all NaN).  A 2-D input gives outputs without the batch axis.  The inputs are not
    written."""
    _need_cuda(u, v, skip)
    if u.dtype != torch.float64 or v.dtype != torch.float64 or (skip is not None and skip.dtype != torch.uint8):
        raise TypeError("field_fit: u, v float64 and skip uint8")
    if u.dim() not in (2, 3) or u.shape != v.shape or (skip is not None and skip.shape != u.shape):
        raise ValueError("field_fit: [batch, n_rows, n_cols] or [n_rows, n_cols] tensors of one shape")
    par = derive_arg({"quantities": DERIVE_QUANTITIES[0], "radius": radius, "order": order})
    flat = u.dim() == 2
    if flat:
        u, v = u[None], v[None]
        skip = None if skip is None else skip[None]
    u, v = u.contiguous(), v.contiguous()
    skip = None if skip is None else skip.contiguous()
    B, nr, nc = u.shape
    fit = torch.empty(6, B, nr, nc, dtype=torch.float64, device=u.device)
    count = torch.empty(B, nr, nc, dtype=torch.uint8, device=u.device)
    fitted = torch.empty(B, nr, nc, dtype=torch.int8, device=u.device)
    with torch.cuda.device(u.device):
        check(lib.tpiv_field_fit(u.data_ptr(), v.data_ptr(), None if skip is None else skip.data_ptr(), B, nr, nc,
                                 par["radius"], par["order"], fit.data_ptr(), count.data_ptr(), fitted.data_ptr(), _stream()))
    return (fit[:, 0], count[0], fitted[0]) if flat else (fit, count, fitted)


def derive(fit, hx, hy, quantities=DERIVE_QUANTITIES):
    """The quantities of DERIVE_QUANTITIES named in `quantities` from field_fit's planes (fit, or the tuple field_fit
    returns): {name: float64 tensor}, elementwise on fit's device.  hx, hy: the signed grid steps along the columns and the
    rows in millimetres; with fields in m/s the slopes dudx = Ux / (hx / 1000), dudy = Uy / (hy / 1000), dvdx, dvdy come out
    in 1/s.  vorticity = dvdx - dudy, divergence = dudx + dvdy, shear = dvdx + dudy, q = -0.5 (dudx dudx + 2 dudy dvdx + dvdy
    dvdy), swirl = sqrt(max(0, dudx dvdy - dudy dvdx - 0.25 (dudx + dvdy)^2)) (the imaginary part of the complex eigenvalue
    of the gradient tensor), u_smooth = U, v_smooth = V.  Every expression left to right as written, one float64 operation
    each."""
    if isinstance(fit, (tuple, list)):
        fit = fit[0]
    names = derive_arg({"quantities": tuple(quantities) if isinstance(quantities, list) else quantities})["quantities"]
    if not isinstance(fit, torch.Tensor) or fit.dtype != torch.float64:
        raise TypeError("derive: fit float64, the planes of field_fit")
    if fit.dim() < 1 or fit.shape[0] != 6:
        raise ValueError("derive: fit holds the six planes U, Ux, Uy, V, Vx, Vy")
    if not is_real(hx) or not is_real(hy) or not hx or not hy or hx != hx or hy != hy:
        raise ValueError(f"derive: hx, hy must be non-zero numbers (millimetres), got {hx!r}, {hy!r}")
    U, Ux, Uy, V, Vx, Vy = fit.unbind(0)
    # (the steps as tensors on fit's device: torch divides by a host scalar as a product with its reciprocal, which is not
    #  the correctly rounded quotient)
    sx = torch.full((), float(hx) / 1000, dtype=torch.float64, device=fit.device)
    sy = torch.full((), float(hy) / 1000, dtype=torch.float64, device=fit.device)
    made = {"u_smooth": U, "v_smooth": V}

    def get(name):
        if name in made:
            return made[name]
        if name in ("dudx", "dudy", "dvdx", "dvdy"):
            out = {"dudx": Ux, "dudy": Uy, "dvdx": Vx, "dvdy": Vy}[name] / (sx if name[-1] == "x" else sy)
        elif name == "vorticity":
            out = get("dvdx") - get("dudy")
        elif name == "divergence":
            out = get("dudx") + get("dvdy")
        elif name == "shear":
            out = get("dvdx") + get("dudy")
        elif name == "q":
            out = (get("dudx") * get("dudx") + 2.0 * get("dudy") * get("dvdx") + get("dvdy") * get("dvdy")) * -0.5
        else:
            s = get("dudx") + get("dvdy")
            disc = get("dudx") * get("dvdy") - get("dudy") * get("dvdx") - (s * s) * 0.25
            out = torch.sqrt(torch.where(disc < 0, torch.zeros_like(disc), disc))     # (a NaN stays NaN)
        made[name] = out
        return out
    return {name: get(name) for name in names}


TRACKS_RADIUS = 1.5              # pixels: generous for the predictor error of a multipass field, about half the 2.9 px mean
TRACKS_RADIUS_MAX = 8.0          # nearest-neighbour spacing at 0.03 particles per pixel
PARTICLE_STATUS = {"matched": 0, "no_candidate": 1, "lost_claim": 2, "outside": 3, "no_particle": 255}

Particles = collections.namedtuple("Particles", "x y peak row_start count")
Matches = collections.namedtuple("Matches", "match status d2 matched")


def tracks_arg(level=None, radius=TRACKS_RADIUS):
    """The arguments of tracks(), checked (no GPU involved): level, the intensity threshold of a particle image, an integer
    in 1..255 and required -- there is no honest default for an intensity threshold; radius, the search radius around the
    predicted position in pixels, a number in (0, 8].  Returns {"level": int, "radius": float}."""
    if level is None:
        raise ValueError("tracks: level is required (the intensity threshold of a particle image, an integer in 1..255)")
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or not 1 <= level <= 255:
        raise ValueError(f"tracks: level must be an integer in 1..255, got {level!r}")
    if not is_real(radius) or not 0 < radius <= TRACKS_RADIUS_MAX:      # (a NaN fails the comparison)
        raise ValueError(f"tracks: radius must be a number in (0, {TRACKS_RADIUS_MAX:g}] (pixels), got {radius!r}")
    return {"level": int(level), "radius": float(radius)}


def particle_table():
    """The table of the sub-pixel fit of particle_detect: float64 [256], ln(max(i, 1)), made on the host (the device and
    a host model read the same numbers, so the fit is the same bits whatever logarithm made them)."""
    return np.log(np.maximum(np.arange(256), 1).astype(np.float64))


@functools.lru_cache(maxsize=None)
def _particle_table_on(device):
    return torch.from_numpy(particle_table()).to(device)


def particle_detect(frames, level, mask=None, capacity=None):
    """Particle images (tpiv_particle_count / tpiv_particle_detect) of uint8 frames [n, H, W] (or [H, W]) on the GPU, H, W >=
    3: the interior pixels that reach `level` (integer 0..255), are not under mask (uint8 [H, W], optional, non-zero =
    masked), exceed their four 8-neighbours before them in raster order and are not below the four behind them, each with
    a three-point log-Gaussian sub-pixel fit per axis.  Returns Particles(x, y, peak, row_start, count): x, y float64
    [n, capacity] in image coordinates (x along the columns, y along the rows downward, pixel (0, 0) centred at the origin),
    peak uint8 [n, capacity], row_start int32 [n, H + 1] (list index of the first particle of each row; entry H = the
    total), count int32 [n] -- every list in raster order of the peak pixel, in every run.  capacity=None counts first, reads
    the totals once on the host and stores exactly the longest list; a given capacity needs no host read and stores the
    first `capacity` particles of each frame, with count and row_start still those of the whole list.  Entries behind a
    frame's last particle are unspecified.  A 2-D input gives outputs without the frame axis.  The inputs are not
    written."""
    _need_cuda(frames, mask)
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or (mask is not None and mask.dtype != torch.uint8):
        raise TypeError("particle_detect: frames uint8 and mask uint8")
    if frames.dim() not in (2, 3):
        raise ValueError("particle_detect: frames must be [n, H, W] or [H, W]")
    flat = frames.dim() == 2
    f = (frames[None] if flat else frames).contiguous()
    n, H, W = f.shape
    if H < 3 or W < 3:
        raise ValueError(f"particle_detect: frames of at least 3 x 3 pixels, got {H} x {W}")
    if mask is not None and tuple(mask.shape) != (H, W):
        raise ValueError(f"particle_detect: mask must be [{H}, {W}], got {tuple(mask.shape)}")
    if mask is not None and mask.device != f.device:
        raise ValueError("particle_detect: frames and mask on one device")
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or not 0 <= level <= 255:
        raise ValueError(f"particle_detect: level must be an integer in 0..255, got {level!r}")
    if capacity is not None and (isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < 0):
        raise ValueError(f"particle_detect: capacity must be None or an integer >= 0, got {capacity!r}")
    mask = None if mask is None else mask.contiguous()
    mp = None if mask is None else mask.data_ptr()
    row_start = torch.empty(n, H + 1, dtype=torch.int32, device=f.device)
    count = torch.empty(n, dtype=torch.int32, device=f.device)
    with torch.cuda.device(f.device):
        check(lib.tpiv_particle_count(f.data_ptr(), n, H, W, int(level), mp, row_start.data_ptr(), count.data_ptr(), _stream()))
        cap = int(count.max()) if capacity is None and n else int(capacity or 0)      # (the one host read)
        x = torch.empty(n, cap, dtype=torch.float64, device=f.device)
        y = torch.empty_like(x)
        peak = torch.empty(n, cap, dtype=torch.uint8, device=f.device)
        if n and cap:
            check(lib.tpiv_particle_detect(f.data_ptr(), n, H, W, int(level), mp, _particle_table_on(f.device).data_ptr(),
                                           row_start.data_ptr(), cap, x.data_ptr(), y.data_ptr(), peak.data_ptr(), _stream()))
    return Particles(x[0], y[0], peak[0], row_start[0], count[0]) if flat else Particles(x, y, peak, row_start, count)


def particle_match(pa, pb, up, vp, xc, yc, radius, shape):
    """Pairs the particle images pa of frame a with pb of frame b (Particles of particle_detect, of n frames each or of
    one) through a predictor (tpiv_particle_match).  up, vp float64 [n, n_rows, n_cols] (or [n_rows, n_cols]) on the GPU: the
    predicted displacement in pixels in image orientation -- u along the columns, v along the rows downward, row 0 the top
    row of windows: a plan's raw field, before the delivered flip and sign -- at the window centres xc [n_cols], yc [n_rows]
    (host sequences, image coordinates, strictly ascending); between the centres it is interpolated bilinearly, outside
    them held constant.  radius: pixels, > 0.  shape: (H, W) of the frames.  A particle of a is matched to the particle of b
    nearest to its predicted position within the radius (the bound inclusive; ties to the lower index), one-to-one: a
    particle of b goes to its nearest claimant (ties to the lower index).  Returns Matches(match, status, d2, matched):
    match int32 [n, capacity of pa] (index into pb's list, -1 unmatched), status uint8 (PARTICLE_STATUS: 0 matched, 1 no
    candidate, 2 lost the candidate to a nearer claimant, 3 predicted outside the frame, 255 behind the list's end), d2
    float64 (squared distance to the nearest candidate at status 0 and 2, NaN otherwise), matched int32 [n].  The result
    does not depend on scheduling.  The inputs are not written."""
    if not isinstance(pa, Particles) or not isinstance(pb, Particles):
        raise TypeError("particle_match: pa, pb are the Particles of particle_detect")
    _need_cuda(pa.x, pb.x, up, vp)
    if not isinstance(up, torch.Tensor) or not isinstance(vp, torch.Tensor) or up.dtype != torch.float64 or vp.dtype != torch.float64:
        raise TypeError("particle_match: up, vp float64")
    flat = pa.x.dim() == 1
    if (pb.x.dim() == 1) != flat or up.dim() != (2 if flat else 3) or up.shape != vp.shape:
        raise ValueError("particle_match: lists of n frames with up, vp [n, n_rows, n_cols], or of one frame with [n_rows, n_cols]")
    if flat:
        pa, pb = Particles(*(t[None] for t in pa)), Particles(*(t[None] for t in pb))
        up, vp = up[None], vp[None]
    H, W = (int(s) for s in shape)
    n, cap_a = pa.x.shape
    cap_b = pb.x.shape[1]
    for p in (pa, pb):
        if p.x.dtype != torch.float64 or p.y.dtype != torch.float64 or p.row_start.dtype != torch.int32:
            raise TypeError("particle_match: x, y float64 and row_start int32")
        if p.x.shape != p.y.shape or p.x.shape[0] != n or tuple(p.row_start.shape) != (n, H + 1):
            raise ValueError(f"particle_match: lists of {n} frames of shape ({H}, {W}): x, y [n, capacity], row_start [n, {H + 1}]")
    if up.shape[0] != n:
        raise ValueError(f"particle_match: up, vp must hold {n} fields, got {up.shape[0]}")
    xc = np.ascontiguousarray(xc, dtype=np.float64).reshape(-1)
    yc = np.ascontiguousarray(yc, dtype=np.float64).reshape(-1)
    if (yc.size, xc.size) != tuple(up.shape[1:]):
        raise ValueError(f"particle_match: {yc.size} x {xc.size} window centres for fields {tuple(up.shape[1:])}")
    if not (np.all(np.diff(xc) > 0) and np.all(np.diff(yc) > 0) and np.isfinite(xc).all() and np.isfinite(yc).all()):
        raise ValueError("particle_match: xc, yc must be finite and strictly ascending")
    if not is_real(radius) or not radius > 0 or radius == float("inf"):
        raise ValueError(f"particle_match: radius must be a positive number (pixels), got {radius!r}")
    dev = pa.x.device
    if any(t.device != dev for t in (pa.y, pa.row_start, pb.x, pb.y, pb.row_start, up, vp)):
        raise ValueError("particle_match: every tensor on one device")
    xa, ya, rsa = pa.x.contiguous(), pa.y.contiguous(), pa.row_start.contiguous()
    xb, yb, rsb = pb.x.contiguous(), pb.y.contiguous(), pb.row_start.contiguous()
    up, vp = up.contiguous(), vp.contiguous()
    centres = torch.from_numpy(np.concatenate([xc, yc])).to(dev)
    match = torch.empty(n, cap_a, dtype=torch.int32, device=dev)
    status = torch.empty(n, cap_a, dtype=torch.uint8, device=dev)
    d2 = torch.empty(n, cap_a, dtype=torch.float64, device=dev)
    matched = torch.empty(n, dtype=torch.int32, device=dev)
    work = torch.empty(2 * n * cap_b, dtype=torch.int64, device=dev)

    def ptr(t):
        return t.data_ptr() if t.numel() else None
    with torch.cuda.device(dev):
        if n:
            check(lib.tpiv_particle_match(ptr(xa), ptr(ya), rsa.data_ptr(), cap_a, ptr(xb), ptr(yb), rsb.data_ptr(), cap_b, n,
                                          H, W, up.data_ptr(), vp.data_ptr(), yc.size, xc.size, centres.data_ptr(),
                                          centres[xc.size:].data_ptr(), float(radius), ptr(match), ptr(status), ptr(d2),
                                          ptr(matched), ptr(work), work.numel() * 8, _stream()))
    return Matches(match[0], status[0], d2[0], matched[0]) if flat else Matches(match, status, d2, matched)


def uncertainty(a, b, u, v, ws, ov, invalid=None, radius=3, want_stats=False):
    """Correlation-statistics uncertainty (Wieneke 2015; tpiv_uncertainty) of fields u, v float64 [batch, n_rows, n_cols] (or
    [n_rows, n_cols]) at geometry (ws, ov) on frames a, b uint8 [batch, H, W] (or [H, W]) on the GPU: the 1-sigma random
    error of every vector in pixels, NaN where the correlation peak gives none, where u or v is not finite and where
    invalid (uint8, optional) is non-zero.  Returns (su, sv), with want_stats also the exact integer sums int64
    [batch, n_rows, n_cols, 8] = C0, S2x, S00x, varx, S2y, S00y, vary, nx + 256 ny.  The inputs are not written."""
    a, b = _frames(a, b)
    _need_cuda(u, v, invalid)
    if u.dtype != torch.float64 or v.dtype != torch.float64 or (invalid is not None and invalid.dtype != torch.uint8):
        raise TypeError("uncertainty: u, v float64 and invalid uint8")
    if u.dim() == 2:
        u, v = u[None], v[None]
        invalid = None if invalid is None else invalid[None]
    B, H, W = a.shape
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)):
        raise ValueError(f"uncertainty: radius must be an integer, got {radius!r}")
    if isinstance(ws, (int, np.integer)) and isinstance(ov, (int, np.integer)) and 0 <= ov < ws <= min(H, W):
        nr, nc = (H - ws) // (ws - ov) + 1, (W - ws) // (ws - ov) + 1
        if tuple(u.shape) != (B, nr, nc) or v.shape != u.shape or (invalid is not None and invalid.shape != u.shape):
            raise ValueError(f"uncertainty: fields must be [{B}, {nr}, {nc}] for these frames, got {tuple(u.shape)}")
    u, v = u.contiguous(), v.contiguous()
    invalid = None if invalid is None else invalid.contiguous()
    su, sv = torch.empty_like(u), torch.empty_like(v)
    stats = torch.empty(*u.shape, 8, dtype=torch.int64, device=u.device) if want_stats else None
    with torch.cuda.device(a.device):
        check(lib.tpiv_uncertainty(a.data_ptr(), b.data_ptr(), B, H, W, int(ws), int(ov), u.data_ptr(), v.data_ptr(),
                                   None if invalid is None else invalid.data_ptr(), int(radius), su.data_ptr(),
                                   sv.data_ptr(), stats.data_ptr() if want_stats else None, _stream()))
    return (su, sv, stats) if want_stats else (su, sv)


def postval(u, v, inv):
    """Device part of the post-validation (PIVbackend.py:884-892) for a batch, IN PLACE on u, v
    (float64 [B, nr, nc]): border interpolation, ring / hole census, fills that do not depend on the
    Delaunay triangulation.  Returns (cls uint8 [B, nr, nc], counts int32 [B, 4] = holes, ring,
    ambiguous, general); see include/torchpiv_hip.h tpiv_postval."""
    _need_cuda(u, v, inv)
    if u.dtype != torch.float64 or v.dtype != torch.float64 or inv.dtype != torch.uint8:
        raise TypeError("postval: u, v float64 and invalid uint8")
    if not (u.is_contiguous() and v.is_contiguous() and inv.is_contiguous()) or u.dim() != 3 \
            or u.shape != v.shape or u.shape != inv.shape:
        raise ValueError("postval: contiguous [batch, n_rows, n_cols] tensors of one shape")
    B, nr, nc = u.shape
    cls = torch.empty(B, nr, nc, dtype=torch.uint8, device=u.device)
    counts = torch.empty(B, 4, dtype=torch.int32, device=u.device)
    with torch.cuda.device(u.device):
        check(lib.tpiv_postval(u.data_ptr(), v.data_ptr(), inv.data_ptr(), B, nr, nc, cls.data_ptr(),
                               counts.data_ptr(), _stream()))
    return cls, counts


def postval_compact(u, v, cls, counts):
    """After postval: the ring cells (with their u, v) and the hole cells of the pairs that need the host
    triangulation, packed pair after pair in np.argwhere order (tpiv_postval_compact).  Returns (offsets int32
    [2, B + 1], ring_rc int32 [R, 2], ring_uv float64 [R, 2], hole_rc int32 [Hc, 2]) with the capacities R = B *
    ceil(cells / 4), Hc = B * cells; the used prefixes are offsets[0, B] and offsets[1, B] entries long."""
    _need_cuda(u, v, cls, counts)
    B, nr, nc = u.shape
    cells = nr * nc
    offsets = torch.empty(2, B + 1, dtype=torch.int32, device=u.device)
    ring_rc = torch.empty(B * ((cells + 3) // 4), 2, dtype=torch.int32, device=u.device)
    ring_uv = torch.empty(B * ((cells + 3) // 4), 2, dtype=torch.float64, device=u.device)
    hole_rc = torch.empty(B * cells, 2, dtype=torch.int32, device=u.device)
    with torch.cuda.device(u.device):
        check(lib.tpiv_postval_compact(u.data_ptr(), v.data_ptr(), cls.data_ptr(), counts.data_ptr(), B, nr, nc,
                                       offsets.data_ptr(), ring_rc.data_ptr(), ring_uv.data_ptr(), hole_rc.data_ptr(),
                                       _stream()))
    return offsets, ring_rc, ring_uv, hole_rc


def finish_fields(u, v, scale, dt):
    """(flip(u, rows) * scale / dt * 1000, -flip(v, rows) * scale / dt * 1000) for a batch of float64 fields on the GPU,
    with the reference's expression (PIVbackend.py:894-898) evaluated left to right: bit-identical to numpy's."""
    _need_cuda(u, v)
    if u.dtype != torch.float64 or v.dtype != torch.float64 or u.shape != v.shape or u.dim() != 3 \
            or not (u.is_contiguous() and v.is_contiguous()):
        raise ValueError("finish_fields: two contiguous float64 tensors [batch, n_rows, n_cols] of one shape")
    B, nr, nc = u.shape
    fu, fv = torch.empty_like(u), torch.empty_like(v)
    with torch.cuda.device(u.device):
        check(lib.tpiv_finish_fields(u.data_ptr(), v.data_ptr(), B, nr, nc, float(scale), float(dt), fu.data_ptr(),
                                     fv.data_ptr(), _stream()))
    return fu, fv


def ensemble_moments(U, V):
    """(mean u, mean v, <u'u'>, <v'v'>, <u'v'>) of stacked fields U, V float64 [n, ...] on the GPU, accumulated in
    stack order like numpy (tpiv_ensemble_moments)."""
    _need_cuda(U, V)
    if U.dtype != torch.float64 or V.dtype != torch.float64 or U.shape != V.shape or U.dim() < 2 or U.shape[0] < 1:
        raise ValueError("ensemble_moments: two float64 stacks [n >= 1, ...] of one shape")
    U, V = U.contiguous(), V.contiguous()
    n, cells = U.shape[0], U[0].numel()
    out = torch.empty((5,) + tuple(U.shape[1:]), dtype=torch.float64, device=U.device)
    with torch.cuda.device(U.device):
        check(lib.tpiv_ensemble_moments(U.data_ptr(), V.data_ptr(), n, cells, out.data_ptr(), _stream()))
    return tuple(out.unbind(0))


def bmp_unpack(raw, desc, lut, H, W, out=None, background=None):
    """Device unpack of raw uncompressed BMP files (tpiv_bmp_unpack).  raw uint8 [bytes] on the GPU, desc
    int64 [n, 6] and lut uint8 [n, 256] (device), see include/torchpiv_hip.h.  Returns uint8 [n, H, W].
    background: uint8 [2, H, W] on the device -- every file leaves as max(px, bg) - bg with bg = background[desc[f][5] != 0],
    in the same pass (tpiv_bmp_unpack_bg)."""
    _need_cuda(raw, desc, lut, background)
    n = desc.shape[0]
    if desc.dtype != torch.int64 or lut.dtype != torch.uint8 or raw.dtype != torch.uint8 or tuple(desc.shape) != (n, 6) \
            or tuple(lut.shape) != (n, 256) or not (desc.is_contiguous() and lut.is_contiguous() and raw.is_contiguous()):
        raise ValueError("bmp_unpack: raw uint8 [bytes], desc int64 [n, 6], lut uint8 [n, 256], all contiguous")
    if out is None:
        out = torch.empty(n, H, W, dtype=torch.uint8, device=raw.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (n, H, W) or not out.is_contiguous() or out.device != raw.device:
        raise ValueError("bmp_unpack: out must be a contiguous uint8 [n, H, W] tensor on the same device")
    if background is not None and (background.dtype != torch.uint8 or tuple(background.shape) != (2, H, W)
                                   or not background.is_contiguous() or background.device != raw.device):
        raise ValueError("bmp_unpack: background must be a contiguous uint8 [2, H, W] tensor on the same device")
    with torch.cuda.device(raw.device):
        if background is None:
            check(lib.tpiv_bmp_unpack(raw.data_ptr(), desc.data_ptr(), lut.data_ptr(), n, H, W, out.data_ptr(), _stream()))
        else:
            check(lib.tpiv_bmp_unpack_bg(raw.data_ptr(), desc.data_ptr(), lut.data_ptr(), n, H, W, background.data_ptr(),
                                         out.data_ptr(), _stream()))
    return out


def _images(frames, name):
    """uint8 frames [n, H, W] or [H, W] on the device, contiguous -> (frames [n, H, W], H, W)."""
    _need_cuda(frames)
    if frames.dtype != torch.uint8 or frames.dim() not in (2, 3) or not frames.is_contiguous():
        raise ValueError(f"{name}: frames must be a contiguous uint8 tensor [n, H, W] or [H, W]")
    f3 = frames[None] if frames.dim() == 2 else frames
    return f3, int(f3.shape[1]), int(f3.shape[2])


def frame_min(frames, acc=None):
    """Per-pixel minimum of uint8 frames [n, H, W] on the device, folded into acc uint8 [H, W] (updated in place and
    returned; None: a fresh one, i.e. the minimum of these frames alone).  Calls over parts of a recording compose:
    frame_min(B, frame_min(A)) == frame_min(cat(A, B)) (tpiv_frame_min)."""
    f, H, W = _images(frames, "frame_min")
    if acc is None:
        acc = torch.full((H, W), 255, dtype=torch.uint8, device=f.device)
    elif acc.dtype != torch.uint8 or tuple(acc.shape) != (H, W) or not acc.is_contiguous() or acc.device != f.device:
        raise ValueError("frame_min: acc must be a contiguous uint8 [H, W] tensor on the frames' device")
    with torch.cuda.device(f.device):
        check(lib.tpiv_frame_min(f.data_ptr(), f.shape[0], H * W, acc.data_ptr(), _stream()))
    return acc


def subtract_background(frames, bg, out=None):
    """max(frames, bg) - bg (frame minus background, clamped at 0) for uint8 frames [n, H, W] or [H, W] on the device
    and a background bg uint8 [H, W].  out: a tensor of the frames' shape to write into -- frames itself (in place) or
    memory that does not overlap them; None: a fresh one (tpiv_subtract_background)."""
    f, H, W = _images(frames, "subtract_background")
    _need_cuda(bg, out)
    if bg.dtype != torch.uint8 or tuple(bg.shape) != (H, W) or not bg.is_contiguous() or bg.device != f.device:
        raise ValueError("subtract_background: bg must be a contiguous uint8 [H, W] tensor on the frames' device")
    if out is None:
        out = torch.empty_like(frames)
    elif out.dtype != torch.uint8 or out.shape != frames.shape or not out.is_contiguous() or out.device != f.device:
        raise ValueError("subtract_background: out must be a contiguous uint8 tensor of the frames' shape and device")
    with torch.cuda.device(f.device):
        check(lib.tpiv_subtract_background(f.data_ptr(), f.shape[0], H * W, bg.data_ptr(), out.data_ptr(), _stream()))
    return out


def _mask_image(mask, H, W, device, name):
    _need_cuda(mask)
    if mask.dtype != torch.uint8 or tuple(mask.shape) != (H, W) or not mask.is_contiguous() or mask.device != device:
        raise ValueError(f"{name}: mask must be a contiguous uint8 [H, W] tensor of the frame shape on the frames' device")


def apply_mask(frames, mask, out=None):
    """mask != 0 ? 0 : frames for uint8 frames [n, H, W] or [H, W] on the device and a mask image uint8 [H, W] (any
    non-zero byte masks).  out: a tensor of the frames' shape to write into -- frames itself (in place) or memory that
    does not overlap them; None: a fresh one (tpiv_apply_mask)."""
    f, H, W = _images(frames, "apply_mask")
    _need_cuda(out)
    _mask_image(mask, H, W, f.device, "apply_mask")
    if out is None:
        out = torch.empty_like(frames)
    elif out.dtype != torch.uint8 or out.shape != frames.shape or not out.is_contiguous() or out.device != f.device:
        raise ValueError("apply_mask: out must be a contiguous uint8 tensor of the frames' shape and device")
    with torch.cuda.device(f.device):
        check(lib.tpiv_apply_mask(f.data_ptr(), f.shape[0], H * W, mask.data_ptr(), out.data_ptr(), _stream()))
    return out


def mask_coverage(mask, ws, ov):
    """int32 [n_rows, n_cols]: the masked (non-zero) pixels of mask uint8 [H, W] (on the device) inside every window of
    the (ws, ov) grid of field_shape (tpiv_mask_coverage)."""
    _need_cuda(mask)
    if mask.dim() != 2:
        raise ValueError("mask_coverage: mask must be a contiguous uint8 [H, W] tensor")
    H, W = int(mask.shape[0]), int(mask.shape[1])
    _mask_image(mask, H, W, mask.device, "mask_coverage")
    nr, nc = C.c_int(), C.c_int()
    check(lib.tpiv_field_shape(H, W, int(ws), int(ov), C.byref(nr), C.byref(nc)))
    count = torch.empty(max(nr.value, 0), max(nc.value, 0), dtype=torch.int32, device=mask.device)
    with torch.cuda.device(mask.device):
        check(lib.tpiv_mask_coverage(mask.data_ptr(), H, W, int(ws), int(ov), count.data_ptr(), _stream()))
    return count


def mask_fields(u, v, inv, grid, invalid_value, status=None):
    """IN PLACE on u, v float64 and inv uint8 [batch, n_rows, n_cols] (contiguous, on the device): wherever grid (uint8 or
    bool [n_rows, n_cols]) is non-zero, u = v = +0.0, inv = invalid_value (0 or 1) and, with a status map (uint8, the
    fields' shape), status = 2 (tpiv_mask_fields).  Returns (u, v, inv) or (u, v, inv, status)."""
    _need_cuda(u, v, inv, grid, status)
    if u.dtype != torch.float64 or v.dtype != torch.float64 or inv.dtype != torch.uint8:
        raise TypeError("mask_fields: u, v float64 and invalid uint8")
    if not (u.is_contiguous() and v.is_contiguous() and inv.is_contiguous()) or u.dim() != 3 \
            or u.shape != v.shape or u.shape != inv.shape:
        raise ValueError("mask_fields: contiguous [batch, n_rows, n_cols] tensors of one shape")
    B, nr, nc = u.shape
    if grid.dtype not in (torch.uint8, torch.bool) or tuple(grid.shape) != (nr, nc) or grid.device != u.device:
        raise ValueError("mask_fields: grid must be a uint8 or bool [n_rows, n_cols] tensor on the fields' device")
    g = grid.to(torch.uint8).contiguous()
    if status is not None and (status.dtype != torch.uint8 or status.shape != u.shape or not status.is_contiguous()
                               or status.device != u.device):
        raise ValueError("mask_fields: status must be a contiguous uint8 tensor of the fields' shape and device")
    with torch.cuda.device(u.device):
        check(lib.tpiv_mask_fields(u.data_ptr(), v.data_ptr(), inv.data_ptr(), None if status is None else status.data_ptr(),
                                   g.data_ptr(), B, nr, nc, int(invalid_value), _stream()))
    return (u, v, inv) if status is None else (u, v, inv, status)


def dynamic_mask(a, b, kind, size, level, grow=0, static=None, out=None, work=None):
    """One mask per pair, uint8 [n, H, W] of bytes 0 / 1, segmented from the frames a, b uint8 [n, H, W] or [H, W] on the
    device (tpiv_dynamic_mask: an erosion and a dilation kernel; the definition is in include/torchpiv_hip.h): the
    opening by the size x size square of {frame >= level} ("bright") or {frame <= level} ("dark"), grown by `grow`, of
    both frames, OR-ed with static (uint8 [H, W], non-zero = masked; None: nothing).  The frames may be any view (one that
    is not contiguous is copied first).  out: a contiguous uint8 tensor [n, H, W] that overlaps no input; None: a fresh
    one.  work: a uint8 workspace of at least n * H * W bytes to reuse from call to call (None: a fresh one)."""
    par = dynamic_mask_arg({"kind": kind, "size": size, "level": level, "grow": grow})
    _need_cuda(a, b, static, out, work)
    if a.dtype != torch.uint8 or b.dtype != torch.uint8 or a.dim() not in (2, 3) or a.shape != b.shape \
            or a.device != b.device:
        raise ValueError("dynamic_mask: a, b must be uint8 tensors [n, H, W] or [H, W] of one shape on one device")
    fa, fb = (t if t.is_contiguous() else t.contiguous() for t in (a, b))
    if fa.dim() == 2:
        fa, fb = fa[None], fb[None]
    n, H, W = (int(s) for s in fa.shape)
    if static is not None:
        _mask_image(static, H, W, fa.device, "dynamic_mask")
    if out is None:
        out = torch.empty(n, H, W, dtype=torch.uint8, device=fa.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (n, H, W) or not out.is_contiguous() or out.device != fa.device:
        raise ValueError("dynamic_mask: out must be a contiguous uint8 [n, H, W] tensor on the frames' device")
    need = n * H * W
    if work is None:
        work = torch.empty(max(need, 16), dtype=torch.uint8, device=fa.device)
    elif work.dtype != torch.uint8 or work.dim() != 1 or not work.is_contiguous() or work.device != fa.device \
            or work.numel() < need:
        raise ValueError(f"dynamic_mask: work must be a contiguous uint8 vector of at least {need} bytes on the frames' device")
    with torch.cuda.device(fa.device):
        check(lib.tpiv_dynamic_mask(fa.data_ptr(), fb.data_ptr(), n, H, W, _lib.DYNMASKS[par["kind"]], par["size"],
                                    par["level"], par["grow"], None if static is None else static.data_ptr(),
                                    out.data_ptr(), work.data_ptr(), _stream()))
    return out


def _mask_stack(masks, f, name):
    _need_cuda(masks)
    if masks.dtype != torch.uint8 or masks.shape != f.shape or not masks.is_contiguous() or masks.device != f.device:
        raise ValueError(f"{name}: masks must be a contiguous uint8 tensor of the frames' shape [n, H, W] on their device")


def apply_mask_pairs(frames, masks, out=None):
    """masks != 0 ? 0 : frames for uint8 frames [n, H, W] on the device and one mask per frame, uint8 [n, H, W] (any
    non-zero byte masks).  out: frames itself (in place) or memory that overlaps neither; None: a fresh tensor
    (tpiv_apply_mask_pairs)."""
    f, H, W = _images(frames, "apply_mask_pairs")
    if frames.dim() != 3:
        raise ValueError("apply_mask_pairs: frames must be a contiguous uint8 tensor [n, H, W]")
    _need_cuda(out)
    _mask_stack(masks, f, "apply_mask_pairs")
    if out is None:
        out = torch.empty_like(frames)
    elif out.dtype != torch.uint8 or out.shape != frames.shape or not out.is_contiguous() or out.device != f.device:
        raise ValueError("apply_mask_pairs: out must be a contiguous uint8 tensor of the frames' shape and device")
    with torch.cuda.device(f.device):
        check(lib.tpiv_apply_mask_pairs(f.data_ptr(), f.shape[0], H * W, masks.data_ptr(), out.data_ptr(), _stream()))
    return out


def mask_coverage_pairs(masks, ws, ov):
    """int32 [n, n_rows, n_cols]: the masked (non-zero) pixels of every mask of masks uint8 [n, H, W] (on the device)
    inside every window of the (ws, ov) grid of field_shape (tpiv_mask_coverage_pairs)."""
    _need_cuda(masks)
    if masks.dim() != 3 or masks.dtype != torch.uint8 or not masks.is_contiguous():
        raise ValueError("mask_coverage_pairs: masks must be a contiguous uint8 [n, H, W] tensor")
    n, H, W = (int(s) for s in masks.shape)
    nr, nc = C.c_int(), C.c_int()
    check(lib.tpiv_field_shape(H, W, int(ws), int(ov), C.byref(nr), C.byref(nc)))
    count = torch.empty(n, max(nr.value, 0), max(nc.value, 0), dtype=torch.int32, device=masks.device)
    with torch.cuda.device(masks.device):
        check(lib.tpiv_mask_coverage_pairs(masks.data_ptr(), n, H, W, int(ws), int(ov), count.data_ptr(), _stream()))
    return count


def mask_fields_pairs(u, v, inv, grids, invalid_value, status=None):
    """mask_fields with one grid per pair: grids uint8 or bool [batch, n_rows, n_cols], the fields' shape
    (tpiv_mask_fields_pairs).  IN PLACE; returns (u, v, inv) or (u, v, inv, status)."""
    _need_cuda(u, v, inv, grids, status)
    if u.dtype != torch.float64 or v.dtype != torch.float64 or inv.dtype != torch.uint8:
        raise TypeError("mask_fields_pairs: u, v float64 and invalid uint8")
    if not (u.is_contiguous() and v.is_contiguous() and inv.is_contiguous()) or u.dim() != 3 \
            or u.shape != v.shape or u.shape != inv.shape:
        raise ValueError("mask_fields_pairs: contiguous [batch, n_rows, n_cols] tensors of one shape")
    B, nr, nc = u.shape
    if grids.dtype not in (torch.uint8, torch.bool) or grids.shape != u.shape or grids.device != u.device:
        raise ValueError("mask_fields_pairs: grids must be a uint8 or bool tensor of the fields' shape on their device")
    g = grids.to(torch.uint8).contiguous()
    if status is not None and (status.dtype != torch.uint8 or status.shape != u.shape or not status.is_contiguous()
                               or status.device != u.device):
        raise ValueError("mask_fields_pairs: status must be a contiguous uint8 tensor of the fields' shape and device")
    with torch.cuda.device(u.device):
        check(lib.tpiv_mask_fields_pairs(u.data_ptr(), v.data_ptr(), inv.data_ptr(),
                                         None if status is None else status.data_ptr(), g.data_ptr(), B, nr, nc,
                                         int(invalid_value), _stream()))
    return (u, v, inv) if status is None else (u, v, inv, status)


def prefilter(frames, kind, size=None, cap=None, background=None, out=None):
    """Spatial pre-filter of uint8 frames [n, H, W] or [H, W] on the device, one launch (tpiv_prefilter): with g = max(f,
    background) - background (g = f without one, background uint8 [H, W]) and the size x size neighbourhood clipped to
    the image, kind "min": g - min(neighbourhood), "mean": max(g - rounded mean(neighbourhood), 0), None: g; then
    min(., cap).  out: a tensor of the frames' shape that does not overlap them (the filter is a stencil: never in
    place); None: a fresh one.  The frames are not written."""
    par = prefilter_arg({"kind": kind, "size": size, "cap": cap})
    f, H, W = _images(frames, "prefilter")
    _need_cuda(background, out)
    if background is not None and (background.dtype != torch.uint8 or tuple(background.shape) != (H, W)
                                   or not background.is_contiguous() or background.device != f.device):
        raise ValueError("prefilter: background must be a contiguous uint8 [H, W] tensor on the frames' device")
    if out is None:
        out = torch.empty_like(frames)
    elif out.dtype != torch.uint8 or out.shape != frames.shape or not out.is_contiguous() or out.device != f.device:
        raise ValueError("prefilter: out must be a contiguous uint8 tensor of the frames' shape and device")
    with torch.cuda.device(f.device):
        check(lib.tpiv_prefilter(f.data_ptr(), f.shape[0], H, W, None if background is None else background.data_ptr(),
                                 _lib.PREFILTERS[par["kind"]], par["size"] or 0, par["cap"] or 255, out.data_ptr(),
                                 _stream()))
    return out


def equalize_grid(H, W, tile):
    """(ky, kx): the tiles of tpiv_equalize along y and x for frames of H x W."""
    return tuple(max(1, (2 * n + tile) // (2 * tile)) for n in (int(H), int(W)))


def equalize(frames, tile=EQUALIZE_DEFAULTS["tile"], clip=EQUALIZE_DEFAULTS["clip"], out=None, return_luts=False, work=None):
    """Tile-wise adaptive histogram equalization of uint8 frames [n, H, W] or [H, W] on the device (tpiv_equalize: a table
    kernel and a map kernel; the definition is in include/torchpiv_hip.h).  tile, clip: as in equalize_arg.  The frames
    may be any view (one that is not contiguous is copied first).  out: a contiguous tensor of the frames' shape -- the
    frames themselves (in place) or memory that does not overlap them; None: a fresh one.  work: a uint8 workspace of at
    least n * ky * kx * 256 bytes to reuse from call to call (None: a fresh one).  return_luts: also return the tables,
    uint8 [n, ky, kx, 256] (a view of the workspace)."""
    par = equalize_arg({"tile": tile, "clip": clip})
    _need_cuda(frames, out, work)
    if frames.dtype != torch.uint8 or frames.dim() not in (2, 3):
        raise ValueError("equalize: frames must be a uint8 tensor [n, H, W] or [H, W]")
    src = frames if frames.is_contiguous() else frames.contiguous()
    f = src[None] if src.dim() == 2 else src
    n, H, W = (int(s) for s in f.shape)
    if out is None:
        out = torch.empty_like(src)
    elif out.dtype != torch.uint8 or out.shape != frames.shape or not out.is_contiguous() or out.device != f.device:
        raise ValueError("equalize: out must be a contiguous uint8 tensor of the frames' shape and device")
    ky, kx = equalize_grid(H, W, par["tile"])
    need = n * ky * kx * 256
    if work is None:
        work = torch.empty(max(need, 16), dtype=torch.uint8, device=f.device)
    elif work.dtype != torch.uint8 or work.dim() != 1 or not work.is_contiguous() or work.device != f.device \
            or work.numel() < need:
        raise ValueError(f"equalize: work must be a contiguous uint8 vector of at least {need} bytes on the frames' device")
    with torch.cuda.device(f.device):
        check(lib.tpiv_equalize(f.data_ptr(), n, H, W, par["tile"], par["clip_q8"], out.data_ptr(), work.data_ptr(),
                                work.numel(), _stream()))
    if return_luts:
        return out, work[:need].view(n, ky, kx, 256)
    return out


def depth_lut(lo, hi, curve="linear"):
    """The tone-map table of a range: numpy uint8 [65536] with, for c = clip(v, lo, hi) - lo and d = hi - lo, "linear":
    (c * 510 + d) // (2 * d) -- 255 c / d rounded half up, in int64 --, "sqrt": floor(255 * sqrt(c / d) + 0.5) in float64.
    Monotone, 0 up to lo and 255 from hi on.  lo, hi: integers, 0 <= lo < hi <= 65535."""
    par = depth_arg({"lo": lo, "hi": hi, "curve": curve})
    lo, hi = par["lo"], par["hi"]
    c = np.clip(np.arange(DEPTH_BINS, dtype=np.int64), lo, hi) - lo
    d = hi - lo
    if par["curve"] == "linear":
        return ((c * 510 + d) // (2 * d)).astype(np.uint8)
    return np.floor(255.0 * np.sqrt(c.astype(np.float64) / np.float64(d)) + 0.5).astype(np.uint8)


def depth_range(hist, clip_low=0.0, clip_high=1e-4):
    """(lo, hi) of a 65536-bin histogram of N > 0 samples (numpy, no GPU): lo = the largest l with count(v < l) <=
    floor(clip_low * N), hi = the smallest h with count(v > h) <= floor(clip_high * N) -- the range that leaves at most
    those fractions of the samples clipped at either end.  hi <= lo (a constant recording) gives hi = lo + 1, and
    (65534, 65535) at lo = 65535."""
    h = np.asarray(hist)
    if h.shape != (DEPTH_BINS,) or h.dtype.kind not in "iu":
        raise ValueError(f"depth_range: hist must be an integer array of shape ({DEPTH_BINS},)")
    for name, c in (("clip_low", clip_low), ("clip_high", clip_high)):
        if isinstance(c, bool) or not 0 <= c < 0.5:
            raise ValueError(f"depth_range: {name} must be a fraction in [0, 0.5), got {c!r}")
    h = h.astype(np.int64)
    if (h < 0).any():
        raise ValueError("depth_range: negative count")
    N = int(h.sum())
    if N <= 0:
        raise ValueError("depth_range: the histogram is empty")
    cum = np.cumsum(h)
    below = np.concatenate([[0], cum[:-1]])              # count(v < l), non-decreasing in l
    above = N - cum                                      # count(v > h), non-increasing in h
    lo = int(np.count_nonzero(below <= int(np.floor(clip_low * N)))) - 1
    hi = int(np.argmax(above <= int(np.floor(clip_high * N))))
    if hi <= lo:
        lo, hi = (DEPTH_BINS - 2, DEPTH_BINS - 1) if lo == DEPTH_BINS - 1 else (lo, lo + 1)
    return lo, hi


def depth_sample(n, sample):
    """The pairs of a recording of n pairs whose frames feed the histogram of depth="auto": min(n, sample) positions spread
    evenly over 0 .. n - 1."""
    if n <= 0:
        return np.zeros(0, dtype=int)
    return np.unique(np.rint(np.linspace(0, n - 1, min(n, int(sample)))).astype(int))


def _deep_frames(frames, name):
    """uint16 frames [n, H, W] or [H, W] on the device, contiguous -> (frames [n, H, W], H, W)."""
    _need_cuda(frames)
    if frames.dtype != torch.uint16 or frames.dim() not in (2, 3) or not frames.is_contiguous():
        raise ValueError(f"{name}: frames must be a contiguous uint16 tensor [n, H, W] or [H, W]")
    f3 = frames[None] if frames.dim() == 2 else frames
    return f3, int(f3.shape[1]), int(f3.shape[2])


def depth_histogram(frames, acc=None):
    """Exact counts of all 65536 values of uint16 frames [n, H, W] (or [H, W]) on the device, added into acc int64 [65536]
    (updated in place and returned; None: a fresh one of zeros).  Calls over parts of a recording compose:
    depth_histogram(B, depth_histogram(A)) is the histogram of cat(A, B) (tpiv_depth_histogram).  The frames are not written."""
    f, H, W = _deep_frames(frames, "depth_histogram")
    if acc is None:
        acc = torch.zeros(DEPTH_BINS, dtype=torch.int64, device=f.device)
    elif not isinstance(acc, torch.Tensor) or acc.dtype != torch.int64 or tuple(acc.shape) != (DEPTH_BINS,) \
            or not acc.is_contiguous() or acc.device != f.device:
        raise ValueError(f"depth_histogram: acc must be a contiguous int64 [{DEPTH_BINS}] tensor on the frames' device")
    with torch.cuda.device(f.device):
        check(lib.tpiv_depth_histogram(f.data_ptr(), f.shape[0], H * W, acc.data_ptr(), _stream()))
    return acc


def _overlap(a, a_bytes, b, b_bytes):
    return a.data_ptr() < b.data_ptr() + b_bytes and b.data_ptr() < a.data_ptr() + a_bytes


def depth_map(frames, lut, offsets=None, shape=None, out=None):
    """Tone map on the device, one launch: out = lut[frames] as uint8 (tpiv_depth_map).  frames: a contiguous uint16
    tensor [n, H, W] or [H, W]; or, the staged form, a flat uint16 buffer with offsets (int64 [n]: the element offset of
    every frame in the buffer; a tensor, array or list -- checked on the host, so hand over host values where a
    synchronisation matters) and shape = (H, W): frame f of the result is the H * W samples from offsets[f] on, in the
    order given (the interleaved slots of a staged batch leave as two contiguous stacks).  lut: uint8 [65536] on the
    frames' device (depth_lut, or any table).  out: a contiguous uint8 tensor of the result's shape that overlaps neither
    the source nor the table; None: a fresh one.  An overlap is refused and nothing is launched.  The source is not written."""
    _need_cuda(frames)
    if not isinstance(lut, torch.Tensor) or lut.dtype != torch.uint8 or tuple(lut.shape) != (DEPTH_BINS,) \
            or not lut.is_contiguous() or lut.device != frames.device:
        raise ValueError(f"depth_map: lut must be a contiguous uint8 [{DEPTH_BINS}] tensor on the frames' device")
    if offsets is None:
        if shape is not None:
            raise ValueError("depth_map: shape goes with offsets (the frames carry their own)")
        f, H, W = _deep_frames(frames, "depth_map")
        n, off_d, out_shape = int(f.shape[0]), None, tuple(frames.shape)
    else:
        if frames.dtype != torch.uint16 or frames.dim() != 1 or not frames.is_contiguous():
            raise ValueError("depth_map: with offsets, frames must be a flat contiguous uint16 buffer")
        try:
            H, W = (int(s) for s in shape)
        except (TypeError, ValueError):
            raise ValueError(f"depth_map: with offsets, shape = (H, W) is needed, got {shape!r}") from None
        if H < 1 or W < 1:
            raise ValueError(f"depth_map: shape must be positive, got {(H, W)}")
        off_h = offsets.detach().cpu() if isinstance(offsets, torch.Tensor) else torch.as_tensor(np.asarray(offsets))
        if off_h.dtype != torch.int64 or off_h.dim() != 1:
            raise ValueError("depth_map: offsets must be int64 [n]")
        n = int(off_h.shape[0])
        if n and (int(off_h.min()) < 0 or int(off_h.max()) + H * W > frames.numel()):
            raise ValueError(f"depth_map: a frame of {H} x {W} samples at offsets {int(off_h.min())}..{int(off_h.max())} "
                             f"leaves the buffer of {frames.numel()} samples")
        f = frames
        off_d = offsets if isinstance(offsets, torch.Tensor) and offsets.device == frames.device and offsets.is_contiguous() \
            else off_h.contiguous().to(frames.device, non_blocking=True)
        out_shape = (n, H, W)
    if out is None:
        out = torch.empty(out_shape, dtype=torch.uint8, device=frames.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != tuple(out_shape) \
            or not out.is_contiguous() or out.device != frames.device:
        raise ValueError(f"depth_map: out must be a contiguous uint8 tensor of shape {tuple(out_shape)} on the frames' device")
    if _overlap(out, out.numel(), f, 2 * f.numel()):
        raise ValueError("depth_map: out overlaps the source frames")
    if _overlap(out, out.numel(), lut, DEPTH_BINS):
        raise ValueError("depth_map: out overlaps the table")
    with torch.cuda.device(frames.device):
        check(lib.tpiv_depth_map(f.data_ptr(), None if off_d is None else off_d.data_ptr(), n, H, W, lut.data_ptr(),
                                 out.data_ptr(), _stream()))
    return out


def _dewarp_form(arg):
    par = dewarp_arg(arg)                    # (its own result passes unchanged)
    if par is None:
        raise ValueError("dewarp: no map given")
    return next(k for k in DEWARP_FORMS if k in par), par


def _poly_terms(xn, yn, K):
    terms = [np.ones_like(xn), xn, yn]
    if K >= 6:
        terms += [xn * xn, xn * yn, yn * yn]
    if K >= 10:
        terms += [xn * xn * xn, xn * xn * yn, xn * yn * yn, yn * yn * yn]
    return terms


def _normalised(x, y, H, W):
    xn = 2.0 * x / (W - 1) - 1.0 if W > 1 else np.zeros_like(x)
    yn = 2.0 * y / (H - 1) - 1.0 if H > 1 else np.zeros_like(y)
    return xn, yn


def dewarp_coords(arg, H, W):
    """(sx, sy): the source coordinates of every pixel of the rectified frame [H, W] under the dewarp= argument, float64
    numpy, before quantisation."""
    form, par = _dewarp_form(arg)
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"dewarp: frame shape must be positive, got {(H, W)}")
    if form == "map":
        xs, ys = par["map"]
        if xs.shape != (H, W):
            raise ValueError(f"dewarp: map of shape {xs.shape} for frames of shape {(H, W)}")
        return xs, ys
    y, x = np.mgrid[0:H, 0:W]
    x, y = x.astype(np.float64), y.astype(np.float64)
    if form == "homography":
        M = par["homography"]
        X = M[0, 0] * x + M[0, 1] * y + M[0, 2]
        Y = M[1, 0] * x + M[1, 1] * y + M[1, 2]
        D = M[2, 0] * x + M[2, 1] * y + M[2, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            return X / D, Y / D
    P = par["poly"]
    xn, yn = _normalised(x, y, H, W)
    sx, sy = np.zeros((H, W)), np.zeros((H, W))
    for k, t in enumerate(_poly_terms(xn, yn, P.shape[1])):
        sx = sx + P[0, k] * t
        sy = sy + P[1, k] * t
    return sx, sy


def dewarp_map(arg, H, W):
    """The backward map of tpiv_dewarp for frames of H x W: numpy int32 [H, W, 2], source x then source y in signed Q8,
    q = floor(s * 256 + 0.5) in float64.  An entry with qx < 0, qy < 0, qx > (W - 1) << 8 or qy > (H - 1) << 8, or with a
    non-finite coordinate, is outside and stored as (-1, -1).  arg: the dewarp= argument (dewarp_arg)."""
    H, W = int(H), int(W)
    if H > 1 << 22 or W > 1 << 22:
        raise ValueError(f"dewarp: frames of {(H, W)} are too large")
    sx, sy = dewarp_coords(arg, H, W)
    ok = np.isfinite(sx) & np.isfinite(sy)
    qx = np.floor(np.where(ok, sx, -1.0) * 256.0 + 0.5)
    qy = np.floor(np.where(ok, sy, -1.0) * 256.0 + 0.5)
    ok &= (qx >= 0) & (qy >= 0) & (qx <= (W - 1) * 256) & (qy <= (H - 1) * 256)
    m = np.full((H, W, 2), -1, dtype=np.int32)
    m[..., 0][ok] = qx[ok].astype(np.int32)
    m[..., 1][ok] = qy[ok].astype(np.int32)
    return m


def dewarp_outside(map):
    """bool [H, W]: the pixels the map int32 [H, W, 2] (numpy array or tensor) leaves to `fill` -- what to pass as mask=
    to keep them out of the fields."""
    m = map.detach().cpu().numpy() if isinstance(map, torch.Tensor) else np.asarray(map)
    if m.ndim != 3 or m.shape[2] != 2 or m.dtype != np.int32:
        raise ValueError("dewarp_outside: the map must be int32 [H, W, 2]")
    H, W = m.shape[:2]
    return (m[..., 0] < 0) | (m[..., 1] < 0) | (m[..., 0] > (W - 1) * 256) | (m[..., 1] > (H - 1) * 256)


def dewarp_cubic_table():
    """The weight table of tpiv_dewarp's cubic interpolation: numpy int16 [256, 4], row f = the Catmull-Rom weights (a =
    -0.5) of t = f / 256 on the taps -1, 0, 1, 2 in Q10, floor(c * 1024 + 0.5) (t and its powers are exact in float64), the
    remainder to 1024 added to weight 1 (f < 128) or 2 (f >= 128): every row sums to 1024, row 0 is (0, 1024, 0, 0), row f
    is row 256 - f reversed, and sum |w| <= 1280."""
    t = np.arange(256, dtype=np.float64) / 256.0
    c = np.stack([((2.0 - t) * t - 1.0) * t * 0.5, (1.5 * t - 2.5) * t * t + 1.0, ((2.0 - 1.5 * t) * t + 0.5) * t,
                  (0.5 * t - 0.5) * t * t], axis=1)
    T = np.floor(c * 1024.0 + 0.5).astype(np.int64)
    rest = 1024 - T.sum(axis=1)
    T[:128, 1] += rest[:128]
    T[128:, 2] += rest[128:]
    return T.astype(np.int16)


def _dewarp_check_map(m, H, W):
    """ValueError unless every entry of the numpy map int32 [H, W, 2] is inside the frame or the outside marker."""
    if m.dtype != np.int32 or m.shape != (H, W, 2):
        raise ValueError(f"dewarp: the map must be int32 [{H}, {W}, 2], got {m.dtype} {m.shape}")
    inside = (m[..., 0] >= 0) & (m[..., 1] >= 0) & (m[..., 0] <= (W - 1) * 256) & (m[..., 1] <= (H - 1) * 256)
    marker = (m[..., 0] == -1) & (m[..., 1] == -1)
    bad = ~(inside | marker)
    if bad.any():
        r, c = np.argwhere(bad)[0]
        raise ValueError(f"dewarp: illegal map entry {tuple(int(q) for q in m[r, c])} at pixel ({int(r)}, {int(c)}): neither "
                         f"inside the {H} x {W} frame nor the outside marker (-1, -1)")


_DEWARP_CHECKED = "_tpiv_dewarp_checked"
_DEWARP_TABLES = {}


def dewarp_upload(map, device):
    """The map (numpy int32 [H, W, 2], dewarp_map's) checked on the host and put on `device` once: the tensor dewarp()
    takes.  ValueError for an entry that is neither inside the frame nor the outside marker."""
    m = np.ascontiguousarray(map)
    if m.ndim != 3:
        raise ValueError("dewarp: the map must be int32 [H, W, 2]")
    _dewarp_check_map(m, m.shape[0], m.shape[1])
    t = torch.from_numpy(m).to(device)
    setattr(t, _DEWARP_CHECKED, t._version)
    return t


def _dewarp_table(device):
    """The cubic weight table on `device`, made once per device."""
    key = str(device)
    if key not in _DEWARP_TABLES:
        _DEWARP_TABLES[key] = torch.from_numpy(dewarp_cubic_table()).to(device)
    return _DEWARP_TABLES[key]


def dewarp(frames, map, interp="cubic", fill=0, offsets=None, shape=None, out=None):
    """Rectification on the device, one launch (tpiv_dewarp; the definition is in include/torchpiv_hip.h): every frame
    sampled through the backward map.  frames: a contiguous uint8 tensor [n, H, W] or [H, W]; or, the offsets form, a flat
    uint8 buffer with offsets (int64 [n]: the element offset of every frame in the buffer; a tensor, array or list,
    checked on the host) and shape = (H, W) -- frames addressed in any order, repeatedly, nothing gathered first.  map:
    int32 [H, W, 2] on the frames' device (dewarp_upload(dewarp_map(...))); a tensor that did not come from dewarp_upload
    is checked on the host at its first use (one copy down), and again only after it was written.  interp "cubic" or
    "linear", fill 0..255.  out: a contiguous uint8 tensor of the result's shape that overlaps none of the source, the map
    or the table; None: a fresh one.  An overlap is refused and nothing is launched.  The source is not written."""
    _need_cuda(frames)
    if not isinstance(interp, str) or interp not in _lib.DEWARP_INTERPS:
        raise ValueError(f"dewarp: interp must be one of {sorted(_lib.DEWARP_INTERPS)}, got {interp!r}")
    if isinstance(fill, (bool, np.bool_)) or not isinstance(fill, (int, np.integer)) or not 0 <= fill <= 255:
        raise ValueError(f"dewarp: fill must be an integer in 0..255, got {fill!r}")
    if frames.dtype != torch.uint8:
        raise ValueError(f"dewarp: frames must be uint8, got {frames.dtype}")
    if offsets is None:
        if shape is not None:
            raise ValueError("dewarp: shape goes with offsets (the frames carry their own)")
        f, H, W = _images(frames, "dewarp")
        n, off_d, out_shape = int(f.shape[0]), None, tuple(frames.shape)
    else:
        if frames.dim() != 1 or not frames.is_contiguous():
            raise ValueError("dewarp: with offsets, frames must be a flat contiguous uint8 buffer")
        try:
            H, W = (int(s) for s in shape)
        except (TypeError, ValueError):
            raise ValueError(f"dewarp: with offsets, shape = (H, W) is needed, got {shape!r}") from None
        if H < 1 or W < 1:
            raise ValueError(f"dewarp: shape must be positive, got {(H, W)}")
        off_h = offsets.detach().cpu() if isinstance(offsets, torch.Tensor) else torch.as_tensor(np.asarray(offsets))
        if off_h.dtype != torch.int64 or off_h.dim() != 1:
            raise ValueError("dewarp: offsets must be int64 [n]")
        n = int(off_h.shape[0])
        if n and (int(off_h.min()) < 0 or int(off_h.max()) + H * W > frames.numel()):
            raise ValueError(f"dewarp: a frame of {H} x {W} pixels at offsets {int(off_h.min())}..{int(off_h.max())} leaves "
                             f"the buffer of {frames.numel()} bytes")
        f = frames
        off_d = offsets if isinstance(offsets, torch.Tensor) and offsets.device == frames.device and offsets.is_contiguous() \
            else off_h.contiguous().to(frames.device, non_blocking=True)
        out_shape = (n, H, W)
    if not isinstance(map, torch.Tensor) or map.dtype != torch.int32 or tuple(map.shape) != (H, W, 2) \
            or not map.is_contiguous() or map.device != frames.device:
        raise ValueError(f"dewarp: map must be a contiguous int32 [{H}, {W}, 2] tensor on the frames' device")
    if getattr(map, _DEWARP_CHECKED, None) != map._version:
        _dewarp_check_map(map.cpu().numpy(), H, W)
        setattr(map, _DEWARP_CHECKED, map._version)
    table = _dewarp_table(frames.device)
    if out is None:
        out = torch.empty(out_shape, dtype=torch.uint8, device=frames.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != tuple(out_shape) \
            or not out.is_contiguous() or out.device != frames.device:
        raise ValueError(f"dewarp: out must be a contiguous uint8 tensor of shape {tuple(out_shape)} on the frames' device")
    if _overlap(out, out.numel(), f, f.numel()):
        raise ValueError("dewarp: out overlaps the source frames (a gather: never in place)")
    if _overlap(out, out.numel(), map, 4 * map.numel()):
        raise ValueError("dewarp: out overlaps the map")
    if _overlap(out, out.numel(), table, 2 * table.numel()):
        raise ValueError("dewarp: out overlaps the table")
    with torch.cuda.device(frames.device):
        check(lib.tpiv_dewarp(f.data_ptr(), None if off_d is None else off_d.data_ptr(), n, H, W, map.data_ptr(),
                              table.data_ptr(), _lib.DEWARP_INTERPS[interp], int(fill), out.data_ptr(), _stream()))
    return out


def _fields3(who, u, v, inv):
    _need_cuda(u, v, inv)
    if u.dtype != torch.float64 or v.dtype != torch.float64 or inv.dtype != torch.uint8:
        raise TypeError(f"{who}: u, v float64 and invalid uint8")
    if u.dim() != 3 or u.shape != v.shape or u.shape != inv.shape:
        raise ValueError(f"{who}: [batch, n_rows, n_cols] tensors of one shape")
    return u.contiguous(), v.contiguous(), inv.contiguous()


def deform_nodes(u, v, inv, smooth=True):
    """The Q8 half-shift nodes of a field (tpiv_deform_nodes; the definition is in include/torchpiv_hip.h): u, v float64 and
    inv uint8 [batch, n_rows, n_cols] on the GPU -> int16 [batch, n_rows, n_cols, 2], x first.  Invalid and non-finite cells
    take the rounded mean of their valid neighbours; smooth: the 3 x 3 binomial afterwards.  The inputs are not written."""
    u, v, inv = _fields3("deform_nodes", u, v, inv)
    B, nr, nc = u.shape
    nodes = torch.empty(B, nr, nc, 2, dtype=torch.int16, device=u.device)
    with torch.cuda.device(u.device):
        check(lib.tpiv_deform_nodes(u.data_ptr(), v.data_ptr(), inv.data_ptr(), B, nr, nc, 1 if smooth else 0,
                                    nodes.data_ptr(), _stream()))
    return nodes


def deform_warp(a, b, nodes, ws, ov, interp="cubic", counter=None, gather=False):
    """Both frames of every pair warped by the dense half shift between the nodes (tpiv_deform_warp): a, b uint8
    [batch, H, W] (or [H, W]) on the GPU, nodes int16 [batch, n_rows, n_cols, 2] of the grid of (ws, ov) -> (wa, wb) uint8
    like the frames, a sampled at -h and b at +h.  counter: an int32 [2] tensor on the device that gains the number of
    tiles sampled from LDS and of tiles gathered.  gather: the per-pixel gather in every tile (the same bytes)."""
    a, b = _frames(a, b)
    _need_cuda(nodes, counter)
    if not isinstance(interp, str) or interp not in _lib.DEWARP_INTERPS:
        raise ValueError(f"deform_warp: interp must be one of {sorted(_lib.DEWARP_INTERPS)}, got {interp!r}")
    B, H, W = a.shape
    if isinstance(ws, (int, np.integer)) and isinstance(ov, (int, np.integer)) and 0 <= ov < ws <= min(H, W):
        nr, nc = (H - ws) // (ws - ov) + 1, (W - ws) // (ws - ov) + 1
        if nodes.dtype != torch.int16 or tuple(nodes.shape) != (B, nr, nc, 2):
            raise ValueError(f"deform_warp: nodes must be int16 [{B}, {nr}, {nc}, 2] for these frames, got {nodes.dtype} "
                             f"{tuple(nodes.shape)}")
    if counter is not None and (counter.dtype != torch.int32 or counter.numel() != 2 or not counter.is_contiguous()):
        raise ValueError("deform_warp: counter must be a contiguous int32 tensor of 2 elements")
    nodes = nodes.contiguous()
    table = _dewarp_table(a.device)
    wa, wb = torch.empty_like(a), torch.empty_like(b)
    kind = _lib.DEWARP_INTERPS[interp] | (_lib.DEFORM_GATHER if gather else 0)
    with torch.cuda.device(a.device):
        check(lib.tpiv_deform_warp(a.data_ptr(), b.data_ptr(), B, H, W, int(ws), int(ov), nodes.data_ptr(),
                                   table.data_ptr(), kind, wa.data_ptr(), wb.data_ptr(),
                                   None if counter is None else counter.data_ptr(), _stream()))
    return wa, wb


def deform_combine(nodes, du, dv, dval):
    """u = nodes_x / 128 + du, v = nodes_y / 128 + dv (one rounding each), invalid = dval (tpiv_deform_combine): nodes int16
    [batch, n_rows, n_cols, 2], du, dv float64 and dval uint8 [batch, n_rows, n_cols] on the GPU -> (u, v, invalid)."""
    du, dv, dval = _fields3("deform_combine", du, dv, dval)
    _need_cuda(nodes)
    B, nr, nc = du.shape
    if nodes.dtype != torch.int16 or tuple(nodes.shape) != (B, nr, nc, 2):
        raise ValueError(f"deform_combine: nodes must be int16 [{B}, {nr}, {nc}, 2], got {nodes.dtype} {tuple(nodes.shape)}")
    nodes = nodes.contiguous()
    u, v, inv = torch.empty_like(du), torch.empty_like(dv), torch.empty_like(dval)
    with torch.cuda.device(du.device):
        check(lib.tpiv_deform_combine(nodes.data_ptr(), du.data_ptr(), dv.data_ptr(), dval.data_ptr(), B, nr, nc,
                                      u.data_ptr(), v.data_ptr(), inv.data_ptr(), _stream()))
    return u, v, inv


DEWARP_FIT_KINDS = {"homography": 4, "poly1": 3, "poly2": 6, "poly3": 10}       # kind -> the fewest points


def dewarp_fit(target_px, image_px, kind="homography", shape=None):
    """Least-squares fit of the backward map from a dot target (numpy, no GPU).  target_px [N, 2]: where the dots belong in
    the rectified frame, (x, y) in pixels; image_px [N, 2]: where they were found in the camera frame.  kind "homography"
    (normalised DLT: both point sets shifted to their centroid and scaled to a mean distance of sqrt 2, the matrix from
    the SVD) or "poly1" / "poly2" / "poly3" (numpy.linalg.lstsq on the coordinates normalised to [-1, 1], for which shape
    = (H, W) of the frames is needed; dewarp_arg has the term order).  Returns the dict for dewarp= -- {"homography": 3 x 3}
    or {"poly": [2, K]}.  ValueError for fewer points than the kind has unknowns (4, 3, 6, 10), or points that do not
    determine the fit."""
    if kind not in DEWARP_FIT_KINDS:
        raise ValueError(f"dewarp_fit: kind must be one of {list(DEWARP_FIT_KINDS)}, got {kind!r}")
    try:
        t, s = np.asarray(target_px, dtype=np.float64), np.asarray(image_px, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("dewarp_fit: target_px and image_px must be arrays [N, 2]") from None
    if t.ndim != 2 or t.shape[1] != 2 or t.shape != s.shape or not (np.isfinite(t).all() and np.isfinite(s).all()):
        raise ValueError(f"dewarp_fit: target_px and image_px must be finite arrays [N, 2] of one shape, got {t.shape} "
                         f"and {s.shape}")
    need = DEWARP_FIT_KINDS[kind]
    if t.shape[0] < need:
        raise ValueError(f"dewarp_fit: kind {kind!r} needs at least {need} points, got {t.shape[0]}")
    if kind == "homography":
        def norm(p):
            c = p.mean(axis=0)
            d = np.sqrt(((p - c) ** 2).sum(axis=1)).mean()
            if not d > 0:
                raise ValueError("dewarp_fit: the points coincide")
            k = np.sqrt(2.0) / d
            return np.array([[k, 0, -k * c[0]], [0, k, -k * c[1]], [0, 0, 1.0]])
        Nt, Ns = norm(t), norm(s)
        tn = (Nt @ np.column_stack([t, np.ones(len(t))]).T).T
        sn = (Ns @ np.column_stack([s, np.ones(len(s))]).T).T
        A = np.zeros((2 * len(t), 9))
        A[0::2, 0:3], A[0::2, 6:9] = tn, -sn[:, 0:1] * tn
        A[1::2, 3:6], A[1::2, 6:9] = tn, -sn[:, 1:2] * tn
        _, sv, vt = np.linalg.svd(A)
        if not sv[7] > 1e-12 * sv[0]:
            raise ValueError("dewarp_fit: the points do not determine a homography (collinear?)")
        M = np.linalg.inv(Ns) @ vt[-1].reshape(3, 3) @ Nt
        return {"homography": M / M[2, 2] if M[2, 2] != 0 else M}
    try:
        H, W = (int(v) for v in shape)
    except (TypeError, ValueError):
        raise ValueError(f"dewarp_fit: kind {kind!r} needs shape = (H, W) of the frames, got {shape!r}") from None
    if H < 2 or W < 2:
        raise ValueError(f"dewarp_fit: shape must be at least 2 x 2, got {(H, W)}")
    xn, yn = _normalised(t[:, 0], t[:, 1], H, W)
    A = np.stack(_poly_terms(xn, yn, need), axis=1)
    coef, _, rank, _ = np.linalg.lstsq(A, s, rcond=None)
    if rank < need:
        raise ValueError(f"dewarp_fit: the points do not determine a polynomial of kind {kind!r}")
    return {"poly": np.ascontiguousarray(coef.T)}


# ---- stereoscopic PIV: camera geometry on the host (numpy float64, no GPU) and the reconstruction (tpiv_stereo_reconstruct).
# World frame: right-handed, millimetres, the light sheet is z = 0, X to the right, Y up, Z towards the cameras.  Rectified
# frame: the camera frames' shape, pixel (x, y) -- x along the columns, y along the rows, downwards -- is the world point
# (X0 + p x, Y0 - p y, 0) with p = scale (mm per pixel) and origin = (X0, Y0).  Camera: P float64 [3, 4], (x_cam, y_cam, 1) ~
# P (X, Y, Z, 1) in camera pixels, y down.

def _stereo_camera(P, who):
    try:
        P = np.array(P, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: P must be a finite float64 [3, 4] matrix") from None
    if P.shape != (3, 4) or not np.isfinite(P).all():
        raise ValueError(f"{who}: P must be a finite float64 [3, 4] matrix, got shape {P.shape}")
    return P


def _stereo_scale(scale, origin, who):
    if not is_real(scale) or not np.isfinite(scale) or not scale > 0:
        raise ValueError(f"{who}: scale must be a finite positive number (mm per pixel), got {scale!r}")
    try:
        X0, Y0 = (float(q) for q in origin)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: origin must be two numbers (X0, Y0) in mm, got {origin!r}") from None
    if not (np.isfinite(X0) and np.isfinite(Y0)):
        raise ValueError(f"{who}: origin must be finite, got {origin!r}")
    return float(scale), X0, Y0


def stereo_fit(world_mm, image_px):
    """The camera matrix P [3, 4] from a calibration target (numpy, no GPU): world_mm [N, 3] the dots' world positions in
    mm, image_px [N, 2] where they were found in the camera frame, (x, y) in pixels.  Normalised DLT: the world points
    shifted to their centroid and scaled to a mean distance of sqrt 3, the image points to sqrt 2 (as dewarp_fit
    normalises), the matrix from the SVD of the [2 N, 12] design matrix.  P is scaled to |P[2, :3]| = 1 and signed so that
    the target points have positive depth P[2] . (X, Y, Z, 1).  ValueError for fewer than 6 points, non-finite input and
    points that do not determine a camera: the normalised design matrix must have rank 11, tested as s[10] > 1e-8 s[0] on
    its singular values (a target whose dots all lie in one plane has rank 8: calibrate on two planes or more)."""
    try:
        w, s = np.asarray(world_mm, dtype=np.float64), np.asarray(image_px, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("stereo_fit: world_mm must be an array [N, 3] and image_px [N, 2]") from None
    if w.ndim != 2 or s.ndim != 2 or w.shape[1:] != (3,) or s.shape[1:] != (2,) or w.shape[0] != s.shape[0] \
            or not (np.isfinite(w).all() and np.isfinite(s).all()):
        raise ValueError(f"stereo_fit: world_mm must be a finite array [N, 3] and image_px [N, 2], got {w.shape} and {s.shape}")
    if w.shape[0] < 6:
        raise ValueError(f"stereo_fit: a camera matrix needs at least 6 points, got {w.shape[0]}")

    def norm(p):
        c = p.mean(axis=0)
        d = np.sqrt(((p - c) ** 2).sum(axis=1)).mean()
        if not d > 0:
            raise ValueError("stereo_fit: the points coincide")
        k = np.sqrt(float(p.shape[1])) / d
        N = np.eye(p.shape[1] + 1)
        N[:-1, :-1] *= k
        N[:-1, -1] = -k * c
        return N
    Nw, Ns = norm(w), norm(s)
    wn = (Nw @ np.column_stack([w, np.ones(len(w))]).T).T
    sn = (Ns @ np.column_stack([s, np.ones(len(s))]).T).T
    A = np.zeros((2 * len(w), 12))
    A[0::2, 0:4], A[0::2, 8:12] = wn, -sn[:, 0:1] * wn
    A[1::2, 4:8], A[1::2, 8:12] = wn, -sn[:, 1:2] * wn
    _, sv, vt = np.linalg.svd(A)
    if not sv[10] > 1e-8 * sv[0]:
        raise ValueError("stereo_fit: the points do not determine a camera matrix (all in one plane?)")
    P = np.linalg.inv(Ns) @ vt[-1].reshape(3, 4) @ Nw
    k = np.sqrt((P[2, :3] ** 2).sum())
    if not k > 0:
        raise ValueError("stereo_fit: the points do not determine a camera matrix")
    P = P / k
    depth = P[2, :3] @ w.T + P[2, 3]
    return -P if depth.mean() < 0 else P


def stereo_centre(P):
    """The centre of projection C [3] of the camera P [3, 4], in mm: C = -P[:, :3]^-1 P[:, 3]."""
    P = _stereo_camera(P, "stereo_centre")
    try:
        return -np.linalg.solve(P[:, :3], P[:, 3])
    except np.linalg.LinAlgError:
        raise ValueError("stereo_centre: P[:, :3] is singular (a camera at infinity)") from None


def stereo_homography(P, scale, origin=(0.0, 0.0)):
    """The backward map of the camera P for dewarp= -- {"homography": stereo_homography(P, scale, origin)} --: the 3 x 3
    matrix that takes the rectified pixel (x, y, 1) to the camera pixel, P @ [[p, 0, X0], [0, -p, Y0], [0, 0, 0], [0, 0, 1]]
    with p = scale in mm per pixel and origin = (X0, Y0) the world position of pixel (0, 0); exact for a pinhole."""
    P = _stereo_camera(P, "stereo_homography")
    p, X0, Y0 = _stereo_scale(scale, origin, "stereo_homography")
    return P @ np.array([[p, 0.0, X0], [0.0, -p, Y0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def stereo_tangents(P, X, Y):
    """The viewing tangents (a, b) of the camera P at the world points (X, Y, 0), arrays of one shape in mm: a = (X - C_x) /
    C_z, b = (Y - C_y) / C_z with C = stereo_centre(P).  To first order a particle at (X, Y, 0) that moves by (dX, dY, dZ) is
    seen in the rectified frame of that camera moving by (dX + a dZ, dY + b dZ).  ValueError unless C_z > 0 (a camera in
    or behind the sheet)."""
    C_ = stereo_centre(P)
    if not (np.isfinite(C_).all() and C_[2] > 0):
        raise ValueError(f"stereo_tangents: the camera centre {tuple(C_)} does not lie in front of the sheet (C_z > 0)")
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    return (X - C_[0]) / C_[2], (Y - C_[1]) / C_[2]


def stereo_planes(P, x, y, scale, origin=(0.0, 0.0)):
    """The tangent planes (a, b) of the camera P for the fields the classes deliver: x, y [n_rows, n_cols] are the pixel
    coordinates of the window centres as get_coordinates returns them (not scaled).  Delivered fields are flipped along
    axis 0 and x, y are not, so cell [r, c] of a delivered field belongs to the window centre (x[r, c], y[n_rows - 1 - r,
    c]) = the world point (X0 + p x, Y0 - p y, 0).  Returns contiguous float64 [n_rows, n_cols] planes in the delivered
    orientation -- what stereo_reconstruct takes."""
    p, X0, Y0 = _stereo_scale(scale, origin, "stereo_planes")
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.ndim != 2 or x.shape != y.shape:
        raise ValueError(f"stereo_planes: x, y must be [n_rows, n_cols] arrays of one shape, got {x.shape} and {y.shape}")
    a, b = stereo_tangents(P, X0 + p * x, Y0 - p * np.flip(y, axis=0))
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


# the cells a workgroup of tpiv_stereo_reconstruct covers at one cell per lane (twice as many at two) and the pairs it
# walks; the lanes of the per-pair summary's workgroup (csrc/piv_kernels.h)
STEREO_BLOCK = (256, 8)
STEREO_SUM_THREADS = 1024


class StereoFields(tuple):
    """What stereo_reconstruct returns: a tuple (U, V, W, res, status, pair_rms, pair_count) -- with sigma followed by sU, sV,
    sW -- whose elements also answer to these names."""
    _names = ("U", "V", "W", "res", "status", "pair_rms", "pair_count", "sU", "sV", "sW")

    def __getattr__(self, name):
        names = StereoFields._names
        if name in names and names.index(name) < len(self):
            return self[names.index(name)]
        raise AttributeError(name)


def stereo_reconstruct(u1, v1, u2, v2, a1, b1, a2, b2, sigma=None, skip=None, fill=0.0):
    """The three components of every cell from the fields of two cameras (tpiv_stereo_reconstruct; include/torchpiv_hip.h
    has the arithmetic).  u1, v1, u2, v2: float64 tensors [batch, n_rows, n_cols] (or [n_rows, n_cols]) on the GPU, the
    fields as the classes deliver them, both cameras with the same scale and dt; a1, b1, a2, b2: float64 [n_rows, n_cols],
    the tangent planes in the same orientation (stereo_planes); sigma: None or the four fields (su1, sv1, su2, sv2) of
    uncertainty=, shaped like u1; skip: None or uint8 / bool [n_rows, n_cols], non-zero = excluded in every pair (U, V, W =
    fill there).  Returns a StereoFields record: U, V, W, res float64 and status uint8 shaped like u1 (0: reconstructed, 1:
    skipped, 2: a non-finite input vector, 3: no geometry), pair_rms float64 and pair_count int32 [batch] (scalars for a 2-D
    input) and, with sigma, sU, sV, sW.  The inputs are not written."""
    fields = (u1, v1, u2, v2)
    planes = (a1, b1, a2, b2)
    sig = () if sigma is None else tuple(sigma)
    if len(sig) not in (0, 4):
        raise ValueError("stereo_reconstruct: sigma takes the four fields (su1, sv1, su2, sv2) or None")
    every = fields + planes + sig
    if any(not isinstance(t, torch.Tensor) for t in every) or (skip is not None and not isinstance(skip, torch.Tensor)):
        raise TypeError("stereo_reconstruct: tensors on the GPU")
    _need_cuda(*every, skip)
    if any(t.dtype != torch.float64 for t in every) or (skip is not None and skip.dtype not in (torch.uint8, torch.bool)):
        raise TypeError("stereo_reconstruct: fields, tangent planes and sigmas float64, skip uint8 or bool")
    if u1.dim() not in (2, 3) or any(t.shape != u1.shape for t in fields + sig):
        raise ValueError("stereo_reconstruct: [batch, n_rows, n_cols] or [n_rows, n_cols] fields of one shape")
    grid = tuple(u1.shape[-2:])
    if any(tuple(t.shape) != grid for t in planes) or (skip is not None and tuple(skip.shape) != grid):
        raise ValueError(f"stereo_reconstruct: the tangent planes and skip must be [{grid[0]}, {grid[1]}]")
    if any(t.device != u1.device for t in every) or (skip is not None and skip.device != u1.device):
        raise ValueError("stereo_reconstruct: every tensor on one device")
    if grid[0] < 1 or grid[1] < 1:
        raise ValueError("stereo_reconstruct: empty grid")
    if not is_real(fill):
        raise ValueError(f"stereo_reconstruct: fill must be a number, got {fill!r}")
    flat = u1.dim() == 2
    B = 1 if flat else u1.shape[0]
    fields = tuple(t.contiguous() for t in fields)
    planes = tuple(t.contiguous() for t in planes)
    sig = tuple(t.contiguous() for t in sig)
    if skip is not None:
        skip = skip.contiguous()
        skip = skip.view(torch.uint8) if skip.dtype == torch.bool else skip
    dev = u1.device
    shape = (B,) + grid
    out = [torch.empty(shape, dtype=torch.float64, device=dev) for _ in range(4 + (3 if sig else 0))]
    status = torch.empty(shape, dtype=torch.uint8, device=dev)
    rms = torch.empty(B, dtype=torch.float64, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    ptr_s = [t.data_ptr() for t in sig] if sig else [None] * 4
    ptr_o = [t.data_ptr() for t in out] + ([] if sig else [None] * 3)
    with torch.cuda.device(dev):
        check(lib.tpiv_stereo_reconstruct(*[t.data_ptr() for t in fields], *ptr_s, None if skip is None else skip.data_ptr(),
                                          *[t.data_ptr() for t in planes], B, grid[0] * grid[1], float(fill), *ptr_o,
                                          status.data_ptr(), rms.data_ptr(), count.data_ptr(), _stream()))
    got = out[:4] + [status, rms, count] + out[4:]
    if flat:
        got = [t[0] for t in got]
    return StereoFields(got)


# ---- stereo self-calibration (Wieneke 2005): the sheet's plane from the disparity of the two rectified views, and the
# cameras expressed in the frame of that plane.  The triangulation is the device's (tpiv_stereo_triangulate); the plane and
# the corrected cameras are host geometry (numpy float64, no GPU).

def stereo_cells(x, y, scale, origin=(0.0, 0.0)):
    """The world positions (X, Y) of the cells in the orientation of the delivered fields: x, y [n_rows, n_cols] are the
    window centres as get_coordinates returns them; cell [r, c] of a delivered field is the world point (X0 + p x[r, c], Y0 -
    p y[n_rows - 1 - r, c], 0) -- the flip stereo_planes applies.  Returns contiguous float64 arrays."""
    p, X0, Y0 = _stereo_scale(scale, origin, "stereo_cells")
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.ndim != 2 or x.shape != y.shape:
        raise ValueError(f"stereo_cells: x, y must be [n_rows, n_cols] arrays of one shape, got {x.shape} and {y.shape}")
    return np.ascontiguousarray(X0 + p * x), np.ascontiguousarray(Y0 - p * np.flip(y, axis=0))


class StereoPoints(tuple):
    """What stereo_triangulate returns: a tuple (X, Y, Z, gap, status, count, sums) -- (status, count, sums) with
    points=False -- whose elements also answer to these names."""

    def __new__(cls, values, names):
        self = super().__new__(cls, values)
        self._names = tuple(names)
        return self

    def __getattr__(self, name):
        names = self.__dict__.get("_names", ())
        if name in names:
            return self[names.index(name)]
        raise AttributeError(name)

    @property
    def count(self):                                  # (tuple.count would answer first)
        return self[self._names.index("count")]


def stereo_triangulate(dx, dy, X, Y, C1, C2, skip=None, gap_max=float("inf"), plane=None, tol=float("inf"),
                       centre=(0.0, 0.0, 0.0), points=True):
    """The points of the light sheet from a disparity field (tpiv_stereo_triangulate; include/torchpiv_hip.h has the
    arithmetic).  dx, dy: float64 tensors [batch, n_rows, n_cols] (or without the batch axis; any cell shape, [cells]
    included) on the GPU, in mm, camera 2's rectified position minus camera 1's along X and Y (up) -- what
    StereoPIV.disparity() returns; X, Y: float64 tensors of the cell shape, the cells on z = 0 (stereo_cells); C1, C2: the
    camera centres (stereo_centre), three numbers each; skip: None or uint8 / bool of the cell shape; gap_max: the longest
    accepted distance between the two lines of sight (status 4 beyond it); plane = (c0, c1, c2) and tol: cells further than
    tol from the plane get status 5 (None: the plane 0 -- give tol with a plane); centre = (Xm, Ym, Zm): subtracted before
    the sums.  Returns a StereoPoints record: X, Y, Z, gap float64 (left out with points=False) and status uint8 shaped
    like dx, count int32 and sums float64 [batch] and [batch, 9] (a scalar and [9] for an input without the batch axis):
    the sums of x, y, z, xx, xy, yy, xz, yz, zz over the status-0 cells -- what stereo_plane takes."""
    every = (dx, dy, X, Y)
    if any(not isinstance(t, torch.Tensor) for t in every) or (skip is not None and not isinstance(skip, torch.Tensor)):
        raise TypeError("stereo_triangulate: tensors on the GPU")
    _need_cuda(*every, skip)
    if any(t.dtype != torch.float64 for t in every) or (skip is not None and skip.dtype not in (torch.uint8, torch.bool)):
        raise TypeError("stereo_triangulate: dx, dy, X, Y float64, skip uint8 or bool")
    grid = tuple(X.shape)
    if X.dim() < 1 or Y.shape != X.shape or dx.shape != dy.shape or dx.dim() not in (X.dim(), X.dim() + 1) \
            or tuple(dx.shape[dx.dim() - X.dim():]) != grid:
        raise ValueError("stereo_triangulate: dx, dy of one shape, [batch] + the shape of X, Y or that shape itself")
    if skip is not None and tuple(skip.shape) != grid:
        raise ValueError(f"stereo_triangulate: skip must have the cells' shape {grid}")
    if any(t.device != dx.device for t in every) or (skip is not None and skip.device != dx.device):
        raise ValueError("stereo_triangulate: every tensor on one device")
    cells = int(np.prod(grid))
    if cells < 1:
        raise ValueError("stereo_triangulate: empty grid")

    def triple(v, what):
        try:
            out = [float(q) for q in v]
        except (TypeError, ValueError):
            out = []
        if len(out) != 3:
            raise ValueError(f"stereo_triangulate: {what} takes three numbers, got {v!r}")
        return out
    cams = triple(C1, "C1") + triple(C2, "C2")
    pl = [0.0, 0.0, 0.0] if plane is None else triple(plane, "plane")
    mid = triple(centre, "centre")
    for name, v in (("gap_max", gap_max), ("tol", tol)):
        if not is_real(v) or not float(v) >= 0:
            raise ValueError(f"stereo_triangulate: {name} must be a number >= 0 (infinity: no test), got {v!r}")
    flat = dx.dim() == X.dim()
    B = 1 if flat else dx.shape[0]
    dx, dy, X, Y = (t.contiguous() for t in every)
    if skip is not None:
        skip = skip.contiguous()
        skip = skip.view(torch.uint8) if skip.dtype == torch.bool else skip
    dev = dx.device
    shape = (B,) + grid
    out = [torch.empty(shape, dtype=torch.float64, device=dev) for _ in range(4)] if points else []
    status = torch.empty(shape, dtype=torch.uint8, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    sums = torch.empty((B, 9), dtype=torch.float64, device=dev)
    host = lambda v: (C.c_double * len(v))(*v)                          # noqa: E731
    with torch.cuda.device(dev):
        check(lib.tpiv_stereo_triangulate(dx.data_ptr(), dy.data_ptr(), X.data_ptr(), Y.data_ptr(),
                                          None if skip is None else skip.data_ptr(), B, cells, host(cams), float(gap_max),
                                          host(pl), float(tol), host(mid), *([t.data_ptr() for t in out] or [None] * 4),
                                          status.data_ptr(), count.data_ptr(), sums.data_ptr(), _stream()))
    got = out + [status, count, sums]
    if flat:
        got = [t[0] for t in got]
    return StereoPoints(got, (("X", "Y", "Z", "gap") if points else ()) + ("status", "count", "sums"))


def stereo_plane(count, sums, centre=(0.0, 0.0, 0.0)):
    """(c0, c1, c2, rms): the least-squares plane Z = c0 + c1 X + c2 Y through the points whose centred sums
    stereo_triangulate returns -- count and sums [9] of ONE item (numbers, arrays or tensors), centre the point the sums
    were taken about -- from the normal equations of the centred moments: Sxx = sum xx - (sum x)^2 / n and so on, (c1, c2)
    from the 2 x 2 block, c0 from the means; rms = the root of the mean squared residual.  ValueError for fewer than 3
    points, non-finite sums, and points on one line: the block's determinant must exceed 1e-12 Sxx Syy."""
    n = int(count)
    s = np.asarray(sums.cpu() if isinstance(sums, torch.Tensor) else sums, dtype=np.float64).reshape(-1)
    Xm, Ym, Zm = (float(q) for q in centre)
    if s.shape != (9,) or not np.isfinite(s).all():
        raise ValueError("stereo_plane: sums takes the nine finite sums of one item")
    if n < 3:
        raise ValueError(f"stereo_plane: a plane needs at least 3 cells, got {n}")
    mx, my, mz = s[0] / n, s[1] / n, s[2] / n
    Sxx, Sxy, Syy = s[3] - s[0] * mx, s[4] - s[0] * my, s[5] - s[1] * my
    Sxz, Syz, Szz = s[6] - s[0] * mz, s[7] - s[1] * mz, s[8] - s[2] * mz
    det = Sxx * Syy - Sxy * Sxy
    if not (Sxx > 0 and Syy > 0 and det > 1e-12 * Sxx * Syy):
        raise ValueError("stereo_plane: the cells lie on one line and do not determine a plane")
    c1 = (Sxz * Syy - Syz * Sxy) / det
    c2 = (Syz * Sxx - Sxz * Sxy) / det
    k = mz - c1 * mx - c2 * my                                         # the plane in centred coordinates: z = k + c1 x + c2 y
    c0 = Zm + k - c1 * Xm - c2 * Ym
    ss = Szz - c1 * Sxz - c2 * Syz
    return float(c0), float(c1), float(c2), float(np.sqrt(max(ss, 0.0) / n))


def stereo_correct(P, plane):
    """(P_new, T): the camera P [3, 4] expressed in the world frame of the measured sheet.  plane = (c0, c1, c2): the sheet
    is Z = c0 + c1 X + c2 Y in the OLD frame.  T [4, 4] is the rigid transform that takes NEW world coordinates to old ones:
    its z axis is the plane's normal n = (-c1, -c2, 1) / |.|, its x axis the old X axis projected into the plane and
    normalised, y = n x x, its origin (0, 0, c0), the plane's point above the old origin.  P_new = P @ T projects a point
    given in the new frame to where P projects the same point given in the old one; the sheet is z = 0 in the new frame.
    ValueError for a non-finite plane and when the corrected centre does not lie in front of the sheet (C_z > 0)."""
    P = _stereo_camera(P, "stereo_correct")
    try:
        c0, c1, c2 = (float(q) for q in plane)
    except (TypeError, ValueError):
        raise ValueError(f"stereo_correct: plane takes three numbers (c0, c1, c2), got {plane!r}") from None
    if not (np.isfinite(c0) and np.isfinite(c1) and np.isfinite(c2)):
        raise ValueError(f"stereo_correct: the plane must be finite, got {(c0, c1, c2)}")
    n = np.array([-c1, -c2, 1.0])
    n /= np.sqrt(n @ n)
    ex = np.array([1.0, 0.0, 0.0]) - n[0] * n
    ex /= np.sqrt(ex @ ex)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = ex, np.cross(n, ex), n, (0.0, 0.0, c0)
    P_new = P @ T
    C_ = stereo_centre(P_new)
    if not (np.isfinite(C_).all() and C_[2] > 0):
        raise ValueError(f"stereo_correct: the corrected camera centre {tuple(C_)} does not lie in front of the sheet (C_z > 0)")
    return P_new, T


class Plan:
    """The multipass pipeline of OfflinePIV.__call__ (PIVbackend.py:873-882) for batches of
    pairs resident on one GPU.  Owns the device workspace; `run` only enqueues kernels."""

    def __init__(self, H, W, ws, ov, n_pass=1, mode="CWS", pass_scale=2.0, val_ratio=1.2,
                 val_win=3, max_batch=1, device=None, precision="exact", outlier=None, mask=None, uncertainty=None,
                 deform=None, ensemble=False, weighting=None, correlation=None):
        # outlier: None, "median" or a dict (outlier_arg): the normalized median test after every pass -- flagged vectors of
        # a pass before the last are replaced by their neighbourhood median before the predictor reads them, flagged
        # vectors of the last pass join the invalid mask (tpiv_plan_set_outlier)
        # mask: None, an image [H, W] or a dict (mask_arg): the windows of every pass whose share of masked pixels exceeds
        # the threshold are excluded -- zero vectors that are invalid to the predictor and to the median test, valid to the
        # post-validation (tpiv_plan_set_mask).  The plan reads the image and the threshold only: the pixel step
        # (apply_mask) and the fill value are the business of whoever owns the frames and delivers the fields.
        # uncertainty: None, "cs" or a dict (uncertainty_arg): the correlation-statistics estimate of every returned vector's
        # random error, behind the last pass on the frames of the run (tpiv_plan_set_uncertainty); read with uncertainty()
        # deform: None, an integer or a dict (deform_arg): that many rounds of image deformation behind the last pass -- the
        # frames warped by the dense field, the first pass on the warped frames, the residual added (tpiv_plan_set_deform);
        # deform_stage() and deform_ms() read what the last round left and what the rounds cost
        # ensemble: sum-of-correlation passes next to run() -- ensemble_begin / _add / _end, run_ensemble
        # (tpiv_plan_set_ensemble); window sizes 16, 32, 64 only, and neither uncertainty= nor deform=
        # correlation: None, "phase", "rpc" or a dict (correlation_arg): every pass takes its peak from the phase-only /
        # robust-phase-correlation map instead of the plain cross-correlation (tpiv_plan_set_correlation); window sizes 16,
        # 32, 64 only, neither uncertainty= nor deform= nor ensemble=, and `precision` has no effect on such a plan
        # weighting: None, "gaussian", "uniform" or a dict (weighting_arg): every pass multiplies its windows by a separable
        # weight in front of the transform (tpiv_plan_set_weighting); window sizes 16, 32, 64 only, neither uncertainty= nor
        # ensemble= nor correlation=; combines with deform= (the residual passes are weighted too), and `precision` has no
        # effect on such a plan
        self.outlier = outlier_arg(outlier)
        self.mask = mask_arg(mask)
        self.deform = deform_arg(deform)
        self.uncertainty_par = uncertainty_arg(uncertainty)
        self.ensemble = bool(ensemble)
        self.correlation = correlation_arg(correlation)
        self.weighting = weighting_arg(weighting)
        refuse_all(dict(uncertainty=self.uncertainty_par, deform=self.deform, ensemble=self.ensemble or None,
                        correlation=self.correlation, weighting=self.weighting),
                   [w for w, _ in pass_sizes(ws, ov, n_pass, pass_scale)], mode)
        mask_shape(self.mask, (H, W))
        if not torch.cuda.is_available():
            raise RuntimeError("torchpiv_amd.Plan needs a ROCm device (there is no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None \
            else torch.device(device)
        if n_pass > 1 and mode not in MODES:
            raise KeyError(mode)
        self._h = C.c_void_p()
        self.H, self.W, self.max_batch = H, W, max_batch
        self.precision = precision
        prec = _precision(precision)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        with torch.cuda.device(self.device):
            check(lib.tpiv_plan_create(C.byref(self._h), H, W, ws, ov, n_pass, MODES.get(mode, 0),
                                       float(pass_scale), float(val_ratio), int(val_win),
                                       int(max_batch), prec))
            try:
                if self.outlier is not None:
                    check(lib.tpiv_plan_set_outlier(self._h, 1, self.outlier["threshold"], self.outlier["eps"],
                                                    self.outlier["min_neighbours"]))
                if self.mask is not None:
                    self.set_mask(self.mask["image"], self.mask["threshold"])
                if self.uncertainty_par is not None:
                    check(lib.tpiv_plan_set_uncertainty(self._h, 1, self.uncertainty_par["radius"]))
                if self.deform is not None:
                    cubic = self.deform["interp"] == "cubic"
                    check(lib.tpiv_plan_set_deform(self._h, self.deform["iterations"], _lib.DEWARP_INTERPS[self.deform["interp"]],
                                                   1 if self.deform["smooth"] else 0,
                                                   _dewarp_table(self.device).data_ptr() if cubic else None))
                if self.ensemble:
                    check(lib.tpiv_plan_set_ensemble(self._h, 1))
                if self.correlation is not None:
                    self.set_correlation(self.correlation)
                if self.weighting is not None:
                    self.set_weighting(self.weighting)
            except Exception:
                self.close()
                raise
        self._pair_masks = False         # the per-pair grids, switched on by the first run_masked
        self.n_pass = lib.tpiv_plan_n_pass(self._h)
        self.geometry = []
        for p in range(self.n_pass):
            w, o, nr, nc = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            check(lib.tpiv_plan_pass_geometry(self._h, p, C.byref(w), C.byref(o), C.byref(nr),
                                              C.byref(nc)))
            self.geometry.append((w.value, o.value, nr.value, nc.value))

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and lib is not None:     # lib is None at interpreter teardown
            lib.tpiv_plan_destroy(h)
            self._h = C.c_void_p()

    __del__ = close

    def set_correlation(self, correlation):
        """Switches the plan's passes to the filtered map (correlation_arg's forms; None: back to the plain
        cross-correlation).  The tables are built here and uploaded once (tpiv_plan_set_correlation)."""
        par = correlation_arg(correlation)
        self._set_tables(lib.tpiv_plan_set_correlation, correlation_tables, par,
                         (_lib.CORR_NONE, 0.0, 0.0, 0.0) if par is None else
                         (_lib.CORRELATIONS[par["kind"]], par["dx"], par["dy"], par["floor"]))
        self.correlation = par

    def set_weighting(self, weighting):
        """Switches the plan's passes to weighted windows (weighting_arg's forms; None: back to the plain passes).  The
        tables are built here and uploaded once (tpiv_plan_set_weighting)."""
        par = weighting_arg(weighting)
        self._set_tables(lib.tpiv_plan_set_weighting, weighting_tables, par,
                         (_lib.WEIGHT_NONE, 0.0, 0.0) if par is None else (_lib.WEIGHTINGS[par["kind"]], par["sx"], par["sy"]))
        self.weighting = par

    def _set_tables(self, setter, tables, par, head):
        """setter(plan, *head, table, length): the table of tables(par, the window size of every pass), or none for par None."""
        with torch.cuda.device(self.device):
            if par is None:
                check(setter(self._h, *head, None, 0))
                return
            sizes = []
            for p in range(lib.tpiv_plan_n_pass(self._h)):
                w = C.c_int()
                check(lib.tpiv_plan_pass_geometry(self._h, p, C.byref(w), None, None, None))
                sizes.append(w.value)
            tab = tables(par, sizes)
            check(setter(self._h, *head, tab.ctypes.data, tab.size))

    @property
    def out_shape(self):
        return self.geometry[-1][2], self.geometry[-1][3]

    def run(self, a, b, out=None):
        """a, b uint8 [batch, H, W] (or [H, W]) on the plan's device.  Returns u, v float64 and
        invalid uint8, [batch, n_rows, n_cols] of the last pass (async on the current stream)."""
        return self._run(a, b, out)

    def _run(self, a, b, out, masks=None, threshold=0.0):
        a, b = _frames(a, b)
        B = a.shape[0]
        if a.shape[1] != self.H or a.shape[2] != self.W:
            raise ValueError("frame shape differs from the plan's")
        if a.device != self.device or b.device != self.device:
            raise ValueError(f"frames live on {a.device}, the plan on {self.device}")
        if B > self.max_batch:
            raise ValueError(f"batch {B} exceeds the plan's max_batch {self.max_batch}")
        nr, nc = self.out_shape
        if out is None:
            u = torch.empty(B, nr, nc, dtype=torch.float64, device=a.device)
            v = torch.empty_like(u)
            inv = torch.empty(B, nr, nc, dtype=torch.uint8, device=a.device)
        else:
            u, v, inv = out
            for t, dt, name in ((u, torch.float64, "u"), (v, torch.float64, "v"), (inv, torch.uint8, "invalid")):
                if not isinstance(t, torch.Tensor) or t.dtype != dt:
                    raise TypeError(f"out[{name}] must be a {dt} tensor")
                if t.device != self.device:
                    raise ValueError(f"out[{name}] lives on {t.device}, the plan on {self.device}")
                if not t.is_contiguous() or t.dim() != 3 or t.shape[0] < B or tuple(t.shape[1:]) != (nr, nc):
                    raise ValueError(f"out[{name}] must be contiguous [>= {B}, {nr}, {nc}], got {tuple(t.shape)}")
        with torch.cuda.device(self.device):
            if masks is None:
                check(lib.tpiv_plan_run(self._h, a.data_ptr(), b.data_ptr(), B, u.data_ptr(),
                                        v.data_ptr(), inv.data_ptr(), _stream()))
            else:
                check(lib.tpiv_plan_run_masked(self._h, a.data_ptr(), b.data_ptr(), masks.data_ptr(), float(threshold), B,
                                               u.data_ptr(), v.data_ptr(), inv.data_ptr(), _stream()))
        return u, v, inv

    def run_masked(self, a, b, masks, threshold=MASK_DEFAULTS["threshold"], out=None):
        """run() with one mask per pair: masks uint8 [batch, H, W] (or [H, W]) on the plan's device, non-zero = masked.
        The cells of every pass whose share of masked pixels exceeds the threshold are excluded pair by pair, exactly as
        a static mask excludes them for every pair (tpiv_plan_run_masked); a static mask of the plan is superseded for
        this run -- OR its image into masks.  The frames are not touched (apply_mask_pairs is the pixel step).  Switches
        the plan's per-pair grids on at first use (ValueError for a plan with ensemble=True); pair_mask_grid() reads them."""
        _need_cuda(masks)
        if masks.dtype != torch.uint8:
            raise TypeError("masks must be uint8")
        m = masks[None] if masks.dim() == 2 else masks
        if m.dim() != 3 or tuple(m.shape[1:]) != (self.H, self.W) or m.device != self.device:
            raise ValueError(f"masks must be [batch, {self.H}, {self.W}] on {self.device}, got {tuple(masks.shape)} on "
                             f"{masks.device}")
        a3 = a[None] if a.dim() == 2 else a
        if m.shape[0] != a3.shape[0]:
            raise ValueError(f"{m.shape[0]} masks for {a3.shape[0]} pairs")
        if not self._pair_masks:
            with torch.cuda.device(self.device):
                check(lib.tpiv_plan_set_pair_masks(self._h, 1))
            self._pair_masks = True
        return self._run(a, b, out, m.contiguous(), threshold)

    def pair_mask_grid(self, p, batch, sync=True):
        """bool [batch, n_rows, n_cols] on the device: the excluded cells of pass p for every pair of the last run_masked,
        unflipped; a copy (sync=False: enqueued on the current stream behind the run, no host wait).  ValueError before
        the first run_masked."""
        pg = C.c_void_p()
        check(lib.tpiv_plan_pass_pair_mask(self._h, p, C.byref(pg)))
        if not 0 <= batch <= self.max_batch:
            raise ValueError(f"batch {batch} exceeds the plan's max_batch {self.max_batch}")
        _, _, nr, nc = self.geometry[p]
        grid = torch.empty(batch, nr, nc, dtype=torch.uint8, device=self.device)
        if batch:
            self._copy_out(((grid, pg, batch * nr * nc),), sync=sync)
        return grid != 0

    def ensemble_begin(self, p):
        """Opens ensemble pass p: zeroes the accumulator and, for p > 0, runs the predictor once on the ensemble field of
        pass p - 1 (ValueError when that pass has not been ended, or for a plan without ensemble=True)."""
        with torch.cuda.device(self.device):
            check(lib.tpiv_plan_ensemble_begin(self._h, int(p), _stream()))
        self._ens_pass = self._ens_last = int(p)

    def ensemble_add(self, a, b):
        """Adds the maps of the pairs a, b uint8 [batch <= max_batch, H, W] to the open pass's accumulator."""
        a, b = _frames(a, b)
        B = a.shape[0]
        if a.shape[1] != self.H or a.shape[2] != self.W:
            raise ValueError("frame shape differs from the plan's")
        if a.device != self.device or b.device != self.device:
            raise ValueError(f"frames live on {a.device}, the plan on {self.device}")
        if B > self.max_batch:
            raise ValueError(f"batch {B} exceeds the plan's max_batch {self.max_batch}")
        with torch.cuda.device(self.device):
            check(lib.tpiv_plan_ensemble_add(self._h, a.data_ptr(), b.data_ptr(), B, _stream()))

    def _ensemble_open(self):
        if not self.ensemble:
            raise ValueError("ensemble correlation is off: Plan(..., ensemble=True)")
        acc, n = C.c_void_p(), C.c_longlong()
        check(lib.tpiv_plan_ensemble_maps(self._h, C.byref(acc), C.byref(n)))
        return acc, n.value

    def ensemble_end(self, out=None):
        """Closes the pass ensemble_begin opened: peak of the mean map, combine with the shared predictor, the plan's settle
        step (mask=, outlier=).  Returns u, v float64 and invalid uint8 [1, n_rows, n_cols] of that pass.  ValueError
        before ensemble_begin or with no pair added (the pass stays open)."""
        p = getattr(self, "_ens_pass", None)
        if p is None:
            raise ValueError("ensemble_end before ensemble_begin")
        _, _, nr, nc = self.geometry[p]
        if out is None:
            u = torch.empty(1, nr, nc, dtype=torch.float64, device=self.device)
            v = torch.empty_like(u)
            inv = torch.empty(1, nr, nc, dtype=torch.uint8, device=self.device)
        else:
            u, v, inv = out
            for t, dt, name in ((u, torch.float64, "u"), (v, torch.float64, "v"), (inv, torch.uint8, "invalid")):
                if not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != self.device or not t.is_contiguous() \
                        or tuple(t.shape) != (1, nr, nc):
                    raise ValueError(f"out[{name}] must be a contiguous {dt} tensor [1, {nr}, {nc}] on {self.device}")
        with torch.cuda.device(self.device):
            check(lib.tpiv_plan_ensemble_end(self._h, u.data_ptr(), v.data_ptr(), inv.data_ptr(), _stream()))
        self._ens_pass = None
        return u, v, inv

    def ensemble_maps(self):
        """(acc float32 [n_rows * n_cols, ws, ws], pairs added): a copy of the accumulator at the geometry of the pass begun
        last (waits for the device).  Test access."""
        acc, n = self._ensemble_open()
        p = getattr(self, "_ens_last", None)
        if p is None:
            raise ValueError("ensemble_maps before ensemble_begin")
        ws, _, nr, nc = self.geometry[p]
        out = torch.empty(nr * nc, ws, ws, dtype=torch.float32, device=self.device)
        self._copy_out(((out, acc, out.numel() * 4),))
        return out, n

    def run_ensemble(self, chunks, out=None):
        """Every pass of the plan as an ensemble pass.  chunks: a callable that returns a fresh iterator of (a, b) device
        batches (uint8 [<= max_batch, H, W]); it is called once per pass, so a recording is read once per pass.  Returns
        u, v, invalid [1, n_rows, n_cols] of the last pass."""
        self._ensemble_open()
        res = None
        for p in range(self.n_pass):
            self.ensemble_begin(p)
            for a, b in chunks():
                self.ensemble_add(a, b)
            res = self.ensemble_end(out if p == self.n_pass - 1 else None)
        return res

    def kernel_name(self, p):
        """Name of the cross-correlation kernel pass p launches (bench / profile labels)."""
        buf = C.create_string_buffer(128)
        lib.tpiv_plan_kernel_name(self._h, p, buf, 128)
        return buf.value.decode()

    def exact_capable(self):
        """precision="exact" and a first-pass window size the exact scheme covers (every even size from 8 to 128)?"""
        ws = self.geometry[0][0]
        return self.precision == "exact" and 8 <= ws <= 128 and ws % 2 == 0

    def exact_fallbacks(self):
        """precision="exact": windows of the last run whose first pass took the float64 transform (waits for the device)."""
        n = C.c_longlong()
        check(lib.tpiv_plan_exact_fallbacks(self._h, C.byref(n)))
        return n.value

    def exact_timing(self):
        """precision="exact": pass1_xcorr of the last get_timing() taken apart (mean ms): the float32 locating pass, the exact
        refinement, the float64 pass of the undecided windows, finalize."""
        arr = (C.c_double * 4)()
        check(lib.tpiv_plan_exact_timing(self._h, arr))
        return dict(zip(("locate_f32", "refine_exact", "undecided_f64", "finalize"), list(arr)))

    def debug_predict(self, p, u_c, v_c, inv_c):
        """Test hook: the plan's banded predictor of pass p on given coarse fields."""
        B = u_c.shape[0]
        _, _, nr, nc = self.geometry[p]
        outs = [torch.empty(B, nr, nc, dtype=torch.float64, device=self.device) for _ in range(4)]
        with torch.cuda.device(self.device):
            check(lib.tpiv_plan_debug_predict(self._h, p, B, u_c.contiguous().data_ptr(),
                                              v_c.contiguous().data_ptr(), inv_c.contiguous().data_ptr(),
                                              *[o.data_ptr() for o in outs], _stream()))
        return outs

    def set_timing(self, enable: bool):
        """Bracket every kernel of run() with hipEvents on the launch stream (bench.py)."""
        check(lib.tpiv_plan_set_timing(self._h, 1 if enable else 0))

    def get_timing(self):
        """({slot name: mean ms}, n_runs) for the runs since the last call; waits for them."""
        n = 2 * self.n_pass - 1
        arr = (C.c_double * n)()
        runs = C.c_int()
        check(lib.tpiv_plan_get_timing(self._h, arr, n, C.byref(runs)))
        names = ["pass1_xcorr"]
        for p in range(1, self.n_pass):
            names += [f"pass{p + 1}_predict", f"pass{p + 1}_xcorr"]
        return dict(zip(names, list(arr))), runs.value

    def _copy_out(self, pairs, sync=True):
        """Copies of plan-owned device arrays: [(destination tensor, source pointer, bytes)].  sync: waits for the device,
        then copies; otherwise the copies are enqueued on the current stream, behind the run, and the host does not wait."""
        if sync:
            torch.cuda.synchronize(self.device)
        with torch.cuda.device(self.device):
            for dst, src, nbytes in pairs:
                args = (C.c_void_p(dst.data_ptr()), src, C.c_size_t(nbytes), 3)      # 3: device to device
                rc = _hip().hipMemcpy(*args) if sync else _hip().hipMemcpyAsync(*args, C.c_void_p(_stream()))
                if rc != 0:
                    raise _lib.HipError(f"{'hipMemcpy' if sync else 'hipMemcpyAsync'} failed: {rc}")

    def pass_fields(self, p, batch):
        """Fields pass p (< n_pass-1) left in the workspace by the last run (copies)."""
        pu, pv, pi = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib.tpiv_plan_pass_fields(self._h, p, C.byref(pu), C.byref(pv), C.byref(pi)))
        _, _, nr, nc = self.geometry[p]
        n = batch * nr * nc
        u = torch.empty(batch, nr, nc, dtype=torch.float64, device=self.device)
        v = torch.empty_like(u)
        inv = torch.empty(batch, nr, nc, dtype=torch.uint8, device=self.device)
        self._copy_out(((u, pu, n * 8), (v, pv, n * 8), (inv, pi, n)))
        return u, v, inv

    def outlier_flag_counts(self, batch):
        """int32 [batch] on the device: vectors per pair the outlier test flagged in the last pass of the last run.
        Enqueued on the current stream behind the run (a copy of the status map and a reduction); no host wait."""
        ps = C.c_void_p()
        check(lib.tpiv_plan_pass_outliers(self._h, self.n_pass - 1, C.byref(ps)))
        nr, nc = self.out_shape
        status = torch.empty(batch, nr, nc, dtype=torch.uint8, device=self.device)
        self._copy_out(((status, ps, batch * nr * nc),), sync=False)
        return (status & 1).sum(dim=(1, 2), dtype=torch.int32)

    def uncertainty(self, batch):
        """(su, sv) float64 [batch, n_rows, n_cols] on the device: the uncertainty of the vectors of the last run, in pixels,
        NaN at its invalid and excluded cells.  Copies, enqueued on the current stream behind the run; no host wait.
        ValueError for a plan without uncertainty=."""
        psu, psv = C.c_void_p(), C.c_void_p()
        check(lib.tpiv_plan_uncertainty(self._h, C.byref(psu), C.byref(psv)))
        nr, nc = self.out_shape
        if not 0 <= batch <= self.max_batch:
            raise ValueError(f"batch {batch} exceeds the plan's max_batch {self.max_batch}")
        su = torch.empty(batch, nr, nc, dtype=torch.float64, device=self.device)
        sv = torch.empty_like(su)
        self._copy_out(((su, psu, batch * nr * nc * 8), (sv, psv, batch * nr * nc * 8)), sync=False)
        return su, sv

    def deform_stage(self, batch):
        """What the last round of the last run left (copies; waits for the device): nodes int16 [batch, n_rows, n_cols, 2],
        wa, wb uint8 [batch, H, W], du, dv float64 and dval uint8 [batch, n_rows, n_cols].  ValueError for a plan without
        deform=."""
        ptr = [C.c_void_p() for _ in range(6)]
        check(lib.tpiv_plan_deform_stage(self._h, *[C.byref(q) for q in ptr]))
        if not 0 <= batch <= self.max_batch:
            raise ValueError(f"batch {batch} exceeds the plan's max_batch {self.max_batch}")
        nr, nc = self.out_shape
        dev = self.device
        nodes = torch.empty(batch, nr, nc, 2, dtype=torch.int16, device=dev)
        wa = torch.empty(batch, self.H, self.W, dtype=torch.uint8, device=dev)
        wb = torch.empty_like(wa)
        du = torch.empty(batch, nr, nc, dtype=torch.float64, device=dev)
        dv = torch.empty_like(du)
        dval = torch.empty(batch, nr, nc, dtype=torch.uint8, device=dev)
        outs = (nodes, wa, wb, du, dv, dval)
        self._copy_out([(t, q, t.numel() * t.element_size()) for t, q in zip(outs, ptr) if t.numel()])
        return outs

    def deform_ms(self):
        """Milliseconds all deformation rounds of the last run took together (waits for them).  ValueError for a plan
        without deform= or before its first run."""
        ms = C.c_double()
        check(lib.tpiv_plan_deform_ms(self._h, C.byref(ms)))
        return ms.value

    def set_mask(self, image, threshold=MASK_DEFAULTS["threshold"]):
        """(Re)computes the plan's grids of excluded cells from a mask image (uint8 [H, W], any device; non-zero = masked)
        and a threshold (tpiv_plan_set_mask: one coverage launch per pass, waits for them); None switches the mask off."""
        with torch.cuda.device(self.device):
            if image is None:
                check(lib.tpiv_plan_set_mask(self._h, None, 0.0, _stream()))
                return
            img = image.to(self.device).contiguous()
            if img.dtype != torch.uint8 or tuple(img.shape) != (self.H, self.W):
                raise ValueError(f"set_mask: a uint8 image of the plan's frame shape {(self.H, self.W)}")
            check(lib.tpiv_plan_set_mask(self._h, img.data_ptr(), float(threshold), _stream()))

    def mask_grid(self, p):
        """bool [n_rows, n_cols] on the device: the excluded cells of pass p, unflipped (row 0 = the top window row); a
        copy.  ValueError for a plan without a mask."""
        pg = C.c_void_p()
        check(lib.tpiv_plan_pass_mask(self._h, p, C.byref(pg)))
        _, _, nr, nc = self.geometry[p]
        grid = torch.empty(nr, nc, dtype=torch.uint8, device=self.device)
        self._copy_out(((grid, pg, nr * nc),))
        return grid != 0

    def outlier_status(self, p, batch):
        """Status map (uint8 [batch, n_rows, n_cols]: bit 0 flagged by the outlier test, bit 1 invalid by the peak ratio)
        pass p -- the last included -- left during the last run (a copy).  ValueError for a plan without the test."""
        ps = C.c_void_p()
        check(lib.tpiv_plan_pass_outliers(self._h, p, C.byref(ps)))
        _, _, nr, nc = self.geometry[p]
        status = torch.empty(batch, nr, nc, dtype=torch.uint8, device=self.device)
        self._copy_out(((status, ps, batch * nr * nc),))
        return status
