"""Drop-in host side of the engine: the reference's public names with the reference's
signatures, defaults and error behaviour (NikNazarov/TorchPIV, src/torchPIV/PIVbackend.py,
cited as B:), driving the HIP library through torchpiv_amd.engine.

What runs where
  * device (libtorchpiv_hip.so): every pass of a pair -- windows, shift, FFT correlation,
    peak, validation, predictor, combine -- with the fields staying on the GPU between passes
    (the reference does three D2H copies and one H2D per pass);
  * device, batched (tpiv_postval): the post-validation of B:884-892 as far as it does not depend on
    Qhull's tie-breaking -- NaN-out, border interpolation, the ring / hole census (both drop decisions
    follow from it, so dropped pairs never leave the GPU) and every hole whose Delaunay-linear value is
    fixed by its N/S or E/W neighbours;
  * host (this file): dataset/decoding, the Delaunay hole fill (scipy/Qhull, as in the reference) for
    the pairs that still hold an ambiguous or wide hole -- counted in OfflinePIV.stats --, flip and
    unit scaling, the generator protocol.

There is no CPU compute path: device="cpu" raises.
"""
from __future__ import annotations

import collections
import contextlib
from time import time
from typing import Generator

import numpy as np
import torch

from . import engine, options
from ._lib import PRECISIONS
from ._qhull import PipelineOwner, blas_one_thread, qhull_fill, qhull_fill_many      # numpy/scipy-only module: the fill worker processes import nothing else
from .io import PIVDataset, StagedBatches, ToTensor, natural_keys, slot_bytes  # noqa: F401  (re-exported like the reference)
from .options import background_arg as _background_arg


# ----------------------------------------------------------------------------------------
# device / mode maps (B:13-18, B:814-818)
# ----------------------------------------------------------------------------------------
class _DeviceDict(dict):
    """name -> torch.device.  The reference keys CUDA devices by torch.cuda.get_device_name(i),
    so eight identical MI355X collapse to one key (the last index wins).  That behaviour is
    kept for those names; 'cuda', 'cuda:N' and plain integers are accepted as well."""

    def __init__(self):
        super().__init__()
        self._filled = False

    def _fill(self):
        if not self._filled:
            self._filled = True
            for i in range(torch.cuda.device_count()):
                try:
                    dict.__setitem__(self, torch.cuda.get_device_name(i), torch.device("cuda", i))
                except Exception:       # no usable GPU in this process
                    break
            dict.__setitem__(self, "cpu", torch.device("cpu"))

    def __getitem__(self, key):
        self._fill()
        if dict.__contains__(self, key):
            return dict.__getitem__(self, key)
        if isinstance(key, torch.device):
            return key
        if isinstance(key, int) and 0 <= key < torch.cuda.device_count():
            return torch.device("cuda", key)
        if isinstance(key, str) and (key == "cuda" or key.startswith("cuda:")):
            d = torch.device(key)
            return torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())
        raise KeyError(key)

    def keys(self):
        self._fill()
        return dict.keys(self)

    def __iter__(self):
        self._fill()
        return dict.__iter__(self)

    def __len__(self):
        self._fill()
        return dict.__len__(self)

    def __contains__(self, key):
        try:
            self[key]
            return True
        except KeyError:
            return False


class DeviceMap:
    devicies = _DeviceDict()          # (sic) the reference's attribute name


def _require_gpu(device: torch.device) -> torch.device:
    if device.type != "cuda":
        raise RuntimeError("torchpiv_amd runs on MI355X only: device='cpu' has no compute path here "
                           "(use the upstream TorchPIV for CPU runs)")
    return device


# ----------------------------------------------------------------------------------------
# geometry (B:425-456, B:522-597, B:220-247)
# ----------------------------------------------------------------------------------------
def get_field_shape(image_size, search_area_size, overlap):
    return (np.array(image_size) - search_area_size) // (search_area_size - overlap) + 1


def get_coordinates(image_size, search_area_size, overlap):
    """(x, y) meshgrid of window-centre coordinates, as the reference returns it."""
    x, y = engine.coordinates_1d(int(image_size[-2]), int(image_size[-1]), int(search_area_size),
                                 int(overlap))
    return np.meshgrid(x, y)


def moving_window_array(array: torch.Tensor, window_size, overlap) -> torch.Tensor:
    """Overlapping windows [N, ws, ws] of a 2-D tensor (a strided view made contiguous).  The
    kernels never materialise this; it is kept for callers that used the reference's helper."""
    H, W = array.shape[-2], array.shape[-1]
    st = window_size - overlap
    n_r, n_c = (H - window_size) // st + 1, (W - window_size) // st + 1
    return torch.as_strided(array, size=(n_r, n_c, window_size, window_size),
                            stride=(W * st, st, W, 1)).reshape(-1, window_size, window_size)


# ----------------------------------------------------------------------------------------
# pass 1 (B:459-520)
# ----------------------------------------------------------------------------------------
def extended_search_area_piv(frame_a, frame_b, window_size=32, overlap=0, validate: bool = False,
                             validation_ratio: float = 1.2, precision: str = "exact"):
    """First-pass PIV of one pair.  frame_a / frame_b: uint8 tensors [H, W] on a ROCm device.
    Returns (u, v, x, y, mask) as numpy arrays like the reference (mask None if not validate).
    Raises ValueError for overlap >= window_size or a window larger than the image.
    precision (extension): "exact" (default) = the map cells behind the result as exact integer correlation sums (64x64
    windows; within 1e-14 px of the reference's float64 pass, bit-identical for most windows), "f64" / "reference" = float64
    transforms like B:513-514 (what "exact" runs for other window sizes), "fast" = float32 transforms."""
    H, W = frame_a.shape[-2], frame_a.shape[-1]
    u, v, inv = engine.pass1(frame_a, frame_b, int(window_size), int(overlap),
                             val_ratio=float(validation_ratio), precision=precision)
    x, y = get_coordinates((H, W), window_size, overlap)
    mask = inv[0].cpu().numpy().astype(bool) if validate else None
    return u[0].cpu().numpy(), v[0].cpu().numpy(), x, y, mask


# ----------------------------------------------------------------------------------------
# multipass iterations (B:677-740, B:744-812)
# ----------------------------------------------------------------------------------------
class _piv_iteration:
    mode = None

    def __init__(self, frame_shape, wind_size, overlap, device) -> None:
        self.frame_shape = (int(frame_shape[-2]), int(frame_shape[-1]))
        self.wind_size, self.overlap = int(wind_size), int(overlap)
        self.n_rows, self.n_cols = get_field_shape(self.frame_shape, self.wind_size, self.overlap)
        self.device = _require_gpu(DeviceMap.devicies[device] if not isinstance(device, torch.device)
                                   else device)
        self.x, self.y = get_coordinates(self.frame_shape, self.wind_size, self.overlap)
        self.slice_x, self.slice_y = self.x[0, :], self.y[:, 0]
        self._ops = {}

    def _operators(self, y0, x0):
        key = (y0[:, 0].tobytes(), x0[0, :].tobytes())
        if key not in self._ops:
            Ay = torch.from_numpy(engine.spline_matrix(y0[:, 0], self.slice_y)).to(self.device)
            Ax = torch.from_numpy(engine.spline_matrix(x0[0, :], self.slice_x)).to(self.device)
            self._ops = {key: (Ay, Ax)}
        return self._ops[key]

    def __call__(self, frame_a, frame_b, x0, y0, u0, v0, validation_mask):
        Ay, Ax = self._operators(np.asarray(y0, dtype=np.float64), np.asarray(x0, dtype=np.float64))
        dev = self.device
        validate = validation_mask is not None
        inv_c = (torch.from_numpy(np.ascontiguousarray(validation_mask).astype(np.uint8)) if validate
                 else torch.zeros(u0.shape, dtype=torch.uint8))
        u_c = torch.from_numpy(np.ascontiguousarray(u0, dtype=np.float64)).to(dev)[None]
        v_c = torch.from_numpy(np.ascontiguousarray(v0, dtype=np.float64)).to(dev)[None]
        # (CWS_Fast: the predictor fields after the invalid-zeroing are all it needs, B:626-633)
        p_u0, p_v0, p_u2, p_v2 = engine.predict("CWS" if self.mode == "CWS_Fast" else self.mode, Ay, Ax, u_c, v_c,
                                                inv_c.to(dev)[None])
        # validate=False: the reference skips the peak-ratio test (val stays None)
        ratio = 1.2 if validate else float("-inf")
        u, v, inv = engine.iterate(self.mode, frame_a.to(dev), frame_b.to(dev), self.wind_size,
                                   self.overlap, p_u0, p_v0, p_u2, p_v2, val_ratio=ratio)
        val = inv[0].cpu().numpy().astype(bool) if validate else None
        return u[0].cpu().numpy(), v[0].cpu().numpy(), self.x, self.y, val


class piv_iteration_CWS(_piv_iteration):
    """Continuous (bilinear) window shift iteration, B:677-740."""
    mode = "CWS"


class piv_iteration_DWS(_piv_iteration):
    """Discrete (integer) window shift iteration, B:744-812."""
    mode = "DWS"


class piv_iteration_CWS_Fast(_piv_iteration):
    """The reference's bicubic window-deformation iteration (B:599-675): every window is resampled inside
    itself by -/+ u0/2 (torch's grid_sample, mode "bicubic", border padding), normalised by its mean and
    correlated; u = u0 + du.  As in the reference it is NOT in IterModMap (OfflinePIV never uses it) and its
    call takes three more arguments, which the reference ignores in favour of the constructor's except for
    the window geometry."""
    mode = "CWS_Fast"

    def __call__(self, frame_a, frame_b, x0, y0, u0, v0, validation_mask, wind_size=None, overlap=None, device=None):
        if wind_size is not None and (int(wind_size), int(overlap if overlap is not None else self.overlap)) != \
                (self.wind_size, self.overlap):
            raise ValueError("piv_iteration_CWS_Fast: wind_size / overlap differ from the constructor's")
        return super().__call__(frame_a, frame_b, x0, y0, u0, v0, validation_mask)


class IterModMap:
    functions = {"DWS": piv_iteration_DWS, "CWS": piv_iteration_CWS}


# ----------------------------------------------------------------------------------------
# post-validation on the host (B:266-344, B:884-892)
# ----------------------------------------------------------------------------------------
def nan_helper(y):
    """(NaN mask, index helper) of a 1-D array -- the reference's helper of the same name (B:311-326)."""
    mask = np.isnan(y)

    def indices(selector):
        return np.flatnonzero(selector)
    return mask, indices


def interpolate_boarders(vec: np.ndarray) -> np.ndarray:
    """Linear 1-D interpolation of NaNs along the four borders (an all-NaN border is left)."""
    if not np.isnan(vec).any():
        return vec
    for line in (vec[0, :], vec[-1, :], vec[:, 0], vec[:, -1]):      # views: edits land in vec
        nans = np.isnan(line)
        if not nans.all():
            idx = np.arange(line.size)
            line[nans] = np.interp(idx[nans], idx[~nans], line[~nans])
    return vec


def getPixelsForInterp(img):
    """(ring, invalid): ring = valid cells 4-adjacent to an invalid (NaN) cell.  The reference
    dilates with OpenCV's 3x3 MORPH_ELLIPSE element, which is the 4-connected cross, with a
    constant zero border (B:275-279)."""
    invalid = np.isnan(img)
    dil = invalid.copy()
    dil[1:, :] |= invalid[:-1, :]
    dil[:-1, :] |= invalid[1:, :]
    dil[:, 1:] |= invalid[:, :-1]
    dil[:, :-1] |= invalid[:, 1:]
    return dil & ~invalid, invalid


TOO_MANY_MSG = "Warning! to many false vectors"      # the reference's stdout line (B:306), spelling included


def fillMissingValues(target_for_interp, interpolator=None):
    """Fill NaN holes by Delaunay-linear interpolation from the ring of valid neighbours (B:284-308), in place.
    None -- the pair is to be dropped -- when the ring holds a quarter of the cells or more (the reference's
    size test on the flattened point list, with its warning line), when there is nothing to interpolate from
    (no invalid vector at all: the reference's interpolator raises on zero points and its bare `except`
    swallows that, B:300-304) or when Qhull refuses the ring.  `interpolator`: optional stand-in for scipy's
    LinearNDInterpolator class."""
    ring, holes = getPixelsForInterp(target_for_interp)
    n_ring = int(np.count_nonzero(ring))
    if 4 * n_ring >= ring.size:                       # 2 coordinates per ring point against size / 2
        print(TOO_MANY_MSG)
        return None
    where_ring, where_holes = np.argwhere(ring), np.argwhere(holes)
    if interpolator is None:
        vals = qhull_fill(where_ring, target_for_interp[ring], where_holes)
    else:
        try:
            vals = interpolator(where_ring, target_for_interp[ring])(where_holes)
        except Exception:
            vals = None
    if vals is None:
        return None
    target_for_interp[holes] = vals
    return target_for_interp


def post_validate(u, v, val):
    """B:884-892: NaN-out invalid vectors, interpolate borders, fill holes.  (None, None) when
    the pair has to be dropped."""
    if val is not None:
        u[val] = np.nan
        v[val] = np.nan
        u = interpolate_boarders(u)
        v = interpolate_boarders(v)
        u = fillMissingValues(u)
        v = fillMissingValues(v)
        if u is None or v is None:
            return None, None
    return u, v


def _ring_of(hole: np.ndarray) -> np.ndarray:
    """Valid cells 4-adjacent to a hole (getPixelsForInterp, B:266-282: 3x3 cross, zero border)."""
    ring = np.zeros_like(hole)
    ring[1:, :] |= hole[:-1, :]
    ring[:-1, :] |= hole[1:, :]
    ring[:, 1:] |= hole[:, :-1]
    ring[:, :-1] |= hole[:, 1:]
    ring &= ~hole
    return ring


def fill_holes_host(u: np.ndarray, v: np.ndarray, hole: np.ndarray, solve=qhull_fill):
    """fillMissingValues (B:284-308) for u AND v with ONE triangulation: both fields carry the same
    holes, so the reference's two interpolators triangulate the same ring points in the same order
    and apply the same barycentric weights; evaluating a two-column interpolator is bit-identical.
    u, v are filled in place; returns False when the reference would drop the pair (Qhull refuses
    the ring, e.g. collinear points; the size test is done by the caller from the ring count)."""
    ring = _ring_of(hole)
    vals = solve(np.argwhere(ring), np.stack([u[ring], v[ring]], axis=1), np.argwhere(hole))
    if vals is None:
        return False
    u[hole] = vals[:, 0]
    v[hole] = vals[:, 1]
    return True


def free_cuda_memory():
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------------------
# the generator API (B:824-903)
# ----------------------------------------------------------------------------------------
Tracks = collections.namedtuple("Tracks", "x y u v residual peak_a peak_b count_a count_b matched")
Tracks.__doc__ = "The particle tracks of one pair (OfflinePIV.tracks has the fields' definitions)."
SinglePixel = collections.namedtuple("SinglePixel", "peak ratio status pairs corr", defaults=(None,))
SinglePixel.__doc__ = "The quality record of OfflinePIV.single_pixel, which has the fields' definitions."

# What a raw frame source (_raw_batches, _load_pair) hands out: [(pair id, staged)] of a batch's pairs in order and the ids of
# the n staged ones; their uint8 frames A, B [n, H, W] on the device behind tone map and rectification (None: none staged)
# and whether they are memory of the object; the background still to be subtracted from each stack (None: none, or the
# unpack fused it); whether the batch is the run's last (asking for more ends the run: a consumer with results in flight
# collects them first); and, where A and B are the halves of ONE tensor [2n, H, W] of the object's, that tensor
Raw = collections.namedtuple("Raw", "order chunk A B owned bg_a bg_b last stack", defaults=(True, None))


class OfflinePIV:
    """for x, y, u, v in OfflinePIV(folder, device, file_fmt, wind_size, overlap, ...)(): ...

    Same constructor signature, defaults, __len__ and generator protocol as the reference:
    yields float64 numpy arrays [n_rows, n_cols] of the last pass; u is flipped along axis 0
    and v flipped and negated; u, v are scaled by scale/dt*1000 and x, y by scale; pairs that
    cannot be decoded or whose hole fill fails are skipped silently.
    """

    verbose = False          # the reference prints timing lines to stdout; off by default here

    def __init__(self, folder: str, device: str, file_fmt: str, wind_size: int, overlap: int,
                 multipass: int = 1, multipass_mode: str = "CWS", dt: int = 1, scale: float = 1.,
                 multipass_scale: float = 2., folder_mode: str = "pairs", precision: str = "exact",
                 validation_ratio: float = 1.2, validation_window: int = 3, background=None, outlier=None,
                 depth=None, mask=None, dewarp=None, uncertainty=None, derive=None, deform=None, correlation=None,
                 weighting=None, dynamic_mask=None, equalize=None, prefilter=None) -> None:
        # precision (extension, keyword after the reference's arguments).  "exact" (default): as "f64", with the map cells
        # that reach the result of a 64x64 first pass evaluated as exact integer correlation sums instead of through a
        # float64 FFT (csrc/xcorr_exact.hip: within 1e-14 px of the reference's float64 pass 1, about 1.5x the rate of
        # "f64"; other first-pass sizes run as "f64").  "f64": the reference's own arithmetic types in every transform --
        # pass 1 in float64 (B:513-514), later passes float32 with a float64 epilogue.
        # "reference": the same plus the reference's operation order in the CWS sampling (bit-identical staged
        # windows).  "fast": pass 1 in float32 too (~1e-6 px from the float64 pass 1, about 1.9x the rate).
        # validation_ratio / validation_window (extensions): the constants the reference hides inside
        # correlation_to_displacement (B:364-365: val_ratio=1.2, validation_window=3), same defaults.
        # background (extension): static background removal -- every frame enters the passes as max(f, bg) - bg.
        # "min": bg_a / bg_b = the per-pixel minimum over the a / b frames of every pair of the dataset (compute_background,
        # computed on first use); a uint8 image [H, W] (both frames) or a pair (bg_a, bg_b): given.  None: frames as read.
        # outlier (extension): None, "median" or a dict with any of threshold / eps / min_neighbours -- the normalized median
        # test (Westerweel & Scarano 2005) on the device after every pass (engine.outlier_arg, tpiv_plan_set_outlier): a
        # flagged vector of a pass before the last is replaced by its neighbourhood median before it predicts the finer
        # windows; a flagged vector of the last pass joins the invalid ones and is filled by the post-validation.  More
        # flagged vectors mean more pairs reach the reference's "to many false vectors" rule (4 * ring >= cells, B:299)
        # and are dropped, exactly as for peak-ratio holes.
        # prefilter (extension): None or a dict with kind ("min", "mean" or None), size (odd, 3..63) and optionally cap
        # (1..255) -- the spatial pre-filter every frame passes on the device after the background and before the passes
        # (engine.prefilter_arg, tpiv_prefilter): minus the minimum / the rounded mean of its size x size neighbourhood,
        # then capped.  For background that is smooth in space but differs from frame to frame.
        # equalize (extension): None, "clahe" or a dict with any of tile (8..256) and clip (1..256) -- tile-wise adaptive
        # histogram equalization of every frame on the device (engine.equalize_arg, tpiv_equalize), the last step in front of
        # the passes: tone map, background, pre-filter and cap, equalize.  For illumination that differs across the frame and
        # for particle images of very different brightness inside one window.
        # mask (extension): None, an image (uint8 or bool [H, W], non-zero = masked) or a dict with "image" and any of
        # threshold / pixels / fill (engine.mask_arg) -- where there is no flow: a wall, a model, its shadow, the rim of the
        # frame.  Masked pixels are set to 0 in both frames (tpiv_apply_mask), the last step of the frame chain: tone map,
        # background, pre-filter and cap, equalize, mask.  The windows of every pass whose share of masked pixels exceeds
        # the threshold are excluded (tpiv_plan_set_mask): zero vectors that the predictor and the median test treat as
        # invalid and the post-validation as valid; the delivered fields carry `fill` there (mask_grid() tells where).
        # depth (extension): None -- 8-bit frames, a 16-bit file decoded as value >> 8 like the reference (cv2's
        # IMREAD_GRAYSCALE) --, or the tone map of deep frames (engine.depth_arg): the files are decoded to uint16 with their
        # full sample range (io.imdecode_deep) and every frame passes out = lut[sample] on the device (tpiv_depth_map) before
        # the background, the pre-filter and the passes.  {"lo", "hi", "curve"}: a fixed range; "auto" / {"auto": True, ...}:
        # the range from the histogram of a sample of pairs (tpiv_depth_histogram + engine.depth_range), resolved on first
        # use; {"lut": table}: the caller's table.  A background image given by the caller is in mapped (uint8) units.
        # dewarp (extension): None or a dict with one backward map -- "homography", "poly" or "map" -- and optionally "interp"
        # and "fill" (engine.dewarp_arg): every frame is rectified on the device (tpiv_dewarp) right after the decode / tone
        # map and before everything else: tone map, dewarp, background, pre-filter and cap, equalize, mask.  For views
        # through an oblique window, a Scheimpflug adapter or a short lens, where the magnification varies across the
        # frame.  A background image given by the caller, the mask and the delivered x, y are in rectified coordinates;
        # background="min" is the minimum of the rectified frames.  Pixels whose source lies outside the camera frame carry
        # `fill`; dewarp_outside() gives their image, fit to be passed as mask=.
        # uncertainty (extension): None, "cs" or a dict with any of kind ("cs") and radius (0..4) -- the correlation-statistics
        # estimate (Wieneke 2015) of every delivered vector's random error, 1 sigma, on the device behind the last pass
        # (engine.uncertainty_arg, tpiv_plan_set_uncertainty).  When set, __call__ yields (x, y, u, v, su, sv) and batched()
        # (i, x, y, u, v, su, sv): su, sv are flipped and scaled like u, v (no sign change), and NaN where the last pass's
        # vector was invalid (the delivered value is an interpolation), in mask-excluded cells and where the correlation
        # peak gives no estimate.
        # derive (extension): None, one name of engine.DERIVE_QUANTITIES, a tuple or list of them, or a dict with
        # "quantities" and any of radius (1..3) and order (1, 2) (engine.derive_arg) -- derivatives of every delivered field on
        # the device: a least-squares polynomial fit over the (2 radius + 1)^2 neighbourhood of every cell that leaves out
        # the excluded cells of mask= / dynamic_mask= and non-finite vectors (engine.field_fit, tpiv_field_fit), then the
        # slopes dudx .. dvdy, vorticity, divergence, shear, q, swirl in 1/s (q: 1/s^2) and the fit's own value u_smooth,
        # v_smooth (engine.derive).  The fit runs on the fields as delivered -- filled, flipped, signed, scaled -- with the
        # steps of the delivered x, y.  When set, every delivered tuple gains ONE trailing element, a dict {name: float64
        # [n_rows, n_cols]} in the order asked for: __call__ yields (x, y, u, v[, su, sv], d), batched() (i, x, y, u, v[, su,
        # sv], d), ensemble() returns (x, y, u, v, d).  Every quantity is NaN in excluded cells (no fill value applies).
        # deform (extension): None, an integer 1..8 or a dict with any of iterations, interp ("cubic" / "linear") and smooth
        # -- that many rounds of iterative image deformation behind the last pass (engine.deform_arg, tpiv_plan_set_deform):
        # both frames are warped by the dense field of the last pass, the first pass measures the residual on the warped
        # frames and the sum is the new field.  For flows with gradients inside a window.  The tuples delivered are the
        # same; only the values differ.
        # correlation (extension): None, "phase", "rpc" or a dict with any of kind, diameter (one number or (d_x, d_y), e^-2
        # diameter in pixels, 0..16) and floor (2^-20..2^-4) -- every pass takes its peak from the phase-only / robust phase
        # correlation map (Eckstein & Vlachos 2009) instead of the plain cross-correlation (engine.correlation_arg,
        # tpiv_plan_set_correlation).  For structure both frames share -- a fixed pattern, a static texture, a glare edge,
        # banding -- that competes with the particle peak.  Window sizes 16, 32 and 64 in every pass (NotImplementedError
        # otherwise); combines with neither uncertainty= nor deform= nor ensemble() (ValueError); precision= has no effect
        # on a filtered pass.  The tuples delivered are the same; only the values differ.
        # weighting (extension): None, "gaussian", "uniform" or a dict with any of kind and sigma (one number or (sigma_x,
        # sigma_y), relative to the half window, 0.2..4; default 0.4) -- every pass multiplies its interrogation windows by a
        # separable weight in front of the transform (engine.weighting_arg, tpiv_plan_set_weighting).  A Gaussian weight
        # has a positive frequency response and a smaller effective footprint than the top-hat window: a large window at
        # high overlap then resolves what a small one resolves and keeps the large window's robustness; the standard
        # companion of deform=, whose residual passes are weighted too.  The bias of the weighted correlation toward zero
        # displacement is not corrected (it vanishes as the residual does under predictor passes and deform=).  Window sizes
        # 16, 32 and 64 in every pass (NotImplementedError otherwise); combines with neither uncertainty= nor correlation=
        # nor ensemble() (ValueError); precision= has no effect on a weighted pass.  The tuples delivered are the same; only
        # the values differ.
        # dynamic_mask (extension): None or a dict (engine.dynamic_mask_arg) -- one mask per PAIR, for bodies that move: a
        # wing, a swimmer, a piston, a free surface, their shadows.  {"kind": "bright" | "dark", "size", "level", "grow"}: the
        # mask is segmented on the device from the pair's own frames (tpiv_dynamic_mask: the opening of {frame >= level} /
        # {frame <= level} by the size x size square, grown by `grow`, of both frames), read behind the background and in
        # front of the pre-filter: tone map, dewarp, background, segment, pre-filter and cap, equalize, mask pixels.  The
        # windows of every pass whose share of masked pixels exceeds the threshold are excluded pair by pair
        # (tpiv_plan_run_masked) with everything mask= says about excluded cells; the delivered fields carry `fill` there and
        # pair_mask(i) shows the mask pair i gets.  threshold / pixels / fill go into this dict when mask= is None; with
        # mask= its image is OR-ed into every pair's mask and its three values apply.  ensemble() is refused (ValueError).
        # The form {"stack": masks [N, H, W]} is ResidentPIV's.
        if precision not in PRECISIONS:
            raise KeyError(precision)
        run = dict(wind_size=wind_size, overlap=overlap, multipass=multipass, multipass_mode=multipass_mode, dt=dt,
                   scale=scale, multipass_scale=multipass_scale, precision=precision, validation_ratio=validation_ratio,
                   validation_window=validation_window)
        opts = options.parse_options(run, stack=False, background=background, outlier=outlier, prefilter=prefilter,
                                     depth=depth, equalize=equalize, mask=mask, dewarp=dewarp, uncertainty=uncertainty,
                                     derive=derive, deform=deform, correlation=correlation, weighting=weighting,
                                     dynamic_mask=dynamic_mask)
        device = DeviceMap.devicies[device]                             # KeyError like B:845
        dataset = PIVDataset(folder, file_fmt, folder_mode, deep=opts.depth is not None,
                             transform=ToTensor(dtype=torch.uint8 if opts.depth is None else torch.uint16))
        iter_function = IterModMap.functions[multipass_mode]            # KeyError like B:850
        self._init_state(device, dataset, iter_function, run, opts)
        if not self:
            return
        if self._mask is not None:
            self._mask_shape(self.frame_shape())
        if self._dewarp is not None:
            self._dewarp_shape(self.frame_shape())
        if self._bg_arg is not None and self._bg_arg != "min":
            _background_arg(background, self.frame_shape())
        _require_gpu(self._device)

    def _init_state(self, device, dataset, iter_function, run, opts):
        """Every attribute of an object, for both constructors: the run parameters (run: a dict of wind_size, overlap,
        multipass, multipass_mode, dt, scale, multipass_scale, precision, validation_ratio and validation_window), the
        thirteen keywords as options.parse_options checked them (opts: an options.Options record), and the state that the methods
        build up, empty."""
        self._device, self._dataset, self._iter_function = device, dataset, iter_function
        self._wind_size, self._overlap, self._dt = run["wind_size"], run["overlap"], run["dt"]
        self._iter, self._iter_scale, self._scale = run["multipass"], run["multipass_scale"], run["scale"]
        self._mode, self._precision = run["multipass_mode"], run["precision"]
        self._val_ratio, self._val_win = float(run["validation_ratio"]), int(run["validation_window"])
        self._bg_arg = opts.background
        self._outlier, self._prefilter, self._equalize = opts.outlier, opts.prefilter, opts.equalize
        self._mask, self._dewarp, self._uncertainty = opts.mask, opts.dewarp, opts.uncertainty
        self._depth = depth = opts.depth
        self._derive = opts.derive            # the delivered tuples gain a dict of derived fields (_derived)
        self._deform = opts.deform            # handed to every plan
        self._correlation = opts.correlation  # handed to every plan but ensemble()'s
        self._weighting = opts.weighting      # handed to every plan but ensemble()'s
        self._dynmask = opts.dynamic_mask     # (threshold, pixels and fill included)
        self._dm_masks = None            # dynamic_mask=: the masks of a launch, uint8 [batch, H, W], reused
        self._dm_work = None             # dynamic_mask=: the segmentation's workspace, kept from launch to launch
        self._dm_frames = None           # dynamic_mask=: a caller's frames minus the background, uint8 [2, batch, H, W], reused
        self._dm_stack = None            # dynamic_mask={"stack"}: the caller's masks with mask='s image, on the device
        self._dw_map = None              # dewarp=: the Q8 map on the device, int32 [H, W, 2], once a run needs it
        self._dw_frames = None           # dewarp=: the rectified frames of a launch, uint8 [2 * batch, H, W] (ResidentPIV: [2, batch, H, W]), reused
        self._mask_dev = None            # mask=: the image on the device, uint8 [H, W], once a run needs it
        self._eq_work = None             # equalize=: the table workspace, uint8 [n * ky * kx * 256], kept from launch to launch
        self._depth_range = (depth["lo"], depth["hi"]) if depth is not None and "lo" in depth else None
        self._depth_lut = None           # the tone-map table in use: uint8 [65536] on the device, once resolved
        self._depth_frames = None        # the mapped frames of a launch, uint8 [2 * batch, H, W] (ResidentPIV: [2, batch, H, W]), reused
        self._pf_frames = None           # over files (_prep_out): the filtered frames of a launch, uint8 [2 * batch, H, W], reused
        self._bg = None                  # the background in use: uint8 [2, H, W] on the device, once resolved
        self._bg_frames = None           # ResidentPIV (_prep_out): the frames of a launch minus the background / filtered, uint8 [2, batch, H, W], reused
        self._plan = None
        self._ens_plan = None            # the plan of ensemble(), made on first use
        self._single_plans = {}          # plans of the one-pair path, per frame shape
        self._reader = None              # the ReadAhead of the latest run over files (_raw_batches; closed when that run ended)
        self._stage, self._stage_key = None, None            # pinned staging buffers of _raw_batches, kept from call to call
        self._raw_dev, self._raw_dev_key = None, None        # their device copies
        self._pool, self._pool_size = None, 0                # fill-worker processes
        self._down_stream = None         # the stream of _post_submit's copies
        self._up_stream = None           # the stream of _raw_batches' uploads
        self.reset_stats()

    def __len__(self) -> int:
        return len(self._dataset)

    def _first_decodable(self, idx):
        """(pair id, frame shape) of the first pair of `idx` that decodes, None without one."""
        for i in idx:
            a, _ = self._dataset[i]
            if a is not None:
                return i, tuple(a.shape)
        return None

    def frame_shape(self):
        """(H, W) of the first decodable pair, None for an empty / undecodable folder."""
        first = self._first_decodable(range(len(self._dataset)))
        return None if first is None else first[1]

    def _make_plan(self, H, W, max_batch, **features):
        """A plan of this object's passes, outlier= and mask=, with the features the caller names."""
        return engine.Plan(H, W, int(self._wind_size), int(self._overlap), n_pass=max(1, int(self._iter)),
                           mode=self._mode, pass_scale=self._iter_scale, max_batch=max_batch, val_ratio=self._val_ratio,
                           val_win=self._val_win, device=self._device, precision=self._precision, outlier=self._outlier,
                           mask=self._mask, **features)

    def _new_plan(self, H, W, max_batch):
        return self._make_plan(H, W, max_batch, uncertainty=self._uncertainty, deform=self._deform,
                               correlation=self._correlation, weighting=self._weighting)

    def _get_plan(self, H, W, max_batch=1):
        if (self._plan is None or (self._plan.H, self._plan.W) != (H, W)
                or self._plan.max_batch < max_batch):
            if self._plan is not None:
                self._plan.close()
            self._plan = self._new_plan(H, W, max_batch)
        return self._plan

    def _staging(self, batch_size, cap):
        """(stage, raw_dev) for a run over files of `batch_size` pairs per batch and `cap` bytes per file slot: three
        page-locked staging buffers [2 * batch_size, cap] (one being read into, one uploading, one of slack) and two device
        copies, kept for the next call (page-locking half a gigabyte takes a tenth of a second)."""
        dev = self._device
        if self._reader is not None:
            # a reader that outlived its (abandoned) generator still fills the buffers ...
            self._reader.close()
            self._reader = None
            # ... and uploads / unpack kernels of that run may still be queued on ITS upload stream and on the compute
            # stream: the staging and device buffers are the same memory, and the new run's first upload carries no
            # dependency on them (an old upload landing afterwards would be unpacked as the new batch 0)
            torch.cuda.synchronize(dev)
        if self._stage_key != (batch_size, cap):
            self._stage = [torch.empty(2 * batch_size, cap, dtype=torch.uint8).pin_memory() for _ in range(3)]
            self._stage_key = (batch_size, cap)
        if self._raw_dev_key != (batch_size, cap, str(dev)):
            self._raw_dev = [torch.empty(2 * batch_size, cap, dtype=torch.uint8, device=dev) for _ in range(2)]
            self._raw_dev_key = (batch_size, cap, str(dev))
        return self._stage, self._raw_dev

    @property
    def depth_range_(self):
        """(lo, hi) of the tone map of depth=: the given range, or what depth="auto" found once it has run; None before
        that, for a caller's own table and without depth."""
        return self._depth_range

    def _depth_pairs(self, sample):
        """The uint16 frames (a, b) of the pairs engine.depth_sample picks from the whole dataset, on the device; pairs that
        cannot be decoded or have another frame shape than the dataset's are left out."""
        shape = self.frame_shape()
        for i in engine.depth_sample(len(self._dataset), sample):
            a, b = self._dataset[int(i)]
            if a is not None and b is not None and tuple(a.shape) == tuple(b.shape) == tuple(shape):
                yield a.to(self._device), b.to(self._device)

    def _side_stream(self, name, device):
        """The stream kept in attribute `name` for `device`, made on first use."""
        stream = getattr(self, name)
        if stream is None or stream.device != device:
            stream = torch.cuda.Stream(device)
            setattr(self, name, stream)
        return stream

    def _scratch(self, name, lead, H, W, device):
        """The reused uint8 buffer of attribute `name`, at least lead + (H, W) large: the one kept there if it has that
        rank, leading extents no smaller than `lead`, the frame shape (H, W) and the device; else a fresh one, kept."""
        buf = getattr(self, name)
        if buf is None or buf.dim() != len(lead) + 2 or any(have < need for have, need in zip(buf.shape, lead)) \
                or tuple(buf.shape[len(lead):]) != (H, W) or buf.device != device:
            buf = torch.empty(tuple(lead) + (H, W), dtype=torch.uint8, device=device)
            setattr(self, name, buf)
        return buf

    def _filtered(self, x, bg, out=None):
        """uint8 frames x [n, H, W] or [H, W] through the background and pre-filter step: with prefilter= one
        tpiv_prefilter launch that subtracts bg (uint8 [H, W], None: nothing) as well, else with bg the subtraction alone,
        else x itself.  out: where a step writes (None: a fresh tensor; the filter is a stencil, never in place)."""
        if self._prefilter is not None:
            return engine.prefilter(x, background=bg, out=out, **self._prefilter)
        if bg is not None:
            return engine.subtract_background(x, bg, out=out)
        return x

    def _finished(self, x, owned, out=None):
        """uint8 frames x through the last two steps in front of the passes: equalize, then mask pixels (one call each
        over x).  owned: x is memory this object made -- an upload, a reused buffer, a gathered copy -- and a step writes
        in place; a caller's tensor is never written: the first step that runs writes into out (None: a fresh tensor),
        and what it wrote is owned.  The one place that decides between in place and copy."""
        for on, step in ((self._equalize is not None, self._equalized),
                         (self._zeroes_pixels() and self._dynmask is None, self._masked)):
            if on:
                x = step(x, out=x if owned else out)
                owned = True
        return x

    def _equalized(self, frames, out=None):
        """uint8 frames [n, H, W] or [H, W] through equalize= (one tpiv_equalize call: the table and the map kernel), into
        out (None: a fresh tensor; _finished chooses).  The table workspace is kept from call to call."""
        eq = self._equalize
        n = frames.shape[0] if frames.dim() == 3 else 1
        ky, kx = engine.equalize_grid(frames.shape[-2], frames.shape[-1], eq["tile"])
        need = n * ky * kx * 256
        work = self._eq_work
        if work is None or work.numel() < need or work.device != frames.device:
            work = self._eq_work = torch.empty(need, dtype=torch.uint8, device=frames.device)
        return engine.equalize(frames, eq["tile"], eq["clip"], out=out, work=work)

    def _mask_shape(self, shape):
        """ValueError unless the mask image has the frame shape (None: not known, e.g. an undecodable folder)."""
        options.mask_shape(self._mask, shape)

    def _zeroes_pixels(self):
        if self._dynmask is not None:
            return self._dynmask["pixels"] == "zero"
        return self._mask is not None and self._mask["pixels"] == "zero"

    def _static_image(self, shape, device):
        """The image of mask= on `device` (uint8 [H, W]; it goes there once), None without mask=."""
        if self._mask is None:
            return None
        self._mask_shape(shape)
        img = self._mask_dev
        if img is None or img.device != device:
            img = self._mask_dev = self._mask["image"].to(device).contiguous()
        return img

    def _pair_masks(self, A, B, ids):
        """dynamic_mask=: the masks uint8 [n, H, W] of the pairs whose frames A, B [n, H, W] are (behind the background, in
        front of the pre-filter), mask='s image included: one tpiv_dynamic_mask call into a buffer kept from launch to
        launch, or the pairs `ids` of the caller's stack."""
        dm = self._dynmask
        n, H, W = (int(s_) for s_ in A.shape)
        static = self._static_image((H, W), A.device)
        if "stack" in dm:
            st = self._dm_stack
            if st is None or st.device != A.device:
                st = (dm["stack"].to(A.device) != 0)
                if static is not None:
                    st |= static != 0
                st = self._dm_stack = st.to(torch.uint8).contiguous()
            ids = list(ids)
            if ids == list(range(ids[0], ids[0] + n)):
                return st[ids[0]:ids[0] + n]
            return st.index_select(0, torch.tensor(ids, dtype=torch.int64, device=A.device))
        masks = self._scratch("_dm_masks", (n,), H, W, A.device)[:n]
        work = self._dm_work
        if work is None or work.numel() < n * H * W or work.device != A.device:
            work = self._dm_work = torch.empty(n * H * W, dtype=torch.uint8, device=A.device)
        return engine.dynamic_mask(A, B, dm["kind"], dm["size"], dm["level"], dm["grow"], static=static, out=masks, work=work)

    def _pair_chain(self, A, B, bg_a, bg_b, owned, out_a=None, out_b=None, ids=None, masks_only=False):
        """dynamic_mask=: the frames A, B (uint8 [n, H, W] or [H, W]) of the pairs `ids` from the background on -- background,
        segment, pre-filter and cap, equalize, mask pixels -- as (A, B, masks), each [n, H, W].  bg_a, bg_b: what is still to
        be subtracted (None: nothing, or done).  The subtraction runs on its own here, where prefilter= otherwise fuses it
        (the same bytes), because the segmentation reads its result.  owned / out_a, out_b: as in _finished -- a caller's
        frames are never written: the first step that runs writes elsewhere."""
        if A.dim() == 2:
            A, B = A[None], B[None]
            out_a, out_b = (None if o is None else o[None] if o.dim() == 2 else o for o in (out_a, out_b))
        n, H, W = (int(s_) for s_ in A.shape)
        if bg_a is not None:
            if owned:
                dst_a, dst_b = A, B
            else:                       # (not out_a: the pre-filter, a stencil, writes there next)
                buf = self._scratch("_dm_frames", (2, n), H, W, A.device)
                dst_a, dst_b = buf[0, :n], buf[1, :n]
            A, B = engine.subtract_background(A, bg_a, out=dst_a), engine.subtract_background(B, bg_b, out=dst_b)
            owned = True
        masks = self._pair_masks(A, B, ids)
        if masks_only:
            return None, None, masks
        fa, fb = self._filtered(A, None, out=out_a), self._filtered(B, None, out=out_b)
        owned |= fa is not A
        fa, fb = self._finished(fa, owned, out=out_a), self._finished(fb, owned, out=out_b)
        owned |= self._equalize is not None
        if self._zeroes_pixels():
            fa = engine.apply_mask_pairs(fa, masks, out=fa if owned else out_a)
            fb = engine.apply_mask_pairs(fb, masks, out=fb if owned else out_b)
        return fa, fb, masks

    def _prepared(self, raw, out=None):
        """(fa, fb, masks): the frames of a Raw record through the preparation steps -- background, pre-filter and cap,
        equalize, mask pixels (_filtered, _finished), with masks None; under dynamic_mask= the chain with the segmentation
        in it and the pairs' masks (_pair_chain).  out: where a step that may not write in place writes, uint8
        [2, n, H, W] (None: fresh tensors).  One launch per step and frame stack; where both stacks are one tensor of this
        object's (raw.stack, with out as contiguous), one launch per step over it -- only a pending background, one per
        stack, takes the two halves one by one."""
        out_a, out_b = (None, None) if out is None else (out[0], out[1])
        if self._dynmask is not None:
            return self._pair_chain(raw.A, raw.B, raw.bg_a, raw.bg_b, raw.owned, out_a, out_b, ids=raw.chunk)
        if raw.stack is not None:
            n, dst = len(raw.chunk), out.flatten(0, 1)
            if raw.bg_a is None:
                frames = self._filtered(raw.stack, None, out=dst)
            else:
                self._filtered(raw.A, raw.bg_a, out=out_a)
                self._filtered(raw.B, raw.bg_b, out=out_b)
                frames = dst
            frames = self._finished(frames, True)
            return frames[:n], frames[n:], None
        fa, fb = self._filtered(raw.A, raw.bg_a, out=out_a), self._filtered(raw.B, raw.bg_b, out=out_b)
        owned = raw.owned or fa is not raw.A
        return self._finished(fa, owned, out=out_a), self._finished(fb, owned, out=out_b), None

    def _run_masked(self, plan, fa, fb, masks):
        """dynamic_mask=: the passes on prepared frames with their masks; (u, v, inv, excluded) with excluded bool
        [n, n_rows, n_cols], the excluded cells of every pair in the orientation of the delivered fields (a copy, enqueued
        behind the run: the next launch overwrites the plan's grids)."""
        u, v, inv = plan.run_masked(fa, fb, masks, self._dynmask["threshold"])
        excluded = torch.flip(plan.pair_mask_grid(plan.n_pass - 1, int(u.shape[0]), sync=False), dims=(1,))
        return u, v, inv, excluded

    def _load_pair(self, i):
        """The Raw record of pair i alone: its uint8 frames on the device behind tone map and rectification, what is to be
        subtracted from them, and whether they are memory of this object.  None for an undecodable pair."""
        a, b = self._dataset[i]
        if a is None or b is None:
            return None
        a = a.to(self._device, non_blocking=True)
        b = b.to(self._device, non_blocking=True)
        shape = (int(a.shape[-2]), int(a.shape[-1]))
        lut = self._depth_table()
        if lut is not None:                             # uint16 as decoded -> uint8, right after the upload
            a, b = engine.depth_map(a, lut), engine.depth_map(b, lut)
        if self._dewarp is not None:                    # rectified next, into the reused buffer (stream order keeps a
            self._dewarp_shape(shape)                   # launch's passes ahead of the next write into it)
            buf = self._scratch("_dw_frames", (2,), shape[0], shape[1], a.device)
            a, b = self._dewarped(a, buf[0]), self._dewarped(b, buf[1])
        bg = self._background(shape)
        bg_a, bg_b = (None, None) if bg is None else (bg[0], bg[1])
        return Raw([(i, True)], [i], a, b, True, bg_a, bg_b)

    def pair_mask(self, i):
        """uint8 [H, W] numpy, 0 / 1: the mask pair i gets under dynamic_mask=, mask='s image included -- for tuning size
        and level.  None without the keyword or for a pair that cannot be decoded."""
        if self._dynmask is None:
            return None
        raw = self._load_pair(int(i))
        if raw is None:
            return None
        return self._pair_chain(raw.A, raw.B, raw.bg_a, raw.bg_b, raw.owned, ids=raw.chunk, masks_only=True)[2][0].cpu().numpy()

    def _masked(self, frames, out=None):
        """uint8 frames [n, H, W] or [H, W] through the pixel step of mask= (one tpiv_apply_mask call), into out (None: a
        fresh tensor; _finished chooses).  The image goes to the device once."""
        return engine.apply_mask(frames, self._static_image(frames.shape[-2:], frames.device), out=out)

    def _dewarp_shape(self, shape):
        """ValueError unless a map given as coordinate arrays has the frame shape (None: not known)."""
        options.dewarp_shape(self._dewarp, shape)

    def _dewarp_map(self, shape, device):
        """The Q8 map of dewarp= for frames of `shape` on `device` (int32 [H, W, 2]): built on the host, checked and
        uploaded once per object and device."""
        m = self._dw_map
        if m is None or tuple(m.shape[:2]) != tuple(shape) or m.device != device:
            self._dewarp_shape(shape)
            m = self._dw_map = engine.dewarp_upload(engine.dewarp_map(self._dewarp, shape[0], shape[1]), device)
        return m

    def _dewarped(self, x, out, offsets=None, shape=None):
        """uint8 frames through dewarp= (one tpiv_dewarp launch) into out, memory of this object: x [n, H, W] or [H, W], or
        a flat buffer whose frames `offsets` address (shape = (H, W)).  The source is not written."""
        dw = self._dewarp
        m = self._dewarp_map(tuple(x.shape[-2:]) if offsets is None else tuple(shape), x.device)
        return engine.dewarp(x, m, dw["interp"], dw["fill"], offsets=offsets, shape=shape, out=out)

    def dewarp_outside(self):
        """bool [H, W]: the pixels of the rectified frames whose source lies outside the camera frame and that carry the
        fill value of dewarp= -- fit to be passed as mask=.  None without dewarp= or without a decodable pair."""
        shape = self.frame_shape()
        if self._dewarp is None or shape is None:
            return None
        self._dewarp_shape(shape)
        return engine.dewarp_outside(engine.dewarp_map(self._dewarp, shape[0], shape[1]))

    def _fill_grid(self, plan):
        """(grid, grid on the device): the excluded cells of the plan's last pass as bool [n_rows, n_cols] in the orientation
        of the delivered fields (flipped along axis 0), kept on the plan."""
        got = getattr(plan, "_fill_grid", None)
        if got is None:
            dev = torch.flip(plan.mask_grid(plan.n_pass - 1), dims=(0,)).contiguous()
            got = plan._fill_grid = (dev.cpu().numpy(), dev)
        return got

    def mask_grid(self):
        """bool [n_rows, n_cols]: the cells of the delivered u, v that are excluded by mask= and carry its fill value, in
        their orientation (flipped along axis 0 against Plan.mask_grid).  None without a mask or without a decodable pair."""
        shape = self.frame_shape()
        if self._mask is None or shape is None:
            return None
        return self._fill_grid(self._single_plan((int(shape[0]), int(shape[1]))))[0].copy()

    def _single_plan(self, shape):
        """The plan of the one-pair path for frames of shape (H, W), made on first use and kept."""
        plan = self._single_plans.get(shape)
        if plan is None:
            plan = self._single_plans[shape] = self._new_plan(shape[0], shape[1], 1)
        return plan

    def _depth_table(self):
        """The tone-map table of depth= on the device (uint8 [65536]), None without depth.  "auto" takes the histogram of
        both frames of the sampled pairs here (one common histogram, so frame a and frame b get the same map), once per
        object -- always over the whole dataset, whatever part of it a run then processes, so that every rank of a
        sharded run finds the same range without a collective."""
        d = self._depth
        if d is None:
            return None
        if self._depth_lut is None:
            if "lut" in d:
                table = d["lut"]
            else:
                if "auto" in d:
                    acc = None
                    for a, b in self._depth_pairs(d["sample"]):
                        acc = engine.depth_histogram(b, engine.depth_histogram(a, acc))
                    if acc is None:
                        raise ValueError("depth='auto': none of the sampled pairs could be decoded")
                    self._depth_range = engine.depth_range(acc.cpu().numpy(), d["clip_low"], d["clip_high"])
                table = engine.depth_lut(self._depth_range[0], self._depth_range[1], d["curve"])
            self._depth_lut = torch.from_numpy(table).to(self._device)
        return self._depth_lut

    def _map_staged(self, raw_d, st, H, W, lut, batch_size):
        """The staged uint16 slots of a batch (raw_d uint8 [files, cap] on the device, io.StagedBatches(deep=True)) through
        the tone map, one launch: uint8 [2n, H, W] = a_0..a_n-1, b_0..b_n-1, in a buffer kept from batch to batch."""
        buf = self._scratch("_depth_frames", (2 * batch_size,), H, W, raw_d.device)
        off = torch.from_numpy(st.desc[:, 0] // 2)              # the slots' element offsets, every a, then every b
        return engine.depth_map(raw_d.view(-1).view(torch.uint16), lut, offsets=off, shape=(H, W), out=buf[:off.shape[0]])

    def _background(self, shape, batch_size=None):
        """The background the frames of shape (H, W) lose (uint8 [2, H, W] on the device: bg_a, bg_b), None without one.
        "min" runs compute_background() here, once per object."""
        if self._bg_arg is None:
            return None
        if self._bg is None:
            if self._bg_arg == "min":
                self._set_background(*self.compute_background(batch_size=batch_size))
            else:
                self._set_background(*self._bg_arg)
        if tuple(self._bg.shape[1:]) != tuple(shape):
            raise ValueError(f"background of shape {tuple(self._bg.shape[1:])} for frames of shape {tuple(shape)}")
        return self._bg

    def _set_background(self, bg_a, bg_b):
        self._bg = torch.stack([bg_a.to(self._device), bg_b.to(self._device)]).contiguous()

    bg_batch = 32            # pairs per upload of compute_background (default)

    def compute_background(self, indices=None, batch_size=None):
        """(bg_a, bg_b): the per-pixel minimum over the a frames and over the b frames of the pairs `indices` (None: every
        pair of the dataset) as uint8 [H, W] tensors on the device -- what background="min" subtracts.  Pairs that cannot
        be decoded or whose frame shape differs from the dataset's (frame_shape()) are left out; with none left both
        images are 255 everywhere (the identity of the minimum: a rank's empty shard).  The frames come from the raw
        source of batched() (_raw_batches: over files the native read-ahead ring and the device unpack, whose staging
        buffers the two share when batch_size and the file size agree), and each batch is folded in with tpiv_frame_min.
        With depth= the minimum is taken over the tone-mapped frames (depth="auto" resolves here first), with dewarp=
        over the rectified frames."""
        shape = self.frame_shape()
        if shape is None:
            raise ValueError("compute_background: the dataset holds no decodable pair")
        H, W = shape
        acc = torch.full((2, H, W), 255, dtype=torch.uint8, device=self._device)
        idx = list(range(len(self._dataset))) if indices is None else list(indices)
        if idx:
            first = self._first_decodable(idx)
            with contextlib.closing(self._raw_batches(idx, int(batch_size or self.bg_batch), H, W, None,
                                                      None if first is None else first[0])) as source:
                for raw in source:
                    if raw.chunk:           # (pairs that are not staged are left out, as batched() leaves them to the one-pair path)
                        engine.frame_min(raw.A, acc[0])
                        engine.frame_min(raw.B, acc[1])
        return acc[0], acc[1]

    def _ensemble_plan(self, H, W, max_batch):
        """The plan of ensemble(): this object's passes with ensemble=True, kept like the plan of batched()."""
        plan = self._ens_plan
        if plan is None or (plan.H, plan.W) != (H, W) or plan.max_batch < max_batch:
            if plan is not None:
                plan.close()
            plan = self._ens_plan = self._make_plan(H, W, max_batch, ensemble=True)
        return plan

    def _ensemble_check(self):
        options.refuse("ensemble", dict(dynamic_mask=self._dynmask, correlation=self._correlation, weighting=self._weighting,
                                        uncertainty=self._uncertainty, deform=self._deform),
                       [w for w, _ in engine.pass_sizes(self._wind_size, self._overlap, self._iter, self._iter_scale)])

    def _raw_batches(self, idx, batch_size, H, W, bg, like=None):
        """The raw frame source over files: one Raw record per batch_size pairs of idx -- read by the native reader threads
        (io.ReadAhead) into pinned staging memory, uploaded, and unpacked (uncompressed BMPs, with the background bg
        [2, H, W] subtracted in the same kernel) or tone-mapped (depth=) and rectified (dewarp=) on the device; these two
        leave bg to the consumer.  A batch none of whose pairs is staged comes with frames None; its order tells the
        consumer which pairs to run one by one.  The frames live in memory that a later batch overwrites: the consumer
        enqueues its work on the current stream before it asks for the next batch, and stream order protects them; the
        events below protect the device copies of the staging slots and the staging memory.  The one place that stages
        files: closing the generator (also mid-run) stops the reader threads and waits for the device.  like: a decodable
        pair of idx, whose files size the staging slots."""
        dev = self._device
        lut = self._depth_table()                     # (depth="auto": the histogram prepass runs here, once, before _staging)
        deep, dewarp = lut is not None, self._dewarp is not None
        fused = None if deep or dewarp else bg        # (a background is in rectified coordinates and mapped units)
        bg_a, bg_b = (None, None) if bg is None or fused is not None else (bg[0], bg[1])
        pairs = self._dataset.img_pairs
        cap = slot_bytes(H, W, pairs[like] if like is not None else (), deep=deep)
        stage, raw_dev = self._staging(batch_size, cap)
        # the host side of the loop below: read-ahead ring, header sweep, host decode of other formats, descriptor tables
        batches = StagedBatches(idx, pairs, batch_size, H, W, [t.numpy() for t in stage], cap, threads=self.read_threads,
                                deep=deep)
        self._reader = batches.reader
        # uploads run on their own stream into a double-buffered device copy of the staging slots, so that the PCIe
        # transfer of batch n + 1 (4 MP: 268 MB, ~5 ms) overlaps the passes of batch n (~3 ms) instead of preceding them
        cur = torch.cuda.current_stream(dev)
        up_stream = self._side_stream("_up_stream", dev)     # (kept: a stream's first use costs milliseconds)
        consumed = [None, None]             # event: the unpack kernel that read raw_dev[k] has run
        release = None                      # upload event of the batch before (its staging buffer is still held)
        n_up = 0

        def let_go(rel):
            if rel is not None:
                if rel[0] is not None:
                    rel[0].synchronize()              # its upload is through: the readers may refill the staging buffer
                batches.release()

        try:
            for k, st in enumerate(batches):
                up, frames, n = None, None, len(st.chunk)
                if n:
                    dbuf, n_up = n_up % 2, n_up + 1
                    with torch.cuda.stream(up_stream):
                        if consumed[dbuf] is not None:
                            up_stream.wait_event(consumed[dbuf])
                        raw_d = raw_dev[dbuf][:st.n_files]
                        raw_d.copy_(stage[st.buf][:st.n_files], non_blocking=True)
                        up = torch.cuda.Event()
                        up.record(up_stream)
                    # unpacked frame order: every a of the batch, then every b (two contiguous stacks)
                    if not deep:
                        desc_d = torch.from_numpy(st.desc).to(dev, non_blocking=True)
                        lut_d = torch.from_numpy(st.lut).to(dev, non_blocking=True)
                    cur.wait_event(up)
                    if deep:
                        # the tone map where the unpack sits: one launch, slots a0 b0 a1 b1 .. -> stacks a_0..a_n-1, b_0..b_n-1
                        frames = self._map_staged(raw_d, st, H, W, lut, batch_size)
                    else:
                        frames = engine.bmp_unpack(raw_d.view(-1), desc_d, lut_d, H, W, background=fused)
                    consumed[dbuf] = torch.cuda.Event()
                    consumed[dbuf].record(cur)
                    if dewarp:
                        # one launch over both stacks, into a buffer kept from batch to batch
                        frames = self._dewarped(frames, self._scratch("_dw_frames", (2 * batch_size,), H, W, dev)[:2 * n])
                # the staging buffer of the batch before goes back now, with this batch's upload and unpack enqueued -- not
                # when the consumer resumes this generator: that is behind its host work, and the readers, which bound the
                # file path, then wait for a buffer (measured: 6.3 k -> 4.3 k pairs/s in half of the runs)
                let_go(release)
                release = (up,)
                yield Raw(st.order, st.chunk, frames[:n] if n else None, frames[n:] if n else None, True, bg_a, bg_b,
                          (k + 1) * batch_size >= len(idx), frames)
            let_go(release)
        finally:
            # consumer finished, raised, or abandoned the run (GeneratorExit lands here): stop the reader threads, then wait
            # for every upload / unpack still queued (they read the staging buffers and write raw_dev, which the next run
            # over files on this object reuses with no events to order itself behind)
            batches.close()
            torch.cuda.synchronize(dev)

    def _prep_out(self, raw, batch_size, H, W):
        """Where _prepared writes what it may not write in place, uint8 [2, n, H, W]: over files the uploaded stacks
        themselves; only the pre-filter, a stencil, writes a buffer kept from batch to batch (stream order keeps a
        batch's passes ahead of the next batch's filter)."""
        n = len(raw.chunk)
        dst = raw.stack if self._prefilter is None else \
            self._scratch("_pf_frames", (2 * batch_size,), H, W, raw.stack.device)[:2 * n]
        return dst.view(2, n, H, W)

    def _frame_batches(self, idx, batch_size, H, W, like):
        """The prepared frame source of batched(), ensemble() and tracks(): (raw, fa, fb, masks) per batch_size pairs of idx
        -- the Raw record of _raw_batches, and its frames through the preparation steps (_prepared: background,
        pre-filter, equalize, mask pixels; masks under dynamic_mask= only) as uint8 [n, H, W] on the device; fa None for
        a batch without a staged pair.  The stacks live in buffers of this object that the next batch overwrites: the
        consumer enqueues its work on the current stream before it asks for the next one.  Closing this generator closes
        the raw source."""
        self._depth_table()                           # depth="auto" and background="min" run their own pass over the
        if self._dewarp is not None:                  # dataset: here, before the raw source stages anything
            self._dewarp_shape((H, W))
        bg = self._background((H, W), batch_size)
        with contextlib.closing(self._raw_batches(idx, batch_size, H, W, bg, like)) as source:
            for raw in source:
                if raw.chunk:
                    yield (raw,) + self._prepared(raw, self._prep_out(raw, batch_size, H, W))
                else:
                    yield raw, None, None, None

    def ensemble(self, indices=None, batch_size: int = 32):
        """Ensemble (sum-of-correlation) PIV over the pairs `indices` (None: all): ONE field (x, y, u, v) from the summed
        correlation maps of all of them (Meinhart, Wereley & Santiago 2000), for recordings too sparsely seeded for single
        pairs.  Every pass adds the maps of all pairs window by window and takes the peak of the mean map once; later
        passes shift every pair's windows by the one predictor of the ensemble field before (engine.Plan.run_ensemble).
        The frames go through the preparation steps of batched(); a recording on disk is read once per pass.  outlier=
        and the grid of mask= apply through the plan, pass by pass, as they do to a pair's fields.  The tuple is finished
        like those of __call__: post-validation (holes filled from their ring), flip, sign, scale / dt -- except that a
        field without a single invalid vector is delivered as it is (the reference drops such a PAIR, B:300-304; for an
        ensemble it is the expected result).  None when the post-validation drops the field (a quarter of the cells or
        more in the ring) or no pair could be read.  Window sizes 16, 32, 64 in every pass (NotImplementedError);
        ValueError with uncertainty= or deform=.  precision= plays no part: the maps are float32."""
        self._ensemble_check()
        idx = list(range(len(self._dataset))) if indices is None else list(indices)
        first = self._first_decodable(idx) if idx else None
        if first is None:
            return None
        H, W = first[1]
        batch_size = int(batch_size)
        plan = self._ensemble_plan(H, W, batch_size)

        def chunks():                           # one pass over the recording; unstaged pairs are left out
            with contextlib.closing(self._frame_batches(idx, batch_size, H, W, first[0])) as batches:
                for raw, fa, fb, _ in batches:
                    if raw.chunk:
                        yield fa, fb
        u, v, inv = plan.run_ensemble(chunks)
        return self._ensemble_finish(plan, (H, W), u, v, inv)

    def _ensemble_finish(self, plan, shape, u, v, inv):
        w, o, _, _ = plan.geometry[-1]
        x, y = get_coordinates(shape, w, o)
        if not bool(inv.any()):
            uv = (u[0].cpu().numpy(), v[0].cpu().numpy())       # nothing to fill, nothing on the border to interpolate
        else:
            uv = self._post_validate_batch(u, v, inv, plan=plan, sigma=False)[0]
        return self._finish(uv, x, y, plan=plan)

    def single_pixel(self, radius: int = 4, bin=1, shift=(0, 0), min_ratio=None, indices=None, batch_size: int = 32,
                     planes: bool = False):
        """Single-pixel ensemble correlation (Westerweel, Geelhoed & Lindken 2004; Kaehler, Scholz & Ortmanns 2006;
        Scharnowski, Hain & Kaehler 2012) over the pairs `indices` (None: all): ONE field (x, y, u, v, q) whose cells are
        bins of bin = k or (k_y, k_x) pixels, k_y * k_x <= 256 -- a single pixel, or e.g. one image row (1, W) of a
        channel flow -- from the correlation summed over the recording instead of over a window, for steady flows
        recorded with many pairs.  radius: the search radius R in 3..16 pixels around shift = (s_y, s_x), ONE integer
        pre-shift (|s| <= 64) for every bin: a displacement is found within (-R, R) of it.  At most 65536 pairs.
        The frames go through the preparation steps of batched() (pairs that cannot be staged are left out) and the
        recording is read once.  x, y: the bin centres times scale (get_coordinates' geometry at window = bin, overlap
        0, per axis); u, v: flip, sign and scale / dt * 1000 as in every delivered field; q: a SinglePixel record, flipped
        like the field, of peak (the correlation coefficient at the peak), ratio (peak to second peak), status (uint8:
        engine.PIXEL_CORR_STATUS) and pairs (the pairs summed), plus corr [n_by, n_bx, D, D], the coefficient planes, with
        planes=True.  A bin whose status is not 0 carries NaN: 1 within reach of the frame edge, 2 constant pixels, 3
        peak on the rim of the search area, 4 no sub-pixel fit, 5 ratio below min_ratio (None: no such test); with mask=
        a bin whose masked share exceeds the mask's threshold has status 6 and the mask's fill value.  None when no pair
        could be read.  ValueError with dynamic_mask=; MemoryError when the accumulator does not fit the free device
        memory.  The window size, the passes, precision=, outlier=, deform=, correlation=, weighting= and uncertainty=
        play no part here; there is no per-bin predictor."""
        idx = list(range(len(self._dataset))) if indices is None else list(indices)
        par = engine.single_pixel_arg(radius, bin, shift, min_ratio)
        if self._dynmask is not None:
            raise ValueError("single_pixel: dynamic_mask= is not supported (one sum over all pairs has no per-pair mask); "
                             "use mask=, or run without it")
        if len(idx) > engine.PIXEL_CORR_PAIRS:
            raise ValueError(f"single_pixel: at most {engine.PIXEL_CORR_PAIRS} pairs, got {len(idx)}")
        first = self._first_decodable(idx) if idx else None
        if first is None:
            return None
        H, W = first[1]
        engine.single_pixel_arg(radius, bin, shift, min_ratio, shape=(H, W))
        (ky, kx), R = par["bin"], par["radius"]
        dev = self._device
        need = engine.pixel_corr_bytes(H, W, (ky, kx), R) + 4 * H * W * 8
        free = torch.cuda.mem_get_info(dev)[0]
        if need > free:
            raise MemoryError(f"single_pixel: the accumulators of bin {(ky, kx)} at radius {R} take {need} bytes, the device "
                              f"has {free} free: use a larger bin or a smaller radius")
        if self._mask is not None:
            self._mask_shape((H, W))
        acc = mom = None
        n = 0
        with contextlib.closing(self._frame_batches(idx, int(batch_size), H, W, first[0])) as batches:
            for raw, fa, fb, _ in batches:
                if raw.chunk:                   # (unstaged pairs are left out)
                    acc, mom = engine.pixel_corr_add(fa, fb, (ky, kx), R, par["shift"], acc=acc, mom=mom)
                    n += len(raw.chunk)
        if not n:
            return None
        out = engine.pixel_corr_peaks(acc, mom, n, (H, W), (ky, kx), R, par["shift"], planes=planes)
        u, v, peak, ratio, status = (t.cpu().numpy() for t in out[:5])
        if par["min_ratio"] is not None:
            low = (status == 0) & (ratio < par["min_ratio"])
            status[low] = engine.PIXEL_CORR_STATUS["ratio"]
            for t in (u, v, peak, ratio):
                t[low] = np.nan
        if self._mask is not None:              # the coverage of every bin, counted once on the host
            img = (self._mask["image"].cpu().numpy() != 0)[:H // ky * ky, :W // kx * kx]
            share = img.reshape(H // ky, ky, W // kx, kx).sum(axis=(1, 3)) / float(ky * kx)
            out_ = share > self._mask["threshold"]
            status[out_] = engine.PIXEL_CORR_STATUS["masked"]
            peak[out_] = ratio[out_] = np.nan
            u[out_] = v[out_] = np.nan          # (the fill goes in below, behind sign and scale)
        xs, ys = engine.pixel_corr_coordinates(H, W, (ky, kx))
        x, y = np.meshgrid(xs, ys)
        u = np.flip(u, axis=0) * self._scale / self._dt * 1000
        v = -np.flip(v, axis=0) * self._scale / self._dt * 1000
        peak, ratio, status = (np.flip(t, axis=0).copy() for t in (peak, ratio, status))
        if self._mask is not None:
            u[status == engine.PIXEL_CORR_STATUS["masked"]] = self._mask["fill"]
            v[status == engine.PIXEL_CORR_STATUS["masked"]] = self._mask["fill"]
        q = SinglePixel(peak, ratio, status, n, np.flip(out.corr.cpu().numpy(), axis=0).copy() if planes else None)
        return x * self._scale, y * self._scale, u, v, q

    def tracks(self, level, radius=engine.TRACKS_RADIUS, indices=None, batch_size: int = 32) -> Generator:
        """Hybrid PIV / PTV ("super-resolution" PIV: Keane, Adrian & Zhang 1995; Cowen & Monismith 1997) over the pairs
        `indices` (None: all): the converged field of a pair predicts where each particle image of frame a lies in frame b,
        and each is paired with the nearest particle image there -- one unbinned vector per particle, at the particle's
        own position.  level: the intensity a particle image's peak pixel must reach, an integer in 1..255, required;
        radius: the search radius around the predicted position in pixels, in (0, 8] (engine.tracks_arg).

        Yields (i, x, y, u, v, t) for every pair the post-validation keeps, batch_size pairs per launch: x, y, u, v are what
        batched() delivers for that pair (numpy arrays; uncertainty= and derive= do not apply to tracks() and add nothing
        to its tuples), t is a Tracks record of numpy arrays over the matched particles only, in raster order of frame a:
          x, y         the position in frame a: image coordinates (x along the columns, y along the rows DOWNWARD, pixel
                       (0, 0) centred at the origin) times scale, millimetres
          u, v         (x_b - x_a) * scale / dt * 1000 and -(y_b - y_a) * scale / dt * 1000: the units and signs of the
                       delivered fields, v positive upward in the image
          residual     the distance between the predicted and the found position in frame b, pixels
          peak_a, peak_b    the peak pixels' intensities
          count_a, count_b, matched    particle images found in either frame, and pairs made (= len(t.x))
        How this relates to the delivered grid: its rows are flipped -- cell [r, c] of the delivered u, v was measured by the
        window whose centre lies at column x[r, c] and image row y[n_rows - 1 - r, c] of the coordinates get_coordinates
        returns (engine.stereo_cells applies the same flip) -- while t.y is the image row itself times scale and is never
        flipped; t.v has the delivered sign, positive toward smaller t.y.
        The frames are prepared as batched() prepares them (pairs that cannot be decoded, or have another frame shape than
        the first, are left out); the particle images are detected on the prepared frames (engine.particle_detect), mask=
        hands its image to the detection (no particle under it), and the predictor is the pair's raw field after the
        post-validation has filled it, interpolated bilinearly between the centres of the last pass's windows
        (engine.particle_match).  deform=, correlation=, weighting= and outlier= act through the plan as in batched().
        ValueError with dynamic_mask=; the arguments are checked at the call, the work starts at the first next()."""
        par = self._tracks_check(level, radius)
        idx = list(range(len(self._dataset))) if indices is None else list(indices)
        first = self._first_decodable(idx) if idx else None
        return self._tracks(par, idx, first, int(batch_size)) if first is not None else iter(())

    def _tracks_check(self, level, radius):
        """The checked arguments of tracks(); ValueError with dynamic_mask=."""
        par = engine.tracks_arg(level, radius)
        if self._dynmask is not None:
            raise ValueError("tracks: dynamic_mask= is not supported (the detection takes one mask image for every pair); "
                             "use mask=, or run without it")
        return par

    def _tracks(self, par, idx, first, batch_size):
        """tracks() over the pairs idx, whose first decodable pair and frame shape are `first`, with the checked arguments par."""
        like, (H, W) = first
        plan = self._get_plan(H, W, max_batch=batch_size)
        w, o, _, _ = plan.geometry[-1]
        x, y = get_coordinates((H, W), w, o)
        nr, nc = x.shape
        # the centres of the windows in image coordinates: window k covers the pixels k (w - o) .. k (w - o) + w - 1
        xc, yc = np.arange(nc) * float(w - o) + (w - 1) / 2, np.arange(nr) * float(w - o) + (w - 1) / 2
        dev = self._device
        image = self._static_image((H, W), dev)
        with contextlib.closing(self._frame_batches(idx, batch_size, H, W, like)) as batches:
            for src, A, B, _ in batches:
                chunk = src.chunk
                if not chunk:           # (none of the batch's pairs is staged: left out)
                    continue
                u, v, inv = plan.run(A, B)
                pa = engine.particle_detect(A, par["level"], mask=image)      # on the frame buffers, before the next batch
                pb = engine.particle_detect(B, par["level"], mask=image)
                raw = self._post_validate_batch(u, v, inv, plan=plan, sigma=False)
                kept = [k for k, uv in enumerate(raw) if uv is not None]
                if not kept:
                    continue
                pred = np.zeros((2, len(chunk), nr, nc))
                for k in kept:
                    pred[0, k], pred[1, k] = raw[k]
                pred = torch.from_numpy(pred).to(dev)
                m = engine.particle_match(pa, pb, pred[0], pred[1], xc, yc, par["radius"], (H, W))
                host = [t.cpu().numpy() for t in (pa.x, pa.y, pa.peak, pa.count, pb.x, pb.y, pb.peak, pb.count) + tuple(m)]
                for k in kept:
                    t = self._tracks_of(*(a[k] for a in host))
                    yield (chunk[k],) + self._finish(raw[k], x, y, plan=plan, derive=False) + (t,)

    def _tracks_of(self, xa, ya, peak_a, count_a, xb, yb, peak_b, count_b, match, status, d2, matched):
        """The Tracks of one pair from its two lists and engine.particle_match's verdicts (numpy): the matched particles in
        frame a's order, positions and displacements in the delivered units and signs."""
        ia = np.flatnonzero(status == engine.PARTICLE_STATUS["matched"])
        ib = match[ia]
        return Tracks(xa[ia] * self._scale, ya[ia] * self._scale,
                      (xb[ib] - xa[ia]) * self._scale / self._dt * 1000, -(yb[ib] - ya[ia]) * self._scale / self._dt * 1000,
                      np.sqrt(d2[ia]), peak_a[ia], peak_b[ib], int(count_a), int(count_b), int(matched))

    def reset_stats(self):
        """Counters of the post-validation: pairs seen, dropped for 'no invalid vector' / 'too many
        false vectors' (decided on the device), finished on the device alone, sent to the host
        triangulation (and dropped there because Qhull refused the ring)."""
        self.stats = {"pairs": 0, "dropped_no_invalid": 0, "dropped_too_many": 0, "device_complete": 0,
                      "host_fallback": 0, "dropped_by_qhull": 0,
                      # host_fallback by hole class: pairs whose only undetermined cells are co-circular
                      # diamonds (isolated invalid vectors: Qhull's tie-break decides), and pairs that hold a wider hole
                      "host_fallback_diamonds_only": 0, "host_fallback_wide_holes": 0,
                      # outlier=...: vectors the test flagged in the last pass (they join the peak-ratio holes)
                      "outliers_flagged": 0}

    fill_workers = 0         # > 0: the host triangulations of a batch run in that many worker processes
    pipeline_depth = 2       # batched() over files: launches in flight before a batch's results are collected
    read_threads = 8         # file reader threads of batched() (a page-cache read into pinned memory runs at ~3 GB/s per thread)
    device_out = False       # batched(): yield u, v as float64 tensors ON THE DEVICE (the finished fields of B:894-898, hole
                             # fills scattered in from the host) instead of numpy arrays -- for callers that go on with them
                             # on the GPU (dist.run_sharded: the end-of-run gather over xGMI)

    def _in_flight(self):
        """Launches of batched() in flight before a batch's results are collected."""
        return self.pipeline_depth

    def auto_host_config(self, ranks_on_node=None):
        """Size the reader threads and the fill-worker processes from the cores this rank really has (affinity mask and
        container quota divided by the ranks of the node, torchpiv_amd.hostcfg) instead of the single-GPU defaults.
        Returns the budget dict."""
        from . import hostcfg
        b = hostcfg.host_budget(ranks_on_node)
        self.read_threads, self.fill_workers = b["read_threads"], b["fill_workers"]
        return b

    def _fill_pool(self):
        """The fill-worker processes (_qhull.FillWorkers), started on first use and again when fill_workers changes."""
        if self.fill_workers <= 0:
            return None
        pool = self._pool
        if pool is None or self._pool_size != self.fill_workers:
            if pool is not None:
                pool.terminate()
            # spawned: the workers never see this process's HIP state; they only run scipy on small arrays (with ONE BLAS
            # thread each: _qhull.single_thread_blas)
            from ._qhull import FillWorkers
            self._pool = pool = FillWorkers(self.fill_workers)
            self._pool_size = self.fill_workers
        return pool

    def close(self):
        if self._pool is not None:
            self._pool.terminate()
            self._pool = None
        if self._plan is not None:
            self._plan.close()
            self._plan = None
        if self._ens_plan is not None:
            self._ens_plan.close()
            self._ens_plan = None
        if self._reader is not None:
            self._reader.close()
            self._reader = None
        self._stage, self._stage_key = None, None
        self._raw_dev, self._raw_dev_key = None, None
        for pl in self._single_plans.values():
            pl.close()
        self._single_plans = {}

    RING_CAP = 256           # ring / hole cells per pair (batch average) that ride on the first, asynchronous copy

    def _post_submit(self, u, v, inv, want_raw=False, plan=None, sigma=True, excluded=None):
        """Device half of B:884-898 for a batch of final fields (u, v float64 [n, nr, nc], modified in
        place; inv uint8): tpiv_postval (NaN-out, border interpolation, census, triangulation-free fills),
        tpiv_postval_compact (the ring points with their values and the hole cells of the pairs that need Qhull, cut out
        and packed in np.argwhere order on the device), the flip and the unit scaling of B:894-898 (the reference's own
        float64 expressions -- u * scale / dt * 1000, three correctly rounded operations -- evaluated by the device on
        the whole batch: bit-identical, and the host is spared five passes over every field), then ASYNCHRONOUS copies of
        the census, the packed lists and the finished fields into pinned memory, on a stream of their own.  Nothing here
        waits for the GPU: the caller may enqueue the next batch before it collects this one.  want_raw: also the raw
        (unflipped, unscaled) fields, for callers of the function-level API.  sigma=False: leave the uncertainty= fields out
        (the one-pair path fetches and finishes them itself)."""
        cls, counts = engine.postval(u, v, inv)
        offsets, ring_rc, ring_uv, hole_rc = engine.postval_compact(u, v, cls, counts)
        fu, fv = engine.finish_fields(u, v, self._scale, self._dt)
        n = u.shape[0]
        cap_r, cap_h = min(ring_rc.shape[0], n * self.RING_CAP), min(hole_rc.shape[0], n * self.RING_CAP)
        src = {"counts": counts, "offsets": offsets, "ring_rc": ring_rc[:cap_r], "ring_uv": ring_uv[:cap_r],
               "hole_rc": hole_rc[:cap_h], "fu": fu, "fv": fv}
        if want_raw:
            src["u"], src["v"] = u, v
        if excluded is not None:                                # dynamic_mask=: where _finish_batch puts the fill value
            src["excluded"] = excluded
        if plan is not None and plan.outlier is not None:
            src["flagged"] = plan.outlier_flag_counts(n)       # rides on the same asynchronous copy as the census
        if sigma and plan is not None and plan.uncertainty_par is not None:
            # uncertainty=: copied out of the plan's buffers now (the next launch overwrites them while this one's results
            # are still in flight), flipped and scaled like the fields; sigma is unsigned, so the sign of fv is taken back
            su, sv = engine.finish_fields(*plan.uncertainty(n), self._scale, self._dt)
            src["fsu"], src["fsv"] = su, sv.neg_()
        host = {k: torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for k, t in src.items()}
        # the copies go down on a stream of their own, behind an event of the compute stream: the next batch's passes
        # start while they run.  (The small kernels above stay on the compute stream: on the side stream too they made
        # the whole generator slower -- 9.1 -> 8.2 k pairs/s, same box.)
        cur = torch.cuda.current_stream(u.device)
        down = self._side_stream("_down_stream", u.device)
        ready = torch.cuda.Event()
        ready.record(cur)
        with torch.cuda.stream(down):
            down.wait_event(ready)
            for k, t in src.items():
                host[k].copy_(t, non_blocking=True)
            done = torch.cuda.Event()
            done.record(down)
        # (every device tensor the copy stream reads stays referenced until the ticket is collected, i.e. past `done`;
        #  the full lists serve the overflow path)
        return done, host, (src, ring_rc, ring_uv, hole_rc, u, v)

    def _post_extract(self, ticket, owner=None):
        """Host half, first stage: drop decisions from the census; the pairs that hold an ambiguous or wide hole
        (counted) arrive with their ring points, values and hole cells already cut out (tpiv_postval_compact) and go to
        the triangulation -- in worker processes when fill_workers > 0: the jobs are handed out here and the answers read
        by _post_complete, so whatever the caller does in between (the next launch, the batch before) overlaps them.
        owner: names the pipeline these jobs belong to in the pool that all pipelines of this object share.
        Returns the state _post_complete takes."""
        done, host, keep_alive = ticket
        done.synchronize()
        cnt = host["counts"].numpy().astype(np.int64)                # [n, 4] holes, ring, ambiguous, general
        nr, nc = host["fu"].shape[1:]
        n = cnt.shape[0]
        ring = cnt[:, 1]
        no_ring = ring == 0                  # nothing to interpolate from (B:300-304; the clean-pair quirk)
        too_many = ~no_ring & (4 * ring >= nr * nc)                  # points.size >= mask.size / 2 (B:299, 305)
        keep = ~no_ring & ~too_many
        need_host = keep & ((cnt[:, 2] + cnt[:, 3]) > 0)
        st = self.stats
        st["pairs"] += n
        if "flagged" in host:
            st["outliers_flagged"] += int(host["flagged"].sum())
        st["dropped_no_invalid"] += int(no_ring.sum())
        st["dropped_too_many"] += int(too_many.sum())
        st["device_complete"] += int((keep & ~need_host).sum())
        st["host_fallback_diamonds_only"] += int((need_host & (cnt[:, 3] == 0)).sum())
        st["host_fallback_wide_holes"] += int((need_host & (cnt[:, 3] > 0)).sum())
        for _ in range(2 * int(too_many.sum())):                  # once for u, once for v (B:306, B:889-890)
            print(TOO_MANY_MSG)
        state = {"keep": keep, "need": np.flatnonzero(need_host), "host": host, "dev": keep_alive[0]}
        if state["need"].size:
            off = host["offsets"].numpy()                            # [2, n + 1]: ring / hole list starts per pair
            rc, uv, hc = host["ring_rc"].numpy(), host["ring_uv"].numpy(), host["hole_rc"].numpy()
            tot_r, tot_h = int(off[0, n]), int(off[1, n])
            if tot_r > rc.shape[0] or tot_h > hc.shape[0]:
                # heavily damaged fields: the lists are longer than the asynchronous copy carried -- fetch them whole
                ring_rc, ring_uv, hole_rc = keep_alive[1:4]
                rc, uv, hc = ring_rc[:tot_r].cpu().numpy(), ring_uv[:tot_r].cpu().numpy(), hole_rc[:tot_h].cpu().numpy()
            # (the lists list pair after pair, row-major inside a pair: np.argwhere's order, the reference's)
            jobs = [(rc[off[0, k]:off[0, k + 1]], uv[off[0, k]:off[0, k + 1]], hc[off[1, k]:off[1, k + 1]])
                    for k in state["need"]]
            state["holes"] = [j[2] for j in jobs]
            pool = self._fill_pool()
            if pool is not None:
                # (round 5: own worker processes behind pipes.  multiprocessing.Pool.map was synchronous here -- with map_async
                #  the pool's handler threads compete with this thread for the GIL and the whole host side got slower,
                #  6.5 k -> 4.8 k pairs/s -- and a batch of 64 pairs waited 2-4 ms for its triangulations)
                state["pending"] = (pool, pool.submit(jobs, owner=owner), owner)
            else:
                with blas_one_thread():
                    state["sols"] = qhull_fill_many(jobs)
        return state

    def _post_complete(self, state):
        """Second stage: the triangulation's values go -- flipped and scaled with the reference's expressions, cell by
        cell -- into the finished fields (and into the raw ones when they were asked for).  Returns the state with the
        per-pair keep flags (False: dropped)."""
        keep, need, host = state["keep"].copy(), state["need"], state["host"]
        if "pending" in state:
            pool, t_, owner = state.pop("pending")
            state["sols"] = pool.collect(t_, forget_older=True, owner=owner)      # (older tickets of this pipeline only)
        if need.size:
            st = self.stats
            fu, fv = host["fu"].numpy(), host["fv"].numpy()
            uk, vk = (host["u"].numpy(), host["v"].numpy()) if "u" in host else (None, None)
            nr = fu.shape[1]
            st["host_fallback"] += len(state["sols"])
            ii, cells_l, vals_l = [], [], []
            for k, vals_k in enumerate(state["sols"]):
                if vals_k is None:
                    st["dropped_by_qhull"] += 1
                    keep[int(need[k])] = False
                    continue
                cells = state["holes"][k]
                ii.append(np.full(cells.shape[0], int(need[k]), dtype=np.int64))
                cells_l.append(cells)
                vals_l.append(vals_k)
            if ii:
                # ONE indexed assignment per field for the whole batch (round 5; per pair before: 4-6 fancy-index stores each)
                ii = np.concatenate(ii)
                cells = np.concatenate(cells_l).astype(np.int64, copy=False)
                vals = np.concatenate(vals_l)
                rr, cc = cells[:, 0], cells[:, 1]
                if uk is not None:
                    uk[ii, rr, cc] = vals[:, 0]
                    vk[ii, rr, cc] = vals[:, 1]
                pu = vals[:, 0] * self._scale / self._dt * 1000          # the reference's expression, cell by cell (B:896-898)
                pv = -vals[:, 1] * self._scale / self._dt * 1000
                fr = nr - 1 - rr
                fu[ii, fr, cc] = pu
                fv[ii, fr, cc] = pv
                if self.device_out:
                    # the same patches into the device copies of the finished fields: ONE small upload + index_put per batch
                    dev = state["dev"]["fu"].device
                    idx = torch.from_numpy(np.stack([ii, fr, cc])).to(dev)
                    val = torch.from_numpy(np.stack([pu, pv])).to(dev)
                    state["dev"]["fu"][idx[0], idx[1], idx[2]] = val[0]
                    state["dev"]["fv"][idx[0], idx[1], idx[2]] = val[1]
        state["keep_final"] = keep
        return state

    def _post_collect(self, ticket):
        """Both host stages at once; per pair None (dropped) or the raw (u, v) before the flip / scaling (the ticket
        must come from _post_submit(..., want_raw=True))."""
        state = self._post_complete(self._post_extract(ticket))
        uk, vk = state["host"]["u"].numpy(), state["host"]["v"].numpy()
        return [(uk[i], vk[i]) if state["keep_final"][i] else None for i in range(uk.shape[0])]

    def _post_validate_batch(self, u, v, inv, plan=None, sigma=True):
        return self._post_collect(self._post_submit(u, v, inv, want_raw=True, plan=plan, sigma=sigma))

    def _post_pipeline(self, x, y, depth=1, plan=None):
        """The host side of batched() as a pipeline: push(meta, ticket) after every launch returns the finished
        entries [(meta, per-pair results)] of the batch pushed `depth` + 1 launches before -- while the GPU works on batch k,
        the census of batch k - depth is taken and its triangulations go to the worker processes; their answers are read,
        patched in and handed out one push later.  The file path uses
        depth 2: a batch's upload (longer than its passes) then overlaps the passes of the batch before instead of being
        waited for.  flush() drains."""
        waiting, extracted = [], []
        owner = PipelineOwner()          # this pipeline's name in the fill-worker pool (shared with every other generator)

        def step(drain=False):
            # the census of the next batch first: it waits for the GPU, and behind that wait its triangulations go to the
            # workers; then the batch before it, whose triangulations were handed out one step ago and have had that whole
            # step (the wait included) to finish, is patched and handed out
            out = []
            if waiting:
                meta, ticket = waiting.pop(0)
                extracted.append((meta, self._post_extract(ticket, owner) if ticket is not None else None))
            if extracted and (len(extracted) > 1 or (drain and not waiting)):
                meta, state = extracted.pop(0)
                out.append((meta, self._finish_batch(self._post_complete(state), x, y, plan) if state is not None else []))
            return out

        class Pipe:
            def push(_, meta, ticket):
                out = step() if len(waiting) >= depth else []
                waiting.append((meta, ticket))
                return out

            def flush(_):
                out = []
                while waiting or extracted:
                    out += step(drain=True)
                return out
        return Pipe()

    def _derived(self, U, V, skip, xs, ys, plan=None):
        """derive=: {name: field} of the finished fields U, V -- stacks [n, n_rows, n_cols] or one pair [n_rows, n_cols],
        device tensors (read in place; the results stay on the device) or numpy arrays (one upload of the two stacks, one
        copy down of all quantities).  skip: the excluded cells as delivered, a device tensor of the fields' shape or of
        one grid, bool or uint8, or None; every quantity is NaN there.  xs, ys: the delivered coordinates, whose steps
        scale the slopes (a grid of one column / row: the nominal step of the last pass)."""
        par = self._derive
        host = not isinstance(U, torch.Tensor)
        if host:
            UV = torch.from_numpy(np.stack([U, V])).to(self._device)
            U, V = UV[0], UV[1]
        one = U.dim() == 2
        if one:
            U, V = U[None], V[None]
        if skip is not None:
            skip = skip.to(torch.uint8).expand(U.shape[0], -1, -1).contiguous()
        if plan is not None:
            w, o = plan.geometry[-1][:2]
        else:
            w, o = options.pass_sizes(self._wind_size, self._overlap, self._iter, self._iter_scale)[-1]
        nominal = (w - o) * self._scale
        hx = float(xs[0, 1] - xs[0, 0]) if xs.shape[1] > 1 else nominal
        hy = float(ys[1, 0] - ys[0, 0]) if ys.shape[0] > 1 else nominal
        got = engine.derive(engine.field_fit(U, V, skip, par["radius"], par["order"]), hx, hy, par["quantities"])
        stack = torch.stack([got[k] for k in par["quantities"]])
        if skip is not None:
            stack.masked_fill_(skip.bool()[None], float("nan"))
        if one:
            stack = stack[:, 0]
        if host:
            stack = stack.cpu().numpy()
        return {k: stack[q] for q, k in enumerate(par["quantities"])}

    def _finish_batch(self, state, x, y, plan=None):
        """The finished tuples of a batch: the device has flipped and scaled the fields (_post_submit), the host stage has
        patched the filled cells (_post_complete); what is left is ONE copy of the two stacks out of the pinned staging
        memory (so that results a caller keeps do not pin pages) and the per-pair views.  Returns per pair None or
        (x, y, u, v), with uncertainty= followed by su, sv and with derive= closed by its dict; x, y are one pair of
        read-only arrays per batch (the reference makes fresh copies per pair; a caller that wants to write into them
        copies first)."""
        keep = state["keep_final"]
        if not keep.any():
            return [None] * keep.size
        if self.device_out:
            U, V = state["dev"]["fu"], state["dev"]["fv"]           # rows of the batch's device stacks (views)
        else:
            U, V = np.array(state["host"]["fu"].numpy()), np.array(state["host"]["fv"].numpy())
        if "excluded" in state["host"]:
            # dynamic_mask=: the fill value into every pair's own excluded cells, after flip and scale (the grids came
            # flipped; mask='s image is part of every pair's mask)
            if self.device_out:
                ex = state["dev"]["excluded"]
                U.masked_fill_(ex, self._dynmask["fill"])
                V.masked_fill_(ex, self._dynmask["fill"])
            else:
                ex = state["host"]["excluded"].numpy()
                U[ex] = self._dynmask["fill"]
                V[ex] = self._dynmask["fill"]
        elif self._mask is not None and plan is not None:
            # mask=: the fill value into the excluded cells of every pair, after flip and scale (the grid is flipped too)
            grid = self._fill_grid(plan)
            if self.device_out:
                U.masked_fill_(grid[1], self._mask["fill"])
                V.masked_fill_(grid[1], self._mask["fill"])
            else:
                U[:, grid[0]] = self._mask["fill"]
                V[:, grid[0]] = self._mask["fill"]
        xs, ys = x * self._scale, y * self._scale
        xs.flags.writeable = False
        ys.flags.writeable = False
        if self._derive is not None:
            # derive=: from the stacks as they are delivered, fills and fill values included; the excluded cells are read
            # from their device copies (dynamic_mask=: every pair's own grid; mask=: the one grid)
            skip = state["dev"].get("excluded")
            if skip is None and self._mask is not None and plan is not None:
                skip = self._fill_grid(plan)[1]
            D = self._derived(U, V, skip, xs, ys, plan)
            sig = ()
            if "fsu" in state["host"]:
                sig = (state["dev"]["fsu"], state["dev"]["fsv"]) if self.device_out else \
                    (np.array(state["host"]["fsu"].numpy()), np.array(state["host"]["fsv"].numpy()))
            return [(xs, ys, U[k], V[k]) + tuple(s_[k] for s_ in sig) + ({q: f[k] for q, f in D.items()},) if keep[k] else None
                    for k in range(keep.size)]
        if "fsu" in state["host"]:
            # uncertainty=: beside the fields, NaN in the excluded cells too (the kernel wrote them; no fill value)
            if self.device_out:
                SU, SV = state["dev"]["fsu"], state["dev"]["fsv"]
            else:
                SU, SV = np.array(state["host"]["fsu"].numpy()), np.array(state["host"]["fsv"].numpy())
            return [(xs, ys, U[k], V[k], SU[k], SV[k]) if keep[k] else None for k in range(keep.size)]
        return [(xs, ys, U[k], V[k]) if keep[k] else None for k in range(keep.size)]

    def _finish(self, uv, x, y, plan=None, sigma=None, excluded=None, derive=True):
        """Flip and unit scaling of B:894-898 (numpy, the reference's own expressions); then, with mask=, the fill value
        into the excluded cells of the plan's last pass.  sigma: the raw (su, sv) of uncertainty=, which take the flip and
        the scaling, no sign and no fill, and follow u, v in the tuple.  derive=: its dict closes the tuple."""
        if uv is None:
            return None
        if derive and self._derive is not None:
            out = self._finish(uv, x, y, plan=plan, sigma=sigma, excluded=excluded, derive=False)
            skip = None
            if excluded is not None:
                skip = torch.from_numpy(np.ascontiguousarray(excluded)).to(self._device)
            elif self._mask is not None and plan is not None:
                skip = self._fill_grid(plan)[1]
            return out + (self._derived(out[2], out[3], skip, out[0], out[1], plan),)
        if sigma is not None:
            su, sv = (np.flip(s_, axis=0) * self._scale / self._dt * 1000 for s_ in sigma)
            return self._finish(uv, x, y, plan=plan, excluded=excluded, derive=False) + (su, sv)
        u, v = uv
        u = np.flip(u, axis=0)
        v = -np.flip(v, axis=0)
        u = u * self._scale / self._dt * 1000
        v = v * self._scale / self._dt * 1000
        if excluded is not None:                        # dynamic_mask=: this pair's own grid (bool numpy, flipped)
            u[excluded] = self._dynmask["fill"]
            v[excluded] = self._dynmask["fill"]
        elif self._mask is not None and plan is not None:
            grid = self._fill_grid(plan)[0]
            u[grid] = self._mask["fill"]
            v[grid] = self._mask["fill"]
        return x * self._scale, y * self._scale, u, v

    # pairs per launch of __call__ (extension): the generator of the reference's API reads ahead and runs
    # `call_batch` pairs through batched(); the fields it yields, their order and the dropped pairs are those of
    # the one-pair-per-launch loop (call_batch = 1, the reference's B:868-901 literally)
    call_batch = 32

    def _one(self, i):
        """Pair i alone: decode on the host, one launch per pass, post-validation, flip / scale (B:868-898).
        None for an undecodable or dropped pair.  Plans of this path are kept per frame shape."""
        raw = self._load_pair(i)
        if raw is None:
            return None
        shape = (int(raw.A.shape[-2]), int(raw.A.shape[-1]))
        plan = self._single_plan(shape)
        # one launch per frame and step; in place from equalize on: the upload and what the steps made are this object's
        fa, fb, masks = self._prepared(raw)
        excluded = None
        if masks is not None:
            u, v, inv, excluded = self._run_masked(plan, fa, fb, masks)
            excluded = excluded[0].cpu().numpy()
        else:
            u, v, inv = plan.run(fa, fb)
        sigma = None if self._uncertainty is None else plan.uncertainty(1)
        w, o, _, _ = plan.geometry[-1]
        x, y = get_coordinates(shape, w, o)
        uv = self._post_validate_batch(u, v, inv, plan=plan, sigma=False)[0]     # (sigma: fetched above, finished on the host)
        if sigma is not None and uv is not None:
            sigma = tuple(s_[0].cpu().numpy() for s_ in sigma)
        return self._finish(uv, x, y, plan=plan, sigma=sigma, excluded=excluded)

    def __call__(self) -> Generator:
        if int(self.call_batch) > 1 and len(self._dataset) > 1:
            # the reference hands out FRESH x, y per pair (B:899-900: x * scale makes a new array), which a caller may
            # write into; batched() shares one read-only pair of coordinate arrays per batch, so copy here
            for out in self.batched(int(self.call_batch)):      # (i, x, y, u, v), with uncertainty= also su, sv
                yield (out[1].copy(), out[2].copy()) + out[3:]
            return
        end_time = time()
        for i in range(len(self._dataset)):
            if self.verbose:
                print(f"Load time {(time() - end_time):.3f} sec", end=" ")
            start = time()
            out = self._one(i)
            if out is None:
                continue
            yield out
            end_time = time()
            if self.verbose:
                print(f"Batch finished in {(end_time - start):.3f} sec")

    def batched(self, batch_size: int = 32, indices=None) -> Generator:
        """Like __call__, but reads, uploads and processes `batch_size` pairs per launch.  Native reader
        threads (io.ReadAhead) put the next batches' files into pinned staging memory -- uncompressed BMPs as their RAW
        FILE BYTES (no host decode: header skip, row flip, padding strip and palette / gray conversion
        run on the device, tpiv_bmp_unpack), other formats decoded on the host -- while the GPU works on
        the current batch (triple-buffered staging, uploads on their own stream: _raw_batches).  Yields (pair_index, x, y, u, v); dropped pairs yield nothing."""
        idx = list(range(len(self._dataset))) if indices is None else list(indices)
        first = self._first_decodable(idx) if idx else None       # the frame shape is the first decodable pair's
        if first is None:
            return
        H, W = first[1]
        plan = self._get_plan(H, W, max_batch=batch_size)
        w, o, _, _ = plan.geometry[-1]
        x, y = get_coordinates((H, W), w, o)
        dev = self._device
        pipe = self._post_pipeline(x, y, depth=self._in_flight(), plan=plan)

        def emit(finished):
            """Results of finished batches in dataset order; the pairs that were not staged run now."""
            for order, res in finished:
                res = iter(res)
                for i, staged in order:
                    out = next(res) if staged else self._one(i)
                    if out is not None:
                        if self.device_out and not staged:      # the one-pair path finishes on the host
                            def up(f):
                                return torch.from_numpy(np.ascontiguousarray(f)).to(dev)
                            out = out[:2] + tuple({k: up(q) for k, q in f.items()} if isinstance(f, dict) else up(f)
                                                  for f in out[2:])
                        yield (i,) + out

        with contextlib.closing(self._frame_batches(idx, batch_size, H, W, first[0])) as batches:
            for raw, fa, fb, masks in batches:
                # (a pair that is not staged -- undecodable, or a frame shape other than the batch's -- takes the one-pair
                #  path when its turn comes, in emit: that skips an undecodable pair like B:138-139 and gives another
                #  shape its own plan)
                ticket = None
                if masks is not None:
                    u, v, inv, excluded = self._run_masked(plan, fa, fb, masks)
                    ticket = self._post_submit(u, v, inv, plan=plan, excluded=excluded)
                elif fa is not None:
                    u, v, inv = plan.run(fa, fb)
                    ticket = self._post_submit(u, v, inv, plan=plan)
                # the host work of the PREVIOUS batches runs while the GPU works on this one
                yield from emit(pipe.push(raw.order, ticket))
                if raw.last:
                    # drained while the source is open: asking it for more ends the run (over files: reader threads
                    # stopped, device synchronised), which the batches in flight need not wait for
                    yield from emit(pipe.flush())
            yield from emit(pipe.flush())         # (nothing left, unless the source ended early: its reader was closed under it)


class ResidentPIV(OfflinePIV):
    """OfflinePIV over frame pairs that already live on the GPU (uint8 tensors [n, H, W]): the same
    passes, post-validation, flip and scaling, without dataset / decoding / upload.  Extension used by
    the end-to-end benchmark and by callers that acquire straight into device memory."""

    def __init__(self, frames_a: torch.Tensor, frames_b: torch.Tensor, wind_size: int, overlap: int,
                 multipass: int = 1, multipass_mode: str = "CWS", dt: int = 1, scale: float = 1.,
                 multipass_scale: float = 2., precision: str = "exact", validation_ratio: float = 1.2,
                 validation_window: int = 3, background=None, outlier=None, depth=None, mask=None,
                 dewarp=None, uncertainty=None, derive=None, deform=None, correlation=None, weighting=None,
                 dynamic_mask=None, equalize=None, prefilter=None) -> None:
        # dewarp (see OfflinePIV): every launch rectifies its pairs into a reused buffer, addressed by their offsets in the
        # caller's stacks (nothing is gathered first, and the caller's frames are never written)
        # depth (see OfflinePIV): the frames are uint16 stacks if and only if it is given; they stay as they are and every
        # launch maps its pairs into a reused uint8 buffer
        depth = engine.depth_arg(depth)
        dtypes = (frames_a.dtype, frames_b.dtype)
        if depth is None and dtypes == (torch.uint16, torch.uint16):
            raise ValueError("ResidentPIV: uint16 frames need depth= (e.g. depth='auto' or {'lo': 0, 'hi': 4095}) to say how "
                             "they map to 8 bits")
        if depth is not None and dtypes == (torch.uint8, torch.uint8):
            raise ValueError("ResidentPIV: depth= goes with uint16 frames; leave it out for uint8 frames")
        want = torch.uint8 if depth is None else torch.uint16
        if frames_a.shape != frames_b.shape or frames_a.dim() != 3 or dtypes != (want, want):
            raise ValueError("ResidentPIV: two uint8 tensors [n, H, W] of one shape" if depth is None else
                             "ResidentPIV: with depth=, two uint16 tensors [n, H, W] of one shape")
        if precision not in PRECISIONS:
            raise KeyError(precision)
        run = dict(wind_size=wind_size, overlap=overlap, multipass=multipass, multipass_mode=multipass_mode, dt=dt,
                   scale=scale, multipass_scale=multipass_scale, precision=precision, validation_ratio=validation_ratio,
                   validation_window=validation_window)
        opts = options.parse_options(run, frames_a.shape, background=background, outlier=outlier, prefilter=prefilter,
                                     depth=depth, equalize=equalize, mask=mask, dewarp=dewarp, uncertainty=uncertainty,
                                     derive=derive, deform=deform, correlation=correlation, weighting=weighting,
                                     dynamic_mask=dynamic_mask)
        device = _require_gpu(frames_a.device)
        self._init_state(device, range(frames_a.shape[0]), IterModMap.functions[multipass_mode], run, opts)
        self._A, self._B = frames_a.contiguous(), frames_b.contiguous()

    def _first_decodable(self, idx):
        return (idx[0], tuple(int(s_) for s_ in self._A.shape[1:])) if len(idx) else None

    def _depth_pairs(self, sample):
        for i in engine.depth_sample(len(self), sample):
            yield self._A[int(i)], self._B[int(i)]

    def _mapped(self, frames, chunk, lut, out=None):
        """The pairs `chunk` of a resident uint16 stack through the tone map: uint8 [len(chunk), H, W], one launch that
        addresses the frames by their offsets (nothing is gathered first)."""
        H, W = frames.shape[1:]
        off = torch.tensor(chunk, dtype=torch.int64) * (H * W)
        return engine.depth_map(frames.view(-1), lut, offsets=off, shape=(H, W), out=out)

    def _select(self, chunk, lut, out=None, dw=None):
        """(A, B, owned): the uint8 frames of the pairs `chunk` and whether they are memory of this object.  Under depth=
        (lut) they are mapped, the pairs addressed by offset (consecutive or not: no gather), into out[0] and out[1]
        (None: fresh tensors): owned.  Under dewarp= they are then rectified into dw[0] and dw[1] (the rectified-frame
        buffer, [2, >= n, H, W]) -- the mapped frames, or without depth= the caller's own, addressed by offset like the tone
        map's: owned.  A run of consecutive pairs is a view of the caller's frames: not owned.  Anything
        else is gathered (a copy of 2 x 4 MB per pair: 0.36 ms per 64 pairs at 4 MP -- the check is per chunk, so a stream
        that repeats or skips stays copy-free per run): owned."""
        n = len(chunk)
        if lut is not None:
            out_a, out_b = (None, None) if out is None else (out[0], out[1])
            A, B = self._mapped(self._A, chunk, lut, out=out_a), self._mapped(self._B, chunk, lut, out=out_b)
            if dw is not None:
                A, B = self._dewarped(A, dw[0, :n]), self._dewarped(B, dw[1, :n])
            return A, B, True
        if dw is not None:
            H, W = self._A.shape[1:]
            off = torch.tensor(chunk, dtype=torch.int64) * (H * W)
            return (self._dewarped(self._A.view(-1), dw[0, :n], offsets=off, shape=(H, W)),
                    self._dewarped(self._B.view(-1), dw[1, :n], offsets=off, shape=(H, W)), True)
        if chunk[-1] - chunk[0] == n - 1 and chunk == list(range(chunk[0], chunk[0] + n)):
            return self._A[chunk[0]:chunk[0] + n], self._B[chunk[0]:chunk[0] + n], False
        sel = torch.tensor(chunk, dtype=torch.int64, device=self._device)
        return self._A.index_select(0, sel), self._B.index_select(0, sel), True

    def _load_pair(self, i):
        H, W = self._A.shape[1:]
        dw = None if self._dewarp is None else self._scratch("_dw_frames", (2, 1), H, W, self._A.device)
        A, B, owned = self._select([i], self._depth_table(), dw=dw)
        bg = self._background((H, W))
        bg_a, bg_b = (None, None) if bg is None else (bg[0], bg[1])
        return Raw([(i, True)], [i], A, B, owned, bg_a, bg_b)

    def compute_background(self, indices=None, batch_size=None):
        """(bg_a, bg_b): the per-pixel minimum of the resident a frames and of the b frames (of the pairs `indices`;
        None: all), uint8 [H, W] on the device (tpiv_frame_min; 255 everywhere for no pair).  batch_size: pairs mapped,
        rectified or gathered at a time (default bg_batch).  With depth= the minimum is taken over the tone-mapped
        frames, with dewarp= over the rectified frames, batch_size pairs at a time."""
        lut = self._depth_table()
        if len(self) and (lut is not None or self._dewarp is not None or indices is not None):
            return super().compute_background(indices, batch_size)
        acc = torch.full((2,) + tuple(self._A.shape[1:]), 255, dtype=torch.uint8, device=self._device)
        if len(self):                                        # the resident stacks as they are: one launch each
            engine.frame_min(self._A, acc[0])
            engine.frame_min(self._B, acc[1])
        return acc[0], acc[1]

    # launches in flight before a batch's census is read.  Two: the copies of a batch's results run on a stream of their own,
    # as kernels (rocprofv3 shows __amd_rocclr_copyBuffer), and the passes of the NEXT batch leave them no registers on any CU
    # until they end -- with one launch in flight the host got a batch's census when the GPU had just run dry (round 5: GPU
    # timeline of the 'isolated spots' case, 0.8 ms idle per 64 pairs)
    resident_depth = 2

    def _in_flight(self):
        return self.resident_depth

    def _raw_batches(self, idx, batch_size, H, W, bg, like=None):
        """The raw frame source over the resident stacks: one Raw record per batch_size pairs of idx, every pair staged --
        _select's frames, mapped and rectified into reused buffers (stream order keeps a launch's passes ahead of the next
        launch's writes into the same memory).  bg [2, H, W] is all left to the consumer."""
        lut = self._depth_table()                     # (depth="auto": the histogram of the sampled pairs, once)
        lead = (2, min(batch_size, len(idx)))         # (no larger than the run needs)
        dbuf = None if lut is None else self._scratch("_depth_frames", lead, H, W, self._A.device)
        dw = None if self._dewarp is None else self._scratch("_dw_frames", lead, H, W, self._A.device)
        bg_a, bg_b = (None, None) if bg is None else (bg[0], bg[1])
        for s in range(0, len(idx), batch_size):
            chunk = idx[s:s + batch_size]
            n = len(chunk)
            A, B, owned = self._select(chunk, lut, out=None if dbuf is None else (dbuf[0, :n], dbuf[1, :n]), dw=dw)
            yield Raw([(i, True) for i in chunk], chunk, A, B, owned, bg_a, bg_b, s + batch_size >= len(idx))

    def _prep_out(self, raw, batch_size, H, W):
        """The background and the filter write a reused buffer, and so does the first later step that meets the caller's
        frames (the tone map and the rectification have buffers of their own that equalize and mask go on in); None where
        every step goes in place."""
        if raw.bg_a is not None or self._prefilter is not None \
                or ((self._equalize is not None or self._zeroes_pixels()) and self._depth is None and self._dewarp is None):
            return self._scratch("_bg_frames", (2, batch_size), H, W, raw.A.device)[:, :len(raw.chunk)]
        return None

    def __call__(self) -> Generator:
        for out in self.batched(1):
            yield (out[1].copy(), out[2].copy()) + out[3:]


class OnlinePIV:
    """The reference's live-acquisition class is a constructor-only stub (B:906-927: it stores its arguments
    and resolves the device; there is no processing method).  Mirrored as such -- frames acquired straight
    into GPU memory go through ResidentPIV."""

    def __init__(self, folder: str, device: str, file_fmt: str, wind_size: int, overlap: int, iterations: int = 1,
                 dt: int = 1, scale: float = 1., resize: int = 2, iter_scale: float = 2.) -> None:
        self._wind_size = wind_size
        self._overlap = overlap
        self._dt = dt
        self._iter = iterations
        self._iter_scale = iter_scale
        self._resize = resize
        self._scale = scale
        self._device = DeviceMap.devicies[device]           # KeyError like B:927


class StereoPIV:
    """Stereoscopic PIV: two cameras that look at the light sheet z = 0 from different sides, run in lockstep, and the
    three components (U, V, W) of every vector from their two in-plane fields (engine.stereo_reconstruct,
    tpiv_stereo_reconstruct).

        piv = StereoPIV(cam1=(a1, b1), cam2=(a2, b2), P=(P1, P2), wind_size=32, overlap=16, scale=0.1, origin=(X0, Y0))
        for i, x, y, U, V, W, res in piv.batched(): ...

    cam1, cam2: the frames a and b of each camera, uint8 tensors [n, H, W] on the GPU (ResidentPIV's); from_folders()
    takes two folders instead (OfflinePIV's).  P = (P1, P2): the cameras, float64 [3, 4] each, (x_cam, y_cam, 1) ~ P (X, Y,
    Z, 1) in camera pixels -- engine.stereo_fit makes one from a calibration target.  scale: mm per pixel of the rectified
    frames, origin = (X0, Y0): the world position of their pixel (0, 0); pixel (x, y) is the world point (X0 + scale x, Y0 -
    scale y, 0).  World frame: right-handed, mm, X to the right, Y up, Z towards the cameras.

    Both cameras are rectified onto the sheet with dewarp={"homography": engine.stereo_homography(P_c, scale, origin),
    "interp": interp, "fill": dewarp_fill} and get the same mask=: the caller's image, if any, OR-ed with the pixels that
    either camera does not see (dewarp_outside() of both), with the caller's threshold / pixels / fill.  Both then exclude
    the same cells; those carry `fill` in U, V, W.  Every other run parameter and keyword goes to both objects unchanged;
    uncertainty= adds sU, sV, sW to what is yielded.  Refused (ValueError, before any GPU call): dewarp=, dynamic_mask=
    (per-camera masks), derive= (two-component derivatives of a three-component field), cameras of different frame shapes
    or pair counts, a scale that is not finite and positive, a P that is not a finite [3, 4] matrix or whose centre does
    not lie in front of the sheet (C_z > 0).

    A pair is delivered when BOTH cameras deliver it: each camera drops pairs by the reference's rules, unchanged (stats
    counts them).  U, V, W are in the unit of the cameras' u, v (scale / dt * 1000), res is the root of the summed squared
    residuals of the four equations in that unit -- a measure of how well the two views agree, dominated by calibration
    and registration errors when it is large everywhere."""

    device_out = False       # True: U, V, W, res (and the sigmas) are yielded as tensors on the device

    _REFUSED = ("dewarp", "dynamic_mask", "derive")

    def __init__(self, cam1, cam2, P, wind_size: int, overlap: int, *, scale: float, origin=(0.0, 0.0), interp="cubic",
                 dewarp_fill=0, mask=None, **keywords) -> None:
        try:
            (a1, b1), (a2, b2) = cam1, cam2
        except (TypeError, ValueError):
            raise ValueError("StereoPIV: cam1 and cam2 are the pairs (frames_a, frames_b) of the two cameras") from None
        frames = (a1, b1, a2, b2)
        if any(not isinstance(t, torch.Tensor) or t.dim() != 3 for t in frames):
            raise ValueError("StereoPIV: every camera takes two tensors [n, H, W]")
        if tuple(a1.shape[1:]) != tuple(a2.shape[1:]):
            raise ValueError(f"StereoPIV: the cameras' frame shapes differ, {tuple(a1.shape[1:])} and {tuple(a2.shape[1:])}")
        if a1.shape[0] != a2.shape[0]:
            raise ValueError(f"StereoPIV: the cameras' pair counts differ, {a1.shape[0]} and {a2.shape[0]}")
        shape = (int(a1.shape[1]), int(a1.shape[2]))
        self._resident = True
        # what self_calibrate() needs to build the same object over the same frames with other cameras
        self._made_from = dict(cam1=(a1, b1), cam2=(a2, b2), wind_size=wind_size, overlap=overlap, scale=scale, origin=origin,
                               interp=interp, dewarp_fill=dewarp_fill, mask=mask, **keywords)
        self._build(P, shape)

    def _build(self, P, shape):
        """The two per-camera objects and everything derived from the cameras P, for the resident frames of this object."""
        m = dict(self._made_from)
        (a1, b1), (a2, b2) = m.pop("cam1"), m.pop("cam2")
        wind_size, overlap, scale, origin = m.pop("wind_size"), m.pop("overlap"), m.pop("scale"), m.pop("origin")
        dw, mask = self._geometry(P, scale, origin, m.pop("interp"), m.pop("dewarp_fill"), m.pop("mask"), m, shape)
        self._frames_a = (a1, a2)
        self._cams = tuple(ResidentPIV(a, b, wind_size, overlap, scale=scale, mask=mask, dewarp=dw[c], **m)
                           for c, (a, b) in enumerate(((a1, b1), (a2, b2))))
        self._after()

    @classmethod
    def from_folders(cls, folder1: str, folder2: str, device: str, file_fmt: str, P, wind_size: int, overlap: int, *,
                     scale: float, origin=(0.0, 0.0), interp="cubic", dewarp_fill=0, mask=None, **keywords):
        """The same over two folders of image files, one per camera (OfflinePIV's folder, device, file_fmt, folder_mode)."""
        self = cls.__new__(cls)
        cls._check(P, scale, origin, keywords)
        # the frame shapes and pair counts, from objects that read the folders and touch nothing else
        probe = [OfflinePIV(f, device, file_fmt, wind_size, overlap, scale=scale, **keywords) for f in (folder1, folder2)]
        shapes, counts = [p.frame_shape() for p in probe], [len(p) for p in probe]
        for p in probe:
            p.close()
        if counts[0] != counts[1]:
            raise ValueError(f"StereoPIV: the cameras' pair counts differ, {counts[0]} and {counts[1]}")
        if shapes[0] is None or shapes[1] is None:
            raise ValueError("StereoPIV: a folder without a decodable pair")
        if tuple(shapes[0]) != tuple(shapes[1]):
            raise ValueError(f"StereoPIV: the cameras' frame shapes differ, {tuple(shapes[0])} and {tuple(shapes[1])}")
        shape = (int(shapes[0][0]), int(shapes[0][1]))
        dw, mask = self._geometry(P, scale, origin, interp, dewarp_fill, mask, keywords, shape)
        self._resident = False
        self._frames_a = None
        self._cams = tuple(OfflinePIV(f, device, file_fmt, wind_size, overlap, scale=scale, mask=mask, dewarp=dw[c], **keywords)
                           for c, f in enumerate((folder1, folder2)))
        self._after()
        return self

    @classmethod
    def _check(cls, P, scale, origin, keywords):
        """The refusals that need no frame: keywords, scale, origin, cameras.  Returns the cameras."""
        for k in cls._REFUSED:
            if keywords.get(k) is not None:
                raise ValueError(f"StereoPIV: {k}= does not combine with a stereo run" + {
                    "dewarp": " (the rectification is the cameras' own: stereo_homography)",
                    "dynamic_mask": " (both cameras must exclude the same cells)",
                    "derive": " (its derivatives are those of a two-component field)"}[k])
        engine.stereo_homography(np.eye(3, 4), scale, origin)           # (scale and origin, checked where they are used)
        try:
            P1, P2 = P
        except (TypeError, ValueError):
            raise ValueError("StereoPIV: P = (P1, P2), one float64 [3, 4] matrix per camera") from None
        cams = []
        for c, Pc in enumerate((P1, P2)):
            try:
                engine.stereo_tangents(Pc, 0.0, 0.0)                     # finite [3, 4], C_z > 0
            except ValueError as e:
                raise ValueError(f"StereoPIV: camera {c + 1}: {e}") from None
            cams.append(np.array(Pc, dtype=np.float64))
        return tuple(cams)

    def _geometry(self, P, scale, origin, interp, dewarp_fill, mask, keywords, shape):
        """Checks; then the two dewarp= dicts and the one mask= dict of the cameras, for frames of `shape`."""
        self._P = self._check(P, scale, origin, keywords)
        self._scale, self._origin, self._shape = float(scale), (float(origin[0]), float(origin[1])), shape
        dw = tuple(engine.dewarp_arg({"homography": engine.stereo_homography(Pc, scale, origin), "interp": interp,
                                      "fill": dewarp_fill}) for Pc in self._P)
        par = engine.mask_arg(mask)
        unseen = np.zeros(shape, dtype=bool)
        for d in dw:
            unseen |= engine.dewarp_outside(engine.dewarp_map(d, shape[0], shape[1]))
        if par is not None:
            image = par["image"].cpu().numpy()
            if image.shape != shape:
                raise ValueError(f"mask: image of shape {image.shape} for frames of shape {shape}")
            unseen |= image != 0
        par = dict(par or {}, image=unseen)
        self._fill = float(par.get("fill", engine.MASK_DEFAULTS["fill"]))
        self._unseen = unseen
        return dw, par

    def _after(self):
        for cam in self._cams:
            cam.device_out = True
        self._uncertainty = self._cams[0]._uncertainty is not None
        self._planes = None
        self._skip = None
        self.reset_stats()

    def __len__(self) -> int:
        return len(self._cams[0])

    def reset_stats(self):
        """stats: pairs delivered, pairs dropped by camera 1 only / camera 2 only / both (undecodable ones included), and
        pair_rms: {pair index: the rms of res over the pair's reconstructed cells}."""
        self._counts = {"delivered": 0, "dropped_camera1_only": 0, "dropped_camera2_only": 0, "dropped_both": 0}
        self._rms = []               # (pair indices, device tensor) per batch, read when stats is

    @property
    def stats(self):
        rms = {}
        for ids, t in self._rms:
            rms.update(zip(ids, t.cpu().numpy().tolist()))
        return dict(self._counts, pair_rms=rms)

    def cameras(self):
        """The two per-camera objects (ResidentPIV / OfflinePIV), for their own stats, mask_grid() and dewarp_outside()."""
        return self._cams

    def _last_pass(self):
        plan = self._cams[0]._single_plan(self._shape)
        w, o, _, _ = plan.geometry[-1]
        return get_coordinates(self._shape, w, o)

    def planes(self):
        """((a1, b1), (a2, b2)): the tangent planes of the two cameras at the cells of the delivered fields, float64 numpy
        [n_rows, n_cols] (engine.stereo_planes at the window centres of the last pass)."""
        if self._planes is None:
            x, y = self._last_pass()
            self._planes = tuple(engine.stereo_planes(Pc, x, y, self._scale, self._origin) for Pc in self._P)
        return self._planes

    def _device_geometry(self):
        """The tangent planes and the excluded cells on the device, made once."""
        if self._skip is None:
            dev = self._cams[0]._device
            grid = self._cams[0].mask_grid()
            planes = [torch.from_numpy(q).to(dev) for cam in self.planes() for q in cam]
            self._skip = (planes, torch.from_numpy(np.ascontiguousarray(grid).view(np.uint8)).to(dev))
        return self._skip

    def batched(self, batch_size: int = 32, indices=None) -> Generator:
        """Runs both cameras' batched() over the same pairs and joins what they deliver on the pair index; the stacks of one
        batch go through ONE engine.stereo_reconstruct call.  Yields (i, x, y, U, V, W, res), with uncertainty= followed by
        sU, sV, sW: x, y as the classes deliver them, the fields float64 [n_rows, n_cols] -- numpy arrays, or tensors on
        the device with device_out.  A pair that either camera drops or cannot decode yields nothing."""
        idx = list(range(len(self))) if indices is None else list(indices)
        if not idx:
            return
        batch_size = int(batch_size)
        (a1, b1, a2, b2), skip = self._device_geometry()

        def stream(cam):
            """(position in idx, tuple) of what the camera delivers, in its order (idx's)."""
            pos = -1
            for out in cam.batched(batch_size, idx):
                pos += 1
                while idx[pos] != out[0]:
                    pos += 1
                yield pos, out
        streams = [stream(cam) for cam in self._cams]
        got = [{}, {}]
        ahead = [None, None]

        def pull(c, hi):
            """Everything camera c delivers below position hi into got[c]; the first tuple past it waits in ahead[c]."""
            while True:
                if ahead[c] is None:
                    ahead[c] = next(streams[c], None)
                    if ahead[c] is None:
                        return
                if ahead[c][0] >= hi:
                    return
                got[c][ahead[c][0]] = ahead[c][1]
                ahead[c] = None

        try:
            for lo in range(0, len(idx), batch_size):
                hi = min(lo + batch_size, len(idx))
                pull(0, hi)
                pull(1, hi)
                both = [p for p in range(lo, hi) if p in got[0] and p in got[1]]
                n1 = sum(1 for p in range(lo, hi) if p in got[0])
                n2 = sum(1 for p in range(lo, hi) if p in got[1])
                st = self._counts
                st["delivered"] += len(both)
                st["dropped_camera1_only"] += n2 - len(both)
                st["dropped_camera2_only"] += n1 - len(both)
                st["dropped_both"] += (hi - lo) - n1 - n2 + len(both)
                if both:
                    one = [got[0][p] for p in both]
                    two = [got[1][p] for p in both]
                    x, y = one[0][1], one[0][2]
                    fields = [torch.stack([t[k] for t in cam]) for cam in (one, two) for k in (3, 4)]
                    sigma = None
                    if self._uncertainty:
                        sigma = [torch.stack([t[k] for t in cam]) for cam in (one, two) for k in (5, 6)]
                    rec = engine.stereo_reconstruct(*fields, a1, b1, a2, b2, sigma=sigma, skip=skip, fill=self._fill)
                    self._rms.append(([idx[p] for p in both], rec.pair_rms))
                    out = [rec.U, rec.V, rec.W, rec.res] + ([rec.sU, rec.sV, rec.sW] if self._uncertainty else [])
                    if not self.device_out:
                        out = [t.cpu().numpy() for t in out]
                    for k, p in enumerate(both):
                        yield (idx[p], x, y) + tuple(t[k] for t in out)
                for c in (0, 1):
                    for p in range(lo, hi):
                        got[c].pop(p, None)
        finally:
            for s in streams:
                s.close()

    def __call__(self) -> Generator:
        for out in self.batched():
            yield (out[1].copy(), out[2].copy()) + out[3:]

    def projections(self):
        """(P1, P2): copies of the cameras this object works with -- the constructor's, or the corrected ones after
        self_calibrate()."""
        return tuple(Pc.copy() for Pc in self._P)

    def disparity(self, indices=None, batch_size: int = 32, *, wind_size=None, overlap=None, multipass=None):
        """Whether the sheet lies where the calibration target stood: the displacement between what the two cameras see AT
        THE SAME INSTANT.  Frame a of camera 1 and frame a of camera 2 of the pairs `indices` (None: all) are rectified,
        each through its own map (engine.dewarp), and correlated as one ensemble -- ResidentPIV(rect1, rect2, ...).ensemble()
        with this object's window sizes, passes and mask, dt = 1.  Returns (x, y, dx, dy) in millimetres, dx along X, dy
        along Y (up), laid out like the delivered fields; None where ensemble() returns None.

        The sign: camera c's rectification puts a particle at (X, Y, z0) where its line of sight meets z = 0, at (X + a_c
        z0, Y + b_c z0) to first order -- the viewing tangents' own definition with dZ = z0.  Camera 2's position minus camera
        1's is what the correlation of rect1 with rect2 measures: a sheet at z = z0 instead of 0 shows as dx = (a2 - a1) z0
        and dy = (b2 - b1) z0; a sheet that is tilted shows a z0 that varies across the field.  The peak is as wide as the
        sheet is thick, (a2 - a1) times the thickness.  This only measures; self_calibrate() corrects the cameras from it.
        wind_size, overlap, multipass: the grid of this measurement, None: the object's own -- a sheet offset is often
        several times the flow's displacement and wants larger windows; the returned x, y describe the grid used.  Resident
        frames only (NotImplementedError for from_folders objects and with depth=); window sizes 16, 32, 64 (ensemble()'s)."""
        got = self._measure(indices, batch_size, wind_size, overlap, multipass, "disparity")
        return None if got is None else got[:4]

    @staticmethod
    def _grid_arg(who, wind_size, overlap, multipass):
        for name, v, low in (("wind_size", wind_size, 1), ("overlap", overlap, 0), ("multipass", multipass, 1)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < low):
                raise ValueError(f"StereoPIV.{who}: {name} must be an integer >= {low} or None, got {v!r}")

    def _measure(self, indices, batch_size, wind_size, overlap, multipass, who):
        """disparity()'s (x, y, dx, dy) followed by the excluded cells of the grid it used (bool, as delivered) and that
        grid's window centres in pixels (get_coordinates: x, y above are scaled as the classes deliver them)."""
        self._grid_arg(who, wind_size, overlap, multipass)
        if not self._resident:
            raise NotImplementedError(f"StereoPIV.{who}: resident frames only (build the object from tensors)")
        one = self._cams[0]
        if one._depth is not None:
            raise NotImplementedError(f"StereoPIV.{who}: 8-bit frames only")
        idx = list(range(len(self))) if indices is None else list(indices)
        if not idx:
            return None
        ws = one._wind_size if wind_size is None else int(wind_size)
        ov = one._overlap if overlap is None else int(overlap)
        n_pass = one._iter if multipass is None else int(multipass)
        H, W = self._shape
        batch_size = int(batch_size)
        rect = []
        for cam, frames in zip(self._cams, self._frames_a):
            frames = frames.contiguous()
            m = cam._dewarp_map((H, W), frames.device)
            out = torch.empty(len(idx), H, W, dtype=torch.uint8, device=frames.device)
            for s in range(0, len(idx), batch_size):
                chunk = idx[s:s + batch_size]
                off = torch.tensor(chunk, dtype=torch.int64) * (H * W)
                engine.dewarp(frames.view(-1), m, cam._dewarp["interp"], cam._dewarp["fill"], offsets=off, shape=(H, W),
                              out=out[s:s + len(chunk)])
            rect.append(out)
        piv = ResidentPIV(rect[0], rect[1], ws, ov, multipass=n_pass, multipass_mode=one._mode,
                          dt=1, scale=self._scale, multipass_scale=one._iter_scale, precision=one._precision,
                          validation_ratio=one._val_ratio, validation_window=one._val_win, outlier=one._outlier,
                          mask=one._mask)
        try:
            got = piv.ensemble(batch_size=batch_size)
            grid = None if got is None else piv.mask_grid()
        finally:
            piv.close()
        if got is None:
            return None
        x, y, u, v = got[:4]
        w, o = engine.pass_sizes(ws, ov, n_pass, one._iter_scale)[-1]
        # scale / dt * 1000 with dt = 1: micrometres -> millimetres
        return x, y, u / 1000.0, v / 1000.0, grid, get_coordinates((H, W), w, o)

    def self_calibrate(self, indices=None, batch_size: int = 32, *, iterations: int = 4, tol=None, trim: float = 3.0,
                       gap_max=None, min_cells=None, apply: bool = True, wind_size=None, overlap=None, multipass=None):
        """Corrects both cameras from the disparity map (Wieneke 2005): the light sheet never lies exactly where the
        calibration target stood.  Every round (at most `iterations`):
          1. disparity() of the pairs `indices` with the current cameras, on the grid wind_size / overlap / multipass (None:
             the object's own), its excluded cells skipped;
          2. every cell's disparity triangulated between the two cameras' lines of sight (engine.stereo_triangulate: the
             disparity belongs to the MIDPOINT of the two rectified positions) and a least-squares plane Z = c0 + c1 X + c2 Y
             through the points (engine.stereo_plane); then, at most twice more and until the count stops changing, cells
             further than trim x the rms residual from the plane are left out and the plane is fitted again; cells whose
             lines of sight pass further than gap_max mm from each other (None: no test) are left out from the start;
          3. both cameras expressed in the frame of that plane (engine.stereo_correct): the sheet becomes z = 0.
        The run stops with the round whose measured plane stays within tol mm of z = 0 at every non-excluded cell, max |c0 +
        c1 X + c2 Y| <= tol; that round's correction is still applied.  tol = None: 0.05 x scale, a twentieth of a pixel of
        sheet height -- about what the disparity pass resolves; a convention, not a measured bound.  RuntimeError when fewer
        than min_cells cells survive a round (None: a quarter of the non-excluded cells, at least 3).
        Returns {"P": (P1, P2) corrected, "T": [4, 4] taking the corrected world frame to the constructor's (the product of
        the rounds' transforms), "rounds": [{"plane": (c0, c1, c2), "rms", "count", "height", "gap": the median distance of
        the lines of sight, "d": the median |disparity|, all in mm}], "converged"}.  apply=True: the object continues with
        the corrected cameras over the same resident frames -- homographies, unseen-pixel mask, tangent planes and skip grid
        are made anew as the constructor makes them, stats is reset; apply=False: the object is left as it was.  Resident
        8-bit frames only (NotImplementedError for from_folders objects and with depth=, before any GPU call)."""
        who = "self_calibrate"
        self._grid_arg(who, wind_size, overlap, multipass)
        if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 1:
            raise ValueError(f"StereoPIV.{who}: iterations must be an integer >= 1, got {iterations!r}")
        if not engine.is_real(trim) or not np.isfinite(trim) or not trim > 0:
            raise ValueError(f"StereoPIV.{who}: trim must be a finite number > 0, got {trim!r}")
        for name, v in (("tol", tol), ("gap_max", gap_max)):
            if v is not None and (not engine.is_real(v) or not np.isfinite(v) or v < 0):
                raise ValueError(f"StereoPIV.{who}: {name} must be a finite number >= 0 or None, got {v!r}")
        if min_cells is not None and (isinstance(min_cells, bool) or not isinstance(min_cells, (int, np.integer)) or min_cells < 3):
            raise ValueError(f"StereoPIV.{who}: min_cells must be an integer >= 3 or None, got {min_cells!r}")
        if not self._resident:
            raise NotImplementedError(f"StereoPIV.{who}: resident frames only (build the object from tensors)")
        if self._cams[0]._depth is not None:
            raise NotImplementedError(f"StereoPIV.{who}: 8-bit frames only")
        tol = 0.05 * self._scale if tol is None else float(tol)
        gap_max = float("inf") if gap_max is None else float(gap_max)
        dev = self._cams[0]._device
        P, T, rounds, converged = self.projections(), np.eye(4), [], False
        for k in range(int(iterations)):
            # round 1 measures with this object; a later round with one built from the same frames and the corrected cameras
            piv = self if k == 0 else StereoPIV(**self._made_from, P=P)
            try:
                got = piv._measure(indices, batch_size, wind_size, overlap, multipass, who)
            finally:
                if piv is not self:
                    piv.close()
            if got is None:
                if indices is not None and not list(indices):
                    raise ValueError(f"StereoPIV.{who}: no pairs to measure the disparity on")
                raise RuntimeError(f"StereoPIV.{who}: round {k + 1}: the disparity pass delivered no field (too many invalid "
                                   "vectors: larger windows may reach the offset)")
            _, _, dx, dy, grid, (x, y) = got
            X, Y = engine.stereo_cells(x, y, self._scale, self._origin)
            free = np.ones(X.shape, dtype=bool) if grid is None else ~grid
            need = max(3, (int(free.sum()) + 3) // 4) if min_cells is None else int(min_cells)
            centre = (float(X.mean()), float(Y.mean()), 0.0)
            C1, C2 = engine.stereo_centre(P[0]), engine.stereo_centre(P[1])
            on = [torch.from_numpy(np.ascontiguousarray(q, dtype=np.float64)).to(dev) for q in (dx, dy, X, Y)]
            skip = torch.from_numpy(np.ascontiguousarray(~free).view(np.uint8)).to(dev)
            first = engine.stereo_triangulate(*on, C1, C2, skip=skip, gap_max=gap_max, centre=centre)
            count = int(first.count)

            def fit(rec):
                if int(rec.count) < need:
                    raise RuntimeError(f"StereoPIV.{who}: round {k + 1}: {int(rec.count)} of {int(free.sum())} non-excluded "
                                       f"cells survive, fewer than min_cells = {need}")
                return engine.stereo_plane(int(rec.count), rec.sums, centre)
            c0, c1, c2, rms = fit(first)
            for _ in range(2):
                rec = engine.stereo_triangulate(*on, C1, C2, skip=skip, gap_max=gap_max, plane=(c0, c1, c2), tol=float(trim) * rms,
                                                centre=centre, points=False)
                if int(rec.count) == count:
                    break
                count = int(rec.count)
                c0, c1, c2, rms = fit(rec)
            used = (first.status == 0).cpu().numpy()
            height = float(np.abs(c0 + c1 * X + c2 * Y)[free].max())
            rounds.append({"plane": (c0, c1, c2), "rms": rms, "count": count, "height": height,
                           "gap": float(np.median(first.gap.cpu().numpy()[used])),
                           "d": float(np.median(np.sqrt(dx * dx + dy * dy)[free]))})
            (P1, T1), (P2, _) = engine.stereo_correct(P[0], (c0, c1, c2)), engine.stereo_correct(P[1], (c0, c1, c2))
            P, T = (P1, P2), T @ T1
            if height <= tol:
                converged = True
                break
        if apply:
            for cam in self._cams:
                cam.close()
            self._build(P, self._shape)
        return {"P": tuple(Pc.copy() for Pc in P), "T": T, "rounds": rounds, "converged": converged}

    def close(self):
        for cam in self._cams:
            cam.close()
