"""The keywords of Plan / OfflinePIV / ResidentPIV / run_folder, checked on the host (no GPU involved): the `*_arg`
parsers on one front end (_front), the table of what does not combine (EXCLUSIONS) and the record of the parsed values.

parse_options checks the keywords in one order for both constructors: depth, background, outlier, prefilter, equalize, mask,
uncertainty, derive, deform, correlation, weighting, what these refuse to combine, dynamic_mask, dewarp -- OfflinePIV checks
precision in front of them and looks up its device and opens its dataset behind them; ResidentPIV checks depth against the
frames' dtype and precision in front of them and asks for the GPU last.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from . import _lib


def is_int(x):
    """An integer that is no bool (bool and np.bool_ are both refused)."""
    return isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))


def is_real(x, lo=None, hi=None):
    """A real number that is no bool, inside [lo, hi] where given (a NaN fails the range)."""
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, (bool, np.bool_)) \
        and (lo is None or lo <= x) and (hi is None or x <= hi)


def number_pair(x):
    """(a, b) as floats of one number (taken twice) or a pair of numbers.  LookupError for a tuple or list that is no pair,
    TypeError / ValueError for what is no number (a bool is none)."""
    if not isinstance(x, (tuple, list)):
        x = (x, x)
    elif len(x) != 2:
        raise LookupError
    if any(isinstance(q, (bool, np.bool_)) for q in x):
        raise TypeError
    return float(x[0]), float(x[1])


def uint8_image(x, rank, name, a_noun, dims, lead=""):
    """A uint8 or bool image or stack of `rank` dimensions, numpy array or tensor, as a contiguous uint8 tensor (True -> 1; a
    uint8 image keeps its bytes).  The messages name it as `a_noun` ("an image") of `dims` ("[H, W]")."""
    noun = a_noun.split()[-1]
    if isinstance(x, np.ndarray):
        if x.dtype not in (np.uint8, np.bool_):
            raise ValueError(f"{name}: a uint8 or bool {noun}, got {x.dtype}")
        x = torch.from_numpy(np.ascontiguousarray(x))
    elif not isinstance(x, torch.Tensor):
        raise ValueError(f"{name}: {lead}a uint8 or bool numpy array or tensor {dims}, got {type(x).__name__}")
    elif x.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"{name}: a uint8 or bool {noun}, got {x.dtype}")
    if x.dim() != rank or x.numel() == 0:
        raise ValueError(f"{name}: {a_noun} {dims}, got shape {tuple(x.shape)}")
    return x.to(torch.uint8).contiguous()


def _front(value, name, keys, form="", defaults=None, short=None, short_int=None, wrap=None, own=None):
    """The steps every keyword shares.  value: what the caller gave.  keys: the known keys as the "known:" text lists them.
    form: the accepted forms, for the messages.  defaults: merged under the given keys.  short: {string: the dict it stands
    for}.  short_int: the key an integer stands for.  wrap: the key anything that is no dict stands for.  own: (the key set
    of the parser's result, the function that turns such a result back into an argument).  Returns (None, None) for None,
    else (the dict given or expanded, that dict over the defaults); ValueError for anything else."""
    if value is None:
        return None, None
    if own is not None and isinstance(value, dict) and set(value) == own[0]:
        value = own[1](value)
    if short is not None and isinstance(value, str):
        if value not in short:
            raise ValueError(f"{name}: {form}, got {value!r}")
        value = dict(short[value])
    if short_int is not None:
        if isinstance(value, (bool, np.bool_)):
            raise ValueError(f"{name}: {form}, got {value!r}")
        if isinstance(value, (int, np.integer)):
            value = {short_int: value}
    if not isinstance(value, dict):
        if wrap is None:
            raise ValueError(f"{name}: {form}, got {type(value).__name__}")
        value = {wrap: value}
    unknown = sorted(set(value) - set(keys), key=str)
    if unknown:
        raise ValueError(f"{name}: unknown key(s) {unknown}; known: {keys}")
    return value, dict(defaults or {}, **value)


CORRELATION_SIZES = (16, 32, 64)
CORRELATION_DEFAULTS = {"kind": "rpc", "diameter": 2.8, "floor": 2.0 ** -10}
CORRELATION_MAX_DIAMETER, CORRELATION_FLOOR_MIN, CORRELATION_FLOOR_MAX = 16.0, 2.0 ** -20, 2.0 ** -4
_CORRELATION = dict(
    name="correlation", keys=sorted(CORRELATION_DEFAULTS), defaults=CORRELATION_DEFAULTS,
    form=f"None, 'phase', 'rpc' or a dict of {sorted(CORRELATION_DEFAULTS)}", short={k: {"kind": k} for k in _lib.CORRELATIONS},
    own=({"kind", "dx", "dy", "floor"},
         lambda r: dict({"kind": r["kind"], "floor": r["floor"]},
                        **({} if r["kind"] == "phase" else {"diameter": (r["dx"], r["dy"])}))))


def correlation_arg(correlation):
    """The correlation= argument of Plan / OfflinePIV / ResidentPIV / run_folder / debug_pass, checked (no GPU involved):
    None (the plain cross-correlation), "phase" (phase-only correlation), "rpc" (robust phase correlation at the default
    particle-image diameter 2.8) or a dict with any of CORRELATION_DEFAULTS' keys -- diameter: the e^-2 diameter in pixels,
    one number or (d_x, d_y), 0..16; floor: 2^-20..2^-4 (include/torchpiv_hip.h: tpiv_plan_set_correlation has the
    definition).  Returns None or {"kind", "dx", "dy", "floor"}; "phase" has dx = dy = 0.  ValueError for anything else."""
    given, par = _front(correlation, **_CORRELATION)
    if par is None:
        return None
    if not isinstance(par["kind"], str) or par["kind"] not in _lib.CORRELATIONS:
        raise ValueError(f"correlation: kind must be one of {sorted(_lib.CORRELATIONS)}, got {par['kind']!r}")
    if par["kind"] == "phase" and "diameter" in given and given["diameter"] not in (0, 0.0, (0, 0), (0.0, 0.0)):
        raise ValueError("correlation: 'phase' has no diameter (it is 'rpc' at diameter 0)")
    try:
        dx, dy = (0.0, 0.0) if par["kind"] == "phase" else number_pair(par["diameter"])
        floor = float(par["floor"])
    except LookupError:
        raise ValueError(f"correlation: diameter must be a number or (d_x, d_y), got {par['diameter']!r}") from None
    except (TypeError, ValueError):
        raise ValueError(f"correlation: diameter and floor must be numbers, got {par['diameter']!r}, {par['floor']!r}") from None
    for q in (dx, dy):
        if not 0.0 <= q <= CORRELATION_MAX_DIAMETER:
            raise ValueError(f"correlation: diameter must be in 0..{CORRELATION_MAX_DIAMETER:g} pixels, got {q!r}")
    if not CORRELATION_FLOOR_MIN <= floor <= CORRELATION_FLOOR_MAX:
        raise ValueError(f"correlation: floor must be in 2^-20..2^-4, got {floor!r}")
    return {"kind": par["kind"], "dx": dx, "dy": dy, "floor": floor}


WEIGHTING_SIZES = (16, 32, 64)
WEIGHTING_DEFAULTS = {"kind": "gaussian", "sigma": 0.4}
WEIGHTING_SIGMA_MIN, WEIGHTING_SIGMA_MAX = 0.2, 4.0
_WEIGHTING = dict(
    name="weighting", keys=sorted(WEIGHTING_DEFAULTS), defaults=WEIGHTING_DEFAULTS,
    form=f"None, 'gaussian', 'uniform' or a dict of {sorted(WEIGHTING_DEFAULTS)}", short={k: {"kind": k} for k in _lib.WEIGHTINGS},
    own=({"kind", "sx", "sy"},
         lambda r: dict({"kind": r["kind"]}, **({} if r["kind"] == "uniform" else {"sigma": (r["sx"], r["sy"])}))))


def weighting_arg(weighting):
    """The weighting= argument of Plan / OfflinePIV / ResidentPIV / run_folder / debug_pass, checked (no GPU involved):
    None (the top-hat window of the plain passes), "gaussian" (at the default sigma 0.4), "uniform" (the top-hat window
    through the weighted kernels) or a dict with any of WEIGHTING_DEFAULTS' keys -- sigma: relative to the half window, one
    number or (sigma_x, sigma_y), 0.2..4 (include/torchpiv_hip.h: tpiv_plan_set_weighting has the definition).  Returns None
    or {"kind", "sx", "sy"}; "uniform" has no sigma (sx = sy = 0).  ValueError for anything else."""
    given, par = _front(weighting, **_WEIGHTING)
    if par is None:
        return None
    if not isinstance(par["kind"], str) or par["kind"] not in _lib.WEIGHTINGS:
        raise ValueError(f"weighting: kind must be one of {sorted(_lib.WEIGHTINGS)}, got {par['kind']!r}")
    if par["kind"] == "uniform":
        if "sigma" in given:
            raise ValueError("weighting: 'uniform' has no sigma")
        return {"kind": "uniform", "sx": 0.0, "sy": 0.0}
    try:
        sx, sy = number_pair(par["sigma"])
    except LookupError:
        raise ValueError(f"weighting: sigma must be a number or (sigma_x, sigma_y), got {par['sigma']!r}") from None
    except (TypeError, ValueError):
        raise ValueError(f"weighting: sigma must be a number or a pair of numbers, got {par['sigma']!r}") from None
    for q in (sx, sy):
        if not WEIGHTING_SIGMA_MIN <= q <= WEIGHTING_SIGMA_MAX:          # (NaN fails both comparisons)
            raise ValueError(f"weighting: sigma must be in {WEIGHTING_SIGMA_MIN:g}..{WEIGHTING_SIGMA_MAX:g} "
                             f"(relative to the half window), got {q!r}")
    return {"kind": "gaussian", "sx": sx, "sy": sy}


OUTLIER_DEFAULTS = {"threshold": 2.0, "eps": 0.1, "min_neighbours": 3}
_OUTLIER = dict(name="outlier", keys=sorted(OUTLIER_DEFAULTS), defaults=OUTLIER_DEFAULTS,
                form=f"None, 'median' or a dict of {sorted(OUTLIER_DEFAULTS)}", short={"median": {}})


def outlier_arg(outlier):
    """The outlier= argument of Plan / OfflinePIV / ResidentPIV / run_folder, checked (no GPU involved): None (no test),
    "median" (the normalized median test at OUTLIER_DEFAULTS) or a dict with any of threshold (> 0), eps (>= 0, pixels)
    and min_neighbours (1..8).  Returns None or the full parameter dict; anything else raises ValueError."""
    given, par = _front(outlier, **_OUTLIER)
    if par is None:
        return None
    try:
        thr, eps, mn = float(par["threshold"]), float(par["eps"]), par["min_neighbours"]
    except (TypeError, ValueError):
        raise ValueError(f"outlier: threshold and eps must be numbers, got {given!r}") from None
    if not thr > 0 or thr == float("inf"):
        raise ValueError(f"outlier: threshold must be a finite number > 0, got {par['threshold']!r}")
    if not eps >= 0 or eps == float("inf"):
        raise ValueError(f"outlier: eps must be a finite number >= 0, got {par['eps']!r}")
    if not is_int(mn) or not 1 <= mn <= 8:
        raise ValueError(f"outlier: min_neighbours must be an integer in 1..8, got {mn!r}")
    return {"threshold": thr, "eps": eps, "min_neighbours": int(mn)}


UNCERTAINTY_DEFAULTS = {"kind": "cs", "radius": 3}
UNCERTAINTY_MAX_RADIUS, UNCERTAINTY_WS = 4, (4, 128)
_UNCERTAINTY = dict(name="uncertainty", keys=sorted(UNCERTAINTY_DEFAULTS), defaults=UNCERTAINTY_DEFAULTS,
                    form=f"None, 'cs' or a dict of {sorted(UNCERTAINTY_DEFAULTS)}", short={"cs": {}})


def uncertainty_arg(uncertainty):
    """The uncertainty= argument of Plan / OfflinePIV / ResidentPIV, checked (no GPU involved): None (no estimate), "cs"
    (correlation statistics at UNCERTAINTY_DEFAULTS) or a dict with any of kind ("cs") and radius (an integer in 0..4, the
    reach of the covariance sum in pixels).  Returns None or the full parameter dict; anything else raises ValueError."""
    _, par = _front(uncertainty, **_UNCERTAINTY)
    if par is None:
        return None
    if par["kind"] != "cs":
        raise ValueError(f"uncertainty: kind must be 'cs' (correlation statistics), got {par['kind']!r}")
    R = par["radius"]
    if not is_int(R) or not 0 <= R <= UNCERTAINTY_MAX_RADIUS:
        raise ValueError(f"uncertainty: radius must be an integer in 0..{UNCERTAINTY_MAX_RADIUS}, got {R!r}")
    return {"kind": "cs", "radius": int(R)}


DERIVE_QUANTITIES = ("dudx", "dudy", "dvdx", "dvdy", "vorticity", "divergence", "shear", "q", "swirl", "u_smooth", "v_smooth")
DERIVE_DEFAULTS = {"radius": 2, "order": 2}
DERIVE_RADII, DERIVE_ORDERS = (1, 2, 3), (1, 2)
_DERIVE = dict(name="derive", keys=["order", "quantities", "radius"], defaults=DERIVE_DEFAULTS, wrap="quantities")


def derive_arg(derive):
    """The derive= argument of OfflinePIV / ResidentPIV / run_folder, checked (no GPU involved): None (nothing derived), one
    name of DERIVE_QUANTITIES, a tuple or list of them (each once), or a dict with "quantities" (a name or a tuple / list)
    and any of radius (1, 2 or 3: the fit takes the (2 radius + 1)^2 neighbourhood) and order (1 or 2: the polynomial),
    defaults DERIVE_DEFAULTS (include/torchpiv_hip.h: tpiv_field_fit has the operator).  Returns None or {"quantities":
    tuple, "radius": int, "order": int}; anything else raises ValueError."""
    _, par = _front(derive, **_DERIVE)
    if par is None:
        return None
    if "quantities" not in par:
        raise ValueError(f"derive: the dict needs 'quantities' (names out of {list(DERIVE_QUANTITIES)})")
    names = par["quantities"]
    if isinstance(names, str):
        names = (names,)
    if not isinstance(names, (tuple, list)) or not names:
        raise ValueError(f"derive: None, a name, a tuple or list of names or a dict of {_DERIVE['keys']}, got "
                         f"{par['quantities']!r}")
    for q in names:
        if not isinstance(q, str) or q not in DERIVE_QUANTITIES:
            raise ValueError(f"derive: unknown quantity {q!r}; known: {list(DERIVE_QUANTITIES)}")
    twice = sorted({q for q in names if list(names).count(q) > 1})
    if twice:
        raise ValueError(f"derive: {twice} named more than once")
    radius, order = par["radius"], par["order"]
    if not is_int(radius) or radius not in DERIVE_RADII:
        raise ValueError(f"derive: radius must be 1, 2 or 3, got {radius!r}")
    if not is_int(order) or order not in DERIVE_ORDERS:
        raise ValueError(f"derive: order must be 1 or 2, got {order!r}")
    return {"quantities": tuple(names), "radius": int(radius), "order": int(order)}


DEFORM_DEFAULTS = {"iterations": 3, "interp": "cubic", "smooth": True}
DEFORM_MAX_ITERATIONS = 8
_DEFORM = dict(name="deform", keys=sorted(DEFORM_DEFAULTS), defaults=DEFORM_DEFAULTS, short_int="iterations",
               form=f"None, an integer 0..{DEFORM_MAX_ITERATIONS} or a dict of {sorted(DEFORM_DEFAULTS)}")


def deform_arg(deform):
    """The deform= argument of Plan / OfflinePIV / ResidentPIV / run_folder, checked (no GPU involved): None or 0 (off), an
    integer 1..8 (that many rounds of image deformation behind the last pass at DEFORM_DEFAULTS) or a dict with any of
    iterations (0..8), interp ("cubic" or "linear") and smooth (bool: the 3 x 3 binomial on the predictor).  Returns None
    (off) or the full parameter dict; anything else raises ValueError."""
    _, par = _front(deform, **_DEFORM)
    if par is None:
        return None
    n = par["iterations"]
    if not is_int(n) or not 0 <= n <= DEFORM_MAX_ITERATIONS:
        raise ValueError(f"deform: iterations must be an integer in 0..{DEFORM_MAX_ITERATIONS}, got {n!r}")
    if not isinstance(par["interp"], str) or par["interp"] not in _lib.DEWARP_INTERPS:
        raise ValueError(f"deform: interp must be one of {sorted(_lib.DEWARP_INTERPS)}, got {par['interp']!r}")
    if not isinstance(par["smooth"], (bool, np.bool_)):
        raise ValueError(f"deform: smooth must be a bool, got {par['smooth']!r}")
    if n == 0:
        return None
    return {"iterations": int(n), "interp": par["interp"], "smooth": bool(par["smooth"])}


MASK_KEYS = ("image", "threshold", "pixels", "fill")
MASK_DEFAULTS = {"threshold": 0.5, "pixels": "zero", "fill": 0.0}
_MASK = dict(name="mask", keys=list(MASK_KEYS), defaults=MASK_DEFAULTS, wrap="image")


def mask_arg(mask):
    """The mask= argument of Plan / OfflinePIV / ResidentPIV / run_folder, checked (no GPU involved): None (no mask), an
    image -- uint8 or bool [H, W], numpy array or tensor, non-zero = masked -- or a dict with that image under "image" and
    any of threshold (a number in [0, 1]: the share of masked pixels above which a window is excluded), pixels ("zero":
    masked pixels are set to 0 in both frames before the passes, "keep": the frames stay as they are) and fill (any
    float, NaN allowed: the value delivered at excluded cells).  Returns None or {"image": contiguous uint8 tensor [H, W],
    "threshold": float, "pixels": str, "fill": float}; anything else raises ValueError."""
    _, par = _front(mask, **_MASK)
    if par is None:
        return None
    if "image" not in par:
        raise ValueError("mask: the dict needs an 'image' (uint8 or bool [H, W])")
    im = uint8_image(par["image"], 2, "mask", "an image", "[H, W]")      # (any non-zero byte of a uint8 image masks)
    thr, fill = par["threshold"], par["fill"]
    if not is_real(thr, 0, 1):
        raise ValueError(f"mask: threshold must be a number in [0, 1], got {thr!r}")
    if not isinstance(par["pixels"], str) or par["pixels"] not in ("zero", "keep"):
        raise ValueError(f"mask: pixels must be 'zero' or 'keep', got {par['pixels']!r}")
    if not is_real(fill):
        raise ValueError(f"mask: fill must be a float (NaN allowed), got {fill!r}")
    return {"image": im, "threshold": float(thr), "pixels": par["pixels"], "fill": float(fill)}


DYNMASK_KINDS = ("bright", "dark")
DYNMASK_KEYS = ("kind", "size", "level", "grow", "stack", "threshold", "pixels", "fill")
_DYNMASK = dict(name="dynamic_mask", keys=list(DYNMASK_KEYS), form=f"None or a dict of {list(DYNMASK_KEYS)}")


def dynamic_mask_arg(dynamic_mask, mask=None, stack=True):
    """The dynamic_mask= argument of OfflinePIV / ResidentPIV / run_folder, checked (no GPU involved).  None: no per-pair
    mask.  {"kind": "bright" | "dark", "size": k, "level": L, "grow": g}: one mask per pair segmented on the device from the
    frames themselves (tpiv_dynamic_mask: k odd in 3..63, L an integer in 0..255, g >= 0, default 0, with k // 2 + g <= 31).
    {"stack": uint8 or bool [N, H, W]}: one mask per pair from the caller, non-zero = masked (stack=False: this form is
    refused, for the classes whose frames do not come with an index the caller knows).  threshold, pixels and fill -- as
    in mask_arg, with its defaults -- are accepted in the dict only when mask= (`mask`: as given or as mask_arg returned
    it) is None; with mask= given, its image is OR-ed into every pair's mask and its three values apply.  Returns None or
    a dict with "threshold", "pixels", "fill" and either "kind", "size", "level", "grow" (ints but for kind) or "stack" (a
    contiguous uint8 tensor); anything else raises ValueError."""
    dynamic_mask, _ = _front(dynamic_mask, **_DYNMASK)
    if dynamic_mask is None:
        return None
    static = mask_arg(mask)                          # (what mask_arg returned passes through it unchanged)
    shared = [k for k in ("threshold", "pixels", "fill") if k in dynamic_mask]
    if static is not None and shared:
        raise ValueError(f"dynamic_mask: {shared} are given with mask= when both keywords are used, not here")
    probe = mask_arg(dict({"image": np.zeros((1, 1), np.uint8)}, **{k: dynamic_mask[k] for k in shared}))
    out = {k: (static if static is not None else probe)[k] for k in ("threshold", "pixels", "fill")}
    if "stack" in dynamic_mask:
        extra = sorted(set(dynamic_mask) & {"kind", "size", "level", "grow"})
        if extra:
            raise ValueError(f"dynamic_mask: 'stack' gives the masks; {extra} belong to the segmented form")
        if not stack:
            raise ValueError("dynamic_mask: the 'stack' form is for ResidentPIV, whose pairs the caller indexes; a run "
                             "over files takes the segmented form")
        out["stack"] = uint8_image(dynamic_mask["stack"], 3, "dynamic_mask", "a stack", "[N, H, W]", lead="stack must be ")
        return out
    missing = [k for k in ("kind", "size", "level") if k not in dynamic_mask]
    if missing:
        raise ValueError(f"dynamic_mask: the dict needs {missing} (or a 'stack')")
    kind, size, level, grow = (dynamic_mask["kind"], dynamic_mask["size"], dynamic_mask["level"], dynamic_mask.get("grow", 0))
    if not isinstance(kind, str) or kind not in DYNMASK_KINDS:
        raise ValueError(f"dynamic_mask: kind must be 'bright' or 'dark', got {kind!r}")
    if not (is_int(size) and 3 <= size <= 63 and size % 2 == 1):
        raise ValueError(f"dynamic_mask: size must be an odd integer in 3..63, got {size!r}")
    if not (is_int(level) and 0 <= level <= 255):
        raise ValueError(f"dynamic_mask: level must be an integer in 0..255, got {level!r}")
    if not (is_int(grow) and grow >= 0 and size // 2 + grow <= 31):
        raise ValueError(f"dynamic_mask: grow must be an integer >= 0 with size // 2 + grow <= 31, got {grow!r}")
    out.update(kind=kind, size=int(size), level=int(level), grow=int(grow))
    return out


PREFILTER_KEYS = ("kind", "size", "cap")
_PREFILTER = dict(name="prefilter", keys=list(PREFILTER_KEYS), form=f"None or a dict of {list(PREFILTER_KEYS)}")


def prefilter_arg(prefilter):
    """The prefilter= argument of OfflinePIV / ResidentPIV / run_folder, checked (no GPU involved): None (no filter) or a
    dict with kind ("min": sliding-minimum subtraction, "mean": local-mean high-pass, None: capping only), size (odd, 3..63;
    required with a kind) and optionally cap (1..255).  Returns None or {"kind", "size", "cap"} with ints (size None
    without a kind, cap None without capping); anything else, a dict that asks for nothing included, raises ValueError."""
    prefilter, _ = _front(prefilter, **_PREFILTER)
    if prefilter is None:
        return None
    kind, size, cap = prefilter.get("kind"), prefilter.get("size"), prefilter.get("cap")
    if kind is not None and (not isinstance(kind, str) or kind not in ("min", "mean")):
        raise ValueError(f"prefilter: kind must be 'min', 'mean' or None, got {kind!r}")
    if kind is not None and size is None:
        raise ValueError(f"prefilter: kind {kind!r} needs a size (odd, 3..63)")
    if size is not None and not (is_int(size) and 3 <= size <= 63 and size % 2 == 1):
        raise ValueError(f"prefilter: size must be an odd integer in 3..63, got {size!r}")
    if kind is None:
        size = None
    if cap is not None and not (is_int(cap) and 1 <= cap <= 255):
        raise ValueError(f"prefilter: cap must be an integer in 1..255, got {cap!r}")
    if kind is None and cap is None:
        raise ValueError("prefilter: the dict asks for nothing (no kind and no cap); pass None for no filter")
    return {"kind": kind, "size": None if size is None else int(size), "cap": None if cap is None else int(cap)}


EQUALIZE_KEYS = ("tile", "clip")
EQUALIZE_DEFAULTS = {"tile": 64, "clip": 3.0}
_EQUALIZE = dict(name="equalize", keys=list(EQUALIZE_KEYS), defaults=EQUALIZE_DEFAULTS,
                 form=f"None, 'clahe' or a dict of {list(EQUALIZE_KEYS)}", short={"clahe": EQUALIZE_DEFAULTS})


def equalize_arg(equalize):
    """The equalize= argument of OfflinePIV / ResidentPIV / run_folder, checked (no GPU involved): None (no equalization),
    "clahe" (tile 64, clip 3.0) or a dict with any of tile (integer, 8..256: the tile size aimed at, in pixels) and clip
    (1..256: the clip limit in units of the uniform bin height; 256 never clips).  Returns None or {"tile": int, "clip":
    float, "clip_q8": int} with clip_q8 = round(256 clip), what tpiv_equalize takes; anything else -- unknown strings or
    keys, bools, a non-integer tile, values out of range, an empty dict -- raises ValueError."""
    given, par = _front(equalize, **_EQUALIZE)
    if par is None:
        return None
    if not given:
        raise ValueError("equalize: the dict names neither tile nor clip; pass 'clahe' for the defaults, None for no filter")
    tile, clip = par["tile"], par["clip"]
    if not is_int(tile) or not 8 <= tile <= 256:
        raise ValueError(f"equalize: tile must be an integer in 8..256, got {tile!r}")
    if not is_real(clip, 1, 256):
        raise ValueError(f"equalize: clip must be a number in 1..256, got {clip!r}")
    return {"tile": int(tile), "clip": float(clip), "clip_q8": int(round(float(clip) * 256))}


DEPTH_BINS = 65536
DEPTH_CURVES = ("linear", "sqrt")
DEPTH_AUTO_DEFAULTS = {"clip_low": 0.0, "clip_high": 1e-4, "sample": 32}
DEPTH_KEYS = ("lo", "hi", "curve", "auto", "clip_low", "clip_high", "sample", "lut")
_DEPTH = dict(name="depth", keys=list(DEPTH_KEYS), form=f"None, 'auto' or a dict of {list(DEPTH_KEYS)}",
              short={"auto": {"auto": True}})


def depth_arg(depth):
    """The depth= argument of OfflinePIV / ResidentPIV / run_folder, checked (no GPU involved).  None: 8-bit frames as
    before.  {"lo", "hi", "curve"}: uint16 frames through depth_lut(lo, hi, curve) (integers 0 <= lo < hi <= 65535; curve
    "linear" by default, or "sqrt").  "auto" or {"auto": True, "clip_low", "clip_high", "sample", "curve"}: lo, hi from
    depth_range of the histogram of `sample` pairs of the recording (clips: fractions in [0, 0.5), defaults 0 and 1e-4;
    sample >= 1, default 32).  {"lut": table}: the caller's own uint8 [65536] table (numpy array or tensor).  Returns None
    or the full dict of its form -- {"lo", "hi", "curve"}, {"auto": True, "clip_low", "clip_high", "sample", "curve"} or
    {"lut": numpy uint8 [65536]}; anything else (unknown keys, mixed forms, a dict that asks for nothing) raises ValueError."""
    depth, _ = _front(depth, **_DEPTH)
    if depth is None:
        return None

    def only(form, allowed):
        extra = sorted(set(depth) - set(allowed))
        if extra:
            raise ValueError(f"depth: key(s) {extra} do not go with {form} (that form takes {list(allowed)})")
    if "lut" in depth:
        only("'lut'", ("lut",))
        lut = depth["lut"]
        if isinstance(lut, torch.Tensor):
            if lut.dtype != torch.uint8:
                raise ValueError(f"depth: lut must be uint8 [{DEPTH_BINS}], got dtype {lut.dtype}")
            lut = lut.detach().cpu().numpy()
        if not isinstance(lut, np.ndarray) or lut.dtype != np.uint8 or lut.shape != (DEPTH_BINS,):
            raise ValueError(f"depth: lut must be a uint8 array or tensor of shape ({DEPTH_BINS},), got "
                             f"{getattr(lut, 'dtype', type(lut).__name__)} {getattr(lut, 'shape', '')}")
        return {"lut": np.ascontiguousarray(lut)}
    curve = depth.get("curve", "linear")
    if not isinstance(curve, str) or curve not in DEPTH_CURVES:
        raise ValueError(f"depth: curve must be one of {list(DEPTH_CURVES)}, got {curve!r}")
    if "auto" in depth:
        only("'auto'", ("auto", "clip_low", "clip_high", "sample", "curve"))
        if depth["auto"] is not True:
            raise ValueError(f"depth: auto must be True (leave the key out for a fixed range), got {depth['auto']!r}")
        par = dict(DEPTH_AUTO_DEFAULTS, **{k: depth[k] for k in DEPTH_AUTO_DEFAULTS if k in depth})
        for k in ("clip_low", "clip_high"):
            if not (is_real(par[k]) and 0 <= par[k] < 0.5):
                raise ValueError(f"depth: {k} must be a fraction in [0, 0.5), got {par[k]!r}")
        if not is_int(par["sample"]) or par["sample"] < 1:
            raise ValueError(f"depth: sample must be an integer >= 1, got {par['sample']!r}")
        return {"auto": True, "clip_low": float(par["clip_low"]), "clip_high": float(par["clip_high"]),
                "sample": int(par["sample"]), "curve": curve}
    if "lo" in depth or "hi" in depth:
        only("a fixed range", ("lo", "hi", "curve"))
        if "lo" not in depth or "hi" not in depth:
            raise ValueError("depth: a fixed range needs both lo and hi")
        lo, hi = depth["lo"], depth["hi"]
        if not is_int(lo) or not is_int(hi) or not 0 <= lo < hi <= DEPTH_BINS - 1:
            raise ValueError(f"depth: lo and hi must be integers with 0 <= lo < hi <= {DEPTH_BINS - 1}, got {lo!r}, {hi!r}")
        return {"lo": int(lo), "hi": int(hi), "curve": curve}
    raise ValueError("depth: the dict asks for nothing (no lo / hi, no auto, no lut); pass None for 8-bit frames")


DEWARP_FORMS = ("homography", "poly", "map")
DEWARP_KEYS = DEWARP_FORMS + ("interp", "fill")
DEWARP_DEFAULTS = {"interp": "cubic", "fill": 0}
DEWARP_POLY_ORDERS = {3: 1, 6: 2, 10: 3}            # coefficients per axis -> order
_DEWARP = dict(name="dewarp", keys=list(DEWARP_KEYS), defaults=DEWARP_DEFAULTS,
               form=f"None or a dict with one of {list(DEWARP_FORMS)}")


def dewarp_arg(dewarp):
    """The dewarp= argument of OfflinePIV / ResidentPIV / run_folder, checked (no GPU involved): None (frames as recorded)
    or a dict that holds exactly one backward map -- where in the camera frame every pixel of the rectified frame comes
    from; pixel centres at the integers, x along the columns, y along the rows, the rectified frame has the camera
    frame's shape --
      "homography": 3 x 3, (x, y, 1) of the output pixel -> the source pixel, homogeneous;
      "poly": float [2, K], K = 3, 6 or 10 -- source x (row 0) and source y (row 1) in pixels as polynomials of order 1, 2
        or 3 in the output coordinates normalised to [-1, 1], xn = 2 x / (W - 1) - 1, yn = 2 y / (H - 1) - 1, with the terms
        in the order 1, xn, yn | xn^2, xn yn, yn^2 | xn^3, xn^2 yn, xn yn^2, yn^3;
      "map": a pair (xs, ys) of float arrays [H, W], the source coordinates themselves (radial models, the output of a
        calibration package); non-finite entries count as outside;
    and optionally "interp" ("cubic", the default: Catmull-Rom; or "linear") and "fill" (integer 0..255, default 0: the
    value of pixels whose source lies outside the camera frame).  Returns None or {form: float64 array(s), "interp": str,
    "fill": int}; anything else raises ValueError."""
    _, par = _front(dewarp, **_DEWARP)
    if par is None:
        return None
    forms = [k for k in DEWARP_FORMS if k in par]
    if len(forms) != 1:
        raise ValueError(f"dewarp: exactly one of {list(DEWARP_FORMS)} is needed, got {forms}")
    form = forms[0]

    def array(x, what):
        if isinstance(x, torch.Tensor):
            x = x.detach().cpu().numpy()
        try:
            a = np.asarray(x)
            if a.dtype.kind not in "fiu":
                raise TypeError
            return np.ascontiguousarray(a, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"dewarp: {what} must be an array of numbers") from None
    if form == "homography":
        val = array(par[form], "the homography")
        if val.shape != (3, 3) or not np.isfinite(val).all():
            raise ValueError(f"dewarp: the homography must be a finite 3 x 3 matrix, got shape {val.shape}")
        if not np.any(val[2] != 0):
            raise ValueError("dewarp: the homography's last row is zero")
    elif form == "poly":
        val = array(par[form], "the polynomial")
        if val.ndim != 2 or val.shape[0] != 2 or val.shape[1] not in DEWARP_POLY_ORDERS or not np.isfinite(val).all():
            raise ValueError(f"dewarp: the polynomial must be finite [2, K] with K in {sorted(DEWARP_POLY_ORDERS)}, got "
                             f"shape {val.shape}")
    else:
        pair = par[form]
        if not isinstance(pair, (tuple, list)) or len(pair) != 2:
            raise ValueError("dewarp: map must be a pair (xs, ys) of float arrays [H, W]")
        xs, ys = array(pair[0], "map xs"), array(pair[1], "map ys")
        if xs.ndim != 2 or xs.shape != ys.shape or xs.size == 0:
            raise ValueError(f"dewarp: map must be a pair of arrays [H, W] of one shape, got {xs.shape} and {ys.shape}")
        val = (xs, ys)
    if not isinstance(par["interp"], str) or par["interp"] not in _lib.DEWARP_INTERPS:
        raise ValueError(f"dewarp: interp must be one of {sorted(_lib.DEWARP_INTERPS)}, got {par['interp']!r}")
    if not is_int(par["fill"]) or not 0 <= par["fill"] <= 255:
        raise ValueError(f"dewarp: fill must be an integer in 0..255, got {par['fill']!r}")
    return {form: val, "interp": par["interp"], "fill": int(par["fill"])}


def background_arg(background, shape=None):
    """The background= argument of OfflinePIV / ResidentPIV, checked: None, "min", or a pair of uint8 images [H, W] as
    torch tensors (one image given for both frames of a pair, or a pair (bg_a, bg_b); numpy arrays or tensors).  shape:
    the frame shape the images must have (None: not known, e.g. an empty folder).  Anything else raises ValueError."""
    if background is None:
        return None
    if isinstance(background, str):
        if background != "min":
            raise ValueError(f"background: None, 'min', a uint8 image [H, W] or a pair of them, got {background!r}")
        return "min"
    imgs = list(background) if isinstance(background, (tuple, list)) else [background, background]
    if len(imgs) != 2:
        raise ValueError(f"background: a pair (bg_a, bg_b) holds two images, got {len(imgs)}")
    out = []
    for im in imgs:
        if isinstance(im, np.ndarray):
            if im.dtype != np.uint8:
                raise ValueError(f"background: uint8 images, got {im.dtype}")
            im = torch.from_numpy(np.ascontiguousarray(im))
        elif not isinstance(im, torch.Tensor):
            raise ValueError(f"background: a uint8 numpy array or tensor [H, W], got {type(im).__name__}")
        elif im.dtype != torch.uint8:
            raise ValueError(f"background: uint8 images, got {im.dtype}")
        if im.dim() != 2:
            raise ValueError(f"background: images [H, W], got shape {tuple(im.shape)}")
        out.append(im)
    if out[0].shape != out[1].shape or (shape is not None and tuple(out[0].shape) != tuple(shape)):
        raise ValueError(f"background: images of the frame shape {None if shape is None else tuple(shape)}, got "
                         f"{tuple(out[0].shape)} and {tuple(out[1].shape)}")
    return out


def pass_sizes(ws, ov, n_pass, pass_scale):
    """[(ws, ov)] of the passes of a plan (PIVbackend.py:856-857: int(x // scale) from pass to pass)."""
    out = [(int(ws), int(ov))]
    for _ in range(max(int(n_pass), 1) - 1):
        w, o = out[-1]
        out.append((int(w // pass_scale), int(o // pass_scale)))
    return out


ENSEMBLE_SIZES = (16, 32, 64)
# in the order they are switched on: at construction a feature meets only those in front of it, ensemble() meets them all
FEATURES = ("uncertainty", "deform", "ensemble", "correlation", "weighting", "dynamic_mask")
SIZES = {"ensemble": ENSEMBLE_SIZES, "correlation": CORRELATION_SIZES, "weighting": WEIGHTING_SIZES}
# One row per refusal, a subject's rows tried top to bottom: (subject, what it meets -- a feature, the mode "CWS_Fast", or
# "sizes": a pass outside SIZES[subject] --, exception, message).  csrc/c_api.cpp guards the same pairs (REFUSALS).
EXCLUSIONS = (
    ("ensemble", "dynamic_mask", ValueError, "ensemble correlation does not combine with dynamic_mask="),
    ("ensemble", "correlation", ValueError, "ensemble correlation does not combine with correlation="),
    ("ensemble", "weighting", ValueError, "ensemble correlation does not combine with weighting="),
    ("ensemble", "uncertainty", ValueError, "ensemble correlation does not combine with uncertainty="),
    ("ensemble", "deform", ValueError, "ensemble correlation does not combine with deform="),
    ("ensemble", "sizes", NotImplementedError,
     "ensemble correlation covers window sizes 16, 32 and 64; a pass of {ws} is not covered"),
    ("correlation", "uncertainty", ValueError, "correlation= does not combine with uncertainty="),
    ("correlation", "deform", ValueError, "correlation= does not combine with deform="),
    ("correlation", "ensemble", ValueError, "correlation= does not combine with ensemble correlation"),
    ("correlation", "CWS_Fast", NotImplementedError, "correlation=: the CWS_Fast iteration has no filtered kernel"),
    ("correlation", "sizes", NotImplementedError,
     "correlation=: filtered passes cover window sizes 16, 32 and 64; a pass of {ws} is not covered"),
    ("weighting", "uncertainty", ValueError,
     "weighting= does not combine with uncertainty= (its estimator sums over a top-hat window)"),
    ("weighting", "ensemble", ValueError, "weighting= does not combine with ensemble correlation"),
    ("weighting", "correlation", ValueError, "weighting= does not combine with correlation="),
    ("weighting", "CWS_Fast", NotImplementedError, "weighting=: the CWS_Fast iteration has no weighted kernel"),
    ("weighting", "sizes", NotImplementedError,
     "weighting=: weighted passes cover window sizes 16, 32 and 64; a pass of {ws} is not covered"),
)


def refuse(subject, on, sizes=(), mode=None):
    """Raises the first row of EXCLUSIONS that `subject` meets: on -- {feature: its parsed value, None where it is off} of
    the other features --, sizes -- the window size of every pass --, mode."""
    for subj, other, exc, msg in EXCLUSIONS:
        if subj != subject:
            continue
        if other == "sizes":
            for ws in sizes:
                if ws not in SIZES[subject]:
                    raise exc(msg.format(ws=ws))
        elif on.get(other) is not None or (other == "CWS_Fast" and mode == "CWS_Fast"):
            raise exc(msg)


def refuse_all(on, sizes, mode=None):
    """refuse() for every feature that is on, each against the features in front of it in FEATURES."""
    for i, subject in enumerate(FEATURES):
        if on.get(subject) is not None:
            refuse(subject, {k: on.get(k) for k in FEATURES[:i]}, sizes, mode)


def ensemble_check(sizes, uncertainty=None, deform=None):
    """What ensemble correlation refuses, checked without a GPU: the window sizes of every pass must be 16, 32 or 64
    (NotImplementedError names the size), and it combines with neither uncertainty= nor deform= (ValueError)."""
    refuse("ensemble", dict(uncertainty=uncertainty, deform=deform), sizes)


def correlation_check(sizes, mode=None, uncertainty=None, deform=None, ensemble=False):
    """What correlation= refuses, checked without a GPU: it combines with neither uncertainty= nor deform= nor ensemble
    correlation (ValueError), the window size of every pass must be 16, 32 or 64 and the mode must not be CWS_Fast
    (NotImplementedError names it)."""
    refuse("correlation", dict(uncertainty=uncertainty, deform=deform, ensemble=ensemble or None), sizes, mode)


def weighting_check(sizes, mode=None, uncertainty=None, ensemble=False, correlation=None):
    """What weighting= refuses, checked without a GPU: it combines with neither uncertainty= (its estimator sums over a
    top-hat window) nor ensemble correlation nor correlation= (ValueError), the window size of every pass must be 16, 32 or
    64 and the mode must not be CWS_Fast (NotImplementedError names it).  It does combine with deform=."""
    refuse("weighting", dict(uncertainty=uncertainty, ensemble=ensemble or None, correlation=correlation), sizes, mode)


KEYWORDS = ("background", "outlier", "prefilter", "depth", "equalize", "mask", "dewarp", "uncertainty", "derive", "deform",
            "correlation", "weighting", "dynamic_mask")
# The thirteen keywords of OfflinePIV / ResidentPIV, as given or as their parsers returned them (None: not given).
Options = namedtuple("Options", KEYWORDS, defaults=(None,) * len(KEYWORDS))


def mask_shape(mask, shape):
    """ValueError unless the image of mask_arg's result has the frame shape (None, for either: nothing to check)."""
    if shape is not None and mask is not None and tuple(mask["image"].shape) != tuple(shape):
        raise ValueError(f"mask of shape {tuple(mask['image'].shape)} for frames of shape {tuple(shape)}")


def dewarp_shape(dewarp, shape):
    """ValueError unless a map given as coordinate arrays (dewarp_arg's result) has the frame shape (None: as above)."""
    if shape is not None and dewarp is not None and "map" in dewarp and tuple(dewarp["map"][0].shape) != tuple(shape):
        raise ValueError(f"dewarp map of shape {tuple(dewarp['map'][0].shape)} for frames of shape {tuple(shape)}")


def parse_options(run, frames_shape=None, stack=True, **given):
    """The keywords of a constructor (given: by name, as the caller gave them) to an Options record of parsed values, in the
    order of the module docstring.  run: the run parameters (a dict with wind_size, overlap, multipass, multipass_scale,
    multipass_mode).  frames_shape: (n, H, W) of the frames where the caller has them -- background, mask, a dewarp map
    and a dynamic_mask stack are then held against it.  stack: whether dynamic_mask= may be the 'stack' form."""
    raw = Options(**given)
    shape = None if frames_shape is None else tuple(frames_shape[1:])
    depth = depth_arg(raw.depth)
    background = background_arg(raw.background, shape)
    outlier, prefilter, equalize = outlier_arg(raw.outlier), prefilter_arg(raw.prefilter), equalize_arg(raw.equalize)
    mask = mask_arg(raw.mask)
    mask_shape(mask, shape)
    opts = Options(background=background, outlier=outlier, prefilter=prefilter, depth=depth, equalize=equalize, mask=mask,
                   uncertainty=uncertainty_arg(raw.uncertainty), derive=derive_arg(raw.derive), deform=deform_arg(raw.deform),
                   correlation=correlation_arg(raw.correlation), weighting=weighting_arg(raw.weighting))
    sizes = [w for w, _ in pass_sizes(run["wind_size"], run["overlap"], run["multipass"], run["multipass_scale"])]
    refuse_all(opts._asdict(), sizes, run["multipass_mode"])
    dynamic_mask = dynamic_mask_arg(raw.dynamic_mask, mask, stack=stack)
    if frames_shape is not None and dynamic_mask is not None and "stack" in dynamic_mask \
            and tuple(dynamic_mask["stack"].shape) != tuple(frames_shape):
        raise ValueError(f"dynamic_mask: a stack of shape {tuple(dynamic_mask['stack'].shape)} for frames of shape "
                         f"{tuple(frames_shape)}")
    dewarp = dewarp_arg(raw.dewarp)
    dewarp_shape(dewarp, shape)
    return opts._replace(dynamic_mask=dynamic_mask, dewarp=dewarp)
