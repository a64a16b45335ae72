"""The predictor hand-off and the combine of a shifted pass (PIVbackend.py, `B:`), in plain numpy float64 -- the yardstick
of the decisions every pass after the first ends in, once the correlation result du, dv, invalid is taken as given.

handoff: what becomes of the spline predictor (u_raw, v_raw: the interpolated fields; mask: the interpolated validity
mask thresholded at 0.5) before the windows are shifted:
    CWS  (B:705-713)   u2 = u_raw / 2                       -- the halves are taken BEFORE the zeroing
                       u0 = 0 where mask else u_raw
    DWS  (B:778-785)   u0 = 0 where mask else u_raw
                       u2 = rint(u0 / 2)                    -- AFTER it; rint rounds ties to even
    CWS_Fast (B:630-633)  u0 as above, no half-shift field (the windows are resampled by -/+ u0 / 2 inside themselves)
combine (B:728-738 / B:800-810; CWS_Fast B:663-672):
    u = 2 * u2 + du                    (CWS_Fast: u = u0 + du)
    mask_u = (du > u0) and (rint(u0) > 0), or invalid       -- strict comparison; per component
    u = u0 where mask_u
and the same for v with its own mask.  Every operation is one IEEE float64 operation in the order written, so a device
that does the same gives the same bits."""
import numpy as np

MODES = ("DWS", "CWS", "CWS_Fast")


def handoff(mode, u_raw, v_raw, mask):
    """(u0, v0, u2, v2) float64 of the shape of u_raw; u2 = v2 = None for "CWS_Fast"."""
    if mode not in MODES:
        raise KeyError(mode)
    u_raw = np.asarray(u_raw, dtype=np.float64)
    v_raw = np.asarray(v_raw, dtype=np.float64)
    m = np.asarray(mask) != 0
    u2 = v2 = None
    if mode == "CWS":
        u2 = u_raw / np.float64(2)
        v2 = v_raw / np.float64(2)
    u0 = u_raw.copy()
    v0 = v_raw.copy()
    u0[m] = 0.0
    v0[m] = 0.0
    if mode == "DWS":
        u2 = np.rint(u0 / np.float64(2))
        v2 = np.rint(v0 / np.float64(2))
    return u0, v0, u2, v2


def clause(d, w0):
    """The reference's own mask of one component: (d > w0) * (rint(w0) > 0)."""
    d = np.asarray(d, dtype=np.float64)
    w0 = np.asarray(w0, dtype=np.float64)
    return (d > w0) & (np.rint(w0) > 0)


def combine(mode, du, dv, invalid, u0, v0, u2, v2):
    """(u, v) float64: the fields the pass returns."""
    if mode not in MODES:
        raise KeyError(mode)
    du = np.asarray(du, dtype=np.float64)
    dv = np.asarray(dv, dtype=np.float64)
    u0 = np.asarray(u0, dtype=np.float64)
    v0 = np.asarray(v0, dtype=np.float64)
    inv = np.zeros(du.shape, bool) if invalid is None else np.asarray(invalid) != 0
    if mode == "CWS_Fast":
        v = v0 + dv
        u = u0 + du
    else:
        v = np.float64(2) * np.asarray(v2, dtype=np.float64) + dv
        u = np.float64(2) * np.asarray(u2, dtype=np.float64) + du
    mask_u = clause(du, u0) | inv
    mask_v = clause(dv, v0) | inv
    return np.where(mask_u, u0, u), np.where(mask_v, v0, v)
