"""Numpy model of the geometric mask (torchpiv_amd/csrc/mask.hip, include/torchpiv_hip.h): the count of masked pixels per
window, the grid of excluded cells, the pixel step and the step that writes excluded cells into the fields of a pass.
Brute force on purpose: nothing here shares a line with the device code."""
import numpy as np


def field_shape(H, W, ws, ov):
    return (H - ws) // (ws - ov) + 1, (W - ws) // (ws - ov) + 1


def coverage(mask, ws, ov):
    """int32 [n_rows, n_cols]: non-zero bytes of mask [H, W] in window (i, j) = rows i (ws - ov) ... + ws, columns
    j (ws - ov) ... + ws."""
    H, W = mask.shape
    nr, nc = field_shape(H, W, ws, ov)
    step = ws - ov
    count = np.zeros((nr, nc), np.int32)
    for i in range(nr):
        for j in range(nc):
            count[i, j] = np.count_nonzero(mask[i * step:i * step + ws, j * step:j * step + ws])
    return count


def grid(count, ws, threshold):
    """bool: excluded cells, count > limit with limit = int(threshold * ws * ws) -- one float64 product, truncated."""
    limit = int(float(threshold) * float(ws * ws))
    return count > limit


def apply(frames, mask):
    """frames uint8 [..., H, W] with the masked pixels (mask != 0) set to 0."""
    keep = np.where(mask != 0, 0x00, 0xFF).astype(np.uint8)
    return frames & keep


def fields(u, v, inv, grid, value, status=None):
    """Copies of u, v, inv [batch, n_rows, n_cols] (and status) with excluded cells at u = v = +0.0, inv = value,
    status = 2."""
    g = np.asarray(grid) != 0
    u, v, inv = u.copy(), v.copy(), inv.copy()
    u[:, g] = 0.0
    v[:, g] = 0.0
    inv[:, g] = value
    if status is None:
        return u, v, inv
    status = status.copy()
    status[:, g] = 2
    return u, v, inv, status
