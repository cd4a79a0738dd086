"""The crop and the band means of the parcel report (include/strata_hip.h: sn2_mosaic_crop_stats), restated in fp64 numpy.

A restatement of the header's rule, NOT a fixture from the reference: the reference crops with shapely's `contains` through
rasterio (`inference/geotiff_raster.py:238-253`), neither is available to this project's tests, so -- as for
`parcel.polygon_keep` -- the stated even-odd rule is the yardstick.  Every expression is written the way the header writes it;
numpy rounds each product, difference, quotient and sum to fp64 on its own.
"""
import numpy as np


def pixel_centres(H, W, x_min, y_max, pix):
    """-> px (W), py (H) fp64: px = x_min + pix * (c + 0.5), py = y_max - pix * (r + 0.5)"""
    x_min, y_max, pix = np.float64(x_min), np.float64(y_max), np.float64(pix)
    px = x_min + pix * (np.arange(W, dtype=np.float64) + 0.5)
    py = y_max - pix * (np.arange(H, dtype=np.float64) + 0.5)
    return px, py


def inside_mask(H, W, x_min, y_max, pix, edges):
    """(H,W) bool: pixel centre inside by the even-odd rule over edges (E,4) = (ax, ay, bx, by)"""
    e = np.asarray(edges, dtype=np.float64).reshape(-1, 4)
    ax, ay, bx, by = (e[:, k] for k in range(4))
    px, py = pixel_centres(H, W, x_min, y_max, pix)
    mask = np.zeros((H, W), dtype=bool)
    for r in range(H):
        with np.errstate(divide="ignore", invalid="ignore"):
            crosses = (ay > py[r]) != (by > py[r])
            xint = ax + (py[r] - ay) * (bx - ax) / (by - ay)
        right = crosses[None, :] & (px[:, None] < xint[None, :])
        mask[r] = np.count_nonzero(right, axis=1) % 2 == 1
    return mask


def crop_stats(bands, x_min, y_max, pix, edges=None):
    """bands (C,H,W) fp32 -> (cropped copy, mean (C) fp64, count (C) int64); edges None: no crop"""
    out = np.array(bands, dtype=np.float32, copy=True)
    C, H, W = out.shape
    if edges is not None:
        out[:, ~inside_mask(H, W, x_min, y_max, pix, edges)] = np.nan
    flat = out.reshape(C, -1).astype(np.float64)
    count = (~np.isnan(flat)).sum(1).astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(count > 0, np.nansum(flat, axis=1) / count, np.nan)
    return out, mean, count
