"""The canvases the GeoTIFF tests share: every (W, H) of the issue's lists for every C, rows just below, at and above the staging
limit, one large canvas, and the atlases built from them.  The values are made once per shape (a fixed seed per shape) and never
changed: coverages in [0, 1] with, planted at fixed places where the canvas has room, NaNs of several payloads, +-0, +-inf,
denormals, and neighbours whose sign-and-exponent bytes are 0xFF then 0x00, so that predictor 3's difference wraps."""
import functools

import numpy as np

WIDTHS = (1, 2, 3, 5, 16, 63, 64, 65, 255, 257)
HEIGHTS = (1, 2, 5)
BANDS = (1, 3, 5, 6, 8)
STAGE_BYTES = 16384                  # sn2_tiff_pack_stage_max(); tests/test_geotiff_host.py holds the library to it
BIG = (6, 1031, 1025)

# bit patterns planted in row-major order from pixel 0 of every band (as many as fit); 0xFF800000 then 0x00000001: the top bytes
# 0xFF, 0x00 follow one another, and 0x00 - 0xFF wraps to 0x01
SPECIALS = np.array([0xFF800000, 0x00000001, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FFFFFFF, 0x80000000, 0x00000000, 0x7F800000,
                     0x807FFFFF, 0x00800000, 0x3F800000, 0xFF7FFFFF, 0x00FF00FF, 0xFF00FF00], dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def canvas(C: int, H: int, W: int, all_nan_band: int = -1) -> np.ndarray:
    """(C,H,W) fp32, read-only.  all_nan_band: that band holds NaNs of two payloads only."""
    rs = np.random.RandomState(1000003 * C + 1009 * H + W)
    a = rs.rand(C, H, W).astype(np.float32)
    u = a.view(np.uint32).reshape(C, -1)
    n = min(len(SPECIALS), u.shape[1])
    for c in range(C):
        u[c, :n] = np.roll(SPECIALS, -c)[:n]                 # another special first in every band, so that 1 x 1 canvases vary
    if u.shape[1] > 40:
        u[:, 33::7] ^= 0x80000000                           # negative values, so the minimum is one
    if 0 <= all_nan_band < C:
        u[all_nan_band, :] = 0x7FC00000
        u[all_nan_band, ::2] = 0xFFC12345
    a.setflags(write=False)
    return a


def shapes_for(C: int):
    """(H, W) of the small canvases of one atlas of C bands: the product of the lists, then the rows around the staging limit in the
    BAND layout (wc = W) and, where C divides it, in the PIXEL layout (wc = W C)"""
    out = [(H, W) for H in HEIGHTS for W in WIDTHS]
    lim = STAGE_BYTES // 4
    out += [(2, lim - 1), (2, lim), (2, lim + 1)]
    if C > 1:                                               # lim // C is AT the limit when C divides it, else the last row below
        out += [(2, lim // C - 1), (2, lim // C), (2, lim // C + 1)]
    return out


def atlas_canvases(C: int):
    """the canvases of `shapes_for(C)`; the second has an all-NaN band"""
    return [canvas(C, H, W, all_nan_band=(C - 1 if i == 1 else -1)) for i, (H, W) in enumerate(shapes_for(C))]


def k4_canvases(C: int):
    """[ordinary, empty, 1 x 1, wide]: the second is flagged 'no file'"""
    return [canvas(C, 5, 65), canvas(C, 1, 1), canvas(C, 1, 1), canvas(C, 2, 5003)], [False, True, False, False]


def arena_of(canvases) -> np.ndarray:
    """the C-band arena of an atlas: canvas k's (C,H,W) at word C base_k"""
    return np.concatenate([c.reshape(-1) for c in canvases])
