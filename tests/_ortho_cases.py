"""The planted inputs of the orthoimage-colour tests: the smallest images and point sets at which the rule or the kernel can still
go wrong.  An image's samples are small integers, so every case can be run with every pixel type (float32 adds a quarter, so a
truncation would show) and in both layouts.  The points of a case are planted on the centres, the inner edges and the outer edges
of its images, one fp32 to either side of each, and are cycled up to T = 3 * 64 + 37 columns: three full waves and a partial one."""
import numpy as np

T_SMALL = 3 * 64 + 37
T_LARGE = 70001                       # 274 workgroups
DTYPES = ("uint8", "uint16", "float32")
LAYOUTS = ("chunky", "planar")
SCALE = {"uint8": 256.0, "uint16": 1.0, "float32": 0.5}
NODATA = 0


def samples(H, W, C, salt=0):
    """(H,W,C) int64, every sample in 1..250 (never the nodata value), different in every band"""
    r, c, b = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
    return (r * 37 + c * 11 + b * 53 + salt) % 250 + 1


def typed(values, dtype, layout):
    """the samples as the pixel array of an OrthoImage: float32 gets a fractional part, planar is (C,H,W)"""
    a = values.astype(np.float32) + np.float32(0.25) * (values != NODATA) if dtype == "float32" else values.astype(dtype)
    return np.ascontiguousarray(a if layout == "chunky" else a.transpose(2, 0, 1))


def f32_neighbours(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


def axis_values(lo, step, n):
    """fp32 coordinates along one axis of an image of n pixels that starts at `lo`: every pixel's centre, every edge (the two
    outer ones included) exactly and one fp32 below and above"""
    out = []
    for k in range(n + 1):
        out += f32_neighbours(np.float64(lo) + k * np.float64(step))
        if k < n:
            out.append(np.float32(np.float64(lo) + (k + 0.5) * np.float64(step)))
    return out


def planted_points(geos):
    """(2,n) fp32: for every image (x0, y0, px, py, W, H) all its x values against four y values -- the first and the last row's
    centre, the top edge and the bottom edge exactly -- and all its y values against the like four x values; then NaN and inf"""
    xs, ys = [], []
    for x0, y0, px, py, W, H in geos:
        bottom = np.float64(y0) - H * np.float64(py)
        ax, ay = axis_values(x0, px, W), axis_values(bottom, py, H)
        fx = [np.float32(x0 + 0.5 * px), np.float32(x0 + (W - 0.5) * px), np.float32(x0), np.float32(np.float64(x0) + W * np.float64(px))]
        fy = [np.float32(y0 - 0.5 * py), np.float32(y0 - (H - 0.5) * py), np.float32(y0), np.float32(bottom)]
        for a, b in ((ax, fy), (fx, ay)):
            gx, gy = np.meshgrid(np.array(a, dtype=np.float32), np.array(b, dtype=np.float32))
            xs.append(gx.reshape(-1))
            ys.append(gy.reshape(-1))
    x0, y0, px, py, W, H = geos[0]
    cx, cy = np.float32(x0 + 0.5 * px), np.float32(y0 - 0.5 * py)
    xs.append(np.array([np.nan, cx, cx, np.inf], dtype=np.float32))
    ys.append(np.array([cy, np.inf, -np.inf, np.nan], dtype=np.float32))
    out = np.stack([np.concatenate(xs), np.concatenate(ys)])
    assert out.shape[1] <= T_SMALL, out.shape                  # every planted point is a column of the T_SMALL cloud
    return out


def cloud_of(xy, T, seed=0):
    """(10,T) fp32: the planted points cycled (or cut) to T columns, z and the seven other rows seeded noise that a call must keep"""
    rng = np.random.default_rng(seed)
    cloud = rng.random((10, T), dtype=np.float32) * np.float32(1000)
    idx = np.arange(T) % xy.shape[1]
    cloud[0], cloud[1] = xy[0, idx], xy[1, idx]
    return cloud


# ---- the geometries: name -> (list of (x0, y0, px, py, H, W, C, salt, nodata pixels [(row, col)]), origin or None) -----------------
GEOMETRIES = {
    "one_pixel": ([(0.0, 1.0, 1.0, 1.0, 1, 1, 3, 5, [])], None),
    "rgb_half": ([(10.0, 20.0, 0.5, 0.5, 5, 4, 3, 0, [])], None),                           # exact in binary
    "uneven_02": ([(-1.0, 3.0, 0.2, 0.3, 4, 3, 3, 7, [])], None),                           # 0.2 and 0.3 are not
    "single_band": ([(5.0, 5.0, 0.25, 0.25, 3, 2, 1, 9, [])], None),
    # two images; the first has nodata pixels (0,2) and (1,1) inside the overlap, the second (2,0) under the first's (1,1)
    "overlap_nodata": ([(0.0, 2.0, 1.0, 1.0, 2, 3, 3, 1, [(0, 2), (1, 1)]), (1.0, 3.0, 1.0, 1.0, 3, 3, 3, 2, [(2, 0)])], None),
    # Lambert-93 magnitudes, the points in fp32 at those magnitudes (steps of 1/16 m in x, 1/2 m in y)
    "lambert": ([(650000.03, 6800000.3, 0.2, 0.7, 4, 5, 3, 3, [])], None),
    # the same image, the cloud shifted: the points are small numbers and keep centimetres
    "lambert_shifted": ([(650000.03, 6800000.3, 0.2, 0.7, 4, 5, 3, 3, [])], (650000.0, 6799990.0)),
}
CASE_NAMES = tuple(GEOMETRIES)


def case_values(name):
    """-> [(x0, y0, px, py, (H,W,C) int64 samples)], origin"""
    geo, origin = GEOMETRIES[name]
    out = []
    for x0, y0, px, py, H, W, C, salt, holes in geo:
        v = samples(H, W, C, salt)
        for r, c in holes:
            v[r, c, :] = NODATA
        out.append((x0, y0, px, py, v))
    return out, origin


def case_map(name):
    """the (bands, rows) a case is coloured with: RGB into rows 3, 4, 5, a single band into row 6 (the infrared call)"""
    return ((0, 1, 2), (3, 4, 5)) if GEOMETRIES[name][0][0][6] == 3 else ((0,), (6,))


def case_points(name):
    """(2,n) fp32 planted points of a case, in the cloud's frame (shifted where the case has an origin)"""
    vals, origin = case_values(name)
    ox, oy = origin if origin is not None else (0.0, 0.0)
    return planted_points([(x0 - ox, y0 - oy, px, py, v.shape[1], v.shape[0]) for x0, y0, px, py, v in vals])


def case_images(name, dtype, layout):
    """-> [(pixels, x0, y0, px, py)] in the FILES' frame, nodata value or None, origin or None"""
    vals, origin = case_values(name)
    has_holes = any(h for *_, h in GEOMETRIES[name][0])
    return [(typed(v, dtype, layout), x0, y0, px, py) for x0, y0, px, py, v in vals], (NODATA if has_holes else None), origin


# ---- answers worked out by hand on "overlap_nodata" (px = 1: image 1 covers x in [0,3), y in (0,2]; image 2 x in [1,4), y in (0,3]).
# (x, y, serving image or 0, its (row, col), class)
HAND = [
    (0.5, 1.5, 1, (0, 0), "first"),          # a centre of image 1
    (1.5, 1.5, 1, (0, 1), "first"),          # both images hold data here: the first wins
    (0.0, 2.0, 1, (0, 0), "first"),          # x0, y0 exactly: inside
    (2.0, 0.5, 1, (1, 2), "first"),          # on the inner edge x = 2: the pixel to the east
    (0.5, 1.0, 1, (1, 0), "first"),          # on the inner edge y = 1: the pixel to the south
    (2.5, 1.5, 2, (1, 1), "second"),         # image 1's pixel (0,2) is nodata: served by image 2 only
    (2.0, 2.0, 2, (1, 1), "second"),         # on two edges, image 1 nodata
    (3.5, 2.5, 2, (0, 2), "second"),         # image 1 does not reach
    (3.0, 0.5, 2, (2, 2), "second"),         # x0 + W px of image 1 exactly: outside it
    (1.5, 0.5, 0, None, "nodata_both"),      # image 1 (1,1) and image 2 (2,0) are nodata
    (1.0, 1.0, 0, None, "nodata_both"),      # the corner of those two pixels
    (-0.5, 1.0, 0, None, "outside"),
    (0.0, 0.0, 0, None, "outside"),          # y0 - H py of both images exactly
    (4.0, 2.5, 0, None, "outside"),          # x0 + W px of image 2 exactly
    (float("nan"), 1.5, 0, None, "outside"),
    (0.5, float("inf"), 0, None, "outside"),
    (0.5, float("-inf"), 0, None, "outside"),
]
