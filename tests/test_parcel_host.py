"""Host side of the parcel preparation (parcel.py): the plot lattice, the shape filter, plot ids and the argument checks of
the sn2_parcel_* entry points (CPU only: no compute call is made)."""
import ctypes
import math
import os

import numpy as np
import pytest

from stratanet2_vegetation_coverage_maps_amd import parcel
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args


def lattice_restated(x_min, x_max, y_min, y_max, args):
    """prepare_utils.py:95-146 with numpy 1.x's dtypes written out: fp32 bounds and extents, fp64 division, fp64 lattice
    (np.float32 scalar + python float -> float64 there), the first centre listed twice."""
    f32, f64 = np.float32, np.float64
    x_min, x_max, y_min, y_max = f32(x_min), f32(x_max), f32(y_min), f32(y_max)
    movement = 2 * math.cos(math.pi / 4) * 10 - 1 * 20 / args.diam_pix
    nx = math.ceil(f64(f32(x_max - x_min)) / f64(movement)) + 1
    ny = math.ceil(f64(f32(y_max - y_min)) / f64(movement)) + 1
    start_x = f64(x_min) + f64(movement / 4)
    start_y = f64(y_min) + f64(movement / 4)
    out = [[start_x, start_y]]
    for i in range(nx):
        cx = start_x + f64(i * movement)
        for j in range(ny):
            out.append([cx, start_y + f64(j * movement)])
    return np.array(out, dtype=np.float64)


def test_movement_is_the_reference_formula():
    args = make_args()
    assert parcel.plot_movement(args) == 2 * math.cos(math.pi / 4) * 10 - 20 / 20
    assert abs(parcel.plot_movement(args) - 13.1421) < 1e-4
    assert parcel.shape_buffer(args) == 30


@pytest.mark.parametrize("extent", [(120.0, 100.0), (5.0, 3.0), (0.0, 0.0), "multiple", (1000.37, 77.5)])
def test_lattice_matches_the_restatement(extent):
    args = make_args()
    mv = parcel.plot_movement(args)
    x0, y0 = np.float32(650001.25), np.float32(6860000.5)
    if extent == "multiple":                      # an extent at a multiple of the movement, up to an fp32 step
        for k in (1, 2, 7):
            xk = np.float32(x0 + np.float32(k * mv))
            for x1 in (np.nextafter(xk, np.float32(0)), xk, np.nextafter(xk, np.float32(np.inf))):
                got = parcel.parcel_plot_centers(x0, x1, y0, y0, args)
                np.testing.assert_array_equal(got, lattice_restated(x0, x1, y0, y0, args).astype(np.float32))
        x1, y1 = np.float32(x0 + np.float32(2 * mv)), np.float32(y0 + np.float32(3 * mv))
    else:
        x1, y1 = np.float32(x0 + np.float32(extent[0])), np.float32(y0 + np.float32(extent[1]))
    got = parcel.parcel_plot_centers(x0, x1, y0, y1, args)
    ref = lattice_restated(x0, x1, y0, y1, args)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, ref.astype(np.float32))
    assert np.array_equal(got[0], got[1])                                         # the first centre twice
    nx = math.ceil(float(np.float32(x1 - x0)) / mv) + 1
    ny = math.ceil(float(np.float32(y1 - y0)) / mv) + 1
    assert len(got) == 1 + nx * ny
    if extent == (0.0, 0.0) or extent == (5.0, 3.0):
        assert len(got) == 1 + (1 if extent == (0.0, 0.0) else 4)               # under one movement: 1 or 2 per axis


def test_keep_sees_the_fp64_lattice():
    args = make_args()
    seen = []

    def keep(lat):
        seen.append(lat.copy())
        return lat[:, 0] < lat[0, 0] + 20
    got = parcel.parcel_plot_centers(650000.0, 650100.0, 6860000.0, 6860050.0, args, keep=keep)
    assert seen[0].dtype == np.float64
    ref = lattice_restated(650000.0, 650100.0, 6860000.0, 6860050.0, args)
    np.testing.assert_array_equal(seen[0], ref)
    np.testing.assert_array_equal(got, ref[ref[:, 0] < ref[0, 0] + 20].astype(np.float32))


def _dense_boundary(rings, step=0.002):
    pts = []
    for r in rings:
        r = np.asarray(r, dtype=np.float64)
        for a, b in zip(r, np.roll(r, -1, axis=0)):
            n = max(2, int(np.hypot(*(b - a)) / step) + 1)
            t = np.linspace(0.0, 1.0, n)[:, None]
            pts.append(a + t * (b - a))
    return np.concatenate(pts)


def test_polygon_keep_against_a_sampled_boundary():
    from scipy.spatial import cKDTree
    ext = np.array([[0, 0], [60, 0], [60, 40], [30, 15], [0, 40]], dtype=np.float64)      # concave (notch at the top)
    hole = np.array([[10, 5], [24, 5], [24, 13], [10, 13]], dtype=np.float64)
    b = 3.0
    keep = parcel.polygon_keep([ext, np.concatenate([hole, hole[:1]])], b)       # closed and open rings
    rng = np.random.default_rng(0)
    pts = np.concatenate([rng.uniform(-6, 66, (4000, 2)) * [1, 46 / 72] + [0, -3],
                          np.array([[17, 9], [30, 20], [30, 14.0], [61, 20], [64, 20], [-2.99, 5], [-3.01, 5]])])
    got = keep(pts)
    dist, _ = cKDTree(_dense_boundary([ext, hole])).query(pts)

    def inside(p, ring):
        x, y = p
        c = False
        for (ax, ay), (bx, by) in zip(ring, np.roll(ring, -1, axis=0)):
            if (ay > y) != (by > y) and x < ax + (y - ay) * (bx - ax) / (by - ay):
                c = not c
        return c
    ins = np.array([inside(p, ext) != inside(p, hole) for p in pts])
    ref = ins | (dist < b)
    sure = np.abs(dist - b) > 0.01                         # away from the sampling error of the dense boundary
    assert np.array_equal(got[sure], ref[sure])
    # hole centre 4 m from its edges, above the notch (3.8 m from it), inside below it, 1 / 4 m outside, 2.99 / 3.01 m outside
    assert [bool(v) for v in got[-7:]] == [False, False, True, True, False, True, False]


def test_plot_ids():
    c = np.array([650123.94, 6860999.5], dtype=np.float32)
    assert parcel.plot_id(7, c) == f"PP00000007_X{int(c[0])}_Y{int(c[1])}"
    assert parcel.plot_id(7, c) == "PP00000007_X650123_Y6860999"
    assert parcel.plot_id(123456789, np.float32([1.9, 2.99])) == "PP123456789_X1_Y2"


def test_center_grid_is_a_csr_of_the_centres_in_reach():
    c = np.array([[0, 0], [5, 5], [5, 5], [40, 0], [1e6, 1e6], [25, 12]], dtype=np.float32)
    start, items, GX, GY, gx0, gy0, inv = parcel.center_grid(c, 10, (0.0, 0.0, 30.0, 10.0))
    assert 1.0 / inv >= 10.0
    assert len(start) == GX * GY + 1 and start[-1] == len(items) == 5           # the far centre is left out
    assert sorted(items.tolist()) == [0, 1, 2, 3, 5]
    for cell in range(GX * GY):
        ids = items[start[cell]:start[cell + 1]]
        assert list(ids) == sorted(ids)
        for q in ids:
            cx = int(np.floor((float(c[q, 0]) - gx0) * inv))
            cy = int(np.floor((float(c[q, 1]) - gy0) * inv))
            assert cy * GX + cx == cell
    assert parcel.center_grid(c[4:5], 10, (0.0, 0.0, 30.0, 10.0)) is None


def _raw_lib():
    from stratanet2_vegetation_coverage_maps_amd import _build, _lib
    path = _lib.LIB_PATH if os.path.exists(_lib.LIB_PATH) else _build.build(verbose=False)
    raw = ctypes.CDLL(path)
    for name, argtypes in list(_lib.SIGNATURES.items()) + list(_lib.SIZE_HELPERS.items()):
        if name.startswith("sn2_parcel"):
            fn = getattr(raw, name)
            fn.argtypes = argtypes
            fn.restype = ctypes.c_size_t if name in _lib.SIZE_HELPERS else ctypes.c_int
    return raw


def test_parcel_argument_checks_return_before_any_device_work():
    """Every call below fails a check before a kernel is launched (0x1000 is never dereferenced)."""
    lib = _raw_lib()
    f = 0x1000
    big = 1 << 31
    cnt, fill, zn = lib.sn2_parcel_count, lib.sn2_parcel_fill, lib.sn2_parcel_znorm
    nw = lib.sn2_parcel_count_ws_words(10, 4)
    assert nw >= 40
    ok = dict(GX=3, GY=3, inv=1 / 10.01, r=10.0)
    # count: NULL pointers, no centres, cells narrower than the disc, rows that do not cover the points, a short workspace
    assert cnt(None, 1000, 256, 4, f, 10, f, f, 3, 3, 0.0, 0.0, ok["inv"], 10.0, f, nw, f, f, None) == -1
    assert cnt(f, 1000, 256, 4, f, 0, f, f, 3, 3, 0.0, 0.0, ok["inv"], 10.0, f, nw, f, f, None) == -1
    assert cnt(f, 1000, 256, 4, f, 10, f, f, 3, 3, 0.0, 0.0, 1 / 9.0, 10.0, f, nw, f, f, None) == -1
    assert cnt(f, 1000, 256, 3, f, 10, f, f, 3, 3, 0.0, 0.0, ok["inv"], 10.0, f, nw, f, f, None) == -1
    assert cnt(f, 1000, 256, 5, f, 10, f, f, 3, 3, 0.0, 0.0, ok["inv"], 10.0, f, nw, f, f, None) == -1
    assert cnt(f, 1000, 256, 4, f, 10, f, f, 3, 3, 0.0, 0.0, ok["inv"], 10.0, f, nw - 1, f, f, None) == -1
    assert cnt(f, 1000, 256, 4, f, 10, f, f, 0, 3, 0.0, 0.0, ok["inv"], 10.0, f, nw, f, f, None) == -1
    # limits: 2^31 points, a (plot, row) table of 2^28 entries
    assert cnt(f, big, 1 << 20, 2048, f, 10, f, f, 3, 3, 0.0, 0.0, ok["inv"], 10.0, f, nw, f, f, None) == -2
    assert cnt(f, 1 << 20, 4, 1 << 18, f, 1 << 10, f, f, 3, 3, 0.0, 0.0, ok["inv"], 10.0, f, nw, f, f, None) == -2
    # fill: NULL, no slots, 2^31 slots
    assert fill(f, 1000, 256, 4, f, 10, f, f, 3, 3, 0.0, 0.0, ok["inv"], 10.0, None, f, 100, f, f, None) == -1
    assert fill(f, 1000, 256, 4, f, 10, f, f, 3, 3, 0.0, 0.0, ok["inv"], 10.0, f, f, 0, f, f, None) == -1
    assert fill(f, 1000, 256, 4, f, 10, f, f, 3, 3, 0.0, 0.0, ok["inv"], 10.0, f, f, big, f, f, None) == -2
    # z-norm: NULL, empty box, an extent beyond 2^26 cells, a short workspace
    zw = lib.sn2_parcel_znorm_ws_words(1000, 1.5, 0.0, 0.0, 300.0, 300.0)
    assert zw > 5 * 1000
    assert zn(f, 1000, 0.0, 0.0, 300.0, 300.0, 1.5, 10.0, None, f, 5, f, 100, f, zw, f, None) == -1
    assert zn(f, 1000, 0.0, 0.0, -1.0, 300.0, 1.5, 10.0, f, f, 5, f, 100, f, zw, f, None) == -1
    assert lib.sn2_parcel_znorm_ws_words(1000, 1.5, 0.0, 0.0, 20000.0, 20000.0) == 0
    assert zn(f, 1000, 0.0, 0.0, 20000.0, 20000.0, 1.5, 10.0, f, f, 5, f, 100, f, zw, f, None) == -2
    assert zn(f, 1000, 0.0, 0.0, 300.0, 300.0, 1.5, 10.0, f, f, 5, f, 100, f, zw - 1, f, None) == -1
    assert lib.sn2_parcel_znorm_ws_words(1000, 1.5, 0.0, 0.0, 3000.0, 3000.0) > 3 * 1999 * 1999   # 3 km x 3 km: supported


def test_synthetic_parcel_has_the_planted_structure():
    from stratanet2_vegetation_coverage_maps_amd.synthetic import make_parcel
    from scipy.spatial import cKDTree
    args = make_args()
    for order in ("scanline", "shuffled"):
        c = make_parcel(order=order, seed=3)
        assert c.dtype == np.float32 and c.shape[0] == 10
        assert c[0].min() == np.float32(650000.0) and c[1].max() == np.float32(6860100.0)
        cen = parcel.parcel_plot_centers(c[0].min(), c[0].max(), c[1].min(), c[1].max(), args)
        counts = np.array([len(v) for v in cKDTree(c[:2].T.astype(np.float64)).query_ball_point(cen.astype(np.float64), 10)])
        assert 50 in counts and 51 in counts
        assert (counts == 0).any()
