"""Planted inputs of the parcel-cut tests (tests/test_cut_parcels_host.py, tests/test_gpu_cut_parcels.py): polygons and tile
points chosen so that every clause of the rule of include/strata_hip.h, "Parcel cut", decides at least one point.  The reference
is always `parcel.polygon_keep` (numpy, fp64) and plain numpy indexing; nothing here calls the code under test."""
import functools

import numpy as np

from stratanet2_vegetation_coverage_maps_amd import parcel

B = 20.0                      # the buffer of every planted case
f32 = np.float32
T_PLANTED = 5 * 2048 + 37     # more than one workgroup of rows, a ragged last step of 64


def _circle(cx, cy, r, n):
    a = 2 * np.pi * np.arange(n) / n
    return np.round(np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], 1) * 1024) / 1024      # on a 2^-10 m grid: an origin shift is exact


def shapes():
    """name -> ring list.  All rings counter-clockwise, the hole too: nonzero winding then calls the hole inside."""
    sq = lambda x0, y0, x1, y1: np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=np.float64)
    return {
        "square": [sq(0, 0, 100, 100)],                                                   # an edge on x = 0, a vertex at the origin
        "concave_L": [np.array([[300, 0], [400, 0], [400, 40], [340, 40], [340, 100], [300, 100]], dtype=np.float64)],
        "holed": [sq(600, 0, 760, 160), sq(640, 40, 720, 120)],
        "two_part": [sq(0, 300, 50, 350), sq(200, 300, 250, 350)],
        "repeated_vertex": [np.array([[300, 300], [300, 300], [360, 300], [360, 360], [300, 360]], dtype=np.float64)],   # l2 == 0
        "horizontal": [np.array([[600, 300], [650, 300], [650, 330], [700, 330], [700, 300], [750, 300], [750, 400], [600, 400]],
                                dtype=np.float64)],
        "circle300": [_circle(1000.0, 100.0, 60.0, 300)],                                 # E exceeds any edge chunk
        "empty": [sq(5000, 5000, 5050, 5050)],                                            # gets no point
        "neighbour": [sq(130, 0, 200, 100)],                                              # its buffer overlaps the square's
    }


NAMES = list(shapes())


def planted():
    """[(label, x, y, {parcel name: belongs})]: x, y as fp32; the parcels not named do not get the point."""
    m20 = f32(-20.0)
    return [
        ("x=-20 exactly: strict <", m20, f32(50), {"square": False}),
        ("x=-20 one fp32 toward zero", np.nextafter(m20, f32(0)), f32(50), {"square": True}),
        ("x=-20 one fp32 away", np.nextafter(m20, f32(-100)), f32(50), {"square": False}),
        ("round join 144 + 256 = 400", f32(-12), f32(-16), {"square": False}),
        ("round join, just inside", f32(-12), f32(-15.9), {"square": True}),
        ("corner of the box, outside the round join", f32(-15), f32(-15), {"square": False}),
        ("py = a vertex's y, inside, far from the boundary", f32(725), f32(330), {"horizontal": True}),
        ("py = a vertex's y, outside", f32(560), f32(330), {"horizontal": False}),
        ("in the hole, nearer than b to its ring", f32(650), f32(80), {"holed": True}),
        ("the hole's centre", f32(680), f32(80), {"holed": False}),
        ("between ring and hole", f32(620), f32(80), {"holed": True}),
        ("in two parcels' buffers", f32(115), f32(50), {"square": True, "neighbour": True}),
        ("in none", f32(2000), f32(2000), {}),
        ("NaN x", f32(np.nan), f32(50), {}),
        ("infinite y", f32(50), f32(np.inf), {}),
        ("-infinite x", f32(-np.inf), f32(50), {}),
        ("the L's notch, far from both edges", f32(370), f32(70), {"concave_L": False}),
        ("the L's notch, near the corner", f32(345), f32(45), {"concave_L": True}),
        ("first part", f32(25), f32(325), {"two_part": True}),
        ("second part", f32(225), f32(325), {"two_part": True}),
        ("between the parts", f32(125), f32(325), {"two_part": False}),
        ("inside the ring with the repeated vertex", f32(330), f32(330), {"repeated_vertex": True}),
        ("near the repeated vertex", f32(290), f32(290), {"repeated_vertex": True}),
        ("the circle's centre", f32(1000), f32(100), {"circle300": True}),
        ("outside the circle, within b", f32(1070), f32(100), {"circle300": True}),
        ("outside the circle, beyond b", f32(1081), f32(100), {"circle300": False}),
    ]


@functools.lru_cache(maxsize=None)
def tile(T=T_PLANTED, seed=0):
    """(10,T) fp32: random points over the planted polygons' surroundings, the planted points spread over the rows (the first
    column, the last, the ragged last step) -> (tile, the planted points' columns).  Rows 2..9 are random."""
    rng = np.random.default_rng(seed)
    t = rng.random((10, T), dtype=np.float32) * f32(255)
    t[0] = (rng.random(T) * 1200 - 60).astype(np.float32)
    t[1] = (rng.random(T) * 520 - 60).astype(np.float32)
    pts = planted()
    cols = np.concatenate([[0, T - 1, T - 20], rng.choice(np.arange(1, T - 40), len(pts) - 3, replace=False)])
    for c, (_, x, y, _) in zip(cols, pts):
        t[0, c], t[1, c] = x, y
    t.setflags(write=False)
    return t, cols


@functools.lru_cache(maxsize=None)
def masks(T=T_PLANTED, seed=0, b=B):
    """the reference: per planted parcel, polygon_keep over the tile's fp32 x, y widened to fp64 -> (K,T) bool"""
    t, _ = tile(T, seed)
    pts = t[:2].T.astype(np.float64)
    m = np.stack([parcel.polygon_keep(r, b)(pts) for r in shapes().values()])
    m.setflags(write=False)
    return m


def classes(T=T_PLANTED, seed=1):
    """(T) uint8 class bytes: 2, 5, 7 and 18 at random, so that dropping (7, 18) removes points of every parcel"""
    return np.random.default_rng(seed).choice(np.array([2, 5, 7, 18], dtype=np.uint8), T)


@functools.lru_cache(maxsize=None)
def many(K=70, T=6000, seed=3, b=4.0):
    """K random five-vertex parcels of about 15 m over one 120 m tile: more candidates than a wave has lanes, several per cell
    -> (ring lists, tile (10,T), masks (K,T), b)"""
    rng = np.random.default_rng(seed)
    rings = []
    for _ in range(K):
        c = rng.random(2) * 120
        a = np.sort(rng.random(5) * 2 * np.pi)
        r = 4 + 8 * rng.random(5)
        rings.append([np.stack([c[0] + r * np.cos(a), c[1] + r * np.sin(a)], 1)])
    t = rng.random((10, T), dtype=np.float32) * f32(255)
    t[0] = (rng.random(T) * 140 - 10).astype(np.float32)
    t[1] = (rng.random(T) * 140 - 10).astype(np.float32)
    pts = t[:2].T.astype(np.float64)
    m = np.stack([parcel.polygon_keep(r, b)(pts) for r in rings])
    t.setflags(write=False)
    m.setflags(write=False)
    return rings, t, m, b
