"""K parcels in one pass, host side (include/strata_hip.h, "the plots of K parcels in one pass"): the parcel table against a
python-loop restatement, the refusals of every entry point (they answer before any device work: every call below fails a check,
no fake pointer is read), header / binding / exports, and the choice `batched=None` makes.  No device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from stratanet2_vegetation_coverage_maps_amd import _lib, parcel
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args

COLS = _lib.SN2_PARCELS_COLS
EINVAL, ELIMIT = _lib.SN2_EINVAL, _lib.SN2_ELIMIT
FAKE = 0x1000                                                # a "device pointer" that is never dereferenced
R, ZR = 10.0, 1.5
f32 = np.float32


def bits64(v):
    return int(np.array(v, dtype=np.float64).view(np.int64))


def pack2(a, b):
    return int(np.array([a, b], dtype=np.float32).view(np.int64)[0])


def table_by_hand(T, P, grids, boxes, radius=R, zradius=ZR):
    """the parcel table restated: prefixes by a python loop, the z-norm grid in numpy's fp32"""
    K = len(T)
    work = sum(int(t) * int(p) for t, p in zip(T, P))
    L = max(2048, (-(-work // 2 ** 26) + 63) // 64 * 64)
    inv = f32(1.0) / (f32(zradius) * f32(1.0001))
    t = np.zeros((K + 1, COLS), dtype=np.int64)
    t0 = row0 = c0 = e0 = g0 = z0 = 0
    for k in range(K):
        b = np.asarray(boxes[k], dtype=np.float32)
        rows = -(-int(T[k]) // L) if P[k] else 0
        zgx = zgy = 0
        g = (0, 0, 0, 0, 0)
        if P[k]:
            zgx, zgy = int(f32(b[2] - b[0]) * inv) + 1, int(f32(b[3] - b[1]) * inv) + 1
            g = (grids[k][2], grids[k][3], bits64(grids[k][4]), bits64(grids[k][5]), bits64(grids[k][6]))
        t[k] = [t0, T[k], row0, c0, P[k], e0, g0, *g, z0, pack2(b[0], b[1]), pack2(b[2], b[3]), zgx | (zgy << 32)]
        t0, row0, c0, e0, z0 = t0 + int(T[k]), row0 + rows, c0 + int(P[k]), e0 + rows * int(P[k]), z0 + zgx * zgy
        if P[k]:
            g0 += grids[k][2] * grids[k][3] + 1
    t[K, [0, 1, 2, 3, 4, 5, 6, 12, 13]] = [t0, L, row0, c0, K, e0, g0, z0, pack2(radius, zradius)]
    return t, L


def a_set(K, empty=()):
    """K parcels with their lattices and centre grids as `prepare_parcels` makes them; the parcels in `empty` have no centre"""
    a = make_args()
    rng = np.random.default_rng(K)
    T, P, grids, boxes = [], [], [], []
    for k in range(K):
        x0, y0 = 650000.0 + 1000 * k, 6860000.0 + 10 * k
        box = np.array([x0, y0, x0 + 40 + 35 * rng.random(), y0 + 30 + 55 * rng.random()], dtype=np.float32)
        cen = parcel.parcel_plot_centers(box[0], box[2], box[1], box[3], a)
        g = None if k in empty else parcel.center_grid(cen, R, box)
        T.append(int(rng.integers(1, 300000)))
        P.append(0 if g is None else len(cen))
        grids.append(g)
        boxes.append(box)
    return T, P, grids, np.array(boxes)


@pytest.mark.parametrize("K,empty", [(1, ()), (4, ()), (5, (0, 2, 4)), (3, (0, 1, 2))])
def test_table_against_the_restatement(K, empty):
    T, P, grids, boxes = a_set(K, empty)
    tab = ops.ParcelTable(T, P, grids, boxes, R, ZR)
    want, L = table_by_hand(T, P, grids, boxes)
    assert tab.host.dtype == np.int64 and tab.host.shape == (K + 1, COLS) and np.array_equal(tab.host, want)
    assert (tab.K, tab.L, tab.T_all, tab.P_all) == (K, L, sum(T), sum(P)) and tab.dev is None
    assert tab.rows == sum(-(-t // L) for t, p in zip(T, P) if p) and tab.entries == sum(-(-t // L) * p for t, p in zip(T, P))
    assert tab.csr_words == sum(len(g[0]) for g in grids if g is not None)
    # the workspaces: the scan's block sums + the entries; the single-parcel z-norm layout over all points and all cells
    scan = lambda n: 2 * (-(-n // 4096) + 2)
    assert tab.count_ws_words == scan(tab.entries) + tab.entries
    assert tab.znorm_ws_words == (scan(tab.zcells) + 3) // 4 * 4 + 5 * tab.T_all + 3 * tab.zcells + 1
    for k in empty:
        assert tab.host[k, 4] == 0 and tab.host[k + 1, 2] == tab.host[k, 2] and tab.host[k + 1, 5] == tab.host[k, 5] and tab.host[k, 15] == 0


def test_one_row_length_for_the_set_grows_with_the_work():
    T, P, grids, boxes = a_set(2)
    T = [2 ** 30, 2 ** 29]                                         # sum T P / 2^26 = 16 P[0] + 8 P[1]
    big = (np.zeros(2, dtype=np.int32), np.zeros(1, dtype=np.int32), 1, 1, 0.0, 0.0, 1.0 / 11.0)
    P, grids = [300, 100], [big, big]
    tab = ops.ParcelTable(T, P, grids, boxes, R, ZR)
    want, L = table_by_hand(T, P, grids, boxes)
    assert 16 * 300 + 8 * 100 == 5600 and L == 5632 and L % 64 == 0 and L == tab.L and np.array_equal(tab.host, want)   # rounded up to 64
    assert tab.entries == -(-T[0] // L) * 300 + -(-T[1] // L) * 100 < 2 ** 28


def _table_call(lib, **kw):
    T, P, grids, boxes = a_set(3)
    a = dict(K=3, T=np.array(T, dtype=np.int64), P=np.array(P, dtype=np.int32), GX=np.array([g[2] for g in grids], dtype=np.int32),
             GY=np.array([g[3] for g in grids], dtype=np.int32), grid=np.array([g[4:7] for g in grids], dtype=np.float64),
             boxes=np.ascontiguousarray(boxes, dtype=np.float32), radius=R, zradius=ZR)
    a.update(kw)
    out = np.zeros((a["K"] + 1 if a["K"] > 0 else 1, COLS), dtype=np.int64)
    L, cw, zw = ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
    p = lambda v: None if v is None else v.ctypes.data
    return lib.sn2_parcels_table(a["K"], p(a["T"]), p(a["P"]), p(a["GX"]), p(a["GY"]), p(a["grid"]), p(a["boxes"]), a["radius"], a["zradius"],
                                 out.ctypes.data, ctypes.byref(L), ctypes.byref(cw), ctypes.byref(zw))


def test_table_builder_refusals():
    lib = _lib.load()
    T, P, grids, boxes = a_set(3)
    assert _table_call(lib) == 0
    for name in ("T", "P", "GX", "GY", "grid", "boxes"):
        assert _table_call(lib, **{name: None}) == EINVAL, name
    assert _table_call(lib, K=0) == EINVAL and _table_call(lib, radius=0.0) == EINVAL and _table_call(lib, zradius=float("nan")) == EINVAL
    assert _table_call(lib, T=np.array([5, 0, 7], dtype=np.int64)) == EINVAL                                  # T_k = 0
    assert _table_call(lib, P=np.array([5, -1, 7], dtype=np.int32)) == EINVAL
    assert _table_call(lib, GX=np.array([5, 0, 7], dtype=np.int32)) == EINVAL
    narrow = np.array([g[4:7] for g in grids], dtype=np.float64)
    narrow[1, 2] = 1.0 / 9.99                                                                                # cells narrower than the radius
    assert _table_call(lib, grid=narrow) == EINVAL
    narrow[1, 2] = 1.0 / 10.0
    assert _table_call(lib, grid=narrow) == 0
    bad = np.array(boxes, dtype=np.float32)
    bad[2, 2] = bad[2, 0] - 1                                                                                # x_max < x_min
    assert _table_call(lib, boxes=bad) == EINVAL
    bad[2, 2] = np.inf
    assert _table_call(lib, boxes=bad) == EINVAL
    # limits: 2^31 points, 2^28 entries, 2^28 centre cells, 2^26 z-norm cells
    assert _table_call(lib, T=np.array([2 ** 30, 2 ** 30, 7], dtype=np.int64)) == ELIMIT
    assert _table_call(lib, T=np.array([2 ** 30, 2 ** 30 - 8, 7], dtype=np.int64)) == 0
    assert _table_call(lib, P=np.array([2 ** 30, 2 ** 30, 7], dtype=np.int32)) == ELIMIT
    assert _table_call(lib, T=np.array([2 ** 30] * 3, dtype=np.int64) // 2, P=np.array([2 ** 28] * 3, dtype=np.int32)) == ELIMIT   # entries
    assert _table_call(lib, T=np.array([64] * 3, dtype=np.int64), P=np.array([2 ** 27] * 3, dtype=np.int32)) == ELIMIT             # one row each
    assert _table_call(lib, T=np.array([64] * 3, dtype=np.int64), P=np.array([2 ** 26] * 3, dtype=np.int32)) == 0
    assert _table_call(lib, GX=np.array([2 ** 14, 3, 3], dtype=np.int32), GY=np.array([2 ** 14, 3, 3], dtype=np.int32)) == ELIMIT
    wide = np.array(boxes, dtype=np.float32)
    wide[0, 2:] = wide[0, :2] + f32(13000.0)                                                                 # (13 km / 1.5 m)^2 > 2^26 cells
    assert _table_call(lib, boxes=wide) == ELIMIT
    wide[0, 2:] = wide[0, :2] + f32(8000.0)
    wide[1, 2:] = wide[1, :2] + f32(8000.0)
    wide[2, 2:] = wide[2, :2] + f32(8000.0)                                                                  # each fits, their sum does not
    assert _table_call(lib, boxes=wide) == ELIMIT
    with pytest.raises(ops.StrataHipError, match="SN2_ELIMIT"):
        ops.ParcelTable(T, P, grids, wide, R, ZR)
    with pytest.raises(ValueError):
        ops.ParcelTable(T, P, [None] + grids[1:], boxes, R, ZR)


def _bad_tables():
    T, P, grids, boxes = a_set(4, empty=(2,))
    good = ops.ParcelTable(T, P, grids, boxes, R, ZR).host
    out = []
    for (r, c, v) in [(1, 1, 0), (1, 1, -5),                                      # T_k <= 0
                      (1, 0, good[1, 0] + 1), (2, 0, good[1, 0]), (3, 0, good[1, 0]),        # unsorted / shifted point bases
                      (1, 2, good[1, 2] + 1), (3, 3, good[3, 3] - 1), (1, 5, 0), (3, 6, 0), (3, 12, 0),
                      (1, 4, good[1, 4] + 1), (2, 4, 1), (1, 7, good[1, 7] + 1), (1, 8, 0), (0, 11, bits64(1.0 / 9.0)), (0, 11, bits64(np.nan)),
                      (0, 13, good[0, 14]), (1, 15, good[1, 15] + 1),
                      (4, 0, good[4, 0] + 1), (4, 1, 4096), (4, 2, good[4, 2] + 1), (4, 4, 3), (4, 5, good[4, 5] - 1), (4, 7, 1),
                      (4, 13, pack2(11.0, ZR))]:
        t = good.copy()
        t[r, c] = v
        out.append((t, EINVAL, (r, c, v)))
    t = good.copy()
    t[0, 1] = 2 ** 31                                                                  # T_all >= 2^31
    out.append((t, ELIMIT, "points"))
    t = good.copy()
    lo = good[0, 13:14].view(np.float32)
    t[0, 14] = pack2(lo[0] + f32(20000.0), lo[1] + f32(20000.0))
    out.append((t, ELIMIT, "z cells"))
    return good, out


def test_argument_checks_return_before_any_device_work():
    lib = _lib.load()
    good, bad = _bad_tables()
    K = 4
    p = lambda a: a.ctypes.data

    def count(**kw):
        a = dict(arena=FAKE, K=K, th=p(good), td=FAKE, centers=FAKE, start=FAKE, items=FAKE, radius=R, ws=FAKE, words=2 ** 40, prefix=FAKE,
                 total=FAKE, plot_start=FAKE, stream=None)
        return lib.sn2_parcels_count(*{**a, **kw}.values())

    def fill(**kw):
        a = dict(arena=FAKE, K=K, th=p(good), td=FAKE, centers=FAKE, start=FAKE, items=FAKE, radius=R, prefix=FAKE, base=FAKE, sum_n=100,
                 raw=FAKE, pidx=FAKE, stream=None)
        return lib.sn2_parcels_fill(*{**a, **kw}.values())

    def znorm(**kw):
        a = dict(arena=FAKE, K=K, th=p(good), td=FAKE, radius=ZR, disc=R, offsets=FAKE, centers=FAKE, of=FAKE, P=3, pidx=FAKE, sum_n=100,
                 ws=FAKE, words=2 ** 40, raw=FAKE, stream=None)
        return lib.sn2_parcels_znorm(*{**a, **kw}.values())

    for fn, ptrs in ((count, ("arena", "th", "td", "centers", "start", "items", "ws", "prefix", "total", "plot_start")),
                     (fill, ("arena", "th", "td", "centers", "start", "items", "prefix", "base", "raw", "pidx")),
                     (znorm, ("arena", "th", "td", "offsets", "centers", "of", "pidx", "ws", "raw"))):
        for name in ptrs:
            assert fn(**{name: None}) == EINVAL, (fn.__name__, name)
        for k in (0, -1, 3):
            assert fn(K=k) == EINVAL, (fn.__name__, k)                      # the table of four parcels is no other set's
        for t, rc, what in bad:
            assert fn(th=p(t)) == rc, (fn.__name__, what)
    assert count(radius=9.0) == EINVAL and fill(radius=11.0) == EINVAL and znorm(radius=R) == EINVAL and znorm(disc=9.0) == EINVAL
    # workspaces: 8-byte aligned and long enough for the count, 16-byte aligned for the z-norm
    assert count(ws=FAKE + 4) == EINVAL and count(words=10) == EINVAL
    assert znorm(ws=FAKE + 8) == EINVAL and znorm(ws=FAKE + 4) == EINVAL and znorm(words=10) == EINVAL
    assert fill(sum_n=0) == EINVAL and fill(sum_n=2 ** 31) == ELIMIT and znorm(sum_n=0) == EINVAL and znorm(sum_n=2 ** 31) == ELIMIT
    assert znorm(P=0) == EINVAL
    # a set without any centre has nothing to count
    T, P, grids, boxes = a_set(2, empty=(0, 1))
    none = ops.ParcelTable(T, P, grids, boxes, R, ZR)
    assert none.P_all == 0 and count(K=2, th=p(none.host)) == EINVAL and fill(K=2, th=p(none.host)) == EINVAL and znorm(K=2, th=p(none.host)) == EINVAL

    # the bounding boxes: starts = point_start and the workgroup prefix, checked on the host copy
    starts = ops.parcels_bbox_starts([5, 4096, 4097, 1])
    assert starts.dtype == np.int64 and starts.tolist() == [[0, 5, 4101, 8198, 8199], [0, 1, 2, 4, 5]]

    def bbox(**kw):
        a = dict(arena=FAKE, T_all=8199, K=4, sh=p(starts), sd=FAKE, state=FAKE, stream=None)
        return lib.sn2_parcels_bbox(*{**a, **kw}.values())
    for name in ("arena", "sh", "sd", "state"):
        assert bbox(**{name: None}) == EINVAL, name
    assert bbox(K=0) == EINVAL and bbox(K=3) == EINVAL and bbox(T_all=8198) == EINVAL and bbox(T_all=0) == EINVAL
    for (r, c, v) in [(0, 0, 1), (0, 2, 5), (0, 2, 4), (0, 3, 9000), (1, 0, 1), (1, 2, 3), (1, 4, 6), (1, 3, 3)]:   # T_k = 0, unsorted, wrong prefix
        s = starts.copy()
        s[r, c] = v
        assert bbox(sh=p(s)) == EINVAL, (r, c, v)
    big = ops.parcels_bbox_starts([2 ** 30, 2 ** 30])
    assert bbox(K=2, T_all=2 ** 31, sh=p(big)) == ELIMIT


def test_box_state_coding_is_order_preserving():
    v = np.array([-np.inf, -6.5e6, -1.0, -1e-30, -0.0, 0.0, 1e-30, 1.0, 650000.06, np.inf], dtype=np.float32)
    u = v.view(np.uint32)
    code = np.where(u >> 31 == 1, ~u, u | np.uint32(0x80000000)).astype(np.uint32)       # common.h: f2ord
    assert (np.diff(code.astype(np.int64)) > 0).all()
    assert ops.parcels_bbox_decode(code.view(np.int32).reshape(-1, 1)).tobytes() == v.tobytes()
    ident = ops.parcels_bbox_identity(3)
    assert ident.dtype == np.int32 and ident.view(np.uint32).tolist() == [[2 ** 32 - 1, 2 ** 32 - 1, 0, 0]] * 3
    assert (code < 2 ** 32 - 1).all() and (code > 0).all()                               # any value moves the identity


def test_header_binding_and_exports_agree():
    import stratanet2_vegetation_coverage_maps_amd as pkg
    from stratanet2_vegetation_coverage_maps_amd import _build
    txt = open(os.path.join(ROOT, "include", "strata_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("sn2_parcels_table", "sn2_parcels_bbox", "sn2_parcels_count", "sn2_parcels_fill", "sn2_parcels_znorm"):
        assert re.search(r"^int\s+%s\s*\(" % name, txt, flags=re.M) and name in _lib.SIGNATURES and hasattr(raw, name)
    assert not re.search(r"^(extern\s+)?size_t\s+sn2_parcels", txt, flags=re.M)         # sizes come back through pointers
    assert _lib.SN2_VERSION == 102 and _lib.load().sn2_version() == 102 and re.search(r"#define SN2_VERSION 102\b", txt)
    assert (COLS, _lib.SN2_PARCELS_BBOX_CHUNK) == (16, 4096)
    assert "ParcelClouds" in pkg.__all__ and pkg.ParcelClouds is parcel.ParcelClouds
    assert "parcels.hip" in _build.SOURCES and "parcel_rules.h" in _build.HEADERS
    assert "arrival order" in txt[txt.index("the plots of K parcels in one pass"):txt.index("#define SN2_PARCELS_COLS")]
    for fn in (parcel.prepare_parcels, parcel.predict_parcels):
        assert inspect.signature(fn).parameters["batched"].default is None
    assert {"arena", "point_start"} <= set(parcel.ParcelClouds.__dataclass_fields__) and isinstance(parcel.ParcelClouds.K, property)


def test_pack_upload_is_one_copy_with_every_array_in_place():
    arrays = [np.arange(7, dtype=np.int64).reshape(1, 7), np.zeros((0, 2), dtype=np.float32), np.arange(5, dtype=np.int32),
              np.linspace(0, 1, 6, dtype=np.float32).reshape(3, 2)]
    out = ops.pack_upload(arrays, "cpu")
    base = out[0].data_ptr()
    for a, t in zip(arrays, out):
        assert tuple(t.shape) == a.shape and t.numpy().dtype == a.dtype and np.array_equal(t.numpy(), a)
        assert (t.data_ptr() - base) % 16 == 0 and t.is_contiguous()
    assert out[3].untyped_storage().data_ptr() == out[0].untyped_storage().data_ptr()


def test_none_picks_the_loop_for_one_parcel_and_the_arena_for_two(monkeypatch):
    a = make_args()
    calls = []

    def one(cloud, args, keep=None, device=None, min_points=parcel.MIN_POINTS):
        calls.append(("loop", cloud.shape[1], min_points))
        return parcel._empty("cpu")

    class Arena(Exception):
        pass

    def arena(clouds, device=None):
        raise Arena(len(clouds))
    monkeypatch.setattr(parcel, "prepare_parcel", one)
    monkeypatch.setattr(parcel.ParcelClouds, "from_clouds", staticmethod(arena))
    c = [np.zeros((10, 5), dtype=np.float32), np.zeros((10, 9), dtype=np.float32)]
    s = parcel.prepare_parcels(c[:1], a)
    assert calls == [("loop", 5, 51)] and isinstance(s, parcel.ParcelSet) and s.n_parcels == 1 and len(s) == 0
    with pytest.raises(Arena):
        parcel.prepare_parcels(c, a)
    with pytest.raises(Arena):
        parcel.prepare_parcels(c[:1], a, batched=True)
    calls.clear()
    s = parcel.prepare_parcels(c, a, batched=False, min_points=2001)
    assert calls == [("loop", 5, 2001), ("loop", 9, 2001)] and s.n_parcels == 2 and s.parcel_start.tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        parcel.prepare_parcels([], a)
    with pytest.raises(ValueError):
        parcel.prepare_parcels(c, a, shapes=[None])
    with pytest.raises(ValueError):
        parcel.prepare_parcels(c, a, min_points=0, batched=False)
