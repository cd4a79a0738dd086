"""Mosaic atlas, host side (include/strata_hip.h, "Mosaic atlas"): the canvas layout and the segment-table builder against
brute-force numpy restatements, the placement arithmetic against `ParcelMosaic`'s, the Philox key rule of a `ParcelSet`, the
argument checks of every new entry point (they answer before any device work: every call below fails a check) and the workspace
macro through a C compiler.  No device."""
import ctypes
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from conftest import ROOT
from stratanet2_vegetation_coverage_maps_amd import _lib, parcel
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
from stratanet2_vegetation_coverage_maps_amd.inference import AtlasReport, MosaicAtlas, ParcelMosaic
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args

COLS, SEG = _lib.SN2_ATLAS_CANVAS_COLS, _lib.SN2_ATLAS_SEG_COLS
EINVAL, ELIMIT = _lib.SN2_EINVAL, _lib.SN2_ELIMIT
FAKE = 0x1000                                                # a "device pointer" that is never dereferenced
SHAPES = [(8, 8), (13, 21), (9, 70), (1, 1), (2100, 1), (40, 300), (700, 700)]


def table_by_hand(shapes, geo=None):
    """the canvas table restated: prefixes by a python loop"""
    K = len(shapes)
    t = np.zeros((K + 1, COLS), dtype=np.int64)
    base = fin = crop = 0
    for k, (H, W) in enumerate(shapes):
        g = np.array(geo[k] if geo is not None else (0.0, 0.0), dtype=np.float64).view(np.int64)
        t[k] = [base, H, W, fin, crop, g[0], g[1], 0]
        base += H * W
        fin += min((H * W + 255) // 256, 1024)
        crop += min(H * ((W + 255) // 256), 2048)
    t[K, 0], t[K, 3], t[K, 4] = base, fin, crop
    return t


def test_canvas_table_is_the_layout_the_header_states():
    geo = [(650000.5 + 1000 * k, 6860000.25 - 3 * k) for k in range(len(SHAPES))]
    H, W = [s[0] for s in SHAPES], [s[1] for s in SHAPES]
    t = ops.atlas_canvas_table(H, W, [g[0] for g in geo], [g[1] for g in geo])
    assert t.dtype == np.int64 and t.shape == (len(SHAPES) + 1, COLS) and np.array_equal(t, table_by_hand(SHAPES, geo))
    assert np.array_equal(ops.atlas_canvas_table(H, W), table_by_hand(SHAPES))
    assert t[4, 4] - t[3, 4] == 1 and t[5, 4] - t[4, 4] == 2048 and t[7, 3] - t[6, 3] == 1024     # the caps of both partitions
    # canvas k is a zero-copy, canvas-major (C,H,W) view of a C-band arena
    tab = ops.AtlasTable(H, W, [g[0] for g in geo], [g[1] for g in geo])
    assert tab.K == len(SHAPES) and tab.pixels == sum(h * w for h, w in SHAPES) and tab.dev is None
    for C in (3, 5):
        arena = torch.arange(C * tab.pixels, dtype=torch.float32)
        for k, (h, w) in enumerate(SHAPES):
            v = tab.view(arena, C, k)
            assert v.shape == (C, h, w) and v.data_ptr() == arena.data_ptr() + 4 * C * tab.base(k) and v.is_contiguous()
            assert v[C - 1, h - 1, w - 1] == C * (tab.base(k) + h * w) - 1
            assert tab.shape(k) == (h, w) and tab.geo(k) == geo[k]
    for bad in (dict(H=[8, 0], W=[8, 8]), dict(H=[8, 8], W=[-1, 8]), dict(H=[], W=[]), dict(H=[4], W=[4], x_min=[np.nan], y_max=[0.0]),
                dict(H=[4], W=[4], x_min=[0.0], y_max=[np.inf])):
        with pytest.raises(ops.StrataHipError, match="SN2_EINVAL"):
            ops.atlas_canvas_table(**bad)
    with pytest.raises(ops.StrataHipError, match="SN2_ELIMIT"):
        ops.atlas_canvas_table([8, 46341], [8, 46341])
    assert ops.atlas_canvas_table([46340], [46340])[1, 0] == 46340 ** 2


def segments_by_hand(place, D, shapes):
    """the segment table restated: one python loop over the plots, the window as the union of the plots' pixels inside the canvas"""
    rows = []
    for b, (c, y, x) in enumerate(place):
        if not rows or rows[-1]["c"] != c:
            rows.append(dict(c=c, first=b, end=b + 1, ys=set(), xs=set()))
        r = rows[-1]
        r["end"] = b + 1
        r["ys"].update((y, y + D - 1))
        r["xs"].update((x, x + D - 1))
    out, wg = [], 0
    for r in rows:
        H, W = shapes[r["c"]]
        y0, y1, x0, x1 = max(min(r["ys"]), 0), min(max(r["ys"]) + 1, H), max(min(r["xs"]), 0), min(max(r["xs"]) + 1, W)
        if y1 <= y0 or x1 <= x0:
            y0 = x0 = h = w = 0
        else:
            h, w = y1 - y0, x1 - x0
        out.append([r["c"], r["first"], r["end"], y0, x0, h, w, wg])
        wg += ((w + 63) // 64) * ((h + 3) // 4)
    out.append([0] * 7 + [wg])
    return np.array(out, dtype=np.int32)


@pytest.mark.parametrize("name,place", [
    ("runs of length one", [(0, 0, 0), (1, 2, 3), (2, 0, 31), (4, 100, 0)]),
    ("a canvas absent from the batch", [(0, 0, 0), (0, 0, 0), (2, 1, 5), (2, 1, 62), (2, 0, 33)]),
    ("windows hanging over every edge", [(1, -3, -2), (1, 9, 17), (2, 5, 66), (2, -7, 0), (5, 35, 290)]),
    ("a run wholly outside its canvas, between two that are not", [(0, 0, 0), (1, 13, 0), (1, 14, 4), (2, 1, 1)]),
    ("one plot of a run outside its canvas", [(0, 0, 0), (1, 13, 0), (1, -8, 4), (2, 1, 1)]),
    ("one run", [(5, 3, 4), (5, 30, 280), (5, 3, 4)]),
    ("more than one tile each way", [(6, 0, 0), (6, 600, 650), (6, 300, 300)]),
])
def test_segment_table_against_the_restatement(name, place):
    D = 8
    t = table_by_hand(SHAPES)
    got = ops.atlas_segments(np.array(place), D, t)
    want = segments_by_hand(place, D, SHAPES)
    assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), name
    S = len(got) - 1
    assert (np.diff(got[:S, 0]) > 0).all() and got[0, 1] == 0 and got[S - 1, 2] == len(place) and np.array_equal(got[1:S, 1], got[:S - 1, 2])
    inside = (got[:S, 3] + got[:S, 5] <= t[got[:S, 0], 1]) & (got[:S, 4] + got[:S, 6] <= t[got[:S, 0], 2])
    assert inside.all() and (got[:S, 3:7] >= 0).all()                 # what sn2_atlas_merge insists on before it launches


def test_segment_cases_are_what_their_names_say():
    t = table_by_hand(SHAPES)
    seg = ops.atlas_segments(np.array([(0, 0, 0), (1, 13, 0), (1, -8, 4), (2, 1, 1)]), 8, t)
    assert seg[1].tolist() == [1, 1, 3, 0, 0, 13, 12, 2]              # rows -8 .. 20 clipped to 0 .. 12; 4 tiles of 4 rows
    seg = ops.atlas_segments(np.array([(0, 0, 0), (1, 13, 0), (1, 14, 4), (2, 1, 1)]), 8, t)
    assert seg[1].tolist() == [1, 1, 3, 0, 0, 0, 0, 2] and seg[2, 7] == 2 and seg[3, 7] == 2 + 2      # nothing left of the run: no workgroup
    seg = ops.atlas_segments(np.array([(6, 0, 0), (6, 600, 650)]), 8, t)
    assert seg[0, 3:7].tolist() == [0, 0, 608, 658] and seg[1, 7] == 11 * 152


def test_decreasing_canvas_order_raises():
    t = table_by_hand(SHAPES)
    with pytest.raises(ValueError, match="non-decreasing"):
        ops.atlas_segments(np.array([(0, 0, 0), (2, 0, 0), (1, 0, 0)]), 8, t)
    with pytest.raises(ValueError, match="non-decreasing"):
        ops.atlas_segments(np.array([(1, 0, 0), (0, 0, 0)]), 8, t)
    for bad in ([(-1, 0, 0)], [(0, 0, 0), (len(SHAPES), 0, 0)]):
        with pytest.raises(ValueError, match="canvas index"):
            ops.atlas_segments(np.array(bad), 8, t)
    with pytest.raises(ValueError):
        ops.atlas_segments(np.zeros((0, 3), dtype=np.int32), 8, t)
    ops.atlas_segments(np.array([(0, 0, 0), (0, 0, 0), (3, 0, 0)]), 8, t)         # equal neighbours are in order


def _cpu_set(counts):
    """a ParcelSet of the given plots per parcel, with nothing behind it but the bookkeeping"""
    P = sum(counts)
    return parcel.ParcelSet(torch.empty(10, 0), torch.zeros(P + 1, dtype=torch.int32), torch.empty(0, dtype=torch.int32),
                            torch.zeros(P, 2), np.full(P, 60, dtype=np.int64), np.arange(P), ["p"] * P, np.zeros((P, 2), dtype=np.float32),
                            np.repeat(np.arange(len(counts)), counts), np.concatenate([[0], np.cumsum(counts)]))


def test_plot_keys_of_a_set_and_of_a_parcel_alone():
    s = _cpu_set([3, 0, 2, 1])
    assert s.n_parcels == 4 and len(s) == 6
    want = [(0 << 32) + 0, (0 << 32) + 1, (0 << 32) + 2, (2 << 32) + 0, (2 << 32) + 1, (3 << 32) + 0]
    keys = s.plot_keys()
    assert keys.dtype == np.int64 and keys.tolist() == want
    alone = parcel.ParcelPlots(*[getattr(s, f) for f in list(parcel.ParcelPlots.__dataclass_fields__)])
    assert alone.plot_keys().tolist() == list(range(6))                        # the default: the keys the package has always used
    assert alone.plot_keys(2 << 32)[:2].tolist() == want[3:5]                  # a parcel alone with the keys it has in the set
    big = _cpu_set([1] * 3 + [2])
    assert big.plot_keys()[-1] == (3 << 32) + 1 and big.plot_keys(1 << 40)[0] == 1 << 40
    for fn in (parcel.ParcelPlots.batches, parcel.predict_parcel_cloud):
        assert inspect.signature(fn).parameters["key_base"].default == 0
    sig = inspect.signature(parcel.predict_parcels).parameters
    assert (sig["batch_size"].default, sig["sampler"].default, sig["prefetch"].default, sig["n_live"].default) == (512, "device", 3, True)


def test_atlas_places_plots_as_each_parcel_mosaic_does():
    a = make_args()
    rng = np.random.default_rng(0)
    centres = [(650000 + 1000 * k + rng.random((n, 2)) * (90, 70) + (0, 6860000)).astype(np.float32) for k, n in enumerate((7, 0, 12, 1))]
    s = _cpu_set([len(c) for c in centres])
    s.centers_host = np.concatenate(centres)
    atlas = MosaicAtlas.for_plots(s, a, device="cpu")
    assert atlas.K == 4 and atlas.empty == [False, True, False, False] and atlas.mosaic(1) is None
    assert torch.isnan(atlas.mean).all() and atlas.mean.numel() == 3 * atlas.table.pixels == atlas.wsum.numel()
    place = atlas.offsets(s.centers_host, s.parcel_of)
    assert place.dtype == np.int32 and place.shape == (20, 3) and np.array_equal(place[:, 0], s.parcel_of)
    for k, c in enumerate(centres):
        if len(c) == 0:
            assert atlas.table.shape(k) == (1, 1)
            continue
        m = parcel.parcel_mosaic(c, a, "cpu")
        assert isinstance(m, ParcelMosaic) and atlas.table.shape(k) == tuple(m.mean.shape[1:]) and atlas.table.geo(k) == (m.x_min, m.y_max)
        assert np.array_equal(place[s.parcel_start[k]:s.parcel_start[k + 1], 1:], m.offsets(c).numpy())
        mean, wsum = atlas.mosaic(k)
        assert mean.shape == m.mean.shape and wsum.shape == m.wsum.shape
        assert mean.data_ptr() == atlas.mean.data_ptr() + 12 * atlas.table.base(k)
    assert set(AtlasReport.__dataclass_fields__) >= {"thresholds", "band_means", "band_counts"}


def test_header_binding_and_exports_agree():
    import stratanet2_vegetation_coverage_maps_amd as pkg
    txt = open(os.path.join(ROOT, "include", "strata_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("sn2_atlas_canvas_table", "sn2_atlas_finalize_ws_words", "sn2_atlas_merge", "sn2_atlas_finalize", "sn2_atlas_crop_stats"):
        assert re.search(r"^int\s+%s\s*\(" % name, txt, flags=re.M) and name in _lib.SIGNATURES and hasattr(raw, name)
    for name in ("ParcelSet", "prepare_parcels", "predict_parcels", "MosaicAtlas", "AtlasReport"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    from stratanet2_vegetation_coverage_maps_amd import _build
    assert "atlas.hip" in _build.SOURCES and "mosaic_rules.h" in _build.HEADERS


def test_workspace_macros_match_the_library_and_the_binding():
    Ks = [1, 4, 16, 1000, 2 ** 20]
    src = '#include <stdio.h>\n#include "strata_hip.h"\nint main(){\n' + "".join(
        f'printf("%zu\\n", (size_t)SN2_ATLAS_FINALIZE_WS_WORDS({k}));\n' for k in Ks) + "".join(
        f'printf("%zu %zu\\n", (size_t)SN2_ATLAS_FINALIZE_BLOCKS({h},{w}), (size_t)SN2_MOSAIC_CROP_BLOCKS({h},{w}));\n' for h, w in SHAPES) + (
        'printf("%d %d %d %d\\n", SN2_ATLAS_CANVAS_COLS, SN2_ATLAS_SEG_COLS, SN2_ATLAS_FINALIZE_MAX_BLOCKS, SN2_ATLAS_FINALIZE_CANVAS_WORDS);'
        'return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got[:len(Ks)] == [ops.atlas_finalize_ws_words(k) for k in Ks] == [k * (10004 + 2048) for k in Ks]
    blocks = np.array(got[len(Ks):-4]).reshape(-1, 2)
    t = ops.atlas_canvas_table([s[0] for s in SHAPES], [s[1] for s in SHAPES])
    assert np.array_equal(np.diff(t[:, 3]), blocks[:, 0]) and np.array_equal(np.diff(t[:, 4]), blocks[:, 1])
    assert got[-4:] == [COLS, SEG, _lib.SN2_ATLAS_FINALIZE_MAX_BLOCKS, _lib.SN2_ATLAS_FINALIZE_CANVAS_WORDS] == [8, 8, 1024, 12052]
    lib = _lib.load()
    words = ctypes.c_size_t()
    assert lib.sn2_atlas_finalize_ws_words(0, ctypes.byref(words)) == EINVAL and lib.sn2_atlas_finalize_ws_words(3, None) == EINVAL


def _bad_tables():
    """(a canvas table that no entry point may take, the answer)"""
    good = table_by_hand([(8, 8), (13, 21), (9, 70)])
    out = []
    for (r, c, v), rc in [((1, 1, 0), EINVAL), ((1, 2, -21), EINVAL), ((0, 1, 0), EINVAL),          # H or W <= 0
                          ((1, 0, 63), EINVAL), ((2, 0, 338), EINVAL), ((3, 0, 900), EINVAL),       # base is not the prefix
                          ((2, 3, 1), EINVAL), ((3, 4, 20), EINVAL), ((0, 7, 1), EINVAL), ((3, 1, 5), EINVAL),
                          ((1, 5, np.array(np.nan).view(np.int64)), EINVAL), ((2, 6, np.array(np.inf).view(np.int64)), EINVAL)]:
        t = good.copy()
        t[r, c] = v
        out.append((t, rc))
    t = good.copy()
    t[1, 1:3] = 46341                                                                              # H W >= 2^31
    out.append((t, ELIMIT))
    t = good.copy()
    t[1, 1:3] = (2 ** 31 - 1, 2)
    out.append((t, ELIMIT))
    return good, out


def test_argument_checks_return_before_any_device_work():
    """every call fails a check: nothing is launched, no fake pointer is read"""
    lib = _lib.load()
    good, bad = _bad_tables()
    K = 3
    p = lambda a: a.ctypes.data
    place = np.array([(0, 0, 0), (1, 2, 3), (1, 4, 5), (2, 1, 60)], dtype=np.int32)
    seg = np.ascontiguousarray(ops.atlas_segments(place, 8, good))
    S = len(seg) - 1
    start = np.array([0, 4, 4, 9], dtype=np.int32)

    def merge(**kw):
        a = dict(rasters=FAKE, weights=FAKE, place=FAKE, B=4, D=8, K=K, ch=p(good), cd=FAKE, sh=p(seg), sd=FAKE, S=S, mean=FAKE, wsum=FAKE,
                 stream=None)
        return lib.sn2_atlas_merge(*{**a, **kw}.values())

    def finalize(**kw):
        a = dict(mean=FAKE, wsum=FAKE, K=K, ch=p(good), cd=FAKE, ws=FAKE, thr=FAKE, bands=FAKE, stream=None)
        return lib.sn2_atlas_finalize(*{**a, **kw}.values())

    def crop(**kw):
        a = dict(bands=FAKE, C=5, K=K, ch=p(good), cd=FAKE, pix=0.625, edges=FAKE, eh=p(start), ed=FAKE, ws=FAKE, mean=FAKE, count=FAKE,
                 stream=None)
        return lib.sn2_atlas_crop_stats(*{**a, **kw}.values())

    for fn, ptrs in ((merge, ("rasters", "weights", "place", "ch", "cd", "sh", "sd", "mean", "wsum")),
                     (finalize, ("mean", "wsum", "ch", "cd", "ws", "thr", "bands")),
                     (crop, ("bands", "ch", "cd", "edges", "eh", "ed", "ws", "mean", "count"))):
        for name in ptrs:
            assert fn(**{name: None}) == EINVAL, (fn.__name__, name)
        for k in (0, -1):
            assert fn(K=k) == EINVAL, (fn.__name__, k)
        for t, rc in bad:
            assert fn(ch=p(t)) == rc, (fn.__name__, t.tolist())
        assert fn(K=2) == EINVAL                                       # the table of three canvases is not one of two

    # the merge's runs
    for kw in (dict(B=0), dict(D=0), dict(S=0), dict(S=5), dict(B=5), dict(B=3)):
        assert merge(**kw) == EINVAL, kw
    for (r, c, v) in [(1, 0, 0), (2, 0, 1), (2, 0, 3), (0, 1, 1), (1, 1, 2), (1, 2, 1), (2, 2, 5), (0, 3, -1), (0, 5, 9), (1, 4, 20), (1, 6, 22),
                      (2, 5, -1), (1, 7, 3), (3, 7, 0)]:
        s = seg.copy()
        s[r, c] = v
        assert merge(sh=p(s)) == EINVAL, (r, c, v)
    # the finalisation's and the crop's workspaces must be 8-byte aligned
    assert finalize(ws=FAKE + 4) == EINVAL and crop(ws=FAKE + 4) == EINVAL
    # the crop: limits per canvas as the single-canvas call's
    nan, inf = float("nan"), float("inf")
    for kw in (dict(C=0), dict(pix=0.0), dict(pix=-1.0), dict(pix=nan), dict(pix=inf)):
        assert crop(**kw) == EINVAL, kw
    for st in ([1, 4, 4, 9], [0, 2, 2, 9], [0, 4, 3, 9], [0, 4, 4, 5], [0, -1, 4, 9]):                 # a ring has three edges or more
        assert crop(eh=p(np.array(st, dtype=np.int32))) == EINVAL, st
    assert crop(eh=p(np.zeros(4, dtype=np.int32))) == EINVAL                                            # no edge at all, but edges given
    assert crop(C=9) == ELIMIT
    assert crop(eh=p(np.array([0, 4, 4 + 2 ** 20 + 1, 9 + 2 ** 20 + 1], dtype=np.int32))) == ELIMIT
