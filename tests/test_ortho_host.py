"""Orthoimage colours, host side (CPU only): the numpy statement of the rule against answers worked out by hand and against
deliberately wrong restatements, the C ABI's argument checks on fake pointers, header / binding / exports, the wrappers'
refusals, and `ortho.open` on files written into tmp_path."""
import ctypes
import os
import re

import numpy as np
import pytest

import _ortho_cases as oc
from conftest import ROOT


def _set(name, dtype="uint8", layout="chunky"):
    from stratanet2_vegetation_coverage_maps_amd import ortho
    images, nodata, origin = oc.case_images(name, dtype, layout)
    return ortho.OrthoSet([ortho.OrthoImage(p, x0, y0, px, py, layout=layout) for p, x0, y0, px, py in images], nodata=nodata), origin


def test_colorize_ref_gives_the_answers_worked_out_by_hand():
    from stratanet2_vegetation_coverage_maps_amd import ortho
    vals, _ = oc.case_values("overlap_nodata")
    classes = {}
    for dtype in oc.DTYPES:
        for layout in oc.LAYOUTS:
            oset, _ = _set("overlap_nodata", dtype, layout)
            cloud = np.full((10, len(oc.HAND)), -7.0, dtype=np.float32)
            cloud[0], cloud[1] = [h[0] for h in oc.HAND], [h[1] for h in oc.HAND]
            res = ortho.colorize_ref(cloud, oset, bands=(2, 0), rows=(6, 3), scale=oc.SCALE[dtype], covered=True)
            want_missing = 0
            for i, (x, y, served, pixel, cls) in enumerate(oc.HAND):
                classes[cls] = classes.get(cls, 0) + 1
                assert res.covered[i] == served, (dtype, layout, i)
                if served == 0:
                    want_missing += 1
                    assert (res.cloud[2:, i] == -7.0).all(), i                     # an unserved point keeps what it had
                    continue
                v = vals[served - 1][4][pixel[0], pixel[1]].astype(np.float64) + (0.25 if dtype == "float32" else 0.0)
                assert res.cloud[6, i] == np.float32(v[2]) * np.float32(oc.SCALE[dtype]), (dtype, layout, i)
                assert res.cloud[3, i] == np.float32(v[0]) * np.float32(oc.SCALE[dtype]), (dtype, layout, i)
                assert (res.cloud[[2, 4, 5, 7, 8, 9], i] == -7.0).all()
            assert res.missing == want_missing
            assert np.array_equal(res.cloud[:2].view(np.uint32), cloud[:2].view(np.uint32))      # rows 0 and 1 are only read
            assert (cloud[2:] == -7.0).all()                                                     # and the input is not touched
    assert set(classes) == {"first", "second", "nodata_both", "outside"} and min(classes.values()) >= 6 * 2


def test_default_scales_and_the_infrared_call():
    from stratanet2_vegetation_coverage_maps_amd import ortho
    px = np.array([[[7, 8, 9]]], dtype=np.uint8)
    cloud = np.zeros((10, 1), dtype=np.float32)
    cloud[0], cloud[1] = 0.5, 0.5
    r = ortho.colorize_ref(cloud, ortho.OrthoImage(px, 0.0, 1.0, 1.0))
    assert r.cloud[3:7, 0].tolist() == [7 * 256.0, 8 * 256.0, 9 * 256.0, 0.0] and r.missing == 0 and r.covered is None
    r = ortho.colorize_ref(r.cloud, ortho.OrthoImage(px.astype(np.uint16) * 300, 0.0, 1.0, 1.0), bands=(0,), rows=(6,))
    assert r.cloud[3:7, 0].tolist() == [7 * 256.0, 8 * 256.0, 9 * 256.0, 2100.0]
    with pytest.raises(ValueError):
        ortho.colorize_ref(cloud, ortho.OrthoImage(px.astype(np.float32), 0.0, 1.0, 1.0))        # float32: scale must be given


# ---- the rule restated point by point, with one switch per deliberate mistake ------------------------------------------------------
def _restated(cloud, images, nodata, bands, rows, scale, wrong=None):
    out = cloud.copy()
    cov = np.zeros(cloud.shape[1], dtype=np.uint8)
    order = list(enumerate(images))
    for i in range(cloud.shape[1]):
        x, y = np.float64(cloud[0, i]), np.float64(cloud[1, i])
        for s, (pix, x0, y0, px, py) in order:
            H, W = pix.shape[:2]
            with np.errstate(all="ignore"):
                if wrong == "fp32":
                    u = np.float64((np.float32(x) - np.float32(x0)) / np.float32(px))
                    v = np.float64((np.float32(y0) - np.float32(y)) / np.float32(py))
                else:
                    u = (x - np.float64(x0)) / np.float64(px)
                    v = (np.float64(y0) - y) / np.float64(py)
                if wrong == "no_flip":
                    v = (y - (np.float64(y0) - H * np.float64(py))) / np.float64(py)
            far = (u <= W and v <= H) if wrong == "far_edge" else (u < W and v < H)
            if not (u >= 0 and v >= 0 and far):
                continue
            col, row = (int(np.round(u)), int(np.round(v))) if wrong == "round" else (int(np.floor(u)), int(np.floor(v)))
            col, row = min(col, W - 1), min(row, H - 1)
            q = [pix[row, col, b] for b in bands]
            if nodata is not None and wrong != "nodata_ignored" and all(np.float64(t) == nodata for t in q):
                continue
            for r, t in zip(rows, q):
                out[r, i] = np.float32(t) * np.float32(scale)
            cov[i] = s + 1
            if wrong != "last_wins":
                break
    return out, cov


def test_wrong_restatements_differ_on_the_planted_points():
    """The restatement equals colorize_ref on every case; each deliberate mistake differs from it on at least one planted point."""
    from stratanet2_vegetation_coverage_maps_amd import ortho
    mistakes = ("round", "no_flip", "far_edge", "fp32", "nodata_ignored", "last_wins")
    differs = {m: [] for m in mistakes}
    for name in oc.CASE_NAMES:
        images, nodata, origin = oc.case_images(name, "uint16", "chunky")
        oset, _ = _set(name, "uint16", "chunky")
        xy = oc.case_points(name)
        cloud = oc.cloud_of(xy, xy.shape[1], seed=3)
        bands, rows = oc.case_map(name)
        ref = ortho.colorize_ref(cloud, oset, bands=bands, rows=rows, scale=3.0, origin=origin, covered=True)
        ox, oy = origin if origin is not None else (0.0, 0.0)
        frame = [(p, float(np.float64(x0) - np.float64(ox)), float(np.float64(y0) - np.float64(oy)), px, py) for p, x0, y0, px, py in images]
        got, cov = _restated(cloud, frame, nodata, bands, rows, 3.0)
        assert np.array_equal(got.view(np.uint32), ref.cloud.view(np.uint32)) and np.array_equal(cov, ref.covered), name
        assert 0 < ref.missing < cloud.shape[1], name
        for m in mistakes:
            bad, bad_cov = _restated(cloud, frame, nodata, bands, rows, 3.0, wrong=m)
            if not (np.array_equal(bad.view(np.uint32), ref.cloud.view(np.uint32)) and np.array_equal(bad_cov, ref.covered)):
                differs[m].append(name)
    assert all(differs[m] for m in mistakes), differs
    assert "lambert" in differs["fp32"] and "overlap_nodata" in differs["nodata_ignored"] and "overlap_nodata" in differs["last_wins"]
    assert "rgb_half" in differs["round"] and "rgb_half" in differs["no_flip"] and "rgb_half" in differs["far_edge"]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
_FAKE = 0x1000                        # never dereferenced: every refused call fails a check first, every accepted one has T = 0


def _good():
    from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
    return ops.ortho_set_struct([(_FAKE, 650000.0, 6800000.0, 0.2, 0.25, 4, 4), (_FAKE, 650001.0, 6800000.0, 0.2, 0.25, 4, 4)],
                                "uint8", 3, "chunky", (0, 1, 2), (3, 4, 5), 256.0)


def test_argument_checks_return_before_any_device_work():
    """One defect at a time; the set is accepted (T = 0: checked, nothing launched) without its defect."""
    from stratanet2_vegetation_coverage_maps_amd import _lib
    lib = _lib.load()

    def call(s, cloud=_FAKE, stride=100, col0=0, T=0, missing=_FAKE):
        return lib.sn2_ortho_colorize(cloud, stride, col0, T, ctypes.byref(s) if s is not None else None, None, missing, None)
    assert call(_good()) == 0
    assert call(None) == -1
    nan, inf = float("nan"), float("inf")
    big = 2 ** 31 - 1
    defects = [("S", 0), ("S", 33), ("C", 0), ("dtype", 3), ("dtype", -1), ("layout", 2), ("n_map", 0), ("n_map", 5),
               ("band", (0, 1, 3, 0)), ("band", (-1, 1, 2, 0)), ("row", (0, 4, 5, 0)), ("row", (3, 1, 5, 0)), ("row", (3, 4, 2, 0)),
               ("row", (3, 4, 10, 0)), ("row", (3, 4, 3, 0)), ("scale", inf), ("scale", nan)]
    for field, value in defects:
        s = _good()
        setattr(s, field, type(getattr(s, field))(*value) if isinstance(value, tuple) else value)
        assert call(s) == -1, (field, value)
    s = _good()
    s.has_nodata, s.nodata = 1, nan
    assert call(s) == -1
    s.nodata = 0.0
    assert call(s) == 0
    for k in (0, 1):
        for field, value in (("x0", nan), ("y0", inf), ("px", 0.0), ("px", inf), ("py", -0.2), ("py", nan), ("W", 0), ("H", 0), ("pixels", None)):
            s = _good()
            setattr(s.image[k], field, value)
            assert call(s) == -1, (k, field, value)
    for W, H, want in ((1 << 20, 1 << 19, -2), (big, big, -2), (1 << 19, 1 << 19, 0)):      # 3 W H against 2^40 samples
        s = _good()
        s.image[1].W, s.image[1].H = W, H
        assert call(s) == want, (W, H)
    s = _good()
    s.S = 1                                                                                    # image[1] is then not looked at
    s.image[1].px = nan
    assert call(s) == 0
    s = _good()
    s.n_map, s.row[0] = 1, 9
    assert call(s) == 0
    # the launch: T = 0 is a no-op that still checks; nothing below reaches a launch
    assert call(_good(), col0=100) == 0 and call(_good(), col0=101) == -1 and call(_good(), col0=-1) == -1 and call(_good(), T=-1) == -1
    assert call(_good(), cloud=None) == -1 and call(_good(), missing=None) == -1 and call(_good(), stride=-1) == -1
    assert call(_good(), col0=3, T=98) == -1 and call(_good(), stride=2 ** 32, T=2 ** 31) == -2
    assert call(_good(), stride=2 ** 63 - 1, col0=2 ** 63 - 2, T=2) == -1


def test_header_binding_and_exports_agree():
    from stratanet2_vegetation_coverage_maps_amd import _lib
    txt = open(os.path.join(ROOT, "include", "strata_hip.h")).read()
    assert "Orthoimage colours" in txt
    assert re.search(r"^int\s+sn2_ortho_colorize\s*\(", txt, flags=re.M)
    assert _lib.SIGNATURES["sn2_ortho_colorize"] == [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.POINTER(_lib.OrthoSet),
                                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "sn2_ortho_colorize")
    import subprocess
    src = ('#include <stdio.h>\n#include "strata_hip.h"\nint main(){printf("%zu %zu %d %d %lld\\n",sizeof(sn2_ortho_image),sizeof(sn2_ortho_set),'
           'SN2_ORTHO_MAX_IMAGES,SN2_ORTHO_MAX_MAP,(long long)SN2_ORTHO_MAX_SAMPLES);return 0;}\n')
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got == [ctypes.sizeof(_lib.OrthoImage), ctypes.sizeof(_lib.OrthoSet), _lib.SN2_ORTHO_MAX_IMAGES, _lib.SN2_ORTHO_MAX_MAP,
                   _lib.SN2_ORTHO_MAX_SAMPLES]
    assert _lib.OrthoSet.image.offset == 72 and _lib.OrthoSet.nodata.offset == 56


def test_wrappers_refuse_before_the_library():
    import torch
    from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
    from stratanet2_vegetation_coverage_maps_amd import OrthoImage, OrthoSet, ortho
    rgb = np.ones((2, 2, 3), dtype=np.uint8)
    for bad in (rgb.astype(np.int16), rgb.astype(np.float64), rgb.astype(np.int32), torch.ones(2, 2, 3, dtype=torch.int16)):
        with pytest.raises(ValueError):
            OrthoImage(bad, 0.0, 2.0, 1.0)
    for geo in ((float("nan"), 2.0, 1.0), (0.0, 2.0, 0.0), (0.0, 2.0, -1.0), (0.0, float("inf"), 1.0)):
        with pytest.raises(ValueError):
            OrthoImage(rgb, *geo)
    with pytest.raises(ValueError):
        OrthoImage(rgb, 0.0, 2.0, 1.0, layout="tiled")
    im = OrthoImage(rgb, 0.0, 2.0, 1.0)
    assert (im.H, im.W, im.C, im.pix_y) == (2, 2, 3, 1.0) and OrthoImage(rgb, 0, 2, 1, layout="planar").C == 2
    assert OrthoSet([im] * 32).C == 3
    with pytest.raises(ValueError):
        OrthoSet([im] * 33)
    with pytest.raises(ValueError):
        OrthoSet([])
    with pytest.raises(ValueError):
        OrthoSet([im, OrthoImage(rgb.astype(np.uint16), 0.0, 2.0, 1.0)])                  # two pixel types
    with pytest.raises(ValueError):
        OrthoSet([im, OrthoImage(rgb[:, :, :1].copy(), 0.0, 2.0, 1.0)])                   # two band counts
    with pytest.raises(ValueError):
        OrthoSet([im, OrthoImage(np.ones((3, 2, 2), dtype=np.uint8), 0.0, 2.0, 1.0, layout="planar")])
    with pytest.raises(ValueError):
        OrthoSet([im], nodata=float("nan"))
    cloud = np.zeros((10, 3), dtype=np.float32)
    for kw in (dict(rows=(0, 4, 5)), dict(rows=(3, 1, 5)), dict(rows=(3, 4, 4)), dict(rows=(3, 4, 10)), dict(rows=(3, 4)), dict(bands=(0, 1, 3)),
               dict(bands=(0, 1, 2, 0, 1), rows=(3, 4, 5, 6, 7)), dict(bands=(), rows=()), dict(scale=float("inf"))):
        with pytest.raises(ValueError):
            ortho.colorize_ref(cloud, im, **kw)
        with pytest.raises(ValueError):
            ortho.colorize(torch.zeros(10, 3), im, **kw)
    with pytest.raises(ValueError):
        ortho.colorize(torch.zeros(10, 3), im)                                            # not on the device
    entry = (_FAKE, 0.0, 2.0, 1.0, 1.0, 2, 2)
    for args in (([entry] * 33, "uint8", 3, "chunky", (0,), (3,), 1.0), ([entry], "int16", 3, "chunky", (0,), (3,), 1.0),
                 ([entry], "uint8", 3, "tiled", (0,), (3,), 1.0), ([entry], "uint8", 3, "chunky", (0,), (1,), 1.0),
                 ([entry], "uint8", 3, "chunky", (0, 1), (3, 3), 1.0), ([], "uint8", 3, "chunky", (0,), (3,), 1.0)):
        with pytest.raises(ValueError):
            ops.ortho_set_struct(*args)
    s = ops.ortho_set_struct([entry] * 32, "uint16", 3, "planar", (2, 0), (6, 9), 1.0, nodata=0)
    assert (s.S, s.dtype, s.layout, s.n_map, s.has_nodata, list(s.band)[:2], list(s.row)[:2]) == (32, 1, 1, 2, 1, [2, 0], [6, 9])
    sh = OrthoSet([OrthoImage(rgb, 650000.03, 6800000.3, 0.2)]).shifted((650000.0, 6799990.0, 12.0)).images[0]
    assert (sh.x_min, sh.y_max) == (650000.03 - 650000.0, 6800000.3 - 6799990.0) and sh.pixels is rgb


# ---- files ---------------------------------------------------------------------------------------------------------------------------
def _world_file(path, px, py, x_min, y_max):
    with open(path, "w") as f:
        f.write(f"{px!r}\n0.0\n0.0\n{-py!r}\n{x_min + px / 2!r}\n{y_max - py / 2!r}\n")


@pytest.mark.parametrize("compression", [None, "tiff_adobe_deflate", "tiff_lzw"])
@pytest.mark.parametrize("mode", ["RGB", "I;16"])
def test_open_reads_tiffs_with_a_world_file(tmp_path, compression, mode):
    from PIL import Image
    from stratanet2_vegetation_coverage_maps_amd import ortho
    rng = np.random.default_rng(5)
    pix = rng.integers(0, 256, size=(5, 4, 3), dtype=np.uint8) if mode == "RGB" else rng.integers(0, 65536, size=(5, 4), dtype=np.uint16)
    path = tmp_path / "slab.tif"
    Image.fromarray(pix).save(path, compression=compression)
    _world_file(tmp_path / "slab.tfw", 0.5, 0.25, 650000.0, 6800000.5)
    im = ortho.open(path)
    assert (im.dtype, im.layout, im.H, im.W, im.C) == (str(pix.dtype), "chunky", 5, 4, 3 if mode == "RGB" else 1)
    assert np.array_equal(im.host().reshape(pix.shape), pix)
    assert (im.x_min, im.y_max, im.pix_x, im.pix_y) == (650000.0, 6800000.5, 0.5, 0.25)
    assert ortho.open(path, georef=(1.0, 2.0, 3.0, 4.0)).x_min == 1.0                      # georef= comes first


def test_open_reads_the_geotiff_tags_and_refuses_what_it_cannot_place(tmp_path):
    from PIL import Image, TiffImagePlugin
    from stratanet2_vegetation_coverage_maps_amd import geotiff, ortho
    # the package's own writer: tags 33550 / 33922, PixelIsArea, float32 samples
    band = np.arange(12, dtype=np.float32).reshape(1, 3, 4) + np.float32(0.5)
    path = tmp_path / "map.tif"
    path.write_bytes(geotiff.assemble(band.view(np.uint8), 1, 3, 4, 650000.25, 6800000.75, 0.5, compress=None))
    im = ortho.open(path)
    assert (im.dtype, im.H, im.W, im.C) == ("float32", 3, 4, 1) and np.array_equal(im.host()[:, :, 0], band[0])
    assert (im.x_min, im.y_max, im.pix_x, im.pix_y) == (650000.25, 6800000.75, 0.5, 0.5)
    # PIL's writer with the two tags, a tie point that is not at pixel (0, 0), and PixelIsPoint: the corner moves half a pixel
    rgb = np.arange(24, dtype=np.uint8).reshape(2, 4, 3)
    for raster_type, half in ((1, 0.0), (2, 0.5)):
        ifd = TiffImagePlugin.ImageFileDirectory_v2()
        ifd[33550] = (0.2, 0.4, 0.0)
        ifd.tagtype[33550] = 12
        ifd[33922] = (1.0, 2.0, 0.0, 100.0, 200.0, 0.0)
        ifd.tagtype[33922] = 12
        ifd[34735] = (1, 1, 0, 1, 1025, 0, 1, raster_type)
        ifd.tagtype[34735] = 3
        p = tmp_path / f"tagged{raster_type}.tif"
        Image.fromarray(rgb).save(p, tiffinfo=ifd)
        im = ortho.open(p)
        assert (im.x_min, im.y_max, im.pix_x, im.pix_y) == (100.0 - (1.0 + half) * 0.2, 200.0 + (2.0 + half) * 0.4, 0.2, 0.4)
        assert np.array_equal(im.host(), rgb)
    # a georeference given as a matrix (tag 34264): the way a GeoTIFF states rotation
    ifd = TiffImagePlugin.ImageFileDirectory_v2()
    ifd[34264] = (0.5, 0.1, 0.0, 100.0, 0.1, -0.5, 0.0, 200.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
    ifd.tagtype[34264] = 12
    Image.fromarray(rgb).save(tmp_path / "matrix.tif", tiffinfo=ifd)
    with pytest.raises(ValueError, match="rotated"):
        ortho.open(tmp_path / "matrix.tif")
    # neither tags nor a world file
    bare = tmp_path / "bare.tif"
    Image.fromarray(rgb).save(bare)
    with pytest.raises(ValueError, match="no georeference"):
        ortho.open(bare)
    assert ortho.open(bare, georef=(0.0, 1.0, 0.5, 0.5)).pix_x == 0.5
    # a rotated world file
    with open(tmp_path / "bare.tfw", "w") as f:
        f.write("0.5\n0.01\n0.01\n-0.5\n10.25\n19.75\n")
    with pytest.raises(ValueError, match="rotated"):
        ortho.open(bare)
    with open(tmp_path / "bare.tfw", "w") as f:
        f.write("0.5\n0\n0\n-0.5\n10.25\n19.75\n")
    im = ortho.open(bare)
    assert (im.x_min, im.y_max) == (10.0, 20.0)
