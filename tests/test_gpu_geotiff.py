"""The GeoTIFF band packer on the device (csrc/tiff_pack.hip, geotiff.py) against the tests' own numpy restatement
(tests/_geotiff_ref.py, pinned without a device by tests/test_geotiff_host.py), bytes against bytes: every canvas of
tests/_geotiff_cases.py in one atlas per band count, in both kernel forms, both layouts and both predictors, with the statistics;
the staging buffer poisoned before, behind and between the blocks; a K-canvas launch against K single-canvas launches; the source
arena unchanged; and a tiny `predict_parcels` through `report`, `write_atlas` and `read`, band 0 opened by libtiff."""
import os

import numpy as np
import pytest
import torch

import _geotiff_cases as GC
import _geotiff_ref as R
from stratanet2_vegetation_coverage_maps_amd import _lib, geotiff
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD, POISON = 256, 0xA5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(canvases, C, layout, predictor, form=0, skip=None):
    """one launch into a poisoned buffer with GUARD bytes on both sides -> (the whole buffer on the host, the packed object, the
    arena's words after the launch)"""
    arena_host = GC.arena_of(canvases)
    arena = torch.from_numpy(arena_host.copy()).to(DEV)
    table = ops.AtlasTable([c.shape[1] for c in canvases], [c.shape[2] for c in canvases], device=DEV)
    lib = _lib.load()
    try:
        assert lib.sn2_debug_tiff_pack_form(form) == 0
        place = ops.tiff_place_table(table.host, C, layout, skip)
        total = int(place[-1, 3])
        buf = torch.full((GUARD + total + GUARD,), POISON, dtype=torch.uint8, device=DEV)
        packed = ops.tiff_pack(arena, C, table, layout, predictor, skip, out=buf[GUARD:GUARD + total])
        torch.cuda.synchronize()
    finally:
        assert lib.sn2_debug_tiff_pack_form(0) == 0
    assert np.array_equal(packed.place, place)
    assert arena.cpu().numpy().view(np.uint32).tobytes() == arena_host.view(np.uint32).tobytes(), "the source arena changed"
    return buf.cpu().numpy(), packed


def first_difference(got, want):
    d = np.flatnonzero(got != want)
    return None if d.size == 0 else (int(d[0]), int(got[d[0]]), int(want[d[0]]), int(d.size))


@pytest.mark.parametrize("form", [0, 1], ids=["rule", "direct"])
@pytest.mark.parametrize("predictor", [1, 3])
@pytest.mark.parametrize("layout", [R.BAND, R.PIXEL], ids=["band", "pixel"])
@pytest.mark.parametrize("C", GC.BANDS)
def test_every_case_in_one_atlas(C, layout, predictor, form):
    """the whole buffer: guard bytes, blocks, the padding between them and the statistics (one canvas has an all-NaN band)"""
    canvases = GC.atlas_canvases(C)
    got, packed = run(canvases, C, layout, predictor, form)
    want = R.expected_buffer(canvases, C, layout, predictor, force_direct=bool(form), poison=POISON, guard=GUARD)
    assert got.shape == want.shape and first_difference(got, want) is None
    packed.read()
    ref = np.stack([R.stats_words(c) for c in canvases])
    assert np.array_equal(packed.counts, ref[:, :, 0].astype(np.uint64))
    some = packed.counts > 0
    assert np.array_equal(packed.min_bits[some], R.key_bits(ref[:, :, 2])[some]) and np.array_equal(packed.max_bits[some], R.key_bits(ref[:, :, 3])[some])
    assert not some[1, C - 1] and np.isnan(packed.minimum[1, C - 1]) and np.isnan(packed.maximum[1, C - 1])
    for k in (0, 7, len(canvases) - 1):
        assert packed.block(k).tobytes() == R.block(canvases[k], layout, predictor).tobytes()
    # the extrema as floats: numpy's own, over the values that are not NaN (numpy's min does not tell -0 from +0: compare values)
    for k in (5, 29):
        for c in range(C):
            v = canvases[k][c][~np.isnan(canvases[k][c])]
            assert packed.minimum[k, c] == v.min() and packed.maximum[k, c] == v.max()


@pytest.mark.parametrize("form", [0, 1], ids=["rule", "direct"])
@pytest.mark.parametrize("layout", [R.BAND, R.PIXEL], ids=["band", "pixel"])
def test_one_large_canvas(layout, form):
    """1031 x 1025 x 6: thousands of workgroups, groups of three rows with a remainder and rows of 24 600 bytes piece by piece, blocks of 25 MB"""
    C, H, W = GC.BIG
    c = GC.canvas(C, H, W)
    for predictor in (1, 3):
        got, packed = run([c], C, layout, predictor, form)
        want = R.expected_buffer([c], C, layout, predictor, force_direct=bool(form), poison=POISON, guard=GUARD)
        assert first_difference(got, want) is None, (predictor,)


@pytest.mark.parametrize("C", [1, 6])
def test_k_canvases_give_the_bytes_of_k_launches(C):
    """K = 4 as [ordinary, flagged 'no file', 1 x 1, wide (the direct form by the rule)] and K = 1"""
    canvases, skip = GC.k4_canvases(C)
    for layout in (R.BAND, R.PIXEL):
        for predictor in (1, 3):
            got, packed = run(canvases, C, layout, predictor, 0, skip)
            want = R.expected_buffer(canvases, C, layout, predictor, skip, poison=POISON, guard=GUARD)
            assert first_difference(got, want) is None, (layout, predictor)
            packed.read()
            assert packed.block(1) is None and packed.place[1, 3] == 0 and packed.place[2, 0] == packed.place[1, 0]
            for k in (0, 2, 3):
                one, p1 = run([canvases[k]], C, layout, predictor)
                p1.read()
                assert p1.block(0).tobytes() == packed.block(k).tobytes(), (layout, predictor, k)
                assert np.array_equal(p1.counts[0], packed.counts[k]) and np.array_equal(p1.min_bits[0], packed.min_bits[k])
                assert np.array_equal(p1.max_bits[0], packed.max_bits[k])
    # every canvas flagged: nothing is launched, nothing but the statistics' initial words is written
    got, packed = run(canvases, C, R.BAND, 3, 0, [True] * 4)
    assert first_difference(got, R.expected_buffer(canvases, C, R.BAND, 3, [True] * 4, poison=POISON, guard=GUARD)) is None
    assert int(packed.place[-1, 0]) == 0 and int(packed.place[-1, 2]) == 0


def test_pack_and_write_bands_through_the_public_functions(tmp_path):
    """geotiff.pack's one read; write_bands in both layouts, with and without compression, read back; libtiff on a single band"""
    b = GC.canvas(6, 5, 65, all_nan_band=4)
    dev = torch.from_numpy(b.copy()).to(DEV)
    table = ops.AtlasTable([5], [65], [10.0], [20.0], device=DEV)
    packed = geotiff.pack(dev.view(-1), 6, table, interleave="pixel", predictor=3).read()
    assert packed.block(0).tobytes() == R.block(b, R.PIXEL, 3).tobytes() and packed.read() is packed
    for name, layout in (("band", R.BAND), ("pixel", R.PIXEL)):
        for compress, predictor in (("deflate", None), ("deflate", 1), (None, None)):
            p = geotiff.write_bands(str(tmp_path / f"{name}_{compress}_{predictor}.tif"), dev, 700000.5, 6600000.25, 0.5, compress=compress,
                                    predictor=predictor, interleave=name)
            r = geotiff.read(p)
            assert np.array_equal(bits(r["bands"]), bits(b)) and r["geotransform"] == [700000.5, 0.5, 0.0, 6600000.25, 0.0, -0.5]
            assert r["band_names"] == list(geotiff.FINAL_RASTER_BANDNAMES)
            assert r["tags"].get(317, (1,))[0] == (3 if (compress and predictor is None) else 1)
            assert "STATISTICS_MINIMUM" not in r["statistics"][4] and float(r["statistics"][4]["STATISTICS_VALID_PERCENT"]) == 0.0
            v = b[0][~np.isnan(b[0])]
            assert np.float32(r["statistics"][0]["STATISTICS_MINIMUM"]) == v.min() and np.float32(r["statistics"][0]["STATISTICS_MAXIMUM"]) == v.max()
            # the file is what the restatement assembles from the same bands and statistics
            want = R.assemble(b, 700000.5, 6600000.25, 0.5, layout, 3 if (compress and predictor is None) else 1, compress == "deflate",
                              stats=r["statistics"])
            assert open(p, "rb").read() == want
    with pytest.raises(ValueError):
        geotiff.write_bands(str(tmp_path / "no.tif"), dev, 0.0, 0.0, 0.5, compress=None, predictor=3)
    one = geotiff.write_bands(str(tmp_path / "one.tif"), dev[2:3], 1.0, 2.0, 0.5)
    from PIL import Image, features
    if features.check("libtiff"):
        assert np.array_equal(bits(np.array(Image.open(one))), bits(b[2]))


def test_predict_parcels_to_files_and_back(tmp_path):
    from stratanet2_vegetation_coverage_maps_amd import PointNet2, parcel
    from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_parcel

    def rings_of(cloud):                     # a pentagon with a triangular hole, as tests/test_gpu_parcel_admissibility.py cuts it
        x0, x1, y0, y1 = (float(v) for v in (cloud[0].min(), cloud[0].max(), cloud[1].min(), cloud[1].max()))
        return [np.array([[x0 + 1.6, y0 + 1.35], [x1 - 2.05, y0 + 1.65], [x1 - 1.45, y1 - 1.8], [0.5 * (x0 + x1), y1 - 15.5], [x0 + 1.25, y1 - 2.2]]),
                np.array([[x0 + 10.0, y0 + 10.0], [x0 + 10.0, y0 + 15.75], [x0 + 16.5, y0 + 14.5]])]
    a = make_args(cuda=0, subsample_size=1024)
    clouds = [make_parcel(width_m=60, height_m=50, plant=False, seed=k, x0=650000 + 1000 * k, **({"density": 0.02} if k == 1 else {}))
              for k in range(3)]
    shapes = [rings_of(c) for c in clouds]
    torch.manual_seed(3)
    model = PointNet2(a).eval()
    atlas = parcel.predict_parcels(model, clouds, a, shapes=shapes, batch_size=512, seed=20240611, fps_start=0)[0]
    rep = atlas.report(shapes, admissibility=5)
    assert rep.empty == [False, True, False] and rep.n_bands == 6
    origin = (100.0, -50.25)
    paths = [str(tmp_path / f"parcel_{k}.tif") for k in range(3)]
    done = geotiff.write_atlas(paths, atlas, rep, origin=origin)
    assert done == [paths[0], None, paths[2]] and not os.path.exists(paths[1])
    for k in (0, 2):
        r = geotiff.read(paths[k])
        want = rep.bands(k).cpu().numpy()
        assert np.array_equal(bits(r["bands"]), bits(want))
        x_min, y_max = rep.table.geo(k)
        assert r["geotransform"] == [x_min + origin[0], atlas.pix, 0.0, y_max + origin[1], 0.0, -atlas.pix]
        assert r["epsg"] == 2154 and np.isnan(r["nodata"]) and r["band_names"] == list(geotiff.FINAL_RASTER_BANDNAMES)
        assert r["tags"][259] == (8,) and r["tags"][317] == (3,) and r["tags"][284] == (2,)
        for c in range(6):
            n = int(rep.band_counts[k, c])
            assert float(r["statistics"][c]["STATISTICS_VALID_PERCENT"]) == 100.0 * n / want[c].size
            if n:
                assert float(r["statistics"][c]["STATISTICS_MEAN"]) == rep.band_means[k, c]
        # the shapefile fields from the file: the report's fp64 means up to the order of the sum (n <= 4 10^4 terms: n 2^-53 < 5e-12)
        fields = geotiff.parcel_predicted_values(paths[k])
        for name, c in geotiff.SHP_FIELDS:
            assert abs(fields[name] - rep.band_means[k, c]) <= 1e-11 * abs(rep.band_means[k, c])
        # band 0 through libtiff: its strips in a single-band header
        from PIL import Image, features
        if features.check("libtiff"):
            data, t = open(paths[k], "rb").read(), r["tags"]
            per = len(t[273]) // 6
            strips = [data[o:o + n] for o, n in zip(t[273][:per], t[279][:per])]
            one = tmp_path / f"band0_{k}.tif"
            one.write_bytes(R.single_band_file(strips, want.shape[1], want.shape[2], t[278][0], True, 3))
            assert np.array_equal(bits(np.array(Image.open(str(one)))), bits(want[0]))
    assert geotiff.write_atlas([paths[0], paths[1], None], atlas, rep, compress=None) == [paths[0], None, None]
    assert np.array_equal(bits(geotiff.read(paths[0])["bands"]), bits(rep.bands(0).cpu().numpy()))
    assert geotiff.parcel_predicted_values(None)["PRED_ADM"] == -1
