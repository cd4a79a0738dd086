"""The parcel cut on the device (csrc/cut.hip; parcel.cut_parcels, las.load_parcels) against `parcel.polygon_keep` in numpy and
plain numpy indexing: counts, the arena's bytes, point_index, the kept shapes -- on the planted inputs of tests/_cut_cases.py, on
70 parcels over one tile, with a longer row, a classification mask, tiles in a ParcelClouds, an origin, LAS files, and into
prepare_parcels."""
import numpy as np
import pytest
import torch

import _cut_cases as cases
import _las_ref as ref
from stratanet2_vegetation_coverage_maps_amd import las, parcel
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args

pytestmark = pytest.mark.gpu
B = cases.B


def check_cut(cut, tile, masks, shapes):
    """cut against the reference masks (K,T) of the host tile (10,T) -> the arena's bytes"""
    K = len(shapes)
    counts = masks.sum(1)
    assert isinstance(cut, parcel.ParcelCut) and cut.counts.shape == (K,) and np.array_equal(cut.counts, counts)
    ids = np.nonzero(counts)[0]
    assert np.array_equal(cut.parcel_index, ids) and len(cut.shapes_kept) == len(ids)
    pc = cut.clouds
    assert isinstance(pc, parcel.ParcelClouds) and pc.K == len(ids) and np.array_equal(np.diff(pc.point_start), counts[ids])
    arena, pidx = pc.arena.cpu().numpy(), cut.point_index.cpu().numpy()
    assert arena.shape == (10, counts.sum()) and arena.dtype == np.float32 and pidx.dtype == np.int32 and pidx.shape == (counts.sum(),)
    for j, k in enumerate(ids):
        s, e = pc.point_start[j], pc.point_start[j + 1]
        assert arena[:, s:e].tobytes() == tile[:, masks[k]].tobytes(), k
        assert np.array_equal(pidx[s:e], np.nonzero(masks[k])[0]), k
        assert pc.cloud(j).data_ptr() == pc.arena[:, s:].data_ptr()             # a view of the arena, no copy
        for r, want in zip(cut.shapes_kept[j], shapes[k]):
            assert np.array_equal(r, np.asarray(want, dtype=np.float64))
    return arena.tobytes() + pidx.tobytes()


@pytest.fixture(scope="module")
def planted():
    tile, _ = cases.tile()
    shapes = list(cases.shapes().values())
    dev = torch.from_numpy(tile.copy()).cuda()
    cut = parcel.cut_parcels(dev, shapes, B)
    return tile, dev, shapes, cases.masks(), cut


def test_planted_set_counts_bytes_and_index(planted):
    tile, dev, shapes, masks, cut = planted
    assert tile.shape[1] == 5 * 2048 + 37
    got = check_cut(cut, tile, masks, shapes)
    empty = cases.NAMES.index("empty")
    assert cut.counts[empty] == 0 and empty not in cut.parcel_index and len(cut.parcel_index) == len(shapes) - 1
    assert cut.point_index.is_cuda and cut.clouds.arena.is_cuda
    again = parcel.cut_parcels(dev, shapes, B)
    assert check_cut(again, tile, masks, shapes) == got                          # a second call: the same bytes
    # the planted points, one by one
    _, cols = cases.tile()
    pidx = cut.point_index.cpu().numpy()
    for c, (label, _, _, want) in zip(cols, cases.planted()):
        got_in = {cases.NAMES[cut.parcel_index[j]] for j in range(cut.clouds.K)
                  if c in pidx[cut.clouds.point_start[j]:cut.clouds.point_start[j + 1]]}
        assert got_in == {n for n, v in want.items() if v}, label


def test_no_parcel_gets_a_point(planted):
    tile, dev, shapes, masks, _ = planted
    cut = parcel.cut_parcels(dev, [shapes[cases.NAMES.index("empty")]], B)
    assert cut.clouds is None and cut.counts.tolist() == [0] and len(cut.parcel_index) == 0 and cut.shapes_kept == []
    assert cut.point_index.is_cuda and cut.point_index.dtype == torch.int32 and cut.point_index.numel() == 0


def test_wrappers_refuse_wrong_dtypes_and_shapes_before_any_launch(planted):
    tile, dev, shapes, masks, _ = planted
    from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
    table = ops.CutTable([parcel.polygon_edges(r) for r in shapes], tile.shape[1], B)
    with pytest.raises(ValueError, match="not uploaded"):
        ops.cut_count(dev, table)
    table.upload(dev.device)
    cls = torch.from_numpy(cases.classes()).cuda()
    drop = ops.cut_drop_words((7,))
    for bad, kw in ((dev.double(), {}), (dev[:, :-1].contiguous(), {}), (dev.t().contiguous().t(), {}),
                    (dev, dict(classification=cls.int(), drop=drop)), (dev, dict(classification=cls[:-1], drop=drop)),
                    (dev, dict(classification=cls)), (dev, dict(drop=drop)), (dev, dict(classification=cls, drop=drop[:4]))):
        with pytest.raises(ValueError):
            ops.cut_count(bad, table, **kw)
    prefix, starts = ops.cut_count(dev, table)
    base = torch.zeros(table.K, dtype=torch.int32, device=dev.device)
    total = int(starts[-1])
    assert total == masks.sum()
    for p, b, n in ((prefix[:-1], base, total), (prefix.long(), base, total), (prefix, base[:-1], total), (prefix, base.long(), total),
                    (prefix, base, 0), (prefix, base, 2 ** 31)):
        with pytest.raises(ValueError):
            ops.cut_fill(dev, table, p, b, n)
    with pytest.raises(ValueError):
        parcel.cut_parcels(dev.double(), shapes, B)
    with pytest.raises(ValueError):
        parcel.cut_parcels(dev, shapes, B, classification=cls[:100], drop_classes=(7,))


def test_seventy_parcels_over_one_small_tile():
    rings, tile, masks, b = cases.many()
    cut = parcel.cut_parcels(torch.from_numpy(tile.copy()).cuda(), rings, b)
    check_cut(cut, tile, masks, rings)


def test_a_longer_row_gives_the_bytes_of_the_default(planted):
    tile, dev, shapes, masks, cut = planted
    from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
    edges = [parcel.polygon_edges(r) for r in shapes]
    assert ops.CutTable(edges, tile.shape[1], B).L == 2048 and ops.CutTable(edges, tile.shape[1], B, max_table=16).L > 2048
    long_row = parcel.cut_parcels(dev, shapes, B, max_table=16)
    assert check_cut(long_row, tile, masks, shapes) == check_cut(cut, tile, masks, shapes)
    one_row = parcel.cut_parcels(dev, shapes, B, max_table=1)                    # the whole tile in one row
    assert check_cut(one_row, tile, masks, shapes) == check_cut(cut, tile, masks, shapes)


def test_classification_mask(planted):
    tile, dev, shapes, masks, cut = planted
    cls = cases.classes()
    cls_dev = torch.from_numpy(cls).cuda()
    dropped = parcel.cut_parcels(dev, shapes, B, classification=cls_dev, drop_classes=(7, 18))
    want = masks & ~np.isin(cls, (7, 18))[None, :]
    assert want.sum() < masks.sum()
    check_cut(dropped, tile, want, shapes)
    none = parcel.cut_parcels(dev, shapes, B, classification=cls_dev, drop_classes=())
    assert check_cut(none, tile, masks, shapes) == check_cut(cut, tile, masks, shapes)
    high = parcel.cut_parcels(dev, shapes, B, classification=cls_dev, drop_classes=(255, 2, 5, 7))     # a bit in the last word
    check_cut(high, tile, masks & (cls == 18)[None, :], shapes)


def test_two_tiles_in_a_parcel_clouds_are_the_cut_of_their_concatenation(planted):
    tile, dev, shapes, masks, cut = planted
    n = 4321
    pc = parcel.ParcelClouds.from_clouds([dev[:, :n], dev[:, n:]])
    assert pc.K == 2
    two = parcel.cut_parcels(pc, shapes, B)
    assert check_cut(two, tile, masks, shapes) == check_cut(cut, tile, masks, shapes)    # point_index: arena columns


def test_origin_shifts_the_shapes_into_the_clouds_frame(planted):
    tile, dev, shapes, masks, cut = planted
    o = np.array([7e5, 6.5e6])
    moved = [[r + o for r in rings] for rings in shapes]
    shifted = parcel.cut_parcels(dev, moved, B, origin=tuple(o))
    assert check_cut(shifted, tile, masks, shapes) == check_cut(cut, tile, masks, shapes)   # shapes_kept: in the cloud's frame


def _las_fields(rng, T, x0=0, y0=0):
    return {"X": rng.integers(-6000, 126000, T) + x0, "Y": rng.integers(-6000, 46000, T) + y0, "Z": rng.integers(0, 3000, T),
            "intensity": rng.integers(0, 60000, T), "returns": rng.integers(0, 64, T),
            "classification": rng.choice(np.array([2, 5, 7, 18]), T), "red": rng.integers(0, 65536, T),
            "green": rng.integers(0, 65536, T), "blue": rng.integers(0, 65536, T), "nir": rng.integers(0, 65536, T)}


@pytest.fixture(scope="module")
def las_files(tmp_path_factory):
    """two hand-written tiles over the planted parcels and a third one 4000 km away, centimetres with scale 0.01"""
    d = tmp_path_factory.mktemp("tiles")
    rng = np.random.default_rng(11)
    fields = [_las_fields(rng, 3000), _las_fields(rng, 2500), _las_fields(rng, 700, x0=400_000_000, y0=400_000_000)]
    paths = []
    for j, (f, fmt, ver) in enumerate(zip(fields, (8, 3, 1), ((1, 4), (1, 2), (1, 2)))):
        p = d / f"tile{j}.las"
        p.write_bytes(ref.write_las(f, fmt, version=ver))
        paths.append(str(p))
    return paths, fields


def _same(a, b):
    assert np.array_equal(a.counts, b.counts) and np.array_equal(a.parcel_index, b.parcel_index)
    assert a.clouds.arena.cpu().numpy().tobytes() == b.clouds.arena.cpu().numpy().tobytes()
    assert np.array_equal(a.point_index.cpu().numpy(), b.point_index.cpu().numpy())
    assert np.array_equal(a.clouds.point_start, b.clouds.point_start)
    assert all(np.array_equal(r, s) for x, y in zip(a.shapes_kept, b.shapes_kept) for r, s in zip(x, y))


@pytest.mark.parametrize("coords", ["reference", "header"])
def test_load_parcels_is_the_cut_of_the_loaded_tiles(las_files, coords, monkeypatch):
    paths, fields = las_files
    shapes = list(cases.shapes().values())
    pc = las.load_parcel_clouds(paths[:2], coords=coords)
    want = parcel.cut_parcels(pc, shapes, B)
    # against numpy from the files' own integers: x = X / 100 in fp64, then fp32 (both modes agree to the last bit or differ by
    # an ulp, so the reference masks are made from the decoded arena)
    arena = pc.arena.cpu().numpy()
    masks = np.stack([parcel.polygon_keep(r, B)(arena[:2].T.astype(np.float64)) for r in shapes])
    check_cut(want, arena, masks, shapes)
    assert want.counts.sum() > 500
    read = []
    upload = las._upload_points
    monkeypatch.setattr(las, "_upload_points", lambda path, *a, **k: (read.append(path), upload(path, *a, **k))[1])
    _same(las.load_parcels(paths[:2], shapes, B, coords=coords), want)
    assert read == paths[:2]
    # a third tile far away: read in the "reference" mode (it gets no point), never opened past its header in the "header" mode
    del read[:]
    got = las.load_parcels(paths, shapes, B, coords=coords)
    _same(got, want)
    assert read == (paths[:2] if coords == "header" else paths)
    if coords == "header":
        del read[:]
        none = las.load_parcels(paths[2:], shapes, B, coords=coords)
        assert read == [] and none.clouds is None and none.counts.tolist() == [0] * len(shapes)
    # the classification byte, decoded into one buffer over both tiles
    cls = np.concatenate([f["classification"] for f in fields[:2]]).astype(np.uint8)
    dropped = las.load_parcels(paths[:2], shapes, B, coords=coords, drop_classes=(7, 18))
    check_cut(dropped, arena, masks & ~np.isin(cls, (7, 18))[None, :], shapes)


def test_load_parcels_origin_keeps_cloud_and_shapes_in_one_frame(tmp_path):
    rng = np.random.default_rng(12)
    f = _las_fields(rng, 2000)
    X0, Y0 = 70_000_000, 650_000_000                                             # Lambert-93 in centimetres
    g = dict(f, X=f["X"] + X0, Y=f["Y"] + Y0)
    a, b = tmp_path / "local.las", tmp_path / "l93.las"
    a.write_bytes(ref.write_las(f, 3))
    b.write_bytes(ref.write_las(g, 3))
    shapes = list(cases.shapes().values())
    moved = [[r + np.array([X0 / 100, Y0 / 100]) for r in rings] for rings in shapes]
    want = las.load_parcels([str(a)], shapes, B)
    _same(las.load_parcels([str(b)], moved, B, origin=(X0, Y0, 0)), want)       # (X + X0 - X0) / 100: the same bits


def test_prepare_parcels_of_the_cut_is_that_of_the_host_cut():
    rng = np.random.default_rng(5)
    T = 20000
    tile = (rng.random((10, T)) * 30).astype(np.float32)
    tile[0] = (rng.random(T) * 130).astype(np.float32)
    tile[1] = (rng.random(T) * 130).astype(np.float32)
    sq = lambda x0, y0, s: [np.array([[x0, y0], [x0 + s, y0], [x0 + s, y0 + s], [x0, y0 + s]], dtype=np.float64)]
    shapes = [sq(25, 25, 30), sq(500, 500, 30), sq(70, 60, 35)]                  # the second gets no point
    args = make_args()
    cut = parcel.cut_parcels(torch.from_numpy(tile).cuda(), shapes)              # buffer: LAS_PARCEL_BUFFER
    pts = tile[:2].T.astype(np.float64)
    masks = [parcel.polygon_keep(r, parcel.LAS_PARCEL_BUFFER)(pts) for r in shapes]
    assert cut.parcel_index.tolist() == [0, 2] and masks[0].sum() > 2000 and (masks[0] & masks[2]).any()
    host = parcel.ParcelClouds.from_clouds([tile[:, masks[0]], tile[:, masks[2]]])
    want = parcel.prepare_parcels(host, args, shapes=[shapes[0], shapes[2]])
    got = parcel.prepare_parcels(cut.clouds, args, shapes=cut.shapes_kept)
    assert len(want) > 4 and len(got) == len(want)
    for name in ("raw", "offsets", "point_index", "centers"):
        assert getattr(got, name).cpu().numpy().tobytes() == getattr(want, name).cpu().numpy().tobytes(), name
