"""The dBase record annotator on the device (sn2_dbf_annotate, csrc/dbf.hip) bit for bit against `records + format_field_ref(...)`,
its argument errors with dst untouched, and a parcel shapefile end to end: shp.read -> cut_parcels -> predict_parcels -> report ->
shp.write_predictions -> shp.read."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import _shp_cases as SC
from stratanet2_vegetation_coverage_maps_amd import _lib, geotiff, shp
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD, POISON = 256, 0xA5
FORMATS = [(50, 10), (12, 3)]                    # the second makes the cut [:size] bite
C = 5


@pytest.fixture(scope="module")
def table():
    """The values -- the planted list, 2 000 random bit patterns below 2^53, two at and above 2^53 -- as (R,C) fp64, and per format
    the reference field of every value and of `missing`, computed ONCE with `format_field_ref`."""
    v = np.concatenate([[p for p, _ in SC.PLANTED], SC.random_doubles(2000, 20240611), [2.0 ** 53, -1e300]])
    assert v.size == 2015
    values = np.ascontiguousarray(v.reshape(-1, C))                                   # (403, 5)
    ref = {}
    for size, decimal in FORMATS:
        text = np.stack([np.frombuffer(shp.format_field_ref(x, size, decimal), dtype=np.uint8) for x in v]).reshape(values.shape + (size,))
        ref[(size, decimal)] = (text, np.frombuffer(shp.format_field_ref(-1.0, size, decimal), dtype=np.uint8))
    for (p, t), x in zip(SC.PLANTED, ref[(50, 10)][0].reshape(-1, 50)):
        assert x.tobytes() == t.rjust(50).encode("ascii")                             # the reference is CPython's literals there
    return values, torch.from_numpy(values).to(DEV), ref


def expected(records, row_of, cols, text, missing_text):
    K = len(records)
    fields = np.where((row_of >= 0)[:, None, None], text[np.maximum(row_of, 0)][:, cols, :], missing_text[None, None, :])
    out = np.concatenate([records, fields.reshape(K, -1)], 1)
    overflow = int(((fields == ord("*")).all(axis=2)).sum())
    return np.ascontiguousarray(out), overflow


def run(records, values_dev, row_of, cols, size, decimal):
    K, L = records.shape
    total = (K * (L + len(cols) * size) + 7) // 8 * 8 + 8
    buf = torch.full((GUARD + total + GUARD,), POISON, dtype=torch.uint8, device=DEV)
    done = ops.dbf_annotate(torch.from_numpy(records).to(DEV), values_dev, torch.from_numpy(row_of).to(DEV), cols, size, decimal, -1.0,
                            out=buf[GUARD:GUARD + total])
    done.read()
    return buf.cpu().numpy(), done


@pytest.mark.parametrize("size,decimal", FORMATS)
@pytest.mark.parametrize("L", [1, 2, 7, 33, 254, 4000])
def test_annotate_is_records_plus_format_field_ref(table, L, size, decimal):
    values, values_dev, ref = table
    text, missing_text = ref[(size, decimal)]
    R = len(values)
    rng = np.random.default_rng(L * 100 + size)
    for K in (1, 3, 64, 65, 257):
        for cols in ([3], [4, 0, 3, 1]):                                              # non-ascending
            records = rng.integers(0, 256, size=(K, L), dtype=np.uint8)
            row_of = ((np.arange(K) * 37 + int(rng.integers(0, R))) % R).astype(np.int32)
            row_of[0] = 0                                                             # the planted rows, in every case
            if K > 1:
                row_of[1] = R - 1                                                     # the row with the two values from 2^53 on
                row_of[2::5] = -1
            want, overflow = expected(records, row_of, cols, text, missing_text)
            got, done = run(records, values_dev, row_of, cols, size, decimal)
            Ld = L + len(cols) * size
            assert done.records.shape == (K, Ld)
            bad = np.nonzero(done.records != want)
            assert bad[0].size == 0, (K, L, cols, bad[0][:4], bad[1][:4])
            assert done.overflow == overflow and (K == 1 or overflow >= 1)
            # nothing but the records and the counter is written: the guards, and the padding before the counter
            assert (got[:GUARD] == POISON).all() and (got[GUARD + done.total:] == POISON).all()
            assert (got[GUARD + K * Ld:GUARD + done.counter_at] == POISON).all()


def test_every_value_once_counts_two_overflows(table):
    values, values_dev, ref = table
    R = len(values)
    rng = np.random.default_rng(1)
    records = rng.integers(0, 256, size=(R, 7), dtype=np.uint8)
    row_of = rng.permutation(R).astype(np.int32)
    cols = [4, 2, 0, 3, 1]
    for size, decimal in FORMATS:
        want, overflow = expected(records, row_of, cols, *ref[(size, decimal)])
        got, done = run(records, values_dev, row_of, cols, size, decimal)
        assert overflow == 2 and done.overflow == 2 and np.array_equal(done.records, want)
    # a row index beyond R reads nothing and gives `missing`
    far = row_of.copy()
    far[5] = R
    want, _ = expected(records, np.where(far == R, -1, far).astype(np.int32), cols, *ref[(50, 10)])
    assert np.array_equal(run(records, values_dev, far, cols, 50, 10)[1].records, want)


def test_every_argument_error_returns_before_any_launch_with_dst_untouched(table):
    values, values_dev, _ = table
    lib = _lib.load()
    K, L, n, size, decimal = 3, 7, 4, 50, 10
    total = (K * (L + n * size) + 7) // 8 * 8 + 8
    src = torch.zeros(K * L, dtype=torch.uint8, device=DEV)
    row_of = torch.zeros(K, dtype=torch.int32, device=DEV)
    dst = torch.full((total,), POISON, dtype=torch.uint8, device=DEV)
    R = len(values)

    def call(**kw):
        a = dict(src=src.data_ptr(), K=K, L=L, values=values_dev.data_ptr(), R=R, C=C, row_of=row_of.data_ptr(), cols=[0, 1, 2, 4], n=None,
                 size=size, decimal=decimal, missing=-1.0, dst=dst.data_ptr(), dst_bytes=total)
        a.update(kw)
        cols = a["cols"]
        n_ = len(cols) if a["n"] is None else a["n"]
        arr = None if cols is None else (ctypes.c_int * max(len(cols), 1))(*cols)
        return lib.sn2_dbf_annotate(a["src"], a["K"], a["L"], a["values"], a["R"], a["C"], a["row_of"], arr, n_, a["size"], a["decimal"],
                                    a["missing"], a["dst"], a["dst_bytes"], ops._stream())
    bad = [dict(src=None), dict(values=None), dict(row_of=None), dict(cols=None, n=4), dict(dst=None),
           dict(K=0), dict(K=-1), dict(L=0), dict(L=65536), dict(size=0), dict(size=255), dict(decimal=-1), dict(decimal=16),
           dict(size=11, decimal=10), dict(cols=[], n=0), dict(cols=[0] * 256), dict(cols=[0, 1, -1, 2]), dict(cols=[0, 1, C, 2]),
           dict(dst_bytes=total - 1), dict(dst_bytes=K * (L + n * size)), dict(L=65535 - n * size + 1), dict(L=65000, size=254, cols=[0, 1, 2]),
           dict(dst=dst.data_ptr() + 8, dst_bytes=total - 8)]
    for kw in bad:
        assert call(**kw) == _lib.SN2_EINVAL, kw
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == POISON).all()
    dst[(K * (L + n * size) + 7) // 8 * 8:].zero_()
    assert call() == 0                                                               # and the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert (dst.cpu().numpy()[:K * (L + n * size)] != POISON).any()


def test_wrapper_refuses_before_any_launch(table):
    values, values_dev, _ = table
    rec = torch.zeros((3, 7), dtype=torch.uint8, device=DEV)
    rows = torch.zeros(3, dtype=torch.int32, device=DEV)
    for args in ((rec.cpu(), values_dev, rows), (rec, values_dev.float(), rows), (rec, values_dev, rows.long()), (rec, values_dev, rows[:2]),
                 (rec.view(-1), values_dev, rows)):
        with pytest.raises(ValueError):
            ops.dbf_annotate(*args, [0, 1])
    with pytest.raises(_lib.StrataHipError):
        ops.dbf_annotate(rec, values_dev, rows, [0, C])


# ---- end to end
def _shapefile(directory, shapes, ids):
    """a shapefile of polygons (None: a null shape) with the fields ID (C 8) and SURF (N 9.2), built like the fixture"""
    cs = []
    for rings in shapes:
        if rings is None:
            cs.append(struct.pack("<i", 0))
            continue
        parts, points = [], []
        for r in rings:
            parts.append(len(points))
            points += [tuple(p) for p in r]
        xs, ys = [p[0] for p in points], [p[1] for p in points]
        cs.append(SC._polygon_content(5, (min(xs), min(ys), max(xs), max(ys)), parts, points))
    fields = [("ID", "C", 8, 0), ("SURF", "N", 9, 2)]
    dbf = SC.dbf_header(fields, n_records=len(shapes)) + b"".join(b" " + i.ljust(8).encode("ascii") + b"%9.2f" % (100.0 + k)
                                                                  for k, i in enumerate(ids)) + b"\x1a"
    return SC.write_fixture(directory, name="job", shp=SC.shp_bytes(cs), shx=SC.shx_bytes(cs), dbf=dbf)


def test_parcel_job_from_shapefile_to_shapefile(tmp_path):
    from stratanet2_vegetation_coverage_maps_amd import PointNet2, parcel
    from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_parcel
    a = make_args(cuda=0, subsample_size=1024)
    tile = make_parcel(width_m=60, height_m=50, plant=False, seed=0, x0=650000)     # the smallest tile of the atlas tests
    x0, x1, y0, y1 = (float(v) for v in (tile[0].min(), tile[0].max(), tile[1].min(), tile[1].max()))
    rect = lambda ax, ay, bx, by: [[(ax, ay), (ax, by), (bx, by), (bx, ay), (ax, ay)]]
    typed = [None,                                                                    # parcel one: a null shape
             rect(x0 + 5000.0, y0 + 5000.0, x0 + 5030.0, y0 + 5030.0),                # parcel two: no point of the tile
             rect(x0 + 1.5, y0 + 1.25, x0 + 29.5, y1 - 1.75),
             [[(x0 + 30.5, y0 + 1.5), (x0 + 30.25, y1 - 2.0), (0.5 * (x0 + x1) + 15.0, y1 - 9.5), (x1 - 1.5, y1 - 1.25), (x1 - 1.75, y0 + 2.0)]]]
    base = _shapefile(tmp_path, typed, ["NUL", "FAR", "WEST", "EAST"])
    src = shp.read(base)
    assert src.shapes[0] is None and src.index_of("EAST") == 3
    real = [k for k, s in enumerate(src.shapes) if s is not None]
    cut = parcel.cut_parcels(torch.from_numpy(tile).to(DEV), [src.shapes[k] for k in real])
    parcel_index = np.asarray(real)[cut.parcel_index]
    assert parcel_index.tolist() == [2, 3]
    torch.manual_seed(3)
    model = PointNet2(a).eval()
    atlas = parcel.predict_parcels(model, cut.clouds, a, shapes=cut.shapes_kept, batch_size=512, seed=20240611, fps_start=0)[0]
    rep5 = atlas.report(cut.shapes_kept)
    rep = atlas.report(cut.shapes_kept, admissibility=5)
    assert rep.empty == [False, False] and rep.n_bands == 6
    (tmp_path / "out").mkdir()
    dst = str(tmp_path / "out" / "job_pred.shp")
    with pytest.raises(ValueError):
        shp.write_predictions(src, dst, rep5, parcel_index=parcel_index)             # PRED_ADM needs the six-band report
    with pytest.raises(ValueError):
        shp.write_predictions(src, base + ".shp", rep, parcel_index=parcel_index)    # src and dst are the same file
    with pytest.raises(ValueError):
        shp.write_predictions(src, dst, rep, parcel_index=[2, 2])
    with pytest.raises(ValueError):
        shp.write_predictions(src, dst, rep, parcel_index=[2, 4])
    with pytest.raises(ValueError):
        shp.write_predictions(src, dst, rep)                                         # two rows, four records, no index
    with pytest.raises(ValueError):
        shp.write_predictions(src, dst, rep, parcel_index=parcel_index, fields=(("SURF", 0),))
    done = shp.write_predictions(src, dst, rep, parcel_index=parcel_index)
    assert done.overflow == 0 and done.rows.tolist() == [-1, -1, 0, 1] and done.fields == [n for n, _ in geotiff.SHP_FIELDS]
    for ext in (".shp", ".shx"):
        assert open(base + ext, "rb").read() == open(dst[:-4] + ext, "rb").read()
    back = shp.read(dst)
    assert back.column("ID") == ["NUL", "FAR", "WEST", "EAST"] and back.column("SURF") == [100.0, 101.0, 102.0, 103.0]
    assert back.records[:, :src.records.shape[1]].tobytes() == src.records.tobytes()
    for name, c in geotiff.SHP_FIELDS:
        got = back.column(name)
        assert got[0] == -1.0 and got[1] == -1.0
        for j, k in enumerate(parcel_index):
            mean = float(rep.band_means[j, c])
            want = float(format(mean, ".10f")) if np.isfinite(mean) else mean
            assert got[k] == want or (np.isnan(got[k]) and np.isnan(want)), (name, k)
            at, _, size, _ = back._slot(name)
            assert back.records[k, at:at + size].tobytes() == format(mean, ".10f")[:50].rjust(50).encode("ascii")
    assert all(np.isfinite(rep.band_means[j, c]) for j in range(2) for _, c in geotiff.SHP_FIELDS[:3])
    # an empty flag sends its record to `missing`; a device tensor of values is taken as it is
    again = shp.write_predictions(src, str(tmp_path / "out" / "again.shp"), torch.from_numpy(rep.band_means).to(DEV), parcel_index=parcel_index,
                                  empty=[True, False])
    assert again.rows.tolist() == [-1, -1, -1, 1]
    b2 = shp.read(again.path)
    assert b2.column("PRED_BASSE")[2] == -1.0 and b2.column("PRED_BASSE")[3] == back.column("PRED_BASSE")[3]
