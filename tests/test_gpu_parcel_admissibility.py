"""PRED_ADM through the parcel entry points: `ParcelMosaic.report(rings, admissibility=s)` and `MosaicAtlas.report(shapes,
admissibility=s)` against the numpy restatement of the admissibility rule (tests/_admissibility_ref.py) applied to the uncropped
`finalize()` and the restated crop (tests/_parcel_report_ref.py): bands bit for bit, counts exactly; the fp64 means bit for bit
against the device's own crop statistics of the restated bands, and within 1e-11 relative of numpy's sum (the bound of
tests/test_gpu_parcel_report.py: n <= 40 000 non-negative terms, n 2^-53 < 5e-12 per order of summation).  The parcels and the
polygons are those of tests/test_gpu_parcel_report.py and tests/test_gpu_parcel_atlas.py."""
import numpy as np
import pytest
import torch

from _admissibility_ref import admissibility
from _parcel_report_ref import crop_stats
from stratanet2_vegetation_coverage_maps_amd import PointNet2, parcel
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
from stratanet2_vegetation_coverage_maps_amd.inference import REPORT_BANDS, REPORT_BANDS_ADM
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_parcel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MEAN_RTOL = 1e-11
SEED = 20240611
KEPT = [0, 1, 2, 3, 5]                      # where the five bands of finalize() lie among the six


def same_cropped(got, want_cropped, source):
    """the NaN mask of the restated crop and, on the survivors, the source's bits"""
    keep = ~np.isnan(want_cropped)
    return np.array_equal(np.isnan(got), ~keep) and got[keep].tobytes() == source[keep].tobytes()


def check_report(rep6, rep5, out5_host, x_min, y_max, pix, rings, s):
    """one parcel's six-band report against its five-band report and the restatement"""
    edges = None if rings is None else parcel.polygon_edges(rings)
    ref = admissibility(out5_host, s)
    want, want_mean, want_count = crop_stats(ref["bands6"], x_min, y_max, pix, edges)
    got = rep6.bands.cpu().numpy()
    assert rep6.n_bands == 6 and got.shape == want.shape
    assert got[KEPT].view(np.uint32).tobytes() == rep5.bands.cpu().numpy().view(np.uint32).tobytes()     # the bytes of report(rings)
    assert same_cropped(got[4], want[4], ref["bands6"][4])                                                # band 4: the restatement, cropped
    assert np.array_equal(rep6.admissibility_stats, ref["stats"])
    assert rep6.threshold == rep5.threshold
    assert np.array_equal(rep6.band_counts, want_count) and np.array_equal(rep6.band_counts[KEPT], rep5.band_counts)
    assert rep6.band_means[KEPT].tobytes() == rep5.band_means.tobytes()
    assert list(rep6.means) == list(REPORT_BANDS_ADM) and rep6.counts["PRED_ADM"] == int(want_count[4])
    assert rep6.means == {k: float(rep6.band_means[i]) for i, k in enumerate(REPORT_BANDS_ADM)}
    # the mean: the device's own statistics of the restated (uncropped) bands give the same fp64 bits ...
    dev = torch.from_numpy(ref["bands6"].copy()).to(DEV)
    mean_d, count_d = ops.mosaic_crop_stats(dev, x_min, y_max, pix, edges)
    assert rep6.band_means.tobytes() == mean_d.cpu().numpy().tobytes() and np.array_equal(count_d.cpu().numpy(), want_count)
    # ... and numpy's fp64 mean of the band lies within the summation bound
    print(f"\nPRED_ADM {rep6.means['PRED_ADM']:.17g} over {rep6.counts['PRED_ADM']} pixels (numpy {want_mean[4]:.17g}), "
          f"stats {rep6.admissibility_stats.tolist()}")
    if want_count[4] > 0:
        assert abs(rep6.means["PRED_ADM"] - want_mean[4]) <= MEAN_RTOL * abs(want_mean[4])
    else:
        assert np.isnan(rep6.means["PRED_ADM"])
    return ref


@pytest.fixture(scope="module")
def one_parcel():
    a = make_args(cuda=0, subsample_size=1024)
    cloud = make_parcel(order="scanline", seed=11)
    x0, x1, y0, y1 = (float(v) for v in (cloud[0].min(), cloud[0].max(), cloud[1].min(), cloud[1].max()))
    rings = [np.array([[x0 + 3.2, y0 + 2.7], [x1 - 4.1, y0 + 3.3], [x1 - 2.9, y1 - 3.6], [0.5 * (x0 + x1), y1 - 31.0], [x0 + 2.5, y1 - 4.4]]),
             np.array([[x0 + 20.0, y0 + 20.0], [x0 + 20.0, y0 + 31.5], [x0 + 33.0, y0 + 29.0]])]
    torch.manual_seed(3)
    model = PointNet2(a).eval()
    mos, _ = parcel.predict_parcel_cloud(model, cloud, a, batch_size=16, rs=np.random.RandomState(2), fps_start=0, shape=rings)
    return mos, rings


def test_report_with_admissibility(one_parcel, monkeypatch):
    mos, rings = one_parcel
    out5, thr = mos.finalize()
    out5_host = out5.cpu().numpy()
    rep5 = mos.report(rings)
    torch.cuda.synchronize()

    counts = {"item": 0, "cpu": 0, "tolist": 0, "numpy": 0, "synchronize": 0}

    def counted(name, fn):
        def wrapper(*args, **kw):
            if name == "synchronize" or args[0].is_cuda:
                counts[name] += 1
            return fn(*args, **kw)
        return wrapper
    for name in ("item", "cpu", "tolist", "numpy"):
        monkeypatch.setattr(torch.Tensor, name, counted(name, getattr(torch.Tensor, name)))
    monkeypatch.setattr(torch.cuda, "synchronize", counted("synchronize", torch.cuda.synchronize))
    rep6 = mos.report(rings, admissibility=5)
    monkeypatch.undo()
    assert counts == {"item": 0, "cpu": 1, "tolist": 0, "numpy": 0, "synchronize": 0}        # still ONE read

    ref = check_report(rep6, rep5, out5_host, mos.x_min, mos.y_max, mos.pix, rings, 5)
    assert ref["stats"][0] >= 1 and rep6.counts["PRED_ADM"] > 1000
    # finalize(admissibility=s): the uncropped six bands; other sieve sizes and no crop go the same way
    six, thr6 = mos.finalize(admissibility=5)
    assert six.cpu().numpy().view(np.uint32).tobytes() == ref["bands6"].view(np.uint32).tobytes()
    assert thr6.cpu().numpy().tobytes() == thr.cpu().numpy().tobytes()
    check_report(mos.report(rings, admissibility=0), rep5, out5_host, mos.x_min, mos.y_max, mos.pix, rings, 0)
    check_report(mos.report(None, admissibility=2), mos.report(), out5_host, mos.x_min, mos.y_max, mos.pix, None, 2)


def test_without_the_argument_nothing_changes(one_parcel):
    mos, rings = one_parcel
    out, thr = mos.finalize()
    want, want_thr = ops.mosaic_finalize(mos.mean.contiguous(), mos.wsum[0].contiguous())
    assert out.shape[0] == 5 and out.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    assert thr.cpu().numpy().tobytes() == want_thr.cpu().numpy().tobytes()
    rep = mos.report(rings)
    mean, count = ops.mosaic_crop_stats(want, mos.x_min, mos.y_max, mos.pix, parcel.polygon_edges(rings))       # crops `want` in place
    assert rep.bands.shape[0] == 5 and rep.bands.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    assert rep.n_bands == 5 and rep.admissibility_stats is None and list(rep.means) == list(REPORT_BANDS) and "PRED_ADM" not in rep.means
    assert rep.band_means.tobytes() == mean.cpu().numpy().tobytes() and np.array_equal(rep.band_counts, count.cpu().numpy())
    assert rep.band_means.shape == (5,) and rep.threshold == float(want_thr[0])


def rings_of(cloud):
    x0, x1, y0, y1 = (float(v) for v in (cloud[0].min(), cloud[0].max(), cloud[1].min(), cloud[1].max()))
    return [np.array([[x0 + 1.6, y0 + 1.35], [x1 - 2.05, y0 + 1.65], [x1 - 1.45, y1 - 1.8], [0.5 * (x0 + x1), y1 - 15.5], [x0 + 1.25, y1 - 2.2]]),
            np.array([[x0 + 10.0, y0 + 10.0], [x0 + 10.0, y0 + 15.75], [x0 + 16.5, y0 + 14.5]])]


def test_two_parcels_through_predict_parcels():
    a = make_args(cuda=0, subsample_size=1024)
    clouds = [make_parcel(width_m=60, height_m=50, plant=False, seed=k, x0=650000 + 1000 * k) for k in range(2)]
    shapes = [rings_of(c) for c in clouds]
    torch.manual_seed(3)
    model = PointNet2(a).eval()
    atlas = parcel.predict_parcels(model, clouds, a, shapes=shapes, batch_size=512, seed=SEED, fps_start=0)[0]
    rep5 = atlas.report(shapes)
    rep6 = atlas.report(shapes, admissibility=5)
    assert rep5.n_bands == 5 and rep5.admissibility_stats is None and rep5.band_means.shape == (2, 5)
    assert rep6.n_bands == 6 and rep6.admissibility_stats.shape == (2, 4) and rep6.band_means.shape == (2, 6) and len(rep6) == 2
    arena5 = atlas.finalize()[0]
    arena6 = atlas.finalize(admissibility=5)[0]
    for k in range(2):
        out5_host = atlas.table.view(arena5, 5, k).cpu().numpy()
        x_min, y_max = atlas.table.geo(k)
        ref = check_report(rep6.parcel(k), rep5.parcel(k), out5_host, x_min, y_max, atlas.pix, shapes[k], 5)
        assert atlas.table.view(arena6, 6, k).cpu().numpy().view(np.uint32).tobytes() == ref["bands6"].view(np.uint32).tobytes()
        assert rep6.bands(k).shape == (6,) + atlas.table.shape(k)
