"""Parcel report on the device (include/strata_hip.h: sn2_mosaic_crop_stats, `ParcelMosaic.report`) against the fp64 numpy
restatement of tests/_parcel_report_ref.py: the NaN mask and the counts exactly, the surviving values bit for bit, the means
within 1e-11 relative (a sum of n <= 40 000 non-negative terms carries a relative error of at most n 2^-53 < 5e-12 in any order;
two orders: twice that)."""
import numpy as np
import pytest
import torch

from _parcel_report_ref import crop_stats, inside_mask
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
from stratanet2_vegetation_coverage_maps_amd import parcel
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_parcel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
X_MIN, Y_MAX, PIX = 651234.5, 6861234.25, 0.625          # Lambert-93 magnitudes: fp32 geometry (a step of 1/16 m in x, 1/2 m in y) fails
MEAN_RTOL = 1e-11


def at(cu, ru, x_min=X_MIN, y_max=Y_MAX, pix=PIX):
    """a vertex given in pixel units (column, row; pixel (r, c) has its centre at (c + 0.5, r + 0.5)) -> metres"""
    return [x_min + pix * cu, y_max - pix * ru]


def make_bands(C, H, W, seed):
    rng = np.random.default_rng(seed)
    b = rng.random((C, H, W), dtype=np.float32)
    b[rng.random((C, H, W)) < 0.2] = np.nan
    return b


def check(bands, rings, x_min=X_MIN, y_max=Y_MAX, pix=PIX):
    """device crop + statistics against the restatement; returns (device bands, mean, count, inside mask) as numpy"""
    edges = None if rings is None else parcel.polygon_edges(rings)
    want, want_mean, want_count = crop_stats(bands, x_min, y_max, pix, edges)
    dev = torch.from_numpy(bands.copy()).to(DEV)
    mean, count = ops.mosaic_crop_stats(dev, x_min, y_max, pix, edges)
    got, mean, count = dev.cpu().numpy(), mean.cpu().numpy(), count.cpu().numpy()
    nan_got, nan_want = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_got, nan_want), f"{np.count_nonzero(nan_got != nan_want)} pixels masked differently"
    assert got[~nan_got].tobytes() == bands[~nan_got].tobytes()                    # the survivors keep their bits
    assert count.dtype == np.int64 and np.array_equal(count, want_count)
    some = want_count > 0
    assert np.isnan(mean[~some]).all()
    rel = np.abs(mean[some] - want_mean[some]) / np.abs(want_mean[some])
    print(f"\nmeans: max relative difference {rel.max() if some.any() else 0.0:.3e} (bound {MEAN_RTOL:.0e}), counts {count.tolist()}")
    assert (rel <= MEAN_RTOL).all()
    inside = None if edges is None else inside_mask(bands.shape[1], bands.shape[2], x_min, y_max, pix, edges)
    return got, mean, count, inside


def concave_with_hole_and_second_part():
    exterior = [at(2.0, 3.0), at(30.0, 3.0),               # a horizontal edge
                at(30.0, 20.5),                            # a vertex at the y of row 20's centres
                at(22.0, 30.0), at(12.0, 20.0),            # this edge passes through the centres of pixels (20, 12) .. (29, 21)
                at(12.0, 33.0), at(2.0, 33.0)]             # concave at (12, 20); another horizontal edge
    hole = [at(5.2, 6.3), at(10.7, 6.3), at(10.7, 11.5), at(5.2, 11.5)]      # its lower edge lies ON the centres of row 11
    part = [at(34.3, 5.1), at(43.9, 8.2), at(38.0, 18.7)]
    return [np.array(exterior), np.array(hole), np.array(part)]


def test_concave_polygon_with_hole_and_second_part():
    H, W = 37, 45
    rings = concave_with_hole_and_second_part()
    bands = make_bands(5, H, W, 1)
    got, mean, count, inside = check(bands, rings)
    # the polygon is what the comments say it is: the centre of pixel (25, 17) lies exactly on the edge (22,30)-(12,20)
    e = parcel.polygon_edges(rings)
    cx, cy = at(17.5, 25.5)
    (ax, ay, bx, by), = e[(e[:, 0] == at(22.0, 30.0)[0]) & (e[:, 1] == at(22.0, 30.0)[1])]
    assert ay != by and ax + (cy - ay) * (bx - ax) / (by - ay) == cx
    assert (e[:, 1] == e[:, 3]).sum() == 4 and at(30.0, 20.5)[1] == Y_MAX - PIX * 20.5
    assert inside[25, 17] and not inside[25, 16]            # px < xint fails on the edge itself: the pixel counts as right of it
    assert inside[4, 20] and not inside[8, 8] and inside[8, 39] and not inside[25, 14] and not inside[2, 20]
    assert 0 < count.min() and count.max() < inside.sum() < H * W
    # fp32 geometry would not do: at these magnitudes an fp32 y has a step of 0.5 m, the centres of the rows are 0.625 m apart
    assert float(np.float32(at(0, 0.5)[1])) != at(0, 0.5)[1] and np.spacing(np.float32(Y_MAX)) == 0.5


def test_edge_chunking_star_of_1500_vertices():
    H, W, V = 70, 130, 1500
    # the star polygon {1500/749}: vertex j is point 749 j mod 1500 of an ellipse, so every edge is almost a diameter and a row
    # near the centre crosses almost all of them (even-odd: a fine radial pattern of inside and outside)
    ang = 2 * np.pi * ((749 * np.arange(V)) % V) / V
    star = np.array([at(65.0 + 60.0 * np.cos(t), 35.0 + 33.0 * np.sin(t)) for t in ang])
    edges = parcel.polygon_edges([star])
    assert edges.shape == (V, 4)                            # six chunks of 256 edges
    py = Y_MAX - PIX * 35.5
    assert np.count_nonzero((edges[:, 1] > py) != (edges[:, 3] > py)) > 1024     # more crossings on a row than the LDS list holds
    got, mean, count, inside = check(make_bands(5, H, W, 2), [star])
    assert 0.05 * H * W < inside.sum() < 0.95 * H * W


@pytest.mark.parametrize("H,W", [(3, 300), (300, 3)])
def test_row_segments(H, W):
    """a row longer than a workgroup's 256 pixels (two segments, the second partly filled), and many rows of three pixels"""
    long_side = [[(10.3, -1.0), (270.7, -1.0), (290.2, 1.2), (262.4, 4.0), (8.8, 4.0)], [(258.3, 0.2), (266.1, 0.3), (262.0, 1.9)]]
    rings = [np.array([at(u, v) if W > H else at(v, u) for u, v in ring]) for ring in long_side]        # exterior and hole
    got, mean, count, inside = check(make_bands(3, H, W, 3 + H), rings)
    inside = inside if W > H else inside.T
    assert inside[:, :8].sum() == 0 and inside[:, 12:256].all() and inside[:, 256:].any() and not inside[:, 292:].any()
    assert not inside[0, 262] and inside[2, 262]


def test_empty_and_full():
    H, W = 19, 23
    bands = make_bands(5, H, W, 5)
    between = [np.array([at(7.6, 4.6), at(8.4, 4.6), at(8.4, 5.4), at(7.6, 5.4)])]      # between four centres: contains none
    got, mean, count, inside = check(bands, between)
    assert not inside.any() and np.isnan(got).all() and count.tolist() == [0] * 5 and np.isnan(mean).all()
    around = [np.array([at(-2.0, -2.0), at(W + 2.0, -2.0), at(W + 2.0, H + 2.0), at(-2.0, H + 2.0)])]
    got, mean, count, inside = check(bands, around)
    assert inside.all() and got.tobytes() == bands.tobytes()


def test_stats_only_leaves_the_bands_alone():
    for C, H, W in ((5, 37, 45), (1, 1, 1), (8, 5, 517)):
        bands = make_bands(C, H, W, 6 + C)
        got, mean, count, _ = check(bands, None)
        assert got.tobytes() == bands.tobytes()
    with pytest.raises(ValueError):
        ops.mosaic_crop_stats(torch.zeros(2, 3, 4, device=DEV), X_MIN, Y_MAX, PIX, np.zeros((0, 4)))
    with pytest.raises(ops.StrataHipError):
        ops.mosaic_crop_stats(torch.zeros(9, 3, 4, device=DEV), X_MIN, Y_MAX, PIX)       # SN2_ELIMIT: nine bands


def test_two_calls_give_the_same_bytes():
    H, W = 70, 130
    bands = make_bands(5, H, W, 7)
    edges = torch.from_numpy(parcel.polygon_edges(concave_with_hole_and_second_part())).to(DEV)
    runs = []
    for _ in range(2):
        dev = torch.from_numpy(bands.copy()).to(DEV)
        mean, count = ops.mosaic_crop_stats(dev, X_MIN, Y_MAX, PIX, edges)
        runs.append((mean.cpu().numpy().tobytes(), count.cpu().numpy().tobytes(), dev.cpu().numpy().tobytes()))
    assert runs[0] == runs[1]
    # and on a mosaic whose row segments outnumber the workgroups (each workgroup then adds several segments)
    big = torch.rand(2, 2100, 300, device=DEV)
    a = [t.cpu().numpy().tobytes() for t in ops.mosaic_crop_stats(big, X_MIN, Y_MAX, PIX)]
    b = [t.cpu().numpy().tobytes() for t in ops.mosaic_crop_stats(big, X_MIN, Y_MAX, PIX)]
    assert a == b
    want = crop_stats(big.cpu().numpy(), X_MIN, Y_MAX, PIX)
    assert np.array_equal(np.frombuffer(a[1], dtype=np.int64), want[2])
    assert np.allclose(np.frombuffer(a[0], dtype=np.float64), want[1], rtol=2e-10, atol=0)     # n = 630 000: 2 n 2^-53 = 1.4e-10


def test_report_end_to_end(monkeypatch):
    from stratanet2_vegetation_coverage_maps_amd import PointNet2
    from stratanet2_vegetation_coverage_maps_amd.inference import REPORT_BANDS
    a = make_args(cuda=0, subsample_size=1024)
    cloud = make_parcel(order="scanline", seed=11)
    x0, x1, y0, y1 = (float(v) for v in (cloud[0].min(), cloud[0].max(), cloud[1].min(), cloud[1].max()))
    rings = [np.array([[x0 + 3.2, y0 + 2.7], [x1 - 4.1, y0 + 3.3], [x1 - 2.9, y1 - 3.6], [0.5 * (x0 + x1), y1 - 31.0], [x0 + 2.5, y1 - 4.4]]),
             np.array([[x0 + 20.0, y0 + 20.0], [x0 + 20.0, y0 + 31.5], [x0 + 33.0, y0 + 29.0]])]
    torch.manual_seed(3)
    model = PointNet2(a).eval()
    mos, pl = parcel.predict_parcel_cloud(model, cloud, a, batch_size=16, rs=np.random.RandomState(2), fps_start=0, shape=rings)
    # the lattice was filtered by the buffered polygon, as the reference filters it
    kept = parcel.prepare_parcel(cloud, a, keep=parcel.polygon_keep(rings, parcel.shape_buffer(a)))
    assert len(pl) > 20 and list(pl.plot_index) == list(kept.plot_index)
    out, thr = mos.finalize()
    out_host, thr_host = out.cpu().numpy(), thr.cpu().numpy()
    edges = parcel.polygon_edges(rings)
    want, want_mean, want_count = crop_stats(out_host, mos.x_min, mos.y_max, mos.pix, edges)
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
    rep = mos.report(rings)
    monkeypatch.undo()
    print(f"\ndevice-to-host reads of report(): {counts}")
    assert counts == {"item": 0, "cpu": 1, "tolist": 0, "numpy": 0, "synchronize": 0}

    assert rep.bands.is_cuda and rep.bands.shape == out.shape
    got = rep.bands.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and got[~np.isnan(got)].tobytes() == out_host[~np.isnan(want)].tobytes()
    assert 0 < np.isnan(want[4]).sum() - np.isnan(out_host[4]).sum()              # the crop removed something
    assert rep.threshold == float(thr_host[0])
    assert np.array_equal(rep.band_counts, want_count) and want_count[0] > 1000
    assert np.abs(rep.band_means - want_mean).max() <= MEAN_RTOL * np.abs(want_mean).max() and (want_mean >= 0).all()
    assert rep.means == {k: float(rep.band_means[i]) for i, k in enumerate(REPORT_BANDS)}
    assert rep.counts == {k: int(want_count[i]) for i, k in enumerate(REPORT_BANDS)}
    for i in range(5):
        assert abs(rep.band_means[i] - want_mean[i]) <= MEAN_RTOL * abs(want_mean[i])
    # without rings: the statistics of the whole mosaic, nothing cropped
    whole = mos.report()
    w_bands, w_mean, w_count = crop_stats(out_host, mos.x_min, mos.y_max, mos.pix, None)
    assert whole.bands.cpu().numpy().tobytes() == out_host.tobytes() and np.array_equal(whole.band_counts, w_count)
    assert np.allclose(whole.band_means, w_mean, rtol=MEAN_RTOL, atol=0) and whole.threshold == rep.threshold
