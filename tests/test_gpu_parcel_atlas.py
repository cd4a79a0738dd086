"""Mosaic atlas on the device (include/strata_hip.h, "Mosaic atlas"; csrc/atlas.hip): canvas by canvas the atlas entry points
must leave the bytes the single-canvas entry points leave on that canvas's view.  Every comparison is on int32 / int64 views of
the bytes, so NaNs are compared too.  The finalisation's medium-band values are multiples of 2^-16: their fp64 sums are exact in
every order, so the single-canvas call's atomic sum and the atlas's fixed-order sum are the same number.  (End to end the values
are the network's: the two sums may then differ in their last fp64 bit, which changes a band only where it moves the fp32 mean
they are rounded to -- one fp64 step out of 2^29.)"""
import numpy as np
import pytest
import torch

from _parcel_report_ref import crop_stats
from test_gpu_parcel_report import MEAN_RTOL, PIX, X_MIN, Y_MAX, at, concave_with_hole_and_second_part, make_bands
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
from stratanet2_vegetation_coverage_maps_amd import parcel
from stratanet2_vegetation_coverage_maps_amd.inference import MosaicAtlas, weights_band
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_parcel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def words(t: torch.Tensor) -> np.ndarray:
    """the bytes of a device tensor as integers"""
    t = t.contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int64).cpu().numpy()


# ---- 1. merge -------------------------------------------------------------------------------------------------------------
MERGE_SHAPES = [(8, 8), (13, 21), (9, 70), (5, 6)]
# (canvas, row, col): runs of 1, 4 and 2 plots, then a batch that continues canvas 2 alone
PLACE = np.array([(0, 0, 0),                                  # the plot IS the canvas
                  (1, 0, 0),                                  # where canvas 0's plot sits: a mixed-up canvas would show
                  (1, 3, 5), (1, 3, 5),                       # two plots at one offset, overlapping the one before
                  (1, 9, 17),                                 # hangs over the bottom and the right edge of 13 x 21
                  (2, 0, 0), (2, 1, 60),                      # columns 60 .. 67: across the 64-column tile, rows 1 .. 8: three 4-row tiles
                  (2, 0, 30), (2, 1, 58)], dtype=np.int32)    # second batch: overlaps the last plot of the first


def merge_inputs():
    rng = np.random.default_rng(11)
    r = rng.random((len(PLACE), 3, 8, 8), dtype=np.float32)
    r[rng.random(r.shape) < 0.2] = np.nan
    return torch.from_numpy(r).to(DEV), torch.from_numpy(weights_band(8).astype(np.float32)).to(DEV)


def fresh_arenas(table):
    mean = torch.full((3 * table.pixels,), float("nan"), dtype=torch.float32, device=DEV)
    wsum = torch.full((3 * table.pixels,), float("nan"), dtype=torch.float32, device=DEV)
    table.view(mean, 3, 3).fill_(123.0)                       # the sentinel canvas: no plot ever lands on it
    table.view(wsum, 3, 3).fill_(-7.0)
    return mean, wsum


def test_merge_equals_the_single_canvas_merge_canvas_by_canvas():
    table = ops.AtlasTable([s[0] for s in MERGE_SHAPES], [s[1] for s in MERGE_SHAPES], device=DEV)
    rasters, w = merge_inputs()
    assert (np.diff(PLACE[:7, 0]) >= 0).all() and np.bincount(PLACE[:7, 0]).tolist() == [1, 4, 2] and (PLACE[7:, 0] == 2).all()
    assert ops.atlas_segments(PLACE[:7], 8, table.host)[:, 7].tolist() == [0, 2, 2 + 4, 2 + 4 + 2 * 3]
    runs = {}
    for cut in ((7, 9), (9,), (1, 2, 3, 5, 6, 9)):            # 7 + 2, all nine in one call, and cuts inside the runs
        mean, wsum = fresh_arenas(table)
        b0 = 0
        for b1 in cut:
            ops.atlas_merge(rasters[b0:b1].contiguous(), w, PLACE[b0:b1], table, mean, wsum)
            b0 = b1
        runs[cut] = (words(mean), words(wsum))
    # the twins: each canvas on its own, NaN-filled, the same plots in the same order through the single-canvas call
    for k, (H, W) in enumerate(MERGE_SHAPES[:3]):
        tm = torch.full((3, H, W), float("nan"), dtype=torch.float32, device=DEV)
        tw = tm.clone()
        idx = np.flatnonzero(PLACE[:, 0] == k)
        ops.mosaic_merge(rasters[torch.from_numpy(idx).to(DEV)].contiguous(), w, torch.from_numpy(PLACE[idx, 1:].copy()).to(DEV), tm, tw)
        lo, hi = 3 * table.base(k), 3 * (table.base(k) + H * W)
        for cut, (m, s) in runs.items():
            assert np.array_equal(m[lo:hi], words(tm).reshape(-1)), (k, cut)
            assert np.array_equal(s[lo:hi], words(tw).reshape(-1)), (k, cut)
        assert not torch.isnan(tm).all() and torch.isnan(tm).any()
    lo = 3 * table.base(3)
    for m, s in runs.values():
        assert (m[lo:].view(np.float32) == 123.0).all() and (s[lo:].view(np.float32) == -7.0).all()          # untouched
    with pytest.raises(ValueError, match="non-decreasing"):
        ops.atlas_merge(rasters[:2].contiguous(), w, PLACE[[1, 0]], table, *fresh_arenas(table))


# ---- 2. finalisation ------------------------------------------------------------------------------------------------------
FIN_SHAPES = [(3, 5), (1, 1), (13, 21), (40, 300)]


def test_finalize_equals_the_single_canvas_finalize_canvas_by_canvas():
    table = ops.AtlasTable([s[0] for s in FIN_SHAPES], [s[1] for s in FIN_SHAPES], device=DEV)
    rng = np.random.default_rng(5)
    mean, wsum = [], []
    for k, (H, W) in enumerate(FIN_SHAPES):
        m = (rng.integers(0, 2 ** 16 + 1, (3, H, W)) / 2.0 ** 16).astype(np.float32)          # multiples of 2^-16 in [0, 1]
        m[rng.random(m.shape) < 0.25] = np.nan
        s = rng.random((3, H, W), dtype=np.float32) + 1.0
        s[rng.random(s.shape) < 0.1] = np.nan
        if k == 0:
            m[:] = np.nan                                                                     # all-NaN: index 0
        if k == 1:
            m[:] = 0.5
        mean.append(m.reshape(-1))
        wsum.append(s.reshape(-1))
    mean, wsum = torch.from_numpy(np.concatenate(mean)).to(DEV), torch.from_numpy(np.concatenate(wsum)).to(DEV)
    assert int(table.host[4, 3] - table.host[3, 3]) == 47                                      # 12 000 pixels: 47 partial sums
    bands, thr = ops.atlas_finalize(mean, wsum, table)
    again = ops.atlas_finalize(mean, wsum, table)
    assert np.array_equal(words(bands), words(again[0])) and np.array_equal(words(thr), words(again[1]))
    assert bands.shape == (5 * table.pixels,) and thr.shape == (4, 2)
    for k in range(4):
        want, want_thr = ops.mosaic_finalize(table.view(mean, 3, k), table.view(wsum, 3, k)[0])
        assert np.array_equal(words(table.view(bands, 5, k)), words(want)), k
        assert np.array_equal(words(thr[k]), words(want_thr)), k
    t = thr.cpu().numpy()
    assert t[0].tolist() == [0.0, 0.0] and torch.isnan(table.view(bands, 5, 0)).all()
    assert 0 < t[2, 1] < 10000 and 0 < t[3, 1] < 10000 and abs(t[3, 0] - t[3, 1] / 10000.0) < 1e-6


# ---- 3. crop and band statistics ------------------------------------------------------------------------------------------
def crop_cases():
    """(H, W, geotransform, rings or None)"""
    geo = [(X_MIN + 1000.0 * k, Y_MAX - 500.0 * k) for k in range(5)]
    half = [np.array([at(*(0.5 * (np.array([(v[0] - X_MIN) / PIX, (Y_MAX - v[1]) / PIX]))), *geo[0]) for v in ring])
            for ring in concave_with_hole_and_second_part()]                                  # the 37 x 45 polygon at half size
    long_side = [[(10.3, -1.0), (270.7, -1.0), (290.2, 1.2), (262.4, 4.0), (8.8, 4.0)], [(258.3, 0.2), (266.1, 0.3), (262.0, 1.9)]]
    two_segments = [np.array([at(u, v, *geo[1]) for u, v in ring]) for ring in long_side]
    column = [np.array([at(-1.0, 100.3, *geo[2]), at(2.0, 100.3, *geo[2]), at(2.0, 2000.7, *geo[2]), at(-1.0, 2000.7, *geo[2])])]
    between = [np.array([at(7.6, 4.6, *geo[4]), at(8.4, 4.6, *geo[4]), at(8.4, 5.4, *geo[4]), at(7.6, 5.4, *geo[4])])]
    return [(19, 23, geo[0], half), (3, 300, geo[1], two_segments), (2100, 1, geo[2], column), (5, 7, geo[3], None),
            (10, 12, geo[4], between)]


def test_crop_stats_equal_the_single_canvas_call_canvas_by_canvas():
    cases = crop_cases()
    K, C = len(cases), 5
    table = ops.AtlasTable([c[0] for c in cases], [c[1] for c in cases], [c[2][0] for c in cases], [c[2][1] for c in cases], device=DEV)
    assert 2100 > 2048 == int(table.host[3, 4] - table.host[2, 4])                            # more row segments than workgroups
    host = [make_bands(C, H, W, 20 + k) for k, (H, W, _, _) in enumerate(cases)]
    arena = torch.from_numpy(np.concatenate([b.reshape(-1) for b in host])).to(DEV)
    edges = [None if r is None else parcel.polygon_edges(r) for _, _, _, r in cases]
    mean, count = ops.atlas_crop_stats(arena, C, table, PIX, edges)
    assert mean.shape == (K, C) and mean.dtype == torch.float64 and count.shape == (K, C) and count.dtype == torch.int64
    mean_h, count_h = mean.cpu().numpy(), count.cpu().numpy()
    for k, (H, W, (x_min, y_max), rings) in enumerate(cases):
        twin = torch.from_numpy(host[k].copy()).to(DEV)
        m1, c1 = ops.mosaic_crop_stats(twin, x_min, y_max, PIX, edges[k])
        got = table.view(arena, C, k)
        assert np.array_equal(words(got), words(twin)), k
        assert np.array_equal(words(mean[k]), words(m1)) and np.array_equal(count_h[k], c1.cpu().numpy()), k        # fp64 means: the bytes
        want, want_mean, want_count = crop_stats(host[k], x_min, y_max, PIX, edges[k])
        g = got.cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(want)) and g[~np.isnan(g)].tobytes() == host[k][~np.isnan(want)].tobytes()
        assert np.array_equal(count_h[k], want_count)
        some = want_count > 0
        assert np.isnan(mean_h[k][~some]).all() and (np.abs(mean_h[k][some] - want_mean[some]) <= MEAN_RTOL * np.abs(want_mean[some])).all()
    assert 0 < count_h[0].min() and count_h[0].max() < 19 * 23 and 0 < count_h[1].min() and 1400 < count_h[2].max() <= 1901
    assert np.array_equal(words(table.view(arena, C, 3)).reshape(-1), host[3].reshape(-1).view(np.int32))           # E = 0: left alone
    assert count_h[3].max() <= 35 and count_h[3].min() > 0
    assert count_h[4].tolist() == [0] * C and np.isnan(mean_h[4]).all() and torch.isnan(table.view(arena, C, 4)).all()
    # no crop at all: the statistics of every canvas, nothing written
    arena2 = torch.from_numpy(np.concatenate([b.reshape(-1) for b in host])).to(DEV)
    mean2, count2 = ops.atlas_crop_stats(arena2, C, table, PIX)
    assert np.array_equal(words(arena2), np.concatenate([b.reshape(-1) for b in host]).view(np.int32))
    assert np.array_equal(count2[3].cpu().numpy(), count_h[3]) and np.array_equal(words(mean2[3]), words(mean[3]))


# ---- 4. end to end --------------------------------------------------------------------------------------------------------
SEED = 20240611


def rings_of(cloud):
    """`test_report_end_to_end`'s pentagon with a hole, at half size for a 60 m x 50 m parcel"""
    x0, x1, y0, y1 = (float(v) for v in (cloud[0].min(), cloud[0].max(), cloud[1].min(), cloud[1].max()))
    return [np.array([[x0 + 1.6, y0 + 1.35], [x1 - 2.05, y0 + 1.65], [x1 - 1.45, y1 - 1.8], [0.5 * (x0 + x1), y1 - 15.5], [x0 + 1.25, y1 - 2.2]]),
            np.array([[x0 + 10.0, y0 + 10.0], [x0 + 10.0, y0 + 15.75], [x0 + 16.5, y0 + 14.5]])]


@pytest.fixture(scope="module")
def four_parcels():
    from stratanet2_vegetation_coverage_maps_amd import PointNet2
    a = make_args(cuda=0, subsample_size=1024)
    clouds = [make_parcel(width_m=60, height_m=50, plant=False, seed=k, x0=650000 + 1000 * k, **({"density": 0.02} if k == 2 else {}))
              for k in range(4)]
    torch.manual_seed(3)
    model = PointNet2(a).eval()
    return a, clouds, [rings_of(c) for c in clouds], model


def atlas_words(atlas, rep):
    return [words(atlas.mean), words(atlas.wsum), words(rep.band_arena), rep.thresholds.view(np.int64), rep.band_means.view(np.int64),
            rep.band_counts]


def test_parcels_in_shared_batches_equal_the_parcels_one_by_one(four_parcels, monkeypatch):
    a, clouds, rings, model = four_parcels
    atlas5, set5 = parcel.predict_parcels(model, clouds, a, shapes=rings, batch_size=5, seed=SEED, fps_start=0)
    atlas, plots = parcel.predict_parcels(model, clouds, a, shapes=rings, batch_size=512, seed=SEED, fps_start=0)
    n = np.diff(plots.parcel_start)
    print(f"\nplots per parcel: {n.tolist()}")
    assert n[2] == 0 and (n[[0, 1, 3]] >= 8).all() and np.array_equal(set5.parcel_start, plots.parcel_start)
    assert isinstance(atlas, MosaicAtlas) and isinstance(plots, parcel.ParcelSet) and plots.n_parcels == 4
    assert np.array_equal(plots.parcel_of, np.repeat(np.arange(4), n))
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
    rep = atlas.report(rings)
    monkeypatch.undo()
    print(f"device-to-host reads of report(): {counts}")
    assert counts == {"item": 0, "cpu": 1, "tolist": 0, "numpy": 0, "synchronize": 0}

    # batches of five cut every parcel into pieces, the batch of 512 holds all of them: the same atlas, the same report
    for x, y in zip(atlas_words(atlas, rep), atlas_words(atlas5, atlas5.report(rings))):
        assert np.array_equal(x, y)
    whole = atlas.finalize()[0]
    for k in range(4):
        mos, pl = parcel.predict_parcel_cloud(model, clouds[k], a, batch_size=16, fps_start=0, sampler="device", seed=SEED,
                                              key_base=k << 32, shape=rings[k])
        one = rep.parcel(k)
        if k == 2:
            assert mos is None and len(pl) == 0 and atlas.mosaic(k) is None and rep.bands(k) is None and one.bands is None
            assert np.isnan(one.band_means).all() and one.band_counts.tolist() == [0] * 5 and np.isnan(one.threshold)
            assert all(np.isnan(v) for v in one.means.values()) and set(one.counts.values()) == {0}
            continue
        assert list(pl.plot_ids) == plots.plot_ids[plots.parcel_start[k]:plots.parcel_start[k + 1]]
        mean, wsum = atlas.mosaic(k)
        assert np.array_equal(words(mean), words(mos.mean)) and np.array_equal(words(wsum), words(mos.wsum)), k
        want = mos.report(rings[k])
        assert np.array_equal(words(one.bands), words(want.bands)), k
        assert one.threshold == want.threshold and np.array_equal(one.band_counts, want.band_counts), k
        assert one.band_means.tobytes() == want.band_means.tobytes() and one.means == want.means and one.counts == want.counts, k
        removed = torch.isnan(one.bands[4]).sum() - torch.isnan(atlas.table.view(whole, 5, k)[4]).sum()
        assert int(removed) > 0 and want.band_counts[0] > 200, k                      # the crop removed something


def test_set_batches_name_the_parcel_of_every_plot(four_parcels):
    a, clouds, rings, _ = four_parcels
    plots = parcel.prepare_parcels(clouds, a, shapes=rings)
    got = list(plots.batches(a, 7, sampler="device", seed=SEED))
    assert np.array_equal(np.concatenate([b["parcel"] for b in got]), plots.parcel_of)
    assert all(len(b["parcel"]) == b["cloud"].shape[0] == len(b["plot_center"]) for b in got) and len(got) == -(-len(plots) // 7)
    assert any(len(set(b["parcel"].tolist())) > 1 for b in got)                       # a batch cuts across parcels
    # a parcel alone, with the keys it has in the set, draws the same points
    k = 1
    alone = parcel.prepare_parcel(clouds[k], a, keep=parcel.polygon_keep(rings[k], parcel.shape_buffer(a)))
    mine = torch.cat([b["cloud"] for b in alone.batches(a, 512, sampler="device", seed=SEED, key_base=k << 32)])
    s0, s1 = plots.parcel_start[k], plots.parcel_start[k + 1]
    theirs = torch.cat([b["cloud"] for b in got])[s0:s1]
    assert np.array_equal(words(mine), words(theirs))
    assert not np.array_equal(words(mine), words(torch.cat([b["cloud"] for b in alone.batches(a, 512, sampler="device", seed=SEED)])))


def test_numpy_sampler_consumes_one_random_state_in_set_order(four_parcels):
    a, clouds, rings, model = four_parcels
    atlas, plots = parcel.predict_parcels(model, clouds, a, shapes=rings, batch_size=7, sampler="numpy", fps_start=0,
                                          rs=np.random.RandomState(5))
    rs = np.random.RandomState(5)
    for k in range(4):
        mos, pl = parcel.predict_parcel_cloud(model, clouds[k], a, batch_size=16, rs=rs, fps_start=0, shape=rings[k])
        if mos is None:
            assert atlas.mosaic(k) is None
            continue
        mean, wsum = atlas.mosaic(k)
        assert np.array_equal(words(mean), words(mos.mean)) and np.array_equal(words(wsum), words(mos.wsum)), k
