"""Per-point scores through the parcel entry points (`parcel.predict_parcel_cloud(points=True)`, `parcel.predict_parcels(points=True)`,
`inference.PointScores`) against the numpy restatement (tests/_point_scores_ref.py) fed the pointwise outputs the model returned for
the same batches.  30 m x 30 m parcels of about 2 10^4 points, 1024 samples per plot, the device sampler."""
import numpy as np
import pytest
import torch

import _point_scores_ref as ref
from stratanet2_vegetation_coverage_maps_amd import PointNet2, parcel
from stratanet2_vegetation_coverage_maps_amd.inference import PointScoreResult, PointScores, predict_batches
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_parcel

pytestmark = pytest.mark.gpu
SEED = 20250117
KW = dict(sampler="device", seed=SEED, fps_start=0)


def words(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def score_words(r: PointScoreResult):
    return [words(r.scores), words(r.weight), r.hits.cpu().numpy()]


def small_parcel(k=0):
    return make_parcel(30, 30, density=32.0, seed=10 + k, plant=False, x0=650000.0 + 1000.0 * k)


def restated(model, plots, args, T, batch_size):
    """The restatement over what the model returns, batch by batch, for `plots` (the loop of the entry points with a recording sink)."""
    rec = []

    def record(cov, proba, cur):
        rec.append(dict(cov=cov.cpu().numpy(), proba=proba.cpu().numpy(), xyz=cur["xyz"].cpu().numpy(), idx=cur["sample_index"].cpu().numpy(),
                        n_live=cur["sample_live"].cpu().numpy(), offsets=cur["point_offsets"].cpu().numpy(),
                        point_index=cur["point_index"].cpu().numpy(),
                        col_base=cur["col_base"].cpu().numpy() if "col_base" in cur else None))
    predict_batches(model, plots.batches(args, batch_size, with_samples=True, **KW), args, lambda rasters, cur: None, point_sink=record)
    return ref.point_scores(rec, T, args.diam_meters), rec


@pytest.fixture(scope="module")
def single():
    a = make_args(cuda=0, subsample_size=1024)
    cloud = small_parcel()
    torch.manual_seed(3)
    model = PointNet2(a).eval()
    mos, plots, scores = parcel.predict_parcel_cloud(model, cloud, a, batch_size=64, points=True, **KW)
    return a, cloud, model, mos, plots, scores


def test_single_parcel_equals_the_restatement(single):
    a, cloud, model, mos, plots, scores = single
    T = cloud.shape[1]
    assert 15000 < T < 30000 and len(plots) >= 4 and isinstance(scores, PointScores)
    res = scores.finalize()
    assert res.scores.shape == (8, T) and res.weight.shape == (T,) and res.hits.shape == (T,) and res.scores.is_cuda
    (s, w, h), rec = restated(model, plots, a, T, 64)
    got_s, got_w, got_h = res.scores.cpu().numpy(), res.weight.cpu().numpy(), res.hits.cpu().numpy()
    print(f"\nT {T}, plots {len(plots)}, points hit {int((h > 0).sum())}, most hits {int(h.max())}, contributions {int(h.sum())}")
    assert h.max() >= 2 and (h == 0).any() and np.array_equal(got_h, h)
    assert got_w.tobytes() == w.tobytes() and got_s.tobytes() == s.tobytes()
    # the batch dicts: with_samples adds its keys and nothing else changes
    plain = next(iter(plots.batches(a, 64, **KW)))
    rich = next(iter(plots.batches(a, 64, with_samples=True, **KW)))
    assert set(plain) == {"cloud", "xyz", "plot_center", "n_live", "fps_start"}
    assert set(rich) - set(plain) == {"sample_index", "sample_live", "plot_range", "point_offsets", "point_index", "diam_meters"}
    assert rich["plot_range"] == (0, min(64, len(plots))) and np.array_equal(words(plain["cloud"]), words(rich["cloud"]))
    assert "sample_live" in next(iter(plots.batches(a, 64, with_samples=True, n_live=False, **KW)))


def test_batch_size_does_not_change_a_byte_and_the_mosaic_is_the_plain_runs(single):
    a, cloud, model, mos, plots, scores = single
    mos2, _, scores2 = parcel.predict_parcel_cloud(model, cloud, a, batch_size=2, points=True, **KW)
    for x, y in zip(score_words(scores.finalize()), score_words(scores2.finalize())):
        assert np.array_equal(x, y)
    out = parcel.predict_parcel_cloud(model, cloud, a, batch_size=64, **KW)
    assert len(out) == 2                                                         # points=False: the return value of before
    for m in (mos, mos2):
        assert np.array_equal(words(m.mean), words(out[0].mean)) and np.array_equal(words(m.wsum), words(out[0].wsum))


def test_hits_lie_in_kept_discs(single):
    a, cloud, model, mos, plots, scores = single
    h = scores.finalize().hits.cpu().numpy()
    xy = cloud[:2].astype(np.float64)
    c = plots.centers_host.astype(np.float64)
    d2 = (xy[0][None] - c[:, :1]) ** 2 + (xy[1][None] - c[:, 1:]) ** 2             # (P,T)
    discs = (d2 <= float(a.diam_meters // 2) ** 2).sum(0)
    assert (h <= discs).all() and (discs == 0).any()                             # a hit per kept disc at most; none outside all discs
    assert (h[discs == 0] == 0).all() and (discs[h > 0] >= 1).all()


@pytest.fixture(scope="module")
def three():
    a = make_args(cuda=0, subsample_size=1024)
    clouds = [small_parcel(k) for k in range(3)]
    torch.manual_seed(3)
    return a, clouds, PointNet2(a).eval()


def test_three_parcels_in_shared_batches_equal_the_parcels_one_by_one(three):
    a, clouds, model = three
    atlas, plots, scores = parcel.predict_parcels(model, clouds, a, batch_size=512, seed=SEED, fps_start=0, points=True)
    T = [c.shape[1] for c in clouds]
    assert scores.T == sum(T) and np.array_equal(plots.point_start, np.concatenate([[0], np.cumsum(T)]))
    assert len(parcel.predict_parcels(model, clouds, a, batch_size=512, seed=SEED, fps_start=0)) == 2
    (s, w, h), rec = restated(model, plots, a, sum(T), 7)                         # batches of seven cut across the parcels
    assert any(len(set(r["col_base"].tolist())) > 1 for r in rec)
    whole = scores.finalize()
    assert whole.scores.cpu().numpy().tobytes() == s.tobytes() and whole.weight.cpu().numpy().tobytes() == w.tobytes()
    assert np.array_equal(whole.hits.cpu().numpy(), h)
    for k in range(3):
        mos, pl, one = parcel.predict_parcel_cloud(model, clouds[k], a, batch_size=16, key_base=k << 32, points=True, **KW)
        mine = scores.parcel(k)
        assert mine.scores.shape == (8, T[k]) and int(one.finalize().hits.sum()) > 1000
        for x, y in zip(score_words(mine), score_words(one.finalize())):
            assert np.array_equal(x, y), k
        mean, wsum = atlas.mosaic(k)
        assert np.array_equal(words(mean), words(mos.mean)) and np.array_equal(words(wsum), words(mos.wsum)), k
    with pytest.raises(ValueError):
        one.parcel(0)                                                             # the scores of one parcel have no parcels


def test_lidar_only_model_runs_the_same_path():
    a = make_args(cuda=0, subsample_size=1024, n_input_feats=6)
    cloud = small_parcel(5)
    torch.manual_seed(4)
    model = PointNet2(a).eval()
    mos, plots, scores = parcel.predict_parcel_cloud(model, cloud, a, batch_size=64, points=True, **KW)
    (s, w, h), _ = restated(model, plots, a, cloud.shape[1], 64)
    res = scores.finalize()
    assert h.max() >= 2 and np.array_equal(res.hits.cpu().numpy(), h)
    assert res.scores.cpu().numpy().tobytes() == s.tobytes() and res.weight.cpu().numpy().tobytes() == w.tobytes()
