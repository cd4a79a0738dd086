"""cross_validation.cross_validate and evaluation.evaluate_table on the device: `evaluate` is `evaluate_table` + one read +
`aggregate`; a 3-fold cross-validation of 12 synthetic resident plots follows `train_full`'s schedule, validates every plot in exactly
one fold, and returns the reports that the numpy restatement (tests/_cv_indicators_ref.py) gives for the concatenated tables.

Plot and batch sizes of tests/test_gpu_train_feed.py's pipeline test (4096 points, batches of 2).  Trained weights are not compared
from run to run: the backward pass adds two of its gradient vectors with float atomics."""
import numpy as np
import pytest
import torch

import _cv_indicators_ref as R
from oracle import network
from stratanet2_vegetation_coverage_maps_amd import PointNet2, cross_validate, evaluation, kfold_indices, losses
from stratanet2_vegetation_coverage_maps_amd.cross_validation import COLUMNS, plain_epoch
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_raw_plot
from stratanet2_vegetation_coverage_maps_amd.train_data import ResidentPlots

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, B, P, FOLDS = 4096, 2, 12, 3


@pytest.fixture(scope="module")
def world():
    sizes = (3000, 5000, N - 316, 6000, 2500, 4500, 3900, 3300, 5200, 2800, 4100, 3600)
    centers = np.array([[100.0 + 25 * p, 300.0 - 25 * p] for p in range(P)], dtype=np.float32)
    raw = [make_raw_plot(m, 900 + p, centers[p]) for p, m in enumerate(sizes)]
    rng = np.random.RandomState(4)
    cov = R.C[rng.randint(0, 8, (P, 4))]
    cov[1::2] = np.clip(cov[1::2] + 0.004, 0.0, 1.0)              # every other plot: a continuous ground truth near its centre
    plots = ResidentPlots.from_plots(raw, centers, cov, DEV)
    kde = losses.KdeTables(np.linspace(-1.0, 30.0, 64), *[np.linspace(0.1, 1.0, 64) ** k for k in (1, 2, 3)], DEV)
    return plots, cov, kde


def _args(tmp_path, **kw):
    return make_args(cuda=0, subsample_size=N, ratio1=0.125, r1=1.0, ratio2=0.25, r2=2.0, stats_path=str(tmp_path), folds=FOLDS,
                     n_epoch=2, n_epoch_test=1, use_early_stopping=False, lr=1e-3, wd=1e-3, step_size=1, lr_decay=0.5, batch_size=B,
                     **kw)


def _make_model(args):
    model = PointNet2(args)
    model.load_state_dict(network.init_state_dict(5))
    return model.cuda().train()


def test_evaluate_is_evaluate_table_plus_aggregate(world, tmp_path):
    plots, cov, kde = world
    args = _args(tmp_path)
    model = _make_model(args)
    ids = [7, 2, 11, 0, 5]
    table, names, counts = evaluation.evaluate_table(model, plots.eval_batches(ids, args, B, seed=3, kde=kde), args, kde=kde)
    assert table.is_cuda and tuple(table.shape) == (5, 15) and table.dtype == torch.float64 and model.training
    assert counts == [N] * 5 and [x.tolist() for x in names] == [[7, 2], [11, 0], [5]]
    t = table.cpu().numpy()
    want, wsumm = evaluation.aggregate(t[:, :7], t[:, 7:11].astype(np.float32), t[:, 11:15], ids, counts)
    got, summ = evaluation.evaluate(model, plots.eval_batches(ids, args, B, seed=3, kde=kde), args, kde=kde)
    assert summ == wsumm and [s["pl_id"] for s in summ] == ids
    assert set(got) == set(want)
    for k in got:
        if k != "per_plot":
            assert got[k] == want[k], k
    assert got["per_plot"]["losses"].tobytes() == want["per_plot"]["losses"].tobytes()
    assert got["per_plot"]["pred"].tobytes() == want["per_plot"]["pred"].tobytes()
    assert np.array_equal(t[:, 11:15], cov[ids]) and np.isfinite(t).all()


def test_three_folds_follow_the_schedule_and_report_the_restatement(world, tmp_path):
    plots, cov, kde = world
    args = _args(tmp_path)
    rates = []

    def trainer(model, opt, feeder, epoch, a):
        rates.append((a.current_fold_id, epoch, opt.lr, feeder.subset.tolist()))
        return plain_epoch(model, opt, feeder, epoch, a)
    relabelled, original, (train_lists, val_lists) = cross_validate(plots, args, _make_model, trainer=trainer, kde=kde, seed=42)
    torch.cuda.synchronize()
    folds = kfold_indices(P, FOLDS, 42)
    # every plot is validated in exactly one fold, the folds are kfold_indices'
    val_order = np.concatenate([v for _, v in folds])
    assert sorted(val_order.tolist()) == list(range(P))
    for rep in (relabelled, original):
        assert rep.plot_ids.cpu().tolist() == val_order.tolist() and rep.n_plots == P
        assert rep.fold_id.cpu().tolist() == [f + 1 for f, (_, v) in enumerate(folds) for _ in v]
        assert np.array_equal(rep.gt.cpu().numpy(), cov[val_order])
    assert [r[3] for r in rates[::2]] == [t.tolist() for t, _ in folds]
    # train_full's schedule: every epoch trains, the evaluated epochs are the rule's, the rate decays between epochs only
    evaluated = [e for e in range(1, args.n_epoch + 1) if e % args.n_epoch_test == 0 or e > args.epoch_to_start_early_stop]
    assert evaluated == [1, 2] and len(train_lists) == len(val_lists) == FOLDS
    steps = (P - P // FOLDS) // B
    for f in range(FOLDS):
        assert [d["epoch"] for d in train_lists[f]] == [1, 2] and [d["step"] for d in train_lists[f]] == [steps, 2 * steps]
        assert [d["epoch"] for d in val_lists[f]] == evaluated and [d["step"] for d in val_lists[f]] == [steps, 2 * steps]
        for d in train_lists[f] + val_lists[f]:
            assert all(np.isfinite(d[k]) for k in ("total_loss", "MAE_loss", "log_loss"))
    assert [(r[0], r[1], r[2]) for r in rates] == [(f, e, 1e-3 * 0.5 ** (e - 1)) for f in (1, 2, 3) for e in (1, 2)]
    assert args.current_fold_id == FOLDS and args.current_epoch == 2
    # both reports are the restatement's of the concatenated tables, read back
    pred, gt = relabelled.pred.cpu().numpy(), relabelled.gt.cpu().numpy()
    assert pred.dtype == np.float32 and pred.shape == (P, 4) and np.isfinite(pred).all()
    assert original.pred.cpu().numpy().tobytes() == pred.tobytes()
    for rep, relabel in ((relabelled, True), (original, False)):
        rows, cls, stats = R.indicators(pred, gt, relabel)
        got = rep.rows()
        nan = np.isnan(rows)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), rows[~nan].view(np.uint64))
        assert np.array_equal(rep.classes(), cls)
        assert rep.n_continuous == stats["continuous"] == (0 if relabel else (val_order % 2 == 1).sum())
        assert rep.class_based == relabel and tuple(rep.means) == (COLUMNS if relabel else COLUMNS[:5])
        for c, name in enumerate(rep.means):
            assert rep.counts[name] == stats["count"][c]
            assert abs(rep.means[name] - stats["sum"][c] / stats["count"][c]) <= 1e-12, name
        for a, margin in enumerate((False, True)):
            for s in range(3):
                assert np.array_equal(rep.confusion(s, margin=margin), stats["cm"][a, s])
                assert rep.confusion(s, margin=margin).sum() == P
        recs = rep.to_records()
        assert [r["pl_id"] for r in recs] == val_order.tolist() and [r["fold_id"] for r in recs] == rep.fold_id.cpu().tolist()
        assert all(r["error_veg_b"] == rows[i, 0] and r["pred_veg_h"] == float(pred[i, 3]) for i, r in enumerate(recs))
        if relabel:
            assert all(r["vt_veg_moy"] in R.C for r in recs)
