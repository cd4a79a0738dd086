"""Cross-validation on the device -- counterpart of the reference's top-level program (`main.py:61-137`): `KFold(n_splits=args.folds,
shuffle=True, random_state=42)` over the labelled plots, `train_full` per fold (`learning/train.py:82-177`), and then
`post_cross_validation_logging` (`learning/accuracy.py:463-509`), which turns the folds' per-plot predictions into the published
figures -- MAE / MAE2 / MAE3, Acc / Acc2 / Acc3 per stratum and the 8 x 8 confusion matrices, plain and "with the 10-point margin" --
once with the ground truths relabelled to their class centres and once with the original labels.

    plots = ResidentPlots.from_dataset(dataset, device)
    relabelled, original, (train_dicts, val_dicts) = cross_validate(plots, args, make_model, kde=tables)
    relabelled.means["acc2_all"], relabelled.confusion("veg_b", normalize="true", margin=True)

`kfold_indices` restates sklearn's split (no sklearn at run time).  `indicators` is ONE `hip_ops.cv_indicators` call (two launches:
include/strata_hip.h, sn2_cv_indicators -- the arithmetic, the tie rule and the layout are stated there) over the (P,4) predictions
and ground truths that `evaluation.evaluate_table` leaves on the device, and ONE device-to-host read of 445 doubles, whatever P; the
per-plot tables are read only when `rows()`, `classes()` or `to_records()` ask for them.

The reference's two oddities are kept as written: `acc_all` is the mean of veg_b and veg_moy only (`accuracy.py:169`), and
`error3_all` takes `error2_veg_moy` (`accuracy.py:242`).  With a continuous ground truth (one that is no class centre after
`round(3)`) the reference raises KeyError and keeps the five MAE columns only; here those rows' class-based entries are NaN,
`class_based` is False and the class-based means are dropped.

Not reproduced: comet logging, the matplotlib figures (`ConfusionMatrixDisplay`), `create_predictions_interpretations`, training
several folds at once on one card.
"""
import numpy as np
import torch

from . import hip_ops as ops
from .evaluation import SUMMARY_KEYS, evaluate, evaluate_table

STRATA = ("veg_b", "veg_moy", "veg_h")
# learning/accuracy.py:13 -- the class centres (include/strata_hip.h states the borders)
BINS_CENTERS = (0.0, 0.10, 0.25, 0.33, 0.50, 0.75, 0.90, 1.0)


def _ten(suffix):
    return ([f"error{suffix}_{s}" for s in STRATA] + [f"error{suffix}_veg_b_and_moy", f"error{suffix}_all"] +
            [f"acc{suffix}_{s}" for s in STRATA] + [f"acc{suffix}_veg_b_and_moy", f"acc{suffix}_all"])


# the 30 columns of a per-plot row, in the order the reference adds them to its frame (V1, V2, V3)
COLUMNS = tuple(_ten("") + _ten("2") + _ten("3"))
# what survives a continuous ground truth: calculate_performance_indicators_V1's MAE block
CONTINUOUS_COLUMNS = COLUMNS[:5]


def kfold_indices(P: int, n_splits: int, seed: int = 42):
    """`sklearn.model_selection.KFold(n_splits, shuffle=True, random_state=seed).split(range(P))` -> [(train_idx, val_idx)], int64
    arrays, both ascending: `np.random.RandomState(seed).shuffle(arange(P))`, cut into n_splits runs of P // n_splits (+1 for the
    first P % n_splits), each run's plots validate one fold."""
    P, n_splits = int(P), int(n_splits)
    if n_splits < 2:
        raise ValueError("kfold_indices: at least 2 splits")
    if n_splits > P:
        raise ValueError(f"kfold_indices: {n_splits} splits of {P} plots")
    order = np.arange(P)
    np.random.RandomState(seed).shuffle(order)
    sizes = np.full(n_splits, P // n_splits, dtype=np.int64)
    sizes[:P % n_splits] += 1
    folds, start = [], 0
    for n in sizes:
        mask = np.zeros(P, dtype=bool)
        mask[order[start:start + n]] = True
        folds.append((np.flatnonzero(~mask).astype(np.int64), np.flatnonzero(mask).astype(np.int64)))
        start += int(n)
    return folds


def closest_class(y):
    """`get_closest_class_center_index` by this project's rule (include/strata_hip.h): the first class that minimises |c[k] - y|,
    the lower class on an exact tie, 0 for NaN.  Host, numpy; `to_records` relabels its ground-truth columns with it."""
    y = np.asarray(y, dtype=np.float64)
    return np.argmin(np.abs(np.asarray(BINS_CENTERS) - y[..., None]), axis=-1)       # argmin: the first minimum; all NaN: 0


class CrossValReport:
    """What `post_cross_validation_logging` computes for one labelling, from the `stats` block of sn2_cv_indicators (already on the
    host) and the per-plot tables (still on the device).

    means: {column: mean over the plots}, NaN entries skipped as `DataFrame.mean()` skips them (a column without an entry: NaN);
        with a continuous ground truth only CONTINUOUS_COLUMNS (`class_based` False).
    counts: {column: the entries that were not NaN};  n_plots;  n_continuous: rows with a ground truth that is no class centre.
    pred (P,4) fp32, gt (P,4) fp64 (as given: before relabelling and rounding), plot_ids, fold_id: the device tensors it was made of."""

    def __init__(self, stats, rows, cls, pred, gt, relabel, fold_id=None, plot_ids=None):
        stats = np.asarray(stats, dtype=np.float64)
        C = ops.CV_COLUMNS
        self.sums = stats[:C].copy()
        self._counts = stats[C:2 * C].astype(np.int64)
        self._cm = stats[2 * C:2 * C + 384].astype(np.int64).reshape(2, 3, 8, 8)
        self.n_continuous = int(stats[2 * C + 384])
        self.class_based = self.n_continuous == 0
        self.n_plots = int(pred.shape[0])
        self.relabel = bool(relabel)
        self._rows, self._cls, self.pred, self.gt, self.fold_id, self.plot_ids = rows, cls, pred, gt, fold_id, plot_ids
        names = COLUMNS if self.class_based else CONTINUOUS_COLUMNS
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(self._counts > 0, self.sums / np.maximum(self._counts, 1), np.nan)
        self.means = {n: float(mean[j]) for j, n in enumerate(names)}
        self.counts = {n: int(self._counts[j]) for j, n in enumerate(names)}

    def confusion(self, strata, normalize=None, margin=False):
        """`compute_confusion_matrix(args, df, strata)` with `args.normalize_cm = normalize`: (8,8), true class x predicted class
        (closest class centres); margin: of `adjust_predictions_based_on_margin(df)`, the "confusion_10pp" matrices.  None: int64
        counts; "true" / "pred" / "all": divided by the row sums / column sums / total as sklearn does, 0 / 0 = 0."""
        s = STRATA.index(strata) if isinstance(strata, str) else int(strata)
        cm = self._cm[1 if margin else 0, s]
        if normalize is None:
            return cm.copy()
        if normalize not in ("true", "pred", "all"):
            raise ValueError("normalize must be None, 'true', 'pred' or 'all'")
        den = {"true": cm.sum(axis=1, keepdims=True), "pred": cm.sum(axis=0, keepdims=True), "all": cm.sum()}[normalize]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.nan_to_num(cm / den)

    def rows(self):
        """The (P,30) per-plot table (COLUMNS), read from the device: O(P)."""
        return self._rows.cpu().numpy()

    def classes(self):
        """(P,9) int32: true class per stratum, predicted class per stratum, class of the margin-adjusted prediction per stratum."""
        return self._cls.cpu().numpy()

    def to_records(self, plot_ids=None):
        """The rows of `PCC_inference_all_placettes_*.csv` as dicts: pl_id, the four predictions, the four ground truths as the
        reference's frame holds them at that point (relabelled to their class centres if this report is; the three strata rounded to
        3 decimals), fold_id when known, then COLUMNS (CONTINUOUS_COLUMNS with a continuous ground truth).  plot_ids: P names; None:
        the report's own `plot_ids`, or 0 .. P-1.  Reads the per-plot tables: O(P)."""
        P = self.n_plots
        if plot_ids is None:
            plot_ids = self.plot_ids if self.plot_ids is not None else range(P)
        if isinstance(plot_ids, torch.Tensor):
            plot_ids = plot_ids.cpu().tolist()
        plot_ids = list(plot_ids)
        if len(plot_ids) != P:
            raise ValueError(f"to_records: {len(plot_ids)} names for {P} plots")
        pred, gt, rows = self.pred.cpu().numpy(), self.gt.cpu().numpy().astype(np.float64), self.rows()
        if self.relabel:
            gt = np.asarray(BINS_CENTERS)[closest_class(gt)]
        gt[:, [0, 2, 3]] = np.rint(gt[:, [0, 2, 3]] * 1000) / 1000
        fold = None if self.fold_id is None else torch.as_tensor(self.fold_id).cpu().tolist()
        names = COLUMNS if self.class_based else CONTINUOUS_COLUMNS
        out = []
        for i in range(P):
            r = {"pl_id": plot_ids[i]}
            r.update(zip(SUMMARY_KEYS[2:6], (float(x) for x in pred[i])))
            r.update(zip(SUMMARY_KEYS[6:10], (float(x) for x in gt[i])))
            if fold is not None:
                r["fold_id"] = fold[i]
            r.update((n, float(rows[i, j])) for j, n in enumerate(names))
            out.append(r)
        return out


def indicators(pred, gt, relabel, fold_id=None, plot_ids=None) -> CrossValReport:
    """pred (P,4) plot-wise predictions (fp32, or the exact fp64 widening that `evaluate_table` keeps), gt (P,4) ground truths, both on
    the device -> the report.  relabel: the ground truths are first moved to their closest class centres (`main.py:102-109`: the
    "relabeled_summary"); False: as they are (the "summary").  One `hip_ops.cv_indicators` call and one read of its `stats`."""
    if not (isinstance(pred, torch.Tensor) and pred.is_cuda and isinstance(gt, torch.Tensor) and gt.is_cuda):
        raise ops.StrataHipError("cross_validation.indicators runs on the HIP device")
    with torch.cuda.device(pred.device):
        pred32 = pred.detach().to(torch.float32).contiguous()
        gt64 = gt.detach().to(torch.float64).contiguous()
        rows, cls, stats = ops.cv_indicators(pred32, gt64, relabel)
        host = stats.cpu().numpy()                                         # the ONE read
    return CrossValReport(host, rows, cls, pred32, gt64, relabel, fold_id=fold_id, plot_ids=plot_ids)


def plain_epoch(model, opt, feeder, epoch, args):
    """The default `trainer` of `cross_validate`: one epoch of `learning/train.py:train` as a plain per-step loop -- the batch from
    `ResidentPlots.fill` (the feeder's ids of epoch `epoch` - 1, its seed and KDE tables), the forward, `losses.projected_total_loss`,
    the backward, `FlatAdam.step` -- -> the reference's train loss dict (the epoch means from the optimiser's device meter: one
    read per epoch).  `args.current_step_in_fold` advances by the epoch's steps."""
    from . import losses
    plots, B, N = feeder.plots, feeder.B, int(args.subsample_size)
    dev = plots.device
    out = {"cloud": torch.empty(B, 10, N, dtype=torch.float32, device=dev), "xyz": torch.empty(B, 3, N, dtype=torch.float32, device=dev),
           "gt": torch.empty(B, 4, dtype=torch.float64, device=dev), "fps_start": torch.empty(2, B, dtype=torch.int32, device=dev)}
    if feeder.kde is not None:
        out["pdf"] = torch.empty(B * N, 3, dtype=torch.float64, device=dev)
    if float(args.m) != 0.0 and feeder.kde is None:
        raise ValueError("cross_validate: args.m != 0 needs the KDE tables (kde=)")
    pdf = out["pdf"] if feeder.kde is not None else torch.ones(B * N, 3, dtype=torch.float64, device=dev)
    model.train()
    with torch.cuda.device(dev):
        opt.meter_reset()
        first = (epoch - 1) * feeder.steps_per_epoch
        for k in range(feeder.steps_per_epoch):
            ids = feeder.batch_ids(first + k)
            plots.fill(ids.to(dev, non_blocking=True), epoch - 1, feeder.seed, args, out, train=feeder.train, noise=feeder.noise,
                       kde=feeder.kde)
            opt.zero_grad()
            cov, proba = model({"cloud": out["cloud"], "xyz": out["xyz"], "fps_start": out["fps_start"]})
            loss, parts, _ = losses.projected_total_loss(cov, proba, out["cloud"], out["gt"], pdf, args, model=model)
            opt.track(loss, *parts)
            loss.backward()
            opt.step()
        meter = opt.meter_read()
    args.current_step_in_fold = getattr(args, "current_step_in_fold", 0) + meter["steps"]
    total, l_abs, l_log = meter["means"][:3]
    return {"total_loss": total, "MAE_loss": l_abs, "log_loss": l_log, "step": args.current_step_in_fold}


def cross_validate(plots, args, make_model, trainer=None, kde=None, batch_size=None, seed=42):
    """`main.py:cross_validate` over a resident plot set -> (relabelled report, original-label report, (per-fold train loss-dict
    lists, per-fold validation loss-dict lists)).

    plots: a complete `train_data.ResidentPlots`; args: the reference's Namespace fields -- folds, n_epoch, n_epoch_test,
    epoch_to_start_early_stop, use_early_stopping, patience_in_epochs, lr, wd, step_size, lr_decay, batch_size, stats_path (the
    checkpoints of `save_state` go there) beside what the model and the feed read; make_model(args) -> a fresh model on the plots'
    device, called once per fold (`initialize_model`); kde: `losses.KdeTables` for the NLL term (needed when args.m != 0).
    trainer(model, opt, feeder, epoch, args) -> the epoch's train loss dict; None: `plain_epoch`.  The feeder of a fold is
    `EpochFeeder(plots, args, batch_size, seed, kde=kde, plot_subset=train_idx)`; `opt` is `FlatAdam(model, lr=args.lr,
    weight_decay=args.wd)` and the schedule `optim.StepLR(opt, args.step_size, args.lr_decay)` (`get_optimizers`).
    The folds are `kfold_indices(plots.P, args.folds, seed)`; the validation plots go through `plots.eval_batches(val_idx, ...)`.

    Per fold, `train_full`'s schedule: epochs 1 .. n_epoch; after an epoch's training, `evaluation.evaluate` when epoch %
    n_epoch_test == 0 or epoch > epoch_to_start_early_stop (its dict, with "epoch", joins the fold's validation list), then
    `model.stop_early(total_loss, epoch, args)` when args.use_early_stopping (True: the fold's training ends); no scheduler step
    after the last epoch; then `load_best_state` (early stopping) or `save_state`, and the final evaluation by `evaluate_table`: its
    (P_fold,15) table stays on the device.  The folds' tables are concatenated there, and each report is one `indicators` call:
    the per-plot predictions are never read.  `args.current_fold_id`, `current_epoch`, `current_step_in_fold` are set as the
    reference sets them."""
    from .optim import FlatAdam, StepLR
    from .train_data import EpochFeeder
    B = int(batch_size if batch_size is not None else args.batch_size)
    trainer = trainer or plain_epoch
    folds = kfold_indices(plots.P, args.folds, seed)
    dev = plots.device
    tables, ids, fold_of = [], [], []
    train_lists, val_lists = [], []
    for fold_id, (train_idx, val_idx) in enumerate(folds, start=1):
        args.current_fold_id = fold_id
        args.current_step_in_fold = 0
        model = make_model(args)
        opt = FlatAdam(model, lr=args.lr, weight_decay=args.wd)
        sched = StepLR(opt, args.step_size, args.lr_decay)
        feeder = EpochFeeder(plots, args, B, seed, kde=kde, plot_subset=train_idx)
        train_dicts, val_dicts = [], []
        for epoch in range(1, int(args.n_epoch) + 1):
            args.current_epoch = epoch
            d = trainer(model, opt, feeder, epoch, args)
            d["epoch"] = epoch
            train_dicts.append(d)
            if epoch % int(args.n_epoch_test) == 0 or epoch > args.epoch_to_start_early_stop:
                v, _ = evaluate(model, plots.eval_batches(val_idx, args, B, seed=seed, kde=kde), args, kde=kde)
                v["epoch"] = epoch
                val_dicts.append(v)
                if args.use_early_stopping and model.stop_early(v["total_loss"], epoch, args):
                    break
            if epoch == int(args.n_epoch):
                break
            sched.step()
        if args.use_early_stopping:
            model.load_best_state(args)
        else:
            model.save_state(args)
        table, names, _ = evaluate_table(model, plots.eval_batches(val_idx, args, B, seed=seed, kde=kde), args, kde=kde)
        tables.append(table)
        ids += [x.to(dev) if isinstance(x, torch.Tensor) else torch.as_tensor(list(x), device=dev) for x in names]
        fold_of.append(torch.full((table.shape[0],), fold_id, dtype=torch.int32, device=dev))
        train_lists.append(train_dicts)
        val_lists.append(val_dicts)
    with torch.cuda.device(dev):
        table = torch.cat(tables, 0)
        plot_ids = torch.cat([x.reshape(-1) for x in ids])
        fold_of = torch.cat(fold_of)
        pred, gt = table[:, 7:11].to(torch.float32).contiguous(), table[:, 11:15].contiguous()
        relabelled = indicators(pred, gt, True, fold_id=fold_of, plot_ids=plot_ids)
        original = indicators(pred, gt, False, fold_id=fold_of, plot_ids=plot_ids)
    return relabelled, original, (train_lists, val_lists)


__all__ = ["kfold_indices", "indicators", "CrossValReport", "cross_validate", "plain_epoch", "closest_class", "COLUMNS", "STRATA",
           "BINS_CENTERS", "CONTINUOUS_COLUMNS"]
