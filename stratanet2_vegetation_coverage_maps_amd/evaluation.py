"""Validation pass on the device -- counterpart of the reference's `learning/test.py:evaluate`, the loop that
`learning/train.py:train_full` runs every `n_epoch_test` epochs and whose `"total_loss"` feeds `model.stop_early(...)`.

The reference evaluates with `batch_size=1`: `loss_abs`, `loss_log`, `loss_e` and `get_absolute_loss_by_strata` are numbers of
ONE plot each, averaged over plots by an `AverageValueMeter`, with four `.item()` per plot.  Here a fold is evaluated in batches:

    per batch of plots:  eval forward (geometry prefetched on side streams, as `inference.predict_parcel`)
                         -> (B*N,4) coverages, probabilities -> per-plot losses + plot-wise coverages   [sn2_plot_losses: 2 launches]
    at the end:          ONE device-to-host read of the (P, 7 + 4 + 4) table -> the reference's dict and per-plot summaries

`plot_losses` is the device entry point (csrc/project.hip), `plot_losses_torch` the same quantities in plain torch ops (any
device): the form the tests hold the kernel to.  A plot's row does not depend on the batch it was evaluated in (include/strata_hip.h:
sn2_plot_losses, "batch invariance"), so the result of a fold does not depend on how it was cut into batches.

`evaluate_table` is the same pass without the read: the (P,15) table stays on the device, which is what `cross_validation`
concatenates over the folds and hands to sn2_cv_indicators -- the performance indicators and confusion matrices of
`learning/accuracy.py` (the reference's own module needs `np.float`, which NumPy 1.24 removed).

Not reproduced (out of scope): `create_predictions_interpretations`, comet logging, the matplotlib figures.
The summaries have the keys of `get_cloud_prediction_summary`.
"""
from collections import deque

import numpy as np
import torch

from . import hip_ops as ops
from ._lib import StrataHipError
from .losses import EPS, get_entropy_loss_torch, get_NLL_loss_torch, kde_densities

# columns of a per-plot row
COLUMNS = ("total", "absolute", "NLL", "entropy", "abs_low", "abs_med", "abs_high")
# learning/test.py:121-131 -> column of the row (`entropy_loss`: computed by the reference, dropped from its dict)
LOSS_KEYS = (("total_loss", 0), ("MAE_loss", 1), ("log_loss", 2), ("MAE_veg_b", 4), ("MAE_veg_moy", 5), ("MAE_veg_h", 6),
             ("entropy_loss", 3))
SUMMARY_KEYS = ("pl_id", "pl_N_points", "pred_veg_b", "pred_sol_nu", "pred_veg_moy", "pred_veg_h", "vt_veg_b", "vt_sol_nu",
                "vt_veg_moy", "vt_veg_h")


def project_plot_torch(coverages, cloud, diam_pix: int):
    """`project_to_plotwise_coverages` (model/project_to_2d.py:7-55) of ONE plot in plain torch ops: coverages (N,4), cloud
    (>=2,N) -> (4,) in the dtype of `coverages`.  Pixel ids from the fp32 positions, operation for operation."""
    D = int(diam_pix)
    xy = cloud[:2].to(device=coverages.device, dtype=torch.float32)
    mn = xy.min(dim=1, keepdim=True).values
    mx = xy.max(dim=1, keepdim=True).values
    pix = torch.floor((xy - mn) / (mx - mn + 0.0001) * D).long().clamp_(0, D - 1)
    cell = pix[0] * D + pix[1]
    vals = torch.stack((coverages[:, 0], coverages[:, 2], coverages[:, 3]))                      # (3,N)
    neg = torch.full((3, D * D), float("-inf"), dtype=coverages.dtype, device=coverages.device)
    pm = neg.scatter_reduce(1, cell.unsqueeze(0).expand(3, -1), vals, "amax", include_self=True)
    occ = torch.zeros(D * D, dtype=torch.bool, device=coverages.device).index_fill_(0, cell, True)   # pixels some point fell into
    n_occ = occ.sum().clamp(min=1).to(coverages.dtype)
    zero = torch.zeros((), dtype=coverages.dtype, device=coverages.device)
    low = torch.where(occ, pm[0], zero).sum() / n_occ
    soil = torch.where(occ, 1 - pm[0], zero).sum() / n_occ
    med = torch.where(occ, pm[1], zero).sum() / n_occ
    high = torch.where(occ, pm[2], zero).sum() / n_occ
    return torch.stack((low, soil, med, high))


def plot_losses_torch(coverages_pointwise, proba_pointwise, clouds, gt, pdf_all, args):
    """The per-plot validation losses in plain torch ops, on any device: a loop over plots of the `*_torch` forms of
    `losses.py` on the plot's own rows plus `get_absolute_loss_by_strata` -> (out (B,7) fp64, pred (B,4) in the dtype of the
    coverages).  A term whose weight is zero is skipped (0), as in the kernels; `pdf_all` may then be None."""
    B, _, N = clouds.shape
    m, e = float(args.m), float(args.e)
    rows, preds = [], []
    for b in range(B):
        sl = slice(b * N, (b + 1) * N)
        pred = project_plot_torch(coverages_pointwise[sl], clouds[b], args.diam_pix)
        g = gt[b].to(device=pred.device, dtype=torch.float64)
        d = torch.stack((pred[0], pred[2], pred[3])) - torch.stack((g[0], g[2], g[3]))          # fp64 by type promotion
        by_strata = (d.pow(2) + EPS).pow(0.5)
        l_abs = by_strata.mean()
        zero = torch.zeros((), dtype=torch.float64, device=pred.device)
        l_log = get_NLL_loss_torch(proba_pointwise[sl], pdf_all[sl].to(pred.device)).double() if m != 0.0 else zero
        l_e = get_entropy_loss_torch(proba_pointwise[sl]).double() if e != 0.0 else zero
        total = l_abs + (m * l_log if m != 0.0 else 0.0) + (e * l_e if e != 0.0 else 0.0)
        rows.append(torch.stack((total, l_abs, l_log, l_e, by_strata[0], by_strata[1], by_strata[2])))
        preds.append(pred)
    return torch.stack(rows), torch.stack(preds)


@torch.no_grad()
def plot_losses(coverages_pointwise, proba_pointwise, clouds, gt, pdf_all, args, geometry=None, model=None, out=None):
    """-> (out (B,7) fp64 = per plot [total, absolute, NLL, entropy, abs_low, abs_med, abs_high], pred (B,4) fp32) on the
    device: two launches for the batch (include/strata_hip.h: sn2_plot_losses).  `pred` is `project_to_plotwise_coverages` of the
    same inputs, bit for bit.  With the pixel ids of a geometry pass at hand (`geometry.p2_pix`, made with `model.p2_diam_pix =
    args.diam_pix`) they are used; without them they are computed from `clouds` (`hip_ops.plot_pixels`: the same ids).
    `pdf_all` may be None when `args.m == 0`.  No autograd.  out = (out, pred): caller-owned buffers."""
    from .project_to_2d import _clouds_on_device
    if not (coverages_pointwise.is_cuda and proba_pointwise.is_cuda):
        raise StrataHipError("evaluation.plot_losses runs on the HIP device (plot_losses_torch is the plain torch form)")
    dev = coverages_pointwise.device
    B, N = clouds.shape[0], clouds.shape[2]
    D = int(args.diam_pix)
    m, e = float(args.m), float(args.e)
    if m != 0.0 and pdf_all is None:
        raise ValueError("plot_losses: args.m != 0 needs the densities pdf_all")
    with torch.cuda.device(dev):
        pix = getattr(geometry, "p2_pix", None) if geometry is not None else None
        if pix is not None and (getattr(geometry, "p2_diam_pix", None) != D or pix.numel() != B * N):
            pix = None                                 # ids of another grid or batch
        cache = getattr(model, "_last_cloud_dev", None) if model is not None else None
        if pix is None:
            clouds_dev = _clouds_on_device(clouds, dev, cache)
            _, pix = ops.plot_pixels(clouds_dev, D)
        if cache is not None:
            model._last_cloud_dev = None               # used once: do not keep the batch's clouds alive
        gt = gt.to(device=dev, dtype=torch.float64).contiguous()
        pdf = pdf_all.to(device=dev, dtype=torch.float64).contiguous() if m != 0.0 else None
        return ops.plot_losses(coverages_pointwise.detach().float().contiguous(), pix, proba_pointwise.detach().float().contiguous(),
                               pdf, gt, B, N, D, m, e, out=out)


def aggregate(rows, pred, gt, plot_ids, n_points, step=0):
    """Per-plot rows (P,7), plot-wise predictions (P,4), ground truth (P,4) (host arrays), names and point counts ->
    (loss_dict, summaries) as `learning/test.py:evaluate` returns them (:121-131): every entry the fp64 mean over PLOTS, added
    in plot order (an AverageValueMeter fed one plot at a time) -- not the mean of batch means."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 7)
    pred, gt = np.asarray(pred), np.asarray(gt)
    P = rows.shape[0]
    if P == 0:
        raise ValueError("evaluate: no plots")
    if not (pred.shape == (P, 4) and gt.shape == (P, 4) and len(plot_ids) == P and len(n_points) == P):
        raise ValueError("aggregate: rows, pred, gt, plot_ids and n_points must describe the same plots")
    loss_dict = {}
    for key, col in LOSS_KEYS[:6]:
        loss_dict[key] = sum(rows[:, col].tolist()) / P
    loss_dict["step"] = step
    key, col = LOSS_KEYS[6]
    loss_dict[key] = sum(rows[:, col].tolist()) / P
    loss_dict["per_plot"] = {"losses": rows, "pred": pred, "columns": COLUMNS}
    summaries = []
    for i in range(P):
        v = [plot_ids[i], int(n_points[i])] + [float(x) for x in pred[i]] + [float(x) for x in gt[i]]
        summaries.append(dict(zip(SUMMARY_KEYS, v)))
    return loss_dict, summaries


def _plot_names(ids, first, B):
    if ids is None:
        return list(range(first, first + B))
    if isinstance(ids, torch.Tensor):
        return ids                                     # read at the end, with everything else
    ids = list(ids)
    if len(ids) != B:
        raise ValueError(f"plot_id: {len(ids)} names for {B} plots")
    return ids


def evaluate_table(model, batches, args, kde=None, prefetch=3):
    """The validation pass of `evaluate` (its arguments) WITHOUT its device-to-host read -> (table, names, counts): table (P,15)
    fp64 on the device = per plot the seven COLUMNS, the plot-wise prediction (4, fp32 widened exactly) and the ground truth (4);
    names: per batch its plot names, a list or the batch's "plot_id" tensor as given (not read); counts: P point counts."""
    dev = model.lin1.weight.device
    if dev.type != "cuda":
        raise StrataHipError("evaluation.evaluate needs the model on a HIP device")
    m = float(args.m)
    D = int(args.diam_pix)
    was_training = model.training
    had_p2 = "p2_diam_pix" in model.__dict__
    old_p2 = model.__dict__.get("p2_diam_pix")
    tables, names, counts = [], [], []
    it = iter(batches)
    window = deque()
    issued = 0
    n_plots = 0

    def fill():
        nonlocal issued
        while len(window) < max(1, prefetch):
            b = next(it, None)
            if b is None:
                return
            if m != 0.0 and kde is None and b.get("pdf_all", None) is None:
                raise ValueError("evaluate: args.m != 0 needs the KDE densities: a batch without \"pdf_all\" and no `kde` tables")
            cd = dict(b)
            cd["cloud"] = b["cloud"].to(device=dev, dtype=torch.float32, non_blocking=True).contiguous()
            cd["xyz"] = b["xyz"].to(device=dev, dtype=torch.float32, non_blocking=True).contiguous()
            geo = model.prefetch_geometry(cd, lane=issued % prefetch) if prefetch > 0 else None
            window.append((cd, geo))
            issued += 1

    try:
        model.eval()
        model.p2_diam_pix = D                          # the geometry passes also leave the pixel ids of the projection
        with torch.no_grad(), torch.cuda.device(dev):
            fill()
            while window:
                cd, geo = window.popleft()
                fill()
                if geo is not None:
                    cd["geometry"] = geo
                cov, proba = model(cd)
                clouds_dev = cd["cloud"]
                model._last_cloud_dev = None
                B, _, N = clouds_dev.shape
                pdf = cd.get("pdf_all", None)
                if pdf is None and m != 0.0:
                    pdf = kde_densities(clouds_dev, args.z_max, kde)
                gt = cd["coverages"].to(device=dev, dtype=torch.float64, non_blocking=True).reshape(B, 4).contiguous()
                out, pred = plot_losses(cov, proba, clouds_dev, gt, pdf, args, geometry=geo)
                tables.append(torch.cat((out, pred.double(), gt), 1))       # (B,15) fp64: fp32 -> fp64 is exact
                names.append(_plot_names(cd.get("plot_id", None), n_plots, B))
                counts += [N] * B
                n_plots += B
            if not tables:
                raise ValueError("evaluate: no plots")
            table = torch.cat(tables, 0)
    finally:
        model.train(was_training)
        if had_p2:
            model.p2_diam_pix = old_p2
        else:
            model.__dict__.pop("p2_diam_pix", None)
    return table, names, counts


def evaluate(model, batches, args, kde=None, prefetch=3):
    """`learning/test.py:evaluate` for a fold given as batches -> (loss_dict, summaries).

    batches: iterable of `cloud_data` dicts as the reference's collate makes them: "cloud" (B,10,N), "xyz" (B,3,N), "coverages"
    (B,4), "plot_id" (B names), optionally "pdf_all" (B*N,3), "fps_start" and "n_live" (PointNet2's additive keys, handed on to the
    geometry passes as they are); B and N may differ between batches.
    kde: a `losses.KdeTables`: a batch without "pdf_all" gets its densities from `kde_densities(cloud, args.z_max, kde)`; neither
    given while `args.m != 0` is an error, raised before the batch's first launch.
    prefetch: geometry passes in flight ahead of the feature pass (`PointNet2.prefetch_geometry`), 0 = none.

    Eval-mode forward under `torch.no_grad()`; `model.training` is restored on return, also when a batch raises.  The per-plot
    rows stay on the device until the last batch: ONE device-to-host read, whatever the number of batches.
    loss_dict: the reference's keys (total_loss, MAE_loss, log_loss, MAE_veg_b, MAE_veg_moy, MAE_veg_h, step) = means over
    plots, plus "entropy_loss" and "per_plot" = {"losses" (P,7), "pred" (P,4), "columns"}; summaries: one dict per plot with the
    keys of `get_cloud_prediction_summary`.  `model.stop_early(loss_dict["total_loss"], epoch, args)` is the intended consumer."""
    table, names, counts = evaluate_table(model, batches, args, kde=kde, prefetch=prefetch)
    dev = table.device
    with torch.cuda.device(dev):
        table = table.cpu().numpy()                                         # the ONE read
        ids_dev = [x for x in names if isinstance(x, torch.Tensor)]
        if ids_dev:
            flat = iter(torch.cat([x.reshape(-1).to(dev) for x in ids_dev]).cpu().numpy().tolist())
            names = [[next(flat) for _ in range(x.numel())] if isinstance(x, torch.Tensor) else x for x in names]
    plot_ids = [n for chunk in names for n in chunk]
    return aggregate(table[:, :7], table[:, 7:11].astype(np.float32), table[:, 11:15], plot_ids, counts,
                     step=getattr(args, "current_step_in_fold", 0))
