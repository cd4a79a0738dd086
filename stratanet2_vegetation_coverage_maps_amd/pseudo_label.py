"""Pseudo-labelling on the device -- counterpart of the reference's `predict.py --task pseudo_labelling` (`predict.py:104-111,
131-134`, `inference/predict_utils.py:62-71`): the plots of unlabelled parcels that have more than 2000 points get the plot-wise
coverages of an eval forward as their `coverages`, and the result is the data set `main_SSL.py` pre-trains on.  Here the plots
never leave the device: a parcel is prepared (`parcel.prepare_parcel`), predicted (`label_plots`) and appended to a growable
`train_data.ResidentPlots` (`sn2_plots_append`, one launch), which `train_data.EpochFeeder` trains from as from any resident set.

    dataset = ResidentPlots.empty(point_capacity, plot_capacity, device)
    for cloud in parcels:
        plots, n = pseudo_label_parcel(model, cloud, args, dataset, shape=rings)
    train_ids, val_ids = pretrain_split(dataset.P)                                        # main_SSL.py:70-71
    kde = KdeTables.from_plots(dataset.raw, device, offsets=dataset.offsets)              # the mixture, fitted without a copy
    feeder = EpochFeeder(dataset, args, batch_size, seed, kde=kde, plot_subset=train_ids)
    evaluate(model, dataset.eval_batches(val_ids, args, batch_size, kde=kde), args, kde=kde)

The labels are this package's predictions on its own subsample draws (`ParcelPlots.batches`: sn2_subsample with sampler="device"),
not the reference's numpy draws.  Out of scope: the `main_SSL.py` driver itself (comet, pickles, logging), LAS reading.
"""
from collections import deque

import numpy as np
import torch

from .parcel import ParcelPlots, polygon_keep, prepare_parcel, shape_buffer
from .project_to_2d import project_batch_to_2d_rasters, project_to_plotwise_coverages
from .train_data import ResidentPlots, plan_append

MIN_POINTS_NB_FOR_PSEUDO_LABELLING = 2000        # inference/predict_utils.py:65: kept iff N_points_in_cloud > 2000


def label_plots(model, plots: ParcelPlots, args, batch_size: int = 64, rs=np.random, fps_start=None, sampler="device", seed=None,
                n_live: bool = True, prefetch: int = 3, mosaic=None) -> torch.Tensor:
    """The plot-wise coverages (len(plots),4) fp32 [low, soil, medium, high] of an eval forward over `plots.batches(args,
    batch_size, rs, fps_start, sampler, seed, n_live)`, on the device: per batch `project_to_plotwise_coverages` of the model's
    point-wise coverages, written into the rows of ONE table.  The geometry passes run `prefetch` batches ahead on side streams
    with `model.p2_diam_pix = args.diam_pix` (they leave the projection's pixel ids; restored afterwards), as under
    `evaluation.evaluate`.  `torch.no_grad()`; `model.training` is restored on return, also when a batch raises.  No
    device-to-host read anywhere.
    mosaic: a `inference.ParcelMosaic` -- the same forward also feeds `project_batch_to_2d_rasters` + `mosaic.add`, the loop of
    `inference.predict_parcel`: one pass over a parcel gives both of `predict.py`'s products."""
    dev = plots.raw.device
    labels = torch.empty(len(plots), 4, dtype=torch.float32, device=dev)
    if len(plots) == 0:
        return labels
    batches = plots.batches(args, batch_size, rs, fps_start, sampler, seed, n_live)
    was_training = model.training
    had_p2 = "p2_diam_pix" in model.__dict__
    old_p2 = model.__dict__.get("p2_diam_pix")
    it = iter(batches)
    window = deque()                       # (batch, geometry handle or None), oldest first
    issued = 0
    row = 0

    def fill():
        nonlocal issued
        while len(window) < max(1, prefetch):
            b = next(it, None)
            if b is None:
                return
            geo = model.prefetch_geometry(b, lane=issued % prefetch) if prefetch > 0 else None
            window.append((b, geo))
            issued += 1

    try:
        model.eval()
        model.p2_diam_pix = int(args.diam_pix)
        with torch.no_grad(), torch.cuda.device(dev):
            fill()
            while window:
                cur, geo = window.popleft()
                fill()
                cd = dict(cur)
                if geo is not None:
                    cd["geometry"] = geo
                cov, _ = model(cd)
                clouds_dev = model._last_cloud_dev[1]
                model._last_cloud_dev = None
                B = clouds_dev.shape[0]
                labels[row:row + B].copy_(project_to_plotwise_coverages(cov, clouds_dev, args, geometry=geo))
                if mosaic is not None:
                    rasters, _ = project_batch_to_2d_rasters(clouds_dev, cov, args)
                    mosaic.add(rasters, cur["plot_center"])
                row += B
    finally:
        model.train(was_training)
        if had_p2:
            model.p2_diam_pix = old_p2
        else:
            model.__dict__.pop("p2_diam_pix", None)
    return labels


def pseudo_label_parcel(model, parcel_cloud, args, dataset: ResidentPlots, min_points: int = MIN_POINTS_NB_FOR_PSEUDO_LABELLING,
                        shape=None, keep=None, centers=None, **label_kw):
    """One parcel into `dataset`: `prepare_parcel(..., min_points=min_points + 1)` -- the plots the reference's filter would drop
    (`n_points <= min_points`) are never extracted or predicted --, `label_plots(model, plots, args, **label_kw)`,
    `dataset.append(plots, labels, min_points=min_points)` -> (the parcel's ParcelPlots, the number of plots appended).
    shape / keep / centers: as `parcel.predict_parcel_cloud`.  A parcel without a kept plot returns 0 and launches nothing after
    the count; a parcel that does not fit the set's capacity raises ValueError before its plots are predicted."""
    min_points = int(min_points)
    if shape is not None and keep is None:
        keep = polygon_keep(shape, shape_buffer(args))
    plots = prepare_parcel(parcel_cloud, args, centers=centers, keep=keep, device=dataset.device, min_points=min_points + 1)
    if len(plots) == 0:
        return plots, 0
    plan_append(plots.n_points, None, min_points, dataset.P, dataset.n_filled, dataset.point_capacity, dataset.plot_capacity)
    labels = label_plots(model, plots, args, **label_kw)
    return plots, dataset.append(plots, labels, min_points=min_points)


def pretrain_split(P: int):
    """The split of `main_SSL.py:70-71`: the last min(int(0.2 P), 100) plots validate, the others train -> (train_ids, val_ids)."""
    P = int(P)
    n_val = min(int(0.2 * P), 100)
    return np.arange(P - n_val), np.arange(P - n_val, P)
