"""Pseudo-labelling a parcel into a resident training set on one GPU (pseudo_label.py): the synthetic 10 ha parcel of
scripts/bench_parcel.py at 40 points/m^2, plots above 2000 points kept.  Prints ONE JSON line; every figure is the median of
--repeats runs after a warm-up, with its range (min, max).

    python scripts/bench_pseudo_label.py [--batch 64] [--repeats 7] [--host-repeats 3]

Timed (host clock around work that ends in a device synchronise, but `append_ms`: HIP events around the one launch):
  prepare_ms        prepare_parcel(min_points=2001)
  label_ms          label_plots over the prepared plots (sampler="device", fps_start=0)
  append_ms         ResidentPlots.append of all of them into an arena allocated beforehand (one sn2_plots_append launch)
  total_ms          pseudo_label_parcel end to end
  mosaic_ms         predict_parcel_cloud (+ finalize) at the same batch size and sampler in the same session: the mosaic
                    task, prepare included -- what total_ms should be in the neighbourhood of (total_over_mosaic)
  host_route_ms     what a user had before: every plot of ParcelPlots.raw and the labels read back with .cpu(), then
                    ResidentPlots.from_plots (host torch.cat + one upload); prepare and label are NOT in it -- compare it with
                    append_ms
  append_GBps       80 B per appended point (40 read, 40 written) over append_ms, beside copy_GBps: a device `copy_` between two
                    buffers of the appended plots' bytes (the same 80 B per point) timed in the same run with the same events
The labels are this package's predictions on its own subsample draws, not the reference's numpy draws."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stratanet2_vegetation_coverage_maps_amd import PointNet2, parcel  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd.pseudo_label import (MIN_POINTS_NB_FOR_PSEUDO_LABELLING, label_plots,  # noqa: E402
                                                                  pseudo_label_parcel)
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_parcel  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd.train_data import ResidentPlots  # noqa: E402


def stat(v, digits=3):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def ev_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--side", type=float, default=316.3, help="side of the square parcel in metres (316.3: 10 ha)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pseudo_label: needs the GPU")
    dev = torch.device("cuda:0")
    args = make_args(cuda=0)
    torch.manual_seed(0)
    model = PointNet2(args).eval()
    m = MIN_POINTS_NB_FOR_PSEUDO_LABELLING
    kw = dict(batch_size=a.batch, fps_start=0, sampler="device", seed=1)
    cloud = make_parcel(a.side, a.side, density=40.0, seed=1)
    cloud_dev = torch.from_numpy(cloud).to(dev)

    def prepare():
        return parcel.prepare_parcel(cloud_dev, args, min_points=m + 1)
    plots = prepare()
    P, SN = len(plots), int(plots.n_points.sum())
    cap = (SN + 1024, P + 8)
    labels = label_plots(model, plots, args, **kw)

    def mosaic():
        return parcel.predict_parcel_cloud(model, cloud_dev, args, **kw)[0].finalize()

    def total():
        return pseudo_label_parcel(model, cloud_dev, args, ResidentPlots.empty(*cap, dev), min_points=m, **kw)[1]

    def host_route():
        off = np.concatenate([[0], np.cumsum(plots.n_points)])
        raw = [plots.raw[:, off[j]:off[j + 1]].cpu() for j in range(P)]
        return ResidentPlots.from_plots(raw, plots.centers_host, labels.cpu().numpy().astype(np.float64), dev)

    def append_once():
        ds = ResidentPlots.empty(*cap, dev)
        return ev_ms(lambda: ds.append(plots, labels))[0], ds

    # warm-up of every timed shape (code objects, allocator), and the two routes must build the same set
    total(), mosaic()
    _, ds = append_once()
    host = host_route()
    same = (ds.P == host.P and torch.equal(ds.raw[:, :ds.n_filled].view(torch.int32), host.raw.view(torch.int32)) and
            torch.equal(ds.offsets, host.offsets) and torch.equal(ds.coverages, host.coverages))
    del ds, host
    src, dst = (torch.empty(10, SN, dtype=torch.float32, device=dev) for _ in range(2))
    src.zero_()
    ev_ms(lambda: dst.copy_(src))

    t = {k: [] for k in ("prepare", "label", "append", "total", "mosaic", "copy")}
    for _ in range(a.repeats):                                   # alternated, so that drift hits every quantity alike
        t["prepare"].append(wall_ms(prepare)[0])
        t["label"].append(wall_ms(lambda: label_plots(model, plots, args, **kw))[0])
        t["append"].append(append_once()[0])
        t["copy"].append(ev_ms(lambda: dst.copy_(src))[0])
        t["total"].append(wall_ms(total)[0])
        t["mosaic"].append(wall_ms(mosaic)[0])
    t["host_route"] = [wall_ms(host_route)[0] for _ in range(a.host_repeats)]
    moved = 80 * SN
    out = {"metric": "10 ha parcel pseudo-labelled into a resident set (pseudo_label_parcel, median)",
           "value": stat(t["total"])["median"], "unit": "ms", "n_gpus": 1, "batch": a.batch, "repeats": a.repeats,
           "points": int(cloud.shape[1]), "plots_kept": P, "plot_points": SN, "min_points": m, "routes_build_the_same_set": bool(same),
           "prepare_ms": stat(t["prepare"]), "label_ms": stat(t["label"]), "append_ms": stat(t["append"], 4),
           "total_ms": stat(t["total"]), "mosaic_ms": stat(t["mosaic"]),
           "total_over_mosaic": round(statistics.median(t["total"]) / statistics.median(t["mosaic"]), 3),
           "host_route_ms": stat(t["host_route"]), "host_route_repeats": a.host_repeats,
           "host_route_over_append": round(statistics.median(t["host_route"]) / statistics.median(t["append"]), 1),
           "append_bytes": moved,
           "append_GBps": stat([moved / (ms * 1e-3) / 1e9 for ms in t["append"]], 1),
           "copy_GBps": stat([moved / (ms * 1e-3) / 1e9 for ms in t["copy"]], 1),
           "plots_per_s_total": round(P / (statistics.median(t["total"]) * 1e-3), 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
