"""Parcel -> plots -> mosaic on one GPU (parcel.py): synthetic parcels of 10 ha and 1 ha at 40 points/m^2.  Prints one JSON
line: per parcel the device time of `prepare_parcel` (HIP events after warm-up, median of --repeat runs; the cloud's
host-to-device copy separately), its entry points' times, `predict_parcel_cloud` + `finalize` end to end in plots/s, the
prediction alone, the reference's CPU preparation (scipy discs + sklearn z-norm loop) timed on a sample of plots and
EXTRAPOLATED to the parcel, the compulsory bytes of the count / fill passes against 8 TB/s, and the z-norm query's
candidate tests per second.  Kernel times: run it under `rocprofv3 --kernel-trace --stats`.

    python scripts/bench_parcel.py [--repeat 10] [--sample 6] [--batch 64] [--sampler numpy|device] [--fps-live on|off]
                                   [--report [--pairs 5]]

--sampler device draws the plots' subsamples with sn2_subsample instead of numpy on the host (`ParcelPlots.batches`); the
prediction figures are then the median of --repeat runs as well, and sn2_subsample / sn2_prepare_plots are timed per parcel.
--fps-live off drops the batches' "n_live" key (sn2_fps_live: the FPS kernels then sample over the repeated points of short plots
as before): the same predictions, a cross-check inside one build.
--report adds, per parcel, `predict_parcel_cloud(shape=rings)` + `ParcelMosaic.report(rings)` (crop to the polygon and band means
on the device, one read of 88 bytes) against the same prediction followed by the host path a user had before: `finalize()`, the
mosaic copied to the host, `polygon_keep(rings, 0)` over the pixel centres, mask, `np.nanmean`.  The two are run alternately,
--pairs times each; medians and ranges of the whole and of the tail after the prediction.  The polygon is the parcel's bounding
box shrunk by 5 m.  Without --report nothing of this runs and the output is what it was.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stratanet2_vegetation_coverage_maps_amd import PointNet2, hip_ops as ops, parcel  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_parcel  # noqa: E402

HBM = 8e12


def ev_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def reference_cpu(cloud, centers, sample, args, rng):
    """The reference's rule on `sample` plots: cKDTree build (once), query_ball_point, sklearn radius_neighbors + the
    per-point np.min loop (utils/load_data.py:237-249).  Returns (tree build s, mean s per plot)."""
    from scipy.spatial import cKDTree
    from sklearn.neighbors import NearestNeighbors
    t = time.perf_counter()
    tree = cKDTree(cloud[:2].T, 50)
    build = time.perf_counter() - t
    per = []
    for k in rng.choice(len(centers), sample, replace=False):
        t = time.perf_counter()
        idx = tree.query_ball_point(centers[k], r=args.diam_meters // 2)
        plot = cloud[:, idx].copy()
        if plot.shape[1] >= 51:
            xyz = plot[:3].T
            _, neigh = NearestNeighbors(n_neighbors=500, algorithm="kd_tree").fit(xyz[:, :2]).radius_neighbors(xyz[:, :2], 1.5)
            z = xyz[:, 2]
            zmin = [np.min(z[neigh[n]]) for n in range(len(z))]
            plot[2] = plot[2] - zmin
        per.append(time.perf_counter() - t)
    return build, float(np.mean(per))


def znorm_candidates(cloud, plots):
    """Candidate tests of the z-norm query: for every plot point, the parcel points in the 3 x 3 cells around its own
    (cells as csrc/parcel.hip bins them)."""
    x, y = cloud[0], cloud[1]
    f32 = np.float32
    inv = f32(1.0) / (f32(1.5) * f32(1.0001))
    gx = int((x.max() - x.min()) * inv) + 1
    gy = int((y.max() - y.min()) * inv) + 1
    cx = np.clip(((x - x.min()) * inv).astype(np.int64), 0, gx - 1)
    cy = np.clip(((y - y.min()) * inv).astype(np.int64), 0, gy - 1)
    h = np.bincount(cy * gx + cx, minlength=gx * gy).reshape(gy, gx)
    p = np.pad(h, 1)
    box = sum(p[1 + dy:1 + dy + gy, 1 + dx:1 + dx + gx] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    i = plots.point_index.cpu().numpy()
    return int(box[cy[i], cx[i]].sum())


def report_times(model, cloud_dev, cloud, args, a, skw):
    """--report: (whole, tail) wall times in ms of the device report and of the host path, alternated a.pairs times"""
    x0, x1, y0, y1 = (float(v) for v in (cloud[0].min(), cloud[0].max(), cloud[1].min(), cloud[1].max()))
    rings = [np.array([[x0 + 5, y0 + 5], [x1 - 5, y0 + 5], [x1 - 5, y1 - 5], [x0 + 5, y1 - 5]])]
    inside = parcel.polygon_keep(rings, 0.0)

    def run(tail):
        t0 = time.perf_counter()
        mos, _ = parcel.predict_parcel_cloud(model, cloud_dev, args, batch_size=a.batch, fps_start=0, shape=rings, **skw)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        res = tail(mos)
        t2 = time.perf_counter()
        return (t2 - t0) * 1e3, (t2 - t1) * 1e3, res

    def device(mos):
        rep = mos.report(rings)                              # its one read waits for the device
        return rep.band_means[:4], rep.band_counts[:4], tuple(rep.bands.shape)

    def host(mos):
        out, thr = mos.finalize()
        h = out.cpu().numpy()
        float(thr[0])
        H, W = h.shape[1:]
        px = mos.x_min + mos.pix * (np.arange(W) + 0.5)
        py = mos.y_max - mos.pix * (np.arange(H) + 0.5)
        mask = inside(np.stack([np.tile(px, H), np.repeat(py, W)], 1)).reshape(H, W)
        h[:, ~mask] = np.nan
        flat = h[:4].reshape(4, -1)
        return np.nanmean(flat, axis=1), (~np.isnan(flat)).sum(1), tuple(h.shape)

    run(device), run(host)                                   # warm-up
    dev, hst = [], []
    for _ in range(a.pairs):
        dev.append(run(device))
        hst.append(run(host))
    (dm, dn, shape), (hm, hn, _) = dev[-1][2], hst[-1][2]

    def stat(v):
        return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    return {"mosaic": shape, "polygon_pixels": int(dn[0]), "pairs": a.pairs,
            "counts_equal": bool(np.array_equal(dn, hn)), "means_max_abs_diff_fp64_vs_fp32_nanmean": float(np.abs(dm - hm).max()),
            "device_e2e_ms": stat([d[0] for d in dev]), "host_e2e_ms": stat([h[0] for h in hst]),
            "device_report_ms": stat([d[1] for d in dev]), "host_crop_means_ms": stat([h[1] for h in hst])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--sample", type=int, default=6)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--sampler", choices=("numpy", "device"), default="numpy")
    ap.add_argument("--fps-live", choices=("on", "off"), default="on")
    ap.add_argument("--report", action="store_true")
    ap.add_argument("--pairs", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_parcel: needs the GPU")
    dev = torch.device("cuda:0")
    args = make_args(cuda=0)
    torch.manual_seed(0)
    model = PointNet2(args).eval()
    rng = np.random.default_rng(0)
    out = {}
    for name, side in (("10ha", 316.3), ("1ha", 100.0)):
        cloud = make_parcel(side, side, density=40.0, seed=1)
        T = cloud.shape[1]
        pinned = torch.from_numpy(cloud).pin_memory()
        h2d, cloud_dev = ev_ms(lambda: pinned.to(dev, non_blocking=True))
        for _ in range(2):
            plots = parcel.prepare_parcel(cloud_dev, args)
        torch.cuda.synchronize()
        times = [ev_ms(lambda: parcel.prepare_parcel(cloud_dev, args))[0] for _ in range(a.repeat)]
        with ops.timing({"sn2_parcel_count", "sn2_parcel_fill", "sn2_parcel_znorm"}) as tm:
            plots = parcel.prepare_parcel(cloud_dev, args)
        entries = {k: round(ms, 4) for k, (c, ms) in sorted(tm.summary().items())}
        P, SN = len(plots), int(plots.n_points.sum())

        skw = {"sampler": "device", "seed": 1} if a.sampler == "device" else {}
        skw["n_live"] = a.fps_live == "on"

        def e2e():
            mos, pl = parcel.predict_parcel_cloud(model, cloud_dev, args, batch_size=a.batch, fps_start=0, **skw)
            res = mos.finalize()
            torch.cuda.synchronize()
            return res
        e2e()
        t = time.perf_counter()
        e2e()
        e2e_s = time.perf_counter() - t

        def predict_only():
            mos = parcel.parcel_mosaic(plots.centers_host, args, dev)
            parcel.predict_parcel(model, plots.batches(args, a.batch, fps_start=0, **skw), mos, args)
            torch.cuda.synchronize()
        predict_only()
        t = time.perf_counter()
        predict_only()
        pred_s = time.perf_counter() - t
        if a.sampler == "device":                   # the plain run above is kept as it was; here: medians and the two entry points
            def clock(fn):
                ts = []
                for _ in range(a.repeat):
                    t = time.perf_counter()
                    fn()
                    ts.append(time.perf_counter() - t)
                return statistics.median(ts)
            e2e_s, pred_s = clock(e2e), clock(predict_only)
            with ops.timing({"sn2_subsample", "sn2_prepare_plots"}) as tm:
                predict_only()
            entries.update({k: round(ms, 4) for k, (c, ms) in sorted(tm.summary().items())})
        centers = parcel.parcel_plot_centers(cloud[0].min(), cloud[0].max(), cloud[1].min(), cloud[1].max(), args)
        build_s, per_plot_s = reference_cpu(cloud, centers, a.sample, args, rng)
        count_fill_bytes = 2 * 8 * T + (9 * 4 + 4) * SN + 9 * 4 * SN           # x,y twice; member rows read + written
        prep_ms = statistics.median(times)
        cand = znorm_candidates(cloud, plots)
        out[name] = {
            "points": T, "plots": P, "plot_points": SN, "sampler": a.sampler, "batch": a.batch, "fps_live": a.fps_live,
            "plots_below_subsample_size": int((plots.n_points + len(parcel.fake_ground_xy(args.diam_meters)) < args.subsample_size).sum()),
            "h2d_ms": round(h2d, 3),
            "prepare_ms_median": round(prep_ms, 3), "prepare_ms_min": round(min(times), 3),
            "entry_ms": entries,
            "predict_ms": round(pred_s * 1e3, 2),
            "e2e_ms": round(e2e_s * 1e3, 2), "e2e_plots_per_s": round(P / e2e_s, 1),
            "prepare_over_predict": round(prep_ms / (pred_s * 1e3), 3),
            "reference_cpu_s_extrapolated": round(build_s + per_plot_s * P, 2),
            "reference_cpu_sample_plots": a.sample,
            "count_fill_compulsory_bytes": count_fill_bytes,
            "count_fill_frac_of_8TBps": round(count_fill_bytes / HBM /
                                              (1e-3 * (entries.get("sn2_parcel_count", 0) + entries.get("sn2_parcel_fill", 0))), 4),
            "znorm_candidate_tests": cand,
            "znorm_candidates_per_s_over_entry": round(cand / (1e-3 * entries.get("sn2_parcel_znorm", float("nan"))), 1),
        }
        if a.report:
            out[name]["report"] = report_times(model, cloud_dev, cloud, args, a, skw)
        print(f"[bench_parcel] {name}: {json.dumps(out[name])}", file=sys.stderr, flush=True)
    ten = out["10ha"]
    print(json.dumps({"metric": "10 ha parcel preparation on the device (prepare_parcel, median)", "value": ten["prepare_ms_median"],
                      "unit": "ms", "n_gpus": 1, "sampler": a.sampler, "target_met": ten["prepare_ms_median"] <= ten["predict_ms"], "parcels": out}))


if __name__ == "__main__":
    main()
