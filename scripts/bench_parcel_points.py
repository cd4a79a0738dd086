"""Per-point scores of a parcel on one GPU (`parcel.predict_parcel_cloud(points=True)`, csrc/points.hip): what the scatter back
costs beside the prediction it rides on.  The parcel is scripts/bench_parcel.py's: 10 ha at 40 points/m^2 (--side, --density),
device sampler.  Prints one JSON line:

  predict_ms / predict_points_ms   `predict_parcel_cloud` without and with points=True, host clock around a call that ends in a device
                                   synchronise, run ALTERNATELY --pairs times after a warm-up pair: median and range of each
  merge                            sn2_points_merge per batch (HIP events around every call of one more run): launches, total and
                                   median ms, the contributions, the bytes they add (nine int64 + one int32 each) and bytes/s
  finalize_ms / read_ms            sn2_points_finalize, and the one device-to-host read of scores, weight and hits together
  host_route_ms_per_batch          what the merge replaces: cov.cpu(), proba.cpu(), then the numpy restatement of the rule
                                   (tests/_point_scores_ref.py) for that batch, on --host-batches batches
  same_bytes_as_host               the device scores of those batches against the restatement

    python scripts/bench_parcel_points.py [--batch 512] [--pairs 5] [--host-batches 2] [--lib PATH]

--lib: another build of the library (`_build.build_variant`, e.g. with -DSN2_POINTS_CHANNEL_MAJOR for the other accumulator layout).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FLOAT_ATOMIC_RATE = 1.3e12            # bytes/s of global fp32 atomic adds on this chip: orientation only, these are 64-bit integer adds


def stat(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--host-batches", type=int, default=2)
    ap.add_argument("--side", type=float, default=316.3)
    ap.add_argument("--density", type=float, default=40.0)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_parcel_points: needs the GPU")
    from stratanet2_vegetation_coverage_maps_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    import _point_scores_ref as ref
    from stratanet2_vegetation_coverage_maps_amd import PointNet2, hip_ops as ops, parcel
    from stratanet2_vegetation_coverage_maps_amd.inference import PointScores, predict_batches
    from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_parcel

    dev = torch.device("cuda:0")
    args = make_args(cuda=0)
    torch.manual_seed(0)
    model = PointNet2(args).eval()
    cloud = make_parcel(a.side, a.side, density=a.density, seed=1)
    T = cloud.shape[1]
    cloud_dev = torch.from_numpy(cloud).to(dev)
    kw = dict(batch_size=a.batch, fps_start=0, sampler="device", seed=1)

    def run(points):
        t = time.perf_counter()
        out = parcel.predict_parcel_cloud(model, cloud_dev, args, points=points, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    run(False), run(True)                                   # warm-up: every shape of the timed window
    plain, pts = [], []
    for _ in range(a.pairs):
        plain.append(run(False)[0])
        pts.append(run(True)[0])

    with ops.timing({"sn2_points_merge"}) as tm:
        _, (mos, plots, scores) = run(True)
    per_call = sorted(x.elapsed_time(y) for _, x, y in tm.events)
    merge_ms = sum(per_call)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    res = scores.finalize()
    ev[1].record()
    pack = torch.cat([res.scores.reshape(-1).view(torch.int32), res.weight.view(torch.int32), res.hits])
    host = pack.cpu().numpy()                                # the one read
    ev[2].record()
    torch.cuda.synchronize()
    hits = host[9 * T:]
    contributions = int(hits.sum())
    added = contributions * (9 * 8 + 4)

    # the host route, on the first batches: the pointwise outputs copied out, the rule in numpy
    host_ms, rec, same = [], [], None
    if a.host_batches > 0:
        acc, hh = np.zeros((T, 9), dtype=np.int64), np.zeros(T, dtype=np.int32)
        part = PointScores(T, dev)

        class Done(Exception):
            pass

        def sink(cov, proba, cur):
            torch.cuda.synchronize()
            t = time.perf_counter()
            c, p = cov.cpu().numpy(), proba.cpu().numpy()
            col, terms = ref.contributions(c, p, cur["xyz"].cpu().numpy(), cur["sample_index"].cpu().numpy(), cur["sample_live"].cpu().numpy(),
                                           cur["point_offsets"].cpu().numpy(), cur["point_index"].cpu().numpy(), T, args.diam_meters)
            ref.accumulate(acc, hh, col, terms)
            host_ms.append((time.perf_counter() - t) * 1e3)
            part.add(cov, proba, cur)
            if len(host_ms) >= a.host_batches:
                raise Done
        try:
            predict_batches(model, plots.batches(args, a.batch, fps_start=0, sampler="device", seed=1, with_samples=True), args,
                            lambda rasters, cur: None, point_sink=sink)
        except Done:
            pass
        torch.cuda.synchronize()
        s, w = ref.finalize(acc, hh)
        r = part.finalize()
        same = bool(r.scores.cpu().numpy().tobytes() == s.tobytes() and r.weight.cpu().numpy().tobytes() == w.tobytes() and
                    np.array_equal(r.hits.cpu().numpy(), hh))

    out = {
        "points": T, "plots": len(plots), "batch": a.batch, "subsample_size": args.subsample_size, "pairs": a.pairs,
        "library": os.path.relpath(_lib.LIB_PATH, ROOT),
        "predict_ms": stat(plain), "predict_points_ms": stat(pts),
        "points_minus_plain_median_ms": round(statistics.median(pts) - statistics.median(plain), 3),
        "merge": {"launches": len(per_call), "total_ms": round(merge_ms, 3), "median_ms": round(statistics.median(per_call), 4),
                  "max_ms": round(per_call[-1], 4), "contributions": contributions, "points_hit": int((hits > 0).sum()),
                  "added_bytes": added, "added_GB_per_s": round(added / (merge_ms * 1e-3) / 1e9, 1),
                  "float_atomic_rate_GB_per_s_orientation": FLOAT_ATOMIC_RATE / 1e9},
        "finalize_ms": round(ev[0].elapsed_time(ev[1]), 3), "read_ms": round(ev[1].elapsed_time(ev[2]), 3),
        "read_bytes": int(pack.numel() * 4),
        "host_route_ms_per_batch": stat(host_ms) if host_ms else None, "host_batches": len(host_ms), "same_bytes_as_host": same,
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
