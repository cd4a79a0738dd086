"""The cross-validation report (`cross_validation.indicators`, sn2_cv_indicators; the reference's `post_cross_validation_logging`
arithmetic, learning/accuracy.py) on synthetic (P,4) tables resident on the device.  NOT on the training hot path: it runs once per
cross-validation.

    python scripts/bench_cv_report.py [--plots 1000 100000 1000000] [--repeat 30] [--host-repeat 3]

prints one JSON line per P: the HIP-event time of the two launches of `hip_ops.cv_indicators` and the wall time of
`cross_validation.indicators` (the launches, the allocations and the ONE read of 445 doubles, ended by that read) -- median, min,
max and spread of `--repeat` calls after a warm-up -- and, timed in the same run, what the host path would cost: the device-to-host
copy of the (P,4) fp32 and (P,4) fp64 tables (ended by a synchronise) plus the numpy fp64 restatement of tests/_cv_indicators_ref.py
on this host (median of `--host-repeat`).  The reference's own path (a pandas `DataFrame.apply` per row and column) is NOT timed:
its module does not import under NumPy >= 1.24.  The last line of each record compares the two results (counts exactly, means)."""
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
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd.cross_validation import indicators  # noqa: E402
import _cv_indicators_ref as R  # noqa: E402


def _stat(v, nd=4):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd),
            "spread": round(max(v) - min(v), nd)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plots", type=int, nargs="+", default=[1000, 100_000, 1_000_000])
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--host-repeat", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cv_report needs the HIP device")
    dev = "cuda:0"
    for P in a.plots:
        pred_h, gt_h = R.random_table(P, 1)
        pred, gt = torch.from_numpy(pred_h).to(dev), torch.from_numpy(gt_h).to(dev)
        for _ in range(3):                                                # warm-up: library load, allocator, this shape
            rep = indicators(pred, gt, True)
        torch.cuda.synchronize()
        kern, call, copy = [], [], []
        for _ in range(a.repeat):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.cv_indicators(pred, gt, True)
            e1.record()
            e1.synchronize()
            kern.append(e0.elapsed_time(e1))
        for _ in range(a.repeat):
            t = time.perf_counter()
            rep = indicators(pred, gt, True)                              # ends in its read of `stats`
            call.append((time.perf_counter() - t) * 1e3)
        for _ in range(a.repeat):
            t = time.perf_counter()
            ph, gh = pred.cpu(), gt.cpu()
            torch.cuda.synchronize()
            copy.append((time.perf_counter() - t) * 1e3)
        host = []
        for _ in range(a.host_repeat):
            t = time.perf_counter()
            rows, cls, stats = R.indicators(ph.numpy(), gh.numpy(), True)
            host.append((time.perf_counter() - t) * 1e3)
        mean_h = stats["sum"] / np.maximum(stats["count"], 1)
        mean_d = np.array([rep.means[n] for n in R.COLUMNS])
        in_bytes, out_bytes = P * (16 + 32), P * (240 + 36)
        k = statistics.median(kern)
        print(json.dumps({
            "metric": "cross-validation report", "unit": "ms", "n_gpus": 1, "dtype": "f64 from f32 predictions", "data": "synthetic",
            "config": {"plots": P, "relabel": True, "repeat": a.repeat, "host_repeat": a.host_repeat},
            "device_two_launches_ms": _stat(kern), "indicators_call_with_read_ms": _stat(call),
            "bytes_moved_by_the_launches": in_bytes + out_bytes, "achieved_GB_per_s": round((in_bytes + out_bytes) / k / 1e6, 1),
            "host_path_ms": {"device_to_host_copy": _stat(copy), "numpy_restatement": _stat(host, 2)},
            "agreement": {"counts_and_confusions_equal": bool(np.array_equal(rep._counts, stats["count"]) and
                                                              np.array_equal(rep._cm, stats["cm"])),
                          "max_abs_mean_difference": float(np.abs(mean_d - mean_h).max())},
            "reference_pandas_path": "not timed: learning/accuracy.py does not import under NumPy >= 1.24"}), flush=True)


if __name__ == "__main__":
    main()
