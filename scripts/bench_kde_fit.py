"""Fitting the KDE mixture of the NLL loss (`losses.KdeTables.fit`, sn2_kde_fit; the reference's `KdeMixture.fit` +
`evaluate_kdes`, learning/kde_mixture.py:50-100): n synthetic heights (the mixture of synthetic.py), resident on the device.

    python scripts/bench_kde_fit.py [--heights 500000] [--grid 5000] [--bw 0.1] [--repeat 30]

prints one JSON line: the HIP-event time of `hip_ops.kde_fit` (median, min, max, spread of `--repeat` calls after a warm-up), the
wall time of the fp64 numpy restatement of the same estimator on this host (tests/test_kde_fit_host.py: `fit_tables`, median of 5,
timed in the same run), and the largest difference between the two tables.  The reference's own path (KDEpy's FFTKDE) is NOT
timed: KDEpy is not a dependency of this project and is absent where this runs.
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
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_plot  # noqa: E402
from test_kde_fit_host import fit_tables  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heights", type=int, default=500_000)
    ap.add_argument("--grid", type=int, default=5000)
    ap.add_argument("--bw", type=float, default=0.1)
    ap.add_argument("--repeat", type=int, default=30)
    a = ap.parse_args()
    z = make_plot(a.heights, 20211007)[1][2].contiguous()
    zd = z.to("cuda:0")
    X, Y = ops.kde_fit(zd, a.bw, a.grid)                           # warm-up (library load, allocator)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        X, Y = ops.kde_fit(zd, a.bw, a.grid)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    zn = z.numpy()
    host = []
    for _ in range(5):
        t = time.perf_counter()
        Xr, Yr = fit_tables(zn, a.bw, a.grid)
        host.append((time.perf_counter() - t) * 1e3)
    Yd = Y.cpu().numpy()
    print(json.dumps({
        "metric": "KDE mixture fit", "unit": "ms", "n_gpus": 1, "dtype": "f64 tables from f32 heights", "data": "synthetic",
        "config": {"heights": a.heights, "grid": a.grid, "bw": a.bw, "repeat": a.repeat},
        "device_ms": {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4),
                      "spread": round(max(ms) - min(ms), 4)},
        "numpy_host_ms": {"median": round(statistics.median(host), 2), "min": round(min(host), 2), "max": round(max(host), 2)},
        "max_abs_table_difference": float(np.abs(Yd - Yr).max()),
        "max_rel_table_difference_where_Y_gt_1e-3": float((np.abs(Yd - Yr) / np.maximum(Yr, 1e-300))[Yr > 1e-3].max()),
        "X_max_abs_difference": float(np.abs(X.cpu().numpy() - Xr).max()),
        "reference_kdepy_path": "not timed: KDEpy is absent"}))


if __name__ == "__main__":
    main()
