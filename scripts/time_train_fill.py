#!/usr/bin/env python3
"""train_data.ResidentPlots.fill (sn2_train_batch [+ sn2_kde_lookup]) alone on an idle chip at bench.py's batch, 16 x 32 768: HIP-event
time around the call -- its host launch work included -- as median / min / max of 40 calls, for train=False, noise=False, the default
and with the KDE densities, on a set of 64 synthetic plots without and with plots above N candidates (the latter runs the
subsample's four launches).  One JSON line per case.

    python scripts/time_train_fill.py"""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stratanet2_vegetation_coverage_maps_amd import losses
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_raw_plot
from stratanet2_vegetation_coverage_maps_amd.train_data import ResidentPlots
dev = torch.device("cuda:0")
B, N = 16, 32768
args = make_args(cuda=0, subsample_size=N, ratio1=1024 / N, r1=1.0, ratio2=0.25, r2=2.0)
tables = losses.KdeTables(np.linspace(-1.0, 30.0, 5000), *[np.linspace(0.1, 1.0, 5000) ** k for k in (1, 2, 3)], dev)
rng = np.random.RandomState(1)
out = {"cloud": torch.empty(B, 10, N, device=dev), "xyz": torch.empty(B, 3, N, device=dev), "gt": torch.empty(B, 4, dtype=torch.float64, device=dev),
       "fps_start": torch.empty(2, B, dtype=torch.int32, device=dev), "pdf": torch.empty(B * N, 3, dtype=torch.float64, device=dev)}
for name, lo, hi in (("all plots <= N", 16000, 32000), ("some plots > N", 16000, 36001)):
    sizes = rng.randint(lo, hi, 64)
    plots = ResidentPlots.from_plots([make_raw_plot(int(n), 7 + p) for p, n in enumerate(sizes)], np.zeros((64, 2), np.float32), rng.rand(64, 4), dev)
    ids = plots.check_ids(rng.permutation(64)[:B]).to(dev)
    for flags in ({"train": False}, {"noise": False}, {}, {"kde": tables}):
        for _ in range(5):
            plots.fill(ids, 1, 2, args, out, **flags)
        torch.cuda.synchronize()
        ts = []
        for _ in range(40):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); plots.fill(ids, 1, 2, args, out, **flags); b.record(); torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        print(json.dumps({"set": name, "flags": {k: (True if k == "kde" else v) for k, v in flags.items()}, "us_median": round(float(np.median(ts)), 1),
                          "us_min": round(min(ts), 1), "us_max": round(max(ts), 1)}), flush=True)
