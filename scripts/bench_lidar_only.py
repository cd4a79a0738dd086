"""A training step on four point features (LiDAR-only plots: make_args(n_input_feats=6)) beside the eight-feature step, 1 x MI355X.

    python scripts/bench_lidar_only.py [--pairs 5] [--steps 200] [--warmup 24] [--plots 16] [--points 32768] [--six-rows]

The headline loop of bench.py (16 x 32 768 points, software-pipelined: eight batches per geometry pass, depth 3 = 32 slots, one
captured graph per slot with the Adam kernel inside, inputs resident, the geometry passes packing the level-0 rows and the
projection's pixel ids) is built once for F = 8 and once for F = 4 in ONE process, and timed in interleaved pairs: F = 8, F = 4,
F = 8, ...  The F = 8 kernels are the parent commit's (profiles/lidar_only/resource_usage_*.txt), so its figure is the yardstick
of the session.  The four-feature model is fed the SAME ten-row clouds (every producer of the package makes those; it reads rows
2, 7, 8, 9), or with --six-rows their rows `synthetic.LIDAR_ROWS`.

Prints one JSON line: ms/step of every run, and per model the median and the range.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stratanet2_vegetation_coverage_maps_amd import PointNet2, losses  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd.optim import FlatAdam, flatten_parameters  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd.pipeline import TrainPipeline  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd.synthetic import LIDAR_ROWS, make_args, make_batch  # noqa: E402

M1, GROUP, DEPTH = 1024, 8, 3


def build(dev, feats, B, N, six_rows, warmup, steps):
    args = make_args(cuda=dev.index or 0, subsample_size=N, n_input_feats=feats + 2, ratio1=M1 / N, r1=1.0, ratio2=0.25, r2=2.0)
    torch.manual_seed(0)
    model = PointNet2(args).train()
    model.p2_diam_pix = args.diam_pix
    flatten_parameters(model)
    opt = FlatAdam(model, lr=1e-3, weight_decay=1e-3, fold_gradient_images=True)
    slots = []
    for j in range(GROUP * DEPTH + GROUP):
        host = make_batch(B, N, first_plot=j * B)
        cloud = host["cloud"][:, list(LIDAR_ROWS)].contiguous() if (six_rows and feats == 4) else host["cloud"]
        slots.append({"cloud": cloud.to(dev), "xyz": host["xyz"].to(dev), "fps_start": torch.zeros(2, B, dtype=torch.int32, device=dev),
                      "gt": host["coverages"].to(dev), "pdf": host["pdf_all"].to(dev)})
    seed = torch.ones((), dtype=torch.float64, device=dev)

    def feature_step(inp, geo=None):
        opt.zero_grad(set_to_none=True)
        cd = {"cloud": inp["cloud"], "xyz": inp["xyz"], "fps_start": inp["fps_start"]}
        if geo is not None:
            cd["geometry"] = geo
        cov, proba = model(cd)
        loss, _, _ = losses.projected_total_loss(cov, proba, inp["cloud"], inp["gt"], inp["pdf"], args, geometry=geo, model=model)
        loss.backward(gradient=seed)
        return loss

    pipe = TrainPipeline(model, opt, feature_step, slots, depth=DEPTH, group=GROUP, phase=(warmup + steps + 1) % GROUP)
    pipe.capture()
    pipe.prime()
    return pipe


def timed(pipe, warmup, steps):
    for _ in range(warmup):
        pipe.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = pipe.step()
    pipe.drain()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    return ms, float(loss.item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--plots", type=int, default=16)
    ap.add_argument("--points", type=int, default=32768)
    ap.add_argument("--six-rows", action="store_true", help="feed the four-feature model six-row clouds instead of ten-row ones")
    a = ap.parse_args()
    if a.steps % GROUP or a.warmup % GROUP:
        # (every run of a pipeline then starts at the same place of a pass group, with the phase bench.py gives its one region)
        raise SystemExit(f"--steps and --warmup must be multiples of {GROUP} (batches per geometry pass)")
    dev = torch.device("cuda:0")
    pipes = {F: build(dev, F, a.plots, a.points, a.six_rows, a.warmup, a.steps) for F in (8, 4)}
    runs = {8: [], 4: []}
    last = {}
    for _ in range(a.pairs):
        for F in (8, 4):
            ms, last[F] = timed(pipes[F], a.warmup, a.steps)
            runs[F].append(round(ms, 4))
    out = {"workload": f"{a.plots} x {a.points} points, pipelined training step (8 batches per geometry pass, depth 3, graphs)",
           "steps": a.steps, "warmup": a.warmup, "pairs": a.pairs, "four_feature_cloud_rows": 6 if a.six_rows else 10}
    for F in (8, 4):
        out[f"F{F}"] = {"ms_per_step": runs[F], "median": round(statistics.median(runs[F]), 4), "min": min(runs[F]), "max": max(runs[F]),
                        "last_loss": round(last[F], 6)}
    out["F4_over_F8_median"] = round(out["F4"]["median"] / out["F8"]["median"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
