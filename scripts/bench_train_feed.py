#!/usr/bin/env python3
"""What feeding fresh training batches costs the pipelined loop: bench.py's headline configuration (16 x 32 768 points, the
batches per geometry pass bench.py picks for the step count, hipGraph feature passes) timed with its slots filled in four ways:

    a  resident slots                     the slots' data never changes (bench.py's mode)
    b  host feeder                        pre-made pinned host batches copied into the slots (bench.py --host-inputs)
    c  train_data.EpochFeeder             every batch made on the device from a resident plot set (csrc/feed.hip)
    d  prepare_batch per step             input_pipeline.prepare_batch(train=True, noise="device", sampler="device") on the side
                                          stream, its tensors copied into the slot: the only way to fresh batches before (c)

    python scripts/bench_train_feed.py [--steps 200 --warmup 20 --repeats 3 --modes abcd --timeout 240]
    python scripts/bench_train_feed.py --mode c ...        (one mode in this process; what the driver starts)
    python scripts/bench_train_feed.py --short-plots --fps-live on|off --modes c

--short-plots: every second plot of the set has 2000 .. 6000 points instead (far fewer than the 32 768 a batch row holds: the row is
mostly repeats, what a sparse real plot looks like); the default set stays as it is.  --fps-live on (default): the slots of (c) and
(d) carry "n_live" (sn2_fps_live: the FPS kernels skip the repeats); off: they do not -- the same losses, a cross-check in one build.

The driver starts one fresh process per mode, each under its own time limit, and stops at the first one that does not end
normally.  Every mode prints one JSON line: ms per step of each of `--repeats` timed regions.  (c) and (d) draw their batches from
the same synthetic set of 256 plots of 16 000 .. 36 000 points (synthetic.make_plot), in the same shuffled order.  The file also
runs on a checkout without train_data: (c) is then reported as skipped."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SET, SET_SEED, FEED_SEED = 256, 4242, 20240229


def run_mode(a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from stratanet2_vegetation_coverage_maps_amd import losses
    from stratanet2_vegetation_coverage_maps_amd.pipeline import TrainPipeline
    from stratanet2_vegetation_coverage_maps_amd.synthetic import make_plot
    try:
        from stratanet2_vegetation_coverage_maps_amd import train_data
    except ImportError:
        train_data = None
    if a.mode == "c" and train_data is None:
        print(json.dumps({"mode": "c", "skipped": "no train_data module in this checkout"}), flush=True)
        return
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    B, N, depth = bench.PLOTS_PER_GPU, bench.N_POINTS, 3
    G = bench.pipe_group_for(a.steps)
    w = bench.build_training(dev, 0, 0, 1, B, N, "ref", "f32", G * depth + G, exchange="none")
    live = a.fps_live == "on" and a.mode in "cd"
    if live:
        for sl in w.slots:
            sl["n_live"] = torch.full((B,), N, dtype=torch.int32, device=dev)
    pipe = TrainPipeline(w.model, w.opt, w.feature_step, w.slots, depth=depth, group=G, split_exchange=w.split,
                         phase=bench.pipe_phase_for(G, a.warmup, a.steps))
    pipe.capture()
    note = {}
    if a.mode == "b":
        pinned = [{k: v.cpu().pin_memory() for k, v in sl.items() if k in ("cloud", "xyz", "gt", "pdf")} for sl in w.slots]
        pipe.set_feeder(lambda i: pinned[i % len(pinned)])
    elif a.mode in "cd":
        rng = np.random.RandomState(SET_SEED)
        sizes = rng.randint(16000, 36001, N_SET)
        if a.short_plots:                               # (a generator of its own: the default set's draws stay as they are)
            sizes[::2] = np.random.RandomState(SET_SEED + 1).randint(2000, 6001, len(sizes[::2]))
        centers = (rng.rand(N_SET, 2) * 1000).astype(np.float32)
        cov = rng.rand(N_SET, 4)
        raw = []
        for p, n in enumerate(sizes):                   # make_plot's rows back in the units load_cloud starts from
            cloud, xyz = make_plot(int(n), SET_SEED + p)
            raw.append(torch.cat([torch.stack([xyz[0] + float(centers[p, 0]), xyz[1] + float(centers[p, 1]), xyz[2]], 0),
                                  torch.floor(cloud[3:7] * 65535.0), torch.floor(cloud[7:8] * 32767.0), cloud[8:10] * 6.0 + 1.0], 0))
        tables = losses.KdeTables(np.linspace(-1.0, 30.0, 5000), *[np.linspace(0.1, 1.0, 5000) ** k for k in (1, 2, 3)], dev)
        note = {"plots": N_SET, "points_min": int(sizes.min()), "points_max": int(sizes.max()),
                "plots_above_N": int((sizes + 316 > N).sum()), "short_plots": bool(a.short_plots), "fps_live": a.fps_live}
        if a.mode == "c":
            plots = train_data.ResidentPlots.from_plots(raw, centers, cov, dev)
            pipe.set_feeder(train_data.EpochFeeder(plots, w.args, B, FEED_SEED, kde=tables,
                                                   generator=torch.Generator().manual_seed(FEED_SEED)))
        else:
            from stratanet2_vegetation_coverage_maps_amd.input_pipeline import prepare_batch
            dev_raw = [p.to(dev) for p in raw]
            gen, orders, spe = torch.Generator().manual_seed(FEED_SEED), [], N_SET // B
            rs = np.random.RandomState(FEED_SEED % 2 ** 31)

            def fresh(i):
                e, k = divmod(i, spe)
                while len(orders) <= e:
                    orders.append(torch.randperm(N_SET, generator=gen).tolist())
                ids = orders[e][k * B:(k + 1) * B]
                d = prepare_batch([dev_raw[p] for p in ids], centers[ids], w.args, train=True, rs=rs, device=dev, noise="device",
                                  sampler="device", seed=FEED_SEED, plot_keys=[e * N_SET + p for p in ids])
                out = {"cloud": d["cloud"], "xyz": d["xyz"], "gt": torch.from_numpy(cov[ids]),
                       "pdf": losses.kde_densities(d["cloud"], w.args.z_max, tables)}
                if live:
                    out["n_live"] = d["n_live"]
                return out
            pipe.set_feeder(fresh)
    pipe.prime()
    for _ in range(a.warmup):
        pipe.step()
    regions = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            loss = pipe.step()
        pipe.drain()
        torch.cuda.synchronize()
        regions.append(round((time.perf_counter() - t0) / a.steps * 1e3, 4))
    best = min(regions)
    print(json.dumps({"mode": a.mode, "ms_per_step": regions, "plots_per_s_best": round(B / (best * 1e-3), 1), "steps": a.steps,
                      "warmup": a.warmup, "batches_per_geometry_pass": G, "plots_per_gpu": B, "points_per_plot": N,
                      "loss": round(float(loss.item()), 6), **note}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=list("abcd"), default=None, help="run this one mode in this process")
    ap.add_argument("--modes", default="abcd")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3, help="timed regions of --steps steps per mode")
    ap.add_argument("--timeout", type=int, default=240, help="seconds each mode's process may take")
    ap.add_argument("--short-plots", action="store_true", help="every second plot of the set of (c) and (d) has 2000 .. 6000 points")
    ap.add_argument("--fps-live", choices=("on", "off"), default="on", help="whether the slots of (c) and (d) carry n_live")
    a = ap.parse_args()
    if a.mode is not None:
        run_mode(a)
        return 0
    for m in a.modes:                                   # this process never touches the GPU: one fresh child per mode
        cmd = [sys.executable, os.path.abspath(__file__), "--mode", m, "--steps", str(a.steps), "--warmup", str(a.warmup),
               "--repeats", str(a.repeats), "--fps-live", a.fps_live] + (["--short-plots"] if a.short_plots else [])
        try:
            rc = subprocess.run(cmd, timeout=a.timeout).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"mode": m, "error": f"no result within {a.timeout} s"}), flush=True)
            return 124
        if rc != 0:                                     # a fault, an abort or an error: nothing more is started on the GPU
            print(json.dumps({"mode": m, "error": f"exit status {rc}"}), flush=True)
            return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
