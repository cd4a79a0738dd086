"""Validation pass (`evaluation.evaluate`, the counterpart of the reference's learning/test.py:evaluate): P plots x N points,
synthetic, resident in HBM when the timed region starts, eval-mode forward + per-plot losses, 1 x MI355X.

    python scripts/bench_eval.py [--plots 512] [--batch 64[,512]] [--points 10000] [--repeat 7]
    python scripts/bench_eval.py --baseline [--plots 512]

prints one JSON line: plots/s of `evaluate` (median of `--repeat` runs after one warm-up, with min and max), the HIP-event time
per batch of the per-plot loss entry point (sn2_plot_losses) next to sn2_projected_loss_forward for the same B, N (median of 30).
`--baseline`: the reference's loop as written -- batch size 1, `model(cloud_data)`, `project_to_plotwise_coverages`,
`get_absolute_loss`, `get_NLL_loss`, `get_entropy_loss`, `.item()` of each -- through API that predates `evaluation.py`, so the
same script times it on the commit before.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stratanet2_vegetation_coverage_maps_amd import PointNet2, hip_ops as ops, losses, project_to_plotwise_coverages  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_batch  # noqa: E402


def timed(fn, repeat):
    fn()                                                         # warm-up (allocator, lazy module load)
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return ts


def rate(P, ts):
    return {"plots_per_s": round(P / statistics.median(ts), 1), "median_s": round(statistics.median(ts), 5),
            "min_s": round(min(ts), 5), "max_s": round(max(ts), 5), "spread_s": round(max(ts) - min(ts), 5)}


def events_ms(fn, n=30):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(out), 4), "min_ms": round(min(out), 4), "max_ms": round(max(out), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plots", type=int, default=512)
    ap.add_argument("--batch", type=str, default="64", help="plots per launch; a comma list times each on the same plots")
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--prefetch", type=int, default=3)
    ap.add_argument("--baseline", action="store_true", help="the reference's loop: batch size 1, the three loss terms, .item() of each")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    P, N = a.plots, a.points
    args = make_args(cuda=0, subsample_size=N)                   # reference defaults: ratios .25/.25, r sqrt2/sqrt8
    torch.manual_seed(0)
    model = PointNet2(args).eval()
    t0 = time.time()
    chunks = []
    for s in range(0, P, 64):
        chunks.append(make_batch(min(64, P - s), N, first_plot=s))
        print(f"[bench_eval] generated {min(P, s + 64)}/{P} plots ({time.time() - t0:.0f}s)", file=sys.stderr, flush=True)
    cloud = torch.cat([c["cloud"] for c in chunks]).to(dev)
    xyz = torch.cat([c["xyz"] for c in chunks]).to(dev)
    gt = torch.cat([c["coverages"] for c in chunks]).to(dev)
    pdf = torch.cat([c["pdf_all"] for c in chunks]).to(dev)
    del chunks

    def batches_of(nb):
        return [{"cloud": cloud[s:s + nb], "xyz": xyz[s:s + nb], "coverages": gt[s:s + nb], "pdf_all": pdf[s * N:(s + nb) * N],
                 "plot_id": list(range(s, min(P, s + nb))), "fps_start": torch.zeros(2, min(nb, P - s), dtype=torch.int64)}
                for s in range(0, P, nb)]

    res = {"metric": "plots/s validation pass (eval fwd + per-plot losses)", "unit": "plots/s", "n_gpus": 1, "dtype": "f32",
           "data": "synthetic", "config": {"plots": P, "points": N, "repeat": a.repeat, "prefetch": a.prefetch}}
    if a.baseline:
        singles = batches_of(1)

        @torch.no_grad()
        def reference_loop():
            meter = [0.0, 0.0, 0.0, 0.0]
            for cd in singles:
                cov, proba = model(cd)
                pred_pl = project_to_plotwise_coverages(cov, cd["cloud"], args)
                loss_abs = losses.get_absolute_loss(pred_pl, cd["coverages"])
                loss_log = losses.get_NLL_loss(proba, cd["pdf_all"])
                loss_e = losses.get_entropy_loss(proba)
                loss = loss_abs + args.m * loss_log + args.e * loss_e
                for i, v in enumerate((loss, loss_abs, loss_log, loss_e)):
                    meter[i] += v.item()
            return [v / len(singles) for v in meter]

        ts = timed(reference_loop, a.repeat)
        res.update(value=rate(P, ts)["plots_per_s"], mode="baseline: reference loop, batch size 1", baseline=rate(P, ts),
                   total_loss=reference_loop()[0])
        print(json.dumps(res))
        return

    from stratanet2_vegetation_coverage_maps_amd import evaluation
    res["evaluate"], res["entry_point"] = {}, {}
    for nb in [int(x) for x in a.batch.split(",") if x]:
        batches = batches_of(nb)
        out = {}

        def run():
            out["r"] = evaluation.evaluate(model, batches, args, prefetch=a.prefetch)

        ts = timed(run, a.repeat)
        res["evaluate"][str(nb)] = dict(rate(P, ts), total_loss=out["r"][0]["total_loss"])
        # the new entry point next to the training step's fused projection + loss, same B, N, same inputs
        B = min(nb, P)
        R = B * N
        g = torch.Generator().manual_seed(1)
        cov = torch.rand(R, 4, generator=g).to(dev)
        proba = torch.softmax(torch.randn(R, 4, generator=g), 1).to(dev)
        _, pix = ops.plot_pixels(cloud[:B].contiguous(), args.diam_pix)
        gtb, pdfb = gt[:B].contiguous(), pdf[:R].contiguous()
        res["entry_point"][str(nb)] = {
            "sn2_plot_losses": events_ms(lambda: ops.plot_losses(cov, pix, proba, pdfb, gtb, B, N, args.diam_pix, args.m, args.e)),
            "sn2_projected_loss_forward": events_ms(lambda: ops.projected_loss_forward(cov, pix, proba, pdfb, gtb, B, N, args.diam_pix,
                                                                                       args.m, args.e))}
    first = next(iter(res["evaluate"].values()))
    res["value"] = first["plots_per_s"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
