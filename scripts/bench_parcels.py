"""K small parcels: one parcel at a time against shared batches over a mosaic atlas, on one GPU.  K = 16 synthetic 1 ha parcels
(`scripts/bench_parcel.py`'s 1 ha case: 100 m x 100 m at 40 points/m^2, seeds 1 .. K) at distinct origins, device sampler,
fps_start = 0, B = 512, each parcel's polygon its bounding box shrunk by 5 m.  Two contenders in one process:

    loop   per parcel `predict_parcel_cloud(shape=rings)` + `ParcelMosaic.report(rings)`: the code as it was before the atlas
    set    `predict_parcels(shapes=...)` + `MosaicAtlas.report(shapes)`

run alternately, --pairs times each after a warm-up, in two forms: "whole" (the calls above, one synchronise at the end) and
"phases" (prepare, predict and report timed apart, a synchronise between them; the loop's phases are the three calls
`predict_parcel_cloud` is made of).  Prints one JSON line: median and range per contender and phase, plots/s over the predict
phase, the share of the prepare phase, and whether the set's predict + report time lies below the loop's in every pair.
The prepare phase has two contenders of its own, timed in every pair right after one another: `prepare_parcels(batched=False)`
(the loop over `prepare_parcel`) and `prepare_parcels(batched=True)` (one pass over a cloud arena, the arena's concatenation
included); "prepare" reports both, whether the batched one lies below the loop in every pair, and the share of the batched
prepare spent in the host lattice / centre-grid code (host clock around `parcel._host_lattices`).  The set's own phases and its
whole job use the default (`batched=None`).
The clouds are on the device before the clock starts (as in bench_parcel.py).  Kernel times: run it under
`rocprofv3 --kernel-trace --stats`; `--one-prepare` makes ONE batched prepare after the clouds are built and exits, so that such a
trace holds the launches of exactly one.

    python scripts/bench_parcels.py [--parcels 16] [--pairs 5] [--batch 512] [--side 100] [--one-prepare]
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
from stratanet2_vegetation_coverage_maps_amd import PointNet2, parcel  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd.inference import MosaicAtlas, predict_batches  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_parcel  # noqa: E402

SEED = 1


def clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parcels", type=int, default=16)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--side", type=float, default=100.0)
    ap.add_argument("--one-prepare", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_parcels: needs the GPU")
    if a.pairs < 5:
        raise SystemExit("bench_parcels: at least five pairs")
    dev = torch.device("cuda:0")
    args = make_args(cuda=0)
    torch.manual_seed(0)
    model = PointNet2(args).eval()
    K = a.parcels
    clouds, rings = [], []
    for k in range(K):
        c = make_parcel(a.side, a.side, density=40.0, seed=1 + k, x0=650000.0 + 1000.0 * k)
        x0, x1, y0, y1 = (float(v) for v in (c[0].min(), c[0].max(), c[1].min(), c[1].max()))
        rings.append([np.array([[x0 + 5, y0 + 5], [x1 - 5, y0 + 5], [x1 - 5, y1 - 5], [x0 + 5, y1 - 5]])])
        clouds.append(torch.from_numpy(c).to(dev))
    kw = dict(fps_start=0, sampler="device", seed=SEED)
    if a.one_prepare:
        torch.cuda.synchronize()
        plots = parcel.prepare_parcels(clouds, args, shapes=rings, batched=True)
        torch.cuda.synchronize()
        print(json.dumps({"one_batched_prepare": True, "parcels": K, "plots": len(plots)}))
        return
    host = {"s": 0.0}
    lattices = parcel._host_lattices

    def timed_lattices(*p, **k):
        t0 = time.perf_counter()
        out = lattices(*p, **k)
        host["s"] += time.perf_counter() - t0
        return out
    parcel._host_lattices = timed_lattices

    def prepare_pair():
        t0 = clock()
        pl = parcel.prepare_parcels(clouds, args, shapes=rings, batched=False)
        t1 = clock()
        host["s"] = 0.0
        pb = parcel.prepare_parcels(clouds, args, shapes=rings, batched=True)
        t2 = clock()
        assert len(pl) == len(pb)
        return {"loop": t1 - t0, "batched": t2 - t1, "host": host["s"]}

    def loop_whole(key=lambda k: 0):
        t0 = clock()
        reps = []
        for k in range(K):
            mos, _ = parcel.predict_parcel_cloud(model, clouds[k], args, batch_size=a.batch, shape=rings[k], key_base=key(k), **kw)
            reps.append(mos.report(rings[k]))
        return {"whole": clock() - t0}, reps

    def set_whole():
        t0 = clock()
        atlas, _ = parcel.predict_parcels(model, clouds, args, shapes=rings, batch_size=a.batch, **kw)
        rep = atlas.report(rings)
        return {"whole": clock() - t0}, rep

    def loop_phases():
        t = {"prepare": 0.0, "predict": 0.0, "report": 0.0}
        n = 0
        for k in range(K):
            t0 = clock()
            plots = parcel.prepare_parcel(clouds[k], args, keep=parcel.polygon_keep(rings[k], parcel.shape_buffer(args)))
            t1 = clock()
            mos = parcel.parcel_mosaic(plots.centers_host, args, plots.raw.device)
            parcel.predict_parcel(model, plots.batches(args, a.batch, np.random, 0, "device", SEED, True), mos, args)
            t2 = clock()
            mos.report(rings[k])
            t3 = clock()
            t["prepare"] += t1 - t0
            t["predict"] += t2 - t1
            t["report"] += t3 - t2
            n += len(plots)
        return t, n

    def set_phases():
        t0 = clock()
        plots = parcel.prepare_parcels(clouds, args, shapes=rings)
        t1 = clock()
        atlas = MosaicAtlas.for_plots(plots, args)
        predict_batches(model, plots.batches(args, a.batch, np.random, 0, "device", SEED, True), args,
                        lambda r, cur: atlas.add(r, cur["plot_center"], cur["parcel"]))
        t2 = clock()
        atlas.report(rings)
        t3 = clock()
        return {"prepare": t1 - t0, "predict": t2 - t1, "report": t3 - t2}, len(plots)

    # warm-up, and the two contenders' results on the same Philox keys
    _, reps = loop_whole(key=lambda k: k << 32)
    _, rep = set_whole()
    equal = all(reps[k].band_means.tobytes() == rep.band_means[k].tobytes() and np.array_equal(reps[k].band_counts, rep.band_counts[k])
                and reps[k].threshold == rep.thresholds[k] for k in range(K))
    loop_phases(), set_phases(), loop_whole(), prepare_pair()

    runs = {"loop": [], "set": []}
    prep = []
    plots_n = 0
    for _ in range(a.pairs):
        lw, sw = loop_whole()[0], set_whole()[0]
        (lp, plots_n), (sp, n2) = loop_phases(), set_phases()
        assert plots_n == n2
        runs["loop"].append({**lw, **lp})
        runs["set"].append({**sw, **sp})
        prep.append(prepare_pair())

    def stat(v):
        return {"median": round(statistics.median(v) * 1e3, 3), "min": round(min(v) * 1e3, 3), "max": round(max(v) * 1e3, 3)}

    out = {}
    for name, rs in runs.items():
        pr = [r["predict"] + r["report"] for r in rs]
        tot = [r["prepare"] + r["predict"] + r["report"] for r in rs]
        out[name] = {"whole_ms": stat([r["whole"] for r in rs]), "prepare_ms": stat([r["prepare"] for r in rs]),
                     "predict_ms": stat([r["predict"] for r in rs]), "report_ms": stat([r["report"] for r in rs]),
                     "predict_report_ms": stat(pr),
                     "predict_plots_per_s": round(plots_n / statistics.median([r["predict"] for r in rs]), 1),
                     "prepare_share_of_phases": round(statistics.median([r["prepare"] / t for r, t in zip(rs, tot)]), 3)}
    lpr = [r["predict"] + r["report"] for r in runs["loop"]]
    spr = [r["predict"] + r["report"] for r in runs["set"]]
    below = all(s < l for s, l in zip(spr, lpr))
    apart = max(spr) < min(lpr)
    print(json.dumps({"metric": f"{K} parcels of {a.side:g} m x {a.side:g} m: predict + report, loop time over set time (medians)",
                      "value": round(statistics.median(lpr) / statistics.median(spr), 3), "unit": "x", "n_gpus": 1,
                      "parcels": K, "plots": plots_n, "batch": a.batch, "pairs": a.pairs, "results_equal_on_the_same_keys": bool(equal),
                      "set_below_loop_in_every_pair": bool(below), "ranges_apart": bool(apart),
                      "whole_loop_over_set": round(statistics.median([r["whole"] for r in runs["loop"]]) /
                                                   statistics.median([r["whole"] for r in runs["set"]]), 3),
                      "prepare": {"loop_ms": stat([r["loop"] for r in prep]), "batched_ms": stat([r["batched"] for r in prep]),
                                  "loop_over_batched": round(statistics.median([r["loop"] for r in prep]) /
                                                             statistics.median([r["batched"] for r in prep]), 3),
                                  "batched_below_loop_in_every_pair": bool(all(r["batched"] < r["loop"] for r in prep)),
                                  "host_lattice_ms": stat([r["host"] for r in prep]),
                                  "host_lattice_share_of_batched": round(statistics.median([r["host"] / r["batched"] for r in prep]), 3)},
                      "loop": out["loop"], "set": out["set"]}))


if __name__ == "__main__":
    main()
