"""What PRED_ADM costs in the parcel report, on one GPU.  Two products, each predicted ONCE and then reported many times:

    10ha   the 10 ha parcel of `scripts/bench_parcel.py --report` (316.3 m square at 40 points/m^2, seed 1), `ParcelMosaic`
    16x1ha the 16 parcels of `scripts/bench_parcels.py` (100 m squares, seeds 1 .. 16, distinct origins), `MosaicAtlas`

each polygon the parcel's bounding box shrunk by 5 m.  Three tails on the same mosaic, run in interleaved triples in one session,
--pairs times each after a warm-up, wall time from the call to the values on the host (every tail ends in a read that waits for
the device):

    report        `report(rings)`: five bands, as before
    report_adm    `report(rings, admissibility=5)`: six bands, PRED_ADM and the admissibility statistics in the same read
    host          the route `report_adm` replaces: `finalize()` -> `.cpu()` -> the numpy restatement of the rule
                  (tests/_admissibility_ref.py) -> crop by `polygon_keep(rings, 0)` and `np.nanmean` on the host

Prints one JSON line: median and range per tail in ms, report_adm - report per triple, and whether the device's PRED_ADM count
equals the host route's.  The host route is a comparison, not a bar.

    python scripts/bench_admissibility.py [--pairs 15] [--batch 512] [--sieve 5]
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
from _admissibility_ref import admissibility  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd import PointNet2, parcel  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_parcel  # noqa: E402


def shrunk_box(cloud, by=5.0):
    x0, x1, y0, y1 = (float(v) for v in (cloud[0].min(), cloud[0].max(), cloud[1].min(), cloud[1].max()))
    return [np.array([[x0 + by, y0 + by], [x1 - by, y0 + by], [x1 - by, y1 - by], [x0 + by, y1 - by]])]


def host_tail(bands5, x_min, y_max, pix, rings, s):
    """bands5 (5,H,W) on the host -> (nanmean of the five reported bands after the crop, the count of PRED_ADM)"""
    six = admissibility(bands5, s)["bands6"]
    H, W = six.shape[1:]
    px = x_min + pix * (np.arange(W) + 0.5)
    py = y_max - pix * (np.arange(H) + 0.5)
    mask = parcel.polygon_keep(rings, 0.0)(np.stack([np.tile(px, H), np.repeat(py, W)], 1)).reshape(H, W)
    six[:, ~mask] = np.nan
    flat = six[:5].reshape(5, -1)
    return np.nanmean(flat, axis=1), int((~np.isnan(flat[4])).sum())


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def stat(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def triples(tails, pairs):
    for fn in tails.values():                                    # warm-up
        fn(), fn()
    times = {k: [] for k in tails}
    last = {}
    for _ in range(pairs):
        for k, fn in tails.items():
            ms, last[k] = clock(fn)
            times[k].append(ms)
    out = {k + "_ms": stat(v) for k, v in times.items()}
    out["report_adm_minus_report_ms"] = stat([a - b for a, b in zip(times["report_adm"], times["report"])])
    return out, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=15)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--sieve", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_admissibility: needs the GPU")
    dev = torch.device("cuda:0")
    args = make_args(cuda=0)
    torch.manual_seed(0)
    model = PointNet2(args).eval()
    kw = dict(sampler="device", seed=1, fps_start=0)
    out = {"pairs": a.pairs, "sieve_size": a.sieve}

    # ---- one 10 ha parcel
    cloud = make_parcel(316.3, 316.3, density=40.0, seed=1)
    rings = shrunk_box(cloud)
    mos, _ = parcel.predict_parcel_cloud(model, torch.from_numpy(cloud).to(dev), args, batch_size=a.batch, shape=rings, **kw)

    def host_one():
        b5, thr = mos.finalize()
        h = b5.cpu().numpy()
        float(thr[0])
        return host_tail(h, mos.x_min, mos.y_max, mos.pix, rings, a.sieve)
    res, last = triples({"report": lambda: mos.report(rings), "report_adm": lambda: mos.report(rings, admissibility=a.sieve),
                         "host": host_one}, a.pairs)
    rep = last["report_adm"]
    res.update(mosaic=tuple(rep.bands.shape), polygon_pixels=int(rep.band_counts[0]), pred_adm=rep.means["PRED_ADM"],
               pred_adm_pixels=rep.counts["PRED_ADM"], admissibility_stats=rep.admissibility_stats.tolist(),
               counts_equal=bool(rep.counts["PRED_ADM"] == last["host"][1]),
               pred_adm_abs_diff_fp64_vs_fp32_nanmean=float(abs(rep.means["PRED_ADM"] - last["host"][0][4])))
    out["10ha"] = res
    print(f"[bench_admissibility] 10ha: {json.dumps(res)}", file=sys.stderr, flush=True)
    del mos

    # ---- sixteen 1 ha parcels in one atlas
    K = 16
    clouds = [make_parcel(100.0, 100.0, density=40.0, seed=1 + k, x0=650000.0 + 1000.0 * k) for k in range(K)]
    shapes = [shrunk_box(c) for c in clouds]
    atlas = parcel.predict_parcels(model, clouds, args, shapes=shapes, batch_size=a.batch, **kw)[0]

    def host_all():
        arena, thr = atlas.finalize()
        h = arena.cpu().numpy()
        thr.cpu()
        res = []
        for k in range(K):
            (H, W), b = atlas.table.shape(k), atlas.table.base(k)
            x_min, y_max = atlas.table.geo(k)
            res.append(host_tail(h[5 * b:5 * (b + H * W)].reshape(5, H, W), x_min, y_max, atlas.pix, shapes[k], a.sieve))
        return res
    res, last = triples({"report": lambda: atlas.report(shapes), "report_adm": lambda: atlas.report(shapes, admissibility=a.sieve),
                         "host": host_all}, a.pairs)
    rep = last["report_adm"]
    res.update(parcels=K, pixels=int(atlas.table.pixels), pred_adm=[float(v) for v in rep.band_means[:, 4]],
               admissibility_stats_sum=rep.admissibility_stats.sum(0).tolist(),
               counts_equal=bool(all(int(rep.band_counts[k, 4]) == last["host"][k][1] for k in range(K))))
    out["16x1ha"] = res
    print(f"[bench_admissibility] 16x1ha: {json.dumps(res)}", file=sys.stderr, flush=True)
    ten = out["10ha"]
    print(json.dumps({"metric": "10 ha parcel: report(rings, admissibility=5) minus report(rings), median of interleaved runs",
                      "value": ten["report_adm_minus_report_ms"]["median"], "unit": "ms", "n_gpus": 1, "products": out}))


if __name__ == "__main__":
    main()
