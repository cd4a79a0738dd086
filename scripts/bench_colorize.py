"""Colouring a LiDAR tile from orthoimages, two routes, on one GPU.  The workload: 1e7 points (--points) over a 1 km x 1 km tile,
already on the device as a (10,T) fp32 cloud, a 5000 x 5000 uint8 RGB image and a 5000 x 5000 uint8 IRC image at 20 cm (--image),
chunky, resident on the device.  Rows 3, 4, 5 come from the RGB image, row 6 from band 0 of the IRC image: two calls.

    host     the route `ortho.colorize` replaces: the cloud copied to the host, `ortho.colorize_ref` twice (numpy: a fancy-indexed
             gather per band), one upload of the coloured cloud
    device   `ortho.colorize` twice

run in interleaved pairs in one process (--pairs), wall time to a synchronised cloud; median and range, and whether the device
route was faster in every pair.  Then by HIP events (median of --runs): each of the two calls alone, and a device `copy_` that
moves the bytes the call reads and writes (x, y and the samples read, the rows written; copy_ of n bytes moves 2 n) as the
bandwidth yardstick.  Two point orders, each in a child process of its own under `timeout`, the second only if the first ended
well: random (the worst case for the gather: neighbouring lanes hit unrelated pixels) and strips (10 m bands in y, by x inside a
band: neighbours in the file are neighbours on the ground, as along a flight line).  One JSON line with both.

    python scripts/bench_colorize.py [--points 10000000] [--image 5000] [--pairs 5] [--runs 15] [--order both|random|strips]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIDE = 1000.0
CHILD_LIMIT_S = 420


def stat(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def workload(T, n, order, seed=0):
    rng = np.random.default_rng(seed)
    cloud = rng.random((10, T), dtype=np.float32) * np.float32(255)
    cloud[0] = (rng.random(T) * SIDE).astype(np.float32)
    cloud[1] = (rng.random(T) * SIDE).astype(np.float32)
    cloud[3:7] = 0.0
    if order == "strips":
        cloud = np.ascontiguousarray(cloud[:, np.lexsort((cloud[0], np.floor(cloud[1] / 10.0)))])
    rgb = rng.integers(1, 256, size=(n, n, 3), dtype=np.uint8)
    irc = rng.integers(1, 256, size=(n, n, 3), dtype=np.uint8)
    return cloud, rgb, irc


def run_order(a):
    import torch
    from stratanet2_vegetation_coverage_maps_amd import ortho
    if not torch.cuda.is_available():
        raise SystemExit("bench_colorize: needs the GPU")
    dev = torch.device("cuda:0")
    cloud, rgb, irc = workload(a.points, a.image, a.order)
    pix = SIDE / a.image
    host_sets = [ortho.OrthoSet([ortho.OrthoImage(p, 0.0, SIDE, pix)]) for p in (rgb, irc)]
    dev_sets = [ortho.OrthoSet([ortho.OrthoImage(torch.from_numpy(p).to(dev), 0.0, SIDE, pix)]) for p in (rgb, irc)]
    calls = [dict(bands=(0, 1, 2), rows=(3, 4, 5)), dict(bands=(0,), rows=(6,))]
    cloud_dev = torch.from_numpy(cloud).to(dev)

    def host_route(c):
        h = c.cpu().numpy()
        for s, kw in zip(host_sets, calls):
            h = ortho.colorize_ref(h, s, **kw).cloud
        out = torch.from_numpy(h).to(dev)
        torch.cuda.synchronize()
        return out

    def device_route(c):
        for s, kw in zip(dev_sets, calls):
            ortho.colorize(c, s, **kw)
        torch.cuda.synchronize()
        return c

    out = {"points": a.points, "order": a.order, "image": [a.image, a.image, 3], "pixel_m": pix, "pairs": a.pairs, "runs": a.runs}
    got = device_route(cloud_dev.clone())
    if a.pairs > 0:
        ref = host_route(cloud_dev)
        out["same_bytes"] = bool(torch.equal(ref.view(torch.int32), got.view(torch.int32)))
        times = {"host": [], "device": []}
        for _ in range(a.pairs):
            for k, fn in (("host", host_route), ("device", device_route)):
                work = cloud_dev.clone()
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn(work)
                times[k].append((time.perf_counter() - t) * 1e3)
        out["host_ms"], out["device_ms"] = stat(times["host"]), stat(times["device"])
        out["device_faster_in_every_pair"] = all(d < h for d, h in zip(times["device"], times["host"]))
        out["speedup_median"] = round(statistics.median(h / d for d, h in zip(times["device"], times["host"])), 1)
        print(f"[bench_colorize] routes: {json.dumps(out)}", file=sys.stderr, flush=True)

    def events(fn):
        ms = []
        for j in range(a.runs + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if j >= 2:
                ms.append(e0.elapsed_time(e1))
        return ms

    work = cloud_dev.clone()
    T = a.points
    for name, s, kw, moved in (("rgb", dev_sets[0], calls[0], (8 + 3 + 12) * T), ("irc", dev_sets[1], calls[1], (8 + 1 + 4) * T)):
        call_ms = events(lambda: ortho.colorize(work, s, **kw))
        src, dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev), torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        copy_ms = events(lambda: dst.copy_(src))
        out[name] = {"call_ms": stat(call_ms), "bytes_moved": moved, "call_GBps": round(moved / statistics.median(call_ms) / 1e6, 1),
                     "copy_same_bytes_ms": stat(copy_ms), "copy_GBps": round(moved / statistics.median(copy_ms) / 1e6, 1),
                     "call_over_copy": round(statistics.median(call_ms) / statistics.median(copy_ms), 2)}
        del src, dst
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--image", type=int, default=5000, help="pixels per side of the two images (the tile is 1 km: 5000 = 20 cm)")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--order", choices=("both", "random", "strips"), default="both")
    a = ap.parse_args()
    if a.order != "both":
        return run_order(a)
    results = {}
    for order in ("random", "strips"):                       # each order a fresh process under its own time limit
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--order", order, "--points", str(a.points),
               "--image", str(a.image), "--pairs", str(a.pairs), "--runs", str(a.runs)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit(f"bench_colorize: the {order} run ended with status {r.returncode}; nothing more is started")
        results[order] = json.loads(r.stdout.strip().splitlines()[-1])
    rnd = results["random"]
    print(json.dumps({"metric": f"{a.points} points coloured from two {a.image} x {a.image} uint8 images (rows 3..6): ortho.colorize x 2, median"
                                + (" of interleaved pairs (host route beside it), random order" if a.pairs > 0 else " by HIP events, random order"),
                      "value": rnd["device_ms"]["median"] if a.pairs > 0 else round(rnd["rgb"]["call_ms"]["median"] + rnd["irc"]["call_ms"]["median"], 4),
                      "unit": "ms", "host_route_ms": rnd.get("host_ms", {}).get("median"), "n_gpus": 1, "results": results}))


if __name__ == "__main__":
    main()
