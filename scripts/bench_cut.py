"""Cutting one LAS tile into parcel clouds by buffered polygon, two routes, on one GPU.  The workload: one synthetic tile
(1 km x 1 km at 10 points / m2 = 1e7 points by default, --points to shrink it, the tile then shrinks with it at the same density)
already on the device as a (10,T) fp32 cloud, and 16 parcels of about 1 ha with 40-vertex outlines on a 4 x 4 lattice, buffer 20 m.

    host     the route `parcel.cut_parcels` replaces: the tile copied to the host, `polygon_keep` per parcel in numpy over every
             tile point, `tile[:, mask_k]`, `ParcelClouds.from_clouds` (one upload)
    device   `parcel.cut_parcels`: the candidate table on the host, one packed upload, count, one read, fill

run in interleaved pairs in one process (--pairs, 15 by default; 0 skips the comparison), wall time to a synchronised ParcelClouds;
median and range, and whether the device route was faster in every pair.  Then by HIP events (median of --runs): the count entry
point (clear + pass + scan + gather) and the fill launch alone, and a device `copy_` of the bytes the fill writes (44 bytes per
hit; read + write = 2 n) as the bandwidth yardstick.  --order strips: the tile's points in 10 m bands instead of random order (the
same points, so the same hits): what spatial coherence of the file is worth to the passes.  One JSON line.

    python scripts/bench_cut.py [--points 10000000] [--pairs 15] [--runs 15] [--order random|strips]
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
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd import parcel  # noqa: E402

BUFFER = parcel.LAS_PARCEL_BUFFER


def stat(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def workload(T, seed=0):
    """(tile (10,T) fp32 on the host, 16 ring lists): the tile's side follows T at 10 points / m2, the parcels its 4 x 4 lattice"""
    rng = np.random.default_rng(seed)
    side = float(np.sqrt(T / 10.0))
    tile = (rng.random((10, T), dtype=np.float32) * np.float32(255))
    tile[0] = (rng.random(T) * side).astype(np.float32)
    tile[1] = (rng.random(T) * side).astype(np.float32)
    shapes = []
    a = 2 * np.pi * np.arange(40) / 40
    for j in range(16):
        cx, cy = (j % 4 + 0.5) * side / 4, (j // 4 + 0.5) * side / 4
        r = 56.4 * (0.8 + 0.4 * rng.random(40))                          # about 1 ha
        shapes.append([np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], 1)])
    return tile, shapes


def host_route(tile_dev, shapes):
    tile = tile_dev.cpu().numpy()
    pts = tile[:2].T.astype(np.float64)
    clouds = []
    for rings in shapes:
        m = parcel.polygon_keep(rings, BUFFER)(pts)
        if m.any():
            clouds.append(tile[:, m])
    pc = parcel.ParcelClouds.from_clouds(clouds, tile_dev.device)
    torch.cuda.synchronize()
    return pc


def device_route(tile_dev, shapes):
    cut = parcel.cut_parcels(tile_dev, shapes, BUFFER)
    torch.cuda.synchronize()
    return cut.clouds


def events(fn, runs, before=None):
    ms = []
    for j in range(runs + 2):
        arg = before() if before is not None else None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(arg) if before is not None else fn()
        b.record()
        b.synchronize()
        if j >= 2:
            ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--pairs", type=int, default=15)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--order", choices=("random", "strips"), default="random",
                    help="the tile's point order: random (the default, the worst case for the wave's lanes), or strips: 10 m bands in "
                         "y, by x inside a band (neighbours in the file are neighbours on the ground, as along a flight line)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cut: needs the GPU")
    dev = torch.device("cuda:0")
    tile, shapes = workload(a.points)
    if a.order == "strips":
        tile = np.ascontiguousarray(tile[:, np.lexsort((tile[0], np.floor(tile[1] / 10.0)))])
    tile_dev = torch.from_numpy(tile).to(dev)
    out = {"points": a.points, "order": a.order, "parcels": len(shapes), "edges": 40 * len(shapes), "buffer_m": BUFFER, "pairs": a.pairs, "runs": a.runs}
    got = device_route(tile_dev, shapes)
    out["hits"] = int(got.arena.shape[1])
    if a.pairs > 0:
        ref = host_route(tile_dev, shapes)
        out["same_bytes"] = bool(torch.equal(ref.arena.view(torch.int32), got.arena.view(torch.int32)) and
                                 np.array_equal(ref.point_start, got.point_start))
        times = {"host": [], "device": []}
        for _ in range(a.pairs):
            for k, fn in (("host", host_route), ("device", device_route)):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn(tile_dev, shapes)
                times[k].append((time.perf_counter() - t) * 1e3)
        out["host_ms"], out["device_ms"] = stat(times["host"]), stat(times["device"])
        out["device_faster_in_every_pair"] = all(d < h for d, h in zip(times["device"], times["host"]))
        out["speedup_median"] = round(statistics.median(h / d for d, h in zip(times["device"], times["host"])), 1)
        print(f"[bench_cut] routes: {json.dumps(out)}", file=sys.stderr, flush=True)
    # ---- the parts of the device route alone
    t0 = time.perf_counter()
    table = ops.CutTable([parcel.polygon_edges(r) for r in shapes], a.points, BUFFER)
    out["table_host_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    out["grid"] = [table.GX, table.GY, len(table.host[1])]
    table.upload(dev)
    prefix, starts = ops.cut_count(tile_dev, table)
    s = starts.cpu().numpy()
    counts = np.diff(s)
    base = np.where(counts > 0, 0, parcel.INT_MIN).astype(np.int32)          # every parcel with points kept: slot = its start
    base_dev, = ops.pack_upload([base], dev)
    sum_n = int(s[-1])
    count_ms = events(lambda: ops.cut_count(tile_dev, table), a.runs)
    fill_ms = events(lambda p: ops.cut_fill(tile_dev, table, p, base_dev, sum_n), a.runs, before=prefix.clone)
    moved = 44 * sum_n
    src, dst = torch.empty(moved, dtype=torch.uint8, device=dev), torch.empty(moved, dtype=torch.uint8, device=dev)
    copy_ms = events(lambda: dst.copy_(src), a.runs)
    read = torch.empty(8 * a.points, dtype=torch.uint8, device=dev)
    read_dst = torch.empty_like(read)
    xy_ms = events(lambda: read_dst.copy_(read), a.runs)
    out.update({"count_ms": stat(count_ms), "fill_ms": stat(fill_ms), "fill_bytes_written": moved,
                "fill_written_GBps": round(moved / statistics.median(fill_ms) / 1e6, 1), "copy_same_bytes_ms": stat(copy_ms),
                "copy_GBps": round(2 * moved / statistics.median(copy_ms) / 1e6, 1), "copy_xy_rows_ms": stat(xy_ms)})
    print(json.dumps({"metric": f"{a.points} tile points cut into {len(shapes)} parcel clouds (40-vertex outlines, buffer {BUFFER} m): "
                                "cut_parcels, median" + (" of interleaved pairs (host route beside it)" if a.pairs > 0 else " of count + fill by HIP events"),
                      "value": out["device_ms"]["median"] if a.pairs > 0 else round(statistics.median(count_ms) + statistics.median(fill_ms), 4),
                      "unit": "ms", "host_route_ms": out.get("host_ms", {}).get("median"), "n_gpus": 1, "results": out}))


if __name__ == "__main__":
    main()
