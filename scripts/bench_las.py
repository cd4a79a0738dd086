"""From the point-record block of a LAS file to the (10,T) fp32 cloud on the device, two routes, on one GPU.  A synthetic format-8
block (38-byte records) of the 10 ha parcel's size (3.9e6 records) and of a 1 ha one (3.9e5), already in host memory in both routes
(reading the file is the same for both and is not timed):

    host     the numpy restatement of the reference's load_las_file (utils/load_data.py:149-184): ten field reads of a packed
             structured dtype (what laspy 1.x does), X / 100 in fp64, np.asarray(..., float32) of the ten rows, then the upload of
             the (10,T) array.  laspy itself is not installed and cannot be timed.
    device   the raw block into a pinned staging buffer, ONE host-to-device copy, ONE launch of sn2_las_decode

run interleaved, --runs times each after a warm-up, wall time from the block in host memory to a synchronised device tensor; median
and range; the host parts of each route (the numpy decode; the copy of the block into the pinned buffer, which las.load_las does
not make: it reads the file into that buffer) and the two uploads from pinned memory alone.  Then the kernel alone by HIP events
(median of --runs): its staged form and its field-by-field form (sn2_debug_las_form), as bytes moved ((L + 40) T) over the time, next to a device-to-device copy of the same number of bytes
(read + write = 2 n) measured in the same run, for record lengths 38, 30, 32, 39 and 131 (direct form only).  One JSON line.

    python scripts/bench_las.py [--runs 15]
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
import _las_ref as R  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd import _lib, las  # noqa: E402


def stat(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def block(T, fmt, L, seed):
    rng = np.random.default_rng(seed)
    f = dict(X=rng.integers(65000000, 65031630, T), Y=rng.integers(686000000, 686031630, T), Z=rng.integers(20000, 24000, T),
             returns=rng.integers(0, 256, T), classification=rng.integers(0, 32, T))
    for k in ("intensity", "red", "green", "blue", "nir"):
        f[k] = rng.integers(0, 65536, T)
    return R.pack_records(f, fmt, L)


def host_route(recs, dt, T, dev):
    rec = np.frombuffer(recs, dtype=dt, count=T)
    b = rec["returns"]
    cloud = np.asarray([rec["X"] / 100, rec["Y"] / 100, rec["Z"] / 100, rec["red"], rec["green"], rec["blue"], rec["nir"],
                        rec["intensity"], b & 15, b >> 4], dtype=np.float32)
    out = torch.from_numpy(cloud).to(dev)
    torch.cuda.synchronize()
    return out


def device_route(recs, header, pinned, dev):
    n = header.n_bytes
    memoryview(pinned.numpy())[:n] = recs
    raw = torch.empty(n, dtype=torch.uint8, device=dev)
    raw.copy_(pinned[:n], non_blocking=True)
    out = las.decode(raw, header)
    torch.cuda.synchronize()
    return out


def events(fn, runs):
    fn(), fn()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_las: needs the GPU")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    out = {"runs": a.runs, "routes": {}, "kernel": {}}
    for name, T in (("10ha", 3900000), ("1ha", 390000)):
        recs = block(T, 8, 38, 1)
        h = las.LasHeader((1, 4), 8, 38, 375, T, (0.01,) * 3, (0.0,) * 3, (0.0,) * 3, (0.0,) * 3, 375)
        dt = R.record_dtype(8, 38)
        pinned = torch.empty(h.n_bytes, dtype=torch.uint8, pin_memory=True)
        for _ in range(2):
            ref, got = host_route(recs, dt, T, dev), device_route(recs, h, pinned, dev)
        same = bool(torch.equal(ref.view(torch.int32), got.view(torch.int32)))
        times = {"host": [], "device": []}
        for _ in range(a.runs):
            for k, fn in (("host", lambda: host_route(recs, dt, T, dev)), ("device", lambda: device_route(recs, h, pinned, dev))):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                times[k].append((time.perf_counter() - t) * 1e3)
        # the parts of the two routes, each alone (host clocks, same number of warm runs)
        def numpy_decode():
            rec = np.frombuffer(recs, dtype=dt, count=T)
            b = rec["returns"]
            return np.asarray([rec["X"] / 100, rec["Y"] / 100, rec["Z"] / 100, rec["red"], rec["green"], rec["blue"], rec["nir"],
                               rec["intensity"], b & 15, b >> 4], dtype=np.float32)

        def fill_pinned():
            memoryview(pinned.numpy())[:h.n_bytes] = recs
        parts = {"host_numpy_decode_alone_ms": [], "device_fill_pinned_alone_ms": []}
        for _ in range(a.runs):
            for k, fn in (("host_numpy_decode_alone_ms", numpy_decode), ("device_fill_pinned_alone_ms", fill_pinned)):
                t = time.perf_counter()
                fn()
                parts[k].append((time.perf_counter() - t) * 1e3)
        cloud = numpy_decode()
        pin_cloud = torch.from_numpy(cloud).pin_memory()
        d40, d38 = torch.empty_like(pin_cloud, device=dev), torch.empty(h.n_bytes, dtype=torch.uint8, device=dev)
        up40 = events(lambda: d40.copy_(pin_cloud, non_blocking=True), a.runs)
        up38 = events(lambda: d38.copy_(pinned, non_blocking=True), a.runs)
        res = {"T": T, "bytes_block": h.n_bytes, "bytes_cloud": 40 * T, "same_bytes": same, "host_ms": stat(times["host"]),
               "device_ms": stat(times["device"]), **{k: stat(v) for k, v in parts.items()},
               "upload_40B_per_point_pinned_ms": stat(up40), "upload_block_pinned_ms": stat(up38)}
        out["routes"][name] = res
        print(f"[bench_las] {name}: {json.dumps(res)}", file=sys.stderr, flush=True)

    # ---- the kernel alone, staged and field by field, beside a device copy of the same bytes
    T = 3900000
    for fmt, L in ((8, 38), (6, 30), (6, 32), (8, 39), (6, 131)):
        raw = torch.from_numpy(np.frombuffer(block(T, fmt, L, 2), dtype=np.uint8).copy()).to(dev)
        h = las.LasHeader((1, 4), fmt, L, 375, T, (0.01,) * 3, (0.0,) * 3, (0.0,) * 3, (0.0,) * 3, 375)
        cloud = torch.empty(10, T, dtype=torch.float32, device=dev)
        moved = (L + 40) * T
        src, dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev), torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        res = {"T": T, "bytes_moved": moved}
        forms = {}
        for form, key in ((0, "staged"), (1, "direct")) if L <= 128 else ((0, "direct"),):     # beyond 128 bytes the rule is the direct form
            assert lib.sn2_debug_las_form(form) == 0
            try:
                ms = events(lambda: las.decode(raw, h, out=cloud), a.runs)
            finally:
                lib.sn2_debug_las_form(0)
            forms[key] = cloud.clone()
            res[key + "_ms"] = stat(ms)
            res[key + "_GBps"] = round(moved / statistics.median(ms) / 1e6, 1)
        if "staged" in forms:
            res["forms_same_bytes"] = bool(torch.equal(forms["staged"].view(torch.int32), forms["direct"].view(torch.int32)))
        cp = events(lambda: dst.copy_(src), a.runs)
        res["copy_same_bytes_ms"] = stat(cp)
        res["copy_GBps"] = round(moved / statistics.median(cp) / 1e6, 1)
        out["kernel"][f"fmt{fmt}_L{L}"] = res
        print(f"[bench_las] fmt{fmt} L{L}: {json.dumps(res)}", file=sys.stderr, flush=True)
    ten = out["routes"]["10ha"]
    print(json.dumps({"metric": "10 ha block (3.9e6 format-8 records) in host memory -> (10,T) fp32 on the device: upload + sn2_las_decode, "
                                "median of interleaved runs (host route beside it)", "value": ten["device_ms"]["median"], "unit": "ms",
                      "host_route_ms": ten["host_ms"]["median"], "n_gpus": 1, "results": out}))


if __name__ == "__main__":
    main()
