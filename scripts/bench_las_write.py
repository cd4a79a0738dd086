"""From per-point scores on the device to a scored LAS file, on one GPU.  The workload is the 10 ha block of scripts/bench_las.py:
3.9e6 format-8 records of 38 bytes, all ten fields appended (76-byte records), classified.

  1. The kernel alone (sn2_las_encode, HIP events), its staged and its byte-by-byte form, beside a device `copy_` of the bytes it
     must move, (L_src + L_dst + 40) T (the source record, the written record, ten 4-byte score values per point), in interleaved
     pairs: median and range of both and the ratio copy time / kernel time (1 = the kernel moves its bytes as fast as a copy does).
  2. The same with a point_index (the gathered form: every lane fetches its own record): a random permutation, the worst case,
     and an ascending index with repeats and gaps, the order a ParcelCut's index has inside a parcel.
  3. `las.write_scored` end to end (read the source file, upload, encode, one device-to-host copy, write the file) beside the host
     route it replaces (read the source records, `.cpu()` of scores, weight and hits, numpy structured packing
     (tests/_las_write_ref.py: encode_ref), tobytes, write the same frame), interleaved, wall time; and both without the files.

    python scripts/bench_las_write.py [--runs 15] [--points 3900000]

Lines on stderr as they are measured, one JSON line on stdout."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _las_ref as R  # noqa: E402
import _las_write_ref as W  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd import _lib, las  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd.inference import PointScoreResult  # noqa: E402

CODES = (3, 2, 4, 5)


def stat(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def fields(T, seed):
    rng = np.random.default_rng(seed)
    f = dict(X=rng.integers(65000000, 65031630, T), Y=rng.integers(686000000, 686031630, T), Z=rng.integers(20000, 24000, T),
             returns=rng.integers(0, 256, T), classification=rng.integers(0, 32, T))
    for k in ("intensity", "red", "green", "blue", "nir"):
        f[k] = rng.integers(0, 65536, T)
    return f


def scores_of(T, seed):
    """what sn2_points_finalize leaves: a fifth of the points unscored (NaN scores, weight 0, hits 0)"""
    rng = np.random.default_rng(seed)
    s = rng.random((8, T), dtype=np.float32)
    w = rng.random(T, dtype=np.float32) * 3
    h = rng.integers(1, 9, size=T).astype(np.int32)
    un = rng.random(T) < 0.2
    s[:, un], w[un], h[un] = np.nan, 0.0, 0
    return s, w.astype(np.float32), h


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def pairs(fn_a, fn_b, runs):
    """fn_a and fn_b by HIP events in interleaved pairs after a warm-up -> (ms of a, ms of b)"""
    for _ in range(2):
        fn_a(), fn_b()
    ms_a, ms_b = [], []
    for _ in range(runs):
        ms_a.append(timed(fn_a))
        ms_b.append(timed(fn_b))
    return ms_a, ms_b


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--points", type=int, default=3900000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_las_write: needs the GPU")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    T, L = a.points, 38
    L_dst = L + 38
    blob = R.write_las(fields(T, 1), 8, L, (1, 4), legacy_count=0)
    recs = blob[375:]
    s, w, h = scores_of(T, 2)
    res = PointScoreResult(torch.from_numpy(s).to(dev), torch.from_numpy(w).to(dev), torch.from_numpy(h).to(dev))
    raw = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to(dev)
    header = las.read_header(blob)
    kw = dict(fields="all", classify=True)
    out = {"runs": a.runs, "T": T, "L_src": L, "L_dst": L_dst, "kernel": {}}

    # ---- 1, 2: the kernel alone beside a copy of the bytes it moves
    moved = (L + L_dst + 40) * T
    src, dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev), torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    dest = torch.empty(T * L_dst, dtype=torch.uint8, device=dev)
    stats = ops.LasEncodeStats(dev)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(T).astype(np.int32)).to(dev)
    want, _ = W.encode_ref(recs, 8, L, T, s, w, h, mask=0x3FF, class_codes=CODES)
    asc = torch.from_numpy(np.sort(np.random.default_rng(4).integers(0, T, size=T)).astype(np.int32)).to(dev)
    for index, tag in ((None, "identity"), (perm, "gathered_random"), (asc, "gathered_ascending")):
        for form, key in ((0, "staged"), (1, "direct")):
            assert lib.sn2_debug_las_encode_form(form) == 0
            try:
                ms_k, ms_c = pairs(lambda: las.encode(raw, header, res, point_index=index, out=dest, stats=stats, **kw),
                                   lambda: dst.copy_(src), a.runs)
            finally:
                lib.sn2_debug_las_encode_form(0)
            r = {"bytes_moved": moved, "kernel_ms": stat(ms_k), "copy_same_bytes_ms": stat(ms_c),
                 "kernel_GBps": round(moved / statistics.median(ms_k) / 1e6, 1), "copy_GBps": round(moved / statistics.median(ms_c) / 1e6, 1),
                 "copy_over_kernel": round(statistics.median(ms_c) / statistics.median(ms_k), 3)}
            if index is None:
                r["same_bytes_as_numpy"] = dest.cpu().numpy().tobytes() == want
            out["kernel"][f"{tag}_{key}"] = r
            print(f"[bench_las_write] {tag} {key}: {json.dumps(r)}", file=sys.stderr, flush=True)

    # ---- 3: write_scored beside the host route, files included and without them
    with tempfile.TemporaryDirectory() as d:
        src_path, dst_dev, dst_host = (os.path.join(d, n) for n in ("src.las", "device.las", "host.las"))
        with open(src_path, "wb") as f:
            f.write(blob)
        head, tail = las.patch_header(blob, T, 0x3FF)

        def device_files():
            las.write_scored(src_path, dst_dev, res, **kw)

        def host_files():
            with open(src_path, "rb") as f:
                f.seek(375)
                r = f.read(T * L)
            packed, _ = W.encode_ref(r, 8, L, T, res.scores.cpu().numpy(), res.weight.cpu().numpy(), res.hits.cpu().numpy(), mask=0x3FF,
                                     class_codes=CODES)
            with open(dst_host, "wb") as f:
                f.write(head)
                f.write(packed)
                f.write(tail)

        def device_memory():
            las._to_host(las.encode(raw, header, res, **kw)[0])

        def host_memory():
            W.encode_ref(recs, 8, L, T, res.scores.cpu().numpy(), res.weight.cpu().numpy(), res.hits.cpu().numpy(), mask=0x3FF,
                         class_codes=CODES)
        for fn in (device_files, host_files, device_memory, host_memory):
            fn()
        with open(dst_dev, "rb") as f1, open(dst_host, "rb") as f2:
            b1, b2 = f1.read(), f2.read()
        same = b1[len(head):] == b2[len(head):] and len(b1) == len(b2)       # (the host route's header carries no statistics)
        t = {k: [] for k in ("device_files", "host_files", "device_memory", "host_memory")}
        for _ in range(a.runs):
            for k, fn in (("device_files", device_files), ("host_files", host_files), ("device_memory", device_memory),
                          ("host_memory", host_memory)):
                t[k].append(wall(fn))
    out["write_scored"] = {"file_bytes": len(b1), "same_point_bytes": same, **{k + "_ms": stat(v) for k, v in t.items()}}
    print(f"[bench_las_write] write_scored: {json.dumps(out['write_scored'])}", file=sys.stderr, flush=True)
    print(json.dumps({"metric": "10 ha block (3.9e6 format-8 records) + per-point scores on the device -> scored LAS file "
                                "(las.write_scored, all ten fields, classified), median of interleaved runs (host route beside it)",
                      "value": out["write_scored"]["device_files_ms"]["median"], "unit": "ms",
                      "host_route_ms": out["write_scored"]["host_files_ms"]["median"], "n_gpus": 1, "results": out}))


if __name__ == "__main__":
    main()
