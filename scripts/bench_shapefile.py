"""The parcel shapefile's two ends on one GPU: the .dbf records annotated on the device against the host route it replaces, and the
reader on a synthetic file.  K = 10^5 records of L = 200 bytes, four F fields of 50 bytes with 10 decimals.

  1. Interleaved pairs in one process, wall time: the DEVICE ROUTE (upload of records and values, the launch, the one read) and the
     HOST ROUTE it replaces (the Python `format` loop plus the `bytes` join); the bytes of both compared before anything is timed.
  2. The kernel alone (HIP events around REPEAT launches back to back, per launch) beside a device `copy_` of the same K (L + 200)
     bytes, in interleaved pairs.
  3. `shp.write_predictions` split into its phases -- upload, launch until done, read, files -- so that the device's share of the
     whole shows; and `shp.read` on a synthetic 10^5-parcel, 40-vertex file (host only).

    python scripts/bench_shapefile.py [--runs 11] [--records 100000]

Lines on stderr as they are measured, one JSON line on stdout."""
import argparse
import json
import os
import statistics
import struct
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stratanet2_vegetation_coverage_maps_amd import shp  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd.geotiff import SHP_FIELDS  # noqa: E402

REPEAT = 20          # launches per timed sample
SIZE, DECIMAL, L = 50, 10, 200


def stat(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def note(key, r):
    print(f"[bench_shapefile] {key}: {json.dumps(r)}", file=sys.stderr, flush=True)


def clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def synthetic_shapefile(base, K, V, rng):
    """K parcels of V-vertex outlines (closed rings of V + 1 points) and a .dbf of records of L bytes: ID C 12, SURF N 12.2, and a C
    field that fills the record.  Written with numpy, record by record layout as the format states it."""
    n = V + 1
    content = 44 + 4 + 16 * n
    rec = np.zeros((K, 8 + content), dtype=np.uint8)
    rec[:, 0:4] = np.arange(1, K + 1, dtype=">i4").view(np.uint8).reshape(K, 4)
    rec[:, 4:8] = np.frombuffer(struct.pack(">i", content // 2), dtype=np.uint8)
    rec[:, 8:12] = np.frombuffer(struct.pack("<i", 5), dtype=np.uint8)
    ang = np.linspace(0.0, 2 * np.pi, V, endpoint=False)
    cx, cy = 650000.0 + 100.0 * (np.arange(K) % 1000), 6860000.0 + 100.0 * (np.arange(K) // 1000)
    r = 30.0 + 10.0 * rng.random((K, V))
    x, y = cx[:, None] + r * np.cos(ang), cy[:, None] + r * np.sin(ang)
    pts = np.stack([np.concatenate([x, x[:, :1]], 1), np.concatenate([y, y[:, :1]], 1)], 2)          # (K, n, 2)
    box = np.stack([pts[:, :, 0].min(1), pts[:, :, 1].min(1), pts[:, :, 0].max(1), pts[:, :, 1].max(1)], 1)
    rec[:, 12:44] = box.astype("<f8").view(np.uint8).reshape(K, 32)
    rec[:, 44:52] = np.frombuffer(struct.pack("<ii", 1, n), dtype=np.uint8)
    rec[:, 52:56] = 0
    rec[:, 56:] = pts.astype("<f8").view(np.uint8).reshape(K, 16 * n)
    header = bytearray(100)
    struct.pack_into(">i", header, 0, 9994)
    struct.pack_into(">i", header, 24, (100 + rec.size) // 2)
    struct.pack_into("<ii", header, 28, 1000, 5)
    with open(base + ".shp", "wb") as f:
        f.write(bytes(header) + rec.tobytes())
    shx = np.zeros((K, 2), dtype=">i4")
    shx[:, 0] = (100 + np.arange(K) * (8 + content)) // 2
    shx[:, 1] = content // 2
    struct.pack_into(">i", header, 24, (100 + 8 * K) // 2)
    with open(base + ".shx", "wb") as f:
        f.write(bytes(header) + shx.tobytes())
    fields = [("ID", "C", 12, 0), ("SURF", "N", 12, 2), ("NOTE", "C", L - 25, 0)]
    h = bytearray(32 + 32 * len(fields) + 1)
    h[0], h[1], h[2], h[3] = 3, 124, 6, 11
    struct.pack_into("<IHH", h, 4, K, len(h), L)
    for i, (name, t, size, d) in enumerate(fields):
        o = 32 + 32 * i
        h[o:o + len(name)] = name.encode("ascii")
        h[o + 11], h[o + 16], h[o + 17] = ord(t), size, d
    h[-1] = 0x0D
    body = np.full((K, L), ord(" "), dtype=np.uint8)
    ids = np.char.encode(np.char.ljust(np.char.add("P", np.arange(K).astype(str)), 12), "ascii")
    body[:, 1:13] = np.frombuffer(b"".join(ids.tolist()), dtype=np.uint8).reshape(K, 12)
    body[:, 25:] = rng.integers(65, 91, size=(K, L - 25), dtype=np.uint8)
    with open(base + ".dbf", "wb") as f:
        f.write(bytes(h) + body.tobytes() + b"\x1a")


def host_route(records, values, cols):
    """what the device route replaces: the Python format loop plus the bytes join"""
    out = []
    for k in range(len(records)):
        out.append(records[k].tobytes())
        for c in cols:
            out.append(format(float(values[k, c]), ".10f")[:SIZE].rjust(SIZE).encode("ascii"))
    return b"".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--vertices", type=int, default=40)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shapefile: needs the GPU")
    if a.runs < 5:
        raise SystemExit("bench_shapefile: at least five runs")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(20240611)
    K = a.records
    cols = [c for _, c in SHP_FIELDS]
    out = {"runs": a.runs, "records": K, "record_bytes": L, "fields": len(cols), "size": SIZE, "decimal": DECIMAL}
    with tempfile.TemporaryDirectory() as d:
        base = os.path.join(d, "parcels")
        synthetic_shapefile(base, K, a.vertices, rng)
        # the reader, host only
        t_read = []
        for _ in range(max(5, a.runs // 2)):
            t0 = time.perf_counter()
            src = shp.read(base)
            t_read.append((time.perf_counter() - t0) * 1e3)
        out["read_ms"] = dict(stat(t_read), parcels=K, vertices=a.vertices, shp_bytes=os.path.getsize(base + ".shp"))
        note("read", out["read_ms"])
        values = rng.random((K, 6))                              # coverages in [0, 1), as band means are
        values[rng.random(K) < 0.01] = np.nan
        rows = np.arange(K, dtype=np.int32)

        def device_route():
            rec = torch.from_numpy(src.records).to(dev)
            val = torch.from_numpy(values).to(dev)
            return ops.dbf_annotate(rec, val, torch.from_numpy(rows).to(dev), cols, SIZE, DECIMAL, -1.0).read()
        same = device_route().records.tobytes() == host_route(src.records, values, cols)
        out["same_bytes_as_host_route"] = bool(same)
        note("same bytes as the host route", same)
        for _ in range(2):
            device_route()
        t_dev, t_host = [], []
        for _ in range(a.runs):
            t0 = clock()
            device_route()
            t1 = clock()
            host_route(src.records, values, cols)
            t2 = time.perf_counter()
            t_dev.append((t1 - t0) * 1e3)
            t_host.append((t2 - t1) * 1e3)
        out["device_route_ms"], out["host_route_ms"] = stat(t_dev), stat(t_host)
        out["host_over_device"] = round(statistics.median(t_host) / statistics.median(t_dev), 2)
        note("routes", {k: out[k] for k in ("device_route_ms", "host_route_ms", "host_over_device")})

        # the kernel alone beside a copy of the same bytes
        rec, val, row = torch.from_numpy(src.records).to(dev), torch.from_numpy(values).to(dev), torch.from_numpy(rows).to(dev)
        Ld = L + len(cols) * SIZE
        dst = torch.empty((K * Ld + 7) // 8 * 8 + 8, dtype=torch.uint8, device=dev)
        a_buf, b_buf = (torch.empty(K * Ld, dtype=torch.uint8, device=dev) for _ in range(2))

        def launch():
            for _ in range(REPEAT):
                ops.dbf_annotate(rec, val, row, cols, SIZE, DECIMAL, -1.0, out=dst)

        def copy():
            for _ in range(REPEAT):
                b_buf.copy_(a_buf)
        for _ in range(2):
            launch(), copy()
        ms_k, ms_c = [], []
        for _ in range(a.runs):
            ms_k.append(timed(launch) / REPEAT)
            ms_c.append(timed(copy) / REPEAT)
        moved = K * L + K * Ld + K * len(cols) * 8               # bytes read and written by the kernel
        out["kernel"] = {"output_bytes": K * Ld, "kernel_ms": stat(ms_k), "copy_same_bytes_ms": stat(ms_c),
                         "kernel_GBps": round(moved / statistics.median(ms_k) / 1e6, 1),
                         "copy_GBps": round(2 * K * Ld / statistics.median(ms_c) / 1e6, 1),
                         "kernel_over_copy": round(statistics.median(ms_k) / statistics.median(ms_c), 2)}
        note("kernel", out["kernel"])

        # write_predictions in its phases
        ph = []
        names = [n for n, _ in SHP_FIELDS]
        for i in range(a.runs):
            t0 = clock()
            r_dev, v_dev, i_dev = torch.from_numpy(src.records).to(dev), torch.from_numpy(values).to(dev), torch.from_numpy(rows).to(dev)
            t1 = clock()
            done = ops.dbf_annotate(r_dev, v_dev, i_dev, cols, SIZE, DECIMAL, -1.0)
            t2 = clock()
            done.read()
            t3 = time.perf_counter()
            shp.write_annotated(src, os.path.join(d, "out_phases"), names, SIZE, DECIMAL, done.records)
            t4 = time.perf_counter()
            shp.write_predictions(src, os.path.join(d, "out_whole"), values, device=dev)
            t5 = clock()
            ph.append({"upload": (t1 - t0) * 1e3, "launch_until_done": (t2 - t1) * 1e3, "read": (t3 - t2) * 1e3, "files": (t4 - t3) * 1e3,
                       "write_predictions": (t5 - t4) * 1e3})
        out["phases_ms"] = {k: stat([p[k] for p in ph]) for k in ph[0]}
        out["written_bytes"] = sum(os.path.getsize(os.path.join(d, "out_whole" + e)) for e in (".shp", ".shx", ".dbf"))
        note("phases", out["phases_ms"])
    print(json.dumps({"metric": f"{K} dBase records of {L} bytes annotated with four F fields: upload, one launch, one read "
                                "(median of interleaved runs; the Python format loop beside it)",
                      "value": out["device_route_ms"]["median"], "unit": "ms", "host_route_ms": out["host_route_ms"]["median"],
                      "n_gpus": 1, "results": out}))


if __name__ == "__main__":
    main()
