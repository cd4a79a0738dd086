"""From the band arena of a parcel report on the device to GeoTIFF files, on one GPU.  Two workloads: the 10 ha canvas
(335 x 335 x 6, filled by tiling a real report canvas) and the 16-parcel atlas of scripts/bench_parcels.py (100 m parcels, six
bands after `report(shapes, admissibility=5)`).

  1. The pack launch alone (sn2_tiff_pack on a place table made before; HIP events around 50 launches back to back, per launch)
     beside a device `copy_` of the same bytes -- the kernel reads the blocks' bytes once and writes them once, as the copy does --
     in interleaved pairs: median and range of both, the ratio copy / kernel, for both layouts, both predictors, and the direct
     form; and `hip_ops.tiff_pack` with what it does around the launch (place table, its upload, the statistics' initialisation).
  2. `geotiff.write_atlas` split into its phases -- pack (launch until done), read (the one device-to-host copy), zlib, file (header,
     assembly, write) -- with deflate + predictor 3 (the default) and without compression.
  3. The same files by the host route, per canvas `.cpu()`, numpy transpose and predictor, zlib and write
     (tests/_geotiff_ref.py: assemble), interleaved with `write_atlas`, wall time: median and range of both.
  Before anything is timed the 16 files are read back (`geotiff.read`, and band 0 through libtiff) and compared with the report.

    python scripts/bench_geotiff.py [--runs 11] [--parcels 16]

Lines on stderr as they are measured, one JSON line on stdout."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _geotiff_ref as R  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd import PointNet2, _lib, geotiff, parcel  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_parcel  # noqa: E402

SEED = 20240611
REPEAT = 50          # launches per timed sample: one launch of a few microseconds measures the clock


def stat(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def pairs(fn_a, fn_b, runs):
    for _ in range(2):
        fn_a(), fn_b()
    ms_a, ms_b = [], []
    for _ in range(runs):
        ms_a.append(timed(fn_a))
        ms_b.append(timed(fn_b))
    return ms_a, ms_b


def clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def kernel_cases(name, arena, C, table, runs, lib, out):
    """1: every layout and predictor, and the direct form, beside a copy of the blocks' bytes"""
    for layout_name, layout in (("band", R.BAND), ("pixel", R.PIXEL)):
        for predictor in (1, 3):
            for form in (0, 1):
                if form == 1 and predictor == 1:
                    continue
                assert lib.sn2_debug_tiff_pack_form(form) == 0
                try:
                    total = int(ops.tiff_place_table(table.host, C, layout)[-1, 3])
                    dst = torch.empty(total, dtype=torch.uint8, device=arena.device)
                    blocks = 4 * arena.numel()
                    src, cpy = (torch.empty(blocks, dtype=torch.uint8, device=arena.device) for _ in range(2))
                    packed = ops.tiff_pack(arena, C, table, layout, predictor, out=dst)
                    place, place_dev = packed.place, packed._place_dev

                    def launch():                # the entry point alone: the statistics keep accumulating, the bytes are the same
                        for _ in range(REPEAT):
                            ops._call("sn2_tiff_pack", ops._ptr(arena), C, table.K, table.host.ctypes.data, ops._ptr(table.dev),
                                      place.ctypes.data, ops._ptr(place_dev), layout, predictor, ops._ptr(dst), dst.numel(), ops._stream())

                    def copy():
                        for _ in range(REPEAT):
                            cpy.copy_(src)

                    def wrapper():
                        for _ in range(REPEAT):
                            ops.tiff_pack(arena, C, table, layout, predictor, out=dst)
                    ms_k, ms_c = (([t / REPEAT for t in v]) for v in pairs(launch, copy, runs))
                    ms_w = [t / REPEAT for t in pairs(wrapper, lambda: None, runs)[0]]
                finally:
                    lib.sn2_debug_tiff_pack_form(0)
                r = {"block_bytes": blocks, "kernel_ms": stat(ms_k), "copy_same_bytes_ms": stat(ms_c), "pack_with_its_setup_ms": stat(ms_w),
                     "kernel_GBps": round(2 * blocks / statistics.median(ms_k) / 1e6, 1),
                     "copy_GBps": round(2 * blocks / statistics.median(ms_c) / 1e6, 1),
                     "copy_over_kernel": round(statistics.median(ms_c) / statistics.median(ms_k), 3)}
                key = f"{name}_{layout_name}_p{predictor}_{'direct' if form else 'rule'}"
                out[key] = r
                print(f"[bench_geotiff] {key}: {json.dumps(r)}", file=sys.stderr, flush=True)


def phases(paths, atlas, rep, compress):
    """2: write_atlas's own steps, timed one by one (the same calls in the same order)"""
    K = len(rep)
    predictor = geotiff._predictor(None, compress)
    skip = [bool(rep.empty[k]) for k in range(K)]
    t0 = clock()
    packed = geotiff.pack(rep.band_arena, rep.n_bands, rep.table, "band", predictor, skip)
    t1 = clock()
    packed.read()
    t2 = time.perf_counter()
    spent = {"zlib": 0.0}
    real = zlib.compress

    def counted(data, level=-1):
        t = time.perf_counter()
        r = real(data, level)
        spent["zlib"] += time.perf_counter() - t
        return r
    geotiff.zlib = type("Z", (), {"compress": staticmethod(counted), "decompress": staticmethod(zlib.decompress)})
    try:
        geos = [rep.table.geo(k) for k in range(K)]
        geotiff._write_packed([None if skip[k] else paths[k] for k in range(K)], packed, [rep.table.shape(k) for k in range(K)], geos,
                              atlas.pix, rep.band_means, compress, predictor, "band", None, 2154, 6, None, True)
    finally:
        geotiff.zlib = zlib
    t3 = time.perf_counter()
    return {"pack": (t1 - t0) * 1e3, "read": (t2 - t1) * 1e3, "zlib": spent["zlib"] * 1e3, "file": (t3 - t2 - spent["zlib"]) * 1e3,
            "whole": (t3 - t0) * 1e3}


def host_route(paths, atlas, rep, compress):
    """3: per canvas .cpu(), numpy transpose and predictor, zlib and write"""
    deflate = compress == "deflate"
    for k, p in enumerate(paths):
        if rep.empty[k]:
            continue
        b = rep.bands(k).cpu().numpy()
        x_min, y_max = rep.table.geo(k)
        data = R.assemble(b, x_min, y_max, atlas.pix, R.BAND, 3 if deflate else 1, deflate)
        with open(p, "wb") as f:
            f.write(data)


class OneCanvas:
    """what write_atlas needs of an atlas and its report, for one canvas of bands on the device"""

    def __init__(self, bands, pix):
        C, H, W = bands.shape
        self.pix, self.n_bands, self.empty = pix, C, [False]
        self.table = ops.AtlasTable([H], [W], [650000.0], [6860000.0], device=bands.device)
        self.band_arena = bands.contiguous().view(-1)
        valid = ~torch.isnan(bands)
        n = valid.sum(dim=(1, 2)).cpu().numpy()
        s = torch.where(valid, bands, torch.zeros_like(bands)).double().sum(dim=(1, 2)).cpu().numpy()
        self.band_means, self.band_counts = (s / np.maximum(n, 1))[None], n[None]

    def __len__(self):
        return 1

    def bands(self, k):
        return self.table.view(self.band_arena, self.n_bands, k)


def file_cases(name, atlas, rep, runs, d, out):
    K = len(rep)
    for compress in ("deflate", None):
        tag = f"{name}_{compress or 'plain'}"
        dev_paths = [os.path.join(d, f"{tag}_dev_{k}.tif") for k in range(K)]
        host_paths = [os.path.join(d, f"{tag}_host_{k}.tif") for k in range(K)]
        for _ in range(2):
            geotiff.write_atlas(dev_paths, atlas, rep, compress=compress)
            host_route(host_paths, atlas, rep, compress)
        same = all(rep.empty[k] or bits(geotiff.read(dev_paths[k])["bands"]).tobytes() == bits(geotiff.read(host_paths[k])["bands"]).tobytes()
                   for k in range(K))
        t_dev, t_host, ph = [], [], []
        for _ in range(runs):
            t0 = clock()
            geotiff.write_atlas(dev_paths, atlas, rep, compress=compress)
            t1 = clock()
            host_route(host_paths, atlas, rep, compress)
            t2 = clock()
            t_dev.append((t1 - t0) * 1e3)
            t_host.append((t2 - t1) * 1e3)
            ph.append(phases(dev_paths, atlas, rep, compress))
        r = {"files": sum(not e for e in rep.empty), "file_bytes": sum(os.path.getsize(p) for k, p in enumerate(dev_paths) if not rep.empty[k]),
             "same_bands_as_host_route": same, "write_atlas_ms": stat(t_dev), "host_route_ms": stat(t_host),
             "host_over_device": round(statistics.median(t_host) / statistics.median(t_dev), 3),
             "phases_ms": {k: stat([p[k] for p in ph]) for k in ph[0]}}
        out[tag] = r
        print(f"[bench_geotiff] {tag}: {json.dumps(r)}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--parcels", type=int, default=16)
    ap.add_argument("--side", type=float, default=100.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_geotiff: needs the GPU")
    if a.runs < 5:
        raise SystemExit("bench_geotiff: at least five runs")
    dev = torch.device("cuda:0")
    lib = _lib.load()
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
    atlas, _ = parcel.predict_parcels(model, clouds, args, shapes=rings, batch_size=512, fps_start=0, sampler="device", seed=SEED)
    rep = atlas.report(rings, admissibility=5)
    torch.cuda.synchronize()
    out = {"runs": a.runs, "parcels": K, "canvases": [list(rep.table.shape(k)) for k in range(K)], "kernel": {}, "files": {}}

    # the 10 ha canvas: a real canvas of the report, tiled to 335 x 335
    b0 = rep.bands(0)
    iy, ix = torch.arange(335, device=dev) % b0.shape[1], torch.arange(335, device=dev) % b0.shape[2]
    big = OneCanvas(b0[:, iy][:, :, ix].contiguous(), atlas.pix)

    with tempfile.TemporaryDirectory() as d:
        # the deliverable first: 16 files, read back to the report's bytes
        paths = [os.path.join(d, f"parcel_{k}.tif") for k in range(K)]
        done = geotiff.write_atlas(paths, atlas, rep)
        ok_read = ok_pil = True
        from PIL import Image, features
        for k, p in enumerate(done):
            if p is None:
                continue
            want = rep.bands(k).cpu().numpy()
            r = geotiff.read(p)
            ok_read &= bits(r["bands"]).tobytes() == bits(want).tobytes()
            if features.check("libtiff"):
                data, t = open(p, "rb").read(), r["tags"]
                per = len(t[273]) // rep.n_bands
                one = os.path.join(d, "band0.tif")
                with open(one, "wb") as f:
                    f.write(R.single_band_file([data[o:o + n] for o, n in zip(t[273][:per], t[279][:per])], want.shape[1], want.shape[2],
                                               t[278][0], True, 3))
                ok_pil &= bits(np.array(Image.open(one))).tobytes() == bits(want[0]).tobytes()
        out["deliverable"] = {"files": sum(p is not None for p in done), "read_gives_the_reports_bytes": bool(ok_read),
                              "libtiff_band0_gives_the_reports_bytes": bool(ok_pil) if features.check("libtiff") else None}
        print(f"[bench_geotiff] deliverable: {json.dumps(out['deliverable'])}", file=sys.stderr, flush=True)

        kernel_cases("canvas335", big.band_arena, 6, big.table, a.runs, lib, out["kernel"])
        kernel_cases(f"atlas{K}", rep.band_arena, rep.n_bands, rep.table, a.runs, lib, out["kernel"])
        file_cases("canvas335", big, big, a.runs, d, out["files"])
        file_cases(f"atlas{K}", atlas, rep, a.runs, d, out["files"])
    key = f"atlas{K}_deflate"
    print(json.dumps({"metric": f"{K} parcel canvases (six bands) on the device -> {K} deflate GeoTIFF files with predictor 3 "
                                "(geotiff.write_atlas), median of interleaved runs (host route beside it)",
                      "value": out["files"][key]["write_atlas_ms"]["median"], "unit": "ms",
                      "host_route_ms": out["files"][key]["host_route_ms"]["median"], "n_gpus": 1, "results": out}))


if __name__ == "__main__":
    main()
