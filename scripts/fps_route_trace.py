"""Which kernels farthest point sampling launches (profiles/fps_route): hip_ops.fps over the sizes and `waves` of
tests/test_gpu_fps_route.py (every template rung of every FPS ladder, 32 samples) and 16 x 32768 -> 1024 with waves 0 and 8.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python scripts/fps_route_trace.py        (the workload)
    python scripts/fps_route_trace.py --list OUT/.../*_kernel_trace.csv > launches.txt                (its launch list)

The list: per stream, in dispatch order, (name, grid, workgroup, LDS bytes) of every kernel whose name starts with fps_ or
spatial_order.  Two commits whose dispatch is the same give the same file."""
import csv
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (B, N, M, waves, bucketed): the cases of tests/test_gpu_fps_route.py, then the benchmark's shape
CASES = ([(2, n, 32, 0, False) for n in (256, 257, 512, 513, 1024, 1025, 2048, 2052, 4100, 8196, 16388)] + [(33, 4096, 32, 0, False)] +
         [(1, n, 32, w, True) for n in (2052, 4100, 8196, 16388, 32772, 65540) for w in (16, 8, 4, 1) if (n, w) != (65540, 4)] +
         [(1, n, 32, w, True) for w, n in ((34, 4036), (36, 8132), (40, 16324), (66, 2052), (68, 4036), (72, 8132))] +
         [(16, 32768, 1024, 0, True), (16, 32768, 1024, 8, True)])


def workload():
    import torch
    from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
    for B, N, M, waves, bucketed in CASES:
        g = torch.Generator().manual_seed(1000 * B + N)
        pos = torch.rand(B, N, 3, generator=g) * torch.tensor([20.0, 20.0, 8.0])
        pos[:, N - N // 4:] = pos[:, :N // 4]
        start = torch.tensor([(977 * b + 13) % N for b in range(B)]).to("cuda:0", torch.int32)
        idx, _, _ = ops.fps(pos.permute(0, 2, 1).contiguous().to("cuda:0"), M, start, bucketed=bucketed, waves=waves)
        torch.cuda.synchronize()
        print(f"{B} x {N} -> {M}, waves={waves}, bucketed={bucketed}: index sum {int(idx.sum())}", flush=True)


def launches(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Dispatch_Id"]))
    streams = {}
    for r in rows:
        name = re.sub(r"\(anonymous namespace\)::", "", r["Kernel_Name"]).replace("void ", "").split("(")[0]
        if not name.startswith(("fps_", "spatial_order")):
            continue
        key = r.get("Stream_Id", r["Queue_Id"])
        streams.setdefault(key, []).append(
            "%s grid %s,%s,%s wg %s,%s,%s lds %s" % ((name,) + tuple(r[f"Grid_Size_{a}"] for a in "XYZ") +
                                                     tuple(r[f"Workgroup_Size_{a}"] for a in "XYZ") + (r["LDS_Block_Size"],)))
    for i, (_, ks) in enumerate(streams.items()):          # streams in the order of their first launch
        print(f"# stream {i}: {len(ks)} launches")
        print("\n".join(ks))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--list":
        launches(sys.argv[2])
    else:
        workload()
