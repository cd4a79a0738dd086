"""Per-level figures of the inverted-index kernels from rocprofv3 output (profiles/interp_order/README.md).

    python scripts/interp_order_profile.py trace KERNEL_TRACE.csv [name filter ...]
        per (kernel, grid): launches, mean and fastest duration in us (the first launch of every row left out when there are
        more than two), and the sum of ALL kernel durations of the run in ms
    python scripts/interp_order_profile.py pmc COUNTER_COLLECTION.csv [name filter ...]
        per (kernel, grid): launches and the mean of every counter (FETCH_SIZE / WRITE_SIZE: KiB)

The grid is what the trace calls it (work-items per axis): a level of inv_hist / inv_fill is told from another by it.
"""
import collections
import csv
import re
import sys

DEFAULT = ("inv_hist", "inv_fill", "inv_scan", "inv_order", "three_nn_grid_kernel", "nn_target_sort")


def short(name):
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    return re.sub(r"^void ", "", name).split("(")[0]


def grid_of(r):
    if "Grid_Size" in r:                 # (counter collection: one number)
        return r["Grid_Size"]
    return "x".join(r[k] for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z") if r.get(k, "1") not in ("1", "")) or "1"


SHAPES = [(160, 32768), (256, 10000)]          # (plots, points): ten headline batches per geometry pass; the parcel loop's batch
REPS = 10


def workload():
    """The per-point 3-NN search and its inverted index alone, on one stream (a kernel's duration is its own), at SHAPES with
    1024 sources per plot: uniform random plots of 20 x 20 x 8 m.  The library's SN2_INV_* switches choose the form."""
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
    for B, N in SHAPES:
        g = torch.Generator().manual_seed(B + N)
        pos = (torch.rand(B, 3, N, generator=g) * torch.tensor([20.0, 20.0, 8.0]).view(1, 3, 1)).to("cuda:0")
        _, c1, a1 = ops.fps(pos, 1024, None)[:3]
        ws = torch.empty(ops.three_nn_ws_words(B, 1024, N), dtype=torch.int32, device="cuda:0")
        for _ in range(REPS):
            knn = ops.three_nn(c1, pos, 3, ws=ws, sorted_copy=True)
            order, si, sw = ops.three_nn_order(ws, B, 1024, N)
            inv = ops.interp_index(knn, B, N, 1024, src_pos=a1, row_order=order, sorted_table=(si, sw))
        torch.cuda.synchronize()
        print(f"{B} x {N}: index sum {int(knn[0].sum())}, list words {int(inv.view(torch.int32)[:B * 1024].sum())}", flush=True)


def main():
    if sys.argv[1] == "workload":
        return workload()
    mode, path, filt = sys.argv[1], sys.argv[2], tuple(sys.argv[3:]) or DEFAULT
    rows = csv.DictReader(open(path))
    if mode == "trace":
        acc, total = collections.defaultdict(list), 0
        for r in rows:
            d = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
            total += d
            k = short(r["Kernel_Name"])
            if any(f in k for f in filt):
                acc[(k, grid_of(r))].append(d)
        print("kernel | grid | launches | mean us | fastest us")
        for (k, g), v in sorted(acc.items()):
            v = v[1:] if len(v) > 2 else v
            print(f"{k} | {g} | {len(v)} | {sum(v) / len(v) / 1e3:.2f} | {min(v) / 1e3:.2f}")
        print(f"sum of all kernel durations: {total / 1e6:.2f} ms")
    elif mode == "pmc":
        acc = collections.defaultdict(lambda: collections.defaultdict(list))
        for r in rows:
            k = short(r["Kernel_Name"])
            if any(f in k for f in filt):
                acc[(k, grid_of(r))][r["Counter_Name"]].append(float(r["Counter_Value"]))
        print("kernel | grid | launches | counter means")
        for (k, g), d in sorted(acc.items()):
            n = max(len(v) for v in d.values())
            print(f"{k} | {g} | {n} | " + ", ".join(f"{c} {sum(v) / len(v):.0f}" for c, v in sorted(d.items())))
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main()
