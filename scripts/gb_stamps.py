"""Diagnostic: phase stamps of workgroup 0 of global_level_bwd_kernel at the headline's shape (16 plots x 256 rows), the level's
backward alone, from a -DSN2_GB_STAMPS build of the library (global_level_bwd.hip) made into build/variants/ (never shipped).
    python scripts/gb_stamps.py [--build-only]"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from stratanet2_vegetation_coverage_maps_amd import _build, _lib
path = os.path.join(_build.VARIANT_DIR, "libgb_dbg.so")
if "--build-only" in sys.argv or not os.path.exists(path):
    path = _build.build_variant("libgb_dbg.so", ["-DSN2_GB_STAMPS"])
    if "--build-only" in sys.argv:
        sys.exit(0)
_lib.LIB_PATH = path
import torch
import test_gpu_global_level_backward as T
B, M2 = 16, 256
lv = T._Level(B, M2, *T._inputs(B, M2))
raw = ctypes.CDLL(path)
names = ["prefetch", "FP3 sums", "exchange 1", "dp, d x3", "FP3 contraction, exchange 2", "SA3 contraction", "commit"]
for it in range(6):
    lv.backward(True)
    out = (ctypes.c_ulonglong * 16)()
    raw.sn2_debug_gb_stamps(out)
    t = list(out)
    print(f"backward {it}: total {t[7] - t[0]} s_memtime ticks (~2.1 GHz here: 55 k = 26 us); " + "; ".join(f"{n} {t[i + 1] - t[i]}" for i, n in enumerate(names)), flush=True)
