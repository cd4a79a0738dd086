"""In-tree build of libstrata_hip.so (gfx950 only).  `hipcc` cross-compiles without a GPU.

    python -m stratanet2_vegetation_coverage_maps_amd._build [--force]

Diagnostic variants of the library (scripts/: phase stamps, timing switches) are made by `build_variant`, from the same
source list and flags, into build/variants/.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(CSRC, "libstrata_hip.so")
VARIANT_DIR = os.path.join(os.path.dirname(HERE), "build", "variants")      # (build/ is ignored by git)
SOURCES = ["geometry.hip", "ball_query.hip", "three_nn.hip", "znorm.hip", "sa.hip", "sa_mfma.hip", "fp.hip", "interp_index.hip", "global_level.hip", "global_level_bwd.hip", "head.hip", "project.hip",
           "loss.hip", "misc.hip", "net.hip", "parcel.hip", "parcels.hip", "sample.hip", "kde.hip", "feed.hip", "plotset.hip", "atlas.hip", "indicators.hip", "points.hip",
           "admissibility.hip", "las.hip", "cut.hip", "las_write.hip", "tiff_pack.hip", "ortho.hip", "dbf.hip"]
HEADERS = ["common.h", "philox.h", "mlp.h", "fp_rows.h", "global_level.h", "loss_rules.h", "mosaic_rules.h", "projection_rules.h", "parcel_rules.h", "plot_sort.h", "fps_ws.h", "point_rules.h",
           "atlas_table.h", "admissibility_rules.h", "las_rules.h", "cut_rules.h", "las_write_rules.h", "tiff_rules.h", "ortho_rules.h", "dbf_rules.h", os.path.join("..", "..", "include", "strata_hip.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wno-unused-result"] + os.environ.get("SN2_EXTRA_HIPCC_FLAGS", "").split()


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _compile(lib, objdir, flags, force, verbose):
    """SOURCES -> object files in `objdir` (those older than their source or a header, or all) -> the shared library `lib`."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    objs, jobs = [], []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(objdir, s.replace(".hip", ".o"))
        objs.append(obj)
        if force or _stale(obj, [src] + hdrs):
            jobs.append([hipcc] + flags + ["-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed ({r.returncode}):\n{r.stdout}")
        return r.stdout

    with ThreadPoolExecutor(max_workers=min(4, max(1, len(jobs)))) as ex:
        list(ex.map(run, jobs))
    if force or jobs or _stale(lib, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", lib])
    return lib


def build(force: bool = False, verbose: bool = True) -> str:
    return _compile(LIB, CSRC, FLAGS, force, verbose)


def build_variant(name: str, extra_flags=(), verbose: bool = False) -> str:
    """The current SOURCES compiled with FLAGS + `extra_flags` (e.g. ["-DSN2_GL_STAMPS"]) into the shared library
    VARIANT_DIR/`name` (a path of its own is taken as it is, but must lie outside csrc/): the shipped library and its object
    files are not touched.  Always a full build (the flags differ from call to call); the object files go to <library>.objs/.
    Load it by setting `_lib.LIB_PATH` to the returned path before the first `_lib.load()`."""
    out = os.path.abspath(os.path.join(VARIANT_DIR, name))
    if os.path.commonpath([out, CSRC]) == CSRC:
        raise ValueError(f"{out}: a variant build must not go into {CSRC}")
    objdir = out + ".objs"
    os.makedirs(objdir, exist_ok=True)
    return _compile(out, objdir, FLAGS + list(extra_flags), True, verbose)


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
