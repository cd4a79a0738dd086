"""The compiler's resource usage of the library's kernels, one line per instantiation (no GPU needed).

    python scripts/resource_usage.py [--match REGEX] [--csrc DIR] file.hip ...  > resource_usage.txt

Compiles each file of csrc/ with the build's flags plus `-Rpass-analysis=kernel-resource-usage` (device code only), demangles the
kernel names and prints `kernel | SGPRs | VGPRs | AGPRs | scratch bytes/lane | VGPR spill | static LDS bytes/block | waves/SIMD`,
sorted by name: the format of profiles/*/resource_usage_*.txt.  `--csrc` points at another tree's csrc/ (the parent commit's,
checked out beside this one) so that both sides are taken with the same compiler and flags.
"""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")


def usage_of(path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wno-unused-result", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o", os.devnull]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise SystemExit(f"hipcc failed on {path}:\n{r.stdout}")
    out, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for f in FIELDS:
            m = re.search(re.escape(f) + r": (\d+)", line)
            if m and (f != "VGPRs" or "Spill" not in line) and (f != "SGPRs" or "Spill" not in line):
                cur[f] = int(m.group(1))
    return out


def demangle(names):
    filt = os.path.join(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), "..", "llvm", "bin", "llvm-cxxfilt")
    r = subprocess.run([filt if os.path.exists(filt) else "c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True)
    return r.stdout.splitlines()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--match", default=".")
    ap.add_argument("--csrc", default=os.path.join(ROOT, "stratanet2_vegetation_coverage_maps_amd", "csrc"))
    ap.add_argument("files", nargs="+")
    a = ap.parse_args()
    rows = {}
    for f in a.files:
        rows.update(usage_of(os.path.join(a.csrc, f)))
    names = list(rows)
    lines = []
    for mangled, plain in zip(names, demangle(names)):
        short = re.sub(r"^(void )?(\(anonymous namespace\)::)?", "", plain)      # (a plain function's mangled name has no return type)
        short = re.sub(r"\(.*$", "", short)
        if re.search(a.match, short):
            lines.append(" | ".join([short] + [str(rows[mangled].get(f, "?")) for f in FIELDS]))
    print("kernel | SGPRs | VGPRs | AGPRs | scratch bytes/lane | VGPR spill | static LDS bytes/block | waves/SIMD")
    print("\n".join(sorted(lines)))


if __name__ == "__main__":
    sys.exit(main())
