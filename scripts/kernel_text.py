"""The compiler's assembly text of the library's kernels as one hash per instantiation (no GPU needed).

    python scripts/kernel_text.py [--csrc DIR] file.hip ...  > kernel_text.txt

Compiles each file of csrc/ with the build's flags plus `--cuda-device-only -S`, cuts the assembly per kernel symbol from its label
to its `.Lfunc_end`, drops comments and the `.loc` / `.file` / `.cfi` lines, takes the function index out of the local labels
(`.LBB<f>_<n>` -> `.LBB_<n>`: a kernel's index in its unit changes when the kernel moves to another unit) and prints
`demangled kernel | sha1` sorted by name.  Two trees whose listings are equal give every kernel the same instructions: the proof
that a change only moved code (profiles/geometry_units/).  `--csrc` points at another tree's csrc/, as in resource_usage.py.
It compares text and knows no instruction by name.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys

from resource_usage import ROOT, demangle


def kernels_of(path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wno-unused-result", "--cuda-device-only", "-S", path, "-o", "-"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise SystemExit(f"hipcc failed on {path}:\n{r.stderr}")
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)", r.stdout, re.M):
        body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), r.stdout, re.M | re.S).group(1)
        lines = [re.sub(r"\s*;.*$", "", line).strip() for line in body.splitlines()]
        lines = [re.sub(r"\.LBB\d+_", ".LBB_", line) for line in lines if line and not re.match(r"\.(loc|file|cfi)", line)]
        out[name] = hashlib.sha1("\n".join(lines).encode()).hexdigest()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(ROOT, "stratanet2_vegetation_coverage_maps_amd", "csrc"))
    ap.add_argument("files", nargs="+")
    a = ap.parse_args()
    rows = {}
    for f in a.files:
        for name, sha in kernels_of(os.path.join(a.csrc, f)).items():
            if rows.setdefault(name, sha) != sha:        # (a static kernel of a header, compiled into several units)
                raise SystemExit(f"{name}: its text in {f} differs from an earlier unit's")
    names = list(rows)
    plain = [re.sub(r"\(.*$", "", re.sub(r"^(void )?(\(anonymous namespace\)::)?", "", p)) for p in demangle(names)]      # as resource_usage.py
    print("\n".join(sorted(f"{p} | {rows[m]}" for m, p in zip(names, plain))))


if __name__ == "__main__":
    sys.exit(main())
