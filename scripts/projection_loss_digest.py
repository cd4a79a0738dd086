"""One `name sha256` line per output tensor of every entry point of csrc/project.hip's projection routes and csrc/loss.hip: two
commits that compute the same bits print the same listing (profiles/projection_rules/).  Run it in one fresh process per commit.

  cases          : every (name, family) of tests/_projection_loss_ref.case_ids() x every (m, e) of me_of(name)
  forward routes : plot_project_forward and plot_pixels (xy cases), plot_project_forward_pix, raster_project (xy cases) once per
                   case; projected_loss_forward, plot_losses, loss_forward per (m, e)
  backward       : plot_project_backward, loss_backward, projected_loss_backward, fed the reference's arg, nocc and fp32-rounded
                   pred as tests/test_gpu_projection_loss.py::test_backward_entries_alone feeds them
  fused route    : dy and the 32 weight-gradient images of sn2_head_backward with sn2_head.loss (and of the two-launch path beside
                   it), the inputs of tests/test_gpu_head_loss_backward.py::test_bits_small_shapes at (1, 64) and (2, 4160), fp32 rows
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _projection_loss_ref as R                                                     # noqa: E402
import test_gpu_head_loss_backward as H                                              # noqa: E402
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops                   # noqa: E402

DEV = "cuda:0"


def digest(name, t):
    torch.cuda.synchronize()
    print(name, hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest(), flush=True)


def digests(tag, names, tensors):
    for n, t in zip(names, tensors):
        digest(f"{tag} {n}", t)


def projection_loss_cases():
    for name, family in R.case_ids():
        c, r = R.case(name, family), R.ref(name, family)
        B, N, D = c.B, c.N, c.D
        d = {k: torch.tensor(getattr(c, k), device=DEV) for k in ("cov", "pix", "proba", "proba_zero", "pdf", "gt")}
        g = torch.tensor([R.G], dtype=torch.float64, device=DEV)
        tag = f"{name}-{family}"
        if c.cloud is not None:
            cloud = torch.tensor(c.cloud, device=DEV)
            digests(f"{tag} plot_project_forward", ("pred", "pix", "arg", "nocc"), ops.plot_project_forward(d["cov"], cloud, D))
            digests(f"{tag} plot_pixels", ("mm", "pix"), ops.plot_pixels(cloud, D))
            digests(f"{tag} raster_project", ("rasters", "pix"), ops.raster_project(d["cov"], cloud, D, c.diam_meters))
        pred, _, arg, nocc = ops.plot_project_forward_pix(d["cov"], d["pix"], B, N, D)
        digests(f"{tag} plot_project_forward_pix", ("pred", "arg", "nocc"), (pred, arg, nocc))
        arg_r, nocc_r = torch.tensor(r["arg"].reshape(-1), device=DEV), torch.tensor(r["nocc"], device=DEV)
        up = torch.tensor(np.random.default_rng(3).standard_normal((B, 4)).astype(np.float32), device=DEV)
        digest(f"{tag} plot_project_backward dcov", ops.plot_project_backward(up, arg_r, nocc_r, d["pix"], B, N, D))
        for m, e in R.me_of(name):
            q = d["proba"] if m != 0.0 else d["proba_zero"]
            tme = f"{tag} m={m} e={e}"
            digests(f"{tme} projected_loss_forward", ("out", "pred", "arg", "nocc"),
                    ops.projected_loss_forward(d["cov"], d["pix"], q, d["pdf"], d["gt"], B, N, D, m, e))
            digests(f"{tme} plot_losses", ("plots", "pred"), ops.plot_losses(d["cov"], d["pix"], q, d["pdf"], d["gt"], B, N, D, m, e))
            pred32 = torch.tensor(R.ref_backward(name, family, m, e)[0], device=DEV)
            digest(f"{tme} loss_forward out", ops.loss_forward(pred32, d["gt"], q, d["pdf"], m, e))
            digests(f"{tme} loss_backward", ("dpred", "dproba"), ops.loss_backward(pred32, d["gt"], q, d["pdf"], m, e, g))
            digests(f"{tme} projected_loss_backward", ("dcov", "dproba"),
                    ops.projected_loss_backward(pred32, d["gt"], q, d["pdf"], B, N, D, m, e, g, arg_r, nocc_r, d["pix"]))


def fused_head_backward_cases():
    for B, N in ((1, 64), (2, 4160)):
        for m, e in ((0.1, 0.04), (0.0, 0.04), (0.1, 0.0)):
            (dy_r, img_r), (dy_n, img_n), _ = H._both(H._inputs(B, N), m, e, torch.float32)
            digests(f"head_backward B={B} N={N} m={m} e={e}", ("two-launch dy", "two-launch images", "fused dy", "fused images"),
                    (dy_r, img_r, dy_n, img_n))


if __name__ == "__main__":
    projection_loss_cases()
    fused_head_backward_cases()
