"""One `name sha256` line per output tensor of the kernels that run the head's forward turn or FP1's row side: two commits that
compute the same bits print the same listing (profiles/head_turn/).  Run it in one fresh process per commit.

  head-forward cases : sn2_head_forward alone, the inputs of tests/test_gpu_head_forward.py (every R x row dtype x dropout)
  eval-forward cases : the model's eval forward (sn2_fp_head_eval) as in test_eval_fused_per_point_layer_and_head, the last
                       shape under both row forms (sn2_debug_fp_rows_form)
  FP1 training rows  : sn2_fp_forward's source-side form as in test_the_two_row_passes_of_the_source_side_forward_give_the_same_bits,
                       both row forms: h1, blk.aux and the running statistics
"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import network                                                           # noqa: E402
from stratanet2_vegetation_coverage_maps_amd import PointNet2, _lib                  # noqa: E402
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops                   # noqa: E402
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_batch  # noqa: E402

DEV = "cuda:0"


def digest(name, t):
    torch.cuda.synchronize()
    print(name, hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest(), flush=True)


def head_forward_cases():
    for R in (1, 63, 64, 65, 805):
        g = torch.Generator().manual_seed(3)
        f = torch.randn(R, 36, generator=g).to(DEV)
        fa = (0.5 + torch.rand(34, generator=g)).to(DEV)
        fc = (0.1 * torch.randn(34, generator=g)).to(DEV)
        torch.manual_seed(7)
        lin1, lin2 = torch.nn.Linear(34, 16).to(DEV), torch.nn.Linear(16, 5).to(DEV)
        mask = torch.randint(0, 1 << 16, (R,), generator=g, dtype=torch.int32).to(DEV)
        for dtype, dn in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            for drop in (False, True):
                cov, proba = torch.full((R, 4), 7.0, device=DEV), torch.full((R, 4), 7.0, device=DEV)
                ops.head_forward(ops.head_desc(f.to(dtype), fa, fc, lin1, lin2, cov, proba, drop_mask=mask if drop else None,
                                               drop_p=0.5 if drop else 0.0))
                tag = f"head_forward R={R} {dn} {'drop' if drop else 'nodrop'}"
                digest(tag + " cov", cov)
                digest(tag + " proba", proba)


def eval_forward_cases():
    for B, N, form in ((2, 4096, 1), (3, 24001, 1), (14, 10000, 1), (14, 10000, 0)):
        args = make_args(subsample_size=N, ratio1=0.03, r1=1.0, ratio2=0.25, r2=2.0)
        args.cuda = 0
        d = make_batch(B, N, first_plot=11)
        d["fps_start"] = torch.zeros(2, B, dtype=torch.long)
        m = PointNet2(args)
        m.load_state_dict(network.init_state_dict(7))
        m.train()
        with torch.no_grad():
            m(d)                                            # running statistics that are not (0, 1)
        m.eval()
        m.fuse_eval_head = True
        try:
            _lib.load().sn2_debug_fp_rows_form(form)
            with torch.no_grad():
                cov, proba = m(d)
            torch.cuda.synchronize()
        finally:
            _lib.load().sn2_debug_fp_rows_form(1)
        tag = f"eval_forward B={B} N={N} rows_form={form}"
        digest(tag + " cov", cov)
        digest(tag + " proba", proba)


def fp1_training_row_cases():
    dev = torch.device(DEV)
    for B, N, M1 in ((72, 1024, 8), (5, 14001, 3500)):
        torch.manual_seed(B * N)
        d = make_batch(B, N, first_plot=3)
        xyz = d["xyz"].to(dev).float().contiguous()
        _, pos1_soa, _ = ops.fps(xyz, M1, torch.zeros(B, dtype=torch.int32, device=dev))[:3]
        knn = ops.three_nn(pos1_soa, xyz, 3)
        h2 = torch.randn(B * M1, 36, device=dev)
        a2, c2 = torch.rand(34, device=dev) + 0.5, torch.randn(34, device=dev) * 0.1
        rows0 = torch.randn(B * N, 12, device=dev)
        try:
            for form in (1, 0):
                _lib.load().sn2_debug_fp_rows_form(form)
                lin, bn = torch.nn.Linear(42, 34).to(dev), torch.nn.BatchNorm1d(34).to(dev)
                with torch.no_grad():
                    g = torch.Generator(device="cpu").manual_seed(5)
                    lin.weight.copy_(torch.randn(34, 42, generator=g) * 0.2)
                    lin.bias.copy_(torch.randn(34, generator=g) * 0.1)
                blk = ops.BlockBuffers(lin, bn)
                h1 = torch.full((B * N, 36), 7.0, device=dev)
                desc = ops.fp_desc(blk, B, N, M1, 34, 8, h2, h1, src_affine=(a2, c2), knn=knn, skip=rows0[:, 0:8])
                assert ops.fp_form(desc, 1) == ops.FP_FORM_SOURCE_SIDE
                ops.fp_forward(desc, 1)
                tag = f"fp1_rows B={B} N={N} M1={M1} rows_form={form}"
                for name, t in (("h1", h1), ("aux", blk.aux), ("running_mean", bn.running_mean), ("running_var", bn.running_var)):
                    digest(f"{tag} {name}", t)
        finally:
            _lib.load().sn2_debug_fp_rows_form(1)


if __name__ == "__main__":
    head_forward_cases()
    eval_forward_cases()
    fp1_training_row_cases()
