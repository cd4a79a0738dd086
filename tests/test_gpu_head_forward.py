"""sn2_head_forward alone (head_fwd_mfma_kernel: lin1 -> ReLU -> dropout -> lin2 -> softmax x sigmoid on a wave's 64-row LDS
tile) against the same head in torch float64 on the CPU: one row, a tile short by one, exactly one tile, one row into a second
tile, and a wave that loops with a ragged end; rows stored as fp32 and as bfloat16; with and without dropout words.
Tolerance: 2e-6 absolute -- the project's figure for two fp32 evaluations of this head that differ by re-association
(test_eval_fused_per_point_layer_and_head); a plain fp32 torch evaluation of these inputs at R = 805 stays within 3e-7 of
float64 for both outputs."""
import functools
from types import SimpleNamespace

import pytest
import torch

from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DROP_P = 0.5
ROWS = [1, 63, 64, 65, 805]
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


@functools.lru_cache(maxsize=None)
def inputs(R):
    """Random rows, weights and dropout words as tests/test_gpu_head_loss_backward.py::_inputs makes them, R given directly
    (made once per R on the CPU, never written)."""
    g = torch.Generator().manual_seed(3)
    f = torch.randn(R, 36, generator=g)
    fa = 0.5 + torch.rand(34, generator=g)
    fc = 0.1 * torch.randn(34, generator=g)
    torch.manual_seed(7)
    lin1, lin2 = torch.nn.Linear(34, 16), torch.nn.Linear(16, 5)
    mask = torch.randint(0, 1 << 16, (R,), generator=g, dtype=torch.int32)
    return SimpleNamespace(R=R, f=f, fa=fa, fc=fc, lin1=lin1, lin2=lin2, mask=mask)


@functools.lru_cache(maxsize=None)
def reference(R, dtype, drop):
    """The head in float64 on the CPU, from the rows as they are stored -> (cov, proba)"""
    x = inputs(R)
    with torch.no_grad():
        f = x.f.to(dtype).double()
        y = x.fa.double() * f[:, :34] + x.fc.double()
        z = torch.relu(y @ x.lin1.weight.double().T + x.lin1.bias.double())
        if drop:
            keep = (x.mask[:, None] >> torch.arange(16, dtype=torch.int32)[None, :]) & 1
            z = torch.where(keep.bool(), z / (1.0 - DROP_P), torch.zeros_like(z))
        s = z @ x.lin2.weight.double().T + x.lin2.bias.double()
        proba = torch.softmax(s[:, :4], 1)
        return proba * torch.sigmoid(s[:, 4:5]), proba


def run(R, dtype, drop):
    """One sn2_head_forward into outputs pre-filled with 7.0 -> (cov, proba) on the CPU"""
    x = inputs(R)
    f = x.f.to(DEV).to(dtype)
    lin1, lin2 = torch.nn.Linear(34, 16).to(DEV), torch.nn.Linear(16, 5).to(DEV)
    lin1.load_state_dict(x.lin1.state_dict())
    lin2.load_state_dict(x.lin2.state_dict())
    cov, proba = torch.full((R, 4), 7.0, device=DEV), torch.full((R, 4), 7.0, device=DEV)
    mask = x.mask.to(DEV) if drop else None
    ops.head_forward(ops.head_desc(f, x.fa.to(DEV), x.fc.to(DEV), lin1, lin2, cov, proba, drop_mask=mask, drop_p=DROP_P if drop else 0.0))
    torch.cuda.synchronize()
    return cov.cpu(), proba.cpu()


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize("R", ROWS)
def test_head_forward_matches_float64(R, dtype, drop):
    cov, proba = run(R, DTYPES[dtype], drop)
    cov_r, proba_r = reference(R, DTYPES[dtype], drop)
    for name, got, ref in (("cov", cov, cov_r), ("proba", proba, proba_r)):
        assert got.shape == (R, 4)
        assert not bool((got == 7.0).any()), f"{name}: rows left unwritten"
        err = float((got.double() - ref).abs().max())
        print(f"R {R} {dtype} drop {drop} {name}: max |d| {err:.3e}")
        torch.testing.assert_close(got.double(), ref, atol=2e-6, rtol=0)
