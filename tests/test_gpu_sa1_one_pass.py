"""SA1's backward in one message pass (csrc/sa_mfma.hip "ONE-PASS ROUTE", csrc/sa.hip: sa_bwd_combine_kernel): with a workspace
(`sn2_sa.bwd_ws`) and no feature gradient wanted, pass C also takes the three sums the first block's weight gradient is linear
in, and a one-workgroup kernel finishes it -- against today's two passes (no workspace) and against fp64 autograd on the CPU.

The module alone, through hip_ops, on a hand-made neighbour table: B = 2 plots (their items interleave), 384 sources, M = 40
centroids (no multiple of 16), cap = 160; the neighbour counts hold 0, 1, 4, 5, 8, 9, 64, 65 and 150 -- both sides of
SN2_SA_OCT_MIN / QUAD_MIN / SOLO_MIN, an empty centroid and a SOLO item of three steps -- the rest are <= 12.  One block-0 bias
makes its channel active for every message, one for none (that gradient row must be exactly 0).

Tolerances: two routes of the same sums differ by the order of float atomics, 1e-5 of a tensor's magnitude (the allowance of
tests/test_gpu_network.py for weight gradients); against fp64 the one-pass dW0 / db0 may be worse than the two-pass one by at most
that, and stays under the project's gradient bound of 1e-3.  bf16 operands keep the two passes (a workspace is then left alone)."""
import numpy as np
import pytest
import torch

from stratanet2_vegetation_coverage_maps_amd import _lib, hip_ops as ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, NSRC, M, CAP, CF, C1, C2 = 2, 384, 40, 160, 8, 16, 16
CIN = CF + 3
ALWAYS, NEVER = 3, 7
ATOM, BOUND = 1e-5, 1e-3
BF16_GRAD = 2e-2            # tests/test_gpu_bf16.py: gradients with bfloat16 operands
NAMES = ("dW0", "db0", "dgamma0", "dbeta0", "dW1", "db1", "dgamma1", "dbeta1")
SHAPES = ((C1, CIN), (C1,), (C1,), (C1,), (C2, C1), (C2,), (C2,), (C2,))
N_FLAT = sum(int(np.prod(s)) for s in SHAPES)


def _inputs():
    g = torch.Generator().manual_seed(6)
    rows0 = torch.zeros(B * NSRC, 12)
    rows0[:, 0:8] = torch.randn(B * NSRC, 8, generator=g)
    rows0[:, 8:11] = torch.rand(B * NSRC, 3, generator=g) * 2.0
    cpos = torch.zeros(B * M, 4)
    cpos[:, 0:3] = torch.rand(B * M, 3, generator=g) * 2.0
    special = [0, 1, 4, 5, 8, 9, 64, 65, 150]
    cnt = torch.zeros(B * M, dtype=torch.int32)
    nbr = torch.zeros(B * M, CAP, dtype=torch.int32)
    for b in range(B):
        counts = special + torch.randint(0, 13, (M - len(special),), generator=g).tolist()
        perm = torch.randperm(M, generator=g).tolist()
        for i, n in zip(perm, counts):
            cnt[b * M + i] = n
            nbr[b * M + i, :n] = torch.randperm(NSRC, generator=g)[:n].sort().values.int()     # ascending, distinct
    p = {"W0": torch.randn(C1, CIN, generator=g) * 0.4, "b0": torch.randn(C1, generator=g) * 0.2,
         "gamma0": torch.rand(C1, generator=g) + 0.5, "beta0": torch.randn(C1, generator=g) * 0.1,
         "W1": torch.randn(C2, C1, generator=g) * 0.3, "b1": torch.randn(C2, generator=g) * 0.1,
         "gamma1": torch.rand(C2, generator=g) + 0.5, "beta1": torch.randn(C2, generator=g) * 0.1}
    p["gamma1"][::3] *= -1.0
    p["b0"][ALWAYS], p["b0"][NEVER] = 9.0, -9.0        # (7 sigma of the pre-activation: checked in _reference)
    dout = torch.randn(B * M, C2, generator=g)
    return rows0, cpos, nbr, cnt, p, dout


def _reference(rows0, cpos, nbr, cnt, p, dout):
    """fp64 autograd over the explicit message tensor (training-mode BatchNorm, first maximum wins)."""
    f64 = torch.float64
    cen, src = [], []
    for i in range(B * M):
        n = int(cnt[i])
        cen += [i] * n
        src += ((i // M) * NSRC + nbr[i, :n].long()).tolist()
    cen, src = torch.tensor(cen), torch.tensor(src)
    r = rows0.to(f64)
    x = torch.cat([r[src, 0:8], r[src, 8:11] - cpos.to(f64)[cen, 0:3]], 1)
    q = {k: v.to(f64).clone().requires_grad_(True) for k, v in p.items()}

    def bn(h, gamma, beta):
        return gamma * (h - h.mean(0)) / torch.sqrt(h.var(0, unbiased=False) + 1e-5) + beta

    h = torch.relu(x @ q["W0"].t() + q["b0"])
    assert bool((h[:, ALWAYS] > 0).all()) and bool((h[:, NEVER] == 0).all())
    y2 = bn(torch.relu(bn(h, q["gamma0"], q["beta0"]) @ q["W1"].t() + q["b1"]), q["gamma1"], q["beta1"])
    out = torch.zeros(B * M, C2, dtype=f64)
    for i in range(B * M):
        idx = (cen == i).nonzero()[:, 0]
        if idx.numel():
            out[i] = y2[idx[y2[idx].argmax(0)], torch.arange(C2)]
    (out * dout.to(f64)).sum().backward()
    g = {"dW0": q["W0"].grad, "db0": q["b0"].grad, "dgamma0": q["gamma0"].grad, "dbeta0": q["beta0"].grad,
         "dW1": q["W1"].grad, "db1": q["b1"].grad, "dgamma1": q["gamma1"].grad, "dbeta1": q["beta1"].grad}
    return {k: v.numpy() for k, v in g.items()}, out.detach().numpy()


class _Module:
    """The two blocks on the device, the tables, and a backward into a fresh zero-filled arena per call."""

    def __init__(self, inputs, with_order, bf16=False):
        rows0, cpos, nbr, cnt, p, dout = inputs
        self.rows0, self.cpos, self.nbr, self.cnt = rows0.to(DEV), cpos.to(DEV), nbr.to(DEV), cnt.to(DEV)
        self.total = cnt.sum().to(torch.int64).reshape(1).to(DEV)
        self.dout = dout.to(DEV)
        self.order = ops.sa_order(self.cnt, B, M) if with_order else None
        self.blocks = []
        for k, (ci, co) in enumerate(((CIN, C1), (C1, C2))):
            lin, bn = torch.nn.Linear(ci, co).to(DEV), torch.nn.BatchNorm1d(co).to(DEV)
            with torch.no_grad():
                lin.weight.copy_(p[f"W{k}"]), lin.bias.copy_(p[f"b{k}"]), bn.weight.copy_(p[f"gamma{k}"]), bn.bias.copy_(p[f"beta{k}"])
                bn.running_mean.copy_(torch.linspace(0.1, 0.4, co)), bn.running_var.copy_(torch.linspace(0.5, 1.5, co))
            blk = ops.BlockBuffers(lin, bn)
            blk.mma_bf16 = bf16
            self.blocks.append(blk)
        self.ext = torch.empty(B * M, C2, device=DEV)
        self.arg = torch.empty(B * M, C2, dtype=torch.int32, device=DEV)
        self.out = torch.empty(B * M, C2, device=DEV)

    def desc(self, **kw):
        return ops.sa_desc(self.blocks, self.rows0[:, 0:8], CF, self.rows0[:, 8:12], self.cpos, self.nbr, self.cnt, self.total,
                           B, NSRC, M, self.ext, self.arg, self.out, order=self.order, **kw)

    def forward(self, frozen=False):
        for blk in self.blocks:
            blk.frozen = frozen
        ops.sa_forward(self.desc(), _lib.BN_FROZEN_KEEP if frozen else True)

    def arena(self):
        return ops.grad_images_alloc(N_FLAT, DEV, ops.SA_BWD_WS_WORDS)          # zero-filled, the workspace behind the images

    def backward(self, one_pass, arena=None):
        """-> ({name: gradient (numpy)}, the workspace as the backward left it)"""
        arena, flat, images, extra = self.arena() if arena is None else arena
        views, o = [], 0
        for s in SHAPES:
            n = int(np.prod(s))
            views.append(flat[o:o + n].view(s))
            o += n
        for k, blk in enumerate(self.blocks):
            blk.grads, blk.grad_images = tuple(views[4 * k:4 * k + 4]), images
        ops.sa_backward(self.desc(dout=self.dout, dfeat=None, with_grads=True, bwd_ws=extra if one_pass else None))
        ops.grad_reduce(arena, N_FLAT, images)
        torch.cuda.synchronize()
        return {n: v.detach().cpu().numpy().copy() for n, v in zip(NAMES, views)}, extra.cpu().numpy().copy()


def _rel(a, b, scale):
    return float(np.abs(a - b).max()) / scale


_CACHE = {}


def _shared():
    if not _CACHE:
        inputs = _inputs()
        ref, out = _reference(*inputs)
        _CACHE.update(inputs=inputs, ref=ref, out=out)
    return _CACHE["inputs"], _CACHE["ref"], _CACHE["out"]


@pytest.mark.parametrize("with_order", [True, False])
def test_one_pass_against_two_passes_and_fp64(with_order):
    inputs, ref, out_ref = _shared()
    m = _Module(inputs, with_order)
    m.forward()
    one, ws = m.backward(True)
    two, ws_two = m.backward(False)
    again, _ = m.backward(True)                        # a fresh arena right after: nothing is left over between calls
    assert _rel(m.out.cpu().numpy(), out_ref, np.abs(out_ref).max()) < 1e-4
    assert np.abs(ws).max() > 0 and not ws_two.any()   # the route was taken / not taken
    for n in NAMES[2:]:
        scale = np.abs(ref[n]).max()
        e = _rel(one[n], two[n], np.abs(two[n]).max())
        print(f"{n}: one-pass vs two-pass {e:.2e}; vs fp64 {_rel(one[n], ref[n], scale):.2e} / {_rel(two[n], ref[n], scale):.2e}")
        assert e <= ATOM, n
        assert _rel(one[n], ref[n], scale) < BOUND, n
    for n in NAMES[:2]:
        scale = np.abs(ref[n]).max()
        e1, e2 = _rel(one[n], ref[n], scale), _rel(two[n], ref[n], scale)
        print(f"{n}: error against fp64: one-pass {e1:.2e}, two-pass {e2:.2e}; second one-pass call differs by "
              f"{_rel(again[n], one[n], scale):.2e}")
        assert e1 <= e2 + ATOM, n
        assert e1 < BOUND, n
        assert _rel(again[n], one[n], scale) <= ATOM, n
    assert not one["dW0"][NEVER].any() and one["db0"][NEVER] == 0          # never active: exactly zero
    assert np.abs(one["dW0"][ALWAYS]).max() > 0
    assert not ref["dW0"][NEVER].any()


def test_frozen_statistics_need_no_combine():
    """Forward on the running statistics (SN2_BN_FROZEN_KEEP): 1 / E := 0, the scaled S_g alone is the gradient -- S_x, S_m are
    not written (the workspace stays zero) and no combine kernel runs."""
    inputs, _, _ = _shared()
    m = _Module(inputs, True)
    m.forward(frozen=True)
    one, ws = m.backward(True)
    two, _ = m.backward(False)
    assert not ws.any()
    for n in NAMES:
        scale = np.abs(two[n]).max()
        e = _rel(one[n], two[n], scale if scale > 0 else 1.0)
        print(f"frozen {n}: one-pass vs two-pass {e:.2e}")
        assert e <= ATOM, n
    assert np.abs(one["dW0"]).max() > 0 and not one["dW0"][NEVER].any()


def test_bf16_operands_keep_the_two_passes():
    """bf16 operands: a workspace changes nothing -- it is left untouched (all zero), which is what shows that pass D ran, and
    the gradients are those of a call without one.  Two calls of that SAME two-pass code do not agree to the fp32 allowance:
    the order of the atomics moves dgamma0 / dbeta0 in the last bits, pass D's dp1 with them, and an element next to a
    rounding boundary then lands on the other bfloat16 value (2^-8 of itself).  So the comparison uses the bound
    tests/test_gpu_bf16.py states for bf16 gradients, 2e-2 of the tensor's magnitude."""
    inputs, _, _ = _shared()
    m = _Module(inputs, True, bf16=True)
    m.forward()
    with_ws, ws = m.backward(True)
    without, _ = m.backward(False)
    assert not ws.any()                                # the workspace was left alone
    for n in NAMES:
        e = _rel(with_ws[n], without[n], np.abs(without[n]).max())
        print(f"bf16 {n}: with a workspace vs without {e:.2e}")
        assert e <= BF16_GRAD, n


def test_captured_graph_replays_the_one_pass_route():
    inputs, _, _ = _shared()
    m = _Module(inputs, True)
    m.forward()
    eager, _ = m.backward(True)
    arena = m.arena()
    graph = torch.cuda.CUDAGraph()
    views = {}
    with ops.graph_capture(graph, DEV):
        arena[0].mul_(0.0)                             # (a kernel node: the arena is zero at the start of every replay)
        m.forward()
        for blk in m.blocks:
            blk.frozen = False
        flat, images, extra = arena[1], arena[2], arena[3]
        o = 0
        for n, s in zip(NAMES, SHAPES):
            k = int(np.prod(s))
            views[n] = flat[o:o + k].view(s)
            o += k
        for k, blk in enumerate(m.blocks):
            blk.grads, blk.grad_images = tuple(views[n] for n in NAMES[4 * k:4 * k + 4]), images
        ops.sa_backward(m.desc(dout=m.dout, dfeat=None, with_grads=True, bwd_ws=extra))
        ops.grad_reduce(arena[0], N_FLAT, images)
    for replay in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for n in NAMES:
            e = _rel(views[n].cpu().numpy(), eager[n], np.abs(eager[n]).max())
            print(f"replay {replay} {n}: vs eager {e:.2e}")
            assert e <= ATOM, (replay, n)
