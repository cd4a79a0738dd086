"""One `name sha256` line per output tensor of the set-abstraction message passes (csrc/sa_mfma.hip) run alone through hip_ops: two
commits that compute the same bits print the same listing (profiles/sa_turn/).  Run it in one fresh process per commit.

  forward cases  : SA1 (8, MLP[11,16,16]), SA2 (16, MLP[19,32]), the third level (32, MLP[35,64]) x fp32 / bf16 operands x
                   train / frozen / eval x order table / none, at two shapes: (a) 2 x 384 sources, 41 centroids, cap 160, with
                   lists of every item class (150 and 129: three SOLO steps; 65; QUADs of 64 ... 9; 8, 5, 4, 1, 0) and (b) 33
                   plots x 64 sources, 24 centroids, cap 32 (plot groups of 8 and a lone plot; one plot of 1s, one of 9s).
                   ext, arg, out, every block's aux rows and running statistics (train / frozen); out (eval).
  backward cases : one plot of 16 centroids (ONE workgroup: no float atomic of these results has a competitor), 192 sources, cap
                   160, after a FROZEN forward (1 / E := 0) and without a feature gradient; SA1 with and without the one-pass
                   workspace, SA2, the third level; fp32 / bf16; table / none.  dW, db of every block after grad_reduce, SA1's
                   dgamma0 / dbeta0 (the last block's dgamma / dbeta come from sa_bwd_prep_kernel and are not listed).
Inputs are continuous values from seeded generators.  `--per-case` folds the listing: one `case sha256` line per case (86), the
sha256 of the case's `name sha256` lines in the order above -- the form kept under profiles/sa_turn/.
"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stratanet2_vegetation_coverage_maps_amd import _lib                             # noqa: E402
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops                   # noqa: E402

DEV = "cuda:0"
KINDS = {"sa1": (8, (11, 16, 16)), "sa2": (16, (19, 32)), "sa3": (32, (35, 64))}
SHAPES = {"a": (2, 384, 41, 160), "b": (33, 64, 24, 32), "bwd": (1, 192, 16, 160)}          # B, Nsrc, M, cap
COUNTS_A = (150, 129, 65, 64, 40, 33, 20, 17, 12, 9, 8, 5, 4, 1, 0)
COUNTS_BWD = (150, 70, 40, 33, 20, 17, 8, 7, 6, 5, 4, 3, 2, 1, 0, 0)
TRAINING = {"train": True, "frozen": _lib.BN_FROZEN_KEEP, "eval": False}


PER_CASE = "--per-case" in sys.argv
LINES = []


def digest(name, t):
    torch.cuda.synchronize()
    LINES.append(f"{name} {hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()}")
    if not PER_CASE:
        print(LINES[-1], flush=True)


def fold(lines):
    """[`case tensor sha256`] -> [`case sha256 of the case's lines`], cases in their order of appearance"""
    cases = {}
    for l in lines:
        cases.setdefault(l.rsplit(" ", 2)[0], []).append(l)
    return [f"{c} {hashlib.sha256(''.join(x + chr(10) for x in ls).encode()).hexdigest()}" for c, ls in cases.items()]


def counts(shape, g):
    B, _, M, _ = SHAPES[shape]
    rows = []
    for b in range(B):
        if shape == "bwd":
            rows.append(list(COUNTS_BWD))
            continue
        if shape == "a":
            c = list(COUNTS_A) + torch.randint(0, 13, (M - len(COUNTS_A),), generator=g).tolist()
        else:
            c = [1] * M if b == 5 else [9] * M if b == 6 else torch.randint(0, 21, (M,), generator=g).tolist()
        perm = torch.randperm(M, generator=g).tolist()
        rows.append([c[perm[i]] for i in range(M)])
    return torch.tensor(rows, dtype=torch.int32).reshape(-1)


class Module:
    def __init__(self, kind, shape, with_order, bf16):
        cf, mlp = KINDS[kind]
        B, Nsrc, M, cap = SHAPES[shape]
        self.B, self.Nsrc, self.M, self.cf, self.cl = B, Nsrc, M, cf, mlp[-1]
        g = torch.Generator().manual_seed(100 * sorted(KINDS).index(kind) + sorted(SHAPES).index(shape) + 11)
        rows = torch.zeros(B * Nsrc, cf + 4)
        rows[:, :cf] = torch.randn(B * Nsrc, cf, generator=g)
        rows[:, cf:cf + 3] = torch.rand(B * Nsrc, 3, generator=g) * 2.0
        cpos = torch.zeros(B * M, 4)
        cpos[:, :3] = torch.rand(B * M, 3, generator=g) * 2.0
        cnt = counts(shape, g)
        nbr = torch.zeros(B * M, cap, dtype=torch.int32)
        for i, n in enumerate(cnt.tolist()):
            nbr[i, :n] = torch.randperm(Nsrc, generator=g)[:n].sort().values.int()
        self.blocks = []
        for k in range(len(mlp) - 1):
            ci, co = mlp[k], mlp[k + 1]
            lin, bn = torch.nn.Linear(ci, co).to(DEV), torch.nn.BatchNorm1d(co).to(DEV)
            gamma = torch.rand(co, generator=g) + 0.5
            if k == len(mlp) - 2:
                gamma[::3] *= -1.0
            with torch.no_grad():
                lin.weight.copy_(torch.randn(co, ci, generator=g) * (0.4 if k == 0 else 0.3))
                lin.bias.copy_(torch.randn(co, generator=g) * 0.1)
                bn.weight.copy_(gamma), bn.bias.copy_(torch.randn(co, generator=g) * 0.1)
                bn.running_mean.copy_(torch.linspace(0.1, 0.4, co)), bn.running_var.copy_(torch.linspace(0.5, 1.5, co))
            blk = ops.BlockBuffers(lin, bn)
            blk.aux.zero_()
            blk.mma_bf16 = bf16
            self.blocks.append(blk)
        self.dout = torch.randn(B * M, self.cl, generator=g).to(DEV)
        self.rows, self.cpos, self.nbr, self.cnt = rows.to(DEV), cpos.to(DEV), nbr.to(DEV), cnt.to(DEV)
        self.total = cnt.sum().to(torch.int64).reshape(1).to(DEV)
        self.order = ops.sa_order(self.cnt, B, M) if with_order else None
        self.ext = torch.full((B * M, self.cl), -777.25, device=DEV)
        self.arg = torch.full((B * M, self.cl), -7777, dtype=torch.int32, device=DEV)
        self.out = torch.full((B * M, self.cl), 555.5, device=DEV)

    def desc(self, **kw):
        return ops.sa_desc(self.blocks, self.rows[:, 0:self.cf], self.cf, self.rows[:, self.cf:self.cf + 4], self.cpos, self.nbr,
                           self.cnt, self.total, self.B, self.Nsrc, self.M, self.ext, self.arg, self.out, order=self.order, **kw)

    def forward(self, mode):
        for blk in self.blocks:
            blk.frozen = mode == "frozen"
        ops.sa_forward(self.desc(), TRAINING[mode])
        torch.cuda.synchronize()

    def backward(self, one_pass):
        """-> [(name, gradient)] of every block: dW, db, dgamma, dbeta, after grad_reduce"""
        shapes = [s for b in self.blocks for s in ((b.cout, b.lin.in_features), (b.cout,), (b.cout,), (b.cout,))]
        n_flat = sum(int(torch.Size(s).numel()) for s in shapes)
        arena, flat, images, extra = ops.grad_images_alloc(n_flat, DEV, ops.SA_BWD_WS_WORDS)
        views, o = [], 0
        for s in shapes:
            n = int(torch.Size(s).numel())
            views.append(flat[o:o + n].view(s))
            o += n
        for k, blk in enumerate(self.blocks):
            blk.grads, blk.grad_images = tuple(views[4 * k:4 * k + 4]), images
        ops.sa_backward(self.desc(dout=self.dout, dfeat=None, with_grads=True, bwd_ws=extra if one_pass else None))
        ops.grad_reduce(arena, n_flat, images)
        torch.cuda.synchronize()
        names = [f"{n}{k}" for k in range(len(self.blocks)) for n in ("dW", "db", "dgamma", "dbeta")]
        return list(zip(names, views))


def forward_cases():
    for kind in KINDS:
        for shape in ("a", "b"):
            for bf16 in (False, True):
                for with_order in (True, False):
                    for mode in ("train", "frozen", "eval"):
                        m = Module(kind, shape, with_order, bf16)
                        m.forward(mode)
                        tag = f"fwd {kind} {shape} {'bf16' if bf16 else 'fp32'} {'order' if with_order else 'noorder'} {mode}"
                        digest(tag + " out", m.out)
                        if mode == "eval":
                            continue
                        digest(tag + " ext", m.ext)
                        digest(tag + " arg", m.arg)
                        for k, blk in enumerate(m.blocks):
                            digest(f"{tag} aux{k}", blk.aux)
                            digest(f"{tag} running_mean{k}", blk.bn.running_mean)
                            digest(f"{tag} running_var{k}", blk.bn.running_var)


def backward_cases():
    for kind in KINDS:
        for one_pass in ((False, True) if kind == "sa1" else (False,)):
            for bf16 in (False, True):
                if one_pass and bf16:
                    continue                                                    # (the one-pass route is fp32 operands only)
                for with_order in (True, False):
                    m = Module(kind, "bwd", with_order, bf16)
                    m.forward("frozen")
                    tag = (f"bwd {kind} {'one-pass' if one_pass else 'two-pass'} {'bf16' if bf16 else 'fp32'} "
                           f"{'order' if with_order else 'noorder'}")
                    last = len(m.blocks) - 1
                    for name, t in m.backward(one_pass):
                        if name in (f"dgamma{last}", f"dbeta{last}"):
                            continue
                        digest(f"{tag} {name}", t)


if __name__ == "__main__":
    forward_cases()
    backward_cases()
    if PER_CASE:
        print("\n".join(fold(LINES)), flush=True)
