"""Dense-row blocks alone: hand-made cases and their fp64 reference, for tests/test_fp_block_ref_host.py (which proves on the CPU
what the GPU test rests on) and tests/test_gpu_fp_blocks.py (which runs csrc/fp.hip and csrc/interp_index.hip on them through
hip_ops).  Not a test module; imports numpy, torch and the oracle's initial weights, never the library.

  * blocks: the six instantiations of csrc/fp.hip -- SA3 <32,3,64>, FP3 <64,32,64>, FP2 <64,16,34>, FP1 <34,8,34>, and the two
    blocks of the 3sa architecture, GSA <64,3,64> and FP4 <64,64,64> -- with the network's row strides (src 36 for FP1's 34
    channels, skip 12 for its 8 channels, 4 for a 3-channel position skip).
  * a case = one block at one shape (B, R_per_plot, S_per_plot) (`Spec`, `SPECS`): the smallest shapes at which each kernel form
    and each switch of the dispatch exists; `Spec.fwd` / `fwd_eval` / `bwd` are the forms (SN2_FP_FORM_*) the case is MEANT to take.
    Several specs share one set of arrays (`data_key`): they differ in what the caller hands over (dskip, gather, the index).
  * weights from oracle.network.init_state_dict (init_state_dict_3sa for GSA / FP4); every fifth gamma negative; W columns
    ZERO_COL (interpolated part) and ca + 1 (skip part) are zero, so those inputs' gradients are exactly zero; channel DEAD has a
    bias below -max(W u) - 1: relu gives 0 on every row, the batch variance is 0 and invstd = 1 / sqrt(eps).
  * no live pre-activation lies within MARGIN = 2^-15 of zero (rows that had one got 1/16 added to their first skip input), so
    fp32 rounding cannot flip a ReLU mask: the kernel's mask IS the reference's, and every gradient difference is rounding.
  * the 3-NN table is hand-made (per-plot indices, as sn2_three_nn's): blocks with one source per plot take idx (0,0,0) and
    w (w0,0,0); otherwise every row names three distinct sources with positive weights, and per plot are planted: source E(b) on
    no list; where a plot has at least 64 rows, source H(b) on 64 ... 126 rows (two chunks of the 63-entry chunk table; at 43 rows
    per plot no list can be that long, the rows being distinct sources); where it has more than 2048 rows, source L(b) on more than
    2048 (a second 2048-row slice of the index); every seventh row has weights (w,0,0), and its slot 1 names E(b) -- a slot
    with weight 0 behind slot 0 is on no list (csrc/interp_index.hip).
  * reference(): fp64 torch autograd of the header's statement (include/strata_hip.h, "dense-row block"); reference_fp32(): the
    same lines in fp32 on the CPU, the yardstick of fp32 rounding.  Both take the rows in blocks of ROW_BLOCK, so that a sum over
    262 146 rows is a sum of per-block sums whatever the BLAS library does with one long product.  bf16=True rounds the operands of the three contractions to
    bfloat16 (oracle.network._LinearBF16), what sn2_block.mma_bf16 does.
"""
import collections
import functools

import numpy as np
import torch

from oracle import network

F64 = torch.float64
EPS, MOMENTUM = 1e-5, 0.1
SPLIT, SOURCE_SIDE, DENSE = 0, 1, 2                  # SN2_FP_FORM_* (tests/test_fp_block_ref_host.py compares them with the library's)
STAT_ROWS = 65536                                    # SN2_STAT_SLOTS * 64: more rows leave the Split form in a training pass
ZERO_COL, DEAD = 5, 7
ZERO_WEIGHT_EVERY, ZERO_WEIGHT_AT = 7, 3             # rows r % 7 == 3 of a plot have weights (w,0,0)
ROW_BLOCK = 4096                                     # rows per product of the reference's linear layer (_run)
MARGIN = 2.0 ** -15                                 # no live pre-activation is closer to zero (make_case: _separate); fp32 rounding of
#                                                      a sum of at most 129 terms of magnitude <= 1 stays below 2^-18

Block = collections.namedtuple("Block", "ca cb cout knn src_stride skip_stride dskip key three_sa")
BLOCKS = {
    "SA3": Block(32, 3, 64, False, 32, 4, False, "sa3_module.nn", False),
    "FP3": Block(64, 32, 64, True, 64, 32, True, "fp3_module.nn", False),
    "FP2": Block(64, 16, 34, True, 64, 16, True, "fp2_module.nn", False),
    "FP1": Block(34, 8, 34, True, 36, 12, False, "fp1_module.nn", False),
    "GSA": Block(64, 3, 64, False, 64, 4, False, "sa4_module.nn", True),
    "FP4": Block(64, 64, 64, True, 64, 64, True, "fp4_module.nn", True),
}

# id; block; B, R_per_plot, S_per_plot; the forms of a training / frozen forward, an eval forward and the backward;
# source_side: hip_ops.SOURCE_SIDE during the calls; dskip: the backward is handed a dskip; gather: False = scatter_ready < 0;
# variant: "built" the backward call builds the index, "morton" prebuilt with src_pos, "perm" prebuilt with a row_perm
Spec = collections.namedtuple("Spec", "id block B Rp S fwd fwd_eval bwd source_side dskip gather bf16 variant")


def _spec(id, block, B, Rp, S, fwd, bwd, source_side=True, dskip=None, gather=True, bf16=False, variant="built"):
    fwd_eval = SOURCE_SIDE if fwd == SOURCE_SIDE else SPLIT              # an eval pass writes no statistic slots: Split at any size
    return Spec(id, block, B, Rp, S, fwd, fwd_eval, bwd, source_side, BLOCKS[block].dskip if dskip is None else dskip, gather, bf16, variant)


def _specs():
    S_, Q, D = SPLIT, SOURCE_SIDE, DENSE
    out = []
    for name, b in BLOCKS.items():                                        # tiny: 129 rows = two workgroups and one row
        S = 43 if not b.knn else 1 if name in ("FP3", "FP4") else 5
        out.append(_spec(f"tiny-{name}", name, 3, 43, S, S_, S_))
        out.append(_spec(f"tiny-{name}-bf16", name, 3, 43, S, S_, S_, bf16=True))
    out.append(_spec("seg-FP2", "FP2", 2, 2049, 40, S_, S_))
    out.append(_spec("edge65536-FP1", "FP1", 1, 65536, 64, S_, S_))
    out.append(_spec("edge65537-FP1", "FP1", 1, 65537, 64, Q, Q))
    out.append(_spec("edge65537-FP1-rows", "FP1", 1, 65537, 64, D, D, source_side=False))
    for name in ("SA3", "GSA"):
        out.append(_spec(f"dense-{name}", name, 3, 21846, 21846, D, D))
    for name in ("FP3", "FP4"):
        out.append(_spec(f"dense-{name}", name, 3, 21846, 1, D, D))
        out.append(_spec(f"dense-{name}-nogather", name, 3, 21846, 1, D, D, gather=False))
    out.append(_spec("densefp2-170", "FP2", 3, 21846, 170, Q, D))
    out.append(_spec("densefp2-171", "FP2", 3, 21846, 171, Q, D))
    out.append(_spec("densefp2-170-rows", "FP2", 3, 21846, 170, D, D, source_side=False))     # (FP2's forward in the Dense form)
    out.append(_spec("densefp1-FP1","FP1", 3, 21846, 170, D, D, source_side=False))
    out.append(_spec("densefp1-171", "FP1", 3, 21846, 171, D, D, source_side=False))          # (the short gather behind FP1's Dense form)
    for v in ("built", "morton", "perm"):
        out.append(_spec(f"src-FP1-{v}", "FP1", 3, 21846, 171, Q, Q, variant=v))
        out.append(_spec(f"src-FP2-{v}", "FP2", 3, 21846, 171, Q, Q, dskip=False, variant=v))
        out.append(_spec(f"tinyplots-FP1-{v}", "FP1", 72, 911, 8, Q, Q, variant=v))
    out.append(_spec("wide-FP1", "FP1", 2, 131073, 64, Q, Q))
    return collections.OrderedDict((s.id, s) for s in out)


SPECS = _specs()
MAX_ROWS, MAX_PLOTS = 262146, 72


def data_key(spec):
    return (spec.block, spec.B, spec.Rp, spec.S)


def forward_specs():
    """One spec per distinct forward call: the arrays, hip_ops.SOURCE_SIDE and the operand type decide it."""
    seen, out = set(), []
    for s in SPECS.values():
        k = data_key(s) + (s.source_side, s.bf16)
        if k not in seen:
            seen.add(k)
            out.append(s)
    return out


def specials(b, Rp, S):
    """(E, H, L) of plot b: the source on no list, on 64 ... 126 rows, on more than 2048 rows (-1: not planted at this shape)"""
    return (b + 1) % S, ((b + 3) % S if Rp >= 64 else -1), ((b + 4) % S if Rp > 2048 else -1)


def _table(g, B, Rp, S):
    """-> idx (B*Rp, 3) int32 per-plot source ids, w (B*Rp, 3) fp32"""
    R = B * Rp
    w = torch.rand(R, 3, generator=g) + 0.2
    if S == 1:
        w[:, 1:] = 0.0
        return torch.zeros(R, 3, dtype=torch.int32), w
    assert S >= 5
    idx = torch.zeros(B, Rp, 3, dtype=torch.int64)
    r = torch.arange(Rp)
    zero_w = r % ZERO_WEIGHT_EVERY == ZERO_WEIGHT_AT
    for b in range(B):
        E, H, L = specials(b, Rp, S)
        pool = torch.tensor([s for s in range(S) if s not in (E, H, L)])
        P = pool.numel()
        assert P >= 3
        i0 = torch.randint(0, P, (Rp,), generator=g)
        i1 = (i0 + 1 + torch.randint(0, P - 1, (Rp,), generator=g)) % P
        lo, hi = torch.minimum(i0, i1), torch.maximum(i0, i1)
        i2 = torch.randint(0, P - 2, (Rp,), generator=g)
        i2 = i2 + (i2 >= lo).long()
        i2 = i2 + (i2 >= hi).long()
        t = torch.stack([pool[i0], pool[i1], pool[i2]], 1)
        if H >= 0:
            rows = torch.randperm(Rp, generator=g)[:min(100, Rp)]
            t[rows, rows % 3] = H
        if L >= 0:
            rows = torch.randperm(Rp, generator=g)[:min(Rp, 2049 + Rp // 8)]
            t[rows, torch.where(zero_w[rows], 0, (rows + 1) % 3)] = L     # (slot 0 where only slot 0 counts; may replace H there)
        t[zero_w, 1] = E                                                   # weight 0: on no list
        idx[b] = t
    w = w.view(B, Rp, 3)
    w[:, zero_w, 1:] = 0.0
    return idx.view(R, 3).to(torch.int32), w.view(R, 3).contiguous()


def list_counts(idx, w, B, Rp, S):
    """(B, S): entries of every source's list as csrc/interp_index.hip counts them (slot 0 always, slots 1, 2 where the weight
    is not 0)"""
    on = torch.ones_like(idx, dtype=torch.bool)
    on[:, 1:] = w[:, 1:] != 0
    plot = torch.arange(B).repeat_interleave(Rp)[:, None].expand(-1, 3)
    flat = (plot * S + idx.long())[on]
    return torch.bincount(flat, minlength=B * S).view(B, S)


@functools.lru_cache(maxsize=None)
def _weights(name):
    b = BLOCKS[name]
    sd = network.init_state_dict_3sa(4) if b.three_sa else network.init_state_dict(4)
    return sd[b.key + ".0.0.weight"].clone(), sd[b.key + ".0.0.bias"].clone()


_DATA = {}


def make_case(spec):
    """-> namespace of CPU arrays, shared between tests and never written to: src (n_src, src_stride), skip (R, skip_stride),
    sa, sc (ca) or None, idx, w or None, W, b, gamma, beta, rm, rv, dy (R, h_stride), dsrc0 (n_src, src_stride), dskip0 (R, cb),
    src_pos (n_src, 4), row_perm (R) int32"""
    key = data_key(spec)
    if key in _DATA:
        return _DATA[key]
    name, B, Rp, S = key
    b = BLOCKS[name]
    assert B <= MAX_PLOTS and B * Rp <= MAX_ROWS
    g = torch.Generator().manual_seed(7919 * sorted(BLOCKS).index(name) + 31 * B + Rp + 1000003 * S)
    R, n_src = B * Rp, (B * S if b.knn else B * Rp)
    hs = (b.cout + 3) // 4 * 4
    c = type("Case", (), {})()
    c.name, c.block, c.B, c.Rp, c.S, c.R, c.n_src, c.hs = name, b, B, Rp, S, R, n_src, hs
    c.src = torch.randn(n_src, b.src_stride, generator=g)
    c.skip = torch.randn(R, b.skip_stride, generator=g)
    if b.knn:
        c.sa = (torch.rand(b.ca, generator=g) + 0.5) * torch.where(torch.arange(b.ca) % 3 == 1, -1.0, 1.0)
        c.sc = torch.randn(b.ca, generator=g) * 0.1
        c.idx, c.w = _table(g, B, Rp, S)
    else:
        c.sa = c.sc = c.idx = c.w = None
    W, bias = _weights(name)
    W, bias = W.clone(), bias.clone()
    W[:, ZERO_COL] = 0.0
    W[:, b.ca + 1] = 0.0
    c.W = W
    u = _separate(c, W, bias, with_bf16=R <= 4096)
    bias[DEAD] = -(float((u @ W[DEAD].double()).max()) + 1.0)
    c.b = bias
    c.gamma, c.beta = torch.rand(b.cout, generator=g) + 0.5, torch.randn(b.cout, generator=g) * 0.1
    c.gamma[::5] *= -1.0
    c.rm, c.rv = torch.linspace(0.1, 0.4, b.cout), torch.linspace(0.5, 1.5, b.cout)
    c.dy = torch.randn(R, hs, generator=g)                                  # (columns beyond cout: padding nobody may use)
    sign = lambda *s: torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0)          # noqa: E731
    c.dsrc0 = sign(n_src, b.src_stride) * torch.randint(1, 9, (n_src, b.src_stride), generator=g).float() / 4
    c.dskip0 = sign(R, b.cb) * torch.randint(1, 9, (R, b.cb), generator=g).float() / 4
    c.src_pos = torch.zeros(n_src, 4)
    c.src_pos[:, :3] = torch.rand(n_src, 3, generator=g) * 2.0 - 1.0
    c.row_perm = torch.stack([torch.randperm(Rp, generator=g) for _ in range(B)]).view(-1).to(torch.int32)
    _DATA[key] = c
    return c


def _bf16(x):
    return x.to(torch.bfloat16).to(x.dtype)


def _separate(c, W, bias, with_bf16):
    """Keep every pre-activation (the dead channel aside) at least MARGIN from zero, in fp64 and -- where the case also runs with
    bfloat16 operands -- with the operands rounded: a row that has one closer gets 1/16 added to its first skip input, until none
    is left.  A ReLU mask is a discontinuity: with 65 538 x 64 continuous pre-activations one sits within fp32 rounding of zero
    in most cases, the kernel and the reference fall on different sides, and one flipped mask moves that row's input gradient by
    a few per cent of the tensor's largest element (seen: dsrc 3.5e-2, db 3.5e-3 with every other figure at 1e-6).  -> u (fp64)"""
    b = c.block
    src = c.src[:, :b.ca].double()
    z = src if c.sa is None else c.sa.double() * src + c.sc.double()
    live = torch.arange(b.cout) != DEAD
    for _ in range(16):
        u = _inputs(c, z, F64)
        pre = u @ W.double().t() + bias.double()
        near = (pre[:, live].abs() < MARGIN).any(1)
        if with_bf16:
            pre = _bf16(u) @ _bf16(W.double()).t() + bias.double()
            near |= (pre[:, live].abs() < MARGIN).any(1)
        if not bool(near.any()):
            return u
        c.skip[near, 0] += 1.0 / 16
    raise AssertionError("pre-activations next to zero in every draw")


def _inputs(c, z, dtype):
    """u = [interp | skip] (R, ca + cb) from z = sa * src + sc (n_src, ca)"""
    b = c.block
    skip = c.skip[:, :b.cb].to(dtype)
    if not b.knn:
        return torch.cat([z, skip], 1)
    w = c.w.to(dtype)
    wn = w / w.sum(1, keepdim=True)
    src = (torch.arange(c.B).repeat_interleave(c.Rp) * c.S)[:, None] + c.idx.long()
    interp = (z[src] * wn[:, :, None]).sum(1)
    return torch.cat([interp, skip], 1)


def _run(c, mode, dtype, backward, bf16, z_in=None, skip_in=None, params=None):
    assert mode in ("train", "frozen", "eval")
    b = c.block
    p = {k: getattr(c, k).to(dtype).clone() for k in ("W", "b", "gamma", "beta")}
    if params is not None:
        p.update({k: v.to(dtype).clone() for k, v in params.items()})
    for v in p.values():
        v.requires_grad_(backward)
    src = c.src[:, :b.ca].to(dtype)
    z = (src if c.sa is None else c.sa.to(dtype) * src + c.sc.to(dtype)) if z_in is None else z_in.to(dtype)
    z = z.clone().requires_grad_(backward)
    skip = (c.skip[:, :b.cb] if skip_in is None else skip_in).to(dtype).clone().requires_grad_(backward)
    w = None
    if b.knn:
        w = c.w.to(dtype)
        wn = w / w.sum(1, keepdim=True)
        rows = (torch.arange(c.B).repeat_interleave(c.Rp) * c.S)[:, None] + c.idx.long()
        # (in blocks of rows for the same reason as the linear layer below: dsrc is then a sum of per-block partial sums, not
        # one chain of up to 21 846 fp32 additions per source)
        interp = torch.cat([(z[rows[i:i + ROW_BLOCK]] * wn[i:i + ROW_BLOCK, :, None]).sum(1) for i in range(0, c.R, ROW_BLOCK)])
    else:
        interp = z * 1.0
    if backward:
        interp.retain_grad()
    u = torch.cat([interp, skip], 1)
    if bf16:
        pre = network._LinearBF16.apply(u, p["W"], p["b"])
    else:
        # the rows in blocks of ROW_BLOCK: dW is then the sum of per-block products, as the kernels' is of per-workgroup ones.
        # One product over 262 146 rows left the fp32 restatement's dW at the mercy of the BLAS library's split of the row sum:
        # 2e-7 of fp64 with one thread count, 1.0e-5 with another.
        pre = torch.cat([u[i:i + ROW_BLOCK] @ p["W"].t() for i in range(0, c.R, ROW_BLOCK)]) + p["b"]
    h = torch.relu(pre)
    rm, rv = c.rm.to(dtype), c.rv.to(dtype)
    if mode == "train":
        mean, var = h.mean(0), h.var(0, unbiased=False)
        new_rm = ((1 - MOMENTUM) * rm + MOMENTUM * mean).detach()
        new_rv = ((1 - MOMENTUM) * rv + MOMENTUM * var * (c.R / (c.R - 1))).detach()
    else:
        mean, var, new_rm, new_rv = rm, rv, rm.clone(), rv.clone()
    invstd = 1.0 / torch.sqrt(var + EPS)
    out = p["gamma"] * (h - mean) * invstd + p["beta"]
    a = (p["gamma"] * invstd).detach()
    res = {"h": h.detach().numpy(), "out": out.detach().numpy(), "a": a.numpy(), "c": (p["beta"].detach() - mean.detach() * a).numpy(),
           "mean": mean.detach().numpy(), "invstd": invstd.detach().numpy(), "running_mean": new_rm.numpy(), "running_var": new_rv.numpy(),
           "batches": 1 if mode == "train" else 0}
    live = torch.arange(b.cout) != DEAD
    res["margin"], res["mask"] = float(pre.detach()[:, live].abs().min()), (pre.detach() > 0).numpy()
    res["loss"] = float((out.detach() * c.dy[:, :b.cout].to(dtype)).sum())
    if backward:
        (out * c.dy[:, :b.cout].to(dtype)).sum().backward()
        for n, k in (("dW", "W"), ("db", "b"), ("dgamma", "gamma"), ("dbeta", "beta")):
            res[n] = p[k].grad.numpy()
        res["dsrc"], res["dskip"], res["du"] = z.grad.numpy(), skip.grad.numpy(), interp.grad.numpy()
    return res


def reference(c, mode, backward=True, bf16=False, **kw):
    """fp64 autograd of the header's statement: u = [sa * interp + sc | skip] (the weights of a row sum to 1, so the affine is
    applied to the source rows), h = relu(W u + b), out = gamma (h - mean) invstd + beta with batch statistics ("train") or the
    running statistics ("frozen", "eval": constants), loss = sum(out * dy).  -> h, out, a, c, mean, invstd, running_mean,
    running_var, batches; with backward: dW, db, dgamma, dbeta, dsrc = d loss / d (sa * src + sc) per source row, dskip, du = the
    same per target row (what scatter_ready < 0 leaves in du_scratch).  Gradients WITHOUT any pre-fill."""
    return _run(c, mode, F64, backward and mode != "eval", bf16, **kw)


def reference_fp32(c, mode, backward=True, bf16=False):
    return _run(c, mode, torch.float32, backward and mode != "eval", bf16)


def unlisted_sources(c):
    """(n_src,) bool: source rows on no list (their dsrc must keep its bits)"""
    if not c.block.knn:
        return np.zeros(c.n_src, dtype=bool)
    return (list_counts(c.idx, c.w, c.B, c.Rp, c.S).view(-1) == 0).numpy()
