"""The global level's forward and the pool kernels alone: hand-made cases and their fp64 references, for
tests/test_global_level_ref_host.py (which proves on the CPU what the GPU test rests on) and tests/test_gpu_global_level_forward.py
(which runs csrc/global_level.hip and the pool kernels of csrc/misc.hip on them through hip_ops).  Not a test module; imports
numpy, torch and the oracle's initial weights, never the library.

The level (include/strata_hip.h, "global level in ONE launch"): SA3 = relu(W3 [x2 | pos2] + b3) -> BatchNorm -> the plot's max of
a h + c (first row wins ties) -> FP3 = relu(Wf [x3 of the plot | x2] + bf) -> BatchNorm.

  * a case = one shape (B, M2) (`SHAPES`; `EXTRA` = 29 plots, the separate launches only).  Weights from
    oracle.network.init_state_dict(4); every fifth gamma negative; running statistics start from linspace values.
  * channel DEAD of each block has a bias below -max(W u) - 1: relu gives 0 on every row, the batch variance is 0, invstd =
    1 / sqrt(eps), and the plot's max is c on every row (a tie of the whole plot: row 0 wins).
  * channel OFFSET of each block has its bias raised until batch mean / batch std is about 8 (`OFFSET_RATIO`): where a variance
    formed as E[h^2] - E[h]^2 from fp32 sums loses digits first.
  * inputs: x2 (B*M2, 32) normal; pos2 (B*M2, 4) uniform in [-1, 1]^3 with a padding column nobody may use; per plot (`plants`):
    row p has its x2 scaled by SCALE so that it attains the signed extremum in several channels, row q > p is a bit-identical copy
    of it in x2 and pos2 (a planted exact tie: p must win), row `lone` (the plot's last row unless q is) is scaled by -SCALE (the
    extremum of other channels sits in the last, partial block / the tail of the max's row loop), row `origin` sits exactly at the
    origin (FP3's interpolation weight there is 1 / 1e-16).  `PAIRS` puts (p, q) into the same lane's row sequence, different row
    quarters of a 16-row tile, different 64-row blocks, different trips and -- on the memory path -- equal and different residues
    mod 16 (`position`).
  * no live pre-activation of either block lies within MARGIN = 2^-15 of zero, with batch statistics and with the running
    statistics (the idea of tests/_fp_block_ref.py: _separate; here a channel that has one gets 1/64 added to its bias, which
    moves no other channel and -- for FP3 -- leaves SA3 and hence x3 alone).  fp32 rounding of a sum of at most 97 terms cannot
    reach that far, so the set of exactly-zero activations is the same in fp32 and fp64, and a negative-gamma channel's max over
    its exact zeros is c to the bit.
  * reference(case, mode) / reference_fp32: the statement above in fp64 / in fp32 on the CPU, modes "train", "frozen", "eval"
    (the last two: the running statistics as constants, nothing updated).
  * decisions(case, ref): per (plot, channel) the first maximum, its gap to the best row that is not a bit-identical copy, and
    whether that decides the row: exactly (the extremum is an exact zero of h: the lowest zero row) or by more than the decision
    bound 2 * OUT_TOL * max |a h + c| -- two rows whose values the output tolerance cannot tell apart may swap.
  * max_case / pool_backward_case: the pool kernels' cases (exact arithmetic on a lattice; fp64 sums of the header's formulas).
"""
import functools

import numpy as np
import torch

from oracle import network

F64 = torch.float64
EPS, MOMENTUM = 1e-5, 0.1
DEAD, OFFSET = 7, 11
OFFSET_RATIO = 8.0
MARGIN = 2.0 ** -15
OUT_TOL = 1e-4                                         # tests/test_gpu_fp_blocks.py: OUT_TOL
SCALE = 5.0
SHAPES = [(1, 40), (3, 64), (2, 65), (2, 256), (2, 257), (1, 625), (28, 64)]
EXTRA = (29, 40)
PAIRS = {
    (1, 40): [(1, 17)],                                # one lane: tiles 0 and 1 of its row sequence
    (3, 64): [(1, 2), (1, 5), (6, 54)],                # one lane, one tile | row quarters 0 and 1 | one lane, tiles 0 and 3
    (2, 65): [(3, 64), (9, 13)],                       # blocks 0 and 1 (the one-row block) | row quarters 2 and 3
    (2, 256): [(3, 70), (100, 200)],                   # blocks 0 and 1 | blocks 1 and 3
    (2, 257): [(5, 256), (16, 32)],                    # trips 0 and 1, residues 5 and 0 | one residue: one thread's row sequence
    (1, 625): [(100, 600)],                            # trips 0 and 2, residues 4 and 8
    (28, 64): [(1, 2), (1, 5), (1, 17), (0, 63), (20, 40), (7, 8)],
    (29, 40): [(1, 2), (1, 5), (1, 17), (0, 39)],
}
BLOCKS = (("sa3", "sa3_module.nn.0", 35), ("fp3", "fp3_module.nn.0", 96))
STATS = ("a", "c", "mean", "invstd")


def position(p, q, M2):
    """Where the pair sits in global_level_fwd_kernel: a set of "lane" (one lane's row sequence: V3[t][j] of one thread),
    "quarter" (different row quarters of one 16-row tile), "block" (different 64-row blocks of one trip), "trip", and on the
    memory path of the max (M2 > 256: thread = (row mod 16, channel)) "residue-same" / "residue-differs"."""
    out = set()
    if p // 256 != q // 256:
        out.add("trip")
    elif p // 64 != q // 64:
        out.add("block")
    elif (p % 16) // 4 != (q % 16) // 4:
        if p // 16 == q // 16:
            out.add("quarter")
    else:
        out.add("lane")
    if M2 > 256:
        out.add("residue-same" if p % 16 == q % 16 else "residue-differs")
    return out


def plants(B, M2):
    """-> per plot (p, q, lone or None, origin): rows of the plot"""
    pairs = PAIRS[(B, M2)]
    out = []
    for b in range(B):
        p, q = pairs[b % len(pairs)]
        assert 0 <= p < q < M2
        lone = M2 - 1 if q != M2 - 1 else None
        origin = next(r for r in range(3 + b % 5, M2) if r not in (p, q, lone))
        out.append((p, q, lone, origin))
    return out


def _offset_bias(wu):
    """the bias at which mean / std of relu(wu + bias) is OFFSET_RATIO (bisection: the ratio grows with the bias)"""
    lo, hi = float(-wu.mean()), float(wu.abs().max() + 100.0 * wu.std())
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        h = torch.relu(wu + mid)
        if float(h.mean() / h.std(unbiased=False)) < OFFSET_RATIO:
            lo = mid
        else:
            hi = mid
    return hi


def _clear_margin(pres, bias):
    """pres: pre-activations WITHOUT bias (fp64, one array per statistics mode); adds 1/64 to the (fp32) bias of a live channel
    until none of its pre-activations lies within MARGIN of zero"""
    for o in range(64):
        if o == DEAD:
            continue
        for _ in range(64):
            if not any(bool(((pre[:, o] + bias[o].double()).abs() < MARGIN).any()) for pre in pres):
                break
            bias[o] += 1.0 / 64
        else:
            raise AssertionError("pre-activations next to zero at every bias")


def _stats(h, rm, rv, mode, R):
    """-> mean, var, new running mean, new running var"""
    if mode == "train":
        mean, var = h.mean(0), h.var(0, unbiased=False)
        return mean, var, (1 - MOMENTUM) * rm + MOMENTUM * mean, (1 - MOMENTUM) * rv + MOMENTUM * var * (R / (R - 1))
    return rm, rv, rm.clone(), rv.clone()


def _pool(y, B, M2):
    """the plot's max of y (B*M2, 64) and the FIRST row attaining it (numpy's argmax returns the first occurrence)"""
    v = y.numpy().reshape(B, M2, 64)
    arg = np.argmax(v, axis=1)
    return torch.from_numpy(np.take_along_axis(v, arg[:, None, :], 1)[:, 0, :].copy()), arg.astype(np.int32)


_CASES = {}


def make_case(B, M2):
    """-> namespace of CPU arrays, shared between tests and never written to: x2 (R, 32), pos2 (R, 4), per block W, b, gamma, beta,
    rm, rv (`c.blk[name]`), plants (per plot p, q, lone, origin)"""
    if (B, M2) in _CASES:
        return _CASES[(B, M2)]
    g = torch.Generator().manual_seed(100 * B + M2)
    R = B * M2
    sd = network.init_state_dict(4)
    c = type("Case", (), {})()
    c.B, c.M2, c.R = B, M2, R
    c.blk = {}
    for name, key, cin in BLOCKS:
        c.blk[name] = dict(W=sd[key + ".0.weight"].clone(), b=sd[key + ".0.bias"].clone(), gamma=torch.rand(64, generator=g) + 0.5,
                           beta=torch.randn(64, generator=g) * 0.1, rm=torch.linspace(0.1, 0.4, 64), rv=torch.linspace(0.5, 1.5, 64))
        c.blk[name]["gamma"][::5] *= -1.0
        assert c.blk[name]["W"].shape == (64, cin)
    c.x2 = torch.randn(R, 32, generator=g)
    c.pos2 = torch.randn(R, 4, generator=g)                                # (column 3: padding nobody may use)
    c.pos2[:, 0:3] = torch.rand(R, 3, generator=g) * 2.0 - 1.0
    c.plants = plants(B, M2)
    for b, (p, q, lone, origin) in enumerate(c.plants):
        o = b * M2
        c.x2[o + p] *= SCALE
        c.x2[o + q], c.pos2[o + q] = c.x2[o + p], c.pos2[o + p]
        if lone is not None:
            c.x2[o + lone] *= -SCALE
        c.pos2[o + origin, 0:3] = 0.0
    # ---- SA3: the dead channel, the offset channel, the margin
    sa3, fp3 = c.blk["sa3"], c.blk["fp3"]
    u = torch.cat([c.x2, c.pos2[:, 0:3]], 1).double()
    wu = u @ sa3["W"].double().t()
    sa3["b"][DEAD] = -(float(wu[:, DEAD].max()) + 1.0)
    sa3["b"][OFFSET] = _offset_bias(wu[:, OFFSET])
    _clear_margin([wu], sa3["b"])
    # ---- FP3 on the plot feature of either statistics mode
    h = torch.relu(wu + sa3["b"].double())
    pres = []
    for mode in ("train", "frozen"):
        mean, var, _, _ = _stats(h, sa3["rm"].double(), sa3["rv"].double(), mode, R)
        a = sa3["gamma"].double() / torch.sqrt(var + EPS)
        x3, _ = _pool(a * h + (sa3["beta"].double() - mean * a), B, M2)
        pres.append(torch.cat([x3.repeat_interleave(M2, 0), c.x2.double()], 1) @ fp3["W"].double().t())
    fp3["b"][DEAD] = -(max(float(p[:, DEAD].max()) for p in pres) + 1.0)
    fp3["b"][OFFSET] = _offset_bias(pres[0][:, OFFSET])
    _clear_margin(pres, fp3["b"])
    _CASES[(B, M2)] = c
    return c


def _run(c, mode, dtype):
    assert mode in ("train", "frozen", "eval")
    B, M2, R = c.B, c.M2, c.R
    x2 = c.x2.to(dtype)
    res = {"batches": 1 if mode == "train" else 0}
    margin = float("inf")

    def block(name, u):
        nonlocal margin
        p = {k: v.to(dtype) for k, v in c.blk[name].items()}
        pre = u @ p["W"].t() + p["b"]
        # rows p and q of a plot are the same numbers, so their products are: a BLAS library may add a row's terms in an order
        # that depends on where the row sits in the matrix (seen: the two rows one ulp of fp64 apart, the copy q the "first" maximum)
        for b_, (p_, q_, _, _) in enumerate(c.plants):
            pre[b_ * M2 + q_] = pre[b_ * M2 + p_]
        h = torch.relu(pre)
        mean, var, new_rm, new_rv = _stats(h, p["rm"], p["rv"], mode, R)
        invstd = 1.0 / torch.sqrt(var + EPS)
        a = p["gamma"] * invstd
        cc = p["beta"] - mean * a
        live = torch.arange(64) != DEAD
        margin = min(margin, float(pre[:, live].abs().min()))
        res.update({f"{name}.a": a.numpy(), f"{name}.c": cc.numpy(), f"{name}.mean": mean.numpy(), f"{name}.invstd": invstd.numpy(),
                    f"{name}.running_mean": new_rm.numpy(), f"{name}.running_var": new_rv.numpy()})
        return h, a * h + cc

    h_sa3, y = block("sa3", torch.cat([x2, c.pos2[:, 0:3].to(dtype)], 1))
    x3, arg3 = _pool(y, B, M2)
    h3, y3 = block("fp3", torch.cat([x3.repeat_interleave(M2, 0), x2], 1))
    res.update(h_sa3=h_sa3.numpy(), y=y.numpy(), x3=x3.numpy(), arg3=arg3, h3=h3.numpy(), out=y3.numpy(), margin=margin)
    return res


def reference(c, mode):
    """fp64 torch of the header's statement.  -> h_sa3, h3 (R, 64); x3 (B, 64), arg3 (B, 64) int32 (first maximum); y = a h + c of SA3
    (R, 64); out = FP3's normalised rows; per block "<name>.a" / .c / .mean / .invstd / .running_mean / .running_var (after one
    step: momentum 0.1, unbiased variance over the B * M2 rows; unchanged in modes frozen and eval); batches: what the step adds
    to num_batches_tracked; margin: the least |pre-activation| of a live channel"""
    return _run(c, mode, F64)


def reference_fp32(c, mode):
    return _run(c, mode, torch.float32)


def decisions(c, ref):
    """Per (plot, channel) of the max, from ref["y"] and ref["h_sa3"] (fp64, or the fp32 restatement's values):
      first (B, 64): the first maximum;  gap: its distance to the best row that is not a bit-identical copy of it (the planted q
      of p);  zero: the extremum is an exact zero of h -- c to the bit on every zero row, the lowest of them wins;  bound: the
      decision bound 2 * OUT_TOL * max |y|;  decided = zero | gap > bound;  planted: the planted pair attains the extremum by more
      than the bound (first == p)."""
    B, M2 = c.B, c.M2
    y = np.asarray(ref["y"], np.float64).reshape(B, M2, 64)
    h = np.asarray(ref["h_sa3"], np.float64).reshape(B, M2, 64)
    first = np.argmax(y, axis=1)
    best = np.take_along_axis(y, first[:, None, :], 1)[:, 0, :]
    rest = y.copy()
    for b, (p, q, _, _) in enumerate(c.plants):
        for ch in range(64):
            f = first[b, ch]
            rest[b, [p, q] if f in (p, q) else [f], ch] = -np.inf
    gap = best - rest.max(1)
    d = type("Decisions", (), {})()
    d.first, d.gap, d.best = first.astype(np.int32), gap, best
    d.zero = np.take_along_axis(h, first[:, None, :], 1)[:, 0, :] == 0.0
    d.bound = 2.0 * OUT_TOL * float(np.abs(y).max())
    d.decided = d.zero | (gap > d.bound)
    d.planted = np.stack([(first[b] == p) & (gap[b] > d.bound) & ~d.zero[b] for b, (p, _, _, _) in enumerate(c.plants)])
    d.undecided_share = float((~d.decided).mean())
    return d


# ---------------------------------------------------------------------------------------------- the pool kernels' cases
MAX_R = (1, 5, 32, 33, 300)
MAX_C = (64, 34)
POOL_B, POOL_R, POOL_STRIDES = (1, 3, 28), (1, 16, 127, 128, 129, 300), (64, 68)
PAD = -777.25


@functools.lru_cache(maxsize=None)
def max_case(B, R, C):
    """sn2_plot_max_forward in exact arithmetic: h (B*R, hs) on the lattice of multiples of 1/8 in [-4, 4] (padding columns PAD),
    a in +-{1/4, 1/2, 1, 2} with a[4] = 0, c multiples of 1/4 in [-2, 2]: a h + c is a multiple of 1/32 below 16 in magnitude, exact
    in fp32 (an fma or a multiply and an add alike).  Planted per plot b, with G = 256 // C row groups and r0 = (2 + b) % R:
    column 1 (a = 1): rows r0 and r0 + G hold the maximum 4 (one thread's row sequence); column 2 (a = -2): rows r0 and r0 + 1 hold
    the minimum -4 (neighbouring row groups); column 3: 1/2 on every row; column 4: a = 0 (all equal: row 0).
    -> namespace h, a, c (fp32 numpy), out (B, C) fp32, arg (B, C) int32"""
    g = torch.Generator().manual_seed(7 + 1000 * B + 10 * R + C)
    hs, G = (C + 3) // 4 * 4, 256 // C
    h = torch.randint(-31, 32, (B, R, hs), generator=g).float() / 8
    a = torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (C,), generator=g)]
    a[::5] *= -1.0
    a[1], a[2], a[4] = 1.0, -2.0, 0.0
    cc = torch.randint(-8, 9, (C,), generator=g).float() / 4
    for b in range(B):
        r0 = (2 + b) % R
        h[b, [r for r in (r0, r0 + G) if r < R], 1] = 4.0
        h[b, [r for r in (r0, r0 + 1) if r < R], 2] = -4.0
    h[:, :, 3] = 0.5
    h[:, :, C:] = PAD
    m = type("MaxCase", (), {})()
    m.B, m.R, m.C, m.hs, m.G = B, R, C, hs, G
    m.h, m.a, m.c = h.view(B * R, hs).numpy(), a.numpy(), cc.numpy()
    y = m.a[None, None, :] * h.numpy()[:, :, :C] + m.c[None, None, :]                      # fp32: exact
    y64 = m.a.astype(np.float64)[None, None, :] * h.numpy()[:, :, :C].astype(np.float64) + m.c.astype(np.float64)[None, None, :]
    assert y.dtype == np.float32 and np.array_equal(y.astype(np.float64), y64)
    m.y = y
    m.arg = np.argmax(y, axis=1).astype(np.int32)
    m.out = np.take_along_axis(y, m.arg[:, None, :].astype(np.int64), 1)[:, 0, :].copy()
    return m


@functools.lru_cache(maxsize=None)
def max_backward_case(B, R, C):
    """sn2_plot_max_backward: dout (B, C), arg (B, C) with entries -1 and R that must write nothing.  -> namespace dout, arg, dy0
    (B*R + 64, hs) pre-filled with PAD, dy (expected)"""
    g = torch.Generator().manual_seed(11 + 1000 * B + 10 * R + C)
    hs = (C + 3) // 4 * 4
    m = type("MaxBackwardCase", (), {})()
    m.B, m.R, m.C, m.hs = B, R, C, hs
    m.dout = torch.randn(B, C, generator=g).numpy()
    arg = torch.randint(0, R, (B, C), generator=g, dtype=torch.int32)
    arg[:, 3], arg[:, 6] = -1, R
    arg[0, 0], arg[B - 1, C - 1] = 0, R - 1
    m.arg = arg.numpy()
    m.dy0 = np.full((B * R + 64, hs), PAD, np.float32)
    m.dy = m.dy0.copy()
    for b in range(B):
        for ch in range(C):
            if 0 <= m.arg[b, ch] < R:
                m.dy[b * R + m.arg[b, ch], ch] = m.dout[b, ch]
    m.written = int(((m.arg >= 0) & (m.arg < R)).sum())
    return m


@functools.lru_cache(maxsize=None)
def pool_backward_case(B, R, stride):
    """sn2_global_pool_backward (C = 64): du (B*R, stride) normal (padding columns PAD), arg, h, mean, invstd random, non-zero
    lattice pre-fills of dx, dgamma, dbeta (ACCUMULATED outputs); plot 0's channel ZERO_CH has an all-zero du column and a zero dx
    pre-fill (the kernel's `g != 0` skip).  -> namespace with the inputs, and per name in ("dx", "dgamma", "dbeta") the fp64 result
    `ref[name]` and the fp32 restatement `r32[name]` of the header's three formulas (pre-fill included)"""
    g = torch.Generator().manual_seed(13 + 1000 * B + 10 * R + stride)
    m = type("PoolBackwardCase", (), {})()
    m.B, m.R, m.stride, m.ZERO_CH = B, R, stride, 9
    du = torch.randn(B * R, stride, generator=g)
    du[:R, m.ZERO_CH] = 0.0
    du[:, 64:] = PAD
    arg = torch.randint(0, R, (B, 64), generator=g)
    arg[0, 0], arg[B - 1, 63] = 0, R - 1
    h = torch.relu(torch.randn(B * R, 64, generator=g))
    mean, invstd = torch.randn(64, generator=g) * 0.3, torch.rand(64, generator=g) + 0.5
    lattice = lambda *s: (torch.randint(1, 9, s, generator=g).float() / 4) * torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0)  # noqa: E731
    dx0, dgamma0, dbeta0 = lattice(B, 64), lattice(64), lattice(64)
    dx0[0, m.ZERO_CH] = 0.0
    m.du, m.arg, m.h, m.mean, m.invstd = du.numpy(), arg.to(torch.int32).numpy(), h.numpy(), mean.numpy(), invstd.numpy()
    m.dx0, m.dgamma0, m.dbeta0 = dx0.numpy(), dgamma0.numpy(), dbeta0.numpy()
    rows = (torch.arange(B)[:, None] * R + arg)                                            # (B, 64) the rows named by arg
    for name, dt in (("ref", F64), ("r32", torch.float32)):
        dx = dx0.to(dt) + du[:, :64].to(dt).view(B, R, 64).sum(1)
        xhat = (h.to(dt).gather(0, rows) - mean.to(dt)) * invstd.to(dt)
        setattr(m, name, {"dx": dx.numpy(), "dbeta": (dbeta0.to(dt) + dx.sum(0)).numpy(), "dgamma": (dgamma0.to(dt) + (dx * xhat).sum(0)).numpy()})
    m.rows = rows.numpy()
    return m


# ---------------------------------------------------------------------------------------------- distances
STAT_ATOL, STAT_RTOL = 1e-5, 1e-4                      # tests/test_gpu_fp_blocks.py: the running statistics' tolerance


def distances(got, ref):
    """The figures both tests assert, from dictionaries with reference()'s keys: -> {name: (distance, bound)}.
    h_sa3, h3, x3 and per block a, c, mean, invstd: the largest difference over the array's largest magnitude (a, c, invstd: over
    the live channels', and the dead channel's invstd relative to itself), bound OUT_TOL; the running statistics: the largest of
    |difference| / (STAT_ATOL + STAT_RTOL |reference|), bound 1 (numpy's allclose)."""
    out = {}
    f = lambda v: np.asarray(v, np.float64)                                                # noqa: E731
    for n in ("h_sa3", "x3", "h3"):
        out[n] = (float(np.abs(f(got[n]) - ref[n]).max() / np.abs(ref[n]).max()), OUT_TOL)
    live = np.arange(64) != DEAD
    for blk, _, _ in BLOCKS:
        for s in STATS:
            k = f"{blk}.{s}"
            out[k] = (float(np.abs(f(got[k])[live] - ref[k][live]).max() / np.abs(ref[k][live]).max()), OUT_TOL)
        k = f"{blk}.invstd"
        out[k + "[DEAD]"] = (float(abs(f(got[k])[DEAD] - ref[k][DEAD]) / ref[k][DEAD]), OUT_TOL)
        for s in ("running_mean", "running_var"):
            k = f"{blk}.{s}"
            out[k] = (float((np.abs(f(got[k]) - ref[k]) / (STAT_ATOL + STAT_RTOL * np.abs(ref[k]))).max()), 1.0)
    return out


def show(tag, dist, other=None):
    """prints every figure next to its bound (and next to `other`'s figure: the fp32 restatement's); -> the names out of bound"""
    for k, (e, bound) in dist.items():
        print(f"{tag} {k:22s} {e:.2e} (bound {bound:.0e}" + (f", fp32 restatement {other[k][0]:.2e})" if other else ")"))
    return [(k, e, bound) for k, (e, bound) in dist.items() if not e <= bound]
