"""Set-abstraction modules alone: hand-made cases and their fp64 reference, for tests/test_sa_module_ref_host.py (which proves on
the CPU what the GPU test rests on) and tests/test_gpu_sa_modules.py (which runs csrc/sa_mfma.hip on them).  Not a test module;
imports numpy and torch, never the library.

  * kinds: "sa2" (cf 16, MLP[19,32]) and "sa3" (cf 32, MLP[35,64]) have ONE block, h = relu(W [feat | pos_j - pos_i] + b), and the
    extremum is taken on h.  Their inputs are small dyadic rationals -- features multiples of 1/8 in [-2, 2], positions multiples
    of 1/16 in [0, 2), W and b multiples of 1/8 in [-1, 1] -- so every product is a multiple of 2^-7 and every partial sum is far
    below 2^17: h is EXACT in fp32 in any summation order, and with bfloat16 operands too (at most 6 significand bits each).  The
    extremum and its slot of a forward pass must therefore equal the fp64 reference bit for bit.  "sa1" (cf 8, MLP[11,16,16]) has
    continuous inputs (the recipe of tests/test_gpu_sa1_one_pass.py): its second block sits behind a BatchNorm affine.
  * layouts: A "classes" (both sides of every item-class threshold, an empty centroid, a three-step SOLO item, short last items),
    B "rounds" (48 SOLO items on 12 waves: four rounds of the snake), C "groups" (33 plots: four groups of 8 and a lone plot; one
    aligned quad of centroids without any neighbour).
    The last four source rows of every plot are on no list: their feature gradient must stay what it was.
  * planted ties (sa2 / sa3): a source row (features and position) stands at TWO slots of a neighbour list, so every channel ties
    between the two.  For the tie to BE the extremum often enough to count, the row is a strong one: its features are 2 sign(sum of
    the W rows of three or four positive-gamma channels), still multiples of 1/8 in [-2, 2].
  * wrong variants of the reference: rule="last" (the highest slot wins a tie), rule="unsigned" (plain maximum whatever gamma's
    sign).  Host code only: the host test shows that each differs from the reference in what the GPU test compares bit for bit.
"""
import functools
import os
import re
import types

import numpy as np
import torch

F64 = torch.float64
SEEDS = {"sa1": 6, "sa2": 1, "sa3": 1}              # tests/test_sa_module_ref_host.py asserts what the choice must give: tie counts, sa1's margin
EPS, MOMENTUM = 1e-5, 0.1
KINDS = {"sa1": (8, (11, 16, 16)), "sa2": (16, (19, 32)), "sa3": (32, (35, 64))}
LAYOUTS = {"A": (2, 384, 41, 160), "B": (2, 128, 24, 96), "C": (33, 64, 24, 32)}            # B, Nsrc, M, cap
UNLISTED = 4                                        # source rows at the end of every plot that no list names
SPECIAL_A = (0, 1, 4, 5, 8, 9, 64, 65, 150)
PLANTED_A = {150: ((15, 16), (63, 64), (148, 149)), 64: ((15, 16), (62, 63)), 8: ((0, 7), (3, 4)), 4: ((0, 3),), 9: ((7, 8),),
             65: ((63, 64),)}                       # (65: the lone message of a SOLO item's second step ties with the first step's last)
PLANTED_B = ((31, 32), (47, 48))                    # on two lists per plot
SPECIAL_C32 = (0, 1, 4, 5, 8, 9, 20, 32)            # plot 32, the lone group: mixed
PLANTED_C32 = {8: ((3, 4),), 4: ((0, 3),), 9: ((7, 8),)}
EMPTY_QUAD_PLOT = 7                                 # layout C: four consecutive centroids (4..7) of this plot have no neighbour --
#                                                     without an order table they are a quad of their own, which no message reaches
CLASS_NAMES = ("SOLO", "QUAD", "OCT", "HEX", "EMPTY")


@functools.lru_cache(maxsize=None)
def thresholds():
    """(SN2_SA_OCT_MIN, SN2_SA_QUAD_MIN, SN2_SA_SOLO_MIN) as include/strata_hip.h defines them."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "strata_hip.h")
    with open(path) as f:
        text = f.read()
    return tuple(int(re.search(rf"#define\s+SN2_SA_{n}_MIN\s+(\d+)", text).group(1)) for n in ("OCT", "QUAD", "SOLO"))


def classes(cnt):
    """Per centroid: the item class sn2_sa_order puts it in ("SOLO" / "QUAD" / "OCT" / "HEX"), "EMPTY" for no neighbour (an empty
    centroid rides in a HEX item)."""
    oct_min, quad_min, solo_min = thresholds()
    c = np.asarray(cnt, dtype=np.int64)
    return np.where(c > solo_min, "SOLO", np.where(c > quad_min, "QUAD", np.where(c > oct_min, "OCT", np.where(c > 0, "HEX", "EMPTY"))))


def _dyadic(g, shape, lo, hi, den):
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float32) / den


def _plant(case, i, pairs, pinned, pair_no):
    """Make the sources at slots (s1, s2) of centroid i's list the same row, a strong one (module docstring).  False, and nothing
    changed, if that would overwrite a row an earlier pair stands on: the caller draws the list again."""
    cf, W, gamma = case.cf, case.params[0]["W"], case.params[-1]["gamma"]
    pos_ch = [c for c in range(W.shape[0]) if gamma[c] > 0]
    base = (i // case.M) * case.Nsrc
    rows = [(base + int(case.nbr[i, s1]), base + int(case.nbr[i, s2])) for s1, s2 in pairs]
    if any(r in pinned for pair in rows for r in pair):
        return False
    for (s1, s2), (r1, r2) in zip(pairs, rows):
        k = 3 + (pair_no[0] & 1)
        chs = [pos_ch[(4 * pair_no[0] + u) % len(pos_ch)] for u in range(k)]
        case.rows[r1, :cf] = torch.where(W[chs, :cf].sum(0) < 0, -2.0, 2.0)
        case.rows[r2] = case.rows[r1]
        pinned.update((r1, r2))
        pair_no[0] += 1
        case.planted.append((i, s1, s2))
    return True


def _list(g, pool, n):
    return torch.randperm(pool, generator=g)[:n].sort().values.int()                         # ascending, distinct


@functools.lru_cache(maxsize=None)
def make_case(kind, layout, seed):
    """-> namespace: rows (B*Nsrc, cf + 4) = [feat | x y z .], cpos (B*M, 4), nbr (B*M, cap) i32 of per-plot source indices
    (ascending and distinct within a list, 0 behind it), cnt, total, params (per block: W, b, gamma, beta, rm, rv), dout,
    dfeat0 (the feature gradient's pre-fill), planted [(centroid, slot, slot)].  Shared between tests: never written to."""
    cf, mlp = KINDS[kind]
    B, Nsrc, M, cap = LAYOUTS[layout]
    g = torch.Generator().manual_seed(1000 * seed + 10 * sorted(KINDS).index(kind) + sorted(LAYOUTS).index(layout))
    exact = kind != "sa1"
    case = types.SimpleNamespace(kind=kind, layout=layout, seed=seed, B=B, Nsrc=Nsrc, M=M, cap=cap, cf=cf, mlp=mlp, exact=exact,
                                 planted=[])
    stride = cf + 4                                                                           # [feat | x y z .], a multiple of 4
    rows = torch.zeros(B * Nsrc, stride)
    cpos = torch.zeros(B * M, 4)
    if exact:
        rows[:, :cf] = _dyadic(g, (B * Nsrc, cf), -16, 16, 8)
        rows[:, cf:cf + 3] = _dyadic(g, (B * Nsrc, 3), 0, 31, 16)
        cpos[:, :3] = _dyadic(g, (B * M, 3), 0, 31, 16)
    else:
        rows[:, :cf] = torch.randn(B * Nsrc, cf, generator=g)
        rows[:, cf:cf + 3] = torch.rand(B * Nsrc, 3, generator=g) * 2.0
        cpos[:, :3] = torch.rand(B * M, 3, generator=g) * 2.0
    case.rows, case.cpos = rows, cpos
    # ---- block parameters
    case.params = []
    for k in range(len(mlp) - 1):
        ci, co = mlp[k], mlp[k + 1]
        if exact:
            W, b = _dyadic(g, (co, ci), -8, 8, 8), _dyadic(g, (co,), -8, 8, 8)
        else:
            W, b = torch.randn(co, ci, generator=g) * (0.4 if k == 0 else 0.3), torch.randn(co, generator=g) * (0.2 if k == 0 else 0.1)
        gamma, beta = torch.rand(co, generator=g) + 0.5, torch.randn(co, generator=g) * 0.1
        if k == len(mlp) - 2:
            gamma[::3] *= -1.0
        case.params.append({"W": W, "b": b, "gamma": gamma, "beta": beta,
                            "rm": torch.linspace(0.1, 0.4, co), "rv": torch.linspace(0.5, 1.5, co)})
    # ---- neighbour lists
    pool = Nsrc - UNLISTED
    cnt = torch.zeros(B * M, dtype=torch.int32)
    nbr = torch.zeros(B * M, cap, dtype=torch.int32)                                          # unused slots: 0, a valid index
    case.cnt, case.nbr = cnt, nbr
    pinned, pair_no = set(), [0]
    for b in range(B):
        if layout == "A":
            counts = list(SPECIAL_A) + torch.randint(0, 13, (M - len(SPECIAL_A),), generator=g).tolist()
            todo, nspecial = PLANTED_A, len(SPECIAL_A)
        elif layout == "B":
            counts = torch.randint(65, 97, (M,), generator=g).tolist()
            todo, nspecial = {}, 0
        else:
            counts = torch.randint(0, 21, (M,), generator=g).tolist()
            todo, nspecial = {}, 0
            if b == 5:
                counts = [1] * M                                                              # HEX only
            if b == 6:
                counts = [9] * M                                                              # QUAD only
            if b == B - 1:
                counts[:len(SPECIAL_C32)] = SPECIAL_C32
                todo, nspecial = PLANTED_C32, len(SPECIAL_C32)
        perm = torch.randperm(M, generator=g).tolist()
        for rank, (i, n) in enumerate(zip(perm, counts)):
            if layout == "C" and b == EMPTY_QUAD_PLOT and 4 <= i < 8:
                n = 0                                                                         # centroids 4..7: an aligned quad, all empty
            pairs = todo.get(n, ()) if rank < nspecial else (PLANTED_B if layout == "B" and rank < 2 else ())
            cnt[b * M + i] = n
            for attempt in range(100):
                nbr[b * M + i, :n] = _list(g, pool, n)
                if not (exact and pairs) or _plant(case, b * M + i, pairs, pinned, pair_no):
                    break
            else:
                raise AssertionError("planted pairs collide in every draw")
    case.total = cnt.sum().to(torch.int64).reshape(1)
    for i, s1, s2 in case.planted:
        base = (i // M) * Nsrc
        assert torch.equal(case.rows[base + int(nbr[i, s1])], case.rows[base + int(nbr[i, s2])])
    cl = mlp[-1]
    case.dout = torch.randn(B * M, cl, generator=g)
    sign = torch.where(torch.rand(B * Nsrc, cf, generator=g) < 0.5, -1.0, 1.0)
    case.dfeat0 = sign * torch.randint(1, 9, (B * Nsrc, cf), generator=g).to(torch.float32) / 4       # nonzero multiples of 1/4
    return case


def case_of(kind, layout):
    """The case the tests run: make_case with the kind's seed."""
    return make_case(kind, layout, SEEDS[kind])


def messages(case):
    """-> (cen, slot, src, start): per message its centroid, its slot in the list and its global source row; start (B*M): the first
    message of a centroid."""
    cnt = case.cnt.long()
    cen = torch.repeat_interleave(torch.arange(case.B * case.M), cnt)
    start = torch.cumsum(cnt, 0) - cnt
    slot = torch.arange(int(cnt.sum())) - start[cen]
    src = (cen // case.M) * case.Nsrc + case.nbr[cen, slot].long()
    return cen, slot, src, start


def grad_names(case):
    return tuple(f"{n}{k}" for k in range(len(case.mlp) - 1) for n in ("dW", "db", "dgamma", "dbeta"))


def _run(case, mode, dout, dfeat0, dtype, rule, arg_in, backward):
    assert mode in ("train", "frozen", "eval") and rule in ("first", "last", "unsigned")
    cen, slot, src, start = messages(case)
    ncent, cap, cf, nl = case.B * case.M, case.cap, case.cf, len(case.mlp) - 1
    rows = case.rows.to(dtype)
    feat = rows[:, :cf].clone().requires_grad_(backward)
    q = [{k: v.to(dtype).clone().requires_grad_(backward and k in ("W", "b", "gamma", "beta")) for k, v in p.items()} for p in case.params]
    x = torch.cat([feat[src], rows[src, cf:cf + 3] - case.cpos.to(dtype)[cen, 0:3]], 1)
    E = x.shape[0]
    new_rm, new_rv = [], []
    for k, p in enumerate(q):
        h = torch.relu(x @ p["W"].t() + p["b"])
        if mode == "train":
            mean, var = h.mean(0), h.var(0, unbiased=False)
            new_rm.append(((1 - MOMENTUM) * p["rm"] + MOMENTUM * mean).detach())
            new_rv.append(((1 - MOMENTUM) * p["rv"] + MOMENTUM * var * (E / (E - 1))).detach())
        else:
            mean, var = p["rm"], p["rv"]
            new_rm.append(p["rm"].clone()), new_rv.append(p["rv"].clone())
        if k < nl - 1:
            x = p["gamma"] * (h - mean) / torch.sqrt(var + EPS) + p["beta"]
    C = h.shape[1]
    gamma, beta = q[-1]["gamma"], q[-1]["beta"]
    sgn = torch.ones(C, dtype=dtype) if rule == "unsigned" else torch.where(gamma.detach() < 0, -1.0, 1.0).to(dtype)
    empty = case.cnt == 0
    if arg_in is None:
        S = torch.full((ncent, cap, C), -float("inf"), dtype=dtype)
        S[cen, slot] = sgn * h.detach()
        best = S.max(1).values
        attained = S == best[:, None, :]
        grid = torch.arange(cap)[None, :, None]
        arg = torch.where(attained, grid, -1).amax(1) if rule == "last" else torch.where(attained, grid, cap).amin(1)
        arg = torch.where(empty[:, None], -1, arg)
    else:
        arg = torch.as_tensor(arg_in).long()
    chosen = h[(start[:, None] + arg.clamp(min=0)).clamp(max=E - 1), torch.arange(C)[None, :]]
    ext = torch.where(empty[:, None], torch.zeros((), dtype=dtype), chosen)
    out = torch.where(empty[:, None], torch.zeros((), dtype=dtype), gamma * (ext - mean) / torch.sqrt(var + EPS) + beta)
    res = {"h": h.detach().numpy(), "ext": ext.detach().numpy(), "arg": arg.to(torch.int32).numpy(), "out": out.detach().numpy(),
           "running_mean": [v.numpy() for v in new_rm], "running_var": [v.numpy() for v in new_rv],
           "batches": 1 if mode == "train" else 0}
    if backward:
        (out * dout.to(dtype)).sum().backward()
        for k, p in enumerate(q):
            for n, key in (("dW", "W"), ("db", "b"), ("dgamma", "gamma"), ("dbeta", "beta")):
                res[f"{n}{k}"] = p[key].grad.numpy()
        res["dfeat"] = (dfeat0.to(dtype) + feat.grad).numpy()
    return res


def reference(case, mode, dout=None, dfeat0=None, rule="first"):
    """fp64, over the explicit message tensor.  The extremum is the SIGNED one, sign(gamma) h of the last block, its slot the lowest
    that attains it; -1 and ext = 0 for a centroid without neighbours (out = 0 there).  With `dout`: autograd through a gather on
    the slot -> dW, db, dgamma, dbeta per block and dfeat = dfeat0 + gradient.  Train mode normalises over all E messages, eps
    1e-5, and moves the running statistics as torch does (momentum 0.1, unbiased variance); frozen and eval take the running
    statistics as constants and leave them."""
    back = dout is not None and mode != "eval"
    return _run(case, mode, dout, case.dfeat0 if dfeat0 is None else dfeat0, F64, rule, None, back)


def reference_fp32(case, mode, arg, dout=None, dfeat0=None):
    """The same formulas in torch fp32 on the CPU, routed by the fp64 reference's `arg`: the yardstick of fp32 rounding."""
    back = dout is not None and mode != "eval"
    return _run(case, mode, dout, case.dfeat0 if dfeat0 is None else dfeat0, torch.float32, "first", arg, back)


def class_mask(case, name):
    """(B*M, 1) fp32: 1 on the centroids of one item class."""
    return torch.from_numpy((classes(case.cnt.numpy()) == name).astype(np.float32))[:, None]


def plot_mask(case, b):
    m = torch.zeros(case.B * case.M, 1)
    m[b * case.M:(b + 1) * case.M] = 1.0
    return m


def tied_positive(case, ref):
    """(B*M, C) int: how many slots attain a POSITIVE signed extremum (0 where it is not positive), and the (B*M, cap, C) mask."""
    cen, slot, _, _ = messages(case)
    C = ref["h"].shape[1]
    sgn = np.where(case.params[-1]["gamma"].numpy() < 0, -1.0, 1.0)
    S = np.full((case.B * case.M, case.cap, C), -np.inf)
    S[cen.numpy(), slot.numpy()] = sgn * ref["h"]
    best = S.max(1)
    attained = (S == best[:, None, :]) & (best[:, None, :] > 0)
    return attained.sum(1), attained
