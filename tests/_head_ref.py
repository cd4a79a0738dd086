"""The pointwise head alone: hand-made cases and their fp64 reference, for tests/test_head_ref_host.py (which proves on the CPU
what the GPU tests rest on), tests/test_gpu_head_backward.py (sn2_head_backward through hip_ops) and
tests/test_gpu_bn_sums_consumer.py (sn2_head_bn_sums).  Not a test module; imports numpy and torch, never the library.

  * the head (include/strata_hip.h: sn2_head): y = fa f + fc on the 34 live columns of rows of 36, pre = W1 y + b1, z = relu(pre),
    dropout by the rows' 16-bit keep words (bit j set = hidden channel j kept and scaled by 1 / (1 - p); p = 1: scale 0),
    s = W2 z + b2, proba = softmax(s[:4]), cov = proba * sigmoid(s[4]).  The backward takes dcov and dproba (either may be
    absent) and returns dy = the gradient with respect to y (NOT f), dW1, db1, dW2, db2.
  * a case = R rows (`make_case`): weights from torch.manual_seed(7) Linear layers, as the two older head tests make them; W1's
    column ZERO_COL is zero (that column of dy is exactly zero); hidden channel DEAD has a bias below -max(W1 y) - 1 (its row of
    dW1, its db1 and its column of dW2 are exactly zero); from 8 rows on, four rows are scaled so that s[4] is +30, -30, +100,
    -100 without dropout (about twice that with: their keep words are 0xFFFF) -- a saturated sigmoid whose expf overflows on the
    far side, and a softmax that is one-hot; the padding columns 34, 35 of f hold PAD.
  * the rows' affine is a BatchNorm's: gamma, beta, mean, invstd are chosen, fa = gamma invstd and fc = beta - mean fa are built
    in fp32 as the library's finalisation builds them (csrc/misc.hip: bn_finalize_kernel).  `make_case(R, gamma_ch, beta_ch)`
    sets channel SWEEP_CH's gamma and beta (the sweep and the fallback of tests/test_gpu_bn_sums_consumer.py).
  * no live pre-activation lies within MARGIN = 2^-15 (times the row's largest |y| where that is above 1: the four scaled rows) of
    zero, in fp64, in the fp32 restatement and from the rows rounded to bfloat16 (`_separate`, as tests/_fp_block_ref.py): the
    kernel's ReLU mask IS the reference's and every difference is rounding.
  * head(): the forward and the hand-written backward in one dtype -- fp64 is the reference (`reference`), fp32 the yardstick of
    fp32 rounding (`reference_fp32`), both from the rows AS STORED (f.to(bfloat16) for bfloat16 rows).  Row sums are taken in
    blocks of ROW_BLOCK rows, so that a sum over 131 137 rows does not hang on the BLAS library's split.  Also the BatchNorm
    sums of the rows, dbeta = sum dy, dgamma = sum dy xhat, xhat = (f - mean) invstd (`row_pass`: in fp64, and in fp32).
  * identity(): what bn_sums_from_consumer_kernel computes, W1^T G with G = (dW1 - beta db1) / gamma, in fp64 from whatever dW1 /
    db1 it is handed; identity_taken(): whether the kernel takes it (else its own row pass), as the header states the rule.
"""
import functools

import numpy as np
import torch

F64, F32 = torch.float64, torch.float32
C, STRIDE, HID, OUT = 34, 36, 16, 5
DEAD, ZERO_COL, SWEEP_CH = 7, 5, 11
MARGIN = 2.0 ** -15
PAD = 777.25
DROP_P = 0.5
EXTREME = (30.0, -30.0, 100.0, -100.0)
ROW_BLOCK = 4096
ROWS = {"fp32": torch.float32, "bf16": torch.bfloat16}
SMALL_ROWS = (1, 63, 64, 65, 255, 256, 257, 805)
SUMS_ROWS = (805, 4160)                               # the consumer identity; 4160 = 65 turns, 17 workgroups
FALLBACK_ROWS = (1, 255, 256, 257, 805)               # the row pass's 256-thread stride loop
_T = float(np.float32(1e-4))                          # the kernel's line: the identity needs |gamma| > 1e-4f on every channel
_T_UP = float(np.nextafter(np.float32(1e-4), np.float32(1.0)))
SWEEP_GAMMAS = (_T_UP, -_T_UP, 3e-4, 1e-3, 1e-2, 1.0)
SWEEP_BETAS = (0.0, 1.0, 8.0)
FALLBACK_GAMMAS = (0.0, _T, -_T)
N_FLAT = HID * C + HID + OUT * HID + OUT
GRAD_SHAPES = (("dW1", (HID, C)), ("db1", (HID,)), ("dW2", (OUT, HID)), ("db2", (OUT,)))


def _mm(a, b):
    """a (R, k) @ b (k, n), the rows in blocks"""
    return torch.cat([a[i:i + ROW_BLOCK] @ b for i in range(0, a.shape[0], ROW_BLOCK)])


def _tmm(a, b):
    """a^T b = sum over the rows, as a sum of per-block products"""
    out = torch.zeros(a.shape[1], b.shape[1], dtype=a.dtype)
    for i in range(0, a.shape[0], ROW_BLOCK):
        out += a[i:i + ROW_BLOCK].t() @ b[i:i + ROW_BLOCK]
    return out


def _colsum(a):
    out = torch.zeros(a.shape[1], dtype=a.dtype)
    for i in range(0, a.shape[0], ROW_BLOCK):
        out += a[i:i + ROW_BLOCK].sum(0)
    return out


def stored(t, rows):
    """the values a buffer of the rows' storage type holds, as fp64"""
    return t.to(ROWS[rows]).to(F64)


def keep_scale(c, drop, drop_p, dtype):
    """(R, 16) factor of the dropout: 1 / (1 - p) where the row's bit is set, else 0 (p = 1: 0 everywhere); None without"""
    if not drop:
        return None
    scale = 1.0 / (1.0 - drop_p) if drop_p < 1.0 else 0.0
    bits = (c.keep[:, None] >> torch.arange(HID, dtype=torch.int32)[None, :]) & 1
    return bits.to(dtype) * scale


def head(c, rows="fp32", drop=False, dcov=True, dproba=True, dtype=F64, drop_p=DROP_P, backward=True, y_in=None, params=None,
         exact_affine=False):
    """The head of case c in `dtype` from the rows as stored -> dict of numpy arrays: y, pre, s, cov, proba, loss (= sum cov dcov +
    sum proba dproba) and, with backward, dpre (R, 16), dy (R, 34), dW1, db1, dW2, db2.  y_in / params replace y or a weight (finite
    differences); exact_affine: fa, fc built in fp64 from gamma, beta, mean, invstd instead of the case's fp32 ones."""
    p = {k: getattr(c, k).to(dtype) for k in ("W1", "b1", "W2", "b2")}
    if params:
        p.update({k: v.to(dtype) for k, v in params.items()})
    f = c.f.to(ROWS[rows]).to(dtype)[:, :C]
    if exact_affine:
        fa = c.gamma.to(dtype) * c.invstd.to(dtype)
        fc = c.beta.to(dtype) - c.mean.to(dtype) * fa
    else:
        fa, fc = c.fa.to(dtype), c.fc.to(dtype)
    y = fa * f + fc if y_in is None else y_in.to(dtype)
    pre = _mm(y, p["W1"].t()) + p["b1"]
    act = pre > 0
    ks = keep_scale(c, drop, drop_p, dtype)
    z1 = torch.relu(pre) if ks is None else torch.relu(pre) * ks
    s = _mm(z1, p["W2"].t()) + p["b2"]
    proba = torch.softmax(s[:, :4], 1)
    sg = torch.sigmoid(s[:, 4:5])
    cov = proba * sg
    gc = c.dcov.to(dtype) if dcov else torch.zeros(c.R, 4, dtype=dtype)
    gp = c.dproba.to(dtype) if dproba else torch.zeros(c.R, 4, dtype=dtype)
    res = {"y": y, "pre": pre, "s": s, "cov": cov, "proba": proba, "loss": (cov * gc).sum() + (proba * gp).sum()}
    if backward:
        dp = gc * sg + gp
        ds = torch.cat([proba * (dp - (dp * proba).sum(1, keepdim=True)), (gc * proba).sum(1, keepdim=True) * sg * (1 - sg)], 1)
        dz1 = _mm(ds, p["W2"])
        dpre = torch.where(act, dz1 if ks is None else dz1 * ks, torch.zeros_like(dz1))
        res.update(dpre=dpre, dy=_mm(dpre, p["W1"]), dW1=_tmm(dpre, y), db1=_colsum(dpre), dW2=_tmm(ds, z1), db2=_colsum(ds))
    out = {k: v.numpy() for k, v in res.items()}
    out["loss"] = float(out["loss"])
    return out


def row_pass(c, f_rows, dy_rows, dtype=F64):
    """The BatchNorm sums over the rows: dbeta = sum dy, dgamma = sum dy xhat, xhat = (f - mean) invstd, from f (R, >= 34) and dy
    (R, >= 34) as handed in (torch, any dtype) -> (dgamma, dbeta) numpy in `dtype`"""
    f, dy = f_rows[:, :C].to(dtype), dy_rows[:, :C].to(dtype)
    xhat = (f - c.mean.to(dtype)) * c.invstd.to(dtype)
    return _colsum(dy * xhat).numpy(), _colsum(dy).numpy()


def identity(c, dW1, db1):
    """bn_sums_from_consumer_kernel's identity in fp64 from dW1 (16, 34) and db1 (16) (numpy) -> (dgamma, dbeta)"""
    W, g, b = c.W1.double().numpy(), c.gamma.double().numpy(), c.beta.double().numpy()
    dW1, db1 = np.asarray(dW1, np.float64), np.asarray(db1, np.float64)
    G = (dW1 - b[None, :] * db1[:, None]) / g[None, :]
    return (W * G).sum(0), (W * db1[:, None]).sum(0)


def identity_taken(c):
    """the kernel's decision (csrc/head.hip: bn_identity_ok on every channel, in fp32): |gamma| > 1e-4 and |beta| <= 64 |gamma|"""
    g, b = np.abs(c.gamma.numpy()), np.abs(c.beta.numpy())
    return bool(np.all((g > np.float32(1e-4)) & (b <= np.float32(64.0) * g)))


def _pre_variants(c):
    """the live pre-activations in fp64, in the fp32 restatement and from the bfloat16 rows, each with its rows' margin"""
    out = []
    for rows, dtype in (("fp32", F64), ("fp32", F32), ("bf16", F64)):
        f = c.f.to(ROWS[rows]).to(dtype)[:, :C]
        y = c.fa.to(dtype) * f + c.fc.to(dtype)
        pre = _mm(y, c.W1.to(dtype).t()) + c.b1.to(dtype)
        margin = MARGIN * y.abs().max(1).values.clamp(min=1.0)
        out.append((pre.double(), margin.double()))
    return out


def _separate(c):
    """Keep every live pre-activation at least its row's margin from zero in all three evaluations: a row that has one closer
    gets 1/16 (of its largest |f|, where that is above 1) added to f[row, 0], until none is left."""
    live = torch.arange(HID) != DEAD
    for _ in range(32):
        near = torch.zeros(c.R, dtype=torch.bool)
        for pre, margin in _pre_variants(c):
            near |= (pre[:, live].abs() < margin[:, None]).any(1)
        if not bool(near.any()):
            return
        c.f[near, 0] += c.f[near, :C].abs().max(1).values.clamp(min=1.0) / 16
    raise AssertionError("pre-activations next to zero in every draw")


def _score4(c, frow, scale):
    """s[4] of the row scale * frow, without dropout, in fp64 (the dead channel's bias is already far below zero)"""
    y = c.fa.double() * (scale * frow.double()) + c.fc.double()
    z = torch.relu(c.W1.double() @ y + c.b1.double())
    return float(c.W2.double()[4] @ z + c.b2.double()[4])


def _plant_extreme_rows(c, g):
    """four rows spread over the case whose s[4] is EXTREME[i] without dropout: a random direction whose s[4] has the wanted
    sign far out, its length by bisection"""
    c.extreme = {}
    if c.R < 8:
        return
    for i, target in enumerate(EXTREME):
        row = i * (c.R - 1) // 3
        for _ in range(64):
            v = torch.randn(C, generator=g)
            if (_score4(c, v, 4096.0) - target) * (_score4(c, v, 0.0) - target) < 0:
                break
        else:
            raise AssertionError("no direction reaches the target score")
        lo, hi = 0.0, 4096.0
        s_lo = _score4(c, v, lo) - target
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            if ((_score4(c, v, mid) - target) < 0) == (s_lo < 0):
                lo = mid
            else:
                hi = mid
        c.f[row, :C] = (0.5 * (lo + hi) * v.double()).float()
        c.keep[row] = 0xFFFF
        c.extreme[row] = target


_CASES = {}


def make_case(R, gamma_ch=None, beta_ch=None):
    """-> namespace of CPU tensors, shared between tests and never written to: f (R, 36) fp32, gamma, beta, mean, invstd, fa, fc
    (34), W1, b1, W2, b2, keep (R) int32, dcov, dproba (R, 4), extreme {row: s[4]}"""
    key = (R, None if gamma_ch is None else float(gamma_ch), None if beta_ch is None else float(beta_ch))
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(100003 + R)
    c = type("Case", (), {})()
    c.R = R
    c.f = torch.randn(R, STRIDE, generator=g)
    c.f[:, C:] = PAD
    c.gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.arange(C) % 5 == 0, -1.0, 1.0)
    c.beta = 0.1 * torch.randn(C, generator=g)
    c.mean = 0.2 * torch.randn(C, generator=g)
    c.invstd = 0.75 + 0.5 * torch.rand(C, generator=g)
    if gamma_ch is not None:
        c.gamma[SWEEP_CH] = float(gamma_ch)
    if beta_ch is not None:
        c.beta[SWEEP_CH] = float(beta_ch)
    c.fa = c.gamma * c.invstd                                   # fp32, as bn_finalize_kernel: a = gamma invstd, c = beta - mean a
    c.fc = c.beta - c.mean * c.fa
    torch.manual_seed(7)
    lin1, lin2 = torch.nn.Linear(C, HID), torch.nn.Linear(HID, OUT)
    c.W1, c.b1 = lin1.weight.detach().clone(), lin1.bias.detach().clone()
    c.W2, c.b2 = lin2.weight.detach().clone(), lin2.bias.detach().clone()
    c.W1[:, ZERO_COL] = 0.0
    c.b1[DEAD] = -1.0e6                                         # (dead while the rows are made; its final value below)
    c.keep = torch.randint(0, 1 << 16, (R,), generator=g, dtype=torch.int32)
    c.dcov = torch.randn(R, 4, generator=g)
    c.dproba = torch.randn(R, 4, generator=g)
    _plant_extreme_rows(c, g)
    _separate(c)
    top = 0.0
    for rows in ROWS:
        y = c.fa.double() * stored(c.f, rows)[:, :C] + c.fc.double()
        top = max(top, float((y @ c.W1[DEAD].double()).max()))
    c.b1[DEAD] = -(top + 1.0)
    _CASES[key] = c
    return c


@functools.lru_cache(maxsize=None)
def reference(R, rows="fp32", drop=False, dcov=True, dproba=True, drop_p=DROP_P, gamma_ch=None, beta_ch=None):
    """The fp64 head of make_case(R, gamma_ch, beta_ch) from the rows as stored, with dgamma / dbeta of the rows (computed once
    per argument set, never changed)"""
    c = make_case(R, gamma_ch, beta_ch)
    r = head(c, rows, drop, dcov, dproba, F64, drop_p)
    r["dgamma"], r["dbeta"] = row_pass(c, stored(c.f, rows), torch.from_numpy(r["dy"]))
    return r


@functools.lru_cache(maxsize=None)
def reference_fp32(R, rows="fp32", drop=False, dcov=True, dproba=True, drop_p=DROP_P, gamma_ch=None, beta_ch=None):
    """The same operations in fp32 on the CPU; dgamma / dbeta: the fp32 row pass over the fp32 dy"""
    c = make_case(R, gamma_ch, beta_ch)
    r = head(c, rows, drop, dcov, dproba, F32, drop_p)
    r["dgamma"], r["dbeta"] = row_pass(c, c.f.to(ROWS[rows]).float(), torch.from_numpy(r["dy"]), F32)
    return r


def rel(a, b):
    """largest distance of a from b, relative to b's largest element"""
    b = np.asarray(b, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - b).max()) / float(np.abs(b).max())
