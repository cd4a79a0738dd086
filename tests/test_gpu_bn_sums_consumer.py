"""bn_sums_from_consumer_kernel alone (csrc/head.hip, behind sn2_head_bn_sums and sn2_fp_bn_sums): dgamma / dbeta of a BatchNorm
taken from the weight gradients of the layer that consumes its output, W^T G with G = (dW - beta db) / gamma, or -- where the
kernel decides against that -- its own pass over the rows.  Yardstick everywhere: the sums over the rows in fp64, dbeta = sum dy,
dgamma = sum dy xhat, xhat = (f - mean) invstd.  Bound: the project's gradient rule, max(1e-5, 8 e32), never above 1e-3, relative
to the tensor's largest element, with e32 the distance of the ROW PASS restated in fp32 on the CPU -- the row pass is what the
identity claims to replace; the identity's own fp32 restatement is never the measure.  Every figure is printed next to its bound.

Head side (hip_ops.head_bn_sums; C = 34, 16 consumer rows, 32 images; tests/_head_ref.py builds the cases):
  * planted: dW1 / db1 are the fp64 reference's rounded to fp32 and split over the images without a further rounding (three
    pieces of each value's significand in images 0, 5 and 31, a pair +t / -t in images 9 and 20, the other images zero), so the
    kernel's own arithmetic is alone: the image fold, the fp64 accumulation, col0, the strides.  dgamma / dbeta are ACCUMULATED
    onto a non-zero pre-fill; ok == 1.  R = 805 and 4160.
  * chained: dW1 / db1 as hip_ops.head_backward left them (float atomics into the images), then head_bn_sums.
  * the sweep: channel 11's gamma over nextafter(1e-4f, 1), -nextafter(1e-4f, 1), 3e-4, 1e-3, 1e-2, 1 and its beta over 0, 1, 8,
    all other channels ordinary, on planted and on chained inputs.
  * the fallback: one gamma 0, exactly 1e-4f, -1e-4f: ok == 0 and every channel's sums are the row pass of f and dy as stored
    (the images hold 1e6: unused), R = 1, 255, 256, 257, 805, fp32 and bfloat16 rows, non-zero pre-fill.
FP side (hip_ops.fp_bn_sums after hip_ops.fp_backward; cases of tests/_fp_block_ref.py with a source affine and a 3-NN table): one
case per block shape, <34,8,34> Split, <64,16,34> SourceSide, <64,64,64> Dense; gamma, beta, mean, invstd consistent with the
case's (sa, sc); the identity against sum dsrc and sum dsrc xhat in fp64; the fallback with one gamma zeroed and dsrc pre-filled
with zero; ca > 64 and missing pointers are refused with SN2_EINVAL and nothing is written.

Measured on an MI355X ("Head backward and consumer-side BatchNorm sums alone"; 122 tests in under 3 s, the
slowest 0.8 s), distance from the fp64 row pass relative to the tensor's largest element:
  planted   dgamma 5.0e-8 / 8.1e-8, dbeta 5.2e-8 / 2.8e-8 at R = 805 / 4160 (1 % of the bound; 4.6e-8 ... 5.2e-8 from the identity
            evaluated in fp64 on the same inputs: the fp32 rounding of pre-fill + sum)
  chained   dgamma 1.4e-7 ... 3.0e-6, dbeta 9.7e-8 ... 2.0e-7 (e32 2.0e-7 ... 1.2e-6); the largest figure of the file is 30 % of its
            bound (dgamma, R = 805, bfloat16 rows)
  fallback  0 ... 3.0e-6 (e32 the same: at R = 1 both are the rounding of pre-fill + sum), at most 12 % of the bound
  FP side   identity 1.1e-7 ... 3.3e-6 (e32 2.1e-7 ... 4.2e-6), at most 19 %; fallback 2.6e-8 ... 6.4e-8
THE SWEEP FOUND A BUG, and the kernel's decision changed.  With the decision it had (|gamma| > 1e-4 alone) dgamma of the swept
channel, chained inputs, R = 805 / 4160, as a multiple of the largest element (bound 1.0e-5 ... 4.9e-5; F = outside):
  gamma   beta:       0                    1                      8
  +1e-4 (next up)    2.8e-6 / 1.4e-7      1.8e-4 F / 6.8e-4 F    8.3e-4 F / 4.9e-3 F
  -1e-4 (next up)    3.7e-6 / 2.1e-7      1.2e-4 F / 1.5e-4 F    2.0e-3 F / 4.1e-3 F
  3e-4               1.6e-6 / 3.2e-7      6.7e-5 F / 1.6e-4 F    2.3e-5 F / 2.2e-3 F
  1e-3               8.1e-7 / 7.7e-7      1.5e-5   / 5.4e-5 F    3.7e-4 F / 4.7e-4 F
  1e-2               4.2e-6 / 2.5e-7      1.3e-6   / 2.8e-6      1.8e-5 F / 1.3e-5 F
  1                  2.6e-6 / 1.3e-7      8.7e-6   / 3.9e-7      6.6e-6   / 1.2e-7
and the same picture on planted inputs (dW1, db1 exact to fp32: 7.9e-6 ... 1.2e-3 at |gamma| = 1e-4, beta = 1 or 8; 12 of 36 points outside, chained 17), so the
float atomics are not the cause.  Not |gamma| but |beta / gamma| decides: beta = 0 is inside at every gamma, the threshold
included; every point outside has |beta / gamma| >= 800, every point with |beta / gamma| <= 100 is inside (at most 28 % of the
bound), and the error divided by 2^-24 |beta / gamma| is 0.08 ... 1.1 over all chained points.  The quotient magnifies by
|beta / gamma| the fp32 rounding of dW1, db1 AND of the rows' affine fc = beta - mean fa, which the identity takes for exact.
The kernel now takes the identity only where also |beta| <= 64 |gamma| on every channel (1.1 x 2^-24 x 64 = 4.2e-6: under half of
the 1e-5 floor); after the change every swept point is inside: dgamma 4.5e-8 ... 8.7e-6, at most 27 % of its bound
(gamma = 1e-2, beta = 0, R = 805 chained: an ordinary channel's figure), the twelve (gamma, beta) points with beta != 0 and
gamma <= 1e-2 answer ok = 0 with the row pass's 4.5e-8 ... 2.9e-6.
"""
import numpy as np
import pytest
import torch

import _fp_block_ref as FR
import _head_ref as H
import test_gpu_fp_blocks as FB
from stratanet2_vegetation_coverage_maps_amd import _lib, hip_ops as ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATOM, BOUND, FACTOR = 1e-5, 1e-3, 8
OK_SENT = -7
SWEEP = [(g, b) for g in H.SWEEP_GAMMAS for b in H.SWEEP_BETAS]


def _prefill(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0) * torch.randint(1, 9, (n,), generator=g).float() / 4).numpy()


def _exact_pieces(v):
    """fp32 v = hi + mid + lo, every piece and every partial sum exact (7 + 8 + 9 significand bits)"""
    v = np.ascontiguousarray(v, np.float32)
    top = lambda x: (x.view(np.int32) & np.int32(-65536)).view(np.float32)          # noqa: E731
    hi = top(v)
    rest = v - hi
    mid = top(rest)
    return hi, mid, rest - mid


def _plant(arena, images, off, v, seed):
    """write fp32 array v into the images at flat offset `off`: pieces in images 0, 5, 31, +t / -t in 9 and 20 -> the fp64 sum"""
    n_img, stride = images
    a = arena[:n_img * stride].view(n_img, stride)
    hi, mid, lo = _exact_pieces(v.reshape(-1))
    t = (np.random.default_rng(seed).standard_normal(v.size) * np.abs(v).max()).astype(np.float32)
    for k, piece in ((0, hi), (5, mid), (31, lo), (9, t), (20, -t)):
        a[k, off:off + v.size] = torch.from_numpy(piece.copy()).to(DEV)
    total = hi.astype(np.float64) + mid + lo
    assert np.array_equal(total, v.reshape(-1).astype(np.float64))
    return total.reshape(v.shape)


class _HeadSums:
    """A head case on the device with its gradient images, ready for head_backward and head_bn_sums."""

    def __init__(self, c, rows, dy_rows=None):
        self.c, dt = c, H.ROWS[rows]
        self.f = c.f.to(DEV).to(dt)
        self.lin1, self.lin2 = torch.nn.Linear(H.C, H.HID).to(DEV), torch.nn.Linear(H.HID, H.OUT).to(DEV)
        with torch.no_grad():
            self.lin1.weight.copy_(c.W1), self.lin1.bias.copy_(c.b1), self.lin2.weight.copy_(c.W2), self.lin2.bias.copy_(c.b2)
        self.arena, flat, self.images, _ = ops.grad_images_alloc(H.N_FLAT, DEV)
        views, o = [], 0
        for _, shape in H.GRAD_SHAPES:
            k = int(np.prod(shape))
            views.append(flat[o:o + k].view(shape))
            o += k
        self.dy = torch.zeros(c.R, H.STRIDE, dtype=dt, device=DEV)
        if dy_rows is not None:
            self.dy[:, :H.C] = dy_rows.to(DEV).to(dt)
        # (the descriptor holds addresses only: the object keeps every buffer)
        self.fa, self.fc, self.keep, self.dcov, self.dproba = (t.to(DEV) for t in (c.fa, c.fc, c.keep, c.dcov, c.dproba))
        self.hd = ops.head_desc(self.f, self.fa, self.fc, self.lin1, self.lin2, dcov=self.dcov, dproba=self.dproba, dy=self.dy,
                                grads=views, grad_images=self.images, drop_mask=self.keep, drop_p=H.DROP_P)

    def plant(self, dW1, db1, seed):
        return (_plant(self.arena, self.images, 0, dW1.astype(np.float32), seed),
                _plant(self.arena, self.images, H.HID * H.C, db1.astype(np.float32), seed + 1))

    def sums(self):
        """one sn2_head_bn_sums onto a non-zero pre-fill -> (dgamma, dbeta) minus the pre-fill as fp64, the pre-fills, ok"""
        c = self.c
        pg, pb = _prefill(H.C, 11), _prefill(H.C, 12)
        dgamma, dbeta = torch.from_numpy(pg.copy()).to(DEV), torch.from_numpy(pb.copy()).to(DEV)
        ok = torch.full((1,), OK_SENT, dtype=torch.int32, device=DEV)
        ops.head_bn_sums(self.hd, c.gamma.to(DEV), c.beta.to(DEV), c.mean.to(DEV), c.invstd.to(DEV), dgamma, dbeta, ok)
        torch.cuda.synchronize()
        return dgamma.cpu().numpy().astype(np.float64) - pg, dbeta.cpu().numpy().astype(np.float64) - pb, pg, pb, int(ok.item())


def _bounds(ref, r32, pre):
    """per tensor (scale, e32, bound): e32 of the fp32 row pass including the rounding of pre-fill + sums"""
    out = []
    for r, r3, p in zip(ref, r32, pre):
        scale = float(np.abs(r).max())
        assert scale > 0
        e32 = float(np.abs(((p + r3.astype(np.float32)).astype(np.float64) - p) - r).max()) / scale
        out.append((scale, e32, min(max(ATOM, FACTOR * e32), BOUND)))
    return out


def _judge(tag, got, ref, r32, pre, channel=None):
    bad = []
    for n, g, r, (scale, e32, bound) in zip(("dgamma", "dbeta"), got, ref, _bounds(ref, r32, pre)):
        err = float(np.abs(g - r).max()) / scale
        at = "" if channel is None else f" (channel {channel}: {abs(g[channel] - r[channel]) / scale:.2e})"
        print(f"{tag} {n}: vs fp64 row pass {err:.2e}{at}, bound {bound:.2e} (e32 {e32:.2e}), {100 * err / bound:.0f} % of it")
        if not err <= bound:
            bad.append((n, err, bound))
    return bad


def _head_refs(R, rows, gamma, beta):
    ref = H.reference(R, rows, True, gamma_ch=gamma, beta_ch=beta)
    r32 = H.reference_fp32(R, rows, True, gamma_ch=gamma, beta_ch=beta)
    return ref, r32


# ------------------------------------------------------------------------------------------------ head side
@pytest.mark.parametrize("R", H.SUMS_ROWS)
def test_head_planted_gradients(R):
    c = H.make_case(R)
    ref, r32 = _head_refs(R, "fp32", None, None)
    m = _HeadSums(c, "fp32", torch.from_numpy(ref["dy"]))
    dW1, db1 = m.plant(ref["dW1"], ref["db1"], 3)
    dg, dbt, pg, pb, ok = m.sums()
    assert ok == 1
    ig, ib = H.identity(c, dW1, db1)
    print(f"R {R} planted: kernel vs the identity in fp64 from the same fp32 inputs: dgamma {H.rel(dg, ig):.2e}, dbeta {H.rel(dbt, ib):.2e} "
          f"(includes the fp32 rounding of pre-fill + sum)")
    bad = _judge(f"R {R} planted", (dg, dbt), (ref["dgamma"], ref["dbeta"]), (r32["dgamma"], r32["dbeta"]), (pg, pb))
    assert not bad, bad


@pytest.mark.parametrize("rows", list(H.ROWS))
@pytest.mark.parametrize("R", H.SUMS_ROWS)
def test_head_chained_after_head_backward(R, rows):
    c = H.make_case(R)
    ref, r32 = _head_refs(R, rows, None, None)
    m = _HeadSums(c, rows)
    ops.head_backward(m.hd)
    dg, dbt, pg, pb, ok = m.sums()
    assert ok == 1
    bad = _judge(f"R {R} {rows} chained", (dg, dbt), (ref["dgamma"], ref["dbeta"]), (r32["dgamma"], r32["dbeta"]), (pg, pb))
    assert not bad, bad


@pytest.mark.parametrize("gamma,beta", SWEEP, ids=[f"gamma{g:.9g}-beta{b:g}" for g, b in SWEEP])
@pytest.mark.parametrize("inputs", ["planted", "chained"])
@pytest.mark.parametrize("R", H.SUMS_ROWS)
def test_head_sweep_of_one_small_gamma(R, inputs, gamma, beta):
    """One line of the sweep table: (R, inputs, gamma, beta) -> ok, the distance of dgamma / dbeta from the fp64 row pass (and of
    the swept channel alone), the bound from the fp32 row pass."""
    c = H.make_case(R, gamma, beta)
    ref, r32 = _head_refs(R, "fp32", gamma, beta)
    if inputs == "planted":
        m = _HeadSums(c, "fp32", torch.from_numpy(ref["dy"]))
        m.plant(ref["dW1"], ref["db1"], 5)
    else:
        m = _HeadSums(c, "fp32")
        ops.head_backward(m.hd)
    dg, dbt, pg, pb, ok = m.sums()
    assert ok == int(H.identity_taken(c)), "the decision is not the header's: |gamma| > 1e-4 and |beta| <= 64 |gamma| on every channel"
    bad = _judge(f"sweep R {R} {inputs} gamma {gamma:.9g} beta {beta:g} ok {ok}", (dg, dbt), (ref["dgamma"], ref["dbeta"]),
                 (r32["dgamma"], r32["dbeta"]), (pg, pb), channel=H.SWEEP_CH)
    assert not bad, bad


@pytest.mark.parametrize("rows", list(H.ROWS))
@pytest.mark.parametrize("gamma", H.FALLBACK_GAMMAS, ids=[f"gamma{g:.9g}" for g in H.FALLBACK_GAMMAS])
@pytest.mark.parametrize("R", H.FALLBACK_ROWS)
def test_head_fallback_is_the_row_pass(R, gamma, rows):
    c = H.make_case(R, gamma, None)
    dy_rows = torch.from_numpy(H.reference(R, rows, True, gamma_ch=gamma)["dy"]).to(H.ROWS[rows])       # dy as stored
    f_rows = c.f.to(H.ROWS[rows])
    ref = H.row_pass(c, f_rows, dy_rows)
    r32 = H.row_pass(c, f_rows.float(), dy_rows.float(), H.F32)
    m = _HeadSums(c, rows, dy_rows)
    m.arena[:m.images[0] * m.images[1]].fill_(1.0e6)                         # dW1 / db1: must not be used
    dg, dbt, pg, pb, ok = m.sums()
    assert ok == 0
    bad = _judge(f"fallback R {R} gamma {gamma:.9g} {rows}", (dg, dbt), ref, r32, (pg, pb))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ FP side
FP_SPECS = ("tiny-FP1", "src-FP2-built", "dense-FP4")       # <34,8,34> Split, <64,16,34> SourceSide, <64,64,64> Dense


def _source_batchnorm(c):
    """gamma, beta, mean, invstd (fp32 tensors) of a BatchNorm whose (a, c) is the case's source affine: invstd a power of two
    and mean dyadic, so gamma = sa / invstd is exact and beta = sc + mean sa is rounded once"""
    ca = c.block.ca
    k = torch.arange(ca)
    invstd = torch.where(k % 2 == 0, 2.0, 0.5)
    mean = 0.25 * ((k % 3).float() - 1.0)
    gamma = c.sa / invstd
    beta = (c.sc.double() + mean.double() * c.sa.double()).float()
    assert torch.equal(gamma * invstd, c.sa)
    return gamma, beta, mean, invstd


def _fp_backward(spec, dsrc_prefill):
    """forward (batch statistics) and backward of a block as tests/test_gpu_fp_blocks.py runs them, the descriptor and the
    un-folded gradient arena kept -> (block, descriptor, dsrc view, what keeps the buffers alive)"""
    m = FB._Block(spec)
    c, b = m.case, m.case.block
    m.forward("train")
    cin = b.ca + b.cb
    n_flat = b.cout * cin + 3 * b.cout
    arena, flat, images, _ = ops.grad_images_alloc(n_flat, DEV)
    o = b.cout * cin
    views = (flat[:o].view(b.cout, cin), flat[o:o + b.cout], flat[o + b.cout:o + 2 * b.cout], flat[o + 2 * b.cout:o + 3 * b.cout])
    m.blk.grads, m.blk.grad_images = views, images
    dsrc = (c.dsrc0 if dsrc_prefill else torch.zeros_like(c.dsrc0)).to(DEV)
    kw = {"dsrc": dsrc, "gather": spec.gather}
    if spec.dskip:
        kw["dskip"] = c.dskip0.to(DEV)
    kw["du_scratch"] = torch.empty(c.R, max(b.ca, c.hs), device=DEV)
    d = m.desc(dy=m.dy, with_grads=True, **kw)
    assert ops.fp_form(d, 3) == FB.FORMS[spec.bwd]
    ops.fp_backward(d)
    torch.cuda.synchronize()
    return m, d, dsrc, (arena, kw)


def _fp_row_sums(c, dsrc, mean, invstd, dtype):
    src = c.src[:, :c.block.ca].to(dtype)
    xhat = (src - mean.to(dtype)) * invstd.to(dtype)
    d = torch.as_tensor(dsrc).to(dtype)
    return (d * xhat).sum(0).numpy(), d.sum(0).numpy()


@pytest.mark.parametrize("fallback", [False, True], ids=["identity", "fallback"])
@pytest.mark.parametrize("spec", [pytest.param(FR.SPECS[i], id=i) for i in FP_SPECS])
def test_fp_side(spec, fallback):
    ref_all, r32_all = FB._ref(spec, "train")
    m, d, dsrc, keep = _fp_backward(spec, dsrc_prefill=not fallback)
    c = m.case
    ca = c.block.ca
    gamma, beta, mean, invstd = _source_batchnorm(c)
    if fallback:
        gamma = gamma.clone()
        gamma[3] = 0.0
        # the row pass reads the dsrc the backward left (zero pre-fill: the network's arena): the yardstick is ITS sums in fp64
        left = dsrc[:, :ca].cpu()
        ref, r32 = _fp_row_sums(c, left, mean, invstd, H.F64), _fp_row_sums(c, left, mean, invstd, H.F32)
        exact = _fp_row_sums(c, ref_all["dsrc"], mean, invstd, H.F64)
        print(f"{spec.id} fallback: the dsrc the backward left, summed in fp64, vs the fp64 reference: dgamma {H.rel(ref[0], exact[0]):.2e}, "
              f"dbeta {H.rel(ref[1], exact[1]):.2e}")
    else:
        ref, r32 = _fp_row_sums(c, ref_all["dsrc"], mean, invstd, H.F64), _fp_row_sums(c, r32_all["dsrc"], mean, invstd, H.F32)
    pg, pb = _prefill(ca, 21), _prefill(ca, 22)
    dgamma, dbeta = torch.from_numpy(pg.copy()).to(DEV), torch.from_numpy(pb.copy()).to(DEV)
    ok = torch.full((1,), OK_SENT, dtype=torch.int32, device=DEV)
    ops.fp_bn_sums(d, gamma.to(DEV), beta.to(DEV), mean.to(DEV), invstd.to(DEV), dgamma, dbeta, ok)
    torch.cuda.synchronize()
    assert int(ok.item()) == (0 if fallback else 1)
    got = (dgamma.cpu().numpy().astype(np.float64) - pg, dbeta.cpu().numpy().astype(np.float64) - pb)
    bad = _judge(f"{spec.id} {'fallback' if fallback else 'identity'}", got, ref, r32, (pg, pb))
    assert not bad, bad


def test_fp_side_refuses_bad_arguments():
    """a missing pointer, and ca > 64 on an otherwise valid descriptor: SN2_EINVAL, nothing written"""
    m, d, dsrc, keep = _fp_backward(FR.SPECS["tiny-FP1"], dsrc_prefill=True)
    ca = m.case.block.ca
    gamma, beta, mean, invstd = (t.to(DEV) for t in _source_batchnorm(m.case))
    dgamma, dbeta = torch.full((ca,), 3.5, device=DEV), torch.full((ca,), -2.5, device=DEV)
    ok = torch.full((1,), OK_SENT, dtype=torch.int32, device=DEV)
    for field in ("dsrc", "knn_idx"):
        saved = getattr(d, field)
        setattr(d, field, None)
        with pytest.raises(_lib.StrataHipError, match="SN2_EINVAL"):
            ops.fp_bn_sums(d, gamma, beta, mean, invstd, dgamma, dbeta, ok)
        setattr(d, field, saved)
    # 68 interpolated channels: a descriptor that passes every other check
    B, Rp, S, CA, CB, CO = 2, 40, 5, 68, 4, 16
    lin, bn = torch.nn.Linear(CA + CB, CO).to(DEV), torch.nn.BatchNorm1d(CO).to(DEV)
    blk = ops.BlockBuffers(lin, bn)
    arena, flat, images, _ = ops.grad_images_alloc(CO * (CA + CB) + 3 * CO, DEV)
    o = CO * (CA + CB)
    blk.grads = (flat[:o].view(CO, CA + CB), flat[o:o + CO], flat[o + CO:o + 2 * CO], flat[o + 2 * CO:o + 3 * CO])
    blk.grad_images = images
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, S, (B * Rp, 3), generator=g, dtype=torch.int32).to(DEV)
    w = (torch.rand(B * Rp, 3, generator=g) + 0.2).to(DEV)
    wide = ops.fp_desc(blk, B, Rp, S, CA, CB, torch.randn(B * S, CA, device=DEV), torch.zeros(B * Rp, CO, device=DEV), knn=(idx, w),
                       skip=torch.randn(B * Rp, CB, device=DEV), dy=torch.zeros(B * Rp, CO, device=DEV),
                       dsrc=torch.zeros(B * S, CA, device=DEV), with_grads=True)
    v = [torch.ones(CA, device=DEV) for _ in range(4)]
    wg, wb = torch.full((CA,), 3.5, device=DEV), torch.full((CA,), -2.5, device=DEV)
    with pytest.raises(_lib.StrataHipError, match="SN2_EINVAL"):
        ops.fp_bn_sums(wide, v[0], v[1], v[2], v[3], wg, wb, ok)
    torch.cuda.synchronize()
    assert bool((dgamma == 3.5).all()) and bool((dbeta == -2.5).all()) and bool((wg == 3.5).all()) and bool((wb == -2.5).all())
    assert int(ok.item()) == OK_SENT
