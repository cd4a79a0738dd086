"""The dense-row blocks alone (csrc/fp.hip, csrc/fp_rows.h, csrc/interp_index.hip through hip_ops.fp_desc / fp_forward /
fp_backward) against fp64: every instantiation -- SA3 <32,3,64>, FP3 <64,32,64>, FP2 <64,16,34>, FP1 <34,8,34>, the 3sa blocks
<64,3,64> and <64,64,64> -- in every kernel form it can take (Split, SourceSide, Dense; forward and backward), both
BatchNorm-sum kernels (and both grids of the larger one), both transposed-interpolation kernels, the eval exception and the
frozen mode, at the smallest shapes that reach them.  tests/_fp_block_ref.py builds the cases and the reference;
tests/test_fp_block_ref_host.py proves on the CPU what this file rests on (the reference against finite differences, the planted
lists, the form every case takes, the edge inputs, the precision of the fp32 restatement).

What is looked at: `ops.fp_form` before every launch; h, a, c, mean, invstd and the running statistics of a forward in modes 1, 0
and BN_FROZEN_KEEP; after a backward (batch statistics, and frozen after a frozen forward) dW, db (folded from a zeroed gradient
arena), dgamma, dbeta (from the call's own row pass, or left alone to the bit behind a `bn_sums_done` word), dsrc and dskip as
output minus a non-zero pre-fill (ACCUMULATED outputs), or the rows of du_scratch where the caller transposes the interpolation
itself.  Exact: 64 sentinel rows behind h, dsrc, dskip and du_scratch; source rows on no list and the padding columns of dsrc; the
input gradient of a zero column of W; the dead channel's activations, its row of dW and its db.

Tolerances (none invented here; every figure is printed next to its bound):
  * h, a, c, mean, invstd, fp32 operands: 1e-4 of the array's largest magnitude (a, c, invstd: of the live channels', and the dead
    channel's 1 / sqrt(eps) to 1e-4 of itself); running statistics: atol 1e-5, rtol 1e-4;
  * gradients, fp32 operands: distance from fp64 relative to the tensor's largest element at most max(1e-5, 8 e32), never above
    1e-3; e32 is the same distance of the reference restated in fp32 on the CPU (for dsrc / dskip including the rounding of
    pre-fill + gradient);
  * bf16 operands (Split only; reference with the same operand rounding): 2e-2 on gradients, 1e-3 on outputs.
Every live pre-activation of a case keeps 2^-15 from zero (tests/_fp_block_ref.py: _separate), so the kernel's ReLU mask is the
reference's -- asserted after every forward.  Without that a first run of this file had one flipped mask in three of the 65 538-row
cases: that row's input gradient off by 3.5e-2 of the tensor's largest element and db by 3.5e-3, every other figure at 1e-6.

Measured on an MI355X ("Dense-row blocks alone"; 178 tests in about 15 s, the slowest 2.9 s), distance from
fp64 relative to the largest element, backward form by form:
  fp32 operands   parameter gradients        input gradients (dsrc / du / dskip)   e32 (parameters; inputs)
    Split         1.5e-8 ... 3.7e-6          9.5e-8 ... 1.1e-6                     6.6e-8 ... 3.9e-6; 1.4e-7 ... 1.2e-6
    SourceSide    2.6e-8 ... 6.0e-6          1.2e-7 ... 7.6e-7                     8.5e-8 ... 9.0e-6; 3.6e-7 ... 1.3e-6
    Dense         2.1e-8 ... 5.5e-6          1.6e-7 ... 2.1e-6                     8.9e-8 ... 5.8e-6; 1.6e-7 ... 2.9e-6
  the largest error is 17 % of its bound (db of the 72-plot case); kernel / e32 is at most 3.9 where the error is above 1e-6, and
  7.0 on one tensor below it (dbeta at 65 536 rows, 7.5e-7 against e32 = 1.1e-7: the bound there is the 1e-5 floor);
  the largest figure, 6.0e-6, is db over 262 146 rows (e32 9.0e-6)
  bf16 operands   4e-8 ... 7.5e-3 (parameter gradients; db sums the rounded d pre-activations), 7e-8 ... 7.1e-4 (inputs)
  h 1.9e-7 ... 4.3e-7 (bf16 operands 7e-8 ... 1.5e-7 against the reference with the same rounding); a, c, mean, invstd
  5e-8 ... 3.3e-7; running statistics 4e-8 (mean), 1.5e-7 (variance)
Two deliberately wrong kernels, built once and not kept: fp_bwd_split_kernel without the dskip rows of a last partial workgroup
fails `dskip` of tiny-FP2 / -FP3 / -FP4 and seg-FP2 (0.29 ... 0.49); the long gather taken from 127 S rows on with its list offset
one entry low fails `dsrc` of densefp2-171 and densefp1-171 (2.4e-2 ... 2.6e-2) while densefp2-170 passes.
"""
import contextlib

import numpy as np
import pytest
import torch

import _fp_block_ref as R
from stratanet2_vegetation_coverage_maps_amd import _lib, hip_ops as ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATOM, BOUND, FACTOR = 1e-5, 1e-3, 8
OUT_TOL, BF16_OUT, BF16_GRAD = 1e-4, 1e-3, 2e-2
STAT_ATOL, STAT_RTOL = 1e-5, 1e-4
GUARD = 64
H_SENT, DU_SENT, GRAD_SENT = -777.25, 333.5, 555.5
TRAINING = {"train": 1, "frozen": _lib.BN_FROZEN_KEEP, "eval": 0}
FORMS = {R.SPLIT: ops.FP_FORM_SPLIT, R.SOURCE_SIDE: ops.FP_FORM_SOURCE_SIDE, R.DENSE: ops.FP_FORM_DENSE}
BN_DONE_SPECS = ("tiny-FP1", "tiny-FP3", "tiny-GSA", "seg-FP2", "src-FP1-built", "src-FP2-perm", "dense-SA3", "densefp2-171",
                 "dense-FP4-nogather", "edge65537-FP1-rows")               # Split, SourceSide and Dense, each more than once

_CACHE = {}


def _ref(spec, mode):
    """(fp64 reference, its fp32 restatement or None with bf16 operands) -- computed once per process, never changed"""
    key = (R.data_key(spec), spec.bf16, mode)
    if key not in _CACHE:
        c = R.make_case(spec)
        _CACHE[key] = (R.reference(c, mode, bf16=spec.bf16), None if spec.bf16 else R.reference_fp32(c, mode))
    return _CACHE[key]


@contextlib.contextmanager
def _source_side(spec):
    saved = ops.SOURCE_SIDE
    ops.SOURCE_SIDE = spec.source_side
    try:
        yield
    finally:
        ops.SOURCE_SIDE = saved


def _guarded(t, fill):
    """(tensor with GUARD sentinel rows appended, the view of its first rows)"""
    full = torch.cat([t, torch.full((GUARD, t.shape[1]), fill, dtype=t.dtype)]).to(DEV)
    return full, full[:t.shape[0]]


class _Block:
    """A case on the device."""

    def __init__(self, spec):
        self.spec, self.case = spec, R.make_case(spec)
        c, b = self.case, self.case.block
        lin, bn = torch.nn.Linear(b.ca + b.cb, b.cout).to(DEV), torch.nn.BatchNorm1d(b.cout).to(DEV)
        with torch.no_grad():
            lin.weight.copy_(c.W), lin.bias.copy_(c.b), bn.weight.copy_(c.gamma), bn.bias.copy_(c.beta)
            bn.running_mean.copy_(c.rm), bn.running_var.copy_(c.rv)
        self.blk = ops.BlockBuffers(lin, bn)
        self.blk.mma_bf16 = spec.bf16
        self.src, self.skip_rows, self.dy = c.src.to(DEV), c.skip.to(DEV), c.dy.to(DEV)
        self.affine = None if c.sa is None else (c.sa.to(DEV), c.sc.to(DEV))
        self.knn = None if c.idx is None else (c.idx.to(DEV), c.w.to(DEV))
        self.h_full, self.h = _guarded(torch.full((c.R, c.hs), H_SENT), H_SENT)

    def desc(self, **kw):
        c, b = self.case, self.case.block
        with _source_side(self.spec):
            return ops.fp_desc(self.blk, c.B, c.Rp, c.S, b.ca, b.cb, self.src, self.h, src_affine=self.affine, knn=self.knn,
                               skip=self.skip_rows[:, 0:b.cb], **kw)

    def statistics(self):
        bn = self.blk.bn
        return bn.running_mean.cpu().numpy().copy(), bn.running_var.cpu().numpy().copy(), int(bn.num_batches_tracked)

    def forward(self, mode):
        self.blk.frozen = mode == "frozen"
        d = self.desc()
        want = self.spec.fwd_eval if mode == "eval" else self.spec.fwd
        assert ops.fp_form(d, TRAINING[mode]) == FORMS[want], (self.spec.id, mode, ops.fp_form(d, TRAINING[mode]))
        ops.fp_forward(d, TRAINING[mode])
        torch.cuda.synchronize()

    def backward(self, bn_done=None):
        """-> {name: numpy}: dW, db, dgamma, dbeta after the fold; dsrc, dskip, du with their sentinel rows; "bn_bits": dgamma /
        dbeta as the call left them (before the fold)"""
        spec, c, b = self.spec, self.case, self.case.block
        cin = b.ca + b.cb
        n_flat = b.cout * cin + 3 * b.cout
        arena, flat, images, _ = ops.grad_images_alloc(n_flat, DEV)
        o = b.cout * cin
        views = (flat[:o].view(b.cout, cin), flat[o:o + b.cout], flat[o + b.cout:o + 2 * b.cout], flat[o + 2 * b.cout:o + 3 * b.cout])
        self.blk.grads, self.blk.grad_images = views, images
        kw, done = {}, None
        if bn_done is not None:
            views[2].copy_(torch.from_numpy(bn_done[0]).to(DEV)), views[3].copy_(torch.from_numpy(bn_done[1]).to(DEV))
            done = torch.ones(1, dtype=torch.int32, device=DEV)
            kw["bn_sums_done"] = done
        dsrc_full, dsrc = _guarded(c.dsrc0, GRAD_SENT)
        kw["dsrc"] = dsrc
        dskip_full = None
        if spec.dskip:
            dskip_full, kw["dskip"] = _guarded(c.dskip0, GRAD_SENT)
        du_full = None
        if b.knn:
            du_full, kw["du_scratch"] = _guarded(torch.full((c.R, max(b.ca, c.hs)), DU_SENT), DU_SENT)
            kw["gather"] = spec.gather
            if spec.variant == "morton":
                kw["interp_index"] = ops.interp_index(self.knn, c.B, c.Rp, c.S, src_pos=c.src_pos.to(DEV))
            elif spec.variant == "perm":
                perm = c.row_perm.to(DEV)
                kw["interp_index"] = ops.interp_index(self.knn, c.B, c.Rp, c.S, row_perm=perm)
                kw["row_perm"] = perm
        d = self.desc(dy=self.dy, with_grads=True, **kw)
        assert ops.fp_form(d, 3) == FORMS[spec.bwd], (spec.id, ops.fp_form(d, 3))
        if spec.variant == "perm":
            assert d.row_perm
        assert d.scatter_ready == (-1 if (b.knn and not spec.gather) else 1 if spec.variant in ("morton", "perm") else 0)
        ops.fp_backward(d)
        torch.cuda.synchronize()
        bn_bits = (views[2].cpu().numpy().copy(), views[3].cpu().numpy().copy())
        ops.grad_reduce(arena, n_flat, images)
        torch.cuda.synchronize()
        got = {n: v.detach().cpu().numpy().copy() for n, v in zip(("dW", "db", "dgamma", "dbeta"), views)}
        got.update(bn_bits=bn_bits, dsrc=dsrc_full.cpu().numpy(), dskip=None if dskip_full is None else dskip_full.cpu().numpy(),
                   du=None if du_full is None else du_full.cpu().numpy(), h=self.h_full.cpu().numpy())
        return got


def _rel(a, b, scale):
    return float(np.abs(np.asarray(a, np.float64) - b).max()) / scale


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32), np.ascontiguousarray(b, np.float32).view(np.int32))


def _check_forward(m, ref, before, mode, tag):
    c, b, bf16 = m.case, m.case.block, m.spec.bf16
    tol = BF16_OUT if bf16 else OUT_TOL
    hf = m.h_full.cpu().numpy()
    assert _same_bits(hf[c.R:], np.full((GUARD, c.hs), H_SENT, np.float32)), "rows behind h were written"
    h = hf[:c.R, :b.cout]
    assert np.isfinite(h).all()
    live = np.arange(b.cout) != R.DEAD
    aux = m.blk.aux.cpu().numpy()
    figures, bad = [], []
    e = _rel(h, ref["h"], np.abs(ref["h"]).max())
    figures.append(f"h {e:.2e}")
    if not e < tol:
        bad.append(("h", e))
    for i, n in enumerate(("a", "c", "mean", "invstd")):
        e = _rel(aux[i][live], ref[n][live], np.abs(ref[n][live]).max())
        e_dead = abs(float(aux[i][R.DEAD]) - ref[n][R.DEAD]) / max(abs(ref[n][R.DEAD]), 1e-30) if ref[n][R.DEAD] != 0 else abs(float(aux[i][R.DEAD]))
        figures.append(f"{n} {e:.2e} (dead channel {e_dead:.1e})")
        if not (e < tol and e_dead < tol):
            bad.append((n, e, e_dead))
    print(f"{tag}: vs fp64, of the largest magnitude (bound {tol:.0e}): " + ", ".join(figures))
    assert not bad, bad
    assert not h[:, R.DEAD].any(), "the dead channel is not zero on every row"
    flipped = int(((h > 0) != ref["mask"]).sum())
    assert flipped == 0, f"{flipped} ReLU masks differ from the reference's (every pre-activation keeps 2^-15 from zero)"
    rm, rv, nbt = m.statistics()
    if mode == "train":
        print(f"{tag}: running mean / var vs fp64 {np.abs(rm - ref['running_mean']).max():.1e} / {np.abs(rv - ref['running_var']).max():.1e} "
              f"(atol {STAT_ATOL:.0e}, rtol {STAT_RTOL:.0e})")
        np.testing.assert_allclose(rm, ref["running_mean"], atol=STAT_ATOL, rtol=STAT_RTOL)
        np.testing.assert_allclose(rv, ref["running_var"], atol=STAT_ATOL, rtol=STAT_RTOL)
        assert nbt == before[2] + 1
    else:
        assert _same_bits(rm, before[0]) and _same_bits(rv, before[1]) and nbt == before[2]


def _check_backward(m, got, ref, r32, tag, bn_done=None):
    """Exact properties first, then every figure is printed, then all are asserted."""
    spec, c, b = m.spec, m.case, m.case.block
    dsrc0, dskip0 = c.dsrc0.numpy(), c.dskip0.numpy()
    # ---- sentinels and what must keep its bits
    assert _same_bits(got["h"][c.R:], np.full((GUARD, c.hs), H_SENT, np.float32)), "rows behind h were written"
    assert _same_bits(got["dsrc"][c.n_src:], np.full((GUARD, b.src_stride), GRAD_SENT, np.float32)), "rows behind dsrc were written"
    dsrc = got["dsrc"][:c.n_src]
    assert _same_bits(dsrc[:, b.ca:], dsrc0[:, b.ca:]), "padding columns of dsrc were written"
    for n in ("dW", "db", "dgamma", "dbeta", "dsrc"):
        assert np.isfinite(got[n]).all(), n
    names = ["dW", "db", "dgamma", "dbeta"]
    parts = {n: (got[n], ref[n], None if r32 is None else r32[n]) for n in names}
    if b.knn:
        du = got["du"]
        assert _same_bits(du[c.R:], np.full((GUARD, du.shape[1]), DU_SENT, np.float32)), "rows behind du_scratch were written"
    if b.knn and not spec.gather:
        assert _same_bits(dsrc, dsrc0), "scatter_ready < 0: dsrc must be left alone"
        rows = du[:c.R].reshape(-1)[:c.R * b.ca].reshape(c.R, b.ca)                    # (R, ca) rows, back to back
        assert np.isfinite(rows).all()
        assert not rows[:, R.ZERO_COL].any(), "the zero column's input gradient is not exactly 0"
        parts["du"] = (rows, ref["du"], r32["du"])
        names.append("du")
    else:
        unlisted = R.unlisted_sources(c)
        assert _same_bits(dsrc[unlisted], dsrc0[unlisted]), "a source row on no list moved"
        assert _same_bits(dsrc[:, R.ZERO_COL], dsrc0[:, R.ZERO_COL]), "the zero column's input gradient is not exactly 0"
        p32 = None if r32 is None else (dsrc0[:, :b.ca] + r32["dsrc"]).astype(np.float64) - dsrc0[:, :b.ca]
        parts["dsrc"] = (dsrc[:, :b.ca].astype(np.float64) - dsrc0[:, :b.ca], ref["dsrc"], p32)
        names.append("dsrc")
    if spec.dskip:
        assert _same_bits(got["dskip"][c.R:], np.full((GUARD, b.cb), GRAD_SENT, np.float32)), "rows behind dskip were written"
        dskip = got["dskip"][:c.R]
        assert np.isfinite(dskip).all()
        assert _same_bits(dskip[:, 1], dskip0[:, 1]), "the zero column's skip gradient is not exactly 0"
        p32 = None if r32 is None else (dskip0 + r32["dskip"]).astype(np.float64) - dskip0
        parts["dskip"] = (dskip.astype(np.float64) - dskip0, ref["dskip"], p32)
        names.append("dskip")
    assert not got["dW"][R.DEAD].any() and got["db"][R.DEAD] == 0.0, "the dead channel has a weight or bias gradient"
    if bn_done is not None:
        for k, n in enumerate(("dgamma", "dbeta")):
            assert _same_bits(got["bn_bits"][k], bn_done[k]) and _same_bits(got[n], bn_done[k]), f"{n} changed behind bn_sums_done"
    # ---- distances
    bad = []
    for n in names:
        g, r, r32n = parts[n]
        scale = np.abs(r).max()
        assert scale > 0, n
        err = _rel(g, r, scale)
        if spec.bf16:
            bound, note = BF16_GRAD, "bf16"
        else:
            e32 = _rel(r32n, r, scale)
            bound, note = min(max(ATOM, FACTOR * e32), BOUND), f"e32 {e32:.2e}"
        print(f"{tag} {n}: vs fp64 {err:.2e}, bound {bound:.2e} ({note})")
        if not err <= bound:
            bad.append((n, err, bound))
    assert not bad, bad


FORWARD = [pytest.param(s, id=s.id) for s in R.forward_specs()]
BACKWARD = [pytest.param(s, id=s.id) for s in R.SPECS.values()]


@pytest.mark.parametrize("mode", ("train", "eval", "frozen"))
@pytest.mark.parametrize("spec", FORWARD)
def test_forward(spec, mode):
    ref = _ref(spec, "frozen" if mode == "eval" else mode)[0]              # an eval pass computes what a frozen one does
    m = _Block(spec)
    before = m.statistics()
    m.forward(mode)
    _check_forward(m, ref, before, mode, f"{spec.id} {mode}")


@pytest.mark.parametrize("mode", ("train", "frozen"))
@pytest.mark.parametrize("spec", BACKWARD)
def test_backward(spec, mode):
    ref, r32 = _ref(spec, mode)
    m = _Block(spec)
    m.forward(mode)
    got = m.backward()
    _check_backward(m, got, ref, r32, f"{spec.id} {mode}")


@pytest.mark.parametrize("mode", ("train", "frozen"))
@pytest.mark.parametrize("spec", [pytest.param(R.SPECS[i], id=i) for i in BN_DONE_SPECS])
def test_backward_behind_a_bn_sums_done_word(spec, mode):
    """dgamma / dbeta handed in complete (the fp64 reference's, rounded to fp32) behind a `bn_sums_done` word: the call launches
    no row pass for them, leaves both to the bit, and still produces dW, db, dsrc and dskip"""
    ref, r32 = _ref(spec, mode)
    m = _Block(spec)
    m.forward(mode)
    done = (ref["dgamma"].astype(np.float32), ref["dbeta"].astype(np.float32))
    got = m.backward(bn_done=done)
    _check_backward(m, got, ref, r32, f"{spec.id} {mode} bn_sums_done", bn_done=done)
