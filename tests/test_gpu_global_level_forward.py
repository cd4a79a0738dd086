"""The forward of the global level in one launch (csrc/global_level.hip: sn2_global_level_forward) and the small kernels around
its pool (csrc/misc.hip: sn2_plot_max_forward, sn2_plot_max_backward, sn2_global_pool_backward), each called alone through
hip_ops against an fp64 restatement.  tests/_global_level_ref.py builds the cases and the references;
tests/test_global_level_ref_host.py proves on the CPU what this file rests on (the reference against torch's fp64 modules, the
ReLU margin, the planted ties and where they sit in the kernel, the dead and the offset channel, the precision of the fp32
restatement, the share of undecided maxima).

Shapes (B, M2) of the level: (1, 40) one partial block, three idle groups, a workgroup exchanging with itself; (3, 64) exactly one
block; (2, 65) a second block of one row; (2, 256) four full blocks, the last shape of the register path of the max; (2, 257) a
second trip with one busy group and one row, the memory path of the max with two unrolled steps and the tail; (1, 625) ten
blocks, three trips; (28, 64) the plot limit and the LDS budget; (29, 40) the separate launches only.

  (a) the one launch against fp64 in training mode; (b) the five launches sn2_fp_forward(sa3), sn2_plot_max_forward,
  sn2_fp_forward(fp3) against the same reference in modes train, BN_FROZEN_KEEP and eval, and in train mode the one launch's
  h_sa3 equal to theirs bit for bit (the header: "the same staging, tiles"); (c) the entry point's refusals before any device
  work; (d) / (e) the plot max forward / backward alone in exact arithmetic at C = 64 and C = 34; (f) the pool backward alone.

Tolerances (none invented here; every figure is printed next to its bound and next to the fp32 restatement's figure):
  * h_sa3, h3, x3, a, c, mean, invstd: 1e-4 of the array's largest magnitude (a, c, mean, invstd: of the live channels', the dead
    channel's invstd to 1e-4 of itself); running statistics: atol 1e-5, rtol 1e-4 -- tests/test_gpu_fp_blocks.py's;
  * the row of a plot's max: the fp64 first maximum wherever its gap to the best non-identical row exceeds the decision bound
    2 * 1e-4 * max |a h + c| (two values the output tolerance cannot tell apart may swap), otherwise a row inside that bound;
    exactly the lowest zero row where the extremum is an exact zero of h (every negative-gamma channel with a zero row, and
    the dead channel: x3 == c to the bit); the planted copy q never; at most 5 % of the (plot, channel) pairs undecided;
  * pool backward: distance from fp64 relative to the largest element at most max(1e-5, 8 e32), never above 1e-3, e32 the fp32
    CPU restatement's distance (ATOM, FACTOR, BOUND of tests/test_gpu_fp_blocks.py); dy exact.

Measured on an MI355X ("Global level forward alone"; 70 tests in 1.0 ... 1.7 s, the slowest 0.6 s: the first
launch of the process; the host file's 77 tests in 2.3 s), distance from fp64 relative to the array's largest magnitude, the
fp32 CPU restatement's figure in brackets:
  one launch, seven shapes   h_sa3 5.0e-8 ... 2.3e-7 [the same]   x3 1.6e-7 ... 2.1e-6 [<= 2.2e-7]   h3 2.7e-7 ... 5.0e-7 [<= 5.4e-7]
    SA3  a <= 8.1e-7, c <= 4.0e-6, mean <= 3.7e-8, invstd <= 1.1e-6 [all <= 1.4e-7]
    FP3  a <= 3.1e-6, c <= 1.5e-5, mean <= 3.1e-7, invstd <= 4.1e-6 [a <= 1.3e-6, c <= 6.9e-7, invstd <= 1.9e-6]
    the dead channel's invstd 5.4e-8 of itself; running statistics at most 0.63 % of atol + rtol |reference|
    the largest error is 15 % of its bound: FP3's c at (1, 625), 1.5e-5, 22 times the restatement's 6.9e-7, not in the offset channel
    the offset channel relative to itself: invstd 9.6e-8 ... 3.9e-6, c 4.2e-8 ... 4.0e-6 [4.4e-9 ... 2.9e-7]: 4 % of the bound
  five launches   train: x3 <= 1.0e-6, FP3's c <= 8.6e-6; frozen and eval: every figure <= 3.8e-7
  h_sa3 of the one launch is the separate launch's, bit for bit, at all seven shapes
  undecided maxima per case   0 / 0.52 / 0 / 0.78 / 0.78 / 0 / 0.33 % of the (plot, channel) pairs, (29, 40) 0.48 %, on the running
    statistics at most 1.56 % (cap 5 %); 22 % of the pairs have their extremum on an exact zero of h
  (3, 64) under a one-sweep wait limit: 2 of 3 workgroups gave up, the same bits
  pool backward   dx 2.8e-8 ... 1.8e-7, dgamma 4.8e-8 ... 2.2e-7, dbeta 4.7e-8 ... 1.9e-7 [the same range]; at most 2.2 % of the
    bound, kernel / e32 <= 3.3
Two deliberately wrong kernels, built once and not kept: `i > bi` for `i < bi` in the group reduction of the register path fails
test_one_launch_against_fp64[2-65] and [2-256] while the existing tests of the level pass; the memory path of the max without its
16-row tail fails [3-64] (the repair under the wait limit), [2-257] and [1-625] -- two existing whole-network tests at M2 = 625
fail on it too.
"""
import numpy as np
import pytest
import torch

import _global_level_ref as G
from test_gpu_global_level_backward import _Level
from stratanet2_vegetation_coverage_maps_amd import _lib, hip_ops as ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATOM, BOUND, FACTOR = 1e-5, 1e-3, 8                   # tests/test_gpu_fp_blocks.py
GUARD = 64
H_SENT, X_SENT, ARG_SENT, AUX_SENT, NBT0 = -777.25, 555.5, -12345, 333.5, 5
TRAINING = {"train": 1, "frozen": _lib.BN_FROZEN_KEEP, "eval": 0}
ARRAYS = ("h_sa3", "h3", "x3", "arg3") + tuple(f"{n}.{s}" for n, _, _ in G.BLOCKS for s in G.STATS + ("running_mean", "running_var"))

_CACHE = {}


def _ref(B, M2, mode):
    """(fp64 reference, its fp32 restatement, the fp64 decisions of the max) -- computed once per process, never changed"""
    mode = "frozen" if mode == "eval" else mode                               # an eval pass computes what a frozen one does
    if (B, M2, mode) not in _CACHE:
        c = G.make_case(B, M2)
        ref = G.reference(c, mode)
        _CACHE[(B, M2, mode)] = (ref, G.reference_fp32(c, mode), G.decisions(c, ref))
    return _CACHE[(B, M2, mode)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


class _Fwd(_Level):
    """A case on the device: the descriptors of _Level (sa3(), fp3(), FP3's table) over guarded, sentinel-filled outputs."""

    def __init__(self, c):                                                    # (not _Level's: that one runs the forward itself)
        self.case, self.B, self.M2 = c, c.B, c.M2
        B, R = c.B, c.R
        self.x2, self.pos2 = c.x2.to(DEV), c.pos2.to(DEV)
        self.blk = {}
        for n, _, cin in G.BLOCKS:
            p = c.blk[n]
            lin, bn = torch.nn.Linear(cin, 64).to(DEV), torch.nn.BatchNorm1d(64).to(DEV)
            with torch.no_grad():
                lin.weight.copy_(p["W"]), lin.bias.copy_(p["b"]), bn.weight.copy_(p["gamma"]), bn.bias.copy_(p["beta"])
            self.blk[n] = ops.BlockBuffers(lin, bn)
        # FP3's table, as _Level builds it: k = 1 from the plot's one source at the origin (weight 1 / d^2; 1 / 1e-16 at the origin)
        idx = torch.zeros(R, 3, dtype=torch.int32, device=DEV)
        w = torch.zeros(R, 3, device=DEV)
        w[:, 0] = 1.0 / self.pos2[:, 0:3].square().sum(1).clamp_min(1e-16)
        assert float(w.max()) > 9e15
        self.knn3 = (idx, w)
        self.full = {"h_sa3": torch.empty(R + GUARD, 64, device=DEV), "h3": torch.empty(R + GUARD, 64, device=DEV),
                     "x3": torch.empty(B + 1, 64, device=DEV), "arg3": torch.empty(B + 1, 64, dtype=torch.int32, device=DEV)}
        self.h_sa3, self.h3 = self.full["h_sa3"][:R], self.full["h3"][:R]
        self.x3, self.arg3 = self.full["x3"][:B], self.full["arg3"][:B]
        self.reset()

    def reset(self):
        """sentinels in every output, the running statistics and counters back at their non-trivial start"""
        for k, v in (("h_sa3", H_SENT), ("h3", H_SENT), ("x3", X_SENT), ("arg3", ARG_SENT)):
            self.full[k].fill_(v)
        with torch.no_grad():
            for n, _, _ in G.BLOCKS:
                bn, p = self.blk[n].bn, self.case.blk[n]
                bn.running_mean.copy_(p["rm"]), bn.running_var.copy_(p["rv"]), bn.num_batches_tracked.fill_(NBT0)
                self.blk[n].aux.fill_(AUX_SENT)
                self.blk[n].frozen = False
        torch.cuda.synchronize()

    def one_launch(self):
        ops.global_level_forward(self.sa3(), self.fp3(), self.x3, self.arg3, owner=self)

    def five_launches(self, mode):
        for n, _, _ in G.BLOCKS:
            self.blk[n].frozen = mode == "frozen"
        ops.fp_forward(self.sa3(), TRAINING[mode])
        x3, arg3 = ops.plot_max_forward(self.h_sa3, self.blk["sa3"].aux[0], self.blk["sa3"].aux[1], self.B, self.M2, 64)
        self.x3.copy_(x3), self.arg3.copy_(arg3)
        ops.fp_forward(self.fp3(), TRAINING[mode])

    def outputs(self):
        """-> {name: numpy} with the guard rows; "batches": the two counters"""
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in self.full.items()}
        for n, _, _ in G.BLOCKS:
            aux, bn = self.blk[n].aux.cpu().numpy(), self.blk[n].bn
            out.update({f"{n}.{s}": aux[i].copy() for i, s in enumerate(G.STATS)})
            out[f"{n}.running_mean"], out[f"{n}.running_var"] = bn.running_mean.cpu().numpy().copy(), bn.running_var.cpu().numpy().copy()
            out[f"{n}.batches"] = int(bn.num_batches_tracked)
        return out

    def forward_gave_up(self):
        return int(self.__dict__["_gl_ws"][0][1][1].item())                   # ctl[1] of the forward's exchange area


def _assert_same_outputs(a, b, what):
    for k in ARRAYS:
        assert _same_bits(a[k], b[k]), f"{what}: {k} differs"
    for n, _, _ in G.BLOCKS:
        assert a[f"{n}.batches"] == b[f"{n}.batches"], what


def _check(lv, out, mode, tag):
    """Every assertion of (a) and (b) on one set of outputs: exact properties first, then every figure is printed, then asserted."""
    c, B, M2, R = lv.case, lv.B, lv.M2, lv.case.R
    ref, r32, d = _ref(B, M2, mode)
    # ---- sentinels, counters, running statistics
    for k, v in (("h_sa3", H_SENT), ("h3", H_SENT)):
        assert _same_bits(out[k][R:], np.full((GUARD, 64), v, np.float32)), f"rows behind {k} were written"
    assert _same_bits(out["x3"][B:], np.full((1, 64), X_SENT, np.float32)), "words behind x3 were written"
    assert np.array_equal(out["arg3"][B:], np.full((1, 64), ARG_SENT, np.int32)), "words behind arg3 were written"
    got = dict(out, h_sa3=out["h_sa3"][:R], h3=out["h3"][:R], x3=out["x3"][:B], arg3=out["arg3"][:B])
    for k in ARRAYS:
        assert np.isfinite(got[k]).all(), k
    for n, _, _ in G.BLOCKS:
        assert got[f"{n}.batches"] == NBT0 + ref["batches"], f"{n}: num_batches_tracked moved by {got[f'{n}.batches'] - NBT0}"
        if mode != "train":
            assert _same_bits(got[f"{n}.running_mean"], c.blk[n]["rm"].numpy()) and _same_bits(got[f"{n}.running_var"], c.blk[n]["rv"].numpy())
    # ---- the dead channel and the ReLU masks
    for k in ("h_sa3", "h3"):
        assert not got[k][:, G.DEAD].any(), f"{k}: the dead channel is not zero on every row"
        flipped = int(((got[k] > 0) != (ref[k] > 0)).sum())
        assert flipped == 0, f"{k}: {flipped} ReLU masks differ from the reference's (every pre-activation keeps 2^-15 from zero)"
    c_dev, a_dev = got["sa3.c"], got["sa3.a"]
    x3, arg3 = got["x3"], got["arg3"]
    assert _same_bits(x3[:, G.DEAD], np.full(B, c_dev[G.DEAD], np.float32)) and not arg3[:, G.DEAD].any()
    # ---- the rows of the max
    assert arg3.min() >= 0 and arg3.max() < M2
    assert _same_bits(x3[d.zero], np.broadcast_to(c_dev, (B, 64))[d.zero]), "an extremum at an exact zero of h is not c to the bit"
    assert np.array_equal(arg3[d.zero], d.first[d.zero]), "an extremum at an exact zero of h is not at the lowest zero row"
    y = ref["y"].reshape(B, M2, 64)
    wrong = [(int(b), int(ch), int(arg3[b, ch]), int(d.first[b, ch]), float(d.gap[b, ch]), float(y[b, arg3[b, ch], ch]), float(d.best[b, ch]),
              float(got["h_sa3"].reshape(B, M2, 64)[b, arg3[b, ch], ch]), float(got["h_sa3"].reshape(B, M2, 64)[b, d.first[b, ch], ch]))
             for b, ch in zip(*np.nonzero(d.decided & (arg3 != d.first)))]
    assert not wrong, f"decided maxima that name another row than the fp64 first maximum (plot, channel, row, fp64 row, gap, fp64 y of " \
                      f"either, device h of either): {wrong[:8]}; plants {c.plants[:8]}"
    named = np.take_along_axis(y, arg3[:, None, :].astype(np.int64), 1)[:, 0, :]
    assert (named >= d.best - d.bound).all(), "an undecided maximum names a row outside the decision bound"
    for b, (p, q, _, _) in enumerate(c.plants):
        assert not (arg3[b] == q).any(), f"plot {b}: the copy q = {q} of row p = {p} was named"
        assert int(d.planted[b].sum()) >= 4 and (arg3[b][d.planted[b]] == p).all()
    # (x3 is the value of the row it names, from the device's own h, a, c: an fma of fp32 operands, exact in fp64 up to the last rounding)
    own = a_dev.astype(np.float64) * np.take_along_axis(got["h_sa3"].reshape(B, M2, 64), arg3[:, None, :].astype(np.int64), 1)[:, 0, :] + c_dev
    assert np.abs(x3 - own).max() <= 2.0 ** -22 * np.abs(own).max()
    undecided = float((~d.decided).mean())
    print(f"{tag}: undecided maxima {undecided:.4f} of the (plot, channel) pairs (cap 0.05), exact-zero extrema {d.zero.mean():.2f}, "
          f"decision bound {d.bound:.2e}")
    assert undecided <= 0.05
    # ---- distances (the offset channel's own figures beside them: where a variance from fp32 sums and sums of squares loses digits first)
    for n, _, _ in G.BLOCKS:
        rel = lambda v, k: abs(float(v[k][G.OFFSET]) - ref[k][G.OFFSET]) / abs(ref[k][G.OFFSET])          # noqa: E731
        print(f"{tag} {n} offset channel, relative to itself: invstd {rel(got, n + '.invstd'):.2e} (fp32 restatement "
              f"{rel(r32, n + '.invstd'):.2e}), c {rel(got, n + '.c'):.2e} ({rel(r32, n + '.c'):.2e})")
    bad = G.show(tag, G.distances(got, ref), G.distances(r32, ref))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ (a) the one launch
@pytest.mark.parametrize("B,M2", G.SHAPES)
def test_one_launch_against_fp64(B, M2):
    lv = _Fwd(G.make_case(B, M2))
    assert ops.global_level_forward_fused(B, lv.blk["sa3"], lv.blk["fp3"])
    lv.one_launch()
    out = lv.outputs()
    assert lv.forward_gave_up() == 0
    _check(lv, out, "train", f"B={B} M2={M2} one launch")
    # the same inputs on reset state: the same bits in every output
    lv.reset()
    lv.one_launch()
    _assert_same_outputs(out, lv.outputs(), "second launch")
    if (B, M2) != (3, 64):
        return
    # every wait gives up after one sweep: the workgroup that leaves last computes the level again, alone (the memory path of the
    # max, FP3's skip rows staged again) -- the bits of the undisturbed launch, statistics and counters updated exactly once
    lib = _lib.load()
    lv.reset()
    lib.sn2_debug_global_spin_limit(1)
    try:
        lv.one_launch()
        out3 = lv.outputs()
        gave_up = lv.forward_gave_up()
    finally:
        lib.sn2_debug_global_spin_limit(0)
    print(f"B={B} M2={M2}: {gave_up} workgroup(s) gave up under a one-sweep wait limit")
    # (three workgroups: the first to publish sweeps once right behind its own stores and cannot find its peers' granules)
    assert gave_up > 0, "no wait gave up: the repair was not exercised"
    _assert_same_outputs(out, out3, "launch under a one-sweep wait limit")
    lv.reset()
    lv.one_launch()
    _assert_same_outputs(out, lv.outputs(), "launch after the repaired one")
    assert lv.forward_gave_up() == gave_up
    ops.global_level_gave_up(torch.device(DEV), warn=False)           # (seen: later tests' checks for NEW give-ups start from here)


# ------------------------------------------------------------------------------------------------ (b) the five launches
@pytest.mark.parametrize("mode", ("train", "frozen", "eval"))
@pytest.mark.parametrize("B,M2", G.SHAPES + [G.EXTRA])
def test_five_launches_against_fp64(B, M2, mode):
    lv = _Fwd(G.make_case(B, M2))
    lv.five_launches(mode)
    out = lv.outputs()
    _check(lv, out, mode, f"B={B} M2={M2} five launches {mode}")
    if mode == "train" and B <= ops.GL_MAX_PLOTS:
        # "the same staging, tiles": SA3's rows of the one launch are the separate launch's, bit for bit
        lv.reset()
        lv.one_launch()
        one = lv.outputs()
        assert _same_bits(one["h_sa3"], out["h_sa3"]), \
            f"h_sa3 of the one launch differs from sn2_fp_forward's in {int((_bits(one['h_sa3']) != _bits(out['h_sa3'])).sum())} words"


# ------------------------------------------------------------------------------------------------ (c) refusals
def test_refusals_before_any_device_work():
    raw = _lib.load()
    EINVAL, ELIMIT = _lib.CONSTANTS["SN2_EINVAL"], _lib.CONSTANTS["SN2_ELIMIT"]

    def call(lv, sa3=None, fp3=None, x3=None):
        ws = ops.global_level_ws(DEV, owner=lv)                               # the real exchange area: nothing here is a made-up address
        before = (ws[0].clone(), ws[1].clone())
        rc = raw.sn2_global_level_forward(lv.sa3() if sa3 is None else sa3, lv.fp3() if fp3 is None else fp3,
                                          (lv.x3 if x3 is None else x3).data_ptr(), lv.arg3.data_ptr(), ws[0].data_ptr(), ws[1].data_ptr(), None)
        out = lv.outputs()
        assert torch.equal(ws[0], before[0]) and torch.equal(ws[1], before[1]), "the exchange area was touched"
        for k, v in (("h_sa3", H_SENT), ("h3", H_SENT), ("x3", X_SENT)):
            assert _same_bits(out[k], np.full(out[k].shape, v, np.float32)), f"{k} was written"
        assert (out["arg3"] == ARG_SENT).all()
        for n, _, _ in G.BLOCKS:
            assert out[f"{n}.batches"] == NBT0 and _same_bits(out[f"{n}.a"], np.full(64, AUX_SENT, np.float32))
            assert _same_bits(out[f"{n}.running_mean"], lv.case.blk[n]["rm"].numpy())
        return rc

    lv = _Fwd(G.make_case(*G.EXTRA))                                          # 29 plots
    assert not ops.global_level_forward_fused(lv.B, lv.blk["sa3"], lv.blk["fp3"])
    ws = ops.global_level_ws(DEV, owner=lv)
    before = (ws[0].clone(), ws[1].clone())
    rc = raw.sn2_global_level_forward(lv.sa3(), lv.fp3(), lv.x3.data_ptr(), lv.arg3.data_ptr(), ws[0].data_ptr(), ws[1].data_ptr(), None)
    assert rc == ELIMIT
    out = lv.outputs()
    assert torch.equal(ws[0], before[0]) and torch.equal(ws[1], before[1]) and (out["arg3"] == ARG_SENT).all()
    assert _same_bits(out["h_sa3"], np.full(out["h_sa3"].shape, H_SENT, np.float32))
    with pytest.raises(ValueError):
        lv.one_launch()                                                       # (hip_ops refuses the workspace for 29 plots)
    lv = _Fwd(G.make_case(3, 64))
    assert ops.global_level_forward_fused(3, lv.blk["sa3"], lv.blk["fp3"])
    for n in ("sa3", "fp3"):                                                  # a block with bfloat16 operands
        lv.blk[n].mma_bf16 = True
        assert not ops.global_level_forward_fused(3, lv.blk["sa3"], lv.blk["fp3"])
        assert call(lv) == ELIMIT
        lv.blk[n].mma_bf16 = False
    # descriptors that do not belong together
    d = lv.fp3()
    d.R_per_plot += 1
    assert call(lv, fp3=d) == EINVAL
    d = lv.fp3()
    d.B -= 1
    assert call(lv, fp3=d) == EINVAL
    d = lv.sa3()
    d.S_per_plot = 1
    assert call(lv, sa3=d) == EINVAL
    other = torch.full((3, 64), X_SENT, device=DEV)
    assert call(lv, x3=other) == EINVAL                                       # fp3's source is not the x3 handed in
    assert _same_bits(other.cpu().numpy(), np.full((3, 64), X_SENT, np.float32))
    # ... and the same descriptors, unchanged, are taken
    lv.one_launch()
    _check(lv, lv.outputs(), "train", "B=3 M2=64 after the refusals")


# ------------------------------------------------------------------------------------------------ (d), (e) the plot max alone
@pytest.mark.parametrize("C", G.MAX_C)
@pytest.mark.parametrize("R", G.MAX_R)
def test_plot_max_forward_alone(R, C):
    B = 3
    m = G.max_case(B, R, C)
    h, a, c = torch.from_numpy(m.h).to(DEV), torch.from_numpy(m.a).to(DEV), torch.from_numpy(m.c).to(DEV)
    out, arg = ops.plot_max_forward(h, a, c, B, R, C)
    torch.cuda.synchronize()
    assert np.array_equal(arg.cpu().numpy(), m.arg), f"{int((arg.cpu().numpy() != m.arg).sum())} rows differ from numpy's first maximum"
    assert _same_bits(out.cpu().numpy(), m.out)
    # the same call into guarded buffers: nothing behind out and arg is written, h keeps its bits (padding columns included)
    out_g = torch.full((B * C + GUARD,), X_SENT, device=DEV)
    arg_g = torch.full((B * C + GUARD,), ARG_SENT, dtype=torch.int32, device=DEV)
    ops._call("sn2_plot_max_forward", h.data_ptr(), a.data_ptr(), c.data_ptr(), B, R, C, out_g.data_ptr(), arg_g.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert _same_bits(out_g[:B * C].cpu().numpy().reshape(B, C), m.out) and np.array_equal(arg_g[:B * C].cpu().numpy().reshape(B, C), m.arg)
    assert _same_bits(out_g[B * C:].cpu().numpy(), np.full(GUARD, X_SENT, np.float32)) and (arg_g[B * C:] == ARG_SENT).all()
    assert _same_bits(h.cpu().numpy(), m.h)


@pytest.mark.parametrize("C", G.MAX_C)
@pytest.mark.parametrize("R", G.MAX_R)
def test_plot_max_backward_alone(R, C):
    B = 3
    m = G.max_backward_case(B, R, C)
    full = torch.from_numpy(m.dy0).to(DEV)
    ops.plot_max_backward(torch.from_numpy(m.dout).to(DEV), torch.from_numpy(m.arg).to(DEV), B, R, C, full[:B * R])
    torch.cuda.synchronize()
    got = full.cpu().numpy()
    # exactly the addressed words equal dout; every other word -- padding columns, guard rows, the rows of entries -1 and R -- keeps its bytes
    assert _same_bits(got, m.dy), f"{int((_bits(got) != _bits(m.dy)).sum())} words differ"
    assert int((_bits(got) != _bits(m.dy0)).sum()) == m.written == B * (C - 2)


# ------------------------------------------------------------------------------------------------ (f) the pool backward alone
@pytest.mark.parametrize("R", G.POOL_R)
@pytest.mark.parametrize("B", G.POOL_B)
def test_global_pool_backward_alone(B, R):
    for stride in G.POOL_STRIDES:
        m = G.pool_backward_case(B, R, stride)
        t = {k: torch.from_numpy(getattr(m, k)).to(DEV) for k in ("du", "arg", "h", "mean", "invstd")}
        dx, dgamma, dbeta = (torch.from_numpy(getattr(m, k)).to(DEV) for k in ("dx0", "dgamma0", "dbeta0"))
        dy_full = torch.zeros(B * R + GUARD, 64, device=DEV)
        dy_full[B * R:] = H_SENT
        dy = dy_full[:B * R]
        if stride == 64:
            ops.global_pool_backward(t["du"], t["arg"], t["h"], t["mean"], t["invstd"], B, R, dx, dy, dgamma, dbeta)
        else:                                                                 # (hip_ops' wrapper takes du rows of 64 floats only)
            ops._call("sn2_global_pool_backward", t["du"].data_ptr(), stride, t["arg"].data_ptr(), t["h"].data_ptr(), t["mean"].data_ptr(),
                      t["invstd"].data_ptr(), B, R, 64, dx.data_ptr(), dy.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), ops._stream())
        torch.cuda.synchronize()
        got = {"dx": dx.cpu().numpy(), "dgamma": dgamma.cpu().numpy(), "dbeta": dbeta.cpu().numpy()}
        dyn = dy_full.cpu().numpy()
        # dy: one word per (plot, channel), the returned dx, at the row arg names; zero elsewhere; nothing behind it; du keeps its bits
        want = np.zeros((B * R + GUARD, 64), np.float32)
        want[B * R:] = H_SENT
        want[m.rows, np.arange(64)[None, :]] = got["dx"]
        assert _same_bits(dyn, want), f"B={B} R={R} stride={stride}: dy differs in {int((_bits(dyn) != _bits(want)).sum())} words"
        assert got["dx"][0, m.ZERO_CH] == 0.0 and int((dyn[:B * R] != 0).sum()) == B * 64 - 1
        assert _same_bits(t["du"].cpu().numpy(), m.du)
        bad = []
        for n in ("dx", "dgamma", "dbeta"):
            scale = float(np.abs(m.ref[n]).max())
            err = float(np.abs(got[n].astype(np.float64) - m.ref[n]).max()) / scale
            e32 = float(np.abs(m.r32[n].astype(np.float64) - m.ref[n]).max()) / scale
            bound = min(max(ATOM, FACTOR * e32), BOUND)
            print(f"B={B} R={R} du_stride={stride} {n}: vs fp64 {err:.2e}, bound {bound:.2e} (e32 {e32:.2e})")
            if not err <= bound:
                bad.append((n, stride, err, bound))
        assert not bad, bad
