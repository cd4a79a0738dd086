"""The set-abstraction message passes alone (csrc/sa_mfma.hip, driven from csrc/sa.hip) against fp64, in every item class, ties
included: SA2 <16,1,32,32> and the third ball-query level <32,1,64,64>, which nothing else runs alone, and what
tests/test_gpu_sa1_one_pass.py leaves out of SA1 <8,2,16,16> (the backward WITH a feature gradient, the eval forward, more than 32
plots).  Through hip_ops on the hand-made cases of tests/_sa_module_ref.py; tests/test_sa_module_ref_host.py proves on the CPU what
this file rests on.

The one-block cases are exact in fp32 and in bfloat16 (dyadic inputs), so `ext` and `arg` of a training or frozen forward are
compared with torch.equal -- "first maximum wins, lowest slot, on the signed extremum" has no tolerance; planted duplicate rows make
every channel tie across slots 15/16 and 63/64, the halves of an OCT half tile, the ends of a HEX quarter tile.  The backward then
routes exactly as the reference does and every gradient difference is rounding.  Layout A runs the backward once with the full
`dout` and once per item class (dout zero elsewhere): a class sets the scale of the tensors it is judged on.  `dfeat` starts from
a non-zero pattern, and rows on no list keep it to the bit.

Tolerances (none invented here):
  * ext, arg, untouched rows, sentinels: exact;  out: 1e-4 of max |out| (tests/test_gpu_sa1_one_pass.py);
  * gradients and dfeat, fp32 operands: the distance from fp64 relative to the tensor's largest element is at most
    max(ATOM = 1e-5, 8 e32), and never above BOUND = 1e-3; e32 is the same distance of the reference RESTATED IN FP32 ON THE CPU,
    routed by the fp64 slots (the kernel adds the same terms in another association; nothing else may differ).  dfeat's distance
    is taken relative to the gradient (dfeat minus the pre-fill), the stricter scale;
  * bf16 operands: 2e-2 for gradients and dfeat, 1e-3 on out (tests/test_gpu_bf16.py); ext / arg still exact;
  * running statistics: atol 1e-5, rtol 1e-4 (test_train_step_vs_reference_golden).
Measured on an MI355X (every figure is printed next to its bound; DESIGN.md section 3, "Set-abstraction modules alone"):
  fp32 operands  parameter gradients 2e-8 ... 1.4e-6 (sa2 / sa3), ... 1.7e-6 (sa1); dfeat 7e-8 ... 2.5e-7; e32 4e-8 ... 8e-7
                 (sa1 ... 1.2e-6); kernel / e32 at most 4.6 -- every bound is ATOM, the largest error 14 % of it
  bf16 operands  4e-8 ... 4.4e-3 (parameter gradients), 1.3e-3 ... 3.3e-3 (dfeat)
  out 4e-8 ... 4e-7; running statistics 5e-8 (mean), 3e-7 (variance); sa1: every slot is the reference's
"""
import numpy as np
import pytest
import torch

import _sa_module_ref as R
from stratanet2_vegetation_coverage_maps_amd import _lib, hip_ops as ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATOM, BOUND, FACTOR = 1e-5, 1e-3, 8
OUT_TOL, BF16_OUT, BF16_GRAD = 1e-4, 1e-3, 2e-2
STAT_ATOL, STAT_RTOL = 1e-5, 1e-4
EXT_SENTINEL, ARG_SENTINEL, OUT_SENTINEL = -777.25, -7777, 555.5
TRAINING = {"train": True, "frozen": _lib.BN_FROZEN_KEEP, "eval": False}

KINDS, LAYOUTS = ("sa2", "sa3"), ("A", "B", "C")
ALL = [pytest.param(k, l, o, b, id=f"{k}-{l}-{'order' if o else 'noorder'}-{'bf16' if b else 'fp32'}")
       for k in KINDS for l in LAYOUTS for o in (True, False) for b in (False, True)]


class _Module:
    """A case on the device: the blocks, the tables, and a backward into a fresh zero-filled arena per call."""

    def __init__(self, case, with_order, bf16=False):
        self.case = c = case
        self.cf, self.cl = c.cf, c.mlp[-1]
        self.rows, self.cpos, self.nbr, self.cnt = c.rows.to(DEV), c.cpos.to(DEV), c.nbr.to(DEV), c.cnt.to(DEV)
        self.total = c.total.to(DEV)
        self.order = ops.sa_order(self.cnt, c.B, c.M) if with_order else None
        self.blocks = []
        for p in c.params:
            co, ci = p["W"].shape
            lin, bn = torch.nn.Linear(ci, co).to(DEV), torch.nn.BatchNorm1d(co).to(DEV)
            with torch.no_grad():
                lin.weight.copy_(p["W"]), lin.bias.copy_(p["b"]), bn.weight.copy_(p["gamma"]), bn.bias.copy_(p["beta"])
                bn.running_mean.copy_(p["rm"]), bn.running_var.copy_(p["rv"])
            blk = ops.BlockBuffers(lin, bn)
            blk.mma_bf16 = bf16
            self.blocks.append(blk)
        n = c.B * c.M
        self.ext = torch.full((n, self.cl), EXT_SENTINEL, device=DEV)
        self.arg = torch.full((n, self.cl), ARG_SENTINEL, dtype=torch.int32, device=DEV)
        self.out = torch.full((n, self.cl), OUT_SENTINEL, device=DEV)
        self.shapes = [s for p in c.params for s in (tuple(p["W"].shape), (p["W"].shape[0],), (p["W"].shape[0],), (p["W"].shape[0],))]
        self.n_flat = sum(int(np.prod(s)) for s in self.shapes)

    def desc(self, **kw):
        c = self.case
        return ops.sa_desc(self.blocks, self.rows[:, 0:self.cf], self.cf, self.rows[:, self.cf:self.cf + 4], self.cpos, self.nbr,
                           self.cnt, self.total, c.B, c.Nsrc, c.M, self.ext, self.arg, self.out, order=self.order, **kw)

    def forward(self, mode):
        for blk in self.blocks:
            blk.frozen = mode == "frozen"
        ops.sa_forward(self.desc(), TRAINING[mode])
        torch.cuda.synchronize()

    def statistics(self):
        return [(b.bn.running_mean.cpu().numpy().copy(), b.bn.running_var.cpu().numpy().copy(), int(b.bn.num_batches_tracked))
                for b in self.blocks]

    def backward(self, dout, dfeat0=None, one_pass=False):
        """-> {name: gradient (numpy)}, with "dfeat" when a pre-fill is given (the two-pass route), "ws" the workspace"""
        arena, flat, images, extra = ops.grad_images_alloc(self.n_flat, DEV, ops.SA_BWD_WS_WORDS)
        views, o = [], 0
        for s in self.shapes:
            n = int(np.prod(s))
            views.append(flat[o:o + n].view(s))
            o += n
        for k, blk in enumerate(self.blocks):
            blk.grads, blk.grad_images = tuple(views[4 * k:4 * k + 4]), images
        dfeat = None if dfeat0 is None else dfeat0.to(DEV).clone()
        ops.sa_backward(self.desc(dout=dout.to(DEV).contiguous(), dfeat=dfeat, with_grads=True, bwd_ws=extra if one_pass else None))
        ops.grad_reduce(arena, self.n_flat, images)
        torch.cuda.synchronize()
        g = {n: v.detach().cpu().numpy().copy() for n, v in zip(R.grad_names(self.case), views)}
        g["ws"] = extra.cpu().numpy().copy()
        if dfeat is not None:
            g["dfeat"] = dfeat.cpu().numpy()
        return g


_CACHE = {}


def _case(kind, layout):
    return R.case_of(kind, layout)


def _masks(case):
    """{name: (B*M, 1) factor on dout}: the full dout; layout A: one per item class; layout C: plot 32, the lone group."""
    m = {"all": torch.ones(case.B * case.M, 1)}
    if case.layout == "A":
        for name in R.CLASS_NAMES[:4]:
            m[name] = R.class_mask(case, name)
    if case.layout == "C":
        m["plot32"] = R.plot_mask(case, case.B - 1)
    return m


def _ref(kind, layout, mode, mask="all"):
    """(fp64 reference, its fp32 restatement routed by the fp64 slots, dout) -- computed once per process, never changed."""
    key = (kind, layout, mode, mask)
    if key not in _CACHE:
        case = _case(kind, layout)
        dout = None if mode == "eval" else case.dout * _masks(case)[mask]
        ref = R.reference(case, mode, dout)
        _CACHE[key] = (ref, R.reference_fp32(case, mode, ref["arg"], dout), dout)
    return _CACHE[key]


def _rel(a, b, scale):
    return float(np.abs(np.asarray(a, np.float64) - b).max()) / scale


def _empty(case):
    return (case.cnt == 0).numpy()


def _check_extremum(m, ref, tag):
    case = m.case
    ext, arg = m.ext.cpu(), m.arg.cpu()
    ext_ref, arg_ref = torch.from_numpy(ref["ext"]).float(), torch.from_numpy(ref["arg"])
    assert torch.equal(ext_ref.double(), torch.from_numpy(ref["ext"]))                  # the fp64 extremum IS an fp32 number
    n_arg, n_ext = int((arg != arg_ref).sum()), int((ext != ext_ref).sum())
    print(f"{tag}: arg differs in {n_arg}, ext in {n_ext} of {arg.numel()} (centroid, channel) pairs")
    assert torch.equal(arg, arg_ref), f"{n_arg} slots differ, first at {(arg != arg_ref).nonzero()[:4].tolist()}"
    assert torch.equal(ext, ext_ref), f"{n_ext} extrema differ, first at {(ext != ext_ref).nonzero()[:4].tolist()}"
    e = torch.from_numpy(_empty(case))
    assert bool(e.any()) == (case.layout != "B")
    assert bool((arg[e] == -1).all()) and bool((ext[e] == 0).all())


def _check_out(m, ref, bf16, tag):
    out = m.out.cpu().numpy()
    err = _rel(out, ref["out"], np.abs(ref["out"]).max())
    tol = BF16_OUT if bf16 else OUT_TOL
    print(f"{tag}: out vs fp64 {err:.2e} (bound {tol:.0e})")
    assert err < tol
    assert not out[_empty(m.case)].any()                                                # exactly 0 without a neighbour


def _check_statistics(m, before, ref, tag):
    for k, ((rm, rv, nbt), (rm0, rv0, nbt0)) in enumerate(zip(m.statistics(), before)):
        if ref["batches"]:
            print(f"{tag}: block {k} running mean / var vs fp64 {np.abs(rm - ref['running_mean'][k]).max():.1e} / "
                  f"{np.abs(rv - ref['running_var'][k]).max():.1e} (atol {STAT_ATOL:.0e}, rtol {STAT_RTOL:.0e})")
            np.testing.assert_allclose(rm, ref["running_mean"][k], atol=STAT_ATOL, rtol=STAT_RTOL)
            np.testing.assert_allclose(rv, ref["running_var"][k], atol=STAT_ATOL, rtol=STAT_RTOL)
            assert nbt == nbt0 + 1
        else:
            assert np.array_equal(rm, rm0) and np.array_equal(rv, rv0) and nbt == nbt0  # to the bit


def _check_gradients(got, ref, ref32, names, bf16, tag, dfeat0=None, bound_only=False):
    """Every figure is printed, then all are asserted.  bound_only (sa1: the thresholds of tests/test_gpu_sa1_one_pass.py): BOUND."""
    bad = []
    for n in names:
        r, r32, g = ref[n], ref32[n], got[n]
        if n == "dfeat":                                                                # relative to the gradient, not the pre-fill
            scale = np.abs(r - dfeat0).max()
        else:
            scale = np.abs(r).max()
        assert scale > 0, n
        err, e32 = _rel(g, r, scale), _rel(r32, r, scale)
        bound = BF16_GRAD if bf16 else (BOUND if bound_only else min(max(ATOM, FACTOR * e32), BOUND))
        print(f"{tag} {n}: vs fp64 {err:.2e}, bound {bound:.2e} (e32 {e32:.2e})")
        if not err <= bound:
            bad.append((n, err, bound, e32))
    assert not bad, bad


def _unlisted(case):
    _, _, src, _ = R.messages(case)
    on = np.zeros(case.B * case.Nsrc, dtype=bool)
    on[src.numpy()] = True
    return ~on


# ------------------------------------------------------------------------------------------------------------ SA2, third level
@pytest.mark.parametrize("kind,layout,with_order,bf16", ALL)
def test_training_forward(kind, layout, with_order, bf16):
    case, (ref, _, _) = _case(kind, layout), _ref(kind, layout, "train")
    tag = f"{kind} {layout} train"
    m = _Module(case, with_order, bf16)
    before = m.statistics()
    m.forward("train")
    _check_extremum(m, ref, tag)
    _check_out(m, ref, bf16, tag)
    _check_statistics(m, before, ref, tag)
    first = [t.clone() for t in (m.ext, m.arg, m.out, m.blocks[0].aux)]
    m.ext.fill_(EXT_SENTINEL), m.arg.fill_(ARG_SENTINEL), m.out.fill_(OUT_SENTINEL), m.blocks[0].aux.zero_()
    m.forward("train")                                                                  # statistics through slots, not atomics:
    for a, b, n in zip(first, (m.ext, m.arg, m.out, m.blocks[0].aux), ("ext", "arg", "out", "aux")):
        assert torch.equal(a, b), f"{n} differs between two calls"                      # the same bits on every call


@pytest.mark.parametrize("kind,layout,with_order,bf16", ALL)
def test_frozen_forward(kind, layout, with_order, bf16):
    case, (ref, _, _) = _case(kind, layout), _ref(kind, layout, "frozen")
    tag = f"{kind} {layout} frozen"
    m = _Module(case, with_order, bf16)
    before = m.statistics()
    m.forward("frozen")
    _check_extremum(m, ref, tag)
    _check_out(m, ref, bf16, tag)
    _check_statistics(m, before, ref, tag)


@pytest.mark.parametrize("kind,layout,with_order,bf16", ALL)
def test_eval_forward(kind, layout, with_order, bf16):
    case, (ref, _, _) = _case(kind, layout), _ref(kind, layout, "eval")
    m = _Module(case, with_order, bf16)
    before = m.statistics()
    m.forward("eval")
    _check_out(m, ref, bf16, f"{kind} {layout} eval")
    assert bool((m.ext == EXT_SENTINEL).all()) and bool((m.arg == ARG_SENTINEL).all())  # left alone, as the header promises
    _check_statistics(m, before, ref, "eval")


@pytest.mark.parametrize("mode", ("train", "frozen"))
@pytest.mark.parametrize("kind,layout,with_order,bf16", ALL)
def test_backward(kind, layout, with_order, bf16, mode):
    case = _case(kind, layout)
    m = _Module(case, with_order, bf16)
    m.forward(mode)
    assert torch.equal(m.arg.cpu(), torch.from_numpy(_ref(kind, layout, mode)[0]["arg"]))       # the routing IS the reference's
    unlisted = _unlisted(case)
    assert unlisted.sum() >= R.UNLISTED * case.B
    for mask in _masks(case):
        ref, ref32, dout = _ref(kind, layout, mode, mask)
        got = m.backward(dout, case.dfeat0)
        assert np.array_equal(got["dfeat"][unlisted], case.dfeat0.numpy()[unlisted]), "a row on no list moved"
        assert not got["ws"].any()
        _check_gradients(got, ref, ref32, R.grad_names(case) + ("dfeat",), bf16, f"{kind} {layout} {mode} dout[{mask}]",
                         dfeat0=case.dfeat0.numpy().astype(np.float64))


# ------------------------------------------------------------------------------------------------------------ SA1
def _check_slots_attain(m, ref, tag):
    """continuous inputs: the slot the kernel names attains the fp64 signed extremum within the out tolerance"""
    case = m.case
    _, _, _, start = R.messages(case)
    arg = m.arg.cpu().long()
    full = ~torch.from_numpy(_empty(case))
    assert bool((arg[~full] == -1).all()) and bool((arg[full] >= 0).all()) and bool((arg[full] < case.cnt.long()[full, None]).all())
    h = torch.from_numpy(ref["h"])
    at = h[(start[:, None] + arg.clamp(min=0)).clamp(max=h.shape[0] - 1), torch.arange(h.shape[1])[None, :]]
    scale = np.abs(ref["ext"]).max()
    d = float((at - torch.from_numpy(ref["ext"]))[full].abs().max()) / scale
    e = _rel(m.ext.cpu().numpy(), ref["ext"], scale)
    same = int((arg.int() == torch.from_numpy(ref["arg"])).sum())
    print(f"{tag}: h at the kernel's slot vs the fp64 extremum {d:.2e}, ext vs fp64 {e:.2e} (bound {OUT_TOL:.0e}); "
          f"{same} of {arg.numel()} slots are the reference's")
    assert d < OUT_TOL and e < OUT_TOL


@pytest.mark.parametrize("mode", ("train", "frozen"))
@pytest.mark.parametrize("with_order", (True, False))
def test_sa1_backward_with_feature_gradient(with_order, mode):
    """the two-pass route with `dfeat`: pass D's k < CF masking at CF = 8"""
    case = _case("sa1", "A")
    m = _Module(case, with_order)
    before = m.statistics()
    m.forward(mode)
    ref = _ref("sa1", "A", mode)[0]
    _check_slots_attain(m, ref, f"sa1 A {mode}")
    _check_out(m, ref, False, f"sa1 A {mode}")
    _check_statistics(m, before, ref, f"sa1 A {mode}")
    unlisted = _unlisted(case)
    for mask in _masks(case):
        ref, ref32, dout = _ref("sa1", "A", mode, mask)
        got = m.backward(dout, case.dfeat0)
        assert np.array_equal(got["dfeat"][unlisted], case.dfeat0.numpy()[unlisted]), "a row on no list moved"
        assert not got["ws"].any()
        _check_gradients(got, ref, ref32, R.grad_names(case) + ("dfeat",), False, f"sa1 A {mode} dout[{mask}]",
                         dfeat0=case.dfeat0.numpy().astype(np.float64), bound_only=True)


@pytest.mark.parametrize("with_order", (True, False))
@pytest.mark.parametrize("layout", ("A", "C"))
def test_sa1_eval_forward(layout, with_order):
    case, (ref, _, _) = _case("sa1", layout), _ref("sa1", layout, "eval")
    m = _Module(case, with_order)
    before = m.statistics()
    m.forward("eval")
    _check_out(m, ref, False, f"sa1 {layout} eval")
    assert bool((m.ext == EXT_SENTINEL).all()) and bool((m.arg == ARG_SENTINEL).all())
    _check_statistics(m, before, ref, "eval")


@pytest.mark.parametrize("with_order", (True, False))
def test_sa1_plot_groups_one_pass(with_order):
    """33 plots: four groups of 8 and a lone one; training forward and the one-pass backward (a workspace, no feature gradient)"""
    case = _case("sa1", "C")
    m = _Module(case, with_order)
    before = m.statistics()
    m.forward("train")
    ref = _ref("sa1", "C", "train")[0]
    _check_slots_attain(m, ref, "sa1 C train")
    _check_out(m, ref, False, "sa1 C train")
    _check_statistics(m, before, ref, "sa1 C train")
    for mask in _masks(case):
        ref, ref32, dout = _ref("sa1", "C", "train", mask)
        got = m.backward(dout, None, one_pass=True)
        assert np.abs(got["ws"]).max() > 0                                              # the route was taken
        _check_gradients(got, ref, ref32, R.grad_names(case), False, f"sa1 C train one-pass dout[{mask}]", bound_only=True)
