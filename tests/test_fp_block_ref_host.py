"""What tests/test_gpu_fp_blocks.py rests on, checked where there is no GPU (tests/_fp_block_ref.py builds the cases):

  * the fp64 reference against a second method: at the tiny shape its gradients equal central finite differences of its own
    forward (sampled coordinates of every gradient, training and frozen statistics) to 1e-6 of the gradient's largest element;
  * the planted lists, counted from the table itself per plot as csrc/interp_index.hip counts them: exactly one empty list;
    the planted list of 64 ... 126 entries wherever a plot has at least 64 rows (at 43 rows per plot no list of distinct rows
    can be that long: there the longest list stays below 64, one chunk); a list above 2048 entries wherever a plot has more than
    2048 rows (at 2049 rows exactly one, holding every row); every index inside its plot, every weight sum positive, three
    distinct sources per row;
  * the forms: for every case and pass, sn2_fp_form on a fake-pointer descriptor returns the form the case is meant to reach, and
    the two gather kernels and the two BatchNorm-sum kernels are each reached from the side the case table says;
  * the edge inputs: both zero columns of W give an exactly zero reference gradient, the dead channel is zero on every row,
    negative gamma channels and negative source-affine factors exist;
  * no ReLU mask hangs on rounding: every live pre-activation keeps 2^-15 from zero (with bfloat16 operands too where a case
    runs with them), and the fp32 restatement's mask is the fp64 mask;
  * the fp32 restatement is within 1e-5 (of the largest element) of fp64 on dW, dsrc and dskip in every case."""
import numpy as np
import pytest
import torch

import _fp_block_ref as R

_FAKE = 0x1000
DATA_SPECS = list({R.data_key(s): s for s in R.SPECS.values() if not s.bf16}.values())
_REF = {}


def _ref(spec, mode):
    k = (R.data_key(spec), mode)
    if k not in _REF:
        _REF[k] = R.reference(R.make_case(spec), mode)
    return _REF[k]


# ------------------------------------------------------------------------------------------------ a second method
@pytest.mark.parametrize("mode", ("train", "frozen"))
@pytest.mark.parametrize("name", sorted(R.BLOCKS))
def test_reference_gradients_equal_central_differences(name, mode):
    spec = R.SPECS[f"tiny-{name}"]
    c = R.make_case(spec)
    ref = _ref(spec, mode)
    b = c.block
    src = c.src[:, :b.ca].double()
    z0 = src if c.sa is None else c.sa.double() * src + c.sc.double()
    base = {"dW": ("W", c.W), "db": ("b", c.b), "dgamma": ("gamma", c.gamma), "dbeta": ("beta", c.beta),
            "dsrc": ("z", z0), "dskip": ("skip", c.skip[:, :b.cb])}
    g = torch.Generator().manual_seed(5)
    eps = 1e-5
    worst = {}
    for gname, (pname, value) in base.items():
        value = value.double()
        grad = ref[gname]
        scale = np.abs(grad).max()
        assert scale > 0
        flat = torch.randperm(value.numel(), generator=g)[:6].tolist()
        if gname == "dW":
            flat += [R.DEAD * value.shape[1] + 2, 3 * value.shape[1] + R.ZERO_COL]       # the dead channel's row, a zero column
        if gname == "dsrc" and b.knn and c.S > 1:
            flat += [((0 + 1) % c.S) * value.shape[1] + 2]                                 # plot 0's source on no list
        err = 0.0
        for i in flat:
            loss = []
            for sgn in (1.0, -1.0):
                v = value.clone().view(-1)
                v[i] += sgn * eps
                v = v.view(value.shape)
                kw = {"z_in": v} if pname == "z" else {"skip_in": v} if pname == "skip" else {"params": {pname: v}}
                loss.append(R.reference(c, mode, backward=False, **kw)["loss"])
            fd = (loss[0] - loss[1]) / (2 * eps)
            err = max(err, abs(fd - grad.reshape(-1)[i]) / scale)
        worst[gname] = err
    print(f"tiny-{name} {mode}: reference vs central differences {worst}")
    assert max(worst.values()) < 1e-6, worst


# ------------------------------------------------------------------------------------------------ planted lists
@pytest.mark.parametrize("spec", [s for s in DATA_SPECS if R.BLOCKS[s.block].knn], ids=lambda s: s.id)
def test_planted_lists_are_in_the_table(spec):
    c = R.make_case(spec)
    B, Rp, S = c.B, c.Rp, c.S
    idx, w = c.idx, c.w
    assert idx.dtype == torch.int32 and int(idx.min()) >= 0 and int(idx.max()) < S       # per-plot ids: inside the plot
    assert bool((w.sum(1) > 0).all()) and bool((w >= 0).all()) and bool((w[:, 0] > 0).all())
    cnt = R.list_counts(idx, w, B, Rp, S)
    if S == 1:
        assert bool((idx == 0).all()) and bool((w[:, 1:] == 0).all()) and bool((cnt == Rp).all())
        return
    s = idx.sort(1).values
    assert bool((s[:, 0] < s[:, 1]).all()) and bool((s[:, 1] < s[:, 2]).all())           # three distinct sources
    zero_w = (w[:, 1] == 0) & (w[:, 2] == 0)
    assert Rp // 7 * B <= int(zero_w.sum()) <= (Rp // 7 + 1) * B
    for b in range(B):
        E, H, L = R.specials(b, Rp, S)
        n = cnt[b]
        assert int((n == 0).sum()) == 1 and int(n[E]) == 0                                # exactly one empty list
        two = (n >= 64) & (n <= 126)
        if Rp >= 64:
            assert bool(two[H]), (b, n.tolist())                                          # the planted list of two chunks
        else:
            assert int(n.max()) < 64
        if Rp > 2048:
            assert int(n[L]) > 2048
            if Rp == 2049:
                assert int(n[L]) == 2049 and int((n > 2048).sum()) == 1                   # every row, the second slice's one included
        assert int(n.sum()) == 3 * Rp - 2 * int(zero_w[b * Rp:(b + 1) * Rp].sum())
    print(f"{spec.id}: list lengths per plot min {cnt.min(1).values.tolist()[:3]} max {cnt.max(1).values.tolist()[:3]}")
    # the named source of a zero-weight slot is the empty one: only the weight keeps it off the list
    E_of = torch.tensor([R.specials(b, Rp, S)[0] for b in range(B)]).repeat_interleave(Rp)
    assert bool((idx[zero_w, 1].long() == E_of[zero_w]).all())
    perm = c.row_perm.view(B, Rp).long()
    assert bool((perm.sort(1).values == torch.arange(Rp)).all()) and not bool((perm == torch.arange(Rp)).all())


# ------------------------------------------------------------------------------------------------ forms
def _shell(spec, backward):
    """The sn2_fp the GPU test's descriptor amounts to, every pointer fake (as _fp_shell of tests/test_cabi.py)."""
    from stratanet2_vegetation_coverage_maps_amd import _lib
    b = R.BLOCKS[spec.block]
    p = _lib.FP()
    p.B, p.R_per_plot, p.S_per_plot, p.ca, p.cb = spec.B, spec.Rp, spec.S, b.ca, b.cb
    p.src, p.src_stride, p.skip, p.skip_stride = _FAKE, b.src_stride, _FAKE, b.skip_stride
    if b.knn:
        p.knn_idx = p.knn_w = _FAKE
        p.src_a = p.src_c = _FAKE
    p.blk.cin, p.blk.cout, p.blk.W, p.blk.b = b.ca + b.cb, b.cout, _FAKE, _FAKE
    p.h, p.h_stride = _FAKE, (b.cout + 3) // 4 * 4
    R_all = spec.B * spec.Rp
    p.blk.mma_bf16 = int(spec.bf16 and R_all <= R.STAT_ROWS)
    # hip_ops.fp_desc hands out the source-side workspace where sn2_fp_source_side(R, cb, 0) holds and SOURCE_SIDE is set
    lib = _lib.load()
    if spec.source_side and b.knn and lib.sn2_fp_source_side(R_all, b.cb, 0):
        p.src_ws = _FAKE
    if backward:
        p.dy = p.blk.dW = p.blk.db = p.blk.dgamma = p.blk.dbeta = _FAKE
        p.blk.grad_replicas = 1
        p.dsrc, p.dsrc_stride = _FAKE, b.src_stride
        if b.knn:
            p.du_scratch, p.scatter_ws = _FAKE, _FAKE
            p.scatter_ready = -1 if not spec.gather else 0 if spec.variant == "built" else 1
        if spec.dskip:
            p.dskip, p.dskip_stride = _FAKE, b.cb
        if spec.variant == "perm":
            p.row_perm = _FAKE
    return p


@pytest.mark.parametrize("spec", list(R.SPECS.values()), ids=lambda s: s.id)
def test_every_case_takes_the_form_it_is_meant_to(spec):
    from ctypes import byref
    from stratanet2_vegetation_coverage_maps_amd import _lib
    lib = _lib.load()
    assert (R.SPLIT, R.SOURCE_SIDE, R.DENSE) == (_lib.SN2_FP_FORM_SPLIT, _lib.SN2_FP_FORM_SOURCE_SIDE, _lib.SN2_FP_FORM_DENSE)
    assert R.STAT_ROWS == 64 * _lib.STAT_SLOTS and _lib.BN_FROZEN_KEEP == 2
    fwd = _shell(spec, False)
    got = (lib.sn2_fp_form(byref(fwd), 1), lib.sn2_fp_form(byref(fwd), 2), lib.sn2_fp_form(byref(fwd), 0),
           lib.sn2_fp_form(byref(_shell(spec, True)), 3))
    assert got == (spec.fwd, spec.fwd, spec.fwd_eval, spec.bwd), (spec.id, got)


def test_the_cases_reach_every_form_and_switch_of_every_block():
    """The case table against the issue's: each instantiation in each form it can take, both gather kernels, both BatchNorm-sum
    kernels and both grids of the larger one, the route thresholds from both sides."""
    reach = {(s.block, "fwd", f) for s in R.SPECS.values() for f in (s.fwd, s.fwd_eval)} | {(s.block, "bwd", s.bwd) for s in R.SPECS.values()}
    for name, b in R.BLOCKS.items():
        for d in ("fwd", "bwd"):
            assert (name, d, R.SPLIT) in reach and (name, d, R.DENSE) in reach, (name, d)
    for name in ("FP1", "FP2"):
        assert (name, "fwd", R.SOURCE_SIDE) in reach and (name, "bwd", R.SOURCE_SIDE) in reach
    assert any(s.block == "FP2" and s.dskip and (s.fwd, s.bwd) == (R.SOURCE_SIDE, R.DENSE) for s in R.SPECS.values())

    def long_gather(s):                                                   # bwd_gather's switch (csrc/fp.hip)
        return s.Rp >= 128 * s.S and R.BLOCKS[s.block].ca <= 64
    gathers = [s for s in R.SPECS.values() if R.BLOCKS[s.block].knn and s.gather and s.bwd != R.SOURCE_SIDE]
    for name in ("FP3", "FP4", "FP2", "FP1"):
        assert any(long_gather(s) for s in gathers if s.block == name), name
    for name in ("FP2", "FP1"):
        assert any(not long_gather(s) for s in gathers if s.block == name), name
    assert long_gather(R.SPECS["densefp2-170"]) and not long_gather(R.SPECS["densefp2-171"])
    assert long_gather(R.SPECS["densefp1-FP1"]) and not long_gather(R.SPECS["densefp1-171"]) and not long_gather(R.SPECS["seg-FP2"])
    # (the edge cases have 65 536 / 65 537 rows over 64 sources: 128 * 64 = 8192 rows is the switch, so they take the long gather,
    # in the Split form below the row threshold and in the Dense form above it)
    assert long_gather(R.SPECS["edge65536-FP1"]) and long_gather(R.SPECS["edge65537-FP1-rows"]) and not long_gather(R.SPECS["tiny-FP1"])
    rows = sorted({s.B * s.Rp for s in R.SPECS.values()})
    assert 65536 in rows and 65537 in rows and 65538 in rows              # fp_bwd_bn_small_kernel | fp_bwd_bn_kernel, one row per thread
    assert max(rows) == 262146 >= 2 ** 18                                 # ... | eight rows per thread
    assert all(s.B <= R.MAX_PLOTS and s.B * s.Rp <= R.MAX_ROWS for s in R.SPECS.values())
    t = R.SPECS["tinyplots-FP1-built"]
    chunks = (3 * t.Rp + 62) // 63 + t.S                                  # SN2_INTERP_CHUNKS
    assert chunks == 52 < 64 and t.B * t.Rp > R.STAT_ROWS
    assert {s.variant for s in R.SPECS.values() if s.id.startswith("src-FP1")} == {"built", "morton", "perm"}
    assert {s.variant for s in R.SPECS.values() if s.id.startswith("src-FP2")} == {"built", "morton", "perm"}
    assert {s.variant for s in R.SPECS.values() if s.id.startswith("tinyplots")} == {"built", "morton", "perm"}


# ------------------------------------------------------------------------------------------------ edge inputs, precision
@pytest.mark.parametrize("spec", DATA_SPECS, ids=lambda s: s.id)
def test_edge_inputs_and_fp32_restatement(spec):
    c = R.make_case(spec)
    b = c.block
    assert bool((c.gamma < 0).any()) and bool((c.gamma > 0).any()) and not c.W[:, R.ZERO_COL].any() and not c.W[:, b.ca + 1].any()
    assert c.sa is None or (bool((c.sa < 0).any()) and bool((c.sa > 0).any()))
    assert c.src.shape[1] == b.src_stride and c.skip.shape[1] == b.skip_stride and bool((c.dsrc0 != 0).all()) and bool((c.dskip0 != 0).all())
    for mode in ("train", "frozen"):
        ref = _ref(spec, mode)
        assert not ref["h"][:, R.DEAD].any() and (ref["h"] > 0).mean() > 0.25            # dead on every row; the rest is alive
        assert not ref["dW"][R.DEAD].any() and ref["db"][R.DEAD] == 0.0
        if mode == "train":
            assert ref["mean"][R.DEAD] == 0.0 and abs(ref["invstd"][R.DEAD] - R.EPS ** -0.5) < 1e-9
        assert not ref["dsrc"][:, R.ZERO_COL].any() and not ref["du"][:, R.ZERO_COL].any() and not ref["dskip"][:, 1].any()
        assert not ref["dsrc"][R.unlisted_sources(c)].any()
        r32 = R.reference_fp32(c, mode)
        # no ReLU mask hangs on fp32 rounding: every live pre-activation keeps MARGIN from zero, and the restatement's mask is fp64's
        assert ref["margin"] >= R.MARGIN and np.array_equal(r32["mask"], ref["mask"]), (ref["margin"], int((r32["mask"] != ref["mask"]).sum()))
        for n in ("dW", "dsrc", "dskip"):
            scale = np.abs(ref[n]).max()
            e = np.abs(r32[n].astype(np.float64) - ref[n]).max() / scale
            print(f"{spec.id} {mode} {n}: fp32 restatement vs fp64 {e:.2e}")
            assert scale > 0 and e < 1e-5, (n, e)
    if b.knn and c.S > 1:
        assert R.unlisted_sources(c).sum() == c.B
    if f"{spec.id}-bf16" in R.SPECS:                                                      # the same with bfloat16 operands
        rb = R.reference(c, "train", bf16=True)
        assert rb["margin"] >= R.MARGIN and not rb["h"][:, R.DEAD].any()
        moved = np.abs(rb["h"] - _ref(spec, "train")["h"]).max() / np.abs(rb["h"]).max()
        print(f"{spec.id}: bf16 operands move h by {moved:.1e} of its largest element")
        assert 1e-4 < moved < 1e-1                                                        # a different precision, and only that
