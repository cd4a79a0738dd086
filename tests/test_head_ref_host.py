"""What tests/test_gpu_head_backward.py and tests/test_gpu_bn_sums_consumer.py rest on, checked where there is no GPU
(tests/_head_ref.py builds the cases and the reference):

  * the fp64 reference against a second method: its hand-written backward equals central finite differences of its own scalar
    objective (sum cov dcov + sum proba dproba) in y, W1, b1, W2 and b2 to 1e-6 of the gradient's largest element, with and
    without dropout, with either incoming gradient absent, on sampled coordinates that include the dead channel, the zero
    column and the four scaled rows;
  * the consumer identity is exact: with y = gamma xhat + beta unrounded, W1^T G with G = (dW1 - beta db1) / gamma equals the
    sums over the rows to 1e-12 of their largest element at every swept (gamma, beta), |gamma| = nextafter(1e-4f) included --
    only rounded inputs make it inexact (evaluated in long double: at |gamma| = 1e-4, beta = 8 plain fp64 is at 2e-12, printed);
  * no ReLU mask hangs on rounding, in every case the GPU files use: every live pre-activation keeps 2^-15 (times the row's
    largest |y| where above 1) from zero in fp64, in the fp32 restatement and from the bfloat16 rows; the fp32 mask is the fp64
    mask; the dead channel is negative on every row by at least 1;
  * the edge inputs: the four scaled rows have s[4] = +-30, +-100 (to 0.5), at least one row's softmax is one-hot to 1e-12, and
    everything stays finite in fp64 and in fp32; the dead channel's row of dW1, its db1 and its column of dW2, and the zero
    column of dy, are exactly zero in the reference; the padding of f holds the sentinel;
  * e32, the distance of the fp32 restatement from fp64 relative to each tensor's largest element, is printed for every case
    (it feeds the GPU files' bound max(1e-5, 8 e32)); for the sweep also a CPU MODEL of the identity from fp32 dW1 / db1 (the
    restatement's, not the kernel's: the kernel is measured in tests/test_gpu_bn_sums_consumer.py)."""
import numpy as np
import pytest
import torch

import _head_ref as H

LARGE = 2 * 256 * 256 + 65                   # the large shape of tests/test_gpu_head_backward.py on a 256-CU device
GRADS = [(True, True), (True, False), (False, True)]
SWEEP = [(g, b) for g in H.SWEEP_GAMMAS for b in H.SWEEP_BETAS]
ALL_CASES = ([(R, None, None) for R in H.SMALL_ROWS + (4160, LARGE)] + [(R, g, b) for R in H.SUMS_ROWS for g, b in SWEEP] +
             [(R, g, None) for R in H.FALLBACK_ROWS for g in H.FALLBACK_GAMMAS])


def _id(case):
    R, g, b = case
    return f"R{R}" + ("" if g is None else f"-gamma{g:.9g}") + ("" if b is None else f"-beta{b:g}")


# ------------------------------------------------------------------------------------------------ a second method
@pytest.mark.parametrize("dcov,dproba", GRADS, ids=["both", "dcov", "dproba"])
@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "drop"])
def test_reference_gradients_equal_central_differences(drop, dcov, dproba):
    R = 65
    c = H.make_case(R)
    ref = H.head(c, "fp32", drop, dcov, dproba)
    base = {"dy": ("y", torch.from_numpy(ref["y"])), "dW1": ("W1", c.W1), "db1": ("b1", c.b1), "dW2": ("W2", c.W2), "db2": ("b2", c.b2)}
    g = torch.Generator().manual_seed(5)
    worst = {}
    for gname, (pname, value) in base.items():
        value = value.double()
        grad = ref[gname]
        scale = np.abs(grad).max()
        assert scale > 0, gname
        flat = torch.randperm(value.numel(), generator=g)[:8].tolist()
        if gname == "dy":
            flat += [row * H.C + 2 for row in c.extreme] + [3 * H.C + H.ZERO_COL]
        if gname == "dW1":
            flat += [H.DEAD * H.C + 2, 3 * H.C + H.ZERO_COL]
        if gname == "db1":
            flat += [H.DEAD]
        if gname == "dW2":
            flat += [2 * H.HID + H.DEAD]
        err = 0.0
        for i in flat:
            eps = 1e-6 * max(1.0, abs(float(value.view(-1)[i])))
            loss = []
            for sgn in (1.0, -1.0):
                v = value.clone().view(-1)
                v[i] += sgn * eps
                v = v.view(value.shape)
                kw = {"y_in": v} if pname == "y" else {"params": {pname: v}}
                loss.append(H.head(c, "fp32", drop, dcov, dproba, backward=False, **kw)["loss"])
            err = max(err, abs((loss[0] - loss[1]) / (2 * eps) - grad.reshape(-1)[i]) / scale)
        worst[gname] = err
    print(f"R {R} drop {drop} dcov {dcov} dproba {dproba}: reference vs central differences {worst}")
    assert max(worst.values()) < 1e-6, worst


# ------------------------------------------------------------------------------------------------ the identity is exact
@pytest.mark.parametrize("gamma,beta", SWEEP + [(None, None)], ids=lambda v: "-" if v is None else f"{v:.9g}")
@pytest.mark.parametrize("R", H.SUMS_ROWS)
def test_identity_in_fp64_equals_the_row_pass(R, gamma, beta):
    """An algebraic identity in dpre, y = gamma xhat + beta and W1: evaluated in numpy's long double from the fp64 reference's dpre,
    because at |gamma| = 1e-4, beta = 8 the cancellation magnifies even fp64 rounding (1.1e-16 x 8e4 per term) past 1e-12."""
    c = H.make_case(R, gamma, beta)
    L = np.longdouble
    for rows in H.ROWS:
        dpre = H.head(c, rows, True, True, True, exact_affine=True)["dpre"].astype(L)
        g, b, W = c.gamma.double().numpy().astype(L), c.beta.double().numpy().astype(L), c.W1.double().numpy().astype(L)
        xhat = (H.stored(c.f, rows)[:, :H.C].numpy().astype(L) - c.mean.double().numpy().astype(L)) * c.invstd.double().numpy().astype(L)
        y = g * xhat + b
        dW1, db1, dy = dpre.T @ y, dpre.sum(0), dpre @ W
        dg, dbt = (dy * xhat).sum(0), dy.sum(0)
        G = (dW1 - b[None, :] * db1[:, None]) / g[None, :]
        ig, ib = (W * G).sum(0), (W * db1[:, None]).sum(0)
        eg, eb = float(np.abs(ig - dg).max() / np.abs(dg).max()), float(np.abs(ib - dbt).max() / np.abs(dbt).max())
        print(f"R {R} gamma {gamma} beta {beta} {rows}: identity vs row pass: dgamma {eg:.2e}, dbeta {eb:.2e} (bound 1e-12)")
        assert eg <= 1e-12 and eb <= 1e-12
        # the same in plain fp64 through H.identity (what the GPU file's planted inputs are made from): printed
        r = H.head(c, rows, True, True, True, exact_affine=True)
        i64 = H.identity(c, r["dW1"], r["db1"])
        print(f"    in fp64: dgamma {H.rel(i64[0], dg.astype(np.float64)):.2e}, dbeta {H.rel(i64[1], dbt.astype(np.float64)):.2e}")


# ------------------------------------------------------------------------------------------------ masks, edges, e32
@pytest.mark.parametrize("case", ALL_CASES, ids=_id)
def test_no_mask_hangs_on_rounding(case):
    c = H.make_case(*case)
    live = torch.arange(H.HID) != H.DEAD
    masks = []
    for (pre, margin), name in zip(H._pre_variants(c), ("fp64", "fp32", "bf16 rows")):
        room = float((pre[:, live].abs() / margin[:, None]).min())
        assert room >= 1.0, (name, room)
        assert float(pre[:, H.DEAD].max()) <= -1.0 + 1e-3, (name, float(pre[:, H.DEAD].max()))
        masks.append(pre > 0)
    assert torch.equal(masks[0], masks[1]), "the fp32 restatement's ReLU mask is not the fp64 mask"
    assert bool((c.f[:, H.C:] == H.PAD).all())
    assert not bool(c.W1[:, H.ZERO_COL].any())


@pytest.mark.parametrize("case", [k for k in ALL_CASES if k[1] is None], ids=_id)
def test_edge_inputs_and_e32(case):
    R = case[0]
    c = H.make_case(R)
    for rows in H.ROWS:
        ref, r32 = H.reference(R, rows, True), H.reference_fp32(R, rows, True)
        for r in (ref, r32):
            for k, v in r.items():
                assert np.isfinite(v).all(), (rows, k)
        assert not ref["dW1"][H.DEAD].any() and ref["db1"][H.DEAD] == 0 and not ref["dW2"][:, H.DEAD].any()
        assert not ref["dy"][:, H.ZERO_COL].any()
        assert np.array_equal(ref["pre"] > 0, r32["pre"] > 0)
        names = [n for n, _ in H.GRAD_SHAPES] + ["dy", "dgamma", "dbeta"]
        print(f"R {R} {rows} drop: e32 " + ", ".join(f"{n} {H.rel(r32[n], ref[n]):.2e}" for n in names))
    if R >= 8:
        nodrop = H.reference(R, "fp32", False)
        assert len(c.extreme) == 4
        for row, target in c.extreme.items():
            assert abs(nodrop["s"][row, 4] - target) < 0.5, (row, target, nodrop["s"][row, 4])
            assert int(c.keep[row]) == 0xFFFF
        assert max(float(nodrop["proba"][row].max()) for row in c.extreme) >= 1.0 - 1e-12
        drop = H.reference(R, "fp32", True)
        assert all(abs(drop["s"][row, 4]) > 50 for row in c.extreme)


@pytest.mark.parametrize("R", H.SUMS_ROWS)
def test_sweep_e32_and_a_model_of_the_identity(R):
    """Printed, not asserted (a model is not a measurement): e32 of the fp32 row pass, which sets the GPU sweep's bound, and the
    identity evaluated in fp64 from the fp32 restatement's dW1 / db1."""
    for gamma, beta in SWEEP:
        c = H.make_case(R, gamma, beta)
        ref, r32 = H.reference(R, "fp32", True, gamma_ch=gamma, beta_ch=beta), H.reference_fp32(R, "fp32", True, gamma_ch=gamma, beta_ch=beta)
        ig, ib = H.identity(c, r32["dW1"], r32["db1"])
        scale = np.abs(ref["dgamma"]).max()
        e32 = H.rel(r32["dgamma"], ref["dgamma"])
        ch = abs(ig[H.SWEEP_CH] - ref["dgamma"][H.SWEEP_CH]) / scale
        print(f"R {R} gamma {gamma:.9g} beta {beta:g}: fp32 row pass e32 {e32:.2e} -> bound {min(max(1e-5, 8 * e32), 1e-3):.2e}; "
              f"model of the identity: dgamma {H.rel(ig, ref['dgamma']):.2e} (swept channel {ch:.2e}), dbeta {H.rel(ib, ref['dbeta']):.2e}")
