"""What tests/test_gpu_sa_modules.py rests on, checked where there is no GPU (tests/_sa_module_ref.py builds the cases):

  * the one-block cases are EXACT: h in fp32 -- as x W^T + b, with the columns permuted, accumulated term by term in reverse --
    equals h in fp64 bit for bit, and inputs and weights survive a bfloat16 round trip: a kernel's extremum and slot can be
    compared with torch.equal, fp32 and bf16 operands alike;
  * the planted ties are there: per item class, (centroid, channel) pairs whose POSITIVE signed extremum is attained by more than
    one slot (at least 16 per class in layout A), and tied pairs across slots 15/16, 63/64, the halves of an OCT half tile and the
    ends of a HEX quarter tile;
  * the wrong variants differ in exactly what the GPU test compares bit for bit: "last" moves `arg` on every planted pair (and the
    feature gradient of both rows), "unsigned" moves `ext` on negative-gamma channels;
  * sa1 (continuous inputs): the extremum leads the runner-up by at least 64 fp32 ulps of the channel's magnitude everywhere, so
    fp32 rounding cannot move a slot;
  * the reference against torch autograd over a dense formulation (a Python loop with `max` per centroid); classes()."""
import numpy as np
import pytest
import torch

import _sa_module_ref as R

EXACT_KINDS, LAYOUTS = ("sa2", "sa3"), ("A", "B", "C")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", EXACT_KINDS)
def test_one_block_cases_are_exact_in_fp32_and_bf16(kind, layout):
    case = R.case_of(kind, layout)
    cen, slot, src, _ = R.messages(case)
    cf, p = case.cf, case.params[0]
    h64 = R.reference(case, "train")["h"]
    x = torch.cat([case.rows[src, :cf], case.rows[src, cf:cf + 3] - case.cpos[cen, 0:3]], 1)
    W, b = p["W"], p["b"]
    assert x.dtype == torch.float32 and W.dtype == torch.float32
    direct = torch.relu(x @ W.t() + b)
    perm = torch.randperm(x.shape[1], generator=torch.Generator().manual_seed(3))
    permuted = torch.relu(x[:, perm] @ W[:, perm].t() + b)
    acc = torch.zeros(x.shape[0], W.shape[0])
    for k in reversed(range(x.shape[1])):
        acc = acc + x[:, k:k + 1] * W[None, :, k]
    reverse = torch.relu(acc + b)
    for name, h in (("x W^T + b", direct), ("columns permuted", permuted), ("term by term, reversed", reverse)):
        assert np.array_equal(h.numpy().astype(np.float64), h64), name
    for name, t in (("x", x), ("W", W), ("features", case.rows[:, :cf]), ("positions", case.rows[:, cf:cf + 3]), ("centroids", case.cpos)):
        assert torch.equal(t.to(torch.bfloat16).to(torch.float32), t), name
    print(f"{kind} {layout}: {x.shape[0]} messages, max |h| {h64.max():.4f}, {100 * (h64 > 0).mean():.0f} % of the activations positive")
    assert 0.25 < (h64 > 0).mean() < 0.75 and h64.max() < 2.0 ** 10


def _slots_tied(att, i, s1, s2):
    return att[i, s1] & att[i, s2]                                    # per channel


@pytest.mark.parametrize("kind", EXACT_KINDS)
def test_ties_are_really_there(kind):
    borders = {"15/16": 0, "63/64": 0, "OCT halves": 0, "HEX ends": 0}
    for layout in LAYOUTS:
        case = R.case_of(kind, layout)
        ref = R.reference(case, "train")
        n, att = R.tied_positive(case, ref)
        cls = R.classes(case.cnt.numpy())
        counts = {c: int((n[cls == c] > 1).sum()) for c in R.CLASS_NAMES[:4] if (cls == c).any()}
        print(f"{kind} {layout}: (centroid, channel) pairs with a tied positive extremum per class: {counts}")
        for c, v in counts.items():
            assert v >= (16 if layout == "A" else 1), (layout, c, v)
        if layout == "A":
            assert set(counts) == set(R.CLASS_NAMES[:4])
            for i, s1, s2 in case.planted:
                live = int(_slots_tied(att, i, s1, s2).sum())
                if (s1, s2) == (15, 16):
                    borders["15/16"] += live
                if (s1, s2) == (63, 64):
                    borders["63/64"] += live
                if cls[i] == "OCT" and s1 < 4 <= s2:
                    borders["OCT halves"] += live
                if cls[i] == "HEX" and (s1, s2) == (0, 3):
                    borders["HEX ends"] += live
        # the lowest of the tied slots is what the reference names
        i, c = np.nonzero(n > 1)
        first = att[i, :, c].argmax(1)
        assert np.array_equal(ref["arg"][i, c], first)
    print(f"{kind} A: tied (centroid, channel) pairs across {borders}")
    assert all(v >= 1 for v in borders.values()), borders


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", EXACT_KINDS)
def test_wrong_variants_differ(kind, layout):
    case = R.case_of(kind, layout)
    ref = R.reference(case, "train", case.dout)
    _, att = R.tied_positive(case, ref)
    last = R.reference(case, "train", case.dout, rule="last")
    assert np.array_equal(last["ext"], ref["ext"])                     # the same value, another slot
    assert len(case.planted) >= 3
    for i, s1, s2 in case.planted:
        ch = np.nonzero(_slots_tied(att, i, s1, s2))[0]
        assert ch.size, ("a planted pair that is nowhere the extremum", i, s1, s2)
        lowest = ch[ref["arg"][i, ch] == s1]                           # (a strong row may stand at a lower slot as well)
        assert lowest.size, (i, s1, s2)
        assert (last["arg"][i, lowest] > ref["arg"][i, lowest]).all(), (i, s1, s2)
        base = (i // case.M) * case.Nsrc
        for s in (s1, s2):
            r = base + int(case.nbr[i, s])
            assert np.abs(last["dfeat"][r] - ref["dfeat"][r]).max() > 1e-6 * np.abs(ref["dfeat"]).max(), (i, s)
    changed = int((last["arg"] != ref["arg"]).sum())
    unsigned = R.reference(case, "train", case.dout, rule="unsigned")
    neg = case.params[-1]["gamma"].numpy() < 0
    many = case.cnt.numpy() > 1
    moved = unsigned["ext"][many][:, neg] != ref["ext"][many][:, neg]
    print(f"{kind} {layout}: 'last' moves {changed} slots; 'unsigned' moves {int(moved.sum())} of {moved.size} extrema on negative-gamma channels")
    assert moved.mean() > 0.5
    assert np.array_equal(unsigned["ext"][:, ~neg], ref["ext"][:, ~neg])


MARGIN = 64 * 2.0 ** -24


@pytest.mark.parametrize("layout", ("A", "C"))
def test_sa1_extremum_leads_by_a_margin(layout):
    case = R.case_of("sa1", layout)
    cen, slot, _, _ = R.messages(case)
    h = R.reference(case, "train")["h"]
    C = h.shape[1]
    sgn = np.where(case.params[-1]["gamma"].numpy() < 0, -1.0, 1.0)
    S = np.full((case.B * case.M, case.cap, C), -np.inf)
    S[cen.numpy(), slot.numpy()] = sgn * h
    top = -np.sort(-S, axis=1)[:, :2]                                  # best, runner-up
    counted = (case.cnt.numpy() >= 2)[:, None] & ~((top[:, 0] == 0) & (top[:, 1] == 0))
    with np.errstate(invalid="ignore"):                                # (-inf - -inf where a centroid has fewer than two messages)
        margin = (top[:, 0] - top[:, 1]) / np.abs(h).max(0)[None, :]
    worst = margin[counted].min()
    print(f"sa1 {layout}: smallest margin of the signed extremum {worst:.2e} of the channel's magnitude over {int(counted.sum())} "
          f"(centroid, channel) pairs; required {MARGIN:.2e}")
    assert counted.sum() > 100 and worst >= MARGIN


def _dense(case, mode):
    """torch autograd over a dense formulation: BatchNorm outputs of all messages, then `max` per centroid in a Python loop."""
    f64 = torch.float64
    cen, _, src, _ = R.messages(case)
    cf = case.cf
    feat = case.rows[:, :cf].to(f64).clone().requires_grad_(True)
    q = [{k: v.to(f64).clone().requires_grad_(k in ("W", "b", "gamma", "beta")) for k, v in p.items()} for p in case.params]
    x = torch.cat([feat[src], case.rows[src, cf:cf + 3].to(f64) - case.cpos[cen, 0:3].to(f64)], 1)
    for p in q:
        h = torch.relu(torch.nn.functional.linear(x, p["W"], p["b"]))
        x = torch.nn.functional.batch_norm(h, p["rm"].clone(), p["rv"].clone(), p["gamma"], p["beta"], mode == "train", 0.1, 1e-5)
    rows = []
    for i in range(case.B * case.M):
        idx = (cen == i).nonzero()[:, 0]
        rows.append(x[idx].max(0).values if idx.numel() else torch.zeros(x.shape[1], dtype=f64))
    out = torch.stack(rows)
    (out * case.dout.to(f64)).sum().backward()
    g = {"out": out.detach().numpy(), "dfeat": (case.dfeat0.to(f64) + feat.grad).numpy()}
    for k, p in enumerate(q):
        for n, key in (("dW", "W"), ("db", "b"), ("dgamma", "gamma"), ("dbeta", "beta")):
            g[f"{n}{k}"] = p[key].grad.numpy()
    return g


@pytest.mark.parametrize("mode", ("train", "frozen"))
@pytest.mark.parametrize("layout", ("A", "C"))
def test_reference_against_dense_autograd(layout, mode):
    case = R.case_of("sa1", layout)                            # continuous inputs: no ties (the margin test)
    ref, dense = R.reference(case, mode, case.dout), _dense(case, mode)
    for n in ("out", "dfeat") + R.grad_names(case):
        scale = np.abs(dense[n]).max()
        e = np.abs(ref[n] - dense[n]).max() / scale
        print(f"sa1 {layout} {mode} {n}: reference vs dense autograd {e:.1e}")
        assert scale > 0 and e < 1e-12, n


def test_running_statistics_follow_torch():
    case = R.case_of("sa2", "A")
    cen, _, src, _ = R.messages(case)
    cf, p = case.cf, case.params[0]
    x = torch.cat([case.rows[src, :cf], case.rows[src, cf:cf + 3] - case.cpos[cen, 0:3]], 1).double()
    bn = torch.nn.BatchNorm1d(p["W"].shape[0]).double()
    with torch.no_grad():
        bn.running_mean.copy_(p["rm"]), bn.running_var.copy_(p["rv"])
    bn(torch.relu(x @ p["W"].double().t() + p["b"].double()))
    ref = R.reference(case, "train")
    assert np.allclose(ref["running_mean"][0], bn.running_mean.numpy(), rtol=1e-13, atol=0)
    assert np.allclose(ref["running_var"][0], bn.running_var.numpy(), rtol=1e-13, atol=0)
    assert ref["batches"] == 1 and R.reference(case, "frozen")["batches"] == 0
    for mode in ("frozen", "eval"):
        kept = R.reference(case, mode)
        assert np.array_equal(kept["running_mean"][0], p["rm"].double().numpy()) and np.array_equal(kept["running_var"][0], p["rv"].double().numpy())


def test_classes_reproduce_the_planted_counts():
    assert R.thresholds() == (4, 8, 64)
    assert list(R.classes([0, 1, 4, 5, 8, 9, 64, 65, 150])) == ["EMPTY", "HEX", "HEX", "OCT", "OCT", "QUAD", "QUAD", "SOLO", "SOLO"]
    for kind in ("sa1",) + EXACT_KINDS:
        a = R.case_of(kind, "A")
        cnt = a.cnt.numpy().reshape(a.B, a.M)
        for b in range(a.B):
            assert set(R.SPECIAL_A) <= set(cnt[b].tolist())
        assert set(R.classes(a.cnt.numpy())) == set(R.CLASS_NAMES)
        assert a.M % 4 == 1                                            # a short last quad
        bb = R.case_of(kind, "B")
        assert set(R.classes(bb.cnt.numpy())) == {"SOLO"} and bb.cnt.max() <= bb.cap and bb.B * bb.M == 48
        c = R.case_of(kind, "C")
        cls = R.classes(c.cnt.numpy()).reshape(c.B, c.M)
        assert set(cls[R.EMPTY_QUAD_PLOT, 4:8]) == {"EMPTY"}
        assert c.B == 33 and set(cls[5]) == {"HEX"} and set(cls[6]) == {"QUAD"} and {"EMPTY", "HEX", "OCT", "QUAD"} <= set(cls[32])
        for case in (a, bb, c):
            nbr, n = case.nbr.numpy(), case.cnt.numpy()
            assert nbr.min() >= 0 and nbr.max() < case.Nsrc - R.UNLISTED
            for i in range(case.B * case.M):
                assert (np.diff(nbr[i, :n[i]]) > 0).all() and not nbr[i, n[i]:].any()
            assert case.rows.shape[1] % 4 == 0 and bool((case.dfeat0 != 0).all())
