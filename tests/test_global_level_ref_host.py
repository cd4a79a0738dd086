"""What tests/test_gpu_global_level_forward.py rests on, checked where there is no GPU (tests/_global_level_ref.py builds the cases):

  * the fp64 reference against a second statement: torch.nn.Linear + ReLU + BatchNorm1d modules in fp64, the per-plot max and the FP3
    block on [plot feature | x2], in train mode and in eval mode, running statistics and num_batches_tracked included;
  * every live pre-activation of both blocks keeps 2^-15 from zero, with batch and with running statistics, and the fp32
    restatement has the same exact zeros as fp64;
  * every plot has its planted pair (p, q bit-identical, q > p) attaining the signed extremum in at least 4 channels by more than the
    decision bound, its `lone` row attaining it in at least one, and a negative-gamma channel with two or more exactly-zero rows;
    over the cases the pairs sit in one lane's row sequence, in different row quarters, blocks and trips, and on the memory path
    of the max in equal and different residues mod 16; one row per plot sits at the origin;
  * the DEAD channel is dead (zero on every row, batch variance 0) and the OFFSET channel's batch mean / batch std lies in [6, 12];
  * the fp32 restatement stays inside the GPU test's tolerances, and at most 5 % of the (plot, channel) pairs are undecided (top-two
    gap among non-identical rows below the decision bound), counted in the fp64 and in the fp32 restatement;
  * the pool kernels' cases: a h + c is exact in fp32 on the lattice, the planted ties tie, arg entries outside the plot exist, the
    zero column is zero, and the fp32 restatement of the pool backward is within 1e-5 of fp64."""
import numpy as np
import pytest
import torch

import _global_level_ref as G

ALL_SHAPES = G.SHAPES + [G.EXTRA]
_REF = {}


def _ref(B, M2, mode, fp32=False):
    k = (B, M2, mode, fp32)
    if k not in _REF:
        _REF[k] = (G.reference_fp32 if fp32 else G.reference)(G.make_case(B, M2), mode)
    return _REF[k]


@pytest.mark.parametrize("mode", ("train", "eval"))
@pytest.mark.parametrize("B,M2", ALL_SHAPES)
def test_reference_equals_torch_modules(B, M2, mode):
    c = G.make_case(B, M2)
    ref = _ref(B, M2, mode)
    mods = {}
    for name, _, cin in G.BLOCKS:
        p = c.blk[name]
        lin, bn = torch.nn.Linear(cin, 64).double(), torch.nn.BatchNorm1d(64).double()
        with torch.no_grad():
            lin.weight.copy_(p["W"]), lin.bias.copy_(p["b"]), bn.weight.copy_(p["gamma"]), bn.bias.copy_(p["beta"])
            bn.running_mean.copy_(p["rm"]), bn.running_var.copy_(p["rv"])
        assert bn.eps == G.EPS and bn.momentum == G.MOMENTUM
        lin.train(mode == "train"), bn.train(mode == "train")
        mods[name] = (lin, bn)
    with torch.no_grad():
        x2 = c.x2.double()
        h_sa3 = torch.relu(mods["sa3"][0](torch.cat([x2, c.pos2[:, 0:3].double()], 1)))
        y = mods["sa3"][1](h_sa3)
        x3 = y.view(B, M2, 64).max(1).values
        h3 = torch.relu(mods["fp3"][0](torch.cat([x3.repeat_interleave(M2, 0), x2], 1)))
        out = mods["fp3"][1](h3)
    close = lambda a, b: np.testing.assert_allclose(np.asarray(a), np.asarray(b), rtol=1e-11, atol=1e-11)      # noqa: E731
    close(ref["h_sa3"], h_sa3), close(ref["y"], y), close(ref["x3"], x3), close(ref["h3"], h3), close(ref["out"], out)
    # the row the reference names attains the modules' max, and no lower row comes within 1e-11 of it (not "equals": the modules'
    # BLAS product may give the bit-identical rows p and q values one ulp apart, in either order)
    v = y.view(B, M2, 64).numpy()
    at = np.take_along_axis(v, ref["arg3"][:, None, :].astype(np.int64), 1)[:, 0, :]
    close(at, x3)
    lower = np.arange(M2)[None, :, None] < ref["arg3"][:, None, :]
    assert not (lower & (v > at[:, None, :] - 1e-11)).any()
    for name, _, _ in G.BLOCKS:
        bn = mods[name][1]
        close(ref[f"{name}.running_mean"], bn.running_mean), close(ref[f"{name}.running_var"], bn.running_var)
        assert int(bn.num_batches_tracked) == ref["batches"] == (1 if mode == "train" else 0)
        if mode == "eval":
            assert np.array_equal(ref[f"{name}.running_mean"], c.blk[name]["rm"].double().numpy())
            assert np.array_equal(ref[f"{name}.running_var"], c.blk[name]["rv"].double().numpy())
    fr = _ref(B, M2, "frozen")
    if mode == "eval":
        assert np.array_equal(fr["arg3"], ref["arg3"])
        for k in ref:
            if isinstance(ref[k], np.ndarray) and k != "arg3":
                close(fr[k], ref[k])


@pytest.mark.parametrize("B,M2", ALL_SHAPES)
def test_margin_dead_and_offset_channels(B, M2):
    c = G.make_case(B, M2)
    for name, _, _ in G.BLOCKS:
        g = c.blk[name]["gamma"]
        assert bool((g[::5] < 0).all()) and int((g < 0).sum()) == 13 and g[G.DEAD] > 0 and g[G.OFFSET] > 0
    for mode in ("train", "frozen"):
        ref, r32 = _ref(B, M2, mode), _ref(B, M2, mode, fp32=True)
        assert ref["margin"] >= G.MARGIN and r32["margin"] >= G.MARGIN / 2, (ref["margin"], r32["margin"])
        for k in ("h_sa3", "h3"):
            assert np.array_equal(ref[k] == 0, r32[k] == 0), k                            # the same exact zeros
            assert not ref[k][:, G.DEAD].any() and not r32[k][:, G.DEAD].any()            # dead on every row
            assert (ref[k] > 0).mean() > 0.25
        assert np.array_equal(ref["x3"][:, G.DEAD], np.broadcast_to(ref["sa3.c"][G.DEAD], (B,))) and not ref["arg3"][:, G.DEAD].any()
    ref = _ref(B, M2, "train")
    for name, _, _ in G.BLOCKS:
        assert ref[f"{name}.mean"][G.DEAD] == 0.0 and abs(ref[f"{name}.invstd"][G.DEAD] - G.EPS ** -0.5) < 1e-9
        ratio = float(ref[f"{name}.mean"][G.OFFSET] * ref[f"{name}.invstd"][G.OFFSET])
        print(f"B={B} M2={M2} {name}: offset channel batch mean / batch std {ratio:.2f}")
        assert 6.0 <= ratio <= 12.0


@pytest.mark.parametrize("B,M2", ALL_SHAPES)
def test_planted_rows_and_ties(B, M2):
    c = G.make_case(B, M2)
    for b, (p, q, lone, origin) in enumerate(c.plants):
        o = b * M2
        assert p < q and torch.equal(c.x2[o + p], c.x2[o + q]) and torch.equal(c.pos2[o + p], c.pos2[o + q])
        assert not c.pos2[o + origin, 0:3].any() and origin not in (p, q, lone)
        assert int((c.pos2[o:o + M2, 0:3].abs().sum(1) == 0).sum()) == 1
        same = (c.x2[o:o + M2] == c.x2[o + p]).all(1)
        assert int(same.sum()) == 2                                                       # no other copy
    for mode in ("train", "frozen"):
        ref = _ref(B, M2, mode)
        d = G.decisions(c, ref)
        assert np.array_equal(d.first, ref["arg3"])
        h = ref["h_sa3"].reshape(B, M2, 64)
        neg = (c.blk["sa3"]["gamma"] < 0).numpy()
        for b, (p, q, lone, _) in enumerate(c.plants):
            assert int(d.planted[b].sum()) >= 4, (b, int(d.planted[b].sum()))
            assert not (d.first[b] == q).any()                                            # the copy never wins
            if lone is not None:
                assert int(((d.first[b] == lone) & (d.gap[b] > d.bound)).sum()) >= 1, b
            zero_rows = (h[b] == 0).sum(0)
            assert int(((zero_rows >= 2) & neg).sum()) >= 1, b
            # on a negative-gamma channel with a zero row the extremum is that zero: c, at the lowest zero row
            for ch in np.nonzero(neg & (zero_rows >= 1))[0]:
                assert d.zero[b, ch] and d.best[b, ch] == ref["sa3.c"][ch] and d.first[b, ch] == int(np.argmax(h[b, :, ch] == 0))
        print(f"B={B} M2={M2} {mode}: planted pair wins {d.planted.sum(1).min()} ... {d.planted.sum(1).max()} channels per plot, "
              f"exact-zero extrema {d.zero.mean():.2f} of the pairs, decision bound {d.bound:.2e}")


def test_the_pairs_reach_every_position():
    seen = {}
    for (B, M2) in G.SHAPES:
        for p, q, _, _ in G.plants(B, M2):
            for k in G.position(p, q, M2):
                seen.setdefault(k, set()).add((B, M2))
    assert set(seen) == {"lane", "quarter", "block", "trip", "residue-same", "residue-differs"}, seen
    assert G.position(1, 2, 64) == {"lane"} and G.position(6, 54, 64) == {"lane"} and G.position(1, 5, 64) == {"quarter"}
    assert G.position(3, 64, 65) == {"block"} and G.position(5, 256, 257) == {"trip", "residue-differs"}
    assert G.position(16, 32, 257) == {"lane", "residue-same"}
    # the register path of the max (one trip) sees lanes, quarters and blocks; the memory path trips and both residue kinds
    assert any(M2 <= 256 for k in ("lane", "quarter", "block") for (_, M2) in seen[k])
    assert all(M2 > 256 for (_, M2) in seen["trip"])
    # the shapes: one partial block | exactly one | a block of one row | the register path's last | the memory path's first |
    # three trips | the plot limit
    assert [(-(-M2 // 64), -(-M2 // 256)) for _, M2 in G.SHAPES] == [(1, 1), (1, 1), (2, 1), (4, 1), (5, 2), (10, 3), (1, 1)]
    assert max(B for B, _ in G.SHAPES) == 28 and G.EXTRA[0] == 29


@pytest.mark.parametrize("mode", ("train", "frozen"))
@pytest.mark.parametrize("B,M2", ALL_SHAPES)
def test_fp32_restatement_and_undecided_share(B, M2, mode):
    c = G.make_case(B, M2)
    ref, r32 = _ref(B, M2, mode), _ref(B, M2, mode, fp32=True)
    bad = G.show(f"B={B} M2={M2} {mode}: fp32 restatement vs fp64", G.distances(r32, ref))
    assert not bad, bad
    d, d32 = G.decisions(c, ref), G.decisions(c, r32)
    print(f"B={B} M2={M2} {mode}: undecided (plot, channel) pairs {d.undecided_share:.4f} (fp64), {d32.undecided_share:.4f} (fp32 restatement)")
    assert d.undecided_share <= 0.05 and d32.undecided_share <= 0.05
    # where fp64 decides, the fp32 restatement names the same row
    assert np.array_equal(r32["arg3"][d.decided], ref["arg3"][d.decided])


# ------------------------------------------------------------------------------------------------ the pool kernels' cases
@pytest.mark.parametrize("C", G.MAX_C)
@pytest.mark.parametrize("R", G.MAX_R)
def test_max_cases_are_exact_and_tied(R, C):
    m = G.max_case(3, R, C)
    assert m.hs == (64 if C == 64 else 36) and m.G == (4 if C == 64 else 7) and 256 - m.G * C == (0 if C == 64 else 18)
    h = m.h.reshape(3, R, m.hs)
    lat = h[:, :, :C]
    assert np.array_equal(lat * 8, np.round(lat * 8)) and np.abs(lat).max() <= 4.0
    assert (m.a < 0).any() and (m.a > 0).any() and m.a[4] == 0 and not m.arg[:, 4].any() and not m.arg[:, 3].any()
    for b in range(3):
        r0 = (2 + b) % R
        assert m.arg[b, 1] == r0 and m.arg[b, 2] == r0
        if r0 + m.G < R:
            assert m.y[b, r0 + m.G, 1] == m.y[b, r0, 1]                                   # one thread's row sequence
        if r0 + 1 < R:
            assert m.y[b, r0 + 1, 2] == m.y[b, r0, 2]                                     # neighbouring row groups
    ties = int(((m.y == m.out[:, None, :]).sum(1) > 1).sum())
    print(f"R={R} C={C}: {ties} of {3 * C} (plot, channel) pairs have tied maxima")
    assert R == 1 or ties >= 6
    mb = G.max_backward_case(3, R, C)
    assert (mb.arg == -1).any() and (mb.arg == R).any() and mb.written == 3 * (C - 2)
    assert int((mb.dy != mb.dy0).sum()) == mb.written and np.all(mb.dy[3 * R:] == G.PAD) and np.all(mb.dy[:, C:] == G.PAD)


@pytest.mark.parametrize("B", G.POOL_B)
@pytest.mark.parametrize("R", G.POOL_R)
def test_pool_backward_cases(B, R):
    for stride in G.POOL_STRIDES:
        m = G.pool_backward_case(B, R, stride)
        assert m.du.shape == (B * R, stride) and not m.du[:R, m.ZERO_CH].any() and m.dx0[0, m.ZERO_CH] == 0 and m.ref["dx"][0, m.ZERO_CH] == 0
        assert int((m.dx0 == 0).sum()) == 1 and (m.dgamma0 != 0).all() and (m.dbeta0 != 0).all()
        assert m.arg.min() == 0 and m.arg.max() == R - 1
        # the header's formulas, term by term in plain Python floats, on a few channels
        for ch in (0, m.ZERO_CH, 63):
            dx = [float(m.dx0[b, ch]) + sum(float(v) for v in m.du[b * R:(b + 1) * R, ch]) for b in range(B)]
            xh = [(float(m.h[b * R + m.arg[b, ch], ch]) - float(m.mean[ch])) * float(m.invstd[ch]) for b in range(B)]
            assert np.allclose(dx, m.ref["dx"][:, ch], rtol=1e-12, atol=1e-12)
            assert abs(float(m.dbeta0[ch]) + sum(dx) - m.ref["dbeta"][ch]) < 1e-11
            assert abs(float(m.dgamma0[ch]) + sum(d * x for d, x in zip(dx, xh)) - m.ref["dgamma"][ch]) < 1e-11
        for n in ("dx", "dgamma", "dbeta"):
            e = float(np.abs(m.r32[n].astype(np.float64) - m.ref[n]).max() / np.abs(m.ref[n]).max())
            assert e < 1e-5, (n, e)
