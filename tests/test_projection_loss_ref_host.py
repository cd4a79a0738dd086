"""What tests/test_gpu_projection_loss.py rests on, proven on the CPU (tests/_projection_loss_ref.py):
  * the fp64 reference IS the pinned oracle (oracle/projection.py, oracle/losses.py in fp64, their autograd gradients to 1e-12,
    P.scatter_max's arg-max exactly) on ragged_cells and two_slices, for all four (m, e) pairs;
  * the cases are not vacuous: empty cells, arg-max points in every channel, nocc = 2025, ties that straddle the slices and are
    won by the earlier point, exact dyadic sums;
  * six wrong restatements of the rule, written in numpy over the kernels' 64-bit keys and slices, DIFFER from the reference on
    the cases that were planted for them (and the right restatement does not);
  * the fp32 restatement keeps every bound the GPU file sets (a bound it cannot keep would be a defect of the case); its
    distance from fp64, `e32`, is printed per case and output (run with -s).
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _projection_loss_ref as R
from oracle import losses, primitives as P, projection

F64, F32 = np.float64, np.float32
MULTI = [n for n, s in R.SHAPES.items() if R.key_parts(s[1]) > 1]          # full_grid, two_slices, clamped
CASES = R.case_ids()
IDS = [f"{n}-{f}" for n, f in CASES]


# ------------------------------------------------------------------------------------------------ against the pinned oracle
@pytest.mark.parametrize("m,e", R.ME, ids=[f"m{m}-e{e}" for m, e in R.ME])
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("name", R.ALL_ME)
def test_reference_is_the_pinned_oracle(name, family, m, e, monkeypatch):
    c, r = R.case(name, family), R.ref(name, family, m, e)
    B, N, D = c.B, c.N, c.D
    if c.cloud is None:            # planted ids: the oracle is handed them in place of its own index arithmetic
        ids = torch.from_numpy(np.stack([c.pix.reshape(B, N) // D, c.pix.reshape(B, N) % D], 1).astype(np.int32))
        monkeypatch.setattr(projection, "p2_pixel_ids", lambda clouds, diam_pix: ids)
        cloud = torch.zeros(B, 2, N)
    else:
        cloud = torch.from_numpy(c.cloud.copy())
    cov = torch.tensor(c.cov, dtype=torch.float64, requires_grad=True)
    proba = torch.tensor(c.proba_for(m), dtype=torch.float64, requires_grad=True)
    gt, pdf = torch.tensor(c.gt), torch.tensor(c.pdf)
    pred = projection.project_to_plotwise_coverages(cov, cloud, SimpleNamespace(diam_pix=D))
    if m != 0.0 and e != 0.0:
        total, (l_abs, l_nll, l_ent) = losses.total_loss(pred, proba, gt, pdf, m, e)
    else:                          # a term that is switched off is skipped, not multiplied by zero
        zero = torch.zeros((), dtype=torch.float64)
        l_abs = losses.absolute_loss(pred, gt)
        l_nll = losses.nll_loss(proba, pdf) if m != 0.0 else zero
        l_ent = losses.entropy_loss(proba) if e != 0.0 else zero
        total = l_abs + m * l_nll + e * l_ent
    pred.retain_grad()
    (R.G * total).backward()
    got = dict(pred=r["pred"], out=r["out"], dpred=r["dpred"], dcov=r["dcov"], dproba=r["dproba"])
    want = dict(pred=pred.detach().numpy(), out=np.array([float(x.detach()) for x in (total, l_abs, l_nll, l_ent)]),
                dpred=pred.grad.numpy(), dcov=cov.grad.numpy(), dproba=np.zeros((c.R, 4)) if proba.grad is None else proba.grad.numpy())
    for k in got:
        d = R.dist(got[k], want[k])
        print(f"{name}-{family} m={m} e={e} {k}: {d:.2e} (bound 1e-12)")
        assert d <= 1e-12, k
    # the per-plot columns: every plot as a batch of one
    for b in (0, B - 1):
        rows = slice(b * N, (b + 1) * N)
        pb, qb = torch.tensor(r["pred"][b:b + 1]), torch.tensor(c.proba_for(m)[rows], dtype=torch.float64)
        la = float(losses.absolute_loss(pb, gt[b:b + 1]))
        ln = float(losses.nll_loss(qb, pdf[rows])) if m != 0.0 else 0.0
        le = float(losses.entropy_loss(qb)) if e != 0.0 else 0.0
        strata = ((pb[0, list(R.CHANNELS)] - gt[b, list(R.CHANNELS)]) ** 2 + R.EPS).sqrt().numpy()
        assert R.dist(r["plots"][b], np.concatenate([[la + m * ln + e * le, la, ln, le], strata])) <= 1e-12
    if family == "dyadic":
        cell = torch.from_numpy((np.arange(B)[:, None] * D * D + c.pix.reshape(B, N)).reshape(-1).astype(np.int64))
        _, arg = P.scatter_max(torch.from_numpy(c.cov.copy()).t(), cell, dim=-1, dim_size=B * D * D)      # (4, B*D*D), global ids
        arg = arg.view(4, B, D * D).numpy()
        local = np.where(arg == B * N, -1, arg - np.arange(B)[None, :, None] * N)
        assert np.array_equal(local[list(R.CHANNELS)].transpose(1, 2, 0), r["arg"])


def test_raster_reference_is_the_pinned_oracle():
    for family in R.FAMILIES:
        c = R.case("ragged_cells", family)
        ref = R.raster(c.cov, c.cell1, c.B, c.N, c.D)
        args = SimpleNamespace(diam_pix=c.D, diam_meters=c.diam_meters)
        for b in range(c.B):
            want = projection.project_to_2d_rasters(torch.from_numpy(c.cloud[b].copy()),
                                                    torch.from_numpy(c.cov.reshape(c.B, c.N, 4)[b].T.copy()), args)
            assert np.array_equal(np.isnan(ref[b]), np.isnan(want)) and np.isnan(want).any() and not np.isnan(want).all()
            assert np.array_equal(np.nan_to_num(ref[b]).astype(F64), np.nan_to_num(want))


# ------------------------------------------------------------------------------------------------ counts on the reference
@pytest.mark.parametrize("name,family", CASES, ids=IDS)
def test_cases_are_not_vacuous(name, family):
    c, r = R.case(name, family), R.ref(name, family)
    B, N, D = c.B, c.N, c.D
    assert r["nocc"].min() >= 1 and (r["arg"] >= 0).any(axis=(0, 1)).all()            # arg-max points in every channel
    for b in range(B):
        full = name == "one_point_d1" or (name == "full_grid" and b == 2)
        assert (r["nocc"][b] == D * D) == full, "empty cells everywhere but where the case says otherwise"
        assert ((r["arg"][b] == -1).all(1) == (r["arg"][b] == -1).any(1)).all()
    if name == "full_grid":
        assert r["nocc"].tolist()[1:] == [1, 2025] and (c.pix.reshape(B, N)[1] == D * D - 1).all()
    # gradient lands exactly on the arg-max points, one per occupied cell and channel
    for k, ch in enumerate(R.CHANNELS):
        assert np.count_nonzero(r["dcov"][:, ch]) == int((r["arg"][:, :, k] >= 0).sum())
    assert not r["dcov"][:, 1].any()
    assert (c.proba[:, 2:] == 0).any() and (c.proba[:, 2:] == 1).any() and (c.R <= 3 or not c.proba_zero[3].any())
    if c.R >= 8:
        assert (c.pdf < 1e-29).any() and (c.pdf < 1e-59).any()
    if family == "dyadic":
        assert (c.cov < 0).any() and (np.abs(c.cov * 8) == np.floor(np.abs(c.cov * 8))).all()
        r32 = R.ref(name, family, f32=True)
        assert np.array_equal(r32["pred"], r["pred"].astype(F32)), "dyadic sums are exact: one correctly rounded quotient"


@pytest.mark.parametrize("name", MULTI)
def test_planted_ties_straddle_the_slices_and_the_earlier_point_wins(name):
    c, r = R.case(name, "dyadic"), R.ref(name, "dyadic")
    B, N, D = c.B, c.N, c.D
    pix, cov = c.pix.reshape(B, N), c.cov.reshape(B, N, 4)
    n = np.arange(N)
    for b in range(B):
        want = 8 if not (name == "full_grid" and b > 0) else 1
        for parts in (R.key_parts(N), R.loss_slices(N)):
            sl = R.slice_of(n, N, parts)
            found = 0
            for cell in np.unique(pix[b]):
                pts = n[pix[b] == cell]
                ok = True
                for k, ch in enumerate(R.CHANNELS):
                    top = pts[cov[b, pts, ch] == r["mx"][b, cell, k]]
                    ok &= len(np.unique(sl[top])) > 1 and r["arg"][b, cell, k] == top.min() and sl[top.min()] < sl[top.max()]
                found += bool(ok)
                if found == want:
                    break
            assert found == want, (b, parts, found)
        i, j = n[:-1024], n[1024:]
        lane = (pix[b, i] == pix[b, j]) & (cov[b, i, 0] == 1) & (cov[b, j, 0] == 1)
        for parts in (R.key_parts(N), R.loss_slices(N)):
            lane &= R.slice_of(i, N, parts) == R.slice_of(j, N, parts)
        assert lane.any(), "a tie at n and n + 1024 of one slice"


# ------------------------------------------------------------------------------------------------ wrong restatements
def keyed(cov, pix, B, N, D, parts, last_wins=False, skip_last_slice=False, drop_last_row=False, mean_all=False):
    """The kernels' own formulation in numpy: 64-bit keys (ordered(value) << 32 | tag), one table per slice, the maximum of the
    slices' maxima -- with four ways of getting it wrong.  -> arg (B, D*D, 3), nocc (B,), pred (B, 4) fp64"""
    DD, per = D * D, -(-N // parts)
    n = np.tile(np.arange(N, dtype=np.uint64), B)
    b = np.repeat(np.arange(B), N)
    sl = (n // np.uint64(per)).astype(np.int64)
    keep = np.ones(B * N, bool)
    if drop_last_row:
        keep &= n.astype(np.int64) != np.minimum(N, (sl + 1) * per) - 1
    if skip_last_slice and parts > 1:
        keep &= sl != parts - 1
    idx = ((b * parts + sl) * DD + pix.astype(np.int64))[keep]
    tag = (n if last_wins else np.uint64(0xFFFFFFFF) - n)[keep]
    arg, val = np.empty((B, DD, 3), np.int64), np.empty((B, DD, 3))
    for k, ch in enumerate(R.CHANNELS):
        u = np.ascontiguousarray(cov[:, ch]).view(np.uint32)[keep]
        o = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint64)
        tab = np.zeros(B * parts * DD, np.uint64)
        np.maximum.at(tab, idx, (o << np.uint64(32)) | tag)
        key = tab.reshape(B, parts, DD).max(1)
        t = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
        arg[:, :, k] = np.where(key == 0, -1, t if last_wins else 0xFFFFFFFF - t)
        o = (key >> np.uint64(32)).astype(np.uint32)
        val[:, :, k] = np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32).view(F32)
    occ = arg[:, :, 0] >= 0
    nocc = occ.sum(1)
    v = np.where(occ[:, :, None], val, 0.0)
    den = np.full(B, float(DD)) if mean_all else np.maximum(nocc, 1)
    pred = np.stack([v[:, :, 0].sum(1), (occ - v[:, :, 0]).sum(1), v[:, :, 1].sum(1), v[:, :, 2].sum(1)], 1) / den[:, None]
    return arg, nocc, pred


def _same(k, r):
    return np.array_equal(k[0], r["arg"]) and np.array_equal(k[1], r["nocc"]) and np.abs(k[2] - r["pred"]).max() <= 1e-12


@pytest.mark.parametrize("name,family", CASES, ids=IDS)
def test_wrong_projections_differ_from_the_reference(name, family):
    c, r = R.case(name, family), R.ref(name, family)
    a = (c.cov, c.pix, c.B, c.N, c.D)
    for parts in sorted({1, R.key_parts(c.N), R.loss_slices(c.N)}):
        assert _same(keyed(*a, parts), r), "the keys and slices, stated right, are the reference"
        if family == "dyadic" and c.N >= 64:
            assert not np.array_equal(keyed(*a, parts, last_wins=True)[0], r["arg"]), "last point wins"
        if parts > 1:
            k = keyed(*a, parts, skip_last_slice=True)
            assert not np.array_equal(k[0], r["arg"]), "last slice left out"
            if name != "full_grid":
                assert not np.array_equal(k[1], r["nocc"]), "last slice left out: the cell only it holds"
        if parts > 1 and name != "full_grid" or c.N == 1:
            k = keyed(*a, parts, drop_last_row=True)
            assert not np.array_equal(k[1], r["nocc"]), "last row of every slice dropped"
    if name != "one_point_d1":
        k = keyed(*a, 1, mean_all=True)
        assert np.abs(k[2] - r["pred"]).max() > 1e-6, "mean over all cells"


@pytest.mark.parametrize("name,family", CASES, ids=IDS)
def test_wrong_loss_terms_differ_from_the_reference(name, family):
    c, r = R.case(name, family), R.ref(name, family)
    m, e = R.ME[0]
    p = c.proba[:, 2:].astype(F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = -(p * np.log(p) + (1 - p) * np.log(1 - p + R.EPS)).sum() / (2.0 * c.R)          # eps missing from one logarithm
        assert not abs(ent - r["out"][3]) <= 1e-6, "exact zeros are there to see it"
        if c.R >= 8:
            f = c.pdf.astype(F32)                                                            # the likelihood formed in fp32
            lik = (c.proba[:, 0] + c.proba[:, 1]) * f[:, 0] + c.proba[:, 2] * f[:, 1] + c.proba[:, 3] * f[:, 2]
            nll = float((-np.log(lik.astype(F64))).sum() / c.R)
            assert not abs(nll - r["out"][2]) <= 1e-6 * max(1.0, abs(r["out"][2])), "densities of 1e-60 are there to see it"


# ------------------------------------------------------------------------------------------------ e32
@pytest.mark.parametrize("name,family", CASES, ids=IDS)
def test_fp32_restatement_keeps_the_bounds_of_the_gpu_file(name, family):
    c = R.case(name, family)
    for m, e in R.me_of(name):
        r, r32 = R.ref(name, family, m, e), R.ref(name, family, m, e, f32=True)
        assert np.array_equal(r32["arg"], r["arg"]) and np.array_equal(r32["nocc"], r["nocc"])
        e_pred = float(np.abs(r32["pred"].astype(F64) - r["pred"]).max())
        e_out = float((np.abs(r32["out"] - r["out"]) / np.maximum(1.0, np.abs(r["out"]))).max())
        e_plots = float((np.abs(r32["plots"] - r["plots"]) / np.maximum(1.0, np.abs(r["plots"]))).max())
        b64, b32 = R.ref_backward(name, family, m, e), R.ref_backward(name, family, m, e, f32=True)
        e_grad = {k: R.dist(b32[i], b64[i]) for i, k in ((1, "dpred"), (2, "dcov"), (3, "dproba"))}
        through = R.dist(r32["dcov"], r["dcov"])        # through a forward that rounds pred: not what the backward is judged on
        print(f"e32 {name}-{family} m={m} e={e}: pred {e_pred:.2e}  out {e_out:.2e}  plots {e_plots:.2e}  " +
              "  ".join(f"{k} {v:.2e}" for k, v in e_grad.items()) + f"  (dcov through a rounded pred {through:.2e})")
        assert e_pred <= 1e-6 and e_out <= 1e-6 and e_plots <= 1e-6
        assert all(8 * v <= 1e-5 for v in e_grad.values())
        if m == 0.0:
            assert r["out"][2] == 0.0 and not r["plots"][:, 2].any() and not r["dproba"][:, :2].any()
        if e == 0.0:
            assert r["out"][3] == 0.0 and not r["plots"][:, 3].any()
        if m == 0.0 and e == 0.0:
            assert not r["dproba"].any() and r["out"][0] == r["out"][1]
