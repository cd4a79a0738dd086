"""sn2_cv_indicators (csrc/indicators.hip) through `hip_ops.cv_indicators` and `cross_validation.indicators`, held to the numpy fp64
restatement of tests/_cv_indicators_ref.py (which tests/test_cv_indicators_host.py holds to the reference's own code): the rows
and classes bit for bit, counts and confusions exactly, the means to the re-association of an fp64 sum.

Shapes: P = 1 (one thread), 1023 / 1024 / 1025 (the slice edge of SN2_CV_SLICE_PLOTS = 1024: one slice, a full one, a second slice of
one plot), 5000 (five slices, the last short).  The random table holds exact ties (0.05, 0.625) as ground truths, NaN predictions
and zeros; the planted table every border from both sides."""
import math

import numpy as np
import pytest
import torch

import _cv_indicators_ref as R
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
from stratanet2_vegetation_coverage_maps_amd.cross_validation import COLUMNS, CONTINUOUS_COLUMNS, indicators

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P_MAX = 5000
# an fp64 sum of at most 5000 non-negative terms of at most 1.05, in ANY order, errs by less than (P-1) 2^-53 sum <= 2.92e-9;
# the mean by less than 5.9e-13 (both sides: the kernel's order and fsum's exact sum rounded once)
MEAN_TOL = 1e-12


@pytest.fixture(scope="module")
def table():
    """(pred, gt) of P_MAX plots and the restatement of every prefix used, computed once."""
    pred, gt = R.random_table(P_MAX, 5, ties=True)
    pred[17::97, 0] = np.nan
    pred[500::811] = np.nan                                       # whole rows
    ref = {}

    def want(P, relabel):
        if (P, relabel) not in ref:
            ref[P, relabel] = R.indicators(pred[:P], gt[:P], relabel)
        return ref[P, relabel]
    return pred, gt, want


def _run(pred, gt, relabel):
    rows, cls, stats = ops.cv_indicators(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), relabel)
    torch.cuda.synchronize()
    return rows.cpu().numpy(), cls.cpu().numpy(), stats.cpu().numpy()


def _same_bits(a, b):
    """fp64 tables equal bit for bit; a NaN equals a NaN (its payload is no part of the contract)."""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def _check(got, want, P):
    rows, cls, stats = got
    wrows, wcls, wstats = want
    assert rows.shape == (P, 30) and cls.shape == (P, 9) and stats.shape == (R.STATS_DOUBLES,)
    assert _same_bits(rows, wrows)
    assert np.array_equal(cls, wcls)
    assert np.array_equal(stats[30:60], wstats["count"].astype(np.float64))
    assert np.array_equal(stats[60:444].reshape(2, 3, 8, 8), wstats["cm"].astype(np.float64))
    assert stats[444] == wstats["continuous"]
    worst = 0.0
    for c in range(30):
        n = int(wstats["count"][c])
        if n == 0:
            assert stats[c] == 0.0
            continue
        col = wrows[:, c]
        mean = math.fsum(col[~np.isnan(col)]) / n
        worst = max(worst, abs(stats[c] / n - mean))
    print(f"P = {P}: largest |mean - fsum / count| = {worst:.3e}")
    assert worst <= MEAN_TOL


@pytest.mark.parametrize("relabel", [False, True])
@pytest.mark.parametrize("P", [1, 1023, 1024, 1025, P_MAX])
def test_rows_classes_and_sums_equal_the_restatement(table, P, relabel):
    pred, gt, want = table
    _check(_run(pred[:P], gt[:P], relabel), want(P, relabel), P)


@pytest.mark.parametrize("relabel", [False, True])
def test_planted_borders_nan_and_continuous_rows(relabel):
    pred, gt = R.planted_table(continuous=True)
    P = len(pred)
    want = R.indicators(pred, gt, relabel)
    got = _run(pred, gt, relabel)
    _check(got, want, P)
    rows, cls, stats = got
    nan_rows = np.isnan(pred[:, 0])
    assert nan_rows.sum() == 8
    assert np.isnan(rows[nan_rows][:, [0, 3, 4, 10, 13, 14, 20, 23, 24]]).all()               # the NaN stays in its stratum's entries
    assert (rows[nan_rows][:, [5, 15, 25]] == 0).all() and (cls[nan_rows, 3] == 0).all()        # accuracies 0, class 0
    assert stats[30] == P - 8                                                                  # and is counted out of the mean
    rep = indicators(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), relabel)
    if relabel:
        assert stats[444] == 0 and rep.class_based and tuple(rep.means) == COLUMNS
    else:
        assert stats[444] == 2 and np.isnan(rows[-2:, 5:]).all() and not np.isnan(rows[-2:, :5]).any()
        assert stats[35] == P - 2
        assert not rep.class_based and rep.n_continuous == 2 and tuple(rep.means) == CONTINUOUS_COLUMNS
    assert _same_bits(rep.rows(), want[0]) and np.array_equal(rep.classes(), want[1])
    for c, name in enumerate(rep.means):
        assert abs(rep.means[name] - stats[c] / stats[30 + c]) == 0.0
    # pred == 0 against gt == 0: inside class 0 in every version
    zero = np.flatnonzero((pred[:, 0] == 0) & (gt[:, 0] == 0) & (pred[:, 2] == 0) & (gt[:, 2] == 0))[-1]
    assert rows[zero, 0] == 0 and rows[zero, 5] == 1 and rows[zero, 10] == 0 and rows[zero, 15] == 1 and rows[zero, 25] == 1


def test_same_bytes_twice_and_a_row_does_not_depend_on_its_place(table):
    pred, gt, _ = table
    p, g = torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV)
    a = ops.cv_indicators(p, g, True)
    b = ops.cv_indicators(p, g, True)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    # plots 1000 .. 1099 alone, and moved to the end of a table of 1300 plots that straddles a slice edge
    sl = slice(1000, 1100)
    alone = ops.cv_indicators(p[sl].contiguous(), g[sl].contiguous(), True)
    perm = torch.cat([torch.arange(0, 1000), torch.arange(1100, 1300), torch.arange(1000, 1100)]).to(DEV)
    moved = ops.cv_indicators(p[perm].contiguous(), g[perm].contiguous(), True)
    torch.cuda.synchronize()
    for k in (0, 1):
        want = a[k][sl].cpu().numpy().tobytes()
        assert alone[k].cpu().numpy().tobytes() == want and moved[k][1200:].cpu().numpy().tobytes() == want
    # a caller-owned workspace, not initialised: the same bytes
    ws = torch.full((ops.cv_indicators_ws_words(P_MAX) + 8,), -1, dtype=torch.int32, device=DEV)
    c = ops.cv_indicators(p, g, True, ws=ws)
    torch.cuda.synchronize()
    for x, y in zip(a, c):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert (ws[-8:] == -1).all()                                                                   # nothing past the stated size
    with pytest.raises(ValueError):
        ops.cv_indicators(p, g.float(), True)
    with pytest.raises(ValueError):
        ops.cv_indicators(p, g, True, ws=ws[:16])
