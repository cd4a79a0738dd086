"""The cross-validation indicators (include/strata_hip.h: sn2_cv_indicators) restated in numpy fp64, expression for expression as the
header states them: the second statement that the kernel, the golden fixture of the reference's `learning/accuracy.py`
(tests/golden/cv_indicators.npz) and `cross_validation.CrossValReport` are held to.

`wrong=` switches ONE rule to a plausible mistake; tests/test_cv_indicators_host.py checks that each of them is seen on the planted
table (a test table that a wrong restatement passes checks nothing)."""
import math

import numpy as np

C = np.array([0.0, 0.10, 0.25, 0.33, 0.50, 0.75, 0.90, 1.0])
LO = np.array([0.0, 0.05, 0.18, 0.29, 0.42, 0.63, 0.83, 0.95])
HI = np.array([0.05, 0.18, 0.29, 0.42, 0.63, 0.83, 0.95, 1.05])
MARGIN = 0.1
STRATA_COLUMNS = (0, 2, 3)
STATS_DOUBLES = 2 * 30 + 2 * 3 * 8 * 8 + 1
WRONG = ("last_minimum", "acc_all_three", "error3_all_error3")


def columns():
    out = []
    for v in ("", "2", "3"):
        for kind in ("error", "acc"):
            out += [f"{kind}{v}_veg_b", f"{kind}{v}_veg_moy", f"{kind}{v}_veg_h", f"{kind}{v}_veg_b_and_moy", f"{kind}{v}_all"]
    return out


COLUMNS = tuple(columns())


def closest(y, wrong=None):
    """The first k that minimises fabs(c[k] - y); every difference NaN: 0."""
    y = np.asarray(y, dtype=np.float64)
    d = np.abs(C - y[..., None])
    if wrong == "last_minimum":
        return np.where(np.isnan(y), 0, 7 - np.argmin(d[..., ::-1], axis=-1))
    return np.argmin(d, axis=-1)


def planted_predictions():
    """Every border a comparison of the header looks at -- the class borders lo / hi, the margin borders lo - 0.1 / hi + 0.1, the
    outer borders of V3 are class borders again -- as the fp32 value nearest to it and that value's two fp32 neighbours (one lies
    below the border, one above), then 0, negative values, values above 1.05 and NaN."""
    edges = sorted(set(LO.tolist() + HI.tolist() + (LO - MARGIN).tolist() + (HI + MARGIN).tolist()))
    vals = []
    for e in edges:
        f = np.float32(e)
        vals += [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    vals += [np.float32(0.0), np.float32(-1e-3), np.float32(-0.25), np.float32(1.0500001), np.float32(1.2), np.float32(np.nan)]
    return np.array(vals, dtype=np.float32)


def planted_table(continuous=False):
    """(pred (P,4) fp32, gt (P,4) fp64): every planted prediction against every class centre as ground truth, the three strata
    shifted against each other so that a row mixes classes; `continuous` appends rows whose ground truth is no class centre."""
    pv = planted_predictions()
    pred, gt = [], []
    for k in range(8):
        for j in range(len(pv)):
            pred.append([pv[j], 0.5, pv[(j + 5) % len(pv)], pv[(j + 11) % len(pv)]])
            gt.append([C[k], 0.0, C[(k + 3) % 8], C[(k + 6) % 8]])
    pred += [[0.0, 1.0, 0.0, 0.0]]                                  # pred == 0 with gt == 0
    gt += [[0.0, 1.0, 0.0, 0.0]]
    if continuous:
        pred += [[0.41, 0.2, 0.1, 0.9], [0.3, 0.2, 0.1, 0.9]]
        gt += [[0.4, 0.1, 0.1, 0.9], [0.33, 0.1, 0.2604, 1.0]]
    return np.array(pred, dtype=np.float32), np.array(gt, dtype=np.float64)


def random_table(P, seed, ties=False):
    """Predictions around the ground truths' class centres (fp32), ground truths near or on centres; no exact closest-class tie unless
    asked for."""
    rng = np.random.RandomState(seed)
    k = rng.randint(0, 8, (P, 4))
    gt = C[k] + np.where(rng.rand(P, 4) < 0.85, 0.0, 0.02 * (rng.rand(P, 4) - 0.5))
    pred = (C[k] + 0.25 * rng.randn(P, 4)).astype(np.float32)
    pred[rng.rand(P, 4) < 0.1] = 0.0
    if ties:
        gt[::7, 0], gt[3::7, 2], gt[5::7, 3] = 0.05, 0.625, 0.95
    return pred, np.clip(gt, 0.0, 1.0)


def indicators(pred, gt, relabel, wrong=None):
    """-> (rows (P,30) fp64, cls (P,9) int32, stats dict: sum, count, cm (2,3,8,8), continuous)."""
    pred = np.asarray(pred)
    assert pred.dtype == np.float32
    gt = np.asarray(gt, dtype=np.float64)
    P = pred.shape[0]
    rows = np.empty((P, 30))
    cls = np.empty((P, 9), dtype=np.int32)
    err, err2, err3, acc, acc2, acc3 = ([None] * 3 for _ in range(6))
    bad = np.zeros(P, dtype=bool)
    with np.errstate(invalid="ignore"):
        for s, col in enumerate(STRATA_COLUMNS):
            p = pred[:, col].astype(np.float64)
            g = gt[:, col]
            if relabel:
                g = C[closest(g, wrong)]
            g = np.rint(g * 1000.0) / 1000.0
            kt = np.full(P, -1)
            for k in range(8):
                kt[g == C[k]] = k
            bad |= kt < 0
            kk = np.maximum(kt, 0)
            lo, hi = LO[kk], HI[kk]
            L, H = LO[np.maximum(kk - 1, 0)], HI[np.minimum(kk + 1, 7)]
            a1 = (lo <= p) & (p <= hi)
            a2 = ((lo - MARGIN) <= p) & (p <= (hi + MARGIN))
            a3 = (L <= p) & (p <= H)
            err[s] = np.abs(p - g)
            acc[s], acc2[s], acc3[s] = a1.astype(np.float64), a2.astype(np.float64), a3.astype(np.float64)
            err2[s] = np.where(a1, 0.0, np.fmin(np.abs(lo - p), np.abs(hi - p)))
            err3[s] = np.where(a3, 0.0, np.fmin(np.abs(L - p), np.abs(H - p)))
            cls[:, s] = closest(g, wrong)
            cls[:, 3 + s] = closest(p, wrong)
        for base, e, a in ((0, err, acc), (10, err2, acc2), (20, err3, acc3)):
            rows[:, base + 0], rows[:, base + 1], rows[:, base + 2] = e
            rows[:, base + 3] = (e[0] + e[1]) / 2.0
            rows[:, base + 4] = ((e[0] + e[1]) + e[2]) / 3.0
            rows[:, base + 5], rows[:, base + 6], rows[:, base + 7] = a
            rows[:, base + 8] = (a[0] + a[1]) / 2.0
            rows[:, base + 9] = ((a[0] + a[1]) + a[2]) / 3.0
        rows[:, 9] = (acc[0] + acc[1]) / 2.0 if wrong != "acc_all_three" else ((acc[0] + acc[1]) + acc[2]) / 3.0
        if wrong != "error3_all_error3":
            rows[:, 24] = ((err3[0] + err2[1]) + err3[2]) / 3.0
    rows[bad, 5:] = np.nan
    for s in range(3):
        cls[:, 6 + s] = np.where(~bad & (rows[:, 15 + s] == 1.0), cls[:, s], cls[:, 3 + s])
    ok = ~np.isnan(rows)
    cm = np.zeros((2, 3, 8, 8), dtype=np.int64)
    for s in range(3):
        np.add.at(cm[0, s], (cls[:, s], cls[:, 3 + s]), 1)
        np.add.at(cm[1, s], (cls[:, s], cls[:, 6 + s]), 1)
    stats = {"sum": np.array([math.fsum(rows[ok[:, c], c]) for c in range(30)]), "count": ok.sum(axis=0).astype(np.int64), "cm": cm,
             "continuous": int(bad.sum())}
    return rows, cls, stats


def stats_block(stats):
    """The stats dict as the SN2_CV_STATS_DOUBLES doubles of the entry point."""
    return np.concatenate([stats["sum"], stats["count"].astype(np.float64), stats["cm"].reshape(-1).astype(np.float64),
                           [float(stats["continuous"])]])
