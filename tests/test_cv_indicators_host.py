"""The cross-validation report without a GPU: the numpy restatement (tests/_cv_indicators_ref.py) against the fixture that the
reference's own `learning/accuracy.py` wrote (tests/golden/cv_indicators.npz, scripts/make_golden_cv_indicators.py), the stated tie
rule, `CrossValReport.confusion` against sklearn, `kfold_indices` against sklearn's KFold, and the argument checks of the entry
point."""
import ctypes

import numpy as np
import pytest

import _cv_indicators_ref as R
from conftest import load_golden

CASES = (("on_plain", "gt_on", False), ("near_relabel", "gt_near", True))


@pytest.fixture(scope="module")
def golden():
    return load_golden("cv_indicators")


def test_constants_and_columns_are_the_references(golden):
    from stratanet2_vegetation_coverage_maps_amd import cross_validation as cv
    assert golden["centers"].tolist() == R.C.tolist() == list(cv.BINS_CENTERS)
    assert golden["borders"][:, 0].tolist() == R.LO.tolist() and golden["borders"][:, 1].tolist() == R.HI.tolist()
    assert list(golden["on_plain/columns"]) == list(R.COLUMNS) == list(cv.COLUMNS)
    assert R.STATS_DOUBLES == cv.ops.CV_STATS_DOUBLES and len(cv.COLUMNS) == cv.ops.CV_COLUMNS


@pytest.mark.parametrize("name,gt,relabel", CASES)
def test_restatement_equals_the_reference_bit_for_bit(golden, name, gt, relabel):
    rows, cls, stats = R.indicators(golden["pred"], golden[gt], relabel)
    want = golden[name + "/rows"]
    assert rows.shape == want.shape == (len(golden["pred"]), 30) and not np.isnan(want).any()
    assert np.array_equal(rows.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(cls, golden[name + "/cls"])
    assert stats["continuous"] == 0
    # the fixture reaches both sides of every decision: hits and misses of the three accuracies in every stratum, adjusted rows
    for c in (5, 6, 7, 15, 16, 17, 25, 26, 27):
        assert 0 < want[:, c].sum() < len(want), R.COLUMNS[c]
    assert (cls[:, 3:6] != cls[:, 6:9]).any()
    # DataFrame.mean() of the reference: every mean within the fp64 re-association of a sum of 393 terms
    mean = stats["sum"] / stats["count"]
    np.testing.assert_allclose(mean, golden[name + "/means"], rtol=0, atol=393 * 2.0 ** -53 * 1.05)


@pytest.mark.parametrize("name,gt,relabel", CASES)
def test_report_confusions_equal_the_references_for_all_normalisations(golden, name, gt, relabel):
    from stratanet2_vegetation_coverage_maps_amd.cross_validation import STRATA, CrossValReport
    pred = golden["pred"]
    rows, cls, stats = R.indicators(pred, golden[gt], relabel)
    rep = CrossValReport(R.stats_block(stats), rows, cls, pred, golden[gt], relabel)
    assert rep.class_based and rep.n_plots == len(pred) and set(rep.means) == set(R.COLUMNS)
    for a, margin in enumerate((False, True)):
        for s, strata in enumerate(STRATA):
            for n, norm in enumerate((None, "true", "pred", "all")):
                got = rep.confusion(strata, normalize=norm, margin=margin)
                assert np.array_equal(got, golden[name + "/cm"][a, s, n]), (margin, strata, norm)
            assert np.array_equal(rep.confusion(s), rep.confusion(strata))
    for c, n in enumerate(R.COLUMNS):
        assert abs(rep.means[n] - golden[name + "/means"][c]) <= 393 * 2.0 ** -53 * 1.05, n


def test_confusion_normalisation_is_sklearns_with_empty_rows_and_columns():
    """True classes 3 and 7 and predicted classes 0 and 5 never occur: 0 / 0 = 0 in every normalisation."""
    from sklearn.metrics import confusion_matrix
    from stratanet2_vegetation_coverage_maps_amd.cross_validation import CrossValReport
    rng = np.random.RandomState(3)
    true = rng.choice([0, 1, 2, 4, 5, 6], 200)
    pred = rng.choice([1, 2, 3, 4, 6, 7], 200)
    cm = np.zeros((2, 3, 8, 8), dtype=np.int64)
    np.add.at(cm[0, 1], (true, pred), 1)
    np.add.at(cm[1, 2], (pred, true), 1)
    stats = {"sum": np.zeros(30), "count": np.zeros(30, dtype=np.int64), "cm": cm, "continuous": 0}
    rep = CrossValReport(R.stats_block(stats), None, None, np.zeros((200, 4), np.float32), np.zeros((200, 4)), False)
    assert all(np.isnan(v) for v in rep.means.values())                     # count 0: NaN, no division error
    for norm in (None, "true", "pred", "all"):
        a = rep.confusion("veg_moy", normalize=norm)
        b = rep.confusion("veg_h", normalize=norm, margin=True)
        assert np.array_equal(a, confusion_matrix(true, pred, labels=range(8), normalize=norm)), norm
        assert np.array_equal(b, confusion_matrix(pred, true, labels=range(8), normalize=norm)), norm
        assert not a[3].any() and not a[:, 0].any() and not np.isnan(a).any()
        assert not rep.confusion("veg_b", normalize=norm).any()
    with pytest.raises(ValueError):
        rep.confusion("veg_b", normalize="rows")


@pytest.mark.parametrize("P", [5, 12, 13, 103])
@pytest.mark.parametrize("n_splits", [2, 3, 5])
def test_kfold_indices_are_sklearns(P, n_splits):
    from sklearn.model_selection import KFold
    from stratanet2_vegetation_coverage_maps_amd import kfold_indices
    for seed in (42, 7):
        want = list(KFold(n_splits=n_splits, shuffle=True, random_state=seed).split(range(P)))
        got = kfold_indices(P, n_splits, seed)
        assert len(got) == len(want) == n_splits
        for (a, b), (c, d) in zip(got, want):
            assert a.tolist() == c.tolist() and b.tolist() == d.tolist()
        assert sorted(np.concatenate([v for _, v in got]).tolist()) == list(range(P))
    assert [v.tolist() for _, v in kfold_indices(P, n_splits)] == [v.tolist() for _, v in kfold_indices(P, n_splits, 42)]
    with pytest.raises(ValueError):
        kfold_indices(P, 1)
    with pytest.raises(ValueError):
        kfold_indices(P, P + 1)


def test_planted_ties_follow_the_stated_rule():
    """0.05 and 0.625 lie exactly between two centres in fp64: the lower class.  0.95, 0.175 and 0.825 are no ties in fp64: their
    two differences, printed, differ in the last bits, and the nearer centre is the lower one."""
    from stratanet2_vegetation_coverage_maps_amd.cross_validation import closest_class
    ys = np.array([0.05, 0.625, 0.95, 0.175, 0.825])
    pairs = ((0, 1), (4, 5), (6, 7), (1, 2), (5, 6))
    for y, (a, b) in zip(ys, pairs):
        print(f"y = {y!r}: |c[{a}] - y| = {abs(R.C[a] - y)!r}, |c[{b}] - y| = {abs(R.C[b] - y)!r}")
    assert [abs(R.C[a] - y) == abs(R.C[b] - y) for y, (a, b) in zip(ys, pairs)] == [True, True, False, False, False]
    assert R.closest(ys).tolist() == [0, 4, 6, 1, 5] == closest_class(ys).tolist()
    assert R.closest(np.array([np.nan, -3.0, 7.0, 0.0, 1.0])).tolist() == [0, 0, 7, 0, 7]
    assert closest_class(np.array([np.nan, -3.0, 7.0])).tolist() == [0, 0, 7]
    # a tie as ground truth of a relabelled report: the lower centre, in the rows too
    pred = np.array([[0.04, 0, 0.6, 0.94]], dtype=np.float32)
    gt = np.array([[0.05, 0, 0.625, 0.95]])
    rows, cls, _ = R.indicators(pred, gt, True)
    assert cls[0, :3].tolist() == [0, 4, 6]
    assert rows[0, 0] == abs(float(pred[0, 0]) - 0.0) and rows[0, 1] == abs(float(pred[0, 2]) - 0.5)


@pytest.mark.parametrize("wrong", R.WRONG)
def test_a_wrong_restatement_differs_on_the_planted_table(wrong):
    """The planted table (with tied ground truths appended for the tie rule) tells each plausible mistake from the stated rule."""
    pred, gt = R.planted_table()
    pred = np.concatenate([pred, np.array([[0.04, 0, 0.6, 0.94], [0.3, 0, 0.7, 0.99]], dtype=np.float32)])
    gt = np.concatenate([gt, np.array([[0.05, 0, 0.625, 0.95], [0.05, 0, 0.625, 0.95]])])
    differs = False
    for relabel in (False, True):
        rows, cls, stats = R.indicators(pred, gt, relabel)
        rows_w, cls_w, stats_w = R.indicators(pred, gt, relabel, wrong=wrong)
        differs |= not (np.array_equal(rows.view(np.uint64), rows_w.view(np.uint64)) and np.array_equal(cls, cls_w))
    assert differs, wrong


def test_planted_table_reaches_every_border_from_both_sides():
    pv = R.planted_predictions().astype(np.float64)
    for e in sorted(set(R.LO.tolist() + R.HI.tolist() + (R.LO - R.MARGIN).tolist() + (R.HI + R.MARGIN).tolist())):
        below, above = pv[pv < e], pv[pv > e]
        assert np.float32(below.max()) == np.nextafter(np.float32(above.min()), np.float32(-np.inf)) or e in pv, e
    assert np.isnan(pv).any() and (pv < 0).any() and (pv > 1.05).any() and (pv == 0).any()


def test_nan_and_continuous_rows_as_stated():
    pred, gt = R.planted_table(continuous=True)
    rows, cls, stats = R.indicators(pred, gt, False)
    assert stats["continuous"] == 2 and np.isnan(rows[-2:, 5:]).all() and not np.isnan(rows[-2:, :5]).any()
    assert cls[-2, 0] == 3 and cls[-1, 1] == 2                                # closest classes of 0.4 and 0.26
    assert (cls[-2:, 6:9] == cls[-2:, 3:6]).all()                             # no margin adjustment without an acc2 entry
    nan_rows = np.isnan(pred[:, 0])
    assert nan_rows.any() and np.isnan(rows[nan_rows, 0]).all() and (rows[nan_rows, 5] == 0).all() and (cls[nan_rows, 3] == 0).all()
    assert stats["count"][0] == len(pred) - nan_rows.sum() and stats["count"][5] == len(pred) - 2
    # relabelled, the continuous rows become class rows
    _, _, stats_r = R.indicators(pred, gt, True)
    assert stats_r["continuous"] == 0
    from stratanet2_vegetation_coverage_maps_amd.cross_validation import CONTINUOUS_COLUMNS, CrossValReport
    rep = CrossValReport(R.stats_block(stats), rows, cls, pred, gt, False)
    assert not rep.class_based and rep.n_continuous == 2 and tuple(rep.means) == CONTINUOUS_COLUMNS


def test_entry_point_argument_checks_return_before_any_device_work():
    """NULL pointers and P < 1: SN2_EINVAL; more than 2^24 plots: SN2_ELIMIT and 0 workspace words (fake pointers: never read)."""
    from stratanet2_vegetation_coverage_maps_amd import _lib
    from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
    lib = _lib.load()
    fake = 0x1000
    args = [fake, fake, 100, 0, fake, fake, fake, fake, None]
    for i in (0, 1, 4, 5, 6, 7):
        a = list(args)
        a[i] = None
        assert lib.sn2_cv_indicators(*a) == _lib.SN2_EINVAL, i
    for P in (0, -5):
        assert lib.sn2_cv_indicators(fake, fake, P, 0, fake, fake, fake, fake, None) == _lib.SN2_EINVAL
    assert lib.sn2_cv_indicators(fake + 4, fake, 100, 0, fake, fake, fake, fake, None) == _lib.SN2_EINVAL      # pred: 16-byte rows
    assert lib.sn2_cv_indicators(fake, fake, (1 << 24) + 1, 1, fake, fake, fake, fake, None) == _lib.SN2_ELIMIT
    words = ctypes.c_size_t(77)
    assert lib.sn2_cv_indicators_ws_words((1 << 24) + 1, ctypes.byref(words)) == _lib.SN2_ELIMIT and words.value == 0
    assert lib.sn2_cv_indicators_ws_words(0, ctypes.byref(words)) == _lib.SN2_EINVAL and words.value == 0
    assert lib.sn2_cv_indicators_ws_words(5, None) == _lib.SN2_EINVAL
    assert ops.cv_indicators_ws_words((1 << 24) + 1) == 0
    per_slice = _lib.CONSTANTS["SN2_CV_WS_SLICE_WORDS"]
    for P, slices in ((1, 1), (1024, 1), (1025, 2), (5000, 5), (1 << 24, 1 << 14)):
        assert lib.sn2_cv_indicators_ws_words(P, ctypes.byref(words)) == 0 and words.value == slices * per_slice
        assert ops.cv_indicators_ws_words(P) == slices * per_slice
