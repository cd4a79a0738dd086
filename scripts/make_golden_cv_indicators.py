"""Golden fixture of the cross-validation indicators, produced by RUNNING THE REFERENCE'S OWN `learning/accuracy.py`.

Runs only where the reference checkout is present (`oracle.make_golden.REF`, as for `oracle/make_golden_aux.py`); no test needs
it.  Imported from the reference, unmodified, and CALLED: `calculate_performance_indicators_V1/V2/V3`,
`adjust_predictions_based_on_margin`, `compute_confusion_matrix`, `get_closest_class_center(_index)` -- on a pandas frame with the
columns of `get_cloud_prediction_summary`, as `post_cross_validation_logging` builds it, the relabelled case through the loop of
`main.py:102-109`.

What is NOT the reference's, and why:
  * `comet_ml` is a module NAME only (absent, un-fetchable; none of its code is needed);
  * `np.float = float`: `accuracy.py` calls `astype(np.float)`, which NumPy 1.24 removed; the alias is what it was;
  * the predictions enter the frame WIDENED to fp64 (exactly): under NumPy < 1.24, which the reference ran on, a float32 scalar
    against a Python float compared in fp64; NumPy 2 would compare in fp32.  The fixture pins the reference's behaviour;
  * the inputs hold no exact closest-class tie (NumPy's argsort pins none: 2.2.6 gives class 0 for 0.05 but class 5 for 0.625) and
    no NaN (`DataFrame.mean(axis=1)` would skip it inside a row; include/strata_hip.h states (a + b) / 2): both are tested against
    the stated rules instead (tests/test_cv_indicators_host.py).

Only arrays are written (inputs and expected outputs); no reference source text is stored.

    python scripts/make_golden_cv_indicators.py        # rewrites tests/golden/cv_indicators.npz
"""
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.make_golden import REF          # noqa: E402
OUT = os.path.join(ROOT, "tests", "golden", "cv_indicators.npz")
STRATA = ("veg_b", "veg_moy", "veg_h")


def import_reference():
    assert os.path.isdir(REF), "the reference checkout is needed to make this fixture"
    m = types.ModuleType("comet_ml")
    m.Experiment = m.OfflineExperiment = type("Absent", (), {})
    sys.modules["comet_ml"] = m
    if not hasattr(np, "float"):
        np.float = float
    import matplotlib
    matplotlib.use("Agg")
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import learning.accuracy as A          # noqa: E402  (reference code)
    return A


def inputs():
    """(pred (P,4) fp32, gt exactly-rounding-to-centres (P,4), gt near centres (P,4)): the planted border predictions of the tests
    (every third combination) and random rows."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _cv_indicators_ref import C, planted_table, random_table
    pp, pg = planted_table()
    keep = ~np.isnan(pp).any(axis=1)
    pp, pg = pp[keep][::3], pg[keep][::3]
    rp, rg = random_table(200, 7)
    rng = np.random.RandomState(11)
    pred = np.concatenate([pp, rp])
    centres = C[np.argmin(np.abs(C - np.concatenate([pg, rg])[..., None]), axis=-1)]
    on = centres + 4e-4 * (2 * rng.rand(*centres.shape) - 1)              # round(3) brings these back to the centres
    on[:len(pp)] = pg                                                      # the planted rows: the centres themselves
    near = np.clip(centres + 0.02 * (rng.rand(*centres.shape) - 0.5), 0.0, 1.0)   # continuous: only the relabelled case takes these
    return pred, on, near


def run(A, pred, gt, relabel):
    import pandas as pd
    keys = ["pred_veg_b", "pred_sol_nu", "pred_veg_moy", "pred_veg_h", "vt_veg_b", "vt_sol_nu", "vt_veg_moy", "vt_veg_h"]
    infos = [dict(zip(keys, [float(x) for x in pred[i]] + [float(x) for x in gt[i]])) for i in range(len(pred))]
    if relabel:
        for info in infos:                                                 # main.py:102-109
            for k in keys[4:]:
                info[k] = A.get_closest_class_center(info[k])
    df = pd.DataFrame(infos)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        df = A.calculate_performance_indicators_V1(df)
        df = A.calculate_performance_indicators_V2(df)
        df = A.calculate_performance_indicators_V3(df)
        cols = [c for c in df.columns if c.startswith("error") or c.startswith("acc")]
        assert len(cols) == 30
        adj = A.adjust_predictions_based_on_margin(df)
    changed = sum(int((adj["pred_" + s] != df["pred_" + s]).sum()) for s in STRATA)
    assert changed > 0, "adjust_predictions_based_on_margin changed nothing"
    idx = np.vectorize(A.get_closest_class_center_index)
    cls = np.stack([idx(df["vt_" + s].values) for s in STRATA] + [idx(df["pred_" + s].values) for s in STRATA] +
                   [idx(adj["pred_" + s].values) for s in STRATA], 1).astype(np.int32)
    cm = np.zeros((2, 3, 4, 8, 8))
    for a, frame in enumerate((df, adj)):
        for s, strata in enumerate(STRATA):
            for n, norm in enumerate((None, "true", "pred", "all")):
                cm[a, s, n] = A.compute_confusion_matrix(types.SimpleNamespace(normalize_cm=norm), frame, strata)
    return {"rows": df[cols].values.astype(np.float64), "columns": np.array(cols), "cls": cls, "cm": cm,
            "means": df[cols].mean().values.astype(np.float64), "vt": df[["vt_veg_b", "vt_veg_moy", "vt_veg_h"]].values}


def main():
    A = import_reference()
    pred, on, near = inputs()
    data = {"pred": pred, "gt_on": on, "gt_near": near, "centers": np.asarray(A.bins_centers, dtype=np.float64),
            "borders": np.array([A.center_to_border_dict[c] for c in A.bins_centers], dtype=np.float64)}
    for name, gt, relabel in (("on_plain", on, False), ("near_relabel", near, True)):
        for k, v in run(A, pred, gt, relabel).items():
            data[f"{name}/{k}"] = v
    np.savez_compressed(OUT, **data)
    print(f"{len(pred)} rows, {len(data)} arrays -> {OUT} ({os.path.getsize(OUT) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
