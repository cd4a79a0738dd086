"""The per-point score kernels (csrc/points.hip: sn2_points_merge, sn2_points_finalize) against the numpy restatement of their
rule (tests/_point_scores_ref.py), bit for bit, on the planted batch of tests/_point_scores_cases.py: three plots of 256 samples
over 500 parcel points."""
import numpy as np
import pytest
import torch

import _point_scores_cases as cases
import _point_scores_ref as ref
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def planted():
    plots = cases.planted()
    whole = cases.batch_of(plots)
    return plots, whole, ref.point_scores([whole], cases.T, cases.DIAM)


def fresh():
    return (torch.zeros(cases.T, ops.POINTS_ACC_WORDS, dtype=torch.int64, device=DEV), torch.zeros(cases.T, dtype=torch.int32, device=DEV))


def merge(acc, hits, bt, col_base=True):
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in bt.items()}
    ops.points_merge(d["cov"], d["proba"], d["xyz"], d["idx"], d["n_live"], d["offsets"], d["point_index"], acc, hits, cases.DIAM,
                     col_base=d["col_base"] if col_base else None)


def result(acc, hits):
    scores, weight = ops.points_finalize(acc, hits)
    return scores.cpu().numpy(), weight.cpu().numpy(), hits.cpu().numpy()


def same_bytes(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def test_kernels_equal_the_restatement_bit_for_bit(planted):
    plots, whole, want = planted
    acc, hits = fresh()
    merge(acc, hits, whole)
    got = result(acc, hits)
    s, w, h = got
    j = plots[0]["planted_samples"]
    print(f"\ncontributions {int(h.sum())}, points hit {int((h > 0).sum())} of {cases.T}, most hits {int(h.max())}")
    print(f"weight at the centre {w[cases.CENTRE]!r}, at r = 10 m {w[cases.RIM]!r}; differing score words "
          f"{int((s.view(np.uint32) != want[0].view(np.uint32)).sum())}, weight words {int((w.view(np.uint32) != want[1].view(np.uint32)).sum())}")
    assert np.array_equal(h, want[2]) and h[cases.SHARED] == 3 and h[cases.NEVER] == 0
    assert same_bytes(got, want)
    # the planted points, spelled out
    assert w[cases.CENTRE] == 1.5 and w[cases.RIM] == 1.0 and w[cases.NEVER] == 0.0 and np.isnan(s[:, cases.NEVER]).all()
    assert (s[:, cases.ZERO] == 0.0).all() and (s[:, cases.ONE_] == 1.0).all()
    v = np.concatenate([plots[0]["cov"][j[cases.CENTRE]], plots[0]["proba"][j[cases.CENTRE]]])
    big = v >= 2.0 ** -7
    assert big.sum() >= 4 and np.array_equal(s[big, cases.CENTRE], v[big])          # a single contribution returns the value itself
    # the accumulator is left as it was: a second finalisation gives the same bytes
    assert same_bytes(result(acc, hits), want)


def test_any_split_and_order_of_the_launches_gives_the_same_bytes(planted):
    plots, whole, want = planted
    acc, hits = fresh()
    for p in plots:                                   # three launches of one plot
        merge(acc, hits, cases.batch_of([p]))
    assert same_bytes(result(acc, hits), want)
    acc, hits = fresh()
    merge(acc, hits, cases.batch_of(plots[::-1]))     # one launch, the plots in reverse
    assert same_bytes(result(acc, hits), want)
    acc, hits = fresh()
    merge(acc, hits, cases.batch_of([plots[2], plots[0]]))
    merge(acc, hits, cases.batch_of([plots[1]]))
    assert same_bytes(result(acc, hits), want)


def test_a_second_merge_adds_to_a_filled_accumulator(planted):
    plots, whole, want = planted
    acc, hits = fresh()
    merge(acc, hits, whole)
    first = acc.clone()
    merge(acc, hits, whole)
    assert torch.equal(acc, 2 * first) and np.array_equal(hits.cpu().numpy(), 2 * want[2])
    assert same_bytes(result(acc, hits), ref.point_scores([whole, whole], cases.T, cases.DIAM))


def test_without_col_base_every_plot_starts_at_column_zero(planted):
    plots, whole, _ = planted
    acc, hits = fresh()
    merge(acc, hits, whole, col_base=False)
    assert same_bytes(result(acc, hits), ref.point_scores([{**whole, "col_base": None}], cases.T, cases.DIAM))


def test_wrapper_refuses_wrong_shapes_before_any_launch(planted):
    _, whole, _ = planted
    acc, hits = fresh()
    with pytest.raises(ValueError):
        merge(acc[:, :8].contiguous(), hits, whole)
    with pytest.raises(ValueError):
        merge(acc, hits, {**whole, "n_live": whole["n_live"][:2]})
    with pytest.raises(ValueError):
        merge(acc, hits, {**whole, "cov": whole["cov"][:-1]})
    assert int(hits.sum()) == 0 and int(acc.abs().sum()) == 0
