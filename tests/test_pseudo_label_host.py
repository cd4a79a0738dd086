"""The host side of pseudo-labelling (no device anywhere in this file): `train_data.plan_append`, the argument checks of
sn2_plots_append, the numpy restatement of the append (tests/_plotset_ref.py) on a hand-written case, the bookkeeping of
`EpochFeeder(plot_subset=...)` and `pseudo_label.pretrain_split`.  tests/test_gpu_plotset.py holds the kernel to the restatement,
tests/test_gpu_pseudo_label.py runs the whole path."""
import ctypes
import os

import numpy as np
import pytest
import torch

from _plotset_ref import dst_start_of, plots_append_ref, sentinel_destination


# ---- plan_append ----------------------------------------------------------------------------------------------------------
def _plan(*a, **kw):
    from stratanet2_vegetation_coverage_maps_amd.train_data import plan_append
    return plan_append(*a, **kw)


def test_plan_append_filter_is_strict():
    n = [1999, 2000, 2001, 2500, 2000]
    sel, start, n_max = _plan(n, None, 2000, 0, 0, 10 ** 6, 100)
    assert sel.tolist() == [2, 3]                                      # n == min_points is dropped, min_points + 1 is kept
    assert start.tolist() == [0, 2001, 4501] and n_max == 2500
    sel, start, n_max = _plan(n, None, None, 0, 0, 10 ** 6, 100)        # no filter: all, in order
    assert sel.tolist() == [0, 1, 2, 3, 4] and start.tolist() == np.concatenate([[0], np.cumsum(n)]).tolist() and n_max == 2500


def test_plan_append_select_with_min_points_and_running_sum():
    n = [5, 0, 7, 3, 9]
    sel, start, n_max = _plan(n, [4, 1, 2, 2, 0, 3], 3, 6, 11, 1000, 100)   # any order, a plot twice, an empty plot, a filter
    assert sel.tolist() == [4, 2, 2, 0]                                 # 0 and 3 points are not > 3
    assert start.tolist() == [11, 20, 27, 34, 39] and n_max == 9
    assert start.tolist() == dst_start_of(n, sel, 11).tolist()
    sel, start, n_max = _plan(n, [3, 1, 3], None, 2, 7, 1000, 100)      # without the filter an empty plot stays
    assert sel.tolist() == [3, 1, 3] and start.tolist() == [7, 10, 10, 13] and n_max == 3
    sel, start, n_max = _plan(n, np.array([2], dtype=np.int32), None, 0, 0, 7, 1)   # exactly full is allowed
    assert sel.tolist() == [2] and start.tolist() == [0, 7]
    for bad in ([5], [-1], [[0, 1]], [0.5]):
        with pytest.raises(ValueError):
            _plan(n, bad, None, 0, 0, 1000, 100)


def test_plan_append_nothing_kept():
    for args in (([10, 20], None, 20), ([10, 20], [], None), ([], None, None)):
        sel, start, n_max = _plan(*args, 3, 17, 17, 3)                  # a full arena: nothing kept never overflows
        assert sel.size == 0 and start.tolist() == [17] and n_max == 0


def test_plan_append_overflow_names_the_capacity_needed():
    n = [100, 200, 300]
    with pytest.raises(ValueError, match=r"5 plots and 650 points") as e:
        _plan(n, None, None, 2, 50, 649, 100)                           # one point short
    assert "649 points" in str(e.value)
    with pytest.raises(ValueError, match=r"5 plots and 650 points"):
        _plan(n, None, None, 2, 50, 10 ** 6, 4)                         # one plot short
    sel, start, _ = _plan(n, None, None, 2, 50, 650, 5)
    assert sel.size == 3 and start[-1] == 650


# ---- the restatement itself -----------------------------------------------------------------------------------------------
def test_restatement_on_a_hand_written_case():
    src_raw = (np.arange(10)[:, None] * 100 + np.arange(9)[None, :]).astype(np.float32)     # value = 100 channel + column
    src_offsets = np.array([0, 2, 2, 6, 9], dtype=np.int32)             # plots of 2, 0, 4, 3 points
    src_centers = np.array([[1, 2], [3, 4], [5, 6], [7, 8]], dtype=np.float32)
    src_cov = np.full((4, 4), np.float32(0.1)) * np.arange(1, 5, dtype=np.float32)[:, None]
    sel = [3, 1, 0]
    start = dst_start_of([2, 0, 4, 3], sel, 3)
    assert start.tolist() == [3, 6, 6, 8]
    dst = sentinel_destination(12, 6)
    raw, offsets, centers, cov = plots_append_ref(src_raw, src_offsets, src_centers, src_cov, sel, *dst, 2, 3, start)
    assert raw[:, 3:8].tolist() == [[100 * c + j for j in (6, 7, 8, 0, 1)] for c in range(10)]
    assert offsets[2:6].tolist() == [3, 6, 6, 8]
    assert centers[2:5].tolist() == [[7, 8], [3, 4], [1, 2]]
    assert cov[2, 0] == float(np.float32(0.1) * np.float32(4)) and cov[2, 0] != 0.4 and cov[4, 3] == float(np.float32(0.1))
    for new, old, lo, hi in ((raw.T, dst[0].T, 3, 8), (offsets, dst[1], 2, 6), (centers, dst[2], 2, 5), (cov, dst[3], 2, 5)):
        keep = np.ones(len(new), dtype=bool)
        keep[lo:hi] = False
        assert new[keep].tobytes() == old[keep].tobytes()               # every other sentinel is intact


# ---- the entry point's argument checks ------------------------------------------------------------------------------------
def test_c_abi_refuses_bad_arguments_before_any_device_work():
    from stratanet2_vegetation_coverage_maps_amd import _build, _lib
    raw = ctypes.CDLL(_lib.LIB_PATH if os.path.exists(_lib.LIB_PATH) else _build.build(verbose=False))
    fn = raw.sn2_plots_append
    fn.restype = ctypes.c_int
    fn.argtypes = _lib.SIGNATURES["sn2_plots_append"]
    EINVAL, ELIMIT = _lib.SN2_EINVAL, _lib.SN2_ELIMIT
    p = 0x1000                                                   # never dereferenced: every call below fails a check first
    good = dict(src_raw=p, src_T=5000, src_offsets=p, src_centers=p, src_cov=p, sel=p, K=3, dst_raw=p, cap_T=9000, dst_offsets=p,
                dst_centers=p, dst_cov=p, cap_P=10, P0=7, T0=100, dst_start=p, new_T=9000, stream=None)

    def call(**kw):
        return fn(*{**good, **kw}.values())
    for name in ("src_raw", "src_offsets", "src_centers", "src_cov", "sel", "dst_raw", "dst_offsets", "dst_centers", "dst_cov",
                 "dst_start"):
        assert call(**{name: None}) == EINVAL, name
    assert call(K=0) == EINVAL and call(K=-1) == EINVAL
    assert call(P0=-1) == EINVAL and call(T0=-1, new_T=50) == EINVAL
    assert call(P0=8) == EINVAL and call(cap_P=9) == EINVAL                       # P0 + K > cap_P (7 + 3 = 10 fits exactly)
    assert call(K=2 ** 31 - 1, P0=2 ** 31 - 1, cap_P=2 ** 31 - 1) == EINVAL       # ... also where the int sum would wrap
    assert call(new_T=9001) == EINVAL                                             # new_T > cap_T (new_T == cap_T fits)
    assert call(new_T=99) == EINVAL                                               # an append cannot shrink the set
    assert call(cap_T=2 ** 31) == ELIMIT and call(cap_T=2 ** 31, new_T=2 ** 31) == ELIMIT
    assert call(src_T=2 ** 31) == ELIMIT
    assert "sn2_plots_append" in _lib.SIGNATURES and _lib.SN2_VERSION == 102      # an added entry point keeps the version


# ---- EpochFeeder(plot_subset=...) -----------------------------------------------------------------------------------------
def _set(P):
    from stratanet2_vegetation_coverage_maps_amd.train_data import ResidentPlots
    plots = ResidentPlots.__new__(ResidentPlots)
    plots.P, plots.version = P, 0
    return plots


def _feeder(plots, B=2, subset=None, gen_seed=99, **kw):
    from stratanet2_vegetation_coverage_maps_amd.train_data import EpochFeeder
    return EpochFeeder(plots, None, B, 5, generator=torch.Generator().manual_seed(gen_seed), plot_subset=subset, **kw)


def test_feeder_subset_epochs_are_permutations_of_the_subset():
    subset = [9, 2, 4, 10, 0, 7, 3]
    f = _feeder(_set(11), B=2, subset=subset)
    assert f.steps_per_epoch == 3 and f.P == 11                         # the generator key keeps the SET's P
    g = torch.Generator().manual_seed(99)
    for e in range(5):
        perm = torch.randperm(7, generator=g)
        ids = [f.batch_ids(3 * e + k) for k in range(3)]
        assert all(x.dtype == torch.int32 and x.numel() == 2 for x in ids)
        seen = torch.cat(ids).tolist()
        assert seen == [subset[j] for j in perm[:6].tolist()]            # subset[randperm(len(subset))], the last one dropped
        assert len(set(seen)) == 6 and set(seen) <= set(subset)
        assert f.locate(3 * e) == (e, 0)
    for bad in ([11], [-1, 2], [], [0.5]):
        with pytest.raises(ValueError):
            _feeder(_set(11), subset=bad)
    with pytest.raises(ValueError):
        _feeder(_set(11), B=4, subset=[1, 2, 3])                         # fewer plots in the subset than in a batch


def test_feeder_without_subset_draws_what_it_always_drew():
    from types import SimpleNamespace
    from stratanet2_vegetation_coverage_maps_amd.train_data import EpochFeeder
    old = EpochFeeder(SimpleNamespace(P=7), None, 2, 5, generator=torch.Generator().manual_seed(99))       # as built today
    new = _feeder(_set(7), B=2, subset=None)
    g = torch.Generator().manual_seed(99)
    perms = [torch.randperm(7, generator=g) for _ in range(4)]
    for i in range(12):
        e, k = divmod(i, 3)
        assert new.batch_ids(i).tolist() == old.batch_ids(i).tolist() == perms[e][2 * k:2 * k + 2].tolist()
    full = _feeder(_set(7), B=2, subset=list(range(7)))                  # the identity subset: the same orders too
    assert [full.batch_ids(i).tolist() for i in range(12)] == [old.batch_ids(i).tolist() for i in range(12)]


def test_feeder_subset_state_dict_round_trip_and_mismatch():
    subset = [9, 2, 4, 10, 0, 7, 3]
    f = _feeder(_set(11), subset=subset)
    want = [f.batch_ids(i).tolist() for i in range(14)]
    for cut in (0, 3, 7):
        sd = f.state_dict(cut)
        assert sd["subset"] == 7 and sd["plots"] == 11
        g = _feeder(_set(11), subset=subset, gen_seed=1)
        g.load_state_dict(sd)
        assert [g.batch_ids(i).tolist() for i in range(14 - cut)] == want[cut:]
    with pytest.raises(ValueError):
        _feeder(_set(11), subset=subset[:6]).load_state_dict(f.state_dict(0))       # another subset length
    with pytest.raises(ValueError):
        _feeder(_set(11)).load_state_dict(f.state_dict(0))                           # a state with a subset into a feeder without
    with pytest.raises(ValueError):
        f.load_state_dict(_feeder(_set(11)).state_dict(0))                           # ... and the other way round
    assert _feeder(_set(11)).state_dict(0)["subset"] is None


def test_feeder_refuses_a_set_that_changed():
    plots = _set(11)
    f = _feeder(plots, subset=[1, 2, 3, 4])
    f.batch_ids(0)
    plots.version += 1                                                   # what append / reserve do
    with pytest.raises(RuntimeError, match="changed"):
        f.batch_ids(1)
    with pytest.raises(RuntimeError, match="changed"):
        f.fill_slot(1, {})
    _feeder(plots, subset=[1, 2, 3, 4]).batch_ids(0)                     # a feeder built now is fine


# ---- pretrain_split -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,n_val", [(4, 0), (30, 6), (499, 99), (500, 100), (1000, 100)])
def test_pretrain_split(P, n_val):
    from stratanet2_vegetation_coverage_maps_amd.pseudo_label import MIN_POINTS_NB_FOR_PSEUDO_LABELLING, pretrain_split
    assert MIN_POINTS_NB_FOR_PSEUDO_LABELLING == 2000
    assert min(int(0.2 * P), 100) == n_val                               # the literals above are main_SSL.py:70's arithmetic
    train, val = pretrain_split(P)
    ref_train, ref_val = np.split(np.arange(P), [P - n_val])             # main_SSL.py:71
    assert np.array_equal(train, ref_train) and np.array_equal(val, ref_val)
    assert len(val) == n_val and len(train) + len(val) == P
