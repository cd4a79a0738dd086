"""sn2_plots_append (csrc/plotset.hip) alone, through hip_ops.plots_append, against the numpy restatement of tests/_plotset_ref.py,
bit for bit: the destination starts as sentinels, so the comparison of the WHOLE arena covers what must be written and what must
stay.  Then the arena bookkeeping of train_data.ResidentPlots (empty / append / reserve) on top of it.

Source plots of 1, 255, 257, 256, 1025, 0, 5, 2 and 300 points: one point, one below / at / above a workgroup's 256 columns,
several workgroups, an empty plot, and plot starts at columns 1, 2 and 3 mod 4."""
import numpy as np
import pytest
import torch

from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args
from stratanet2_vegetation_coverage_maps_amd.train_data import ResidentPlots
from _plotset_ref import (SENTINEL_F32, SENTINEL_F64, SENTINEL_I32, dst_start_of, plots_append_ref, sentinel_destination)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 255, 257, 256, 1025, 0, 5, 2, 300)


@pytest.fixture(scope="module")
def source():
    rng = np.random.RandomState(7)
    T = sum(SIZES)
    raw = rng.randint(0, 2 ** 32, size=(10, T), dtype=np.uint64).astype(np.uint32).view(np.float32)   # any bit pattern, NaNs included
    offsets = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    assert {int(o) % 4 for o in offsets[:-1]} == {0, 1, 2, 3}
    centers = (rng.rand(len(SIZES), 2) * 1e6).astype(np.float32)
    cov = rng.rand(len(SIZES), 4).astype(np.float32)
    cov[:, 1] = np.float32(0.1)                                        # not representable shortly: widened, never re-rounded
    host = (raw, offsets, centers, cov)
    return host, tuple(torch.from_numpy(a).to(DEV) for a in host)


# (selection, P0, T0, spare plots, spare columns)
CASES = {
    "one_plot": ([4], 0, 0, 3, 100),
    "descending_nonadjacent_twice": ([8, 6, 3, 6, 1], 0, 0, 1, 7),
    "empty_between": ([2, 5, 7], 3, 777, 2, 50),
    "every_size_odd_start": ([0, 1, 2, 3, 4], 2, 13, 4, 1),
    "more_rows_than_columns": ([5, 5, 0, 5], 1, 3, 1, 1),
    "all_exactly_full": (list(range(len(SIZES))), 5, 1, 0, 0),
}


@pytest.mark.parametrize("name", list(CASES))
def test_append_equals_the_restatement_and_keeps_every_sentinel(source, name):
    (raw, offsets, centers, cov), dev = source
    sel, P0, T0, spare_P, spare_T = CASES[name]
    K = len(sel)
    start = dst_start_of(SIZES, sel, T0)
    new_T = int(start[-1])
    cap_T, cap_P = new_T + spare_T, P0 + K + spare_P
    dst = sentinel_destination(cap_T, cap_P)
    want = plots_append_ref(raw, offsets, centers, cov, sel, *dst, P0, T0, start)
    got_dev = [torch.from_numpy(a.copy()).to(DEV) for a in dst]
    table = torch.from_numpy(np.concatenate([sel, start]).astype(np.int32)).to(DEV)
    ops.plots_append(*dev, table[:K], *got_dev, P0, T0, table[K:], new_T)
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in got_dev]
    for g, w, what in zip(got, want, ("raw", "offsets", "centers", "coverages")):
        assert g.tobytes() == w.tobytes(), what
    g_raw, g_off, g_cen, g_cov = got
    # the sentinels, spelled out: columns at or beyond the new total and below T0 in all ten rows, table rows outside the append
    assert (g_raw.view(np.uint32)[:, new_T:] == SENTINEL_F32).all() and (g_raw.view(np.uint32)[:, :T0] == SENTINEL_F32).all()
    assert (g_off[:P0] == SENTINEL_I32).all() and (g_off[P0 + K + 1:] == SENTINEL_I32).all()
    assert g_off[P0:P0 + K + 1].tolist() == start.tolist()
    for tab, s in ((g_cen.view(np.uint32), SENTINEL_F32), (g_cov.view(np.uint64), SENTINEL_F64)):
        assert (tab[:P0] == s).all() and (tab[P0 + K:] == s).all()
    assert g_cov[P0:P0 + K].tobytes() == cov[sel].astype(np.float64).tobytes()
    assert g_cov[P0, 1] == float(np.float32(0.1)) and g_cov[P0, 1] != 0.1
    if new_T > T0:
        assert not (g_raw.view(np.uint32)[:, T0:new_T] == SENTINEL_F32).any()


def test_wrapper_refuses_bad_arguments_on_the_host(source):
    _, dev = source
    dst = [torch.from_numpy(a).to(DEV) for a in sentinel_destination(64, 4)]
    table = torch.tensor([0, 6, 0, 1, 6], dtype=torch.int32, device=DEV)          # plots 0 and 6: 1 + 5 points
    sel, start = table[:2], table[2:]
    before = [t.clone() for t in dst]
    for kw in (dict(P0=3), dict(P0=-1), dict(new_T=65), dict(T0=7, new_T=6)):
        a = dict(P0=0, T0=0, new_T=6)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.plots_append(*dev, sel, *dst, a["P0"], a["T0"], start, a["new_T"])
    with pytest.raises(ValueError):
        ops.plots_append(*dev, sel.long(), *dst, 0, 0, start, 6)                   # a selection of another dtype
    with pytest.raises(ValueError):
        ops.plots_append(*dev[:3], dev[3].double(), sel, *dst, 0, 0, start, 6)     # fp64 source coverages
    with pytest.raises(ValueError):
        ops.plots_append(*dev, sel, *dst, 0, 0, table[1:], 6)                      # a start table that is not K + 1 long
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(dst, before))


def _host_plots(source, ids):
    (raw, offsets, centers, cov), _ = source
    return [raw[:, offsets[p]:offsets[p + 1]] for p in ids], centers[ids], cov[ids].astype(np.float64)


def _same_set(a: ResidentPlots, b: ResidentPlots):
    assert a.P == b.P and a.n_filled == b.n_filled and a.n_points_max == b.n_points_max
    assert a.n_points.tolist() == b.n_points.tolist()
    assert torch.equal(a.raw[:, :a.n_filled].view(torch.int32), b.raw[:, :b.n_filled].view(torch.int32))
    assert torch.equal(a.offsets, b.offsets) and torch.equal(a.centers, b.centers)
    assert torch.equal(a.coverages.view(torch.int64), b.coverages.view(torch.int64))
    for t, shape in ((a.offsets, (a.P + 1,)), (a.centers, (a.P, 2)), (a.coverages, (a.P, 4))):
        assert tuple(t.shape) == shape and t.is_contiguous()


def test_resident_plots_arena_grows_by_appends_and_reserve(source):
    """empty -> two appends (a parcel-like source: any object with raw / offsets / centers / n_points; then another ResidentPlots)
    -> the set `from_plots` builds on the host from the same plots.  Real values here (the set is compared through torch)."""
    from types import SimpleNamespace
    (raw, offsets, centers, cov), dev = source
    raw = np.nan_to_num(raw, nan=1.0, posinf=2.0, neginf=3.0)
    src = SimpleNamespace(raw=torch.from_numpy(raw).to(DEV), offsets=dev[1], centers=dev[2], n_points=np.array(SIZES))
    host_source = ((raw, offsets, centers, cov), None)
    s = ResidentPlots.empty(3000, 9, DEV)
    assert s.P == 0 and s.n_filled == 0 and s.offsets.tolist() == [0] and s.point_capacity == 3000 and s.plot_capacity == 9
    args = make_args(subsample_size=64)
    with pytest.raises(ValueError):
        s.fill([0], 0, 1, args, {})                                                # an empty set is refused on the host
    with pytest.raises(ValueError):
        from stratanet2_vegetation_coverage_maps_amd.train_data import EpochFeeder
        EpochFeeder(s, args, 1, 1)
    assert s.append(src, dev[3], min_points=2000) == 0 and s.version == 0          # nothing kept: no launch, nothing changes
    assert s.append(src, dev[3], select=[8, 1, 6], min_points=5) == 2              # 300 and 255 points; 5 is not > 5
    assert (s.P, s.n_filled, s.n_points_max, s.version) == (2, 555, 300, 1)
    _same_set(s, ResidentPlots.from_plots(*_host_plots(host_source, [8, 1]), DEV))
    with pytest.raises(ValueError, match=r"5 plots and 3630 points"):              # 555 + 3 x 1025 points do not fit 3000
        s.append(src, dev[3], select=[4, 4, 4])
    with pytest.raises(ValueError, match=r"10 plots"):
        s.append(src, dev[3], select=[0] * 8)
    assert (s.P, s.n_filled, s.version) == (2, 555, 1)                             # a refused append changes nothing
    other = ResidentPlots.from_plots(*_host_plots(host_source, [4, 5, 2]), DEV)    # a set as the source: its fp64 rows stay out,
    assert s.append(other, dev[3][[4, 5, 2]].contiguous(), select=[2, 1, 0]) == 3  # the coverages are the argument's
    assert (s.P, s.n_filled, s.n_points_max, s.version) == (5, 555 + 257 + 0 + 1025, 1025, 2)
    want = ResidentPlots.from_plots(*_host_plots(host_source, [8, 1, 2, 5, 4]), DEV)
    _same_set(s, want)
    with pytest.raises(ValueError):
        s.append(s, dev[3][:5].contiguous())
    with pytest.raises(ValueError):
        s.reserve(1836, 9)                                                         # below the fill
    s.reserve(5000, 12)
    assert (s.point_capacity, s.plot_capacity, s.version) == (5000, 12, 3)
    _same_set(s, want)
    assert s.append(src, dev[3], select=[7]) == 1 and s.offsets.tolist()[-2:] == [1837, 1839]
    torch.cuda.synchronize()
