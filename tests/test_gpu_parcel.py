"""Parcel -> plots on the device (parcel.py, csrc/parcel.hip) against the reference's CPU preparation: scipy's cKDTree discs
(`extract_cloud`, sorted: this package's order) and the oracle's per-plot z-normalisation (`pre_transform`)."""
import numpy as np
import pytest
import torch

from oracle.prepare import normalize_z_with_minz_in_a_radius
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
from stratanet2_vegetation_coverage_maps_amd import parcel
from stratanet2_vegetation_coverage_maps_amd.inference import predict_parcel
from stratanet2_vegetation_coverage_maps_amd.input_pipeline import prepare_batch
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_parcel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def lattice_of(cloud, args):
    return parcel.parcel_plot_centers(cloud[0].min(), cloud[0].max(), cloud[1].min(), cloud[1].max(), args)


def scipy_discs(cloud, centers, args):
    from scipy.spatial import cKDTree
    tree = cKDTree(cloud[:2].T, leafsize=50)
    return [np.array(sorted(tree.query_ball_point(c, r=args.diam_meters // 2)), dtype=np.int64) for c in centers]


def znorm_kdtree(plot, radius=1.5):
    """normalize_z_with_minz_in_a_radius through scipy's kd-tree (inclusive, fp64): the oracle at sizes its O(n^2) loop
    cannot reach; held to the oracle on small plots below."""
    from scipy.spatial import cKDTree
    xy = plot[:2].T.astype(np.float64)
    z = plot[2]
    nb = cKDTree(xy).query_ball_point(xy, radius)
    zmin = np.array([z[n].min() for n in nb], dtype=np.float32)
    return (z - zmin).astype(np.float32)


def cpu_plots(cloud, args, centers=None):
    centers = lattice_of(cloud, args) if centers is None else centers
    discs = scipy_discs(cloud, centers, args)
    kept = [k for k, d in enumerate(discs) if len(d) >= 51]
    return centers, discs, kept


@pytest.fixture(scope="module", params=["scanline", "shuffled"])
def small(request):
    args = make_args()
    cloud = make_parcel(order=request.param, seed=11)
    centers, discs, kept = cpu_plots(cloud, args)
    plots = parcel.prepare_parcel(cloud, args)
    torch.cuda.synchronize()
    return args, cloud, centers, discs, kept, plots


def test_extraction_matches_scipy(small):
    args, cloud, centers, discs, kept, plots = small
    counts = np.array([len(d) for d in discs])
    assert 50 in counts and 51 in counts                           # the planted discs: dropped / kept
    np.testing.assert_array_equal(plots.plot_index, kept)
    np.testing.assert_array_equal(plots.n_points, counts[kept])
    off = plots.offsets.cpu().numpy()
    np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(counts[kept])]))
    pidx = plots.point_index.cpu().numpy()
    raw = plots.raw.cpu().numpy()
    for j, k in enumerate(kept):
        np.testing.assert_array_equal(pidx[off[j]:off[j + 1]], discs[k])
        ref = cloud[:, discs[k]]
        rows = [0, 1] + list(range(3, 10))
        assert raw[rows, off[j]:off[j + 1]].tobytes() == ref[rows].tobytes()
    np.testing.assert_array_equal(plots.centers.cpu().numpy(), centers[kept])
    assert plots.plot_ids == [parcel.plot_id(k, centers[k]) for k in kept]


def test_znorm_is_per_plot_and_matches_the_oracle(small):
    args, cloud, centers, discs, kept, plots = small
    off = plots.offsets.cpu().numpy()
    zrow = plots.raw[2].cpu().numpy()
    whole = ops.znorm(torch.from_numpy(np.ascontiguousarray(cloud[:3])).to(DEV), 1.5)[1].cpu().numpy()
    differs = 0
    for j, k in enumerate(kept):
        ref = normalize_z_with_minz_in_a_radius(cloud[:, discs[k]], 1.5)[2]
        assert zrow[off[j]:off[j + 1]].tobytes() == ref.tobytes(), f"plot {k}"
        differs += int(np.count_nonzero(zrow[off[j]:off[j + 1]] != whole[discs[k]]))
    assert differs > 0                     # disc-edge points whose lowest neighbour lies outside the disc: a parcel-wide
    #                                        z-norm is not the reference's rule


def test_kdtree_restatement_matches_the_oracle(small):
    args, cloud, centers, discs, kept, plots = small
    for k in kept[:6]:
        p = cloud[:, discs[k]]
        assert znorm_kdtree(p).tobytes() == normalize_z_with_minz_in_a_radius(p, 1.5)[2].tobytes()


def test_output_is_deterministic():
    args = make_args()
    cloud = torch.from_numpy(make_parcel(order="shuffled", seed=5, density=8.0)).to(DEV)
    a = parcel.prepare_parcel(cloud, args)
    b = parcel.prepare_parcel(cloud, args)
    for name in ("raw", "offsets", "point_index"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.shape == y.shape and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), name


def test_batches_equal_prepare_batch(small):
    args, cloud, centers, discs, kept, plots = small
    a = make_args(subsample_size=700)
    mine = list(plots.batches(a, 7, rs=np.random.RandomState(5)))
    rs = np.random.RandomState(5)
    assert len(mine) == -(-len(kept) // 7)
    for b, d in enumerate(mine):
        ks = kept[7 * b:7 * b + 7]
        plots_cpu = [normalize_z_with_minz_in_a_radius(cloud[:, discs[k]], 1.5) for k in ks]
        ref = prepare_batch(plots_cpu, centers[ks], a, train=False, rs=rs)
        assert torch.equal(d["cloud"], ref["cloud"]) and torch.equal(d["xyz"], ref["xyz"]), f"batch {b}"
        np.testing.assert_array_equal(d["plot_center"], centers[ks])


def test_predict_parcel_cloud_end_to_end(small):
    from stratanet2_vegetation_coverage_maps_amd import PointNet2
    args, cloud, centers, discs, kept, plots = small
    a = make_args(cuda=0, subsample_size=1024)
    torch.manual_seed(3)
    model = PointNet2(a).eval()
    mos, pl = parcel.predict_parcel_cloud(model, cloud, a, batch_size=16, rs=np.random.RandomState(2), fps_start=0)
    assert list(pl.plot_index) == kept
    ref_mos = parcel.parcel_mosaic(centers[kept], a, DEV)
    assert ref_mos.mean.shape == mos.mean.shape
    rs = np.random.RandomState(2)
    batches = []
    for s in range(0, len(kept), 16):
        ks = kept[s:s + 16]
        d = prepare_batch([normalize_z_with_minz_in_a_radius(cloud[:, discs[k]], 1.5) for k in ks], centers[ks], a, train=False,
                          rs=rs)
        d.update(plot_center=centers[ks], fps_start=torch.zeros(2, len(ks), dtype=torch.int64))
        batches.append(d)
    assert predict_parcel(model, batches, ref_mos, a) == len(kept)
    got, ref = mos.result(), ref_mos.result()
    assert (~torch.isnan(got[0])).any()
    assert torch.equal(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(ref, nan=-7.0))
    out, thr = mos.finalize()
    assert out.shape[0] == 5


def test_scale_parcel_matches_scipy():
    args = make_args()
    cloud = make_parcel(316.3, 316.3, density=42.0, seed=2)
    assert cloud.shape[1] >= 4_000_000
    centers, discs, kept = cpu_plots(cloud, args)
    assert len(kept) >= 600
    plots = parcel.prepare_parcel(cloud, args)
    np.testing.assert_array_equal(plots.plot_index, kept)
    np.testing.assert_array_equal(plots.n_points, [len(discs[k]) for k in kept])
    pidx = plots.point_index.cpu().numpy()
    np.testing.assert_array_equal(pidx, np.concatenate([discs[k] for k in kept]))
    off = plots.offsets.cpu().numpy()
    zrow = plots.raw[2].cpu().numpy()
    for j in np.random.RandomState(0).choice(len(kept), 16, replace=False):
        k = kept[j]
        assert zrow[off[j]:off[j + 1]].tobytes() == znorm_kdtree(cloud[:, discs[k]]).tobytes(), f"plot {k}"


def test_edges():
    args = make_args()
    cloud = make_parcel(order="shuffled", seed=4)
    far = np.array([[1e6, 2e6], [cloud[0].min() - 50, cloud[1].min()]], dtype=np.float32)
    empty = parcel.prepare_parcel(cloud, args, centers=far)                        # centres far outside: no plot
    assert len(empty) == 0 and empty.raw.shape == (10, 0) and empty.offsets.cpu().tolist() == [0]
    assert len(parcel.prepare_parcel(cloud[:, :30], args)) == 0                    # too few points for any plot
    assert len(parcel.prepare_parcel(cloud, args, centers=np.zeros((0, 2), np.float32))) == 0
    mos, pl = parcel.predict_parcel_cloud(None, cloud, args, centers=far)
    assert mos is None and len(pl) == 0
    lat = lattice_of(cloud, args)
    one = lat[40:41]
    p1 = parcel.prepare_parcel(cloud, args, centers=one)                           # a single centre
    d = scipy_discs(cloud, one, args)[0]
    assert len(p1) == 1 and p1.point_index.cpu().numpy().tolist() == d.tolist()
    mixed = np.concatenate([far[:1], lat[40:43], lat[40:41], far[1:], lat[:2]]).astype(np.float32)   # duplicates, far ones
    pm = parcel.prepare_parcel(cloud, args, centers=mixed)
    discs = scipy_discs(cloud, mixed, args)
    kept = [k for k, dd in enumerate(discs) if len(dd) >= 51]
    np.testing.assert_array_equal(pm.plot_index, kept)
    np.testing.assert_array_equal(pm.point_index.cpu().numpy(), np.concatenate([discs[k] for k in kept]))
    off = pm.offsets.cpu().numpy()
    zrow = pm.raw[2].cpu().numpy()
    for j, k in enumerate(kept):
        assert zrow[off[j]:off[j + 1]].tobytes() == normalize_z_with_minz_in_a_radius(cloud[:, discs[k]], 1.5)[2].tobytes()
