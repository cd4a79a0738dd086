"""K parcels prepared in one pass over a cloud arena (parcel.ParcelClouds, prepare_parcels(batched=True), csrc/parcels.hip) against
the loop over `prepare_parcel` (byte for byte), against scipy's discs and the oracle's z-normalisation (independent of the loop),
and the two device-to-host reads the batched sequence is allowed.  60 m x 50 m parcels at about 8 points/m^2: the smallest that
hold every case."""
import numpy as np
import pytest
import torch

from oracle.prepare import normalize_z_with_minz_in_a_radius
from stratanet2_vegetation_coverage_maps_amd import parcel
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_parcel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FIELDS = ("raw", "offsets", "point_index", "centers", "n_points", "plot_index", "plot_ids", "centers_host", "parcel_of", "parcel_start")
SEED = 20240611


def hole_rings(cloud):
    """a pentagon with a triangular hole inside the parcel's box"""
    x0, x1, y0, y1 = (float(v) for v in (cloud[0].min(), cloud[0].max(), cloud[1].min(), cloud[1].max()))
    return [np.array([[x0 + 1.6, y0 + 1.35], [x1 - 2.05, y0 + 1.65], [x1 - 1.45, y1 - 1.8], [0.5 * (x0 + x1), y1 - 15.5], [x0 + 1.25, y1 - 2.2]]),
            np.array([[x0 + 10.0, y0 + 10.0], [x0 + 10.0, y0 + 15.75], [x0 + 16.5, y0 + 14.5]])]


def far_ring(cloud):
    """a square 10 km away: its buffer keeps no lattice centre"""
    x0, y0 = float(cloud[0].min()) + 10000.0, float(cloud[1].min())
    return [np.array([[x0, y0], [x0 + 50, y0], [x0 + 50, y0 + 50], [x0, y0 + 50]])]


@pytest.fixture(scope="module")
def seven():
    """(args, clouds, shapes): dense with the planted 50 / 51-point discs; its shuffled twin at the SAME coordinates; sparse, no kept
    plot; T = L + 1; T < 64; a shape that keeps no centre; a polygon with a hole"""
    a = make_args()
    dense = make_parcel(60, 50, density=8.0, seed=1)
    twin = np.ascontiguousarray(dense[:, np.random.default_rng(5).permutation(dense.shape[1])])
    sparse = make_parcel(60, 50, density=0.02, seed=2, plant=False, x0=651000.0)
    other = make_parcel(60, 50, density=8.0, seed=3, plant=False, x0=652000.0)
    row_plus_one = np.ascontiguousarray(other[:, :parcel.ROW_POINTS + 1])
    tiny = np.ascontiguousarray(make_parcel(60, 50, density=8.0, seed=4, plant=False, x0=653000.0)[:, :50])
    no_centre = make_parcel(60, 50, density=8.0, seed=5, plant=False, x0=654000.0)
    holed = make_parcel(60, 50, density=8.0, seed=6, plant=False, x0=655000.0)
    clouds = [dense, twin, sparse, row_plus_one, tiny, no_centre, holed]
    shapes = [None, None, None, None, None, far_ring(no_centre), hole_rings(holed)]
    assert row_plus_one.shape[1] == 2049 and tiny.shape[1] < 64
    return a, clouds, shapes


def as_bytes(s):
    out = {}
    for f in FIELDS:
        v = getattr(s, f)
        if isinstance(v, torch.Tensor):
            v = (v.view(torch.int32) if v.dtype == torch.float32 else v).cpu().numpy()
        out[f] = (list(v) if isinstance(v, list) else (str(v.dtype), v.shape, v.tobytes()))
    return out


def assert_same_set(got, want):
    g, w = as_bytes(got), as_bytes(want)
    for f in FIELDS:
        assert g[f] == w[f], f


@pytest.fixture(scope="module")
def prepared(seven):
    a, clouds, shapes = seven
    loop = parcel.prepare_parcels(clouds, a, shapes=shapes, batched=False)
    batched = parcel.prepare_parcels(clouds, a, shapes=shapes, batched=True)
    torch.cuda.synchronize()
    return loop, batched


def test_batched_set_is_the_loops_set_byte_for_byte(seven, prepared):
    a, clouds, shapes = seven
    loop, batched = prepared
    n = np.diff(loop.parcel_start)
    print(f"\nplots per parcel: {n.tolist()}, plot points {int(loop.n_points.sum())}")
    assert isinstance(batched, parcel.ParcelSet) and batched.n_parcels == 7
    assert n[0] == n[1] > 8 and n[2] == 0 and n[3] > 0 and n[4] == 0 and n[5] == 0 and n[6] > 8        # the cases are what their names say
    # the planted discs: 50 points (dropped) and 51 + the box's corner point, which lies in that disc at this parcel size (kept)
    assert 52 in loop.n_points[:n[0]] and 50 not in loop.n_points[:n[0]] and loop.n_points.min() >= 51
    assert_same_set(batched, loop)
    # point_index is relative to the plot's own parcel
    T = np.array([c.shape[1] for c in clouds])
    pidx, off = batched.point_index.cpu().numpy(), batched.offsets.cpu().numpy()
    for j, k in enumerate(batched.parcel_of):
        seg = pidx[off[j]:off[j + 1]]
        assert seg.min() >= 0 and seg.max() < T[k] and (np.diff(seg) > 0).all()


def test_min_points_2001_and_an_all_empty_set(seven):
    a, clouds, shapes = seven
    loop = parcel.prepare_parcels(clouds, a, shapes=shapes, batched=False, min_points=2001)
    batched = parcel.prepare_parcels(clouds, a, shapes=shapes, batched=True, min_points=2001)
    assert 0 < len(loop) and (loop.n_points >= 2001).all()
    assert_same_set(batched, loop)
    empties, eshapes = [clouds[2], clouds[4], clouds[5], clouds[2]], [None, None, shapes[5], None]
    loop = parcel.prepare_parcels(empties, a, shapes=eshapes, batched=False)
    batched = parcel.prepare_parcels(empties, a, shapes=eshapes, batched=True)
    assert len(loop) == 0 and loop.n_parcels == 4 and loop.parcel_start.tolist() == [0] * 5
    assert_same_set(batched, loop)
    # no centre anywhere: nothing to count
    none = parcel.prepare_parcels([clouds[5], clouds[5]], a, shapes=[shapes[5], shapes[5]], batched=True)
    assert_same_set(none, parcel.prepare_parcels([clouds[5], clouds[5]], a, shapes=[shapes[5], shapes[5]], batched=False))


def test_discs_and_z_against_scipy_and_the_oracle(seven, prepared):
    """independent of the loop: the shuffled twin (every point of parcel 0 lies on one of its own) and the polygon with a hole"""
    from scipy.spatial import cKDTree
    a, clouds, shapes = seven
    _, got = prepared
    off, pidx, raw = got.offsets.cpu().numpy(), got.point_index.cpu().numpy(), got.raw.cpu().numpy()
    rows = [0, 1] + list(range(3, 10))
    for k in (1, 6):
        cloud = clouds[k]
        keep = parcel.polygon_keep(shapes[k], parcel.shape_buffer(a)) if shapes[k] is not None else None
        centers = parcel.parcel_plot_centers(cloud[0].min(), cloud[0].max(), cloud[1].min(), cloud[1].max(), a, keep)
        tree = cKDTree(cloud[:2].T, leafsize=50)
        discs = [np.array(sorted(tree.query_ball_point(c, r=a.diam_meters // 2)), dtype=np.int64) for c in centers]
        kept = [p for p, d in enumerate(discs) if len(d) >= 51]
        j0, j1 = got.parcel_start[k], got.parcel_start[k + 1]
        assert list(got.plot_index[j0:j1]) == kept and len(kept) > 0
        assert np.array_equal(got.centers_host[j0:j1], centers[kept])
        smallest = sorted(kept, key=lambda p: len(discs[p]))[:8]
        for j, p in zip(range(j0, j1), kept):
            assert np.array_equal(pidx[off[j]:off[j + 1]], discs[p]), (k, p)
            assert raw[rows, off[j]:off[j + 1]].tobytes() == cloud[:, discs[p]][rows].tobytes(), (k, p)
            if p in smallest:
                ref = normalize_z_with_minz_in_a_radius(cloud[:, discs[p]], 1.5)[2]
                assert raw[2, off[j]:off[j + 1]].tobytes() == ref.tobytes(), (k, p)


def test_boxes_equal_torch_min_max_bit_for_bit(seven):
    a, clouds, shapes = seven
    big = make_parcel(60, 50, density=8.0, seed=7, x0=-30.0, y0=-20.0, plant=False)       # both signs, several workgroups
    assert big.shape[1] > 2 * 4096 and big[0].min() < 0 < big[0].max()
    one_point = np.ascontiguousarray(clouds[3][:, 17:18])
    cs = [clouds[0], one_point, big, clouds[4], clouds[3]]
    pc = parcel.ParcelClouds.from_clouds(cs, DEV)
    assert pc.K == 5 and pc.arena.shape == (10, sum(c.shape[1] for c in cs)) and pc.point_start.tolist() == np.concatenate(
        [[0], np.cumsum([c.shape[1] for c in cs])]).tolist()
    got = pc.boxes()
    again = pc.boxes()
    assert got.dtype == np.float32 and got.shape == (5, 4) and got.tobytes() == again.tobytes()
    for k, c in enumerate(cs):
        t = torch.from_numpy(c).to(DEV)
        want = torch.cat([t[:2].min(1).values, t[:2].max(1).values]).cpu().numpy()
        assert got[k].tobytes() == want.tobytes(), k
        assert torch.equal(pc.cloud(k), t)
    for bad in ([clouds[0][:9]], [clouds[0][:, :0]], [clouds[0][0]], []):
        with pytest.raises(ValueError):
            parcel.ParcelClouds.from_clouds(bad, DEV)


@pytest.mark.parametrize("K", [2, 7])
def test_two_host_reads_and_nothing_else(seven, prepared, monkeypatch, K):
    a, clouds, shapes = seven
    dev_clouds = [torch.from_numpy(c).to(DEV) for c in clouds[:K]]
    torch.cuda.synchronize()
    counts = {"item": 0, "cpu": 0, "tolist": 0, "numpy": 0, "synchronize": 0}

    def counted(name, fn):
        def wrapper(*args, **kw):
            if name == "synchronize" or args[0].is_cuda:
                counts[name] += 1
            return fn(*args, **kw)
        return wrapper
    for name in ("item", "cpu", "tolist", "numpy"):
        monkeypatch.setattr(torch.Tensor, name, counted(name, getattr(torch.Tensor, name)))
    monkeypatch.setattr(torch.cuda, "synchronize", counted("synchronize", torch.cuda.synchronize))
    got = parcel.prepare_parcels(dev_clouds, a, shapes=shapes[:K], batched=True)
    monkeypatch.undo()
    print(f"\ndevice-to-host reads of prepare_parcels(batched=True), K = {K}: {counts}")
    assert counts == {"item": 0, "cpu": 2, "tolist": 0, "numpy": 0, "synchronize": 0}
    assert len(got) == prepared[0].parcel_start[K]


def test_two_calls_give_the_same_bytes(seven, prepared):
    a, clouds, shapes = seven
    pc = parcel.ParcelClouds.from_clouds(clouds, DEV)
    first = parcel.prepare_parcels(pc, a, shapes=shapes, batched=True)
    second = parcel.prepare_parcels(pc, a, shapes=shapes, batched=True)
    assert_same_set(first, second)
    assert_same_set(first, prepared[1])
    # a ParcelClouds goes through the loop as well, and None chooses the batched pass for K >= 2
    assert_same_set(parcel.prepare_parcels(pc, a, shapes=shapes, batched=False), prepared[0])
    assert_same_set(parcel.prepare_parcels(pc, a, shapes=shapes), prepared[0])


def test_predict_parcels_batched_and_looped_prepare_give_the_same_atlas(seven):
    from stratanet2_vegetation_coverage_maps_amd import PointNet2
    _, clouds, shapes = seven
    a = make_args(cuda=0, subsample_size=1024)
    torch.manual_seed(3)
    model = PointNet2(a).eval()
    ks = [0, 2, 5, 6]
    cs, sh = [clouds[k] for k in ks], [shapes[k] if shapes[k] is not None else hole_rings(clouds[k]) for k in ks]
    out = []
    for batched in (True, False):
        atlas, plots = parcel.predict_parcels(model, cs, a, shapes=sh, batch_size=512, seed=SEED, fps_start=0, batched=batched)
        rep = atlas.report(sh)
        words = [t.view(torch.int32).cpu().numpy() for t in (atlas.mean, atlas.wsum, rep.band_arena)]
        out.append((words + [rep.thresholds.view(np.int64), rep.band_means.view(np.int64), rep.band_counts], as_bytes(plots)))
    assert len(out[0][0][0]) > 0 and out[0][1] == out[1][1]
    for x, y in zip(out[0][0], out[1][0]):
        assert np.array_equal(x, y)
