"""Orthoimage colours on the device (csrc/ortho.hip, ortho.py) against the numpy statement of the rule (ortho.colorize_ref), bit for
bit: every planted case of tests/_ortho_cases.py with every pixel type and both layouts, inside an arena with poisoned guard bands;
many workgroups; a ParcelClouds in one launch; the shifted frame; determinism; and LAS files end to end."""
import numpy as np
import pytest
import torch

import _las_cases as LC
import _las_ref as LR
import _ortho_cases as oc
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
from stratanet2_vegetation_coverage_maps_amd import las, ortho, parcel
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_parcel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 67                            # columns of poison on either side (no multiple of anything)
POISON = np.uint32(0xDEADBEEF)


def same(got, want, what=""):
    g = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert g.dtype == want.dtype and g.shape == want.shape, what
    if g.tobytes() != want.tobytes():
        bits = np.uint32 if g.dtype == np.float32 else g.dtype
        bad = np.argwhere(g.view(bits) != want.view(bits))
        raise AssertionError(f"{what}: {len(bad)} values differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")


def make_set(name, dtype, layout, on_device=False):
    images, nodata, origin = oc.case_images(name, dtype, layout)
    px = [torch.from_numpy(p).to(DEV) if on_device else p for p, *_ in images]
    return ortho.OrthoSet([ortho.OrthoImage(p, x0, y0, a, b, layout=layout) for p, (_, x0, y0, a, b) in zip(px, images)], nodata=nodata), origin


def guarded(cloud):
    """the cloud in the middle of a poisoned (10, GUARD + T + GUARD) arena"""
    arena = np.full((10, cloud.shape[1] + 2 * GUARD), POISON, dtype=np.uint32).view(np.float32)
    arena[:, GUARD:GUARD + cloud.shape[1]] = cloud
    return arena


@pytest.mark.parametrize("layout", oc.LAYOUTS)
@pytest.mark.parametrize("dtype", oc.DTYPES)
@pytest.mark.parametrize("name", oc.CASE_NAMES)
def test_every_case_bit_for_bit(name, dtype, layout):
    """Rows, `covered` and `missing` against colorize_ref; the rows not asked for, the unserved columns and the guard bands on
    both sides of col0 .. col0 + T keep their bytes (col0 = GUARD > 0 inside a larger arena)."""
    oset, origin = make_set(name, dtype, layout, on_device=(layout == "planar"))
    bands, rows = oc.case_map(name)
    scale = oc.SCALE[dtype]
    cloud = oc.cloud_of(oc.case_points(name), oc.T_SMALL, seed=1)
    ref = ortho.colorize_ref(cloud, oset, bands=bands, rows=rows, scale=scale, origin=origin, covered=True)
    assert 0 < ref.missing < oc.T_SMALL and set(ref.covered.tolist()) == set(range(len(oset.images) + 1))
    want = guarded(ref.cloud)
    # the C ABI's form: columns col0 .. col0 + T of the arena
    arena = torch.from_numpy(guarded(cloud)).to(DEV)
    shifted = oset if origin is None else oset.shifted(origin)
    cov = torch.full((oc.T_SMALL,), 0xEE, dtype=torch.uint8, device=DEV)
    missing = ops.ortho_colorize(arena, shifted.struct(DEV, bands, rows, scale), col0=GUARD, T=oc.T_SMALL, covered=cov)
    same(arena, want, f"{name} {dtype} {layout}: arena")
    same(cov, ref.covered, "covered")
    assert int(missing) == ref.missing
    # the package's form, on a column view of the same arena
    arena = torch.from_numpy(guarded(cloud)).to(DEV)
    res = ortho.colorize(arena[:, GUARD:GUARD + oc.T_SMALL], oset, bands=bands, rows=rows, scale=scale, origin=origin, covered=True)
    assert isinstance(res.missing, torch.Tensor) and res.missing.is_cuda and res.missing.dtype == torch.int64
    same(arena, want, f"{name} {dtype} {layout}: view")
    same(res.covered, ref.covered, "covered")
    assert int(res.missing) == ref.missing


def _large_cloud():
    rng = np.random.default_rng(11)
    xy = oc.case_points("overlap_nodata")
    cloud = oc.cloud_of(xy, oc.T_LARGE, seed=2)
    n = oc.T_LARGE - xy.shape[1]
    cloud[0, xy.shape[1]:] = (rng.random(n) * 6 - 1).astype(np.float32)
    cloud[1, xy.shape[1]:] = (rng.random(n) * 5 - 1).astype(np.float32)
    return cloud


@pytest.mark.parametrize("dtype,layout", [("uint8", "chunky"), ("uint16", "planar")])
def test_many_workgroups_and_the_same_bytes_twice(dtype, layout):
    oset, _ = make_set("overlap_nodata", dtype, layout)
    cloud = _large_cloud()
    ref = ortho.colorize_ref(cloud, oset, bands=(2, 1, 0, 1), rows=(9, 3, 6, 4), scale=oc.SCALE[dtype], covered=True)
    assert 1000 < ref.missing < oc.T_LARGE - 1000
    runs = []
    for _ in range(2):
        dev = torch.from_numpy(cloud).to(DEV)
        res = ortho.colorize(dev, oset, bands=(2, 1, 0, 1), rows=(9, 3, 6, 4), scale=oc.SCALE[dtype], covered=True)
        runs.append((dev.cpu().numpy(), res.covered.cpu().numpy(), int(res.missing)))
    same(runs[0][0], ref.cloud, "cloud")
    same(runs[0][1], ref.covered, "covered")
    assert runs[0][2] == ref.missing
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes() and runs[0][2] == runs[1][2]


def test_parcel_clouds_in_one_launch_equal_k_single_launches():
    oset, _ = make_set("rgb_half", "uint8", "chunky")
    xy = oc.case_points("rgb_half")
    clouds = [oc.cloud_of(xy, 300, seed=5), oc.cloud_of(xy[:, ::-1], 129, seed=6), oc.cloud_of(xy, 77, seed=7)]
    clouds[2][0] += np.float32(1000.0)                                    # the third parcel lies outside every image
    pc = parcel.ParcelClouds.from_clouds(clouds, device=DEV)
    res = ortho.colorize(pc, oset, covered=True)
    assert res.cloud is pc and tuple(res.covered.shape) == (300 + 129 + 77,)
    singles = [ortho.colorize(torch.from_numpy(c).to(DEV), oset, covered=True) for c in clouds]
    refs = [ortho.colorize_ref(c, oset, covered=True) for c in clouds]
    assert refs[2].missing == 77 and 0 < refs[0].missing < 300
    for k in range(3):
        same(pc.cloud(k).contiguous(), refs[k].cloud, f"parcel {k}")
        same(singles[k].cloud, refs[k].cloud, f"single {k}")
        same(res.covered[int(pc.point_start[k]):int(pc.point_start[k + 1])], refs[k].covered, f"covered {k}")
        same(singles[k].covered, refs[k].covered, f"single covered {k}")
    assert int(res.missing) == sum(int(s.missing) for s in singles) == sum(r.missing for r in refs)


def test_shifted_frame_equals_the_unshifted_one_on_representable_coordinates():
    """An image at Lambert-93 magnitudes with a corner and pixel size exact in binary; points on a 1/16 m x 1/2 m lattice, which
    fp32 holds exactly at those magnitudes AND after the shift: both frames must give the same rows."""
    origin = (650000.0, 6799990.0)
    px = oc.typed(oc.samples(6, 7, 3, 4), "uint8", "chunky")
    oset = ortho.OrthoSet([ortho.OrthoImage(px, 650000.5, 6800000.0, 0.5)])
    gx, gy = np.meshgrid(np.arange(-1.0, 5.0, 1 / 16), np.arange(5.0, 11.5, 0.5))
    local = np.stack([gx.reshape(-1), gy.reshape(-1)])
    world = (local + np.array(origin)[:, None]).astype(np.float32)
    assert np.array_equal(world.astype(np.float64) - np.array(origin)[:, None], local)
    T = local.shape[1]
    a, b = oc.cloud_of(world, T, seed=8), oc.cloud_of(local.astype(np.float32), T, seed=8)
    ra = ortho.colorize(torch.from_numpy(a).to(DEV), oset, covered=True)
    rb = ortho.colorize(torch.from_numpy(b).to(DEV), oset, origin=origin, covered=True)
    same(ra.cloud[2:], rb.cloud[2:].cpu().numpy(), "rows 2..9")
    same(ra.covered, rb.covered.cpu().numpy(), "covered")
    assert 0 < int(ra.missing) == int(rb.missing) < T
    same(rb.cloud, ortho.colorize_ref(b, oset, origin=origin).cloud, "against the rule")


def _las_fields(T, seed):
    """fields of T records whose `reference` coordinates lie inside a 4 m x 4 m square (centimetre integers, edges included)"""
    rng = np.random.default_rng(seed)
    f = LC.make_fields(T, seed)
    f["X"] = rng.integers(0, 400, size=T).astype(np.int32)
    f["Y"] = rng.integers(1, 401, size=T).astype(np.int32)
    f["X"][:4], f["Y"][:4] = [0, 399, 50, 200], [400, 1, 350, 200]
    f["Z"] = rng.integers(-500, 3000, size=T).astype(np.int32)
    return f


@pytest.mark.parametrize("origin", [None, (100, -200, 7)])
def test_format_6_file_coloured_equals_the_format_8_file_that_carries_the_colours(tmp_path, origin):
    """A format-6 file (no colour fields) decoded and coloured from a tiny RGB and a tiny IRC image, against a format-8 file
    that carries pixel * 256 in its colour fields at the same points, through las.load_las: the two clouds bit for bit."""
    T = 300
    f = _las_fields(T, 21)
    rng = np.random.default_rng(22)
    rgb = ortho.OrthoImage(rng.integers(0, 256, size=(8, 8, 3), dtype=np.uint8), 0.0, 4.0 + 0.01, 0.5 + 1 / 512)
    irc = ortho.OrthoImage(rng.integers(0, 256, size=(5, 4, 3), dtype=np.uint8), -0.26, 4.503, 1.25, 1.0)
    plain = tmp_path / "plain.las"
    plain.write_bytes(LR.write_las(f, 6, version=(1, 4)))
    bare = LR.decode_ref_file(plain.read_bytes())[0]
    assert (bare[3:7] == 0).all()
    painted = ortho.colorize_ref(ortho.colorize_ref(bare, rgb).cloud, irc, bands=(0,), rows=(6,))
    assert painted.missing == 0
    for k, row in (("red", 3), ("green", 4), ("blue", 5), ("nir", 6)):
        f[k] = painted.cloud[row].astype(np.uint16)
        assert np.array_equal(f[k].astype(np.float32), painted.cloud[row])
    coloured = tmp_path / "coloured.las"
    coloured.write_bytes(LR.write_las(f, 8, version=(1, 4)))
    want = las.load_las(str(coloured), DEV, origin=origin)
    got = ortho.load_las_colorized(str(plain), rgb, irc, device=DEV, origin=origin)
    same(got, want.cpu().numpy(), "the coloured cloud")
    assert float(got[3:7].abs().sum()) > 0
    # the same through the header's scale and offset, origin in metres
    o = None if origin is None else (1.0, -2.0, 0.07)
    want = las.load_las(str(coloured), DEV, coords="header", origin=o)
    got, cls = ortho.load_las_colorized(str(plain), ortho.OrthoSet([rgb]), ortho.OrthoSet([irc]), device=DEV, coords="header", origin=o,
                                        classification=True)
    same(got, want.cpu().numpy(), "the coloured cloud, header mode")
    assert tuple(cls.shape) == (T,)


def test_prepare_parcel_runs_on_a_coloured_cloud():
    cloud = make_parcel(60, 50, density=8.0, seed=1)
    cloud[3:7] = 0.0
    x0, y1 = float(np.floor(cloud[0].min())), float(np.ceil(cloud[1].max()))
    W, H = int(np.ceil((cloud[0].max() - x0) / 0.5)) + 1, int(np.ceil((y1 - cloud[1].min()) / 0.5)) + 1
    rng = np.random.default_rng(3)
    rgb = ortho.OrthoImage(rng.integers(1, 256, size=(H, W, 3), dtype=np.uint8), x0, y1, 0.5)
    irc = ortho.OrthoImage(rng.integers(1, 256, size=(H, W), dtype=np.uint8), x0, y1, 0.5)
    dev = torch.from_numpy(cloud).to(DEV)
    assert int(ortho.colorize(dev, rgb).missing) == 0 and int(ortho.colorize(dev, irc, bands=(0,), rows=(6,)).missing) == 0
    same(dev, ortho.colorize_ref(ortho.colorize_ref(cloud, rgb).cloud, irc, bands=(0,), rows=(6,)).cloud, "coloured parcel")
    plots = parcel.prepare_parcel(dev, make_args())
    assert len(plots.plot_ids) > 4
    assert float(dev[3:7].min()) >= 256.0
