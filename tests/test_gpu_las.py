"""The LAS decoder on the device (csrc/las.hip, las.py) against the tests' own numpy reader (tests/_las_ref.py), bit for bit: every
case of tests/_las_cases.py in both coordinate modes, with and without an origin; decoding into an arena; independence of what
follows the block; the file-level entry points; and the parcel preparation fed from a file."""
import numpy as np
import pytest
import torch

import _las_cases as C
import _las_ref as R
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
from stratanet2_vegetation_coverage_maps_amd import las, parcel
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_parcel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = [("reference", None), ("reference", C.ORIGIN_RAW), ("header", None), ("header", C.ORIGIN_M)]


def dev_bytes(b, extra=0, fill=0):
    """the bytes on the device (a fresh allocation: 16-byte aligned), followed by `extra` bytes of `fill`"""
    a = np.frombuffer(b, dtype=np.uint8)
    if extra:
        a = np.concatenate([a, np.full(extra, fill, dtype=np.uint8)])
    return torch.from_numpy(a.copy()).to(DEV)


def header_of(fmt, L, T):
    return las.LasHeader((1, 4), fmt, L, 375, T, C.SCALE, C.OFFSET, (0.0,) * 3, (0.0,) * 3, 375)


def same(got: torch.Tensor, want: np.ndarray, what=""):
    g = got.cpu().numpy()
    assert g.dtype == want.dtype and g.shape == want.shape, what
    if g.tobytes() != want.tobytes():
        bad = np.argwhere(g.view(np.uint32 if g.dtype == np.float32 else g.dtype) != want.view(np.uint32 if g.dtype == np.float32 else want.dtype))
        raise AssertionError(f"{what}: {len(bad)} values differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")


@pytest.mark.parametrize("name,fmt,L,T", C.CASES, ids=C.CASE_IDS)
def test_every_case_both_modes_bit_for_bit(name, fmt, L, T):
    L = R.LAYOUTS[fmt][1] if L is None else L
    recs = R.pack_records(C.make_fields(T, seed=fmt), fmt, L)
    raw = dev_bytes(recs)
    h = header_of(fmt, L, T)
    for coords, origin in MODES:
        want, want_cls = R.decode_ref(recs, fmt, L, T, coords, origin, C.SCALE, C.OFFSET)
        cloud, cls = las.decode(raw, h, coords, origin, classification=True)
        same(cloud, want, f"{name} {coords} {origin}")
        same(cls, want_cls, f"{name} classification")
        assert tuple(cloud.shape) == (10, T) and cloud.is_contiguous()
    same(las.decode(raw, h), R.decode_ref(recs, fmt, L, T)[0], f"{name} without classification")


def test_the_quotient_at_the_int32_extremes():
    """The fp64 quotient of the `reference` mode and the three separately rounded operations of the `header` mode on the values
    where a shortcut (a reciprocal, an fp32 division, a fused multiply-add) would show."""
    xs = np.array([C.I32_MIN, C.I32_MAX, C.I32_MIN + 1, C.I32_MAX - 1, -1, 1, 49, 50, 51, -49, -50, -51, 686012345, 65012345] +
                  list(range(-300, 300)) + list(np.random.default_rng(9).integers(C.I32_MIN, C.I32_MAX, 3000)), dtype=np.int64)
    T = len(xs)
    f = C.make_fields(T, 2)
    f["X"], f["Y"], f["Z"] = xs.astype(np.int32), xs[::-1].astype(np.int32), np.roll(xs, 7).astype(np.int32)
    recs = R.pack_records(f, 6)
    for coords, origin in MODES + [("reference", (C.I32_MAX, C.I32_MIN, 7)), ("header", (-21474836.48, 1e-3, 123456.789))]:
        want, _ = R.decode_ref(recs, 6, 30, T, coords, origin, C.SCALE, C.OFFSET)
        same(las.decode(dev_bytes(recs), header_of(6, 30, T), coords, origin), want, f"{coords} {origin}")


def test_arena_decode_leaves_the_other_columns_alone():
    fa, fb = C.make_fields(300, 11), C.make_fields(257, 12)
    ra, rb = R.pack_records(fa, 8, 39), R.pack_records(fb, 3)
    wa, ca = R.decode_ref(ra, 8, 39, 300)
    wb, cb = R.decode_ref(rb, 3, 34, 257, "header", C.ORIGIN_M, C.SCALE, C.OFFSET)
    stride, col_a, col_b = 300 + 257 + 13, 5, 5 + 300 + 3
    sentinel = -12345.5
    arena = torch.full((10, stride), sentinel, dtype=torch.float32, device=DEV)
    cls = torch.full((stride,), 0x77, dtype=torch.uint8, device=DEV)
    out = las.decode(dev_bytes(ra), header_of(8, 39, 300), out=arena, col0=col_a, classification=cls)
    assert out[0].data_ptr() == arena.data_ptr()
    las.decode(dev_bytes(rb), header_of(3, 34, 257), "header", C.ORIGIN_M, out=arena, col0=col_b, classification=cls)
    want = np.full((10, stride), sentinel, dtype=np.float32)
    want[:, col_a:col_a + 300], want[:, col_b:col_b + 257] = wa, wb
    want_cls = np.full(stride, 0x77, dtype=np.uint8)
    want_cls[col_a:col_a + 300], want_cls[col_b:col_b + 257] = ca, cb
    same(arena, want, "arena")
    same(cls, want_cls, "classification")
    # a column view of a wider tensor is an arena too (row stride > row length)
    view = torch.full((10, stride), sentinel, dtype=torch.float32, device=DEV)
    las.decode(dev_bytes(ra), header_of(8, 39, 300), out=view[:, col_a:col_a + 300])
    want[:, col_b:col_b + 257] = sentinel
    same(view, want, "view")
    with pytest.raises(ValueError):
        las.decode(dev_bytes(ra), header_of(8, 39, 300), out=arena, col0=stride - 299)


@pytest.mark.parametrize("fmt,L,T", [(8, 38, 257), (8, 41, 255), (6, 131, 100), (0, 20, 1)])
def test_output_does_not_depend_on_what_follows_the_block(fmt, L, T):
    recs = R.pack_records(C.make_fields(T, 21), fmt, L)
    want, want_cls = R.decode_ref(recs, fmt, L, T)
    h = header_of(fmt, L, T)
    for fill in (0x00, 0xFF):
        big = dev_bytes(recs, extra=4096, fill=fill)
        # n_bytes is the block's own length: the view ends where the records end, the allocation goes on
        cloud, cls = las.decode(big[:T * L], h, classification=True)
        same(cloud, want, f"followed by {fill:#x}")
        same(cls, want_cls, f"classification, followed by {fill:#x}")


def test_both_kernel_forms_give_the_same_bytes():
    """Records of at most 128 bytes go through LDS, longer ones are read field by field; sn2_debug_las_form(1) sends a short record
    through the second form."""
    from stratanet2_vegetation_coverage_maps_amd import _lib
    recs = R.pack_records(C.make_fields(1000, 5), 8, 39)
    want, _ = R.decode_ref(recs, 8, 39, 1000)
    raw, h = dev_bytes(recs), header_of(8, 39, 1000)
    try:
        assert _lib.load().sn2_debug_las_form(1) == 0
        direct = las.decode(raw, h)
    finally:
        assert _lib.load().sn2_debug_las_form(0) == 0
    same(direct, want, "direct form")
    same(las.decode(raw, h), want, "staged form")


def write_file(tmp_path, name, fields, fmt, L=None, version=(1, 4), pad=0):
    p = tmp_path / name
    blob = R.write_las(fields, fmt, L, version, scale=C.SCALE, offset=C.OFFSET, pad_after_header=pad)
    p.write_bytes(blob)
    return str(p), blob


def test_load_las_of_a_file(tmp_path):
    for fmt, L, version, pad, T in ((8, None, (1, 4), 0, 1000), (3, 37, (1, 2), 123, 257), (6, None, (1, 4), 54, 1)):
        path, blob = write_file(tmp_path, f"f{fmt}.las", C.make_fields(T, 30 + fmt), fmt, L, version, pad)
        for coords, origin in MODES:
            want, want_cls = R.decode_ref_file(blob, coords, origin)
            cloud, cls = las.load_las(path, DEV, coords, origin, classification=True)
            same(cloud, want, f"format {fmt} {coords}")
            same(cls, want_cls, "classification")
        same(las.load_las(path), R.decode_ref_file(blob)[0], "defaults")
    with pytest.raises(ValueError, match="LAZ"):
        p = tmp_path / "z.las"
        p.write_bytes(R.write_las(C.make_fields(3), 3, format_byte=0x83))
        las.load_las(str(p))


def parcel_fields(cloud):
    """the fields of a synthetic parcel cloud (10,T) whose `reference` decode is that cloud: centimetre integers"""
    f = {k: np.round(cloud[i].astype(np.float64) * 100).astype(np.int32) for i, k in enumerate("XYZ")}
    for i, k in ((3, "red"), (4, "green"), (5, "blue"), (6, "nir"), (7, "intensity")):
        f[k] = np.clip(np.round(cloud[i]), 0, 65535).astype(np.uint16)
    f["returns"] = (np.clip(cloud[8], 0, 15).astype(np.uint8) | (np.clip(cloud[9], 0, 15).astype(np.uint8) << 4))
    return f


def test_load_parcel_clouds_is_from_clouds_of_the_decoded_clouds(tmp_path):
    paths, blobs = [], []
    for k, (T, fmt) in enumerate(((5000, 8), (257, 7), (4097, 8))):
        cloud = make_parcel(30, 20, density=10.0, seed=40 + k, plant=False, x0=650000.0 + 1000 * k)[:, :T]
        p, b = write_file(tmp_path, f"p{k}.las", parcel_fields(cloud), fmt)
        paths.append(p)
        blobs.append(b)
    decoded = [R.decode_ref_file(b)[0] for b in blobs]
    want = parcel.ParcelClouds.from_clouds(decoded, device=DEV)
    got = las.load_parcel_clouds(paths, DEV)
    same(got.arena, want.arena.cpu().numpy(), "arena")
    assert got.point_start.tolist() == want.point_start.tolist() and got.K == 3
    assert got.boxes().tobytes() == want.boxes().tobytes()
    assert got.boxes().tobytes() == np.array([[c[0].min(), c[1].min(), c[0].max(), c[1].max()] for c in decoded], dtype=np.float32).tobytes()
    for k in range(3):
        same(got.cloud(k), decoded[k], f"cloud {k}")


def test_prepare_parcel_from_a_file_is_prepare_parcel_of_the_reference_decode(tmp_path):
    a = make_args()
    cloud = make_parcel(60, 50, density=8.0, seed=1)
    path, blob = write_file(tmp_path, "parcel.las", parcel_fields(cloud), 8)
    want = parcel.prepare_parcel(R.decode_ref_file(blob)[0], a, device=DEV)
    got = parcel.prepare_parcel(las.load_las(path, DEV), a)
    assert len(want.plot_ids) > 4
    same(got.raw, want.raw.cpu().numpy(), "raw")
    same(got.offsets, want.offsets.cpu().numpy(), "offsets")
    assert list(got.plot_ids) == list(want.plot_ids)


def test_load_plot_is_znorm_of_the_reference_decode(tmp_path):
    a = make_args()
    cloud = make_parcel(12, 12, density=8.0, seed=3, plant=False)
    path, blob = write_file(tmp_path, "plot.las", parcel_fields(cloud), 8, version=(1, 4), pad=54)
    ref = R.decode_ref_file(blob)[0]
    zout = ops.znorm(torch.from_numpy(np.ascontiguousarray(ref[:3])).to(DEV), float(getattr(a, "znorm_radius_in_meters", 1.5)))[1]
    want = ref.copy()
    want[2] = zout.cpu().numpy()
    got = las.load_plot(path, a, DEV)
    same(got, want, "plot")
    assert (want[2] >= 0).all() and (want[2] != ref[2]).any()
