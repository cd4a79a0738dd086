"""The LAS decoder without a device: records typed out by hand pin the bit positions of the tests' own reader (tests/_las_ref.py:
`decode_ref`, which the GPU tests hold the kernel to); las.read_header round trips and refuses; planted wrong restatements of the
rule each differ from `decode_ref` on the cases; the argument checks of sn2_las_decode return their codes before any device work."""
import ctypes

import numpy as np
import pytest

import _las_cases as C
import _las_ref as R

H = float.fromhex
# ---- hand-written records.  Typed as the bytes a file holds, with the ten values and the classification they must give in the
# `reference` mode (coordinates: the raw integer / 100 as the nearest fp32, written as hex floats).
# format 8, 38 bytes: X Y Z | intensity | byte 14 | flags | class | user | scan angle | source id | GPS time | R G B | NIR
FMT8_A = bytes.fromhex("7902e003 b9b7e328 00000080  ffff 5a ff 05 ee 48f4 0102  000000000000f83f  0000 0080 ffff  0201")
FMT8_A_ROWS = [H("0x1.3d716ep+19"),      # X = 0x03e00279 = 65 012 345 -> 650 123.45 -> 650 123.4375
               H("0x1.a2b56ep+22"),      # Y = 0x28e3b7b9 = 686 012 345 -> 6 860 123.45 -> 6 860 123.5
               H("-0x1.47ae14p+24"),     # Z = 0x80000000 = INT32_MIN -> -21 474 836.48 -> -21 474 836
               0.0, 32768.0, 65535.0,    # R = 0x0000, G = 0x8000, B = 0xffff
               258.0,                    # NIR = 0x0102
               65535.0,                  # intensity = 0xffff: unsigned
               10.0, 5.0]                # byte 14 = 0x5a: return number = 0xa (bits 0-3), number of returns = 0x5 (bits 4-7)
FMT8_A_CLASS = 5                         # byte 16; byte 15 = 0xff is the flag byte
FMT8_B = bytes.fromhex("ffffffff ffffff7f 39300000  0080 a5 00 ff 00 0700 ffff  00000000000000c0  ffff 0100 ff7f  0000")
FMT8_B_ROWS = [H("-0x1.47ae14p-7"),      # X = -1 -> -0.01
               H("0x1.47ae14p+24"),      # Y = INT32_MAX -> 21 474 836.47 -> 21 474 836
               H("0x1.edccccp+6"),       # Z = 0x3039 = 12 345 -> 123.45
               65535.0, 1.0, 32767.0, 0.0, 32768.0,
               5.0, 10.0]                # byte 14 = 0xa5
FMT8_B_CLASS = 255
# format 1, 28 bytes: X Y Z | intensity | byte 14 | class | scan angle rank | user | source id | GPS time
FMT1_A = bytes.fromhex("7902e003 b9b7e328 37750000  0100 5a 02 fb ee 0900  000000000000f83f")
FMT1_A_ROWS = [H("0x1.3d716ep+19"), H("0x1.a2b56ep+22"),
               H("0x1.2c11ecp+8"),       # Z = 0x7537 = 30 007 -> 300.07
               0.0, 0.0, 0.0, 0.0,       # no colour in format 1
               1.0,
               2.0, 3.0]                 # byte 14 = 0x5a = 0b01 011 010: return number = 0b010 (bits 0-2), number of returns = 0b011 (bits 3-5)
FMT1_A_CLASS = 2                         # byte 15
FMT1_B = bytes.fromhex("00000080 9cffffff ffffff7f  ffff ff a5 7f 00 ffff  0000000000000000")
FMT1_B_ROWS = [H("-0x1.47ae14p+24"), -1.0, H("0x1.47ae14p+24"),    # INT32_MIN, -100, INT32_MAX
               0.0, 0.0, 0.0, 0.0, 65535.0,
               7.0, 7.0]                 # byte 14 = 0xff: bits 6-7 (scan direction, edge of flight line) are not returns
FMT1_B_CLASS = 0xA5                      # the byte as it stands, flag bits included


def test_hand_written_records_pin_the_readers_bit_positions():
    for fmt, recs, rows, cls in ((8, FMT8_A + FMT8_B, [FMT8_A_ROWS, FMT8_B_ROWS], [FMT8_A_CLASS, FMT8_B_CLASS]),
                                 (1, FMT1_A + FMT1_B, [FMT1_A_ROWS, FMT1_B_ROWS], [FMT1_A_CLASS, FMT1_B_CLASS])):
        L = {8: 38, 1: 28}[fmt]
        assert len(recs) == 2 * L
        cloud, c = R.decode_ref(recs, fmt, L, 2)
        want = np.array(rows, dtype=np.float64).T
        assert (want == want.astype(np.float32)).all(), "the expected values are fp32 numbers"
        assert cloud.dtype == np.float32 and cloud.tobytes() == want.astype(np.float32).tobytes(), fmt
        assert c.tolist() == cls
        # the writer packs the same bytes from the field values
        if fmt == 8:
            f = dict(X=[65012345, -1], Y=[686012345, 2 ** 31 - 1], Z=[-2 ** 31, 12345], intensity=[65535, 32768], returns=[0x5A, 0xA5],
                     flags=[0xFF, 0], classification=[5, 255], user_data=[0xEE, 0], scan_angle=[-3000, 7], point_source_id=[513, 65535],
                     gps_time=[1.5, -2.0], red=[0, 65535], green=[32768, 1], blue=[65535, 32767], nir=[258, 0])
        else:
            f = dict(X=[65012345, -2 ** 31], Y=[686012345, -100], Z=[30007, 2 ** 31 - 1], intensity=[1, 65535], returns=[0x5A, 0xFF],
                     classification=[2, 0xA5], scan_angle_rank=[-5, 127], user_data=[0xEE, 0], point_source_id=[9, 65535], gps_time=[1.5, 0.0])
        assert R.pack_records(f, fmt) == recs
    # the header mode on the same record: (X * 0.001 + 585 000) - 650 000 in fp64 = 12.345 (to an fp64 rounding), where fp32 of the
    # unshifted 650 012.345 has a step of 1/16
    cloud, _ = R.decode_ref(FMT8_A, 8, 38, 1, "header", origin=(650000.0, 0.0, 0.0), scale=(0.001, 0.01, 0.01), offset=(585000.0, 0.0, 0.0))
    assert cloud[0, 0] == np.float32((65012345 * 0.001 + 585000.0) - 650000.0) and abs(float(cloud[0, 0]) - 12.345) < 1e-5
    cloud, _ = R.decode_ref(FMT8_A, 8, 38, 1, "reference", origin=(65000000, 0, 0))
    assert cloud[0, 0] == np.float32(123.45)


# ---- las.read_header
def _fields(T=5, seed=3):
    return C.make_fields(T, seed)


@pytest.mark.parametrize("version,fmt", [((1, 2), 3), ((1, 4), 8), ((1, 4), 1), ((1, 2), 0)])
def test_read_header_round_trip(version, fmt, tmp_path):
    from stratanet2_vegetation_coverage_maps_amd import las
    L = R.LAYOUTS[fmt][1] + 3
    blob = R.write_las(_fields(7), fmt, L, version, scale=C.SCALE, offset=C.OFFSET, pad_after_header=54)
    p = tmp_path / "a.las"
    p.write_bytes(blob)
    for src in (blob, str(p)):
        h = las.read_header(src)
        assert (h.version, h.point_format, h.record_length, h.n_points) == (version, fmt, L, 7)
        assert h.header_size == R.HEADER_SIZE[version[1]] and h.offset_to_points == h.header_size + 54
        assert h.scale == C.SCALE and h.offset == C.OFFSET and h.n_bytes == 7 * L
        f = _fields(7)
        for a, k in enumerate("XYZ"):
            v = f[k].astype(np.float64) * C.SCALE[a] + C.OFFSET[a]
            assert h.mins[a] == v.min() and h.maxs[a] == v.max()
        assert R.parse(blob)[:4] == (fmt, L, 7, h.offset_to_points)


def test_read_header_takes_the_64_bit_count_when_the_legacy_count_is_zero():
    from stratanet2_vegetation_coverage_maps_amd import las
    blob = R.write_las(_fields(9), 6, None, (1, 4), legacy_count=0)
    assert las.read_header(blob).n_points == 9
    # a legacy count that is there wins; version 1.2 has no second count: zero points
    assert las.read_header(R.write_las(_fields(9), 1, None, (1, 4))).n_points == 9
    blob12 = R.write_las(_fields(9), 1, None, (1, 2), legacy_count=0)
    assert las.read_header(blob12).n_points == 0


def test_read_header_refusals():
    from stratanet2_vegetation_coverage_maps_amd import las
    f = _fields(4)
    good = R.write_las(f, 3)
    assert las.read_header(good).n_points == 4
    with pytest.raises(ValueError, match="signature"):
        las.read_header(R.write_las(f, 3, signature=b"LASX"))
    with pytest.raises(ValueError, match="signature"):
        las.read_header(b"LASF" + bytes(100))                       # cut short
    for laz in (0x80 | 3, 0x40 | 3, 0xC0 | 1):
        with pytest.raises(ValueError, match="LAZ"):
            las.read_header(R.write_las(f, 3, format_byte=laz))
    with pytest.raises(ValueError, match="format 11"):
        las.read_header(R.write_las(f, 3, format_byte=11))
    with pytest.raises(ValueError, match="record length"):
        las.read_header(R.write_las(f, 0, 34, format_byte=7))       # 34 bytes are not a format-7 record
    with pytest.raises(ValueError, match="shorter"):
        las.read_header(good[:-1])
    with pytest.raises(ValueError, match="shorter"):
        las.read_header(R.write_las(f, 3, legacy_count=5))


# ---- planted wrong restatements: each must differ from decode_ref on the cases, or the cases would not notice the bug
def _case_bytes(fmt, T=4096, seed=7, L=None):
    f = C.make_fields(T, seed)
    return f, R.pack_records(f, fmt, L), (R.LAYOUTS[fmt][1] if L is None else L)


def test_planted_fp32_division_differs():
    f, recs, L = _case_bytes(8)
    cloud, _ = R.decode_ref(recs, 8, L, 4096)
    wrong = f["X"].astype(np.float32) / np.float32(100)
    assert (wrong != cloud[0]).mean() > 0.05
    lam = np.random.default_rng(0).integers(600000000, 720000000, size=100000)
    assert ((lam.astype(np.float32) / np.float32(100)) != (lam / 100).astype(np.float32)).mean() > 0.1


def test_planted_three_bit_returns_on_format_6_differ():
    f, recs, L = _case_bytes(6)
    cloud, _ = R.decode_ref(recs, 6, L, 4096)
    b = f["returns"].astype(np.int64)
    assert ((b & 7) != cloud[8]).any() and (((b >> 3) & 7) != cloud[9]).any()
    # and the classification read at byte 15 of a format-6 record is its flag byte
    assert (f["flags"] != R.decode_ref(recs, 6, L, 4096)[1]).any()


def test_planted_signed_intensity_differs():
    f, recs, L = _case_bytes(0)
    cloud, _ = R.decode_ref(recs, 0, L, 4096)
    assert (f["intensity"].view(np.int16).astype(np.float32) != cloud[7]).any()
    assert cloud[7].min() == 0.0 and cloud[7].max() == 65535.0


def test_planted_scale_and_offset_in_reference_mode_differ():
    f, recs, L = _case_bytes(8)
    ref, _ = R.decode_ref(recs, 8, L, 4096, "reference")
    hdr, _ = R.decode_ref(recs, 8, L, 4096, "header", scale=C.SCALE, offset=C.OFFSET)
    for a in range(3):
        assert (ref[a] != hdr[a]).mean() > 0.9
    # (X * 0.01 in fp64 for X / 100 is NOT planted: the two agree after the fp32 rounding on every sampled value)


def test_planted_format_3_colour_offset_on_format_7_differs():
    f, recs, L = _case_bytes(7)
    cloud, _ = R.decode_ref(recs, 7, L, 4096)
    raw = np.frombuffer(recs, dtype=np.uint8).reshape(4096, L)
    red_at_28 = raw[:, 28].astype(np.float32) + 256 * raw[:, 29].astype(np.float32)
    red_at_30 = raw[:, 30].astype(np.float32) + 256 * raw[:, 31].astype(np.float32)
    assert (red_at_30 == cloud[3]).all() and (red_at_28 != cloud[3]).mean() > 0.9


def test_cases_hold_the_edges_the_issue_names():
    f = C.make_fields(257)
    for k in "XYZ":
        assert {C.I32_MIN, C.I32_MAX, -1, 686012345} <= set(f[k].tolist())
    for k in ("intensity", "red", "green", "blue", "nir"):
        assert {0, 32768, 65535} <= set(f[k].tolist())
    assert {0x00, 0xFF, 0x5A, 0xA5} <= set(f["returns"].tolist())
    assert {c[3] for c in C.CASES} >= {1, 255, 256, 257, 2 ** 20 + 3}
    assert {(c[1], c[2]) for c in C.CASES} >= {(f_, None) for f_ in (0, 1, 2, 3, 6, 7, 8, 10)} | {(8, 39), (8, 41), (6, 33)}


# ---- the C ABI
def test_las_is_part_of_the_build_and_the_version_stays():
    from stratanet2_vegetation_coverage_maps_amd import _build, _lib
    assert "las.hip" in _build.SOURCES and "las_rules.h" in _build.HEADERS
    assert _lib.SN2_VERSION == 102 and _lib.load().sn2_version() == 102
    assert {"sn2_las_decode", "sn2_las_record_min_length"} <= set(_lib.SIGNATURES)


def test_record_min_length_is_the_table():
    from stratanet2_vegetation_coverage_maps_amd import _lib
    from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
    lib = _lib.load()
    table = {0: 20, 1: 28, 2: 26, 3: 34, 4: 57, 5: 63, 6: 30, 7: 36, 8: 38, 9: 59, 10: 67}
    for fmt, n in table.items():
        assert lib.sn2_las_record_min_length(fmt) == n == ops.las_record_min_length(fmt) == R.LAYOUTS[fmt][1], fmt
    for bad in (-1, 11, 0x80, 0x43, 255):
        assert lib.sn2_las_record_min_length(bad) == -1
        with pytest.raises(ValueError):
            ops.las_record_min_length(bad)


def test_decode_argument_checks_return_before_any_device_work():
    from stratanet2_vegetation_coverage_maps_amd import _lib
    lib = _lib.load()
    fake = 0x10000                                            # 16-byte aligned, never dereferenced: every call fails a check first
    xf = (ctypes.c_double * 9)(*([0.01] * 3 + [0.0] * 6))
    r0 = (ctypes.c_longlong * 3)(0, 0, 0)

    def call(records=fake, n_bytes=38 * 100, fmt=8, L=38, T=100, mode=0, xform=None, raw0=None, out=fake, row_stride=100, col0=0,
             cls=None):
        return lib.sn2_las_decode(records, n_bytes, fmt, L, T, mode, xform, raw0, out, row_stride, col0, cls, None)
    EINVAL, ELIMIT = -1, -2
    assert call(records=None) == EINVAL and call(out=None) == EINVAL
    assert call(T=0) == EINVAL and call(T=-5) == EINVAL
    assert call(fmt=0x80 | 8) == EINVAL and call(fmt=0x40 | 8) == EINVAL            # LAZ
    assert call(fmt=11) == EINVAL and call(fmt=-1) == EINVAL
    for fmt, least in R.LAYOUTS.items():
        assert call(fmt=fmt, L=least[1] - 1, n_bytes=10 ** 6) == EINVAL, fmt          # below the format's least length
    assert call(L=65536, n_bytes=10 ** 8) == EINVAL
    assert call(n_bytes=38 * 100 - 1) == EINVAL                                       # n_bytes < T L
    assert call(T=2 ** 31, n_bytes=38 * 2 ** 31, row_stride=2 ** 31) == ELIMIT
    assert call(records=fake + 4) == EINVAL and call(records=fake + 8) == EINVAL      # not 16-byte aligned
    assert call(col0=1) == EINVAL and call(col0=-1) == EINVAL and call(row_stride=99) == EINVAL   # col0 + T > row_stride
    assert call(mode=2) == EINVAL and call(mode=-1) == EINVAL
    assert call(mode=1, xform=None) == EINVAL                                         # the header mode needs its transform
    big = (ctypes.c_longlong * 3)(0, 2 ** 52 + 1, 0)
    assert call(raw0=big) == EINVAL
    assert lib.sn2_debug_las_form(2) == EINVAL and lib.sn2_debug_las_form(0) == 0
    del xf, r0


def test_from_arena_refuses_what_is_not_an_arena():
    import torch
    from stratanet2_vegetation_coverage_maps_amd.parcel import ParcelClouds
    with pytest.raises(ValueError):
        ParcelClouds.from_arena(torch.zeros(10, 5), [2, 3])                           # not on the device
    with pytest.raises(ValueError):
        ParcelClouds.from_arena(torch.zeros(10, 5), [5, 0])
    with pytest.raises(ValueError):
        ParcelClouds.from_arena(torch.zeros(10, 5), [])
