"""A LAS writer and a numpy reader for the tests of the LAS decoder.  They share no code with the kernel (csrc/las.hip,
csrc/las_rules.h) nor with las.read_header: the record layouts are written out here a second time, as packed numpy structured
dtypes with explicit offsets, from the ASPRS LAS 1.4 specification (tables 7-16).  The rule `decode_ref` applies is the one of
include/strata_hip.h, "LAS point records", in numpy fp64, then fp32."""
import struct

import numpy as np

_BASE_LEGACY = [("X", "<i4", 0), ("Y", "<i4", 4), ("Z", "<i4", 8), ("intensity", "<u2", 12), ("returns", "u1", 14),
                ("classification", "u1", 15), ("scan_angle_rank", "i1", 16), ("user_data", "u1", 17), ("point_source_id", "<u2", 18)]
_BASE_EXTENDED = [("X", "<i4", 0), ("Y", "<i4", 4), ("Z", "<i4", 8), ("intensity", "<u2", 12), ("returns", "u1", 14),
                  ("flags", "u1", 15), ("classification", "u1", 16), ("user_data", "u1", 17), ("scan_angle", "<i2", 18),
                  ("point_source_id", "<u2", 20), ("gps_time", "<f8", 22)]


def _rgb(at):
    return [("red", "<u2", at), ("green", "<u2", at + 2), ("blue", "<u2", at + 4)]


def _wave(at):
    return [("wave_descriptor", "u1", at), ("wave_offset", "<u8", at + 1), ("wave_size", "<u4", at + 9), ("wave_location", "<f4", at + 13),
            ("wave_dx", "<f4", at + 17), ("wave_dy", "<f4", at + 21), ("wave_dz", "<f4", at + 25)]


# format -> (fields, least record length)
LAYOUTS = {
    0: (_BASE_LEGACY, 20),
    1: (_BASE_LEGACY + [("gps_time", "<f8", 20)], 28),
    2: (_BASE_LEGACY + _rgb(20), 26),
    3: (_BASE_LEGACY + [("gps_time", "<f8", 20)] + _rgb(28), 34),
    4: (_BASE_LEGACY + [("gps_time", "<f8", 20)] + _wave(28), 57),
    5: (_BASE_LEGACY + [("gps_time", "<f8", 20)] + _rgb(28) + _wave(34), 63),
    6: (_BASE_EXTENDED, 30),
    7: (_BASE_EXTENDED + _rgb(30), 36),
    8: (_BASE_EXTENDED + _rgb(30) + [("nir", "<u2", 36)], 38),
    9: (_BASE_EXTENDED + _wave(30), 59),
    10: (_BASE_EXTENDED + _rgb(30) + [("nir", "<u2", 36)] + _wave(38), 67),
}
HEADER_SIZE = {0: 227, 1: 227, 2: 227, 3: 235, 4: 375}      # by minor version


def record_dtype(fmt, L=None):
    fields, least = LAYOUTS[fmt]
    L = least if L is None else L
    assert L >= least
    return np.dtype({"names": [f[0] for f in fields], "formats": [f[1] for f in fields], "offsets": [f[2] for f in fields],
                     "itemsize": L})


def pack_records(fields, fmt, L=None, fill=0xA7):
    """fields: name -> (T) array; names the format lacks are ignored, absent ones are zero.  The bytes no field covers (extra
    bytes) are `fill`.  -> T * L bytes"""
    dt = record_dtype(fmt, L)
    T = len(fields["X"])
    rec = np.frombuffer(bytes([fill]) * (T * dt.itemsize), dtype=dt).copy()
    for name in dt.names:
        rec[name] = fields[name] if name in fields else 0
    return rec.tobytes()


def write_las(fields, fmt, L=None, version=(1, 2), scale=(0.01, 0.01, 0.01), offset=(0.0, 0.0, 0.0), legacy_count=None,
              pad_after_header=0, format_byte=None, signature=b"LASF"):
    """-> the bytes of a LAS file.  legacy_count: what goes into the 32-bit count (None = T); version 1.4 also gets the 64-bit
    count.  pad_after_header: bytes between header and records (stands for the VLRs).  format_byte: overrides the header's byte."""
    L = LAYOUTS[fmt][1] if L is None else L
    T = len(fields["X"])
    hs = HEADER_SIZE[version[1]]
    h = bytearray(hs)
    h[0:4] = signature
    h[24], h[25] = version
    h[26:26 + 8] = b"TESTSYS\0"
    struct.pack_into("<HHHI I", h, 90, 1, 2024, hs, hs + pad_after_header, 0)
    struct.pack_into("<BHI", h, 104, fmt if format_byte is None else format_byte, L, T if legacy_count is None else legacy_count)
    X, Y, Z = (np.asarray(fields[k], dtype=np.float64) for k in "XYZ")
    m = [((v * s + o).max() if T else 0.0, (v * s + o).min() if T else 0.0) for v, s, o in zip((X, Y, Z), scale, offset)]
    struct.pack_into("<12d", h, 131, *scale, *offset, m[0][0], m[0][1], m[1][0], m[1][1], m[2][0], m[2][1])
    if version[1] >= 4:
        struct.pack_into("<Q", h, 247, T)
    return bytes(h) + bytes(pad_after_header) + pack_records(fields, fmt, L)


def parse(file_bytes):
    """-> (fmt, L, T, offset_to_points, scale, offset) of a file of `write_las` (the tests' own header reader)"""
    off = struct.unpack_from("<I", file_bytes, 96)[0]
    fmt, L, T = struct.unpack_from("<BHI", file_bytes, 104)
    if T == 0 and file_bytes[25] >= 4:
        T = struct.unpack_from("<Q", file_bytes, 247)[0]
    d = struct.unpack_from("<6d", file_bytes, 131)
    return fmt, L, T, off, d[:3], d[3:]


def decode_ref(records, fmt, L, T, coords="reference", origin=None, scale=None, offset=None):
    """records: bytes that start at the first record -> (cloud (10,T) fp32, classification (T) uint8): the rule in numpy."""
    rec = np.frombuffer(records, dtype=record_dtype(fmt, L), count=T)
    rows = []
    for a, k in enumerate("XYZ"):
        if coords == "reference":
            o = 0 if origin is None else int(origin[a])
            rows.append((rec[k].astype(np.int64) - o) / 100)                     # int64 / int: a correctly rounded fp64 quotient
        else:
            o = 0.0 if origin is None else float(origin[a])
            rows.append(((rec[k].astype(np.float64) * np.float64(scale[a])) + np.float64(offset[a])) - np.float64(o))
    zero = np.zeros(T)
    for k in ("red", "green", "blue", "nir"):
        rows.append(rec[k].astype(np.float64) if k in rec.dtype.names else zero)
    rows.append(rec["intensity"].astype(np.float64))
    b = rec["returns"].astype(np.int64)
    if fmt >= 6:
        rows += [b & 15, b >> 4]
    else:
        rows += [b & 7, (b >> 3) & 7]
    return np.asarray(rows, dtype=np.float32), rec["classification"].copy()


def decode_ref_file(file_bytes, coords="reference", origin=None):
    fmt, L, T, off, scale, offset = parse(file_bytes)
    return decode_ref(file_bytes[off:], fmt, L, T, coords, origin, scale, offset)
