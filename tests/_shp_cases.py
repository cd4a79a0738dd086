"""One shapefile typed out by hand, shared by tests/test_shp_host.py and tests/test_gpu_shapefile.py: `struct.pack_into` only, every
offset spelled out, after the ESRI Shapefile Technical Description (July 1998) and dBase III.  Nothing of the package under test
builds these bytes.

Records: 0 a square, 1 a square with a hole (two parts), 2 a two-part polygon, 3 a PolygonZ with an M block, 4 a null shape, 5 a
closed ring with a repeated vertex.  The .dbf has one field of each type C / N / F / L / D, a blank numeric (record 1), an
asterisk-filled numeric (record 2), a record whose deletion flag is '*' (record 3) and an odd record length (33)."""
import struct

import numpy as np

# the rings as literals: what the reader must give back, part by part
RINGS = [
    [[(0.0, 0.0), (0.0, 10.0), (10.0, 10.0), (10.0, 0.0), (0.0, 0.0)]],
    [[(20.0, 0.0), (20.0, 12.0), (32.0, 12.0), (32.0, 0.0), (20.0, 0.0)],
     [(24.0, 4.0), (28.0, 4.0), (28.0, 8.0), (24.0, 8.0), (24.0, 4.0)]],
    [[(40.0, 0.0), (40.0, 5.0), (45.0, 5.0), (40.0, 0.0)],
     [(50.5, 0.25), (50.5, 5.25), (55.5, 5.25), (55.5, 0.25), (50.5, 0.25)]],
    [[(700000.125, 6600000.5), (700000.125, 6600010.5), (700010.375, 6600010.5), (700000.125, 6600000.5)]],
    None,
    [[(60.0, 0.0), (60.0, 10.0), (60.0, 10.0), (70.0, 10.0), (70.0, 0.0), (60.0, 0.0)]],
]
TYPES = [5, 5, 5, 15, 0, 5]
BOXES = [(0.0, 0.0, 10.0, 10.0), (20.0, 0.0, 32.0, 12.0), (40.0, 0.0, 55.5, 5.25), (700000.125, 6600000.5, 700010.375, 6600010.5), None,
         (60.0, 0.0, 70.0, 10.0)]
# the box of record 2 AS THE FILE STATES IT is wrong on purpose: the reader recomputes
STATED_BOX_2 = (-1.0, -1.0, 1.0, 1.0)

FIELDS = [("ID", "C", 6, 0), ("NPLOT", "N", 5, 0), ("SCORE", "F", 12, 4), ("OK", "L", 1, 0), ("DAY", "D", 8, 0)]
RECORD_LEN = 1 + 6 + 5 + 12 + 1 + 8                  # 33: odd
HEADER_LEN = 32 + 32 * 5 + 1                         # 193
# the records as the file holds them: flag, ID, NPLOT, SCORE, OK, DAY
RECORD_TEXT = [
    b" " + b"P1    " + b"   12" + b"      0.5000" + b"T" + b"20240611",
    b" " + b"P2    " + b"     " + b"     -1.2500" + b"F" + b"20240612",
    b" " + b"P\xe9    " + b"*****" + b"************" + b"?" + b"        ",
    b"*" + b"P1    " + b"    7" + b"  1.0000e+02" + b"T" + b"20240613",
    b" " + b"NULL  " + b"    0" + b"            " + b" " + b"20240614",
    b" " + b"P6" + b"\0\0\0\0" + b"  -45" + b"      3.0000" + b"T" + b"20240615",
]
COLUMNS = {
    "ID": ["P1", "P2", "P\xe9", "P1", "NULL", "P6"],
    "NPLOT": [12, None, None, 7, 0, -45],
    "SCORE": [0.5, -1.25, None, 100.0, None, 3.0],
    "OK": ["T", "F", "?", "T", " ", "T"],
    "DAY": ["20240611", "20240612", "        ", "20240613", "20240614", "20240615"],
}
DATE = (124, 6, 11)                                  # YY MM DD: 2024-06-11


def _polygon_content(shape_type, box, parts, points, z_and_m=False):
    """The content of one polygon record: little-endian throughout."""
    n_parts, n_points = len(parts), len(points)
    size = 44 + 4 * n_parts + 16 * n_points
    if z_and_m:
        size += (16 + 8 * n_points) * 2              # Zmin, Zmax, Z[n]; Mmin, Mmax, M[n]
    b = bytearray(size)
    struct.pack_into("<i", b, 0, shape_type)         # byte 0: shape type
    struct.pack_into("<4d", b, 4, *box)              # byte 4: box x_min, y_min, x_max, y_max
    struct.pack_into("<i", b, 36, n_parts)           # byte 36: NumParts
    struct.pack_into("<i", b, 40, n_points)          # byte 40: NumPoints
    for i, p in enumerate(parts):
        struct.pack_into("<i", b, 44 + 4 * i, p)     # byte 44: Parts[]
    x = 44 + 4 * n_parts                             # then Points[]
    for i, (px, py) in enumerate(points):
        struct.pack_into("<2d", b, x + 16 * i, px, py)
    if z_and_m:
        y = x + 16 * n_points
        struct.pack_into("<2d", b, y, 100.0, 103.0)                            # Z range
        for i in range(n_points):
            struct.pack_into("<d", b, y + 16 + 8 * i, 100.0 + i)               # Z[]
        m = y + 16 + 8 * n_points
        struct.pack_into("<2d", b, m, -1e39, -1e39)                            # M range: "no data"
        for i in range(n_points):
            struct.pack_into("<d", b, m + 16 + 8 * i, -1e39)                   # M[]
    return bytes(b)


def contents():
    out = []
    for k, rings in enumerate(RINGS):
        if rings is None:
            out.append(struct.pack("<i", 0))         # a null shape: the type alone
            continue
        parts, points = [], []
        for r in rings:
            parts.append(len(points))
            points += r
        box = STATED_BOX_2 if k == 2 else BOXES[k]
        out.append(_polygon_content(TYPES[k], box, parts, points, z_and_m=TYPES[k] == 15))
    return out


def _main_header(total_bytes, shape_type=5):
    h = bytearray(100)
    struct.pack_into(">i", h, 0, 9994)               # byte 0: file code, big-endian
    struct.pack_into(">i", h, 24, total_bytes // 2)  # byte 24: length in 16-bit words, big-endian
    struct.pack_into("<i", h, 28, 1000)              # byte 28: version, little-endian
    struct.pack_into("<i", h, 32, shape_type)        # byte 32: shape type, little-endian
    struct.pack_into("<4d", h, 36, 0.0, 0.0, 700010.375, 6600010.5)            # byte 36: the file's box
    return h


def shp_bytes(cs=None) -> bytes:
    cs = contents() if cs is None else cs
    body = bytearray()
    for k, c in enumerate(cs):
        body += struct.pack(">ii", k + 1, len(c) // 2)                         # record number (1-based), content length in words
        body += c
    return bytes(_main_header(100 + len(body)) + body)


def shx_bytes(cs=None) -> bytes:
    cs = contents() if cs is None else cs
    body, at = bytearray(), 100
    for c in cs:
        body += struct.pack(">ii", at // 2, len(c) // 2)                       # offset and content length, in words
        at += 8 + len(c)
    return bytes(_main_header(100 + len(body)) + body)


def dbf_header(fields=FIELDS, n_records=6, header_len=None, record_len=None) -> bytes:
    n = len(fields)
    h = bytearray(32 + 32 * n + 1)
    h[0] = 0x03                                      # byte 0: dBase III without memo
    h[1], h[2], h[3] = DATE                          # bytes 1..3: YY MM DD
    struct.pack_into("<I", h, 4, n_records)          # byte 4: record count
    struct.pack_into("<H", h, 8, len(h) if header_len is None else header_len)       # byte 8: header length
    struct.pack_into("<H", h, 10, 1 + sum(f[2] for f in fields) if record_len is None else record_len)   # byte 10: record length
    for i, (name, typ, size, dec) in enumerate(fields):
        d = 32 + 32 * i
        raw = name.encode("ascii")
        h[d:d + len(raw)] = raw                      # descriptor byte 0: the name, NUL-padded to 11
        h[d + 11] = ord(typ)                         # byte 11: type
        h[d + 16] = size                             # byte 16: length
        h[d + 17] = dec                              # byte 17: decimals
    h[32 + 32 * n] = 0x0D
    return bytes(h)


def dbf_bytes(trailer=b"\x1a") -> bytes:
    assert all(len(r) == RECORD_LEN for r in RECORD_TEXT)
    return dbf_header() + b"".join(RECORD_TEXT) + trailer


PRJ = b'PROJCS["RGF93_Lambert_93"]'
CPG = b"ISO-8859-1"


def write_fixture(directory, name="parcels", **files):
    """Writes the triple (and .prj, .cpg) into `directory`; a keyword shp= / dbf= / shx= replaces that file's bytes.  -> the base path."""
    base = str(directory / name)
    data = {"shp": shp_bytes(), "shx": shx_bytes(), "dbf": dbf_bytes(), "prj": PRJ, "cpg": CPG}
    data.update(files)
    for ext, b in data.items():
        if b is not None:
            with open(f"{base}.{ext}", "wb") as f:
                f.write(b)
    return base


# ---- the planted values of the formatting rule, with CPython's text at decimal = 10 (typed, not computed)
PLANTED = [
    (1.0 / 2048, "0.0004882812"),                    # an exact tie, down to even
    (3.0 / 2048, "0.0014648438"),                    # an exact tie, up to even
    (2.0 ** -34, "0.0000000001"),
    (2.0 ** -35, "0.0000000000"),
    (-2.0 ** -35, "-0.0000000000"),
    (-0.0, "-0.0000000000"),
    (1.0 - 2.0 ** -53, "1.0000000000"),
    (0.99999999995, "0.9999999999"),
    (2.0 ** 53 - 1, "9007199254740991.0000000000"),
    (4503599627370495.5, "4503599627370495.5000000000"),
    (5e-324, "0.0000000000"),
    (float("nan"), "nan"),
    (float("inf"), "inf"),
]


def random_doubles(n, seed):
    """n doubles drawn as random bit patterns with |v| < 2^53 (biased exponent below 1023 + 53), either sign"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2 ** 63, size=2 * n, dtype=np.uint64) | (rng.integers(0, 2, size=2 * n, dtype=np.uint64) << np.uint64(63))
    bits = bits[((bits >> np.uint64(52)) & np.uint64(0x7FF)) < 1023 + 53]
    # the draw above keeps about half; fill up with small exponents so that the count is exact
    extra = (rng.integers(0, 2 ** 52, size=n, dtype=np.uint64) | (rng.integers(960, 1076, size=n, dtype=np.uint64) << np.uint64(52)))
    return np.concatenate([bits, extra])[:n].view(np.float64).copy()
