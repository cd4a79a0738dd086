"""A numpy restatement of the GeoTIFF band packer (include/strata_hip.h, "GeoTIFF image data") and of the file geotiff.py lays out:
the image data block in both layouts, both predictors, the statistics, the place table and the file assembly -- written from the
header's text, not from the kernel's code.  Also the five WRONG restatements tests/test_geotiff_host.py shows to differ."""
import struct
import zlib

import numpy as np

BAND, PIXEL = 0, 1
STAGE_BYTES = 16384          # a workgroup's whole rows, and the piece of a longer row


def rows_u32(bands: np.ndarray, layout: int) -> np.ndarray:
    """(C,H,W) fp32 -> (rows, wc) uint32: row q of the block as the floats' bit patterns"""
    C, H, W = bands.shape
    u = np.ascontiguousarray(bands, dtype=np.float32).view(np.uint32)
    if layout == PIXEL:
        return np.ascontiguousarray(u.transpose(1, 2, 0)).reshape(H, W * C)
    return u.reshape(C * H, W)


def own_bytes(rows: np.ndarray) -> np.ndarray:
    """(n, wc) uint32 -> (n, 4 wc) uint8: little-endian, the fp32's own bytes (predictor 1)"""
    return np.ascontiguousarray(rows.astype("<u4")).view(np.uint8).reshape(rows.shape[0], -1)


def planes(rows: np.ndarray) -> np.ndarray:
    """t of the rule: plane p holds byte 3 - p of every float of the row"""
    n, wc = rows.shape
    b = own_bytes(rows).reshape(n, wc, 4)
    return np.ascontiguousarray(b[:, :, ::-1].transpose(0, 2, 1)).reshape(n, 4 * wc)


def predictor3(rows: np.ndarray, stride: int) -> np.ndarray:
    t = planes(rows)
    out = t.copy()
    out[:, stride:] = t[:, stride:] - t[:, :-stride]              # uint8 arithmetic: mod 256
    return out


def block(bands: np.ndarray, layout: int, predictor: int) -> np.ndarray:
    rows = rows_u32(bands, layout)
    stride = bands.shape[0] if layout == PIXEL else 1
    return (own_bytes(rows) if predictor == 1 else predictor3(rows, stride)).reshape(-1)


# ---- the five wrong restatements (predictor 3) -----------------------------------------------------------------------------
def wrong_lsb_first(bands, layout):
    rows = rows_u32(bands, layout)
    n, wc = rows.shape
    t = np.ascontiguousarray(own_bytes(rows).reshape(n, wc, 4).transpose(0, 2, 1)).reshape(n, 4 * wc)
    s = bands.shape[0] if layout == PIXEL else 1
    out = t.copy()
    out[:, s:] = t[:, s:] - t[:, :-s]
    return out.reshape(-1)


def wrong_difference_before_shuffle(bands, layout):
    rows = rows_u32(bands, layout)
    n, wc = rows.shape
    b = own_bytes(rows)
    s = bands.shape[0] if layout == PIXEL else 1
    d = b.copy()
    d[:, s:] = b[:, s:] - b[:, :-s]
    return np.ascontiguousarray(d.reshape(n, wc, 4)[:, :, ::-1].transpose(0, 2, 1)).reshape(-1)


def wrong_stride_one(bands, layout):
    return predictor3(rows_u32(bands, layout), 1).reshape(-1)


def wrong_across_rows(bands, layout):
    t = planes(rows_u32(bands, layout)).reshape(1, -1)
    s = bands.shape[0] if layout == PIXEL else 1
    out = t.copy()
    out[:, s:] = t[:, s:] - t[:, :-s]
    return out.reshape(-1)


def wrong_float_difference(bands, layout):
    rows = rows_u32(bands, layout)
    s = bands.shape[0] if layout == PIXEL else 1
    f = rows.view(np.float32)
    d = f.copy()
    with np.errstate(all="ignore"):
        d[:, s:] = f[:, s:] - f[:, :-s]
    return planes(d.view(np.uint32)).reshape(-1)


WRONG = {"planes LSB-first": wrong_lsb_first, "difference before the shuffle": wrong_difference_before_shuffle,
         "stride 1 in the PIXEL layout": wrong_stride_one, "differencing across the row boundary": wrong_across_rows,
         "a float difference": wrong_float_difference}


# ---- the statistics -------------------------------------------------------------------------------------------------------
def key(bits: np.ndarray) -> np.ndarray:
    bits = np.asarray(bits, dtype=np.uint32)
    return bits ^ np.where(bits >> 31, np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)


def key_bits(k: np.ndarray) -> np.ndarray:
    k = np.asarray(k, dtype=np.uint32)
    return k ^ np.where(k >> 31, np.uint32(0x80000000), np.uint32(0xFFFFFFFF)).astype(np.uint32)


def stats_words(bands: np.ndarray) -> np.ndarray:
    """(C,4) uint32: the sixteen bytes per band as the device holds them -- count (uint64, low word first), key of the minimum, of
    the maximum; an all-NaN band keeps 0, 0xFFFFFFFF, 0"""
    C = bands.shape[0]
    out = np.zeros((C, 4), dtype=np.uint32)
    for c in range(C):
        u = np.ascontiguousarray(bands[c], dtype=np.float32).view(np.uint32).reshape(-1)
        u = u[(u & 0x7FFFFFFF) <= 0x7F800000]
        out[c, 0], out[c, 1] = u.size & 0xFFFFFFFF, u.size >> 32
        out[c, 2] = key(u).min() if u.size else 0xFFFFFFFF
        out[c, 3] = key(u).max() if u.size else 0
    return out


# ---- the place table ------------------------------------------------------------------------------------------------------
def units(C, H, W, layout, force_direct=False):
    wc = W * C if layout == PIXEL else W
    rb = 4 * wc
    if rb <= STAGE_BYTES and not force_direct:
        R = min(STAGE_BYTES // rb, H)
        groups = -(-H // R)
        return groups if layout == PIXEL else groups * C
    return (H if layout == PIXEL else C * H) * -(-rb // STAGE_BYTES)


def place_table(shapes, C, layout, skip=None, force_direct=False) -> np.ndarray:
    K = len(shapes)
    t = np.zeros((K + 1, 4), dtype=np.int64)
    base = wg = 0
    for k, (H, W) in enumerate(shapes):
        no = bool(skip[k]) if skip is not None else False
        nbytes = 0 if no else 4 * C * H * W
        t[k] = [base, int(no), wg, nbytes]
        base += -(-nbytes // 16) * 16
        wg += 0 if no else units(C, H, W, layout, force_direct)
    t[K] = [base, 0, wg, base + 16 * K * C]
    return t


def expected_buffer(canvases, C, layout, predictor, skip=None, force_direct=False, poison=0xA5, guard=0) -> np.ndarray:
    """the staging buffer after the launch when it held `poison` before: guard bytes | blocks with untouched padding | statistics |
    guard bytes.  canvases: (C,H,W) arrays."""
    place = place_table([c.shape[1:] for c in canvases], C, layout, skip, force_direct)
    K = len(canvases)
    buf = np.full(guard + int(place[K, 3]) + guard, poison, dtype=np.uint8)
    for k, c in enumerate(canvases):
        words = np.tile(np.array([0, 0, 0xFFFFFFFF, 0], dtype=np.uint32), (C, 1))
        if not place[k, 1]:
            b = block(c, layout, predictor)
            buf[guard + place[k, 0]:guard + place[k, 0] + b.size] = b
            words = stats_words(c)
        at = guard + int(place[K, 0]) + 16 * C * k
        buf[at:at + 16 * C] = words.astype("<u4").view(np.uint8).reshape(-1)
    return buf


# ---- the file -------------------------------------------------------------------------------------------------------------
def metadata_text(names, stats=None) -> bytes:
    s = "<GDALMetadata>\n"
    for i, n in enumerate(names):
        s += '  <Item name="DESCRIPTION" sample="%d" role="description">%s</Item>\n' % (i, n)
        if stats is not None and stats[i]:
            for k in sorted(stats[i]):
                s += '  <Item name="%s" sample="%d">%s</Item>\n' % (k, i, stats[i][k])
    return (s + "</GDALMetadata>\n").encode("ascii") + b"\0"


def assemble(bands, x_min, y_max, pix, layout=BAND, predictor=1, deflate=False, level=6, names=None, epsg=2154, stats=None,
             rows_per_strip=None) -> bytes:
    """the file of (C,H,W) bands, laid out as the header of geotiff.py says: IFD at 8, long values in tag order on even offsets, strips"""
    C, H, W = bands.shape
    data = block(bands, layout, predictor)
    rb = 4 * W * (C if layout == PIXEL else 1)
    rps = min(max(1, 65536 // rb), H) if rows_per_strip is None else min(rows_per_strip, H)
    strips = []
    for p in range(1 if layout == PIXEL else C):
        for r in range(0, H, rps):
            raw = data[(p * H + r) * rb:(p * H + min(r + rps, H)) * rb].tobytes()
            strips.append(zlib.compress(raw, level) if deflate else raw)
    ns = len(strips)
    SHORT, LONG, ASCII, DOUBLE = 3, 4, 2, 12
    fmt = {SHORT: "H", LONG: "I", DOUBLE: "d"}
    entries = [(256, LONG, (W,)), (257, LONG, (H,)), (258, SHORT, (32,) * C), (259, SHORT, (8 if deflate else 1,)), (262, SHORT, (1,)),
               (273, LONG, "offsets"), (277, SHORT, (C,)), (278, LONG, (rps,)), (279, LONG, tuple(len(s) for s in strips)),
               (284, SHORT, (1 if layout == PIXEL or C == 1 else 2,))]
    if predictor == 3:
        entries.append((317, SHORT, (3,)))
    if C > 1:
        entries.append((338, SHORT, (0,) * (C - 1)))
    entries += [(339, SHORT, (3,) * C), (33550, DOUBLE, (pix, pix, 0.0)), (33922, DOUBLE, (0.0, 0.0, 0.0, x_min, y_max, 0.0)),
                (34735, SHORT, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, epsg)),
                (42112, ASCII, metadata_text(names or default_names(C), stats)), (42113, ASCII, b"nan\0")]
    cursor = 8 + 2 + 12 * len(entries) + 4
    where = []
    for tag, typ, v in entries:
        size = (ns * 4) if isinstance(v, str) else (len(v) if typ == ASCII else len(v) * struct.calcsize(fmt[typ]))
        if size > 4:
            cursor += cursor % 2
            where.append(cursor)
            cursor += size
        else:
            where.append(None)
    cursor += cursor % 2
    offsets, o = [], cursor
    for s in strips:
        offsets.append(o)
        o += len(s)
    head = bytearray(cursor)
    head[0:8] = b"II*\0" + struct.pack("<I", 8)
    head[8:10] = struct.pack("<H", len(entries))
    for i, ((tag, typ, v), at) in enumerate(zip(entries, where)):
        if isinstance(v, str):
            v = tuple(offsets)
        payload = v if typ == ASCII else struct.pack("<" + fmt[typ] * len(v), *v)
        e = 10 + 12 * i
        head[e:e + 8] = struct.pack("<HHI", tag, typ, len(v))
        if at is None:
            head[e + 8:e + 8 + len(payload)] = payload
        else:
            head[e + 8:e + 12] = struct.pack("<I", at)
            head[at:at + len(payload)] = payload
    return bytes(head) + b"".join(strips)


def default_names(C):
    six = ["VegetationBasse", "VegetationIntermediaire", "VegetationHaute", "VegetationIntermediaireDiscretisee", "Admissibilite",
           "PonderationPredictions"]
    if C == 6:
        return six
    if C == 5:
        return six[:4] + six[5:]
    return ["band_%d" % i for i in range(C)]


def single_band_file(strips, H, W, rps, deflate, predictor) -> bytes:
    """the strips of ONE band wrapped into a C = 1 header of the fewest tags: what libtiff is asked to open"""
    entries = [(256, 4, (W,)), (257, 4, (H,)), (258, 3, (32,)), (259, 3, (8 if deflate else 1,)), (262, 3, (1,)), (273, 4, "offsets"),
               (277, 3, (1,)), (278, 4, (rps,)), (279, 4, tuple(len(s) for s in strips)), (284, 3, (1,))]
    if predictor == 3:
        entries.append((317, 3, (3,)))
    entries.append((339, 3, (3,)))
    ns = len(strips)
    cursor = 8 + 2 + 12 * len(entries) + 4
    at_off = at_cnt = None
    if ns > 1:
        at_off, at_cnt = cursor, cursor + 4 * ns
        cursor += 8 * ns
    offsets, o = [], cursor
    for s in strips:
        offsets.append(o)
        o += len(s)
    head = bytearray(cursor)
    head[0:8] = b"II*\0" + struct.pack("<I", 8)
    head[8:10] = struct.pack("<H", len(entries))
    for i, (tag, typ, v) in enumerate(entries):
        if isinstance(v, str):
            v = tuple(offsets)
        e = 10 + 12 * i
        head[e:e + 8] = struct.pack("<HHI", tag, typ, len(v))
        payload = struct.pack("<" + ("H" if typ == 3 else "I") * len(v), *v)
        if len(payload) <= 4:
            head[e + 8:e + 8 + len(payload)] = payload
        else:
            at = at_off if tag == 273 else at_cnt
            head[e + 8:e + 12] = struct.pack("<I", at)
            head[at:at + len(payload)] = payload
    return bytes(head) + b"".join(strips)
