"""LAS files to the (10,T) device cloud of the reference's `load_las_file` (utils/load_data.py:149-184), decoded on the device.

    cloud = las.load_las(path)                       # (10,T) fp32 on the device: x, y, z, r, g, b, nir, intensity, return_num, num_returns
    plots = prepare_parcel(cloud, args)              # ... predict_parcel_cloud, pseudo_label_parcel take it as it is
    pc = las.load_parcel_clouds(paths)               # K files into one ParcelClouds arena, no second copy

The header is parsed on the host (`read_header`, pure `struct`); the point-record block goes to the device as the file holds it,
through a pinned staging buffer in one copy, and ONE launch of sn2_las_decode (csrc/las.hip) writes the ten rows.

The reference reads its files with laspy 1.x (`laspy.file.File`), which laspy 2 removed; it is not a dependency of this package.
The record layout here is therefore OUR reading of the ASPRS LAS 1.0-1.4 specification (include/strata_hip.h, "LAS point
records"), pinned by hand-written records in the tests.  Two coordinate modes:
  coords="reference" (default): load_las_file's arithmetic, raw integer / 100 in fp64, then fp32; the header's scale and offset
      are not used, exactly as the reference ignores them.  origin = (X0, Y0, Z0) INTEGER raw units, subtracted before the division.
  coords="header": (X * scale + offset) - origin in fp64, then fp32 -- laspy's `.x` for origin 0.  origin in metres.
An origin keeps centimetres where fp32 alone cannot: at Lambert-93 northings (6.5e6 m) fp32 has a step of 0.5 m.
Nothing is filtered: the reference's three file-name-specific `clean` filters (utils/load_data.py:187-202) are the caller's, to
be applied as a mask on the device.  LAZ is refused.

Writing (csrc/las_write.hip; include/strata_hip.h, "LAS point records, written"): the way back for the per-point scores.

    mosaic, plots, scores = predict_parcel_cloud(model, cloud, args, points=True)
    las.write_scored(src, dst, scores, fields="all", classify=True)       # src's records + class byte + ten extra-byte fields
    las.write_parcels(tile_paths, cut, dst_paths, result)                   # one file per kept parcel of a ParcelCut

The records are NOT re-encoded from the fp32 cloud: `encode` copies every byte the source record holds and only sets the
classification and appends extra bytes, in one launch.  The header, the VLRs and the Extra Bytes descriptors are patched on the
host (`patch_header`, pure `struct`) -- like the record layout OUR reading of the specification: no third-party LAS reader can be
run beside this package.
"""
import os
import struct
from dataclasses import dataclass, replace
from typing import Tuple

import numpy as np
import torch

from . import hip_ops as ops

HEADER_BYTES_1_0 = 227       # LAS 1.0 - 1.2; 1.3: 235; 1.4: 375
HEADER_BYTES_1_4 = 375


@dataclass(frozen=True)
class LasHeader:
    version: Tuple[int, int]
    point_format: int
    record_length: int
    offset_to_points: int
    n_points: int
    scale: Tuple[float, float, float]
    offset: Tuple[float, float, float]
    mins: Tuple[float, float, float]
    maxs: Tuple[float, float, float]
    header_size: int

    @property
    def n_bytes(self) -> int:
        """bytes of the point-record block"""
        return self.n_points * self.record_length


def _head_bytes(src, n=HEADER_BYTES_1_4):
    """(the first n bytes, the total size) of a path or a bytes-like object"""
    if isinstance(src, (bytes, bytearray, memoryview)):
        b = bytes(src[:n])
        return b, len(src)
    with open(src, "rb") as f:
        return f.read(n), os.fstat(f.fileno()).st_size


def read_header(path_or_bytes) -> LasHeader:
    """The public header block of a LAS 1.0-1.4 file.  ValueError on a bad signature, a LAZ file, a point format the decoder does
    not know, a record length below the format's, or a file shorter than offset + n_points * record_length."""
    b, size = _head_bytes(path_or_bytes)
    if len(b) < HEADER_BYTES_1_0 or b[:4] != b"LASF":
        raise ValueError("not a LAS file: the signature is not 'LASF' (or the header is cut short)")
    major, minor = b[24], b[25]
    header_size, offset_to_points = struct.unpack_from("<HI", b, 94)
    fmt_byte, record_length, legacy_count = struct.unpack_from("<BHI", b, 104)
    if fmt_byte & 0xC0:
        raise ValueError(f"LAZ (compressed) point data, format byte 0x{fmt_byte:02x}: decompress the file first")
    if fmt_byte > 10:
        raise ValueError(f"unsupported LAS point format {fmt_byte} (0..10 are defined)")
    least = ops.las_record_min_length(fmt_byte)
    if record_length < least:
        raise ValueError(f"record length {record_length} below the {least} bytes of point format {fmt_byte}")
    n_points = legacy_count
    if legacy_count == 0 and (major, minor) >= (1, 4):
        if len(b) < HEADER_BYTES_1_4:
            raise ValueError("LAS 1.4 header cut short")
        n_points = struct.unpack_from("<Q", b, 247)[0]
    d = struct.unpack_from("<12d", b, 131)
    if offset_to_points < header_size or size < offset_to_points + n_points * record_length:
        raise ValueError(f"file of {size} bytes is shorter than its header says: {n_points} records of {record_length} bytes "
                         f"from byte {offset_to_points}")
    return LasHeader((major, minor), fmt_byte, record_length, offset_to_points, n_points, d[0:3], d[3:6], (d[7], d[9], d[11]),
                     (d[6], d[8], d[10]), header_size)


def decode(raw, header: LasHeader, coords: str = "reference", origin=None, out=None, col0: int = 0, classification=False):
    """raw: uint8 device tensor that starts at the first record (`header.n_bytes` bytes or more) -> the (10,T) cloud, or columns
    col0 .. col0 + T of `out` (10, >= col0 + T), e.g. a ParcelClouds arena.  origin: (X0, Y0, Z0) integers for "reference",
    metres for "header"; None = 0.  classification: True -> (cloud, classification (T) uint8); or a uint8 tensor as long as
    out's rows, written at col0 .. col0 + T."""
    T = header.n_points
    cls = classification
    if cls is True:
        cls = torch.empty((out.shape[1] if out is not None else T), dtype=torch.uint8, device=raw.device)
    elif cls is False:
        cls = None
    if coords == "header":
        o = (0.0, 0.0, 0.0) if origin is None else tuple(float(v) for v in origin)
        kw = dict(xform=tuple(header.scale) + tuple(header.offset) + o)
    else:
        if origin is not None and any(int(v) != v for v in origin):
            raise ValueError("origin: the 'reference' mode takes integer raw units (X0, Y0, Z0)")
        kw = dict(raw0=origin)
    with torch.cuda.device(raw.device):
        cloud = ops.las_decode(raw, header.point_format, header.record_length, T, coords, out=out, col0=col0, classification=cls, **kw)
    return (cloud, cls) if classification is not False else cloud


def _device(device):
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def _upload_points(path, header: LasHeader, dev, pinned=None):
    """The point-record block of `path` on `dev`: read into a pinned staging buffer, ONE host-to-device copy.  pinned: a pinned
    uint8 buffer to reuse (at least header.n_bytes long)."""
    n = header.n_bytes
    if pinned is None or pinned.numel() < n:
        pinned = torch.empty(max(n, 16), dtype=torch.uint8, pin_memory=True)
    view = memoryview(pinned.numpy())[:n]
    with open(path, "rb") as f:
        f.seek(header.offset_to_points)
        got = f.readinto(view) if n else 0
    if got != n:
        raise ValueError(f"{path}: read {got} of {n} bytes of point records")
    raw = torch.empty(max(n, 16), dtype=torch.uint8, device=dev)
    raw[:n].copy_(pinned[:n], non_blocking=True)
    return raw[:n], pinned


def load_las(path, device=None, coords: str = "reference", origin=None, classification=False):
    """`load_las_file(path)` of the reference on the device: (10,T) fp32 -- with classification=True, (cloud, (T) uint8)."""
    h = read_header(path)
    dev = _device(device)
    raw, pinned = _upload_points(path, h, dev)
    res = decode(raw, h, coords, origin, classification=classification)
    torch.cuda.current_stream(dev).synchronize()          # the staging buffer goes away with this call
    return res


def load_plot(path, args, device=None, coords: str = "reference", origin=None):
    """The `cloud` of the reference's get_cloud_data (utils/load_data.py:122-126) for one plot file: load_las, then the local
    z-normalisation (`pre_transform`, znorm_radius_in_meters) on rows 0..2 -- WITHOUT `clean`, its three file-name-specific
    filters.  -> (10,T) fp32 on the device."""
    cloud = load_las(path, device, coords, origin)
    with torch.cuda.device(cloud.device):
        cloud[2] = ops.znorm(cloud[:3].contiguous(), float(getattr(args, "znorm_radius_in_meters", 1.5)))[1]
    return cloud


def load_parcel_clouds(paths, device=None, coords: str = "reference", origin=None, classification=False, headers=None):
    """K parcel files -> ParcelClouds: the K headers are read first, ONE (10, sum T) arena is allocated, and file k is decoded
    into the columns point_start[k] ..: one upload and one launch per file, the clouds' memory held once.  origin: one triple
    for every file (so the parcels keep their relative positions) or None.  classification=True: (ParcelClouds, (sum T) uint8),
    the class byte of every arena column.  headers: the files' `read_header` results where the caller already has them."""
    from .parcel import ParcelClouds
    paths = list(paths)
    if not paths:
        raise ValueError("load_parcel_clouds: no file")
    heads = [read_header(p) for p in paths] if headers is None else list(headers)
    if len(heads) != len(paths):
        raise ValueError("load_parcel_clouds: one header per file")
    counts = [h.n_points for h in heads]
    if min(counts) == 0:
        raise ValueError(f"load_parcel_clouds: {paths[counts.index(0)]} holds no point")
    if sum(counts) >= 2 ** 31:
        raise ValueError("load_parcel_clouds: at most 2^31 - 1 points in all")
    dev = _device(device)
    arena = torch.empty(10, sum(counts), dtype=torch.float32, device=dev)
    cls = torch.empty(sum(counts), dtype=torch.uint8, device=dev) if classification else None
    pinned = torch.empty(max(h.n_bytes for h in heads), dtype=torch.uint8, pin_memory=True)
    col0 = 0
    for p, h in zip(paths, heads):
        raw, pinned = _upload_points(p, h, dev, pinned)
        decode(raw, h, coords, origin, out=arena, col0=col0, classification=cls if classification else False)
        torch.cuda.current_stream(dev).synchronize()      # the next file overwrites the staging buffer
        col0 += h.n_points
    pc = ParcelClouds.from_arena(arena, counts)
    return (pc, cls) if classification else pc


def load_parcels(paths, shapes, buffer_m: float = 20, coords: str = "reference", origin=None, drop_classes=(), device=None):
    """LAS tiles + K parcel polygons -> `parcel.ParcelCut`: `load_parcel_clouds(paths)` over the tiles, their classification byte
    into one (T_all) buffer when drop_classes is given, then `parcel.cut_parcels` over the arena -- no host pass over points.
    `point_index` of the result indexes the columns of the arena of the tiles READ, in the order of `paths`.

    shapes: K ring lists in the FILES' frame (metres, e.g. Lambert-93).  origin: the triple `load_parcel_clouds` takes -- raw
    integer units (centimetres) in the "reference" mode, metres in the "header" mode --; the same shift, in metres, is subtracted
    from the shapes, so cloud and polygons stay in one frame and `shapes_kept` comes back in the cloud's.
    coords="header": a tile whose header box (`read_header`'s mins / maxs) misses every parcel's expanded bounding box is not read
    at all, a host test that trusts the header's extents (a file whose writer left them empty loses its points).
    coords="reference" ignores the header's scale and offset, so there every tile is read."""
    from .parcel import ParcelCut, cut_parcels, polygon_edges, shift_rings
    paths, shapes = list(paths), list(shapes)
    if not paths:
        raise ValueError("load_parcels: no file")
    if not shapes:
        raise ValueError("load_parcels: no parcel")
    o = (0.0, 0.0, 0.0) if origin is None else tuple(origin)
    shift = (float(o[0]), float(o[1])) if coords == "header" else (int(o[0]) / 100, int(o[1]) / 100)
    heads = [read_header(p) for p in paths]
    dev = _device(device)
    if coords == "header":
        boxes = ops.cut_boxes([polygon_edges(r) for r in shift_rings(shapes, shift)], buffer_m)
        keep = []
        for h in heads:
            lo, hi = np.array(h.mins[:2]) - shift, np.array(h.maxs[:2]) - shift
            slack = 2.0 ** -22 * max(float(np.abs(lo).max()), float(np.abs(hi).max()))       # the decoder rounds x, y to fp32
            keep.append(h.n_points > 0 and bool(((boxes[:, 0] <= hi[0] + slack) & (boxes[:, 2] >= lo[0] - slack) &
                                                 (boxes[:, 1] <= hi[1] + slack) & (boxes[:, 3] >= lo[1] - slack)).any()))
        paths, heads = [p for p, k in zip(paths, keep) if k], [h for h, k in zip(heads, keep) if k]
        if not paths:
            return ParcelCut(None, np.zeros(0, dtype=np.int64), np.zeros(len(shapes), dtype=np.int64),
                             torch.empty(0, dtype=torch.int32, device=dev), [])
    drop = tuple(drop_classes)
    if drop:
        pc, cls = load_parcel_clouds(paths, dev, coords, origin, classification=True, headers=heads)
    else:
        pc, cls = load_parcel_clouds(paths, dev, coords, origin, headers=heads), None
    return cut_parcels(pc, shapes, buffer_m, origin=shift, classification=cls, drop_classes=drop)


# ---- writing: records annotated on the device (ops.las_encode), the header and the VLRs patched on the host -----------------------
FIELDS = ops.LAS_FIELDS
DEFAULT_CLASS_CODES = (3, 2, 4, 5)        # ASPRS standard classes: low vegetation, ground, medium vegetation, high vegetation
VLR_HEADER_BYTES, EVLR_HEADER_BYTES, DESCRIPTOR_BYTES = 54, 60, 192
EXTRA_BYTES_USER_ID, EXTRA_BYTES_RECORD_ID = b"LASF_Spec", 4
_TYPE_BYTES = (0, 1, 1, 2, 2, 4, 4, 8, 8, 4, 8)      # Extra Bytes data types 1..10: u8 i8 u16 i16 u32 i32 u64 i64 f32 f64
_FIELD_DESCRIPTIONS = ("coverage, low vegetation", "coverage, bare soil", "coverage, medium vegetation", "coverage, high vegetation",
                       "probability, low vegetation", "probability, bare soil", "probability, medium vegetation",
                       "probability, high vegetation", "sum of the plots' weights", "plots that sampled the point")      # 31 bytes at most


def _scores_of(result):
    """PointScores -> its finalize(); a PointScoreResult (anything with scores, weight, hits) as it is; None -> three Nones"""
    if result is None:
        return None, None, None
    if hasattr(result, "finalize") and not hasattr(result, "scores"):
        result = result.finalize()
    return result.scores, result.weight, result.hits


def encode(raw, header: LasHeader, result=None, *, point_index=None, col0: int = 0, n_out=None, fields=(), classify: bool = False,
           class_codes=DEFAULT_CLASS_CODES, unscored=None, out=None, stats=None):
    """Source records annotated with per-point scores, on the device, in one launch (ops.las_encode) -> (records uint8 on the
    device: n_out records of header.record_length + E bytes, `ops.LasEncodeStats`).

    raw: the source records as the file holds them (`read_records`), header.n_points of them.  result: an
    `inference.PointScoreResult` or `PointScores` (None: a pure copy or gather).  Output record i is source record point_index[i]
    (int32 on the device; None: record i) with score column col0 + i.  fields: names out of `FIELDS`, or "all": appended as extra
    bytes in FIELDS' order, fp32 but `hits`, a uint16 that saturates at 65535.  classify: the classification becomes
    class_codes[argmax of the four class probabilities] (ties to the lowest index) where hits > 0 and `unscored` elsewhere (None:
    the source's class stays); formats 0-5 keep their three flag bits and take codes up to 31.  stats: a LasEncodeStats to
    accumulate into (several launches for one file)."""
    scores, weight, hits = _scores_of(result)
    with torch.cuda.device(raw.device):
        return ops.las_encode(raw, header.point_format, header.record_length, header.n_points, point_index=point_index, n_out=n_out,
                              scores=scores, weight=weight, hits=hits, col0=col0, field_mask=ops.las_field_mask(fields),
                              class_codes=tuple(class_codes) if classify else None, unscored=-1 if unscored is None else int(unscored),
                              out=out, stats=stats)


def read_records(path, device=None):
    """-> (raw, header): the point-record block of a LAS file on the device as the file holds it (one pinned host-to-device copy,
    what `load_las` does before it decodes) and its `read_header`."""
    h = read_header(path)
    dev = _device(device)
    raw, pinned = _upload_points(path, h, dev)
    torch.cuda.current_stream(dev).synchronize()          # the staging buffer goes away with this call
    return raw, h


def _descriptor(data_type: int, name: bytes, options: int = 0, description: bytes = b"") -> bytes:
    """One 192-byte Extra Bytes descriptor: reserved[2], data_type, options, name[32], unused[4], no_data[24], min[24], max[24],
    scale[24], offset[24], description[32]"""
    d = bytearray(DESCRIPTOR_BYTES)
    name, description = name[:31], description[:31]        # both NUL-terminated in their 32 bytes
    d[2], d[3] = data_type, options
    d[4:4 + len(name)] = name
    d[160:160 + len(description)] = description
    return bytes(d)


def _descriptor_bytes(d: bytes) -> int:
    """the bytes of a record that a descriptor covers: type 0 holds its size in `options`, 11..30 are 2- and 3-tuples of 1..10"""
    t = d[2]
    if t == 0:
        return d[3]
    if t > 30:
        raise ValueError(f"Extra Bytes descriptor with data type {t}")
    return (1 + (t - 1) // 10) * _TYPE_BYTES[(t - 1) % 10 + 1]


def extra_bytes_descriptors(field_mask: int) -> bytes:
    """the descriptors of the appended fields, in the order of the bytes: data type 9 (fp32), 3 (uint16) for hits"""
    return b"".join(_descriptor(3 if k == 9 else 9, FIELDS[k].encode(), 0, _FIELD_DESCRIPTIONS[k].encode())
                    for k in range(10) if (field_mask >> k) & 1)


def _walk_vlrs(block: bytes, n: int):
    """(start, end) of each of the n VLRs at the head of `block`"""
    at, spans = 0, []
    for _ in range(n):
        if at + VLR_HEADER_BYTES > len(block):
            raise ValueError("the VLRs run past the offset to the point data")
        end = at + VLR_HEADER_BYTES + struct.unpack_from("<H", block, at + 20)[0]
        if end > len(block):
            raise ValueError("the VLRs run past the offset to the point data")
        spans.append((at, end))
        at = end
    return spans


def patch_header(src, n_points: int, field_mask: int = 0, stats=None):
    """The frame of a written file around its point records -> (head, tail): `head` = the source's public header, patched, its
    VLRs (the CRS among them) verbatim, the Extra Bytes VLR, and whatever else the source holds before its points; `tail` = the
    source's EVLRs verbatim.  src: a path or the file's bytes.  n_points records of the source's length + E follow `head`.
    stats: a read `ops.LasEncodeStats` (extents and by-return counts; None: zeros).

    Patched: offset to points (96), number of VLRs (100), record length (105), legacy count (107) and legacy by-return (111) --
    both zero where the source's legacy count was zero in a 1.4 file --, the extents at 179 (max X, min X, max Y, min Y, max Z, min
    Z as raw * scale + offset in fp64); for 1.4 the first-EVLR offset (235), the 64-bit count (247) and the fifteen by-return counts
    (255).  Extra Bytes VLR (user id LASF_Spec, record id 4): the source's is extended; source extra bytes that no descriptor
    covers get a data-type-0 descriptor first, so ours line up with the appended bytes.  This is OUR reading of the
    specification (tables 3, 4, 24-26 of LAS 1.4 R15); waveform packets are not followed."""
    h = read_header(src)
    E = ops.las_extra_bytes(field_mask)
    if isinstance(src, (bytes, bytearray, memoryview)):
        blob = bytes(src)
        front = blob[:h.offset_to_points]
    else:
        blob = None
        with open(src, "rb") as f:
            front = f.read(h.offset_to_points)
    head = bytearray(front[:h.header_size])
    block = front[h.header_size:]
    n_vlr = struct.unpack_from("<I", head, 100)[0]
    spans = _walk_vlrs(block, n_vlr)
    vlrs = [block[a:b] for a, b in spans]
    padding = block[spans[-1][1] if spans else 0:]
    if E:
        own = [i for i, v in enumerate(vlrs) if v[2:18].rstrip(b"\0") == EXTRA_BYTES_USER_ID and
               struct.unpack_from("<H", v, 18)[0] == EXTRA_BYTES_RECORD_ID]
        payload = vlrs[own[0]][VLR_HEADER_BYTES:] if own else b""
        if len(payload) % DESCRIPTOR_BYTES:
            raise ValueError("the source's Extra Bytes VLR is no whole number of descriptors")
        covered = sum(_descriptor_bytes(payload[i:i + DESCRIPTOR_BYTES]) for i in range(0, len(payload), DESCRIPTOR_BYTES))
        have = h.record_length - ops.las_record_min_length(h.point_format)
        if covered > have:
            raise ValueError(f"the source's Extra Bytes descriptors cover {covered} bytes, its records hold {have}")
        gap = have - covered
        while gap:                                         # `options` is one byte
            payload += _descriptor(0, b"undocumented", min(gap, 255), b"the source's undocumented extra bytes")
            gap -= min(gap, 255)
        payload += extra_bytes_descriptors(field_mask)
        if len(payload) > 65535:
            raise ValueError("more Extra Bytes descriptors than one VLR holds")
        if own:
            v = bytearray(vlrs[own[0]][:VLR_HEADER_BYTES])
        else:
            v = bytearray(VLR_HEADER_BYTES)
            v[2:2 + len(EXTRA_BYTES_USER_ID)] = EXTRA_BYTES_USER_ID
            struct.pack_into("<H", v, 18, EXTRA_BYTES_RECORD_ID)
            v[22:22 + 11] = b"Extra Bytes"
        struct.pack_into("<H", v, 20, len(payload))
        if own:
            vlrs[own[0]] = bytes(v) + payload
        else:
            vlrs.append(bytes(v) + payload)
    body = b"".join(vlrs) + padding
    offset_to_points = h.header_size + len(body)
    L_dst = h.record_length + E
    is14 = h.version >= (1, 4) and h.header_size >= HEADER_BYTES_1_4
    src_legacy = struct.unpack_from("<I", head, 107)[0]
    by_return = (0,) * 15 if stats is None or stats.by_return is None else tuple(stats.by_return)
    legacy = not (is14 and src_legacy == 0) and n_points < 2 ** 32 and max(by_return[:5]) < 2 ** 32
    if not legacy and not is14:
        raise ValueError(f"{n_points} points do not fit the 32-bit count of a LAS {h.version[0]}.{h.version[1]} header")
    struct.pack_into("<II", head, 96, offset_to_points, len(vlrs))
    struct.pack_into("<H", head, 105, L_dst)
    struct.pack_into("<I5I", head, 107, *((n_points,) + by_return[:5] if legacy else (0,) * 6))
    ext = [0.0] * 6
    if stats is not None and stats.mins is not None:
        for a in range(3):
            ext[2 * a] = float(np.float64(stats.maxs[a]) * np.float64(h.scale[a]) + np.float64(h.offset[a]))
            ext[2 * a + 1] = float(np.float64(stats.mins[a]) * np.float64(h.scale[a]) + np.float64(h.offset[a]))
    struct.pack_into("<6d", head, 179, *ext)
    tail = b""
    if is14:
        first_evlr, n_evlr = struct.unpack_from("<QI", head, 235)
        if n_evlr:
            if first_evlr < h.offset_to_points + h.n_bytes:
                raise ValueError("the source's EVLRs start inside its point records")
            if blob is not None:
                tail = blob[first_evlr:]
            else:
                with open(src, "rb") as f:
                    f.seek(first_evlr)
                    tail = f.read()
        struct.pack_into("<Q", head, 235, offset_to_points + n_points * L_dst if n_evlr else 0)
        struct.pack_into("<Q15Q", head, 247, n_points, *by_return)
    return bytes(head) + body, tail


def _to_host(records: torch.Tensor) -> memoryview:
    """the device bytes on the host: ONE device-to-host copy into pinned memory"""
    pinned = torch.empty(max(records.numel(), 1), dtype=torch.uint8, pin_memory=True)
    pinned[:records.numel()].copy_(records, non_blocking=True)
    torch.cuda.current_stream(records.device).synchronize()
    return memoryview(pinned.numpy())[:records.numel()]


def _write_file(dst_path, head: bytes, records: memoryview, tail: bytes):
    with open(dst_path, "wb") as f:
        f.write(head)
        f.write(records)
        f.write(tail)


def write_scored(src_path, dst_path, result, device=None, **kw):
    """The whole-file case: src_path's records with `result`'s scores -- column i is record i, as `predict_parcel_cloud(load_las(
    src_path), points=True)` gives them -- to dst_path.  Upload, `encode` (kw: fields, classify, class_codes, unscored, ...), one
    device-to-host copy of the block and one of the statistics, then the file.  -> the read LasEncodeStats"""
    raw, h = read_records(src_path, device)
    records, stats = encode(raw, h, result, **kw)
    n = records.numel() // (h.record_length + ops.las_extra_bytes(ops.las_field_mask(kw.get("fields", ()))))
    host = _to_host(records)
    stats.read()
    if stats.n_bad:
        raise ValueError(f"write_scored: {stats.n_bad} point_index entries outside the source's {h.n_points} records")
    head, tail = patch_header(src_path, n, ops.las_field_mask(kw.get("fields", ())), stats)
    _write_file(dst_path, head, host, tail)
    return stats


def write_parcels(tile_paths, cut, dst_paths, result=None, device=None, **kw):
    """One LAS file per kept parcel of a `parcel.ParcelCut`, with the tiles' exact integer coordinates: parcel k's records are the
    source records cut.point_index[point_start[k] : point_start[k+1]] of the arena of the tiles READ (tile_paths, in the order
    `load_parcels` read them), its score columns the same range of `result` (what `predict_parcels(..., points=True)` returns over
    cut.clouds; None: no scores, a pure gather).  The header, VLRs and EVLRs are the first tile's.  The tiles must agree in point
    format, record length, scale and offset: ValueError names the first that differs.  A point_index entry outside the tiles
    raises ValueError after the parcel's one read.  -> the parcels' read LasEncodeStats"""
    tile_paths, dst_paths = list(tile_paths), list(dst_paths)
    if not tile_paths:
        raise ValueError("write_parcels: no tile")
    K = 0 if cut.clouds is None else cut.clouds.K
    if len(dst_paths) != K:
        raise ValueError(f"write_parcels: {len(dst_paths)} paths for {K} kept parcels")
    heads = [read_header(p) for p in tile_paths]
    for p, h in zip(tile_paths[1:], heads[1:]):
        for what in ("point_format", "record_length", "scale", "offset"):
            if getattr(h, what) != getattr(heads[0], what):
                raise ValueError(f"write_parcels: {p} differs from {tile_paths[0]} in {what}: {getattr(h, what)} != {getattr(heads[0], what)}")
    if K == 0:
        return []
    total = sum(h.n_points for h in heads)
    if total >= 2 ** 31:
        raise ValueError("write_parcels: at most 2^31 - 1 points in all")
    dev = cut.point_index.device if device is None else torch.device(device)
    h0 = heads[0]
    arena = torch.empty(max(total * h0.record_length, 16), dtype=torch.uint8, device=dev)
    pinned = torch.empty(max(max(h.n_bytes for h in heads), 16), dtype=torch.uint8, pin_memory=True)
    at = 0
    for p, h in zip(tile_paths, heads):
        if h.n_bytes:
            view = memoryview(pinned.numpy())[:h.n_bytes]
            with open(p, "rb") as f:
                f.seek(h.offset_to_points)
                got = f.readinto(view)
            if got != h.n_bytes:
                raise ValueError(f"{p}: read {got} of {h.n_bytes} bytes of point records")
            arena[at:at + h.n_bytes].copy_(pinned[:h.n_bytes], non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()  # the next tile overwrites the staging buffer
            at += h.n_bytes
    h_all = replace(h0, n_points=total)
    mask = ops.las_field_mask(kw.get("fields", ()))
    start = np.asarray(cut.clouds.point_start, dtype=np.int64)
    out = []
    for k, dst in enumerate(dst_paths):
        p0, p1 = int(start[k]), int(start[k + 1])
        records, stats = encode(arena[:total * h0.record_length], h_all, result, point_index=cut.point_index[p0:p1], col0=p0, **kw)
        host = _to_host(records)
        stats.read()
        if stats.n_bad:
            raise ValueError(f"write_parcels: parcel {k}: {stats.n_bad} point_index entries outside the tiles' {total} records")
        head, tail = patch_header(tile_paths[0], p1 - p0, mask, stats)
        _write_file(dst, head, host, tail)
        out.append(stats)
    return out
