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
"""
import os
import struct
from dataclasses import dataclass
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
