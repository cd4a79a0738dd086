"""The two ends of the reference's parcel job: the parcel shapefile read (`shapefile.Reader` and `get_shape`,
inference/prepare_utils.py:33) and the copy of it whose records carry the PRED_* fields
(`update_shapefile_with_predictions`, inference/predict_utils.py:149-177).

The ESRI shapefile triple .shp / .shx / .dbf is parsed here with `struct` and numpy (include/strata_hip.h, "Parcel shapefiles": OUR
reading of the ESRI Shapefile Technical Description and of dBase III, pinned by files typed out by hand, not by pyshp -- neither pyshp
nor shapely is needed, and neither is used).  Writing annotates and never re-encodes: .shp, .shx, .prj and .cpg are copied byte for
byte, the .dbf keeps every source record byte and gains n fields of type F that are formatted on the device
(`hip_ops.dbf_annotate`, csrc/dbf.hip), fetched with the records in ONE device-to-host read.

UNPINNED: pyshp rewrites .shp / .shx from the parsed shapes and stamps today's date, and formats an F value as
`format(float(v), ".10f")[:size].rjust(size)` with size 50 -- as we remember pyshp 2.x; it could not be run here."""
import os
import shutil
import struct
from dataclasses import dataclass, field

import numpy as np
import torch

from . import hip_ops as ops
from .geotiff import SHP_FIELDS

POLYGON_TYPES = (5, 15, 25)                 # Polygon, PolygonZ, PolygonM; 0 is the null shape
SIBLINGS = (".shx", ".prj", ".cpg")
OVERFLOW_FROM = 2.0 ** 53                   # a finite |v| from here on fills its field with '*'


def _base(path) -> str:
    path = os.fspath(path)
    root, ext = os.path.splitext(path)
    return root if ext.lower() in (".shp", ".shx", ".dbf") else path


def format_field_ref(v, size: int, decimal: int) -> bytes:
    """The Python restatement of the device's field (csrc/dbf_rules.h): pyshp's expression as we remember it, and the dBase
    overflow convention for a finite |v| >= 2^53."""
    v = float(v)
    if np.isfinite(v) and abs(v) >= OVERFLOW_FROM:
        return b"*" * size
    return format(v, ".%df" % decimal)[:size].rjust(size).encode("ascii")


@dataclass
class ParcelShapes:
    """`shp.read`: shapes -- K entries, entry k a list of fp64 (V,2) arrays, one per part in file order (views into `points`), None
    for a null shape: what `cut_parcels`, `prepare_parcels(shapes=...)`, `atlas.report` and `polygon_edges` take --; boxes (K,4) fp64
    x_min, y_min, x_max, y_max recomputed from the vertices (NaN for a null shape); fields [(name, type, size, decimal)];
    records (K,L) uint8, the raw record bytes, deletion flag included; dbf_header, the raw header bytes; siblings, the extensions
    of the sibling files present; shape_types (K,) and points (P,2)."""
    path: str
    shapes: list
    boxes: np.ndarray
    fields: list
    records: np.ndarray
    dbf_header: bytes
    siblings: tuple
    shape_types: np.ndarray
    points: np.ndarray
    _columns: dict = field(default_factory=dict, repr=False)

    def __len__(self):
        return len(self.shapes)

    def _slot(self, name):
        at = 1
        for n, t, size, dec in self.fields:
            if n == name:
                return at, t, size, dec
            at += size
        raise KeyError(name)

    def column(self, name) -> list:
        """The decoded values of a field: C -> str, right-stripped (latin-1); N / F -> int / float, None for blanks or asterisks
        (N with decimals, or with a point in the text: float); L and D -> the text."""
        if name not in self._columns:
            at, t, size, dec = self._slot(name)
            out = []
            for k in range(len(self.records)):
                text = self.records[k, at:at + size].tobytes().decode("latin-1")
                if t == "C":
                    out.append(text.rstrip(" \0"))
                elif t in ("N", "F"):
                    s = text.strip(" \0")
                    if s == "" or "*" in s:
                        out.append(None)
                    elif t == "N" and dec == 0 and "." not in s and "e" not in s.lower():
                        out.append(int(s))
                    else:
                        out.append(float(s))
                else:
                    out.append(text)
            self._columns[name] = out
        return self._columns[name]

    def index_of(self, value, field="ID") -> int:
        """The record index `get_shape` finds: the first record whose `field` equals `value`; KeyError otherwise."""
        for k, v in enumerate(self.column(field)):
            if v == value:
                return k
        raise KeyError(value)


def _read_shp(data: bytes, path: str):
    if len(data) < 100:
        raise ValueError(f"{path}: {len(data)} bytes, a .shp header has 100")
    code, = struct.unpack_from(">i", data, 0)
    words, = struct.unpack_from(">i", data, 24)
    version, file_type = struct.unpack_from("<ii", data, 28)
    if code != 9994:
        raise ValueError(f"{path}: file code {code}, expected 9994")
    if version != 1000:
        raise ValueError(f"{path}: version {version}, expected 1000")
    if words * 2 != len(data):
        raise ValueError(f"{path}: the header states {words * 2} bytes, the file has {len(data)}")
    if file_type not in (0,) + POLYGON_TYPES:
        raise ValueError(f"{path}: shape type {file_type}, only polygons (5, 15, 25) are read")
    types, part_lists, chunks = [], [], []
    at, total = 100, 0
    while at < len(data):
        k = len(types)
        if at + 8 > len(data):
            raise ValueError(f"{path}: record {k}: its header runs past the file")
        clen, = struct.unpack_from(">i", data, at + 4)                  # (the record number at `at` is not trusted, nor needed)
        body, end = at + 8, at + 8 + 2 * clen
        if clen < 2 or end > len(data):
            raise ValueError(f"{path}: record {k}: a content length of {clen} words runs past the file")
        t, = struct.unpack_from("<i", data, body)
        if t not in (0,) + POLYGON_TYPES:
            raise ValueError(f"{path}: record {k}: shape type {t}, only 0, 5, 15 and 25 are read")
        types.append(t)
        if t == 0:
            part_lists.append(None)
        else:
            if 2 * clen < 44:
                raise ValueError(f"{path}: record {k}: {2 * clen} bytes cannot hold a polygon's box and counts")
            n_parts, n_points = struct.unpack_from("<ii", data, body + 36)
            need = 44 + 4 * n_parts + 16 * n_points
            if n_parts < 1 or n_points < 1 or need > 2 * clen:
                raise ValueError(f"{path}: record {k}: {n_parts} parts and {n_points} points do not fit {2 * clen} bytes")
            parts = np.frombuffer(data, dtype="<i4", count=n_parts, offset=body + 44).astype(np.int64)
            if parts[0] != 0 or (np.diff(parts) <= 0).any() or parts[-1] >= n_points:
                raise ValueError(f"{path}: record {k}: Parts {parts.tolist()} must start at 0, increase strictly and stay below {n_points}")
            bounds = np.concatenate([parts, [n_points]])
            if (np.diff(bounds) < 2).any():
                raise ValueError(f"{path}: record {k}: a part with fewer than 2 vertices")
            pts = np.frombuffer(data, dtype="<f8", count=2 * n_points, offset=body + 44 + 4 * n_parts).reshape(n_points, 2)
            if not np.isfinite(pts).all():
                raise ValueError(f"{path}: record {k}: a vertex that is not finite")
            part_lists.append(bounds + total)
            chunks.append(pts)
            total += n_points
        at = end
    points = np.ascontiguousarray(np.concatenate(chunks, 0), dtype=np.float64) if chunks else np.zeros((0, 2), dtype=np.float64)
    shapes, boxes = [], np.full((len(types), 4), np.nan, dtype=np.float64)
    for k, bounds in enumerate(part_lists):
        if bounds is None:
            shapes.append(None)
            continue
        shapes.append([points[a:b] for a, b in zip(bounds[:-1], bounds[1:])])
        v = points[bounds[0]:bounds[-1]]
        boxes[k] = (v[:, 0].min(), v[:, 1].min(), v[:, 0].max(), v[:, 1].max())
    return shapes, boxes, np.asarray(types, dtype=np.int32), points


def parse_dbf_header(data: bytes, path: str = ".dbf"):
    """-> (K, header_len, L, fields) of a .dbf's bytes; ValueError on a header that does not describe them."""
    if len(data) < 33:
        raise ValueError(f"{path}: {len(data)} bytes cannot hold a dBase header")
    K, = struct.unpack_from("<I", data, 4)
    header_len, L = struct.unpack_from("<HH", data, 8)
    if header_len < 33 or header_len > len(data) or L < 1:
        raise ValueError(f"{path}: a header of {header_len} bytes and records of {L} in a file of {len(data)}")
    fields, at = [], 32
    while at < header_len and data[at] != 0x0D:
        if at + 32 > header_len:
            raise ValueError(f"{path}: field descriptor {len(fields)} runs past the header's {header_len} bytes")
        name = data[at:at + 11].split(b"\0", 1)[0].decode("latin-1")
        fields.append((name, chr(data[at + 11]), data[at + 16], data[at + 17]))
        at += 32
    if at != header_len - 1 or data[at] != 0x0D:
        raise ValueError(f"{path}: the field descriptors end at byte {at}, the header says {header_len - 1}")
    names = [f[0] for f in fields]
    if len(set(names)) != len(names):
        raise ValueError(f"{path}: duplicate field names in {names}")
    if 1 + sum(f[2] for f in fields) != L:
        raise ValueError(f"{path}: the fields take {1 + sum(f[2] for f in fields)} bytes, the header says records of {L}")
    if len(data) < header_len + K * L:
        raise ValueError(f"{path}: {K} records of {L} bytes after a header of {header_len} need {header_len + K * L} bytes, "
                         f"the file has {len(data)}")
    return K, header_len, L, fields


def read(path) -> ParcelShapes:
    """The parcel shapefile at `path` (the .shp file, or the base name) -> `ParcelShapes`.  The record offsets come from walking the
    .shp; the .shx is not read.  Everything the files state is checked against their bytes before anything is returned:
    ValueError names the record."""
    base = _base(path)
    with open(base + ".shp", "rb") as f:
        shp_data = f.read()
    with open(base + ".dbf", "rb") as f:
        dbf_data = f.read()
    shapes, boxes, types, points = _read_shp(shp_data, base + ".shp")
    K, header_len, L, fields = parse_dbf_header(dbf_data, base + ".dbf")
    if K != len(shapes):
        raise ValueError(f"{base}.dbf: {K} records for the {len(shapes)} shapes of the .shp")
    records = np.frombuffer(dbf_data, dtype=np.uint8, count=K * L, offset=header_len).reshape(K, L).copy()
    siblings = tuple(e for e in SIBLINGS if os.path.exists(base + e))
    return ParcelShapes(base + ".shp", shapes, boxes, fields, records, dbf_data[:header_len], siblings, types, points)


@dataclass
class WrittenShapefile:
    """`shp.write_predictions`: path of the written .shp, files (every path written), fields (the appended names), rows (K,) the
    value row of every record (-1: `missing`), overflow: the fields filled with '*' (a finite |v| >= 2^53)."""
    path: str
    files: list
    fields: list
    rows: np.ndarray
    overflow: int


def extended_dbf_header(header: bytes, names, size: int, decimal: int) -> bytes:
    """The source's .dbf header with len(names) descriptors of type F appended before the 0x0D: header_len += 32 n,
    record_len += n size, the date bytes kept."""
    n = len(names)
    header_len, L = struct.unpack_from("<HH", header, 8)
    out = bytearray(header[:-1])
    for name in names:
        raw = name.encode("ascii")
        if not 1 <= len(raw) <= 10:
            raise ValueError(f"field name {name!r}: 1 to 10 ASCII characters")
        d = bytearray(32)
        d[0:len(raw)] = raw
        d[11] = ord("F")
        d[16], d[17] = size, decimal
        out += d
    out += b"\x0d"
    struct.pack_into("<HH", out, 8, header_len + 32 * n, L + n * size)
    return bytes(out)


def write_annotated(shapes: ParcelShapes, dst, names, size: int, decimal: int, annotated) -> list:
    """The files of a shapefile whose records are already annotated: annotated (K, L + n size) uint8, every row the source record
    followed by the n fields.  .shp and the siblings are copied byte for byte; the .dbf is the extended header, the rows, one 0x1A.
    -> the paths written."""
    src_base, dst_base = _base(shapes.path), _base(dst)
    K, L = shapes.records.shape
    annotated = np.ascontiguousarray(annotated, dtype=np.uint8)
    if annotated.shape != (K, L + len(names) * size):
        raise ValueError(f"annotated: expected {(K, L + len(names) * size)}, got {annotated.shape}")
    header = extended_dbf_header(shapes.dbf_header, names, size, decimal)
    files = []
    for ext in (".shp",) + tuple(shapes.siblings):
        shutil.copyfile(src_base + ext, dst_base + ext)
        files.append(dst_base + ext)
    with open(dst_base + ".dbf", "wb") as f:
        f.write(header)
        f.write(annotated.tobytes())
        f.write(b"\x1a")
    files.append(dst_base + ".dbf")
    return files


def write_predictions(src, dst, values, parcel_index=None, empty=None, fields=SHP_FIELDS, size: int = 50, decimal: int = 10,
                      missing: float = -1.0, device=None) -> WrittenShapefile:
    """`update_shapefile_with_predictions`: the shapefile `src` (a path or a `ParcelShapes`) copied to `dst` with one F field per
    entry of `fields` = ((name, column), ...) appended to every record.

    values: an `AtlasReport` (its band_means and empty; n_bands == 6 when a field asks for column 4, PRED_ADM) or an (R,C) fp64
    array or device tensor (a host array is uploaded: R C 8 bytes).  parcel_index (R,): the shapefile record of value row j --
    `ParcelCut.parcel_index` --, None = the identity (R == K).  empty: None or R flags.  A record with no row, or whose row is
    empty, gets `missing` in every field: the reference's mock -1 for a parcel without a .tif.
    .shp, .shx, .prj, .cpg: copied byte for byte.  .dbf: the source's header extended, every record the source's bytes followed
    by the fields formatted on the device, one 0x1A.  ONE launch, ONE device-to-host read."""
    shapes = src if isinstance(src, ParcelShapes) else read(src)
    src_base, dst_base = _base(shapes.path), _base(dst)
    for ext in (".shp", ".dbf") + shapes.siblings:
        if os.path.exists(dst_base + ext) and os.path.samefile(src_base + ext, dst_base + ext):
            raise ValueError(f"{dst_base}{ext}: src and dst are the same file")
    if os.path.abspath(src_base) == os.path.abspath(dst_base):
        raise ValueError(f"{dst_base}: src and dst are the same file")
    names, cols = [str(f[0]) for f in fields], [int(f[1]) for f in fields]
    n, size, decimal = len(names), int(size), int(decimal)
    K, L = shapes.records.shape
    have = [f[0] for f in shapes.fields]
    for name in names:
        if name in have or names.count(name) > 1:
            raise ValueError(f"field {name!r} already exists")
    if n < 1 or len(have) + n > 255:
        raise ValueError(f"{len(have)} + {n} fields: a table holds 1 to 255")
    if not 1 <= size <= 254 or not 0 <= decimal <= 15 or decimal + 2 > size:
        raise ValueError(f"size {size}, decimal {decimal}: expected 1..254, 0..15 and decimal + 2 <= size")
    if L + n * size > 65535:
        raise ValueError(f"records of {L + n * size} bytes: at most 65535")
    if hasattr(values, "band_means") and hasattr(values, "n_bands"):
        if (max(cols) >= 4 and values.n_bands != 6) or max(cols) >= values.n_bands:          # bands 0..3 are the same in both layouts
            raise ValueError(f"the report has {values.n_bands} bands: band {max(cols)} (PRED_ADM is band 4 of six) needs "
                             "report(admissibility=...)")
        if empty is None:
            empty = values.empty
        values = values.band_means
    if not isinstance(values, torch.Tensor):
        values = torch.from_numpy(np.ascontiguousarray(np.asarray(values, dtype=np.float64)))
    if values.dim() != 2 or values.dtype != torch.float64 or values.shape[0] < 1:
        raise ValueError(f"values: expected (R,C) fp64 with R >= 1, got {tuple(values.shape)} {values.dtype}")
    R, C = values.shape
    if min(cols) < 0 or max(cols) >= C:
        raise ValueError(f"fields: columns {cols} of {C}")
    if parcel_index is None:
        if R != K:
            raise ValueError(f"values: {R} rows for {K} records; pass parcel_index")
        parcel_index = np.arange(K)
    parcel_index = np.asarray(parcel_index, dtype=np.int64).reshape(-1)
    if len(parcel_index) != R:
        raise ValueError(f"parcel_index: expected one entry per value row ({R}), got {len(parcel_index)}")
    if (parcel_index < 0).any() or (parcel_index >= K).any():
        raise ValueError(f"parcel_index: entries outside [0, {K})")
    if len(np.unique(parcel_index)) != R:
        raise ValueError("parcel_index: a record is named twice")
    rows = np.full(K, -1, dtype=np.int32)
    rows[parcel_index] = np.arange(R, dtype=np.int32)
    if empty is not None:
        empty = np.asarray(empty, dtype=bool).reshape(-1)
        if len(empty) != R:
            raise ValueError(f"empty: expected one flag per value row ({R}), got {len(empty)}")
        rows[parcel_index[empty]] = -1
    dev = values.device if values.is_cuda else torch.device("cuda" if device is None else device)
    with torch.cuda.device(dev):
        values = values.to(dev).contiguous()
        records = torch.from_numpy(shapes.records).to(dev)
        done = ops.dbf_annotate(records, values, torch.from_numpy(rows).to(dev), cols, size, decimal, missing).read()
    files = write_annotated(shapes, dst_base, names, size, decimal, done.records)
    return WrittenShapefile(dst_base + ".shp", files, names, rows, done.overflow)
