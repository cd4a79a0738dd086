"""The map files: a float32 GeoTIFF per parcel, as the reference's `merge_geotiff_rasters` (inference/geotiff_raster.py:199-235)
leaves them through GDAL -- six named bands, EPSG:2154, NaN as nodata -- written from the band arena of a `MosaicAtlas` report.

The rows of every file are packed on the device (include/strata_hip.h, "GeoTIFF image data"; csrc/tiff_pack.hip): ONE launch turns
the arena of all K canvases into the bytes the files hold after their headers, under predictor 1 or 3, band-sequential or
pixel-interleaved, and ONE device-to-host read brings them back together with the per-band statistics.  The header is laid out
here with `struct`; strips are slices of the packed block, passed through `zlib`.  GDAL and rasterio are not needed, and not used.

The file: classic little-endian TIFF, the IFD at byte 8, then the values that do not fit an entry, in tag order on even offsets,
then the strips.  Tags, ascending: 256 257 258 259 262 273 277 278 279 284 [317] [338] 339 33550 33922 34735 42112 42113.
PINNED by libtiff reading the files back: single-band files and, band by band, the BAND layout.  UNPINNED:
predictor 3 at stride C (the PIXEL layout) and the text of tag 42112, our reading of GDAL's metadata format."""
import re
import struct
import zlib
from typing import Optional

import numpy as np
import torch

from . import hip_ops as ops

FINAL_RASTER_BANDNAMES = ("VegetationBasse", "VegetationIntermediaire", "VegetationHaute", "VegetationIntermediaireDiscretisee",
                          "Admissibilite", "PonderationPredictions")
# the shapefile fields of `get_parcel_predicted_values` (inference/predict_utils.py:124-146) and the band each is the mean of
SHP_FIELDS = (("PRED_BASSE", 0), ("PRED_INTER", 1), ("PRED_HAUTE", 2), ("PRED_ADM", 4))
STRIP_BYTES = 65536
COMPRESSION = {None: 1, "none": 1, "deflate": 8}
_TYPE = {1: "B", 2: "c", 3: "H", 4: "I", 12: "d"}          # BYTE, ASCII, SHORT, LONG, DOUBLE
_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 12: 8}


def default_band_names(C: int):
    if C == 6:
        return list(FINAL_RASTER_BANDNAMES)
    if C == 5:
        return [n for n in FINAL_RASTER_BANDNAMES if n != "Admissibilite"]
    return [f"band_{i}" for i in range(C)]


def pack(band_arena, C, table, interleave="band", predictor=1, skip=None):
    """The image data blocks of `table`'s canvases on the device: `hip_ops.tiff_pack`.  -> a `hip_ops.TiffPacked`; its `.read()` is
    the ONE device-to-host copy."""
    return ops.tiff_pack(band_arena, C, table, ops.tiff_layout(interleave), predictor, skip)


def strip_rows(row_bytes: int, H: int) -> int:
    """rows per strip: the largest whole number of rows within 64 KiB, at least one, at most H"""
    return min(max(1, STRIP_BYTES // row_bytes), H)


def gdal_metadata(band_names, stats=None) -> str:
    """The text of tag 42112 (UNPINNED: our reading of GDAL's format).  stats: None, or per band None / a dict of STATISTICS_* items."""
    lines = ["<GDALMetadata>"]
    for i, name in enumerate(band_names):
        esc = str(name).replace("&", "&amp;").replace("<", "&lt;").replace(">", "&gt;")
        lines.append(f'  <Item name="DESCRIPTION" sample="{i}" role="description">{esc}</Item>')
        for key, value in sorted(((stats[i] or {}) if stats is not None else {}).items()):
            lines.append(f'  <Item name="{key}" sample="{i}">{value}</Item>')
    lines.append("</GDALMetadata>")
    return "\n".join(lines) + "\n"


def band_statistics(counts, minimum, maximum, pixels: int, means=None):
    """The STATISTICS_* items of every band from the packer's integers (and the report's fp64 means, when given)."""
    out = []
    for c in range(len(counts)):
        d = {"STATISTICS_VALID_PERCENT": "%.17g" % (100.0 * int(counts[c]) / pixels)}
        if int(counts[c]) > 0:
            d["STATISTICS_MINIMUM"] = "%.9g" % float(minimum[c])
            d["STATISTICS_MAXIMUM"] = "%.9g" % float(maximum[c])
            if means is not None and np.isfinite(means[c]):
                d["STATISTICS_MEAN"] = "%.17g" % float(means[c])
        out.append(d)
    return out


def assemble(block, C, H, W, x_min, y_max, pix, interleave="band", predictor=1, compress="deflate", level=6, rows_per_strip=None,
             band_names=None, epsg=2154, stats=None) -> bytes:
    """The whole file from a canvas's image data block (uint8, C H W 4 bytes in `interleave`'s layout under `predictor`)."""
    if compress not in COMPRESSION:
        raise ValueError(f"compress: expected 'deflate' or None, got {compress!r}")
    comp = COMPRESSION[compress]
    if predictor == 3 and comp == 1:
        raise ValueError("predictor 3 without compression is refused: readers that bypass libtiff ignore the tag there")
    pixel = ops.tiff_layout(interleave) == ops.TIFF_LAYOUTS["pixel"]
    block = np.ascontiguousarray(block, dtype=np.uint8).reshape(-1)
    if block.size != 4 * C * H * W:
        raise ValueError(f"block: expected {4 * C * H * W} bytes, got {block.size}")
    names = default_band_names(C) if band_names is None else list(band_names)
    if len(names) != C:
        raise ValueError(f"band_names: expected {C}, got {len(names)}")
    row_bytes = 4 * W * (C if pixel else 1)
    rps = strip_rows(row_bytes, H) if rows_per_strip is None else int(rows_per_strip)
    if rps < 1:
        raise ValueError("rows_per_strip: at least one row")
    rps = min(rps, H)
    strips = []
    for plane in range(1 if pixel else C):                   # BAND: strips never straddle a band, offsets band-major
        for r in range(0, H, rps):
            a = (plane * H + r) * row_bytes
            raw = block[a:a + min(rps, H - r) * row_bytes].tobytes()
            strips.append(zlib.compress(raw, level) if comp == 8 else raw)
    n = len(strips)
    tags = [(256, 4, [W]), (257, 4, [H]), (258, 3, [32] * C), (259, 3, [comp]), (262, 3, [1]), (273, 4, None), (277, 3, [C]),
            (278, 4, [rps]), (279, 4, [len(s) for s in strips]), (284, 3, [1 if (pixel or C == 1) else 2])]
    if predictor == 3:
        tags.append((317, 3, [3]))
    if C > 1:
        tags.append((338, 3, [0] * (C - 1)))
    tags += [(339, 3, [3] * C), (33550, 12, [float(pix), float(pix), 0.0]),
             (33922, 12, [0.0, 0.0, 0.0, float(x_min), float(y_max), 0.0]),
             (34735, 3, [1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, int(epsg)]),
             (42112, 2, gdal_metadata(names, stats).encode("ascii", "xmlcharrefreplace") + b"\0"), (42113, 2, b"nan\0")]
    at = 8 + 2 + 12 * len(tags) + 4                          # the first byte after the IFD
    sized = []
    for tag, typ, values in tags:
        count = n if values is None else len(values)
        size = count * _SIZE[typ]
        off = None
        if size > 4:
            at += at & 1
            off = at
            at += size
        sized.append((tag, typ, values, count, off))
    at += at & 1
    total = at + sum(len(s) for s in strips)
    if total >= 2 ** 32:
        raise ValueError(f"a classic TIFF cannot address {total} bytes")
    offsets, o = [], at
    for s in strips:
        offsets.append(o)
        o += len(s)
    out = bytearray(at)
    out[0:8] = struct.pack("<2sHI", b"II", 42, 8)
    struct.pack_into("<H", out, 8, len(tags))
    for i, (tag, typ, values, count, off) in enumerate(sized):
        values = offsets if values is None else values
        data = bytes(values) if typ == 2 else struct.pack("<%d%s" % (count, _TYPE[typ]), *values)
        e = 10 + 12 * i
        struct.pack_into("<HHI", out, e, tag, typ, count)
        if off is None:
            out[e + 8:e + 8 + len(data)] = data
        else:
            struct.pack_into("<I", out, e + 8, off)
            out[off:off + len(data)] = data
    return bytes(out) + b"".join(strips)


def _write_packed(paths, packed, shapes, geos, pix, means, compress, predictor, interleave, band_names, epsg, level, rows_per_strip,
                  statistics):
    packed.read()
    done = []
    for k, path in enumerate(paths):
        block = packed.block(k)
        if block is None or path is None:
            done.append(None)
            continue
        (H, W), (x_min, y_max) = shapes[k], geos[k]
        stats = None
        if statistics:
            stats = band_statistics(packed.counts[k], packed.minimum[k], packed.maximum[k], H * W, None if means is None else means[k])
        data = assemble(block, packed.C, H, W, x_min, y_max, pix, interleave, predictor, compress, level, rows_per_strip, band_names,
                        epsg, stats)
        with open(path, "wb") as f:
            f.write(data)
        done.append(path)
    return done


def _predictor(predictor, compress):
    if compress not in COMPRESSION:
        raise ValueError(f"compress: expected 'deflate' or None, got {compress!r}")
    if predictor is None:
        predictor = 3 if COMPRESSION[compress] == 8 else 1
    if predictor not in (1, 3):
        raise ValueError(f"predictor: expected 1, 3 or None, got {predictor!r}")
    if predictor == 3 and COMPRESSION[compress] == 1:
        raise ValueError("predictor 3 without compression is refused: readers that bypass libtiff ignore the tag there")
    return predictor


def write_atlas(paths, atlas, report, origin=None, compress="deflate", predictor=None, interleave="band", band_names=None, epsg=2154,
                level=6, rows_per_strip=None, statistics=True):
    """One GeoTIFF per parcel of a `MosaicAtlas` report: K files from ONE launch and ONE device-to-host read.  paths: K entries, a
    path or None; an empty parcel or a None path writes nothing and gives None at that index.  origin = (x0, y0) is added in fp64
    to every tie point (canvases that live in a shifted frame land in Lambert-93).  predictor None: 3 with deflate, 1 without.
    -> the K paths written (None where none was)."""
    K = len(report)
    if len(paths) != K:
        raise ValueError(f"paths: expected one entry per parcel ({K}), got {len(paths)}")
    predictor = _predictor(predictor, compress)
    skip = [bool(report.empty[k]) or paths[k] is None for k in range(K)]
    x0, y0 = (0.0, 0.0) if origin is None else (float(origin[0]), float(origin[1]))
    with torch.cuda.device(report.band_arena.device):
        packed = pack(report.band_arena, report.n_bands, report.table, interleave, predictor, skip)
    geos = [(report.table.geo(k)[0] + x0, report.table.geo(k)[1] + y0) for k in range(K)]
    return _write_packed([None if skip[k] else paths[k] for k in range(K)], packed, [report.table.shape(k) for k in range(K)], geos,
                         atlas.pix, report.band_means, compress, predictor, interleave, band_names, epsg, level, rows_per_strip, statistics)


def write_bands(path, bands, x_min, y_max, pix, compress="deflate", predictor=None, interleave="band", band_names=None, epsg=2154,
                level=6, rows_per_strip=None, statistics=True, means=None):
    """(C,H,W) fp32 bands on the device -> one file: the K = 1 case through the same kernel."""
    if bands.dim() != 3 or bands.dtype != torch.float32:
        raise ValueError(f"bands: expected (C,H,W) fp32, got {tuple(bands.shape)} {bands.dtype}")
    predictor = _predictor(predictor, compress)
    C, H, W = bands.shape
    table = ops.AtlasTable([H], [W], [float(x_min)], [float(y_max)], device=bands.device)
    with torch.cuda.device(bands.device):
        packed = pack(bands.contiguous().view(-1), C, table, interleave, predictor)
    return _write_packed([path], packed, [(H, W)], [(float(x_min), float(y_max))], pix, None if means is None else [means], compress,
                         predictor, interleave, band_names, epsg, level, rows_per_strip, statistics)[0]


def write_parcel(path, mosaic, report, origin=None, **kw):
    """A `ParcelMosaic` and its `ParcelReport` -> one file (`write_bands` with the mosaic's geotransform and the report's means)."""
    x0, y0 = (0.0, 0.0) if origin is None else (float(origin[0]), float(origin[1]))
    return write_bands(path, report.bands, mosaic.x_min + x0, mosaic.y_max + y0, mosaic.pix, means=report.band_means, **kw)


# ---- reading back ------------------------------------------------------------------------------------------------------------
def unpredict_rows(rows: np.ndarray, stride: int) -> np.ndarray:
    """(n, 4 wc) uint8 rows under predictor 3 -> the rows' fp32 bytes: running sums mod 256 at `stride`, then the planes woven."""
    n, rb = rows.shape
    wc = rb // 4
    t = rows.copy()
    for s in range(stride):
        t[:, s::stride] = np.cumsum(t[:, s::stride], axis=1, dtype=np.uint64).astype(np.uint8)
    return np.ascontiguousarray(t.reshape(n, 4, wc)[:, ::-1, :].transpose(0, 2, 1)).reshape(n, rb)


def read(path):
    """A minimal reader of what this module writes: classic little-endian TIFF, strips, float32, compression 1 / 8, predictor 1 / 3,
    planar configuration 1 / 2.  -> dict: bands (C,H,W) fp32, geotransform [x_min, pix, 0, y_max, 0, -pix], epsg, nodata, band_names,
    statistics (per band a dict of the STATISTICS_* strings), tags {tag: tuple or bytes}."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"II*\0":
        raise ValueError(f"{path}: not a classic little-endian TIFF")
    ifd, = struct.unpack_from("<I", data, 4)
    n, = struct.unpack_from("<H", data, ifd)
    tags = {}
    for i in range(n):
        e = ifd + 2 + 12 * i
        tag, typ, count = struct.unpack_from("<HHI", data, e)
        if typ not in _SIZE:
            continue
        size = count * _SIZE[typ]
        off = e + 8 if size <= 4 else struct.unpack_from("<I", data, e + 8)[0]
        tags[tag] = data[off:off + size] if typ == 2 else struct.unpack_from("<%d%s" % (count, _TYPE[typ]), data, off)
    W, H, C = tags[256][0], tags[257][0], tags.get(277, (1,))[0]
    comp, planar, predictor = tags.get(259, (1,))[0], tags.get(284, (1,))[0], tags.get(317, (1,))[0]
    if set(tags[258]) != {32} or set(tags.get(339, (1,))) != {3} or comp not in (1, 8) or predictor not in (1, 3) or 322 in tags:
        raise ValueError(f"{path}: only float32 strips, compression 1 / 8 and predictor 1 / 3 are read")
    pixel = planar == 1
    wc = W * C if pixel else W
    rps = min(tags.get(278, (H,))[0], H)
    parts = []
    for off, cnt in zip(tags[273], tags[279]):
        raw = data[off:off + cnt]
        parts.append(zlib.decompress(raw) if comp == 8 else raw)
    rows = np.frombuffer(b"".join(parts), dtype=np.uint8)
    want = 4 * C * H * W
    if rows.size != want or len(parts) != (1 if pixel else C) * -(-H // rps):
        raise ValueError(f"{path}: {rows.size} bytes in {len(parts)} strips for {C}x{H}x{W} float32")
    rows = rows.reshape(-1, 4 * wc)
    if predictor == 3:
        rows = unpredict_rows(rows, C if pixel else 1)
    fl = np.ascontiguousarray(rows).view("<f4")
    bands = np.ascontiguousarray(fl.reshape(H, W, C).transpose(2, 0, 1)) if pixel else fl.reshape(C, H, W).copy()
    geo = None
    if 33550 in tags and 33922 in tags:
        sx, sy = tags[33550][0], tags[33550][1]
        i, j, _, x, y, _ = tags[33922][:6]
        geo = [x - i * sx, sx, 0.0, y + j * sy, 0.0, -sy]
    epsg = None
    keys = tags.get(34735)
    if keys:
        for a in range(4, 4 + 4 * keys[3], 4):
            if keys[a] == 3072 and keys[a + 1] == 0:
                epsg = keys[a + 3]
    nodata = float(tags[42113].rstrip(b"\0").decode("ascii")) if 42113 in tags else None
    names, stats = [None] * C, [dict() for _ in range(C)]
    if 42112 in tags:
        text = tags[42112].rstrip(b"\0").decode("ascii")
        for m in re.finditer(r'<Item name="([^"]+)" sample="(\d+)"(?: role="([^"]+)")?>([^<]*)</Item>', text):
            key, c, role, value = m.group(1), int(m.group(2)), m.group(3), m.group(4)
            value = value.replace("&lt;", "<").replace("&gt;", ">").replace("&amp;", "&")
            if c < C:
                if role == "description":
                    names[c] = value
                else:
                    stats[c][key] = value
    return {"bands": bands, "geotransform": geo, "epsg": epsg, "nodata": nodata, "band_names": names, "statistics": stats, "tags": tags}


def parcel_predicted_values(path: Optional[str]) -> dict:
    """`get_parcel_predicted_values` (inference/predict_utils.py:124-146): the four PRED_* shapefile fields, the means over the
    pixels that are not NaN of bands 0, 1, 2 and 4 of the file's first five bands (in fp64; the reference's `np.nanmean` sums in
    fp32); -1 each for None.  A band without a pixel gives NaN, as `nanmean` does."""
    if path is None:
        return {name: -1 for name, _ in SHP_FIELDS}
    bands = read(path)["bands"][:5].astype(np.float64)
    if bands.shape[0] < 5:
        raise ValueError(f"{path}: {bands.shape[0]} bands, the fields need five")
    valid = ~np.isnan(bands)
    sums, counts = np.where(valid, bands, 0.0).sum(axis=(1, 2)), valid.sum(axis=(1, 2))
    means = np.where(counts > 0, sums / np.maximum(counts, 1), np.nan)
    return {name: float(means[b]) for name, b in SHP_FIELDS}
