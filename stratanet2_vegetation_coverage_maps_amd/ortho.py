"""Colours for LiDAR points from georeferenced orthoimages, looked up on the device (csrc/ortho.hip; include/strata_hip.h,
"Orthoimage colours").

    rgb = ortho.OrthoSet([ortho.open(p) for p in rgb_slabs], nodata=0)      # or OrthoImage(pixels, x_min, y_max, pix) directly
    irc = ortho.OrthoSet([ortho.open(p) for p in irc_slabs], nodata=0)
    cloud = las.load_las(path)                                               # format 0, 1 or 6: rows 3..6 are zero
    ortho.colorize(cloud, rgb)                                               # rows 3, 4, 5 in place
    res = ortho.colorize(cloud, irc, bands=(0,), rows=(6,))                  # row 6; int(res.missing): points no image served
    cloud = ortho.load_las_colorized(path, rgb, irc)                         # the three calls in one

LiDAR as it is delivered carries no colour; the eight-feature network reads `red, green, blue, near_infrared` from rows 3..6 of
the (10,T) cloud.  The reference's files had them painted on upstream by tools that are not part of it, so the rule here is OURS
(stated once in csrc/ortho_rules.h, restated in numpy by `colorize_ref`): the pixel whose area holds the point, the first image
of the list that covers the point with a pixel that is not nodata, value = (float)sample * scale.  Two choices are UNPINNED
against GDAL or pdal: a point exactly on a pixel edge goes east / south, and the default `scale` (256 for 8-bit images: the
16-bit range that the loader divides by 65 536; 1 for 16-bit images).

An image is north up, without rotation: (x_min, y_max) is the OUTER corner of its top-left pixel, as in `geotiff.write_bands` and
a GDAL geotransform.  A cloud in a shifted frame (origin= of `las.load_las`, `parcel.cut_parcels`) takes the same shift in metres:
`colorize(..., origin=(dx, dy))` subtracts it from the images' corners in fp64 on the host.
"""
import builtins
import math
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from . import hip_ops as ops

DTYPES = ("uint8", "uint16", "float32")
LAYOUTS = ("chunky", "planar")
MAX_IMAGES = _lib.SN2_ORTHO_MAX_IMAGES
DEFAULT_SCALE = {"uint8": 256.0, "uint16": 1.0}
WORLD_FILE_SUFFIXES = (".tfw", ".j2w", ".wld")


def _dtype_name(pixels) -> str:
    return str(pixels.dtype).split(".")[-1]


class OrthoImage:
    """One orthoimage: `pixels` (H,W,C) for layout "chunky", (C,H,W) for "planar", or (H,W) for one band -- a device tensor or
    a numpy array, uint8, uint16 or float32, contiguous.  (x_min, y_max): the outer corner of the top-left pixel; pix_x, pix_y > 0
    the pixel sizes in metres (pix_y None = pix_x)."""

    def __init__(self, pixels, x_min, y_max, pix_x, pix_y=None, layout="chunky"):
        if layout not in LAYOUTS:
            raise ValueError(f"layout: expected one of {LAYOUTS}, got {layout!r}")
        if not isinstance(pixels, torch.Tensor):
            pixels = np.ascontiguousarray(pixels)
        elif not pixels.is_contiguous():
            raise ValueError("pixels: the tensor must be contiguous")
        name = _dtype_name(pixels)
        if name not in DTYPES:
            raise ValueError(f"pixels: expected one of {DTYPES}, got {name}")
        shape = tuple(int(n) for n in pixels.shape)
        if len(shape) == 2:
            H, W, C = shape[0], shape[1], 1
        elif len(shape) == 3:
            (H, W, C) = shape if layout == "chunky" else (shape[1], shape[2], shape[0])
        else:
            raise ValueError(f"pixels: expected (H,W), (H,W,C) or (C,H,W), got {shape}")
        if min(H, W, C) < 1:
            raise ValueError(f"pixels: an empty image {shape}")
        if H >= 2 ** 31 or W >= 2 ** 31 or H * W * C >= _lib.SN2_ORTHO_MAX_SAMPLES:
            raise ValueError(f"pixels: {shape} is beyond the {_lib.SN2_ORTHO_MAX_SAMPLES} samples of one image")
        pix_y = pix_x if pix_y is None else pix_y
        geo = tuple(float(v) for v in (x_min, y_max, pix_x, pix_y))
        if not all(math.isfinite(v) for v in geo) or not (geo[2] > 0 and geo[3] > 0):
            raise ValueError(f"georeference: x_min, y_max finite and pix_x, pix_y finite and > 0, got {geo}")
        self.pixels, self.dtype, self.layout = pixels, name, layout
        self.H, self.W, self.C = H, W, C
        self.x_min, self.y_max, self.pix_x, self.pix_y = geo
        self._dev = {}

    def shifted(self, shift) -> "OrthoImage":
        """the same pixels (not copied) in a frame moved by (dx, dy) metres: corner - shift, in fp64"""
        out = OrthoImage.__new__(OrthoImage)
        out.__dict__.update(self.__dict__)
        out.x_min, out.y_max = float(np.float64(self.x_min) - np.float64(shift[0])), float(np.float64(self.y_max) - np.float64(shift[1]))
        return out

    def host(self) -> np.ndarray:
        """the pixels as a numpy array (H,W,C) or (C,H,W)"""
        p = self.pixels
        if isinstance(p, torch.Tensor):
            p = p.detach().cpu().reshape(-1).view(torch.uint8).numpy().view(np.dtype(self.dtype))
        return p.reshape((self.H, self.W, self.C) if self.layout == "chunky" else (self.C, self.H, self.W))

    def device_bytes(self, device) -> torch.Tensor:
        """the pixels' bytes on `device` (uploaded once per device and kept; a tensor that is there already is viewed)"""
        device = torch.device(device)
        key = (device.type, device.index)
        if key not in self._dev:
            p = self.pixels
            if isinstance(p, torch.Tensor):
                t = p.detach().reshape(-1).view(torch.uint8)
                t = t if t.device == device else t.to(device)
            else:
                t = torch.from_numpy(p.reshape(-1).view(np.uint8)).to(device)
            self._dev[key] = t
        return self._dev[key]


class OrthoSet:
    """Up to 32 images with one pixel type, band count and layout, tried in list order.  nodata: a pixel all of whose SAMPLED
    bands equal it serves no point (None: every pixel serves)."""

    def __init__(self, images, nodata=None):
        images = list(images)
        if not 1 <= len(images) <= MAX_IMAGES:
            raise ValueError(f"OrthoSet: 1 to {MAX_IMAGES} images, got {len(images)}")
        for im in images:
            if not isinstance(im, OrthoImage):
                raise ValueError("OrthoSet: expected OrthoImage objects")
            if (im.dtype, im.C, im.layout) != (images[0].dtype, images[0].C, images[0].layout):
                raise ValueError(f"OrthoSet: one pixel type, band count and layout for all images, got {(im.dtype, im.C, im.layout)} "
                                 f"beside {(images[0].dtype, images[0].C, images[0].layout)}")
        if nodata is not None and math.isnan(float(nodata)):
            raise ValueError("OrthoSet: nodata must not be NaN (a NaN equals nothing)")
        self.images, self.nodata = images, None if nodata is None else float(nodata)
        self.dtype, self.C, self.layout = images[0].dtype, images[0].C, images[0].layout

    def shifted(self, shift) -> "OrthoSet":
        """the set in a frame moved by (dx, dy) metres (a third component is ignored); the pixels are shared"""
        return OrthoSet([im.shifted(shift) for im in self.images], self.nodata)

    def mapping(self, bands, rows, scale):
        """the checked (bands, rows, scale) of a call"""
        bands, rows = tuple(int(b) for b in bands), tuple(int(r) for r in rows)
        if scale is None:
            if self.dtype not in DEFAULT_SCALE:
                raise ValueError("scale: a float32 image has no default scale, give one")
            scale = DEFAULT_SCALE[self.dtype]
        ops.ortho_check_mapping(self.C, bands, rows, scale)
        return bands, rows, float(scale)

    def struct(self, device, bands, rows, scale) -> "_lib.OrthoSet":
        entries = [(im.device_bytes(device).data_ptr(), im.x_min, im.y_max, im.pix_x, im.pix_y, im.W, im.H) for im in self.images]
        return ops.ortho_set_struct(entries, self.dtype, self.C, self.layout, bands, rows, scale, self.nodata)


@dataclass
class ColorizeResult:
    cloud: object                      # what was passed in, coloured in place (colorize_ref: the coloured copy)
    missing: object                    # points no image served: a device int64 scalar until int() reads it (colorize_ref: int)
    covered: Optional[object] = None   # (T) uint8: 1-based index of the serving image, 0 = missing


def _as_set(ortho, origin) -> OrthoSet:
    if isinstance(ortho, OrthoImage):
        ortho = OrthoSet([ortho])
    if not isinstance(ortho, OrthoSet):
        raise ValueError("ortho: expected an OrthoSet or an OrthoImage")
    if origin is not None:
        if len(origin) < 2:
            raise ValueError("origin: (dx, dy) in metres")
        ortho = ortho.shifted((float(origin[0]), float(origin[1])))
    return ortho


def colorize(cloud, ortho, bands=(0, 1, 2), rows=(3, 4, 5), scale=None, origin=None, covered=False) -> ColorizeResult:
    """Rows `rows` of the cloud := bands `bands` of the images * scale, in place, in ONE launch.  cloud: a (10,T) fp32 device
    tensor (unit stride along T; a column view of a larger arena is fine) or a `parcel.ParcelClouds`, whose arena is coloured for
    all K parcels at once.  origin: the cloud's shift (dx, dy) in metres.  covered=True also returns the serving image per point.
    `missing` stays on the device: no read is forced."""
    from .parcel import ParcelClouds
    arena = cloud.arena if isinstance(cloud, ParcelClouds) else cloud
    oset = _as_set(ortho, origin)
    bands, rows, scale = oset.mapping(bands, rows, scale)
    if not isinstance(arena, torch.Tensor) or not arena.is_cuda:
        raise ValueError("cloud: expected a (10,T) fp32 tensor on the HIP device or a ParcelClouds")
    dev = arena.device
    with torch.cuda.device(dev):
        st = oset.struct(dev, bands, rows, scale)
        missing = torch.zeros(1, dtype=torch.int64, device=dev)
        cov = torch.empty(arena.shape[1] if arena.dim() == 2 else 0, dtype=torch.uint8, device=dev) if covered else None
        ops.ortho_colorize(arena, st, covered=cov, missing=missing)
    return ColorizeResult(cloud, missing.reshape(()), cov)


def colorize_ref(cloud, ortho, bands=(0, 1, 2), rows=(3, 4, 5), scale=None, origin=None, covered=False) -> ColorizeResult:
    """The rule in numpy, on host arrays: cloud (10,T) fp32 -> a coloured COPY, `missing` as an int, `covered` (T) uint8.  What
    the kernel gives bit for bit."""
    oset = _as_set(ortho, origin)
    bands, rows, scale = oset.mapping(bands, rows, scale)
    out = np.array(cloud, dtype=np.float32, copy=True)
    if out.ndim != 2 or out.shape[0] != 10:
        raise ValueError(f"cloud: expected (10,T), got {out.shape}")
    T = out.shape[1]
    x, y = out[0].astype(np.float64), out[1].astype(np.float64)
    open_ = np.ones(T, dtype=bool)
    cov = np.zeros(T, dtype=np.uint8)
    for s, im in enumerate(oset.images):
        with np.errstate(invalid="ignore", over="ignore"):
            u = (x - np.float64(im.x_min)) / np.float64(im.pix_x)
            v = (np.float64(im.y_max) - y) / np.float64(im.pix_y)
            inside = open_ & (u >= 0.0) & (u < np.float64(im.W)) & (v >= 0.0) & (v < np.float64(im.H))
        idx = np.nonzero(inside)[0]
        if len(idx) == 0:
            continue
        col, row = np.floor(u[idx]).astype(np.int64), np.floor(v[idx]).astype(np.int64)
        px = im.host()
        samples = [px[row, col, b] if im.layout == "chunky" else px[b, row, col] for b in bands]
        nodata = np.zeros(len(idx), dtype=bool)
        if oset.nodata is not None:
            nodata = np.logical_and.reduce([q.astype(np.float64) == np.float64(oset.nodata) for q in samples])
        j = idx[~nodata]
        for r, q in zip(rows, samples):
            out[r, j] = q[~nodata].astype(np.float32) * np.float32(scale)
        cov[j] = s + 1
        open_[j] = False
    return ColorizeResult(out, int(open_.sum()), cov if covered else None)


# ---- files -------------------------------------------------------------------------------------------------------------------------
def _north_up(a, b, d, e, what):
    """pixel sizes of the affine terms x = a col + b row + c, y = d col + e row + f: (pix_x, pix_y), or ValueError"""
    if b != 0.0 or d != 0.0:
        raise ValueError(f"{what}: a rotated or sheared georeference is not supported")
    if not (a > 0.0 and e < 0.0):
        raise ValueError(f"{what}: expected a north-up image (pixel width > 0, pixel height < 0), got {a}, {e}")
    return float(a), float(-e)


def _georef_tags(img, path):
    """(x_min, y_max, pix_x, pix_y) from the GeoTIFF tags of a PIL image, or None where it carries none"""
    tags = getattr(img, "tag_v2", None)
    if tags is None:
        return None
    scale, tie, matrix, keys = tags.get(33550), tags.get(33922), tags.get(34264), tags.get(34735)
    half = 0.0
    if keys is not None:                                     # GeoKeyDirectory: a header of four shorts, then (key, location, count, value)
        keys = tuple(keys)
        for k in range(4, len(keys) - 3, 4):
            if keys[k] == 1025 and keys[k + 1] == 0 and keys[k + 3] == 2:        # GTRasterTypeGeoKey = RasterPixelIsPoint
                half = 0.5
    if scale is not None and tie is not None:
        scale, tie = tuple(float(v) for v in scale), tuple(float(v) for v in tie)
        if len(scale) < 2 or len(tie) != 6:
            raise ValueError(f"{path}: expected one tie point and a pixel scale in the GeoTIFF tags")
        px, py = _north_up(scale[0], 0.0, 0.0, -scale[1], path)
        return tie[3] - (tie[0] + half) * px, tie[4] + (tie[1] + half) * py, px, py
    if matrix is not None:                                   # how a GeoTIFF states a rotated or sheared raster
        raise ValueError(f"{path}: a georeference given as a ModelTransformation matrix (rotated or sheared rasters) is not supported")
    return None


def _georef_world_file(path):
    """(x_min, y_max, pix_x, pix_y) from the world file beside `path` (six numbers: a, d, b, e, then x and y of the CENTRE of the
    top-left pixel), or None where there is none"""
    stem = os.path.splitext(path)[0]
    for suffix in WORLD_FILE_SUFFIXES:
        for name in (stem + suffix, stem + suffix.upper()):
            if os.path.exists(name):
                with builtins.open(name) as f:
                    v = [float(t.replace(",", ".")) for t in f.read().split()]
                if len(v) != 6:
                    raise ValueError(f"{name}: a world file holds six numbers, got {len(v)}")
                a, d, b, e, cx, cy = v
                px, py = _north_up(a, b, d, e, name)
                return cx - 0.5 * px, cy + 0.5 * py, px, py
    return None


def open(path, georef=None) -> OrthoImage:  # noqa: A001 (ortho.open, as in PIL.Image.open)
    """An image file -> OrthoImage on the host, chunky.  The pixels come through PIL (imported here: the rest of the module does
    not need it).  The georeference is, in this order: `georef` = (x_min, y_max, pix_x, pix_y); the GeoTIFF tags 33550 / 33922
    (a PixelIsPoint raster type moves the corner by half a pixel); a world file beside the image (.tfw, .j2w, .wld).
    A rotated or sheared georeference, or none at all, raises ValueError."""
    from PIL import Image
    path = os.fspath(path)
    with Image.open(path) as img:
        geo = tuple(georef) if georef is not None else _georef_tags(img, path)
        mode = img.mode
        if mode in ("L", "RGB", "RGBA", "F") or mode.startswith("I;16"):
            pixels = np.asarray(img)
        elif mode == "I":
            wide = np.asarray(img)
            if wide.size and (wide.min() < 0 or wide.max() > 65535):
                raise ValueError(f"{path}: 32-bit integer samples outside 0..65535")
            pixels = wide.astype(np.uint16)
        else:
            raise ValueError(f"{path}: image mode {mode!r} is not supported (8-bit grey, RGB, RGBA, 16-bit grey, float32)")
    if geo is None:
        geo = _georef_world_file(path)
    if geo is None:
        raise ValueError(f"{path}: no georeference: no GeoTIFF tags, no world file {WORLD_FILE_SUFFIXES}, no georef=")
    if len(geo) != 4:
        raise ValueError("georef: (x_min, y_max, pix_x, pix_y)")
    if pixels.dtype.kind == "u" and pixels.dtype.itemsize == 2:
        pixels = pixels.astype(np.uint16)                    # native byte order
    elif pixels.dtype.kind == "f":
        pixels = pixels.astype(np.float32)
    return OrthoImage(np.ascontiguousarray(pixels), geo[0], geo[1], geo[2], geo[3], layout="chunky")


def load_las_colorized(path, rgb=None, irc=None, **load_las_kwargs):
    """`las.load_las(path, **kw)`, then `colorize(cloud, rgb)` into rows 3, 4, 5 and `colorize(cloud, irc, bands=(0,), rows=(6,))`,
    in the cloud's frame: the origin of the "header" mode is in metres, that of the "reference" mode raw units / 100.  rgb, irc:
    an OrthoSet / OrthoImage or None.  -> what load_las returns."""
    from . import las
    res = las.load_las(path, **load_las_kwargs)
    cloud = res[0] if isinstance(res, tuple) else res
    o = load_las_kwargs.get("origin")
    shift = None
    if o is not None:
        shift = (float(o[0]), float(o[1])) if load_las_kwargs.get("coords", "reference") == "header" else (int(o[0]) / 100, int(o[1]) / 100)
    if rgb is not None:
        colorize(cloud, rgb, origin=shift)
    if irc is not None:
        colorize(cloud, irc, bands=(0,), rows=(6,), origin=shift)
    return res
