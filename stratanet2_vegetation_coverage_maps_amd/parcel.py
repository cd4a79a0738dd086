"""A parcel point cloud -> its prepared plots on the device -> the parcel mosaic: the counterpart of the reference's
`prepare.py` (`inference/prepare_utils.py:95-173`: plot centres, `extract_cloud_data`: discs and `pre_transform`) followed
by `predict.py`, without the GIS file I/O.

    plots = prepare_parcel(cloud, args, keep=polygon_keep([exterior, *holes], shape_buffer(args)))
    for batch in plots.batches(args, 20): ...           # the dicts `inference.predict_parcel` takes
    mosaic, plots = predict_parcel_cloud(model, cloud, args, shape=[exterior, *holes])
    report = mosaic.report([exterior, *holes])          # bands cropped to the polygon, PRED_BASSE / PRED_INTER / PRED_HAUTE
    plots = prepare_parcels(clouds, args, shapes=shapes) # K parcels in one pass over a cloud arena (ParcelClouds, csrc/parcels.hip)

Rules kept from the reference (the centres in `parcel_plot_centers`, the discs and the z-normalisation in
csrc/parcel.hip):
  - plot centres on a lattice of step 2 cos(pi/4) 10 - 20/diam_pix metres from the fp32 bounding box, the first centre
    listed twice, centres kept by the parcel shape buffered by 20 + diam_meters//2, then cast to fp32;
  - a plot is every point with fp64 dx*dx + dy*dy <= (diam_meters//2)^2 from its centre (scipy's inclusive test), and it is
    kept iff it has at least 51 points (`< 50` gives None, prepare.py keeps `> 50`);
  - z of a plot point = z - the least z of the PLOT's points within znorm_radius_in_meters (1.5 m, inclusive).
Where it differs: a plot's points are in ascending parcel index (the reference returns kd-tree order; the order only
decides which points a random subsample picks); `polygon_keep` restates shapely's buffer test with exact round joins
(see there).
"""
import math
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from . import hip_ops as ops
from .inference import MosaicAtlas, ParcelMosaic, PointScores, predict_batches, predict_parcel
from .input_pipeline import check_sampler, draw_plot_randoms, draw_seed, fake_ground_xy, live_counts

MIN_POINTS = 51              # prepare_utils.py:67-69 (< 50: None) and prepare.py:93 (> 50)
LAS_PARCEL_BUFFER = 20       # prepare_utils.py:148
INT_MIN = -(2 ** 31)
ROW_POINTS = 2048            # points per wave of the count / fill passes
MAX_TABLE = 1 << 26          # (plot, row) entries of the count table before rows get longer


def plot_movement(args) -> float:
    """Lattice step (prepare_utils.py:115-128): 2 cos(45 deg) 10 - 20 / diam_pix (13.1421 m at diam_pix = 20)."""
    return 2 * math.cos(math.pi / 4) * 10 - 1 * 20 / args.diam_pix


def shape_buffer(args) -> int:
    """The buffer of the parcel shape a centre must lie in (prepare_utils.py:148-151): 20 + diam_meters // 2."""
    return LAS_PARCEL_BUFFER + args.diam_meters // 2


def parcel_plot_centers(x_min, x_max, y_min, y_max, args, keep=None) -> np.ndarray:
    """Plot centres of `divide_parcel_las_and_get_disk_centers` (prepare_utils.py:95-173) -> (P,2) float32.

    x_min..y_max: the fp32 bounding box of the parcel (`get_xy_range`).  Dtypes as under the reference's numpy 1.x:
    the extents are fp32 differences, nx = ceil(extent / movement) + 1 divides in fp64, and every lattice coordinate is
    fp64 (an np.float32 scalar plus a python float is fp64 there).  Centres run x outer, y inner, after a first centre
    equal to the lattice's first.  keep: None (all), or a callable taking the fp64 lattice (n,2) and returning a bool mask
    (`polygon_keep`, or shapely's `shape.buffer(b).contains` where it is installed).  The survivors are cast to fp32."""
    f32 = np.float32
    x_min, x_max, y_min, y_max = f32(x_min), f32(x_max), f32(y_min), f32(y_max)
    mv = plot_movement(args)
    nx = math.ceil(float(f32(x_max - x_min)) / mv) + 1
    ny = math.ceil(float(f32(y_max - y_min)) / mv) + 1
    sx, sy = float(x_min) + mv / 4, float(y_min) + mv / 4
    xs = sx + np.arange(nx, dtype=np.float64) * mv
    ys = sy + np.arange(ny, dtype=np.float64) * mv
    lattice = np.empty((1 + nx * ny, 2), dtype=np.float64)
    lattice[0] = (sx, sy)
    lattice[1:, 0] = np.repeat(xs, ny)
    lattice[1:, 1] = np.tile(ys, nx)
    if keep is not None:
        mask = np.asarray(keep(lattice), dtype=bool).reshape(-1)
        if mask.shape[0] != lattice.shape[0]:
            raise ValueError("keep must return one bool per lattice point")
        lattice = lattice[mask]
    return lattice.astype(np.float32)


def polygon_edges(rings) -> np.ndarray:
    """The rings of a polygon -- [exterior, *holes], and those of every further part of a multi-part polygon --, each a (V,2)
    array, closed (last vertex = first) or not -> (E,4) float64 = (ax, ay, bx, by): every ring edge, the closing one included, in
    ring order.  What `polygon_keep` tests and `hip_ops.mosaic_crop_stats` takes."""
    segs = []
    for r in rings:
        r = np.asarray(r, dtype=np.float64).reshape(-1, 2)
        if len(r) > 1 and np.array_equal(r[0], r[-1]):
            r = r[:-1]
        if len(r) < 2:
            raise ValueError("a ring needs at least two vertices")
        segs.append(np.concatenate([r, np.roll(r, -1, axis=0)], 1))
    return np.ascontiguousarray(np.concatenate(segs, 0))


def polygon_keep(rings, buffer_m: float):
    """Host restatement of `shape.buffer(buffer_m).contains(Point(x, y))` for a polygon: rings = [exterior, *holes], each
    a (V,2) array (closed or not).  A point is kept iff it is inside by the even-odd rule or its distance to the boundary
    is < buffer_m (`contains` excludes the buffer's own boundary).

    Deviation: shapely draws the round joins of a buffer with 16 segments per quarter circle, inside the true circle, so a
    point within about 4 cm of the offset curve near a convex vertex (at a 30 m buffer) may be classed differently here."""
    seg = polygon_edges(rings)
    ax, ay, bx, by = (seg[:, k][None, :] for k in range(4))
    dx, dy = bx - ax, by - ay
    l2 = dx * dx + dy * dy
    b2 = float(buffer_m) * float(buffer_m)

    def keep(pts):
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
        out = np.empty(len(pts), dtype=bool)
        for s in range(0, len(pts), 2048):
            px, py = pts[s:s + 2048, :1], pts[s:s + 2048, 1:]
            with np.errstate(divide="ignore", invalid="ignore"):
                crosses = (ay > py) != (by > py)
                xint = ax + (py - ay) * dx / dy
                inside = np.count_nonzero(crosses & (px < xint), axis=1) % 2 == 1
                t = np.where(l2 > 0, ((px - ax) * dx + (py - ay) * dy) / l2, 0.0)
            t = np.clip(t, 0.0, 1.0)
            ex, ey = ax + t * dx - px, ay + t * dy - py
            out[s:s + 2048] = inside | ((ex * ex + ey * ey).min(axis=1) < b2)
        return out
    return keep


def plot_id(plot_idx: int, center) -> str:
    """`define_plot_id(define_a_plot_name(plot_idx), center)` (prepare_utils.py:84-92)."""
    return f"PP{str(int(plot_idx)).zfill(8)}_X{int(center[0])}_Y{int(center[1])}"


def center_grid(centers: np.ndarray, radius: float, bbox):
    """CSR of the centres that can reach the parcel's bounding box over square cells of side >= radius (host side of
    csrc/parcel.hip): (cell_start (GX*GY+1), cell_items, GX, GY, gx0, gy0, cell_inv), or None when no centre is within
    reach.  Cells grow beyond radius for very wide centre sets (at most 2048 per side)."""
    c = centers.astype(np.float64)
    x_min, y_min, x_max, y_max = (float(v) for v in bbox)
    reach = float(radius) + 1.0
    ids = np.nonzero((c[:, 0] >= x_min - reach) & (c[:, 0] <= x_max + reach) &
                     (c[:, 1] >= y_min - reach) & (c[:, 1] <= y_max + reach))[0]
    if len(ids) == 0:
        return None
    cx, cy = c[ids, 0], c[ids, 1]
    gx0, gy0 = float(cx.min()), float(cy.min())
    side = max(float(radius) * 1.001, max(float(cx.max()) - gx0, float(cy.max()) - gy0) / 2048)
    inv = 1.0 / side
    ix = np.floor((cx - gx0) * inv).astype(np.int64)          # the kernels' floor((v - g0) * inv), in fp64
    iy = np.floor((cy - gy0) * inv).astype(np.int64)
    GX, GY = int(ix.max()) + 1, int(iy.max()) + 1
    cell = iy * GX + ix
    order = np.lexsort((ids, cell))                            # by cell, ascending centre id inside a cell
    start = np.zeros(GX * GY + 1, dtype=np.int64)
    np.cumsum(np.bincount(cell, minlength=GX * GY), out=start[1:])
    return start.astype(np.int32), ids[order].astype(np.int32), GX, GY, gx0, gy0, inv


@dataclass
class ParcelPlots:
    """The kept plots of a parcel, ragged and device resident: raw (10,ΣN) fp32 (z row normalised per plot, the other rows
    the parcel's values), offsets (P+1) int32, point_index (ΣN) int32 (columns of the parcel), centers (P,2) fp32.  On the
    host: n_points (P), plot_index (P) (the plot's index in the list of centres), plot_ids, centers_host (P,2) fp32."""
    raw: torch.Tensor
    offsets: torch.Tensor
    point_index: torch.Tensor
    centers: torch.Tensor
    n_points: np.ndarray
    plot_index: np.ndarray
    plot_ids: List[str]
    centers_host: np.ndarray

    def __len__(self):
        return len(self.n_points)

    def batches(self, args, batch_size: int, rs=np.random, fps_start: Optional[int] = None, sampler="numpy", seed=None,
                n_live: bool = True, key_base: int = 0, with_samples: bool = False):
        """The input dicts of `inference.predict_parcel` ("cloud", "xyz", "plot_center", "n_live"), built on the device from raw /
        offsets by `sn2_prepare_plots` in eval mode.  Random draws: `draw_plot_randoms` per plot in plot order, so the
        batches equal `input_pipeline.prepare_batch(plots, centers, args, train=False, rs=rs)` on the same plots and seed.
        fps_start: None (the model draws the FPS starts) or one start index for every plot.
        sampler="device": the subsamples come from `hip_ops.subsample` instead (no host loop over plots, no index table
        copied per batch), keyed by `seed` (None: one 64-bit seed from `rs`, drawn when the first batch is asked for) and
        the plot's position in this ParcelPlots, so a plot's points do not depend on `batch_size`.
        "n_live" (B) int32 = `input_pipeline.live_counts`: with either sampler a plot of fewer than subsample_size candidates is
        its candidates in order, then repeats (a sparse parcel: half of its plots); the FPS kernels skip the repeats.  n_live=False
        leaves the key out (same predictions; a cross-check and a timing comparison).
        key_base: the device sampler's key of plot i is key_base + i (`plot_keys`); a parcel run with key_base = k << 32 draws
        the points it draws as parcel k of a `ParcelSet`.
        with_samples=True: every dict also says where its samples came from -- what `inference.PointScores.add` scatters the
        pointwise outputs back by: "sample_index" (B,N) int32 (the subsample it was gathered with), "sample_live" (B) int32
        (`live_counts`, whatever `n_live` says), "plot_range" (b0, b1) the batch's plots, "point_offsets" (B+1) int32 their
        positions in "point_index" (this object's, not copied), "diam_meters", and for a `ParcelSet` "col_base" (B) int32, the
        first arena column of each plot's parcel.  False: the dicts are exactly the ones above."""
        check_sampler(sampler)                       # here, not in the generator: a bad argument fails at the call
        if sampler == "numpy" and seed is not None:
            raise ValueError("seed belongs to sampler='device'")
        return self._batches(args, batch_size, rs, fps_start, sampler, seed, n_live, int(key_base), bool(with_samples))

    def plot_keys(self, key_base: int = 0) -> np.ndarray:
        """(P) int64: the Philox key of every plot for `hip_ops.subsample` = key_base + the plot's position."""
        return int(key_base) + np.arange(len(self), dtype=np.int64)

    def _batches(self, args, batch_size, rs, fps_start, sampler, seed, with_live=True, key_base=0, with_samples=False):
        dev = self.raw.device
        fake = fake_ground_xy(args.diam_meters)
        fake_dev = torch.from_numpy(fake).to(dev)
        N = args.subsample_size
        n_live = torch.from_numpy(live_counts(self.n_points, len(fake), N)).to(dev)
        if sampler == "device":
            seed = draw_seed(rs) if seed is None else int(seed)
            keys = torch.from_numpy(self.plot_keys(key_base)).to(dev)
        for b0 in range(0, len(self), batch_size):
            b1 = min(len(self), b0 + batch_size)
            if sampler == "device":
                with torch.cuda.device(dev):
                    idx = ops.subsample(self.offsets[b0:b1 + 1], len(fake), N, seed, keys[b0:b1],
                                        n_max=int(self.n_points[b0:b1].max()) + len(fake))
            else:
                draws = [draw_plot_randoms(int(n) + len(fake), N, False, rs, False) for n in self.n_points[b0:b1]]
                idx = torch.from_numpy(np.stack([d["idx"] for d in draws])).to(dev)
            with torch.cuda.device(dev):
                cloud, xyz = ops.prepare_plots(self.raw, self.offsets[b0:b1 + 1], self.centers[b0:b1], fake_dev, idx, args.z_max)
            d = {"cloud": cloud, "xyz": xyz, "plot_center": self.centers_host[b0:b1]}
            if with_live:
                d["n_live"] = n_live[b0:b1]
            if fps_start is not None:
                d["fps_start"] = torch.full((2, b1 - b0), int(fps_start), dtype=torch.int64)
            if with_samples:
                d.update(sample_index=idx, sample_live=n_live[b0:b1], plot_range=(b0, b1), point_offsets=self.offsets[b0:b1 + 1],
                         point_index=self.point_index, diam_meters=float(args.diam_meters))
            yield d


def _empty(dev) -> ParcelPlots:
    return ParcelPlots(torch.empty(10, 0, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                       torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, 2, dtype=torch.float32, device=dev),
                       np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), [], np.zeros((0, 2), dtype=np.float32))


def prepare_parcel(parcel_cloud, args, centers=None, keep=None, device=None, min_points: int = MIN_POINTS) -> ParcelPlots:
    """parcel_cloud: (10,T) float32, numpy or a device tensor, in the reference's channel order and absolute metres ->
    the kept plots (>= min_points points: 51) of the parcel, prepared on the device.  centers: None (the reference's lattice over
    the parcel's bounding box, `parcel_plot_centers` with `keep`) or a (P,2) set of plot centres (any: duplicates and centres
    without points included).  min_points: a plot is kept iff it has at least that many points (pseudo-labelling keeps the
    plots above 2000: the others are then never extracted); the kept plots' bytes do not depend on it."""
    min_points = int(min_points)
    if min_points < 1:
        raise ValueError("prepare_parcel: min_points must be at least 1")
    dev = torch.device(device) if device is not None else (
        parcel_cloud.device if isinstance(parcel_cloud, torch.Tensor) and parcel_cloud.is_cuda else torch.device("cuda"))
    cloud = torch.as_tensor(parcel_cloud).to(device=dev, dtype=torch.float32).contiguous()
    if cloud.dim() != 2 or cloud.shape[0] != 10 or cloud.shape[1] == 0:
        raise ValueError(f"parcel_cloud: expected (10,T) with T > 0, got {tuple(cloud.shape)}")
    T = cloud.shape[1]
    if T >= 2 ** 31:
        raise ValueError("parcel_cloud: at most 2^31 - 1 points")
    with torch.cuda.device(dev):
        box = torch.cat([cloud[:2].min(1).values, cloud[:2].max(1).values]).cpu().numpy()   # fp32, get_xy_range
        bbox = (box[0], box[1], box[2], box[3])                  # x_min, y_min, x_max, y_max
        if centers is None:
            centers = parcel_plot_centers(box[0], box[2], box[1], box[3], args, keep)
        centers = np.ascontiguousarray(np.asarray(centers, dtype=np.float32).reshape(-1, 2))
        P = len(centers)
        radius = args.diam_meters // 2
        grid = center_grid(centers, radius, bbox) if P else None
        if grid is None:
            return _empty(dev)
        L = max(ROW_POINTS, -(-T * P // MAX_TABLE + 63) // 64 * 64)     # rows * P <= about MAX_TABLE
        rows = -(-T // L)
        cen = torch.from_numpy(centers).to(dev)
        g = (torch.from_numpy(grid[0]).to(dev), torch.from_numpy(grid[1]).to(dev)) + grid[2:]
        prefix, total = ops.parcel_count(cloud, cen, g, radius, L, rows)
        starts = torch.cat([prefix[::rows].to(torch.int64), total]).cpu().numpy()
        if starts[-1] >= 2 ** 31:
            raise ValueError(f"prepare_parcel: {starts[-1]} plot points in all discs, at most 2^31 - 1")
        starts = starts[:-1]
        counts = np.diff(starts)
        kept = counts >= min_points
        if not kept.any():
            return _empty(dev)
        n_points = counts[kept]
        offsets = np.concatenate([[0], np.cumsum(n_points)])
        base = np.full(P, INT_MIN, dtype=np.int64)
        base[kept] = offsets[:-1] - starts[:-1][kept]
        raw, pidx = ops.parcel_fill(cloud, cen, g, radius, L, rows, prefix, torch.from_numpy(base.astype(np.int32)).to(dev),
                                    int(offsets[-1]))
        offsets_dev = torch.from_numpy(offsets.astype(np.int32)).to(dev)
        centers_kept = np.ascontiguousarray(centers[kept])
        cen_kept = torch.from_numpy(centers_kept).to(dev)
        ops.parcel_znorm(cloud, bbox, float(getattr(args, "znorm_radius_in_meters", 1.5)), radius, offsets_dev, cen_kept, pidx,
                         raw)
    plot_index = np.nonzero(kept)[0]
    return ParcelPlots(raw, offsets_dev, pidx, cen_kept, n_points, plot_index,
                       [plot_id(k, centers[k]) for k in plot_index], centers_kept)


def mosaic_extent(centers_host: np.ndarray, args):
    """(x_min, y_max, height_pix, width_pix) of the mosaic that holds every plot raster of the given centres: left = min cx -
    diam_meters//2, top = max cy + diam_meters//2, pixels of diam_meters/diam_pix metres, plot windows placed as
    `ParcelMosaic.offsets` places them."""
    half = args.diam_meters // 2
    c = torch.as_tensor(np.asarray(centers_host), dtype=torch.float64).reshape(-1, 2)
    left, top = float(c[:, 0].min()) - half, float(c[:, 1].max()) + half
    pix = args.diam_meters / args.diam_pix
    rows = torch.round((top - (c[:, 1] + half)) / pix)                # as ParcelMosaic.offsets
    cols = torch.round(((c[:, 0] - half) - left) / pix)
    return left, top, int(rows.max()) + args.diam_pix, int(cols.max()) + args.diam_pix


def parcel_mosaic(centers_host: np.ndarray, args, device) -> ParcelMosaic:
    """The `ParcelMosaic` of `mosaic_extent`."""
    return ParcelMosaic(*mosaic_extent(centers_host, args), args, device)


def predict_parcel_cloud(model, parcel_cloud, args, batch_size: int = 20, rs=np.random, keep=None, prefetch: int = 3,
                         centers=None, fps_start: Optional[int] = None, sampler="numpy", seed=None, n_live: bool = True,
                         shape=None, key_base: int = 0, points: bool = False):
    """prepare_parcel + a mosaic sized to the plots + `inference.predict_parcel` -> (ParcelMosaic, ParcelPlots).  The mosaic
    is None when the parcel has no kept plot.  `mosaic.finalize()` gives the coverage bands.  sampler, seed, n_live: as
    `ParcelPlots.batches`.  shape: the rings of the parcel polygon (`polygon_edges`); with keep=None the lattice is then
    filtered by `polygon_keep(shape, shape_buffer(args))` as the reference filters it, and `mosaic.report(shape)` gives the
    bands cropped to the polygon and the parcel's band means.  key_base: as `ParcelPlots.batches`.
    points=True: -> (ParcelMosaic, ParcelPlots, `inference.PointScores`): the model's pointwise coverages and class
    probabilities merged back onto the parcel's own points, one more launch per batch; the mosaic's bytes are those of
    points=False."""
    check_sampler(sampler)
    if shape is not None and keep is None:
        keep = polygon_keep(shape, shape_buffer(args))
    plots = prepare_parcel(parcel_cloud, args, centers=centers, keep=keep)
    scores = PointScores(parcel_cloud.shape[1], plots.raw.device) if points else None
    if len(plots) == 0:
        return (None, plots, scores) if points else (None, plots)
    mosaic = parcel_mosaic(plots.centers_host, args, plots.raw.device)
    predict_parcel(model, plots.batches(args, batch_size, rs, fps_start, sampler, seed, n_live, key_base, with_samples=points),
                   mosaic, args, prefetch=prefetch, point_sink=scores.add if points else None)
    return (mosaic, plots, scores) if points else (mosaic, plots)


@dataclass
class ParcelSet(ParcelPlots):
    """The kept plots of K parcels as ONE `ParcelPlots` (raw concatenated, offsets shifted; plot ids, centres, n_points and
    plot_index as they are per parcel; point_index relative to the plot's own parcel cloud) plus parcel_of (P): the parcel of
    every plot, and parcel_start (K+1): parcel k owns the plots parcel_start[k] .. parcel_start[k+1] (none is legal).  Both on
    the host.  point_start (K+1) int64, host: the first column of every parcel's cloud in the arena of all K (`ParcelClouds.
    point_start`; what `prepare_parcels` already computes), for scattering per-point results back (`batches(with_samples=True)`)."""
    parcel_of: np.ndarray = None
    parcel_start: np.ndarray = None
    point_start: np.ndarray = None

    @property
    def n_parcels(self) -> int:
        return len(self.parcel_start) - 1

    def plot_keys(self, key_base: int = 0) -> np.ndarray:
        """key_base + (parcel index << 32) + the plot's position inside its parcel: what the parcel's own `ParcelPlots` gives
        with key_base = k << 32, so a plot draws the same points in a set and alone."""
        k = self.parcel_of.astype(np.int64)
        return int(key_base) + (k << 32) + (np.arange(len(self), dtype=np.int64) - self.parcel_start[k])

    def _batches(self, args, batch_size, rs, fps_start, sampler, seed, with_live=True, key_base=0, with_samples=False):
        """`ParcelPlots.batches` over the whole set -- a batch may cut across parcels -- with one more key, "parcel": (B,) the
        parcel of every plot, on the host (non-decreasing); with_samples: and "col_base" (B) int32 on the device."""
        if with_samples:
            if self.point_start is None:
                raise ValueError("ParcelSet.batches(with_samples=True) needs point_start (prepare_parcels sets it)")
            col_base = torch.from_numpy(np.asarray(self.point_start, dtype=np.int64)[self.parcel_of].astype(np.int32)).to(self.raw.device)
        b0 = 0
        for d in super()._batches(args, batch_size, rs, fps_start, sampler, seed, with_live, key_base, with_samples):
            b1 = b0 + len(d["plot_center"])
            d["parcel"] = self.parcel_of[b0:b1]
            if with_samples:
                d["col_base"] = col_base[b0:b1]
            b0 = b1
            yield d


@dataclass
class ParcelClouds:
    """K parcel clouds in ONE (10, T_all) fp32 device array, channel-major: parcel k owns the columns point_start[k] ..
    point_start[k+1] (host, int64).  What the batched `prepare_parcels` works on (csrc/parcels.hip).  The arena is not to be
    written after `from_clouds`: `boxes` folds into a state that already holds what it found before."""
    arena: torch.Tensor
    point_start: np.ndarray
    _starts_host: np.ndarray = None
    _starts_dev: torch.Tensor = None
    _box_state: torch.Tensor = None

    @property
    def K(self) -> int:
        return len(self.point_start) - 1

    @classmethod
    def from_clouds(cls, clouds, device=None) -> "ParcelClouds":
        """clouds: K arrays (10,T>0), numpy or tensors -> one concatenation; host arrays are joined on the host and uploaded
        once.  device: None = that of the first device tensor, else the current HIP device."""
        clouds = list(clouds)
        if len(clouds) == 0:
            raise ValueError("ParcelClouds: no parcel")
        for c in clouds:
            if len(getattr(c, "shape", ())) != 2 or c.shape[0] != 10 or c.shape[1] == 0:
                raise ValueError(f"ParcelClouds: expected (10,T) with T > 0, got {tuple(getattr(c, 'shape', ()))}")
        T = np.array([c.shape[1] for c in clouds], dtype=np.int64)
        if T.sum() >= 2 ** 31:
            raise ValueError("ParcelClouds: at most 2^31 - 1 points in all")
        on_dev = [c for c in clouds if isinstance(c, torch.Tensor) and c.is_cuda]
        dev = torch.device(device) if device is not None else (on_dev[0].device if on_dev else torch.device("cuda"))
        if not on_dev:
            host = np.concatenate([np.asarray(c, dtype=np.float32) for c in clouds], axis=1)
            arena = torch.from_numpy(np.ascontiguousarray(host)).to(dev)
        else:
            arena = torch.cat([torch.as_tensor(c).to(device=dev, dtype=torch.float32) for c in clouds], dim=1).contiguous()
        starts = ops.parcels_bbox_starts(T)
        starts_dev, state = ops.pack_upload([starts, ops.parcels_bbox_identity(len(T))], dev)
        return cls(arena, starts[0].copy(), starts, starts_dev, state)

    @classmethod
    def from_arena(cls, arena: torch.Tensor, counts) -> "ParcelClouds":
        """An arena that is already filled -- (10, sum counts) fp32 on the device, parcel k in the next counts[k] > 0 columns (e.g.
        las.load_parcel_clouds decodes each file into its columns) -- with the bookkeeping of `from_clouds` and no concatenation:
        the arena is taken as it is, not copied."""
        T = np.asarray(counts, dtype=np.int64).reshape(-1)
        if len(T) == 0 or (T <= 0).any():
            raise ValueError("ParcelClouds: every parcel needs T > 0 points")
        if T.sum() >= 2 ** 31:
            raise ValueError("ParcelClouds: at most 2^31 - 1 points in all")
        if (not isinstance(arena, torch.Tensor) or not arena.is_cuda or arena.dtype != torch.float32 or not arena.is_contiguous()
                or tuple(arena.shape) != (10, int(T.sum()))):
            raise ValueError(f"ParcelClouds: expected a contiguous (10,{int(T.sum())}) fp32 device tensor")
        starts = ops.parcels_bbox_starts(T)
        starts_dev, state = ops.pack_upload([starts, ops.parcels_bbox_identity(len(T))], arena.device)
        return cls(arena, starts[0].copy(), starts, starts_dev, state)

    def cloud(self, k: int) -> torch.Tensor:
        """parcel k's (10,T_k) view of the arena"""
        return self.arena[:, int(self.point_start[k]):int(self.point_start[k + 1])]

    def boxes(self) -> np.ndarray:
        """(K,4) fp32 = x_min, y_min, x_max, y_max of every parcel (`cloud[:2].min(1)`, `.max(1)`): one launch, one read."""
        with torch.cuda.device(self.arena.device):
            state = ops.parcels_bbox(self.arena, self._starts_host, self._starts_dev, self._box_state)
        return ops.parcels_bbox_decode(state.cpu().numpy())


@dataclass
class ParcelCut:
    """What `cut_parcels` makes of a tile and K polygons.  clouds: a `ParcelClouds` over the parcels that got points (None when
    no parcel got any); parcel_index: their shape ids, ascending (host int64); counts (K,): points per shape, zeros included;
    point_index: device int32, the tile column of every arena column; shapes_kept: the kept parcels' rings in the cloud's frame,
    ready for `prepare_parcels(cut.clouds, args, shapes=cut.shapes_kept)` and `predict_parcels`."""
    clouds: Optional[ParcelClouds]
    parcel_index: np.ndarray
    counts: np.ndarray
    point_index: torch.Tensor
    shapes_kept: list


def shift_rings(shapes, origin=None):
    """K ring lists -> the same as fp64 (V,2) arrays, `origin` = (x0, y0) subtracted in fp64 from every vertex (None: nothing)."""
    o = np.zeros(2, dtype=np.float64) if origin is None else np.asarray(origin, dtype=np.float64).reshape(-1)[:2]
    if o.shape != (2,) or not np.isfinite(o).all():
        raise ValueError("origin: expected finite (x0, y0)")
    return [[np.asarray(r, dtype=np.float64).reshape(-1, 2) - o for r in rings] for rings in shapes]


def cut_parcels(cloud, shapes, buffer_m: float = LAS_PARCEL_BUFFER, origin=None, classification=None, drop_classes=(), device=None,
                max_table: int = MAX_TABLE) -> ParcelCut:
    """The points of a LAS tile cut into one cloud per parcel on the device (csrc/cut.hip): parcel k gets every point that
    `polygon_keep(shapes[k], buffer_m)` keeps -- inside the polygon by even-odd, or nearer than buffer_m to its boundary in fp64
    --, in ascending tile index, byte for byte `tile[:, mask_k]`.  A point in two parcels' buffers is copied into both.

    cloud: a (10,T) device tensor (las.load_las), or a `ParcelClouds` of tiles (las.load_parcel_clouds): its arena is taken as ONE
    cloud and `point_index` then indexes arena columns.  shapes: K ring lists ([exterior, *holes, *further parts], each (V,2)), as
    `prepare_parcels(shapes=...)` takes them.  The cloud and the shapes MUST be in one frame: origin = (x0, y0) is subtracted in
    fp64 from every ring vertex on the host, so polygons in Lambert-93 metres meet a cloud decoded with las.load_las(origin=...)
    (in its "reference" mode that origin is in raw centimetres: pass (X0 / 100, Y0 / 100) here).  classification: (T) uint8 on
    the device (las.decode(classification=...)); a point whose class is in drop_classes belongs to no parcel.  max_table: the
    (parcel, row) entries up to which a row is 2048 points.
    One packed upload, count, ONE device-to-host read (the K + 1 parcel starts), fill; more than 2^31 - 1 hits raise ValueError.
    The buffer inherits `polygon_keep`'s deviation from shapely's 16-segment round joins."""
    if isinstance(cloud, ParcelClouds):
        cloud = cloud.arena
    if not isinstance(cloud, torch.Tensor):
        cloud = torch.from_numpy(np.ascontiguousarray(np.asarray(cloud, dtype=np.float32))).to(
            torch.device("cuda") if device is None else torch.device(device))
    elif device is not None and cloud.device != torch.device(device):
        cloud = cloud.to(device)
    if cloud.dim() != 2 or cloud.shape[0] != 10 or cloud.shape[1] == 0:
        raise ValueError(f"cut_parcels: expected a (10,T) cloud with T > 0, got {tuple(cloud.shape)}")
    cloud = cloud.contiguous()
    shapes = list(shapes)
    K = len(shapes)
    if K == 0:
        raise ValueError("cut_parcels: no parcel")
    rings = shift_rings(shapes, origin)
    drop = ops.cut_drop_words(drop_classes)
    if classification is None and drop.any():
        raise ValueError("cut_parcels: drop_classes needs the points' classification")
    if classification is None or not drop.any():
        classification, drop = None, None                         # an empty drop set: the pass without a mask
    dev = cloud.device
    table = ops.CutTable([polygon_edges(r) for r in rings], cloud.shape[1], buffer_m, max_table=max_table)
    with torch.cuda.device(dev):
        table.upload(dev)
        prefix, starts_dev = ops.cut_count(cloud, table, classification, drop)
        starts = starts_dev.cpu().numpy()                                                # the one read
        if starts[-1] >= 2 ** 31:
            raise ValueError(f"cut_parcels: {starts[-1]} points in all parcels, at most 2^31 - 1 in one cut")
        counts = np.diff(starts).astype(np.int64)
        kept = counts > 0
        if not kept.any():
            return ParcelCut(None, np.zeros(0, dtype=np.int64), counts, torch.empty(0, dtype=torch.int32, device=dev), [])
        offsets = np.concatenate([[0], np.cumsum(counts[kept])])
        base = np.full(K, INT_MIN, dtype=np.int64)
        base[kept] = offsets[:-1] - starts[:-1][kept]
        base_dev, = ops.pack_upload([base.astype(np.int32)], dev)
        out, pidx = ops.cut_fill(cloud, table, prefix, base_dev, int(offsets[-1]), classification, drop)
    ids = np.nonzero(kept)[0].astype(np.int64)
    return ParcelCut(ParcelClouds.from_arena(out, counts[kept]), ids, counts, pidx, [rings[k] for k in ids])


def _keep_of(k, args, shapes, keeps):
    keep = keeps[k] if keeps is not None else None
    if keep is None and shapes is not None and shapes[k] is not None:
        keep = polygon_keep(shapes[k], shape_buffer(args))
    return keep


def _host_lattices(boxes, args, shapes, keeps, radius):
    """Per parcel, on the host and by the functions `prepare_parcel` uses: (centres (P,2) fp32, `center_grid`'s tuple or None)."""
    out = []
    for k, box in enumerate(boxes):
        centers = parcel_plot_centers(box[0], box[2], box[1], box[3], args, _keep_of(k, args, shapes, keeps))
        centers = np.ascontiguousarray(np.asarray(centers, dtype=np.float32).reshape(-1, 2))
        out.append((centers, center_grid(centers, radius, (box[0], box[1], box[2], box[3])) if len(centers) else None))
    return out


def _empty_set(K, dev) -> ParcelSet:
    e = _empty(dev)
    return ParcelSet(e.raw, e.offsets, e.point_index, e.centers, e.n_points, e.plot_index, [], e.centers_host,
                     np.zeros(0, dtype=np.int64), np.zeros(K + 1, dtype=np.int64))


def _prepare_batched(pc: ParcelClouds, args, shapes, keeps, min_points: int, strict: bool):
    """The batched sequence of `prepare_parcels` -> ParcelSet; None when a limit of the arena kernels is exceeded and `strict` is
    off (the caller then loops)."""
    K, dev = pc.K, pc.arena.device
    radius = args.diam_meters // 2
    zradius = float(getattr(args, "znorm_radius_in_meters", 1.5))
    boxes = pc.boxes()                                                                   # read 1
    lat = _host_lattices(boxes, args, shapes, keeps, radius)
    centers = [c if g is not None else c[:0] for c, g in lat]                            # no centre within reach: none at all
    grids = [g for _, g in lat]
    try:
        table = ops.ParcelTable(np.diff(pc.point_start), [len(c) for c in centers], grids, boxes, radius, zradius)
    except ops.StrataHipError as e:
        if strict or "SN2_ELIMIT" not in str(e):
            raise
        return None
    if table.P_all == 0:
        return _empty_set(K, dev)
    cen_all = np.concatenate(centers).astype(np.float32).reshape(-1, 2)
    item0 = np.concatenate([[0], np.cumsum([len(g[1]) for g in grids if g is not None])])
    cell_start = np.concatenate([g[0] + np.int32(o) for g, o in zip([g for g in grids if g is not None], item0)]).astype(np.int32)
    cell_items = np.concatenate([g[1] for g in grids if g is not None]).astype(np.int32)
    with torch.cuda.device(dev):
        table.dev, cen_dev, start_dev, items_dev = ops.pack_upload([table.host, cen_all, cell_start, cell_items], dev)
        prefix, plot_start = ops.parcels_count(pc.arena, table, cen_dev, start_dev, items_dev)
        starts = plot_start.cpu().numpy()                                                # read 2
        if starts[-1] >= 2 ** 31:
            raise ValueError(f"prepare_parcels: {starts[-1]} plot points in all discs of all parcels, at most 2^31 - 1 in one "
                             "batched pass: prepare the parcels with batched=False")
        counts = np.diff(starts)
        kept = counts >= min_points
        if not kept.any():
            return _empty_set(K, dev)
        n_points = counts[kept].astype(np.int64)
        offsets = np.concatenate([[0], np.cumsum(n_points)])
        base = np.full(table.P_all, INT_MIN, dtype=np.int64)
        base[kept] = offsets[:-1] - starts[:-1][kept]
        parcel_all = np.repeat(np.arange(K, dtype=np.int64), [len(c) for c in centers])
        parcel_of = parcel_all[kept]
        centers_kept = np.ascontiguousarray(cen_all[kept])
        base_dev, offsets_dev, cen_kept, of_dev = ops.pack_upload(
            [base.astype(np.int32), offsets.astype(np.int32), centers_kept, parcel_of.astype(np.int32)], dev)
        raw, pidx = ops.parcels_fill(pc.arena, table, cen_dev, start_dev, items_dev, prefix, base_dev, int(offsets[-1]))
        ops.parcels_znorm(pc.arena, table, offsets_dev, cen_kept, of_dev, pidx, raw)
    c0 = table.host[:K, 3]
    plot_index = np.nonzero(kept)[0] - c0[parcel_of]                                     # the plot's index among its parcel's centres
    per_parcel = np.bincount(parcel_of, minlength=K).astype(np.int64)
    return ParcelSet(raw, offsets_dev, pidx, cen_kept, n_points, plot_index.astype(np.int64),
                     [plot_id(i, c) for i, c in zip(plot_index, centers_kept)], centers_kept, parcel_of,
                     np.concatenate([[0], np.cumsum(per_parcel)]))


def prepare_parcels(clouds, args, shapes=None, keeps=None, device=None, min_points: int = MIN_POINTS, batched=None) -> ParcelSet:
    """The plots of K parcels as a `ParcelSet`.  clouds: a list of (10,T) clouds or a `ParcelClouds`.  shapes: per parcel the
    rings of its polygon or None -- the lattice is filtered by `polygon_keep(shape, shape_buffer(args))` --; keeps: per parcel a
    `keep` callable or None, which goes before the shape.
    batched=False: `prepare_parcel` of every cloud, unchanged, concatenated.  batched=True: all parcels in one pass over a cloud
    arena (csrc/parcels.hip) -- the boxes (device-to-host read 1), the lattices and centre grids on the host by the functions
    `prepare_parcel` uses, one packed upload, count, the plots' starts (read 2), kept / offsets / plot_base on the host, one
    packed upload, fill, z-norm -- about 16 launches and 2 reads for the set instead of as many per parcel.  The `ParcelSet` is
    the loop's, byte for byte.  More than 2^31 - 1 hits over all parcels raise ValueError (the loop's limit is per parcel).
    batched=None: batched when K >= 2 and the arena kernels' limits hold (2^31 points, 2^28 (plot, row) entries and centre
    cells, 2^26 z-norm cells in all), else the loop."""
    pc = clouds if isinstance(clouds, ParcelClouds) else None
    K = pc.K if pc is not None else len(clouds)
    if K == 0:
        raise ValueError("prepare_parcels: no parcel")
    for name, v in (("shapes", shapes), ("keeps", keeps)):
        if v is not None and len(v) != K:
            raise ValueError(f"prepare_parcels: {name} needs one entry per parcel")
    min_points = int(min_points)
    if min_points < 1:
        raise ValueError("prepare_parcels: min_points must be at least 1")
    if batched is None:
        batched = K >= 2 and (pc is not None or (all(len(getattr(c, "shape", ())) == 2 for c in clouds) and
                                                 sum(int(c.shape[1]) for c in clouds) < 2 ** 31))
        strict = False
    else:
        strict = True
    if batched:
        if pc is None:
            pc = ParcelClouds.from_clouds(clouds, device)
        out = _prepare_batched(pc, args, shapes, keeps, min_points, strict)
        if out is not None:
            out.point_start = np.asarray(pc.point_start, dtype=np.int64).copy()
            return out
    if pc is not None:
        clouds = [pc.cloud(k) for k in range(K)]
    point_start = np.concatenate([[0], np.cumsum([int(c.shape[1]) for c in clouds])]).astype(np.int64)
    parts = [prepare_parcel(cloud, args, keep=_keep_of(k, args, shapes, keeps), device=device, min_points=min_points)
             for k, cloud in enumerate(clouds)]
    dev = parts[0].raw.device
    counts = np.array([len(p) for p in parts], dtype=np.int64)
    n_points = np.concatenate([p.n_points for p in parts]).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(n_points)])
    if offsets[-1] >= 2 ** 31:
        raise ValueError(f"prepare_parcels: {offsets[-1]} plot points in all parcels, at most 2^31 - 1")
    return ParcelSet(torch.cat([p.raw for p in parts], 1), torch.from_numpy(offsets.astype(np.int32)).to(dev),
                     torch.cat([p.point_index for p in parts]), torch.cat([p.centers for p in parts]), n_points,
                     np.concatenate([p.plot_index for p in parts]), [i for p in parts for i in p.plot_ids],
                     np.concatenate([p.centers_host for p in parts]).astype(np.float32).reshape(-1, 2),
                     np.repeat(np.arange(K, dtype=np.int64), counts), np.concatenate([[0], np.cumsum(counts)]), point_start)


def predict_parcels(model, clouds, args, shapes=None, batch_size: int = 512, sampler="device", seed=None,
                    fps_start: Optional[int] = None, prefetch: int = 3, n_live: bool = True, rs=np.random, batched=None,
                    points: bool = False):
    """K parcels predicted in shared batches: `prepare_parcels` (batched: as there), a `MosaicAtlas` with one canvas per parcel, and
    `inference.predict_parcel`'s prefetching loop over the set's batches, which cut across parcels -- each batch ends in ONE
    `atlas.add` -> (MosaicAtlas, ParcelSet).  `atlas.report(shapes)` gives every parcel's cropped bands and band means with one
    device-to-host read.  Canvas k holds the bytes of `predict_parcel_cloud(model, clouds[k], ..., key_base=k << 32)`'s mosaic
    (an eval forward of a plot does not depend on the batch it is in).
    points=True: -> (MosaicAtlas, ParcelSet, `inference.PointScores`) over the columns of the whole cloud arena (`plots.point_start`);
    `scores.parcel(k)` holds the bytes of that parcel's own `predict_parcel_cloud(..., key_base=k << 32, points=True)` scores."""
    check_sampler(sampler)
    plots = prepare_parcels(clouds, args, shapes=shapes, batched=batched)
    atlas = MosaicAtlas.for_plots(plots, args)
    scores = PointScores(int(plots.point_start[-1]), plots.raw.device, plots.point_start) if points else None
    if len(plots):
        predict_batches(model, plots.batches(args, batch_size, rs, fps_start, sampler, seed, n_live, with_samples=points), args,
                        lambda rasters, cur: atlas.add(rasters, cur["plot_center"], cur["parcel"]), prefetch=prefetch,
                        point_sink=scores.add if points else None)
    return (atlas, plots, scores) if points else (atlas, plots)
