"""Parcel inference on the device -- counterpart of the reference loop `predict.py:96-141` +
`inference/predict_utils.py:94-116` + the raster merge of `inference/geotiff_raster.py`, without the GIS file I/O
(GDAL / rasterio / shapefile are out of scope: DESIGN.md section 7).  The admissibility band and PRED_ADM are built on the
device by a stated rule of this project's, on request: `finalize(admissibility=s)`, `report(..., admissibility=s)`.

    per batch of plots:  eval forward -> (B*N,4) coverages -> fixed-grid max rasters (B,3,D,D)   [project_to_2d_rasters]
                         -> radial weight band                                                  [add_weights_band_to_rasters]
                         -> weighted accumulation into the parcel grid                          [rasterio.merge callback]
    at the end:          mosaic = sum(w*v) / sum(w), NaN where no plot has data

Pixel placement follows `get_geotransform` (geotiff_raster.py:46-61): a plot's top-left corner is
(center_x - diam_meters//2, center_y + diam_meters//2) and a pixel is diam_meters/diam_pix metres wide.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import hip_ops as ops
from .project_to_2d import project_batch_to_2d_rasters


def weights_band(diam_pix: int) -> np.ndarray:
    """`add_weights_band_to_rasters` (geotiff_raster.py:103-118): 1.5 - r on the normalised pixel-centre grid, NaN for
    r > 0.5 (outside the disc inscribed in the raster)."""
    x = (np.arange(-diam_pix // 2, diam_pix // 2, 1) + 0.5) / diam_pix       # loader.py:108-125
    xx, yy = np.meshgrid(x, x, sparse=True)
    r = np.sqrt(xx ** 2 + yy ** 2)
    w = 1.5 - r
    w[r > 0.5] = np.nan
    return w


def add_weights_band_to_rasters(img_to_write: np.ndarray, args) -> np.ndarray:
    """(C,D,D) -> (2C,D,D): one weight band per score band, as the reference writes into each plot GeoTIFF."""
    w = weights_band(args.diam_pix)
    return np.concatenate([img_to_write] + [w[None]] * len(img_to_write), 0)


class ParcelMosaic:
    """Running mosaic of plot rasters on a parcel grid (device resident), merged plot after plot with the rule of the
    reference's rasterio.merge callback (`_weighted_average_of_rasters`, geotiff_raster.py:294-347)."""

    def __init__(self, x_min: float, y_max: float, height_pix: int, width_pix: int, args, device):
        self.args = args
        self.x_min, self.y_max = float(x_min), float(y_max)
        self.pix = args.diam_meters / args.diam_pix
        nan = float("nan")
        self.mean = torch.full((3, height_pix, width_pix), nan, dtype=torch.float32, device=device)
        self.wsum = torch.full((3, height_pix, width_pix), nan, dtype=torch.float32, device=device)
        self.w = torch.from_numpy(weights_band(args.diam_pix).astype(np.float32)).to(device)

    def offsets(self, plot_centers) -> torch.Tensor:
        """(B,2) plot centres in metres -> (B,2) int32 (row, col) of the plots' top-left pixels (`get_geotransform`)."""
        c = torch.as_tensor(plot_centers, dtype=torch.float64).reshape(-1, 2)
        half = self.args.diam_meters // 2
        col = torch.round(((c[:, 0] - half) - self.x_min) / self.pix)
        row = torch.round((self.y_max - (c[:, 1] + half)) / self.pix)
        return torch.stack([row, col], 1).to(torch.int32)

    def add(self, rasters: torch.Tensor, plot_centers):
        off = self.offsets(plot_centers)
        D = self.args.diam_pix
        y0, x0 = int(off[:, 0].min()), int(off[:, 1].min())
        win = (y0, x0, int(off[:, 0].max()) + D - y0, int(off[:, 1].max()) + D - x0)
        ops.mosaic_merge(rasters.contiguous(), self.w, off.to(rasters.device), self.mean, self.wsum, win)

    def result(self) -> torch.Tensor:
        """(4,H,W): [low, med, high] merged scores + ONE weight band (`finalize_merged_raster` :270-275 keeps the
        first of the three identical weight layers)."""
        return torch.cat([self.mean, self.wsum[:1]], 0)

    def finalize(self, admissibility=None):
        """`finalize_merged_raster` (geotiff_raster.py:262-285): (5,H,W) = [Vb, Vm_soft, Vh, Vm_hard, weights] and the
        hard-medium-vegetation threshold that `insert_hard_med_veg_raster_band` (:119-144) searches for.
        admissibility: None (the default) stops there, before the reference's last, GIS step.  An integer s >= 0 adds that step
        by this project's stated rule (`ADMISSIBILITY` below): (6,H,W) = [Vb, Vm_soft, Vh, Vm_hard, Adm, weights], the reference's
        band order, with the sieve size s."""
        out, thr = ops.mosaic_finalize(self.mean.contiguous(), self.wsum[0].contiguous())
        if admissibility is not None:
            out, _ = ops.mosaic_admissibility(out, admissibility)
        return out, thr

    def report(self, rings=None, admissibility=None) -> "ParcelReport":
        """`finalize()`, then the crop of `crop_merged_raster` (geotiff_raster.py:238-253) on its (5,H,W) output in place --
        every pixel whose centre is not inside the parcel polygon becomes NaN --, then the band-wise means of the cropped
        mosaic that `get_parcel_predicted_values` (predict_utils.py:124-146) writes into the shapefile.  rings: every ring of
        the polygon, each a (V,2) array, closed or not -- exterior, holes, all parts of a multi-part polygon
        (`parcel.polygon_edges`; the inside test is `parcel.polygon_keep`'s even-odd rule, include/strata_hip.h:
        sn2_mosaic_crop_stats); None: no crop, the means of the whole mosaic.  Everything stays on the device but ONE
        device-to-host read of the threshold, the means and the counts together.

        admissibility: None (the default): five bands, the means of REPORT_BANDS, no PRED_ADM.  An integer s >= 0: the
        admissibility band is inserted before the crop, as the reference does (`ADMISSIBILITY` below: the rule is ours, s and the
        1.5 px tie are readings, not pinned facts); the report then has six bands, the means of REPORT_BANDS_ADM -- PRED_ADM among
        them -- and `admissibility_stats`, still with the ONE read.
        Where it differs from the reference: the reference sends the fp32-cast coordinates of the outside pixels back through
        `rowcol` (geotiff_raster.py:244-251), which at Lambert-93 magnitudes (an fp32 step of 0.5 m) masks a neighbouring
        pixel now and then -- here the pixel that was tested is masked; and the means are fp64 sums, not numpy's fp32
        pairwise `nanmean`."""
        adm = admissibility is not None
        C = 6 if adm else 5
        # threshold + index | means | counts | the admissibility statistics
        pack = torch.empty(1 + 2 * C + (4 if adm else 0), dtype=torch.int64, device=self.mean.device)
        thr, means, counts = pack[:1].view(torch.float32), pack[1:1 + C].view(torch.float64), pack[1 + C:1 + 2 * C]
        bands, _ = ops.mosaic_finalize(self.mean.contiguous(), self.wsum[0].contiguous(), thr=thr)
        if adm:
            six = torch.empty((6,) + tuple(bands.shape[1:]), dtype=torch.float32, device=bands.device)
            bands, _ = ops.mosaic_admissibility(bands, admissibility, out=(six, pack[1 + 2 * C:]))
        edges = None
        if rings is not None:
            from .parcel import polygon_edges
            edges = polygon_edges(rings)
        ops.mosaic_crop_stats(bands, self.x_min, self.y_max, self.pix, edges, out=(means, counts))
        host = pack.cpu().numpy()                                                      # the one read
        m, n = host[1:1 + C].view(np.float64).copy(), host[1 + C:1 + 2 * C].copy()
        names = REPORT_BANDS_ADM if adm else REPORT_BANDS
        return ParcelReport(bands, float(host[:1].view(np.float32)[0]),
                            {k: float(m[i]) for i, k in enumerate(names)}, {k: int(n[i]) for i, k in enumerate(names)},
                            m, n, C, host[1 + 2 * C:].copy() if adm else None)


REPORT_BANDS = ("PRED_BASSE", "PRED_INTER", "PRED_HAUTE", "hard_med")          # bands 0..3 of `finalize()`; band 4 = weights
# bands 0..4 of `finalize(admissibility=s)`; band 5 = weights.  The four PRED_ names are the reference's shapefile fields
REPORT_BANDS_ADM = ("PRED_BASSE", "PRED_INTER", "PRED_HAUTE", "hard_med", "PRED_ADM")

ADMISSIBILITY = """The admissibility band (include/strata_hip.h, "Admissibility band"; DESIGN.md section 6m) restates
`insert_admissibility_raster` (geotiff_raster.py:149-196) on the pixel grid: sieve the hard medium-vegetation band, call a pixel
inaccessible when everything within 1.5 px of its centre is hard medium vegetation (or outside the mosaic's data), and give every
other pixel max(Vb, Vm_soft).  The reference does this with rasterio `sieve` / `shapes`, a shapely buffer of -1.5 and
`geometry_mask`, which cannot be run beside this package, so the rule is OURS and two of its choices are readings, not pinned facts:
  the sieve size s -- 5 by the reference's comment ("Eliminate zones < 5 pixels"), 0 by its call as written (the mask it passes
      excludes the valid pixels, so nothing inside the parcel is sieved): s is an explicit argument without a default;
  the tie -- a pixel centre exactly 1.5 px from a pixel that is not hard medium vegetation (two columns or two rows away) lies ON
      the buffered outline; we count it as inaccessible (csrc/admissibility_rules.h: adm_offset_tested)."""


@dataclass
class ParcelReport:
    """`ParcelMosaic.report`: bands (5,H,W) on the device = [Vb, Vm_soft, Vh, Vm_hard, weights], NaN outside the parcel polygon
    (and wherever no plot has data); threshold of the hard medium-vegetation band; means / counts: per name of REPORT_BANDS the
    mean over, and the number of, the band's pixels that are not NaN; band_means (5) fp64 / band_counts (5) int64: the same for
    all five bands in order.  With `report(..., admissibility=s)`: n_bands = 6, bands (6,H,W) = [Vb, Vm_soft, Vh, Vm_hard, Adm,
    weights], the names are REPORT_BANDS_ADM -- means["PRED_ADM"] is the mean of band 4 over its pixels that are not NaN after
    the crop --, band_means / band_counts have six entries and admissibility_stats (4) int64 = the uncropped canvas's regions,
    regions smaller than s, sieved pixels and inaccessible pixels."""
    bands: torch.Tensor
    threshold: float
    means: dict
    counts: dict
    band_means: np.ndarray
    band_counts: np.ndarray
    n_bands: int = 5
    admissibility_stats: Optional[np.ndarray] = None


@torch.no_grad()
def predict_parcel(model, batches, mosaic: ParcelMosaic, args, prefetch: int = 3, point_sink=None):
    """`batches`: iterable of dicts with "cloud" (B,10,N), "xyz" (B,3,N), "plot_center" (B,2) (the reference DataLoader's
    collate of `inference/predict_utils.py:74-82`), optionally PointNet2's additive keys "fps_start" and "n_live" (`ParcelPlots.batches`
    sets "n_live"), which reach the geometry passes as they are.  Returns the number of plots processed.
    prefetch: how many batches ahead the position-only kernels (FPS, ball query, 3-NN) run, each on its own side stream
    (`PointNet2.prefetch_geometry`), while this batch's feature kernels, rasters and merge run.  FPS is M sequential rounds
    in one workgroup per plot -- 64 plots keep 64 of 256 CUs busy for most of an un-overlapped batch -- so several passes
    in flight is what fills the chip; 0 = no overlap.  point_sink: as `predict_batches`."""
    return predict_batches(model, batches, args, lambda rasters, cur: mosaic.add(rasters, cur["plot_center"]), prefetch=prefetch,
                           point_sink=point_sink)


SCORE_NAMES = ("cov_low", "cov_soil", "cov_med", "cov_high", "proba_0", "proba_1", "proba_2", "proba_3")   # rows of `scores`


@dataclass
class PointScoreResult:
    """`PointScores.finalize`, all on the device: scores (8,T) fp32 -- rows 0..3 the pointwise coverages, rows 4..7 the pointwise
    class probabilities, in the network's column order --, weight (T) fp32 the sum of the contributions' weights, hits (T) int32
    the number of plots that sampled the point.  A point no plot sampled has NaN scores, weight 0 and hits 0."""
    scores: torch.Tensor
    weight: torch.Tensor
    hits: torch.Tensor


class PointScores:
    """The network's pointwise outputs merged back onto the T points of a parcel cloud (or of a `parcel.ParcelClouds` arena), on the
    device (include/strata_hip.h, "Per-point scores"): every real point a plot's subsample drew gets that plot's (B*N,4) coverages
    and (B*N,4) class probabilities, and a point drawn by several overlapping plots their average under the mosaic's radial weight
    1.5 - r, taken at the point.  These are the MODEL's outputs on ITS subsample draws -- what `utils/visualize_predictions.py`
    plots per plot --, not a reference output: another seed draws other points, and a point no plot drew has no score.
    The sums are 64-bit integers, so the bytes do not depend on the batch size or the order of the plots.
    point_start (K+1): the first column of every parcel of an arena (`ParcelClouds.point_start`), for `parcel(k)`."""

    def __init__(self, T: int, device, point_start=None):
        self.T = int(T)
        self.acc = torch.zeros(self.T, ops.POINTS_ACC_WORDS, dtype=torch.int64, device=device)
        self.hits = torch.zeros(self.T, dtype=torch.int32, device=device)
        self.point_start = None if point_start is None else np.asarray(point_start, dtype=np.int64)
        self._result = None

    def add(self, cov: torch.Tensor, proba: torch.Tensor, batch: dict):
        """One batch of `ParcelPlots.batches(..., with_samples=True)` and the eval forward's outputs for it: ONE launch in stream
        order behind the forward, no synchronisation."""
        if "sample_index" not in batch:
            raise ValueError("PointScores.add: the batch carries no samples (ParcelPlots.batches(..., with_samples=True))")
        with torch.cuda.device(self.acc.device):
            ops.points_merge(cov.contiguous(), proba.contiguous(), batch["xyz"], batch["sample_index"], batch["sample_live"],
                             batch["point_offsets"], batch["point_index"], self.acc, self.hits, batch["diam_meters"],
                             col_base=batch.get("col_base"))
        self._result = None

    def finalize(self) -> PointScoreResult:
        if self._result is None:
            with torch.cuda.device(self.acc.device):
                scores, weight = ops.points_finalize(self.acc, self.hits)
            self._result = PointScoreResult(scores, weight, self.hits)
        return self._result

    def parcel(self, k: int) -> PointScoreResult:
        """parcel k's views of `finalize()`: scores (8,T_k), weight (T_k), hits (T_k)."""
        if self.point_start is None:
            raise ValueError("PointScores.parcel: these scores are of one parcel (no point_start)")
        r, p0, p1 = self.finalize(), int(self.point_start[k]), int(self.point_start[k + 1])
        return PointScoreResult(r.scores[:, p0:p1], r.weight[p0:p1], r.hits[p0:p1])


@torch.no_grad()
def predict_batches(model, batches, args, sink, prefetch: int = 3, point_sink=None):
    """The prefetching loop of `predict_parcel`: every batch's rasters (B,3,D,D) go to `sink(rasters, batch)` -- a
    `ParcelMosaic.add`, or a `MosaicAtlas.add` for batches that cut across parcels.  Returns the number of plots processed.
    point_sink: None, or a callable that gets `(cov, proba, batch)` -- the forward's pointwise outputs, (B*N,4) each -- after the
    raster sink (`PointScores.add`)."""
    from collections import deque
    model.eval()
    n = 0
    it = iter(batches)
    window = deque()                       # (batch, geometry handle or None), oldest first
    issued = 0

    def fill():
        nonlocal issued
        while len(window) < max(1, prefetch):
            b = next(it, None)
            if b is None:
                return
            geo = model.prefetch_geometry(b, lane=issued % prefetch) if prefetch > 0 else None
            window.append((b, geo))
            issued += 1

    fill()
    while window:
        cur, geo = window.popleft()
        fill()
        cd = dict(cur)
        if geo is not None:
            cd["geometry"] = geo
        cov, proba = model(cd)
        clouds_dev = model._last_cloud_dev[1]
        model._last_cloud_dev = None
        rasters, _ = project_batch_to_2d_rasters(clouds_dev, cov, args)
        sink(rasters, cur)
        if point_sink is not None:
            point_sink(cov, proba, cur)
        n += clouds_dev.shape[0]
    # (no check of hip_ops.fps_gave_up here: it reads a device word, i.e. synchronises; callers that synchronise anyway --
    # reading the mosaic back -- may ask for it)
    return n


class MosaicAtlas:
    """The running mosaics of K parcels in one arena on the device (include/strata_hip.h, "Mosaic atlas"): what K `ParcelMosaic`s
    hold, canvas k the bytes of parcel k's own mosaic, but merged, finalised, cropped and read back K canvases at a time.
    canvases: per parcel (x_min, y_max, height_pix, width_pix), or None for a parcel without plots (it owns a one-pixel canvas
    that nothing is merged into; `mosaic(k)` and its report's bands are None)."""

    def __init__(self, canvases, args, device):
        self.args = args
        self.pix = args.diam_meters / args.diam_pix
        self.empty = [c is None for c in canvases]
        full = [(0.0, 0.0, 1, 1) if c is None else c for c in canvases]
        self.table = ops.AtlasTable([c[2] for c in full], [c[3] for c in full], [float(c[0]) for c in full], [float(c[1]) for c in full],
                                    device=device)
        self.K = self.table.K
        self._x_min = torch.tensor([float(c[0]) for c in full], dtype=torch.float64)
        self._y_max = torch.tensor([float(c[1]) for c in full], dtype=torch.float64)
        nan = float("nan")
        self.mean = torch.full((3 * self.table.pixels,), nan, dtype=torch.float32, device=device)
        self.wsum = torch.full((3 * self.table.pixels,), nan, dtype=torch.float32, device=device)
        self.w = torch.from_numpy(weights_band(args.diam_pix).astype(np.float32)).to(device)

    @classmethod
    def for_plots(cls, parcel_set, args, device=None):
        """One canvas per parcel of a `parcel.ParcelSet`, each sized as `parcel.parcel_mosaic` sizes a parcel's own."""
        from .parcel import mosaic_extent
        start = parcel_set.parcel_start
        canvases = [mosaic_extent(parcel_set.centers_host[start[k]:start[k + 1]], args) if start[k + 1] > start[k] else None
                    for k in range(len(start) - 1)]
        return cls(canvases, args, parcel_set.raw.device if device is None else device)

    def offsets(self, plot_centers, parcel) -> np.ndarray:
        """(B,2) plot centres in metres and (B,) parcel indices -> (B,3) int32 (canvas, row, col) of the plots' top-left pixels
        (`ParcelMosaic.offsets`' arithmetic with the geotransform of each plot's own canvas), on the host."""
        c = torch.as_tensor(plot_centers, dtype=torch.float64).reshape(-1, 2)
        k = torch.as_tensor(np.asarray(parcel), dtype=torch.int64).reshape(-1)
        half = self.args.diam_meters // 2
        col = torch.round(((c[:, 0] - half) - self._x_min[k]) / self.pix)
        row = torch.round((self._y_max[k] - (c[:, 1] + half)) / self.pix)
        return torch.stack([k.to(torch.float64), row, col], 1).to(torch.int32).numpy()

    def add(self, rasters: torch.Tensor, plot_centers, parcel):
        """Fold a batch's rasters, in order, each into the canvas of its parcel: ONE launch.  parcel: (B,) non-decreasing."""
        ops.atlas_merge(rasters.contiguous(), self.w, self.offsets(plot_centers, parcel), self.table, self.mean, self.wsum)

    def mosaic(self, k: int):
        """(mean, wsum): parcel k's (3,H,W) views of the arenas -- what its `ParcelMosaic` holds --, None without plots."""
        if self.empty[k]:
            return None
        return self.table.view(self.mean, 3, k), self.table.view(self.wsum, 3, k)

    def finalize(self, admissibility=None):
        """`ParcelMosaic.finalize` of every canvas at once: (the (5,H_k,W_k) band arena, thr (K,2)); with an integer
        admissibility = s the (6,H_k,W_k) arena, the admissibility band inserted canvas by canvas."""
        bands, thr = ops.atlas_finalize(self.mean, self.wsum, self.table)
        if admissibility is not None:
            bands, _ = ops.atlas_admissibility(bands, self.table, admissibility)
        return bands, thr

    def report(self, shapes=None, admissibility=None) -> "AtlasReport":
        """`ParcelMosaic.report` of all K parcels: one finalisation, one crop and one statistics pass over the atlas, and ONE
        device-to-host read of the K thresholds, means and counts together.  shapes: None (no crop), or per parcel the rings of
        its polygon or None.  admissibility: as `ParcelMosaic.report` takes it -- None: five bands; an integer s >= 0: six, the
        admissibility band inserted in every canvas before the crop, its statistics in the same read."""
        adm = admissibility is not None
        C, K = (6 if adm else 5), self.K
        # thresholds + indices | means | counts | the admissibility statistics
        pack = torch.empty(K + 2 * K * C + (4 * K if adm else 0), dtype=torch.int64, device=self.mean.device)
        thr = pack[:K].view(torch.float32).view(K, 2)
        means, counts = pack[K:K + K * C].view(torch.float64).view(K, C), pack[K + K * C:K + 2 * K * C].view(K, C)
        bands, _ = ops.atlas_finalize(self.mean, self.wsum, self.table, thr=thr)
        if adm:
            six = torch.empty(6 * self.table.pixels, dtype=torch.float32, device=bands.device)
            bands, _ = ops.atlas_admissibility(bands, self.table, admissibility, out=(six, pack[K + 2 * K * C:].view(K, 4)))
        edges = None
        if shapes is not None:
            from .parcel import polygon_edges
            if len(shapes) != K:
                raise ValueError(f"shapes: expected one entry per parcel ({K}), got {len(shapes)}")
            edges = [None if (r is None or self.empty[k]) else polygon_edges(r) for k, r in enumerate(shapes)]
        ops.atlas_crop_stats(bands, C, self.table, self.pix, edges, out=(means, counts))
        host = pack.cpu().numpy()                                                          # the one read
        thresholds = host[:K].view(np.float32).reshape(K, 2)[:, 0].astype(np.float64)
        thresholds[np.asarray(self.empty, dtype=bool)] = np.nan
        return AtlasReport(thresholds, host[K:K + K * C].view(np.float64).reshape(K, C).copy(),
                           host[K + K * C:K + 2 * K * C].reshape(K, C).copy(), bands, self.table, list(self.empty), C,
                           host[K + 2 * K * C:].reshape(K, 4).copy() if adm else None)


@dataclass
class AtlasReport:
    """`MosaicAtlas.report`: thresholds (K) fp64, band_means (K,5) fp64 and band_counts (K,5) int64 on the host, the cropped band
    arena on the device.  bands(k): parcel k's (5,H,W) view; parcel(k): its `ParcelReport`.  A parcel without plots has None
    bands, a NaN threshold, NaN means and zero counts.  With `report(..., admissibility=s)`: n_bands = 6 -- six bands per canvas,
    six columns of means and counts -- and admissibility_stats (K,4) int64 (zeros for a parcel without plots)."""
    thresholds: np.ndarray
    band_means: np.ndarray
    band_counts: np.ndarray
    band_arena: torch.Tensor
    table: object
    empty: list
    n_bands: int = 5
    admissibility_stats: Optional[np.ndarray] = None

    def __len__(self):
        return len(self.thresholds)

    def bands(self, k: int):
        return None if self.empty[k] else self.table.view(self.band_arena, self.n_bands, k)

    def parcel(self, k: int) -> ParcelReport:
        m, n = self.band_means[k], self.band_counts[k]
        names = REPORT_BANDS_ADM if self.n_bands == 6 else REPORT_BANDS
        return ParcelReport(self.bands(k), float(self.thresholds[k]), {b: float(m[i]) for i, b in enumerate(names)},
                            {b: int(n[i]) for i, b in enumerate(names)}, m, n, self.n_bands,
                            None if self.admissibility_stats is None else self.admissibility_stats[k])
