"""Seeded synthetic plots in the exact format the reference DataLoader hands to `PointNet2.forward`
(no real LAS data exists offline).

Format contract (reference `data_loader/loader.py:73-87`, `config.py:54-65`):
    cloud (B,10,N) fp32 rows = [x/10, y/10, z/z_max, red, green, blue, nir, intensity, return_num, num_returns]
    xyz   (B,3,N)  fp32      = centred, un-rescaled metres (copied before rescale, `loader.py:79`)
Geometry: 10 m-radius disc (`loader.py:127-132`); z mixture 55 % ground |N(0,0.05)|, 25 % U(0,1.5),
20 % U(1.5,20) (strata limits `learning/kde_mixture.py:54-58`, z_max `config.py:73`).
"""
import math
from types import SimpleNamespace

import torch

BASE_SEED = 20211007
Z_MAX = 24.24
# the rows of a ten-row cloud that LiDAR without colour has: x, y, z, intensity, return_num, num_returns.  `cloud[:, LIDAR_ROWS]` is the
# six-row cloud of a four-feature model (make_args(n_input_feats=6)); the same model reads exactly these rows of the ten-row cloud
LIDAR_ROWS = (0, 1, 2, 7, 8, 9)


def make_args(**kw):
    """The fields of the reference `config.py` Namespace that the hot path reads
    (`model/point_net2.py:73-85`, `model/project_to_2d.py:21,26,68-78`), with the reference defaults."""
    d = dict(cuda=None, subsample_size=10000, n_class=4, drop=0.0, n_input_feats=10, ratio1=0.25,
             r1=math.sqrt(2.0), ratio2=0.25, r2=math.sqrt(8.0), patience_in_epochs=30, log_embeddings=False,
             diam_pix=20, diam_meters=20, z_max=Z_MAX, m=0.10, e=0.2 / 5, epoch_to_start_early_stop=250,
             current_fold_id=-1, stats_path=".")
    d.update(kw)
    return SimpleNamespace(**d)


def make_plot(n_points: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(n_points, 9, generator=g, dtype=torch.float32)
    nrm = torch.randn(n_points, generator=g, dtype=torch.float32)
    rad = 10.0 * torch.sqrt(u[:, 0])
    th = (2.0 * math.pi) * u[:, 1]
    x, y = rad * torch.cos(th), rad * torch.sin(th)
    sel = u[:, 2]
    z = torch.where(sel < 0.55, (0.05 * nrm).abs(),
                    torch.where(sel < 0.80, 1.5 * u[:, 3], 1.5 + 18.5 * u[:, 3]))
    rgbn_i = u[:, 4:9]
    g2 = torch.Generator().manual_seed(seed + 7919)
    ret = torch.randint(0, 7, (n_points, 2), generator=g2).float() / 6.0
    xyz = torch.stack([x, y, z], 0)
    cloud = torch.cat([torch.stack([x / 10.0, y / 10.0, z / Z_MAX], 0), rgbn_i.t(), ret.t()], 0)
    return cloud.contiguous(), xyz.contiguous()


def make_raw_plot(n_points: int, seed: int, center=(0.0, 0.0)):
    """`make_plot(n_points, seed)` as a RAW plot (10, n) fp32 in the units `load_cloud` starts from (`loader.py:73-87`, channel order
    of `hip_ops.prepare_plots`): absolute metres around `center`, 16-bit colours, 15-bit intensity, return numbers from 1."""
    cloud, xyz = make_plot(n_points, seed)
    cx, cy = (float(c) for c in center)
    return torch.cat([torch.stack([xyz[0] + cx, xyz[1] + cy, xyz[2]], 0), torch.floor(cloud[3:7] * 65535.0),
                      torch.floor(cloud[7:8] * 32767.0), cloud[8:10] * 6.0 + 1.0], 0).contiguous()


def make_batch(batch_size: int, n_points: int, first_plot: int = 0, base_seed: int = BASE_SEED):
    """Returns the `cloud_data` dict of the reference (CPU tensors) plus the harness-side extras of the
    training step: `coverages` (B,4) float64 ground truth and `pdf_all` (B*N,3) float64 (stand-in for the
    KDE mixture evaluated at the points' z: `learning/loss_functions.py:27-42`)."""
    clouds, xyzs = [], []
    for p in range(first_plot, first_plot + batch_size):
        c, x = make_plot(n_points, base_seed + p)
        clouds.append(c)
        xyzs.append(x)
    g = torch.Generator().manual_seed(base_seed * 31 + first_plot)
    gt = torch.rand(batch_size, 4, generator=g, dtype=torch.float64)
    pdf = 0.05 + 0.95 * torch.rand(batch_size * n_points, 3, generator=g, dtype=torch.float64)
    return {"cloud": torch.stack(clouds), "xyz": torch.stack(xyzs), "coverages": gt, "pdf_all": pdf}


def make_parcel(width_m: float = 120.0, height_m: float = 100.0, density: float = 4.0, seed: int = 0, order: str = "scanline",
                x0: float = 650000.0, y0: float = 6860000.0, args=None, plant: bool = True):
    """A seeded parcel cloud (10,T) float32 in the reference's channel order and absolute Lambert-93-like metres, as
    `load_las_file` makes it: integer centimetres / 100, cast to fp32 (spacing 1/16 m in x, 1/2 m in y at these values).

    Mean density `density` points/m^2, four times higher on the left half than on the right, with an empty 50 m x 36 m
    gap.
    Four corner points fix the bounding box to (x0, y0, x0 + width_m, y0 + height_m), so the plot lattice is known; with
    `plant`, inside the gap two lattice discs get exactly 50 and 51 points, and around a few lattice centres points are
    planted at exactly 10 m (kept: the disc test is inclusive), pairs at exactly 1.5 m (the z-norm test is inclusive), and
    a low point just outside a disc next to a point just inside (the per-plot z-norm differs there from a parcel-wide one).
    order: "scanline" (sorted by 5 m strips, then y: flight lines) or "shuffled"."""
    import numpy as np
    from .parcel import parcel_plot_centers
    args = args or make_args()
    rng = np.random.default_rng(seed)
    f32 = np.float32
    x0, y0 = float(f32(x0)), float(f32(y0))
    area = width_m * height_m
    n = int(rng.poisson(density * area))
    u = rng.random((n, 2))
    left = rng.random(n) < 0.8                                    # 4:1 between the halves
    px = np.where(left, u[:, 0] * 0.5, 0.5 + u[:, 0] * 0.5) * width_m
    py = u[:, 1] * height_m
    gx, gy = 0.45 * width_m, 0.4 * height_m
    out_gap = ~((px >= gx) & (px <= gx + 50) & (py >= gy) & (py <= gy + 36))
    xy = np.stack([np.round((x0 + px[out_gap]) * 100) / 100, np.round((y0 + py[out_gap]) * 100) / 100], 1)
    corners = np.array([[x0, y0], [x0 + width_m, y0 + height_m], [x0, y0 + height_m], [x0 + width_m, y0]])
    pts = [np.concatenate([corners, xy])]
    zs = [None]
    cen = parcel_plot_centers(x0, f32(x0 + width_m), y0, f32(y0 + height_m), args).astype(np.float64)[1:]
    if plant:
        gap_lo, gap_hi = np.array([x0 + gx, y0 + gy]), np.array([x0 + gx + 50, y0 + gy + 36])
        inner = np.all((cen >= gap_lo + 11) & (cen <= gap_hi - 11), axis=1)
        sparse = cen[inner]
        if len(sparse) < 2:
            raise ValueError("make_parcel: the gap holds fewer than two lattice discs (parcel too small)")
        for c, k in zip(sparse[:2], (50, 51)):                    # discs of exactly 50 and 51 points
            a, r = rng.random(k) * 2 * np.pi, 3.0 * np.sqrt(rng.random(k))
            pts.append(np.stack([c[0] + r * np.cos(a), c[1] + r * np.sin(a)], 1))
        dense = cen[np.all((cen >= np.array([x0 + 15, y0 + 15])) & (cen <= np.array([x0 + gx - 15, y0 + height_m - 15])), 1)]
        for c in dense[::3]:
            c = c.astype(f32).astype(np.float64)                  # the fp32 centre the discs are cut around
            pts.append(c + np.array([[6.0, 8.0], [-10.0, 0.0], [0.0, 10.0], [-6.0, -8.0]]))      # exactly 10 m
            pts.append(c + np.array([[2.0, 2.0], [3.5, 2.0], [2.0, 3.5]]))                       # exactly 1.5 m apart
            pts.append(c + np.array([[9.5, 0.0], [10.5, 0.0]]))                                  # in / out of the disc
    xy = np.concatenate(pts).astype(f32)
    T = len(xy)
    z = np.round(np.where(rng.random(T) < 0.55, np.abs(0.05 * rng.standard_normal(T)),
                          np.where(rng.random(T) < 0.5, 1.5 * rng.random(T), 1.5 + 18.5 * rng.random(T))) * 100) / 100
    if plant:                                     # planted pairs: the second, 1.5 m away, and the out-of-disc point lower
        k = T - 9 * len(dense[::3])
        for j in range(len(dense[::3])):
            b = k + 9 * j
            z[b + 4], z[b + 5], z[b + 6] = 3.0, -2.0, 4.0
            z[b + 7], z[b + 8] = 1.0, -5.0
    z = z + 100.0                                 # absolute altitudes
    feats = np.stack([rng.integers(0, 65536, T), rng.integers(0, 65536, T), rng.integers(0, 65536, T),
                      rng.integers(0, 65536, T), rng.integers(0, 32768, T)]).astype(np.float64)
    nret = rng.integers(1, 5, T)
    ret = np.minimum(rng.integers(1, 5, T), nret)
    cloud = np.concatenate([xy.T.astype(np.float64), z[None], feats, ret[None], nret[None]]).astype(f32)
    if order == "shuffled":
        perm = rng.permutation(T)
    elif order == "scanline":
        perm = np.lexsort((cloud[1], np.floor((cloud[0] - f32(x0)) / 5)))
    else:
        raise ValueError("order must be 'scanline' or 'shuffled'")
    return np.ascontiguousarray(cloud[:, perm])
