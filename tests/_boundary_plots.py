"""Plots that sit ON the decisions of the geometry and pixel-id kernels, built from the oracle's arithmetic alone, for
tests/test_boundary_plots_host.py (which proves on the CPU that they reach those decisions) and tests/test_gpu_boundary_geometry.py
(which runs the kernels on them).  Not a test module; imports the oracle, numpy and torch, never the library.

  * lattice plots: a 10 m disc snapped to 0.25 m (exact in fp32: products and sums of coordinate differences are exact) or to
    centimetres as `load_las_file` forms them (round(v * 100) / 100, cast to fp32); 55 % of the points have z exactly 0;
  * degenerate plots, padded with repeats of earlier points as `sample_cloud` pads a short plot: flat (z = 0), line (y = z = 0),
    half disc (x >= 0), two positions, one position;
  * planted shells: points whose canonical d2 to an anchor is exactly fp32(r*r), the fp32 below it, the fp32 above it;
  * planted 3-NN ties: targets with the same fp32 d2 to two DISTINCT sources at rank 1/2, 2/3, 3/4, and targets on a source;
  * pixel-edge values: 129 consecutive fp32 values around the value at which the oracle's pixel id steps, for each of the 19
    interior edges of both grids;
  * wrong variants: the oracle restated with ONE line changed (`<=` in the ball, highest index on a k-NN tie, the pixel
    multiply-add fused, the bounding-box scale pre-multiplied, the bounding-box epsilon dropped).  Host code only: the host test
    shows that each differs from the oracle on these inputs, so a kernel that made the same mistake would fail the GPU test.
"""
import functools
import math

import numpy as np
import torch

from oracle import primitives as P
from oracle import projection

SEED = 7                                         # every generator below derives its streams from this one number
RADII = (1.0, 2.0 ** 0.5, 2.0, 8.0 ** 0.5)
D_PIX, D_METERS = 20, 20
Z_MAX = 24.24
F32 = np.float32


# ------------------------------------------------------------------------------------------------------------ fp32 neighbours
def f32_ord(v):
    """fp32 -> int64 whose order is the order of the floats and whose consecutive values are consecutive floats."""
    b = np.asarray(v, dtype=F32).view(np.int32).astype(np.int64)
    return np.where(b >= 0, b, -(b & 0x7FFFFFFF))


def f32_unord(o):
    o = np.asarray(o, dtype=np.int64)
    return np.where(o >= 0, o, (-o) | 0x80000000).astype(np.uint32).view(F32)


def f32_window(center, half):
    """The 2 * half + 1 consecutive fp32 values around `center` (the nextafter walk, both ways)."""
    return f32_unord(f32_ord(center) + np.arange(-half, half + 1))


def shell_values(r):
    """(fp32(r*r), the largest fp32 below it, the smallest fp32 above it): the three places a planted d2 goes."""
    thr = F32(P.r2_threshold(r).item())
    return thr, np.nextafter(thr, F32(0)), np.nextafter(thr, F32(np.inf))


# ------------------------------------------------------------------------------------------------------------ plots
def _snap(v, step):
    if step == 0.25:
        return (np.round(v / 0.25) * 0.25).astype(F32)           # exact in fp32
    if step == 0.01:
        return (np.round(v * 100) / 100).astype(F32)             # load_las_file: integer centimetres / 100, cast
    raise ValueError("step must be 0.25 or 0.01")


def lattice_plot(n, step, seed, kind="disc"):
    """(3, n) fp32: n draws from a disc of radius 10 m around the origin, snapped to `step`; 55 % with z exactly 0, the rest
    U(0, 1.5) and U(1.5, 20) as the synthetic plots.  kind: "disc", "flat" (z = 0), "line" (y = z = 0), "half" (x >= 0)."""
    g = np.random.default_rng([SEED, seed])
    rad, th = 9.75 * np.sqrt(g.random(n)), 2 * np.pi * g.random(n)        # 9.75: a snapped point stays inside the disc
    x, y = rad * np.cos(th), rad * np.sin(th)
    sel, u = g.random(n), g.random(n)
    z = np.where(sel < 0.55, 0.0, np.where(sel < 0.80, 1.5 * u, 1.5 + 18.5 * u))
    if kind == "half":
        x = np.abs(x)
    if kind in ("flat", "line"):
        z = np.zeros(n)
    if kind == "line":
        x, y = 19.5 * g.random(n) - 9.75, np.zeros(n)
    return torch.from_numpy(np.stack([_snap(x, step), _snap(y, step), _snap(z, step)]))


def pad_with_repeats(p, n, seed):
    """(3, k) -> (3, n): the k points, then n - k of them drawn with replacement (`sample_cloud` on a short plot)."""
    k = p.shape[1]
    g = torch.Generator().manual_seed(SEED * 1000 + seed)
    return torch.cat([p, p[:, torch.randint(0, k, (n - k,), generator=g)]], 1).contiguous()


def degenerate_plot(kind, n, seed):
    """(3, n) fp32.  flat / line / half: 3 n / 4, n / 3, 7 n / 8 lattice draws padded with repeats; two / one: that many
    positions and nothing else."""
    if kind == "flat":
        return pad_with_repeats(lattice_plot(3 * n // 4, 0.01, seed, "flat"), n, seed)
    if kind == "line":
        return pad_with_repeats(lattice_plot(n // 3, 0.01, seed, "line"), n, seed)
    if kind == "half":
        return pad_with_repeats(lattice_plot(7 * n // 8, 0.25, seed, "half"), n, seed)
    if kind == "two":
        return pad_with_repeats(torch.tensor([[1.25, -3.0], [-2.5, 4.75], [0.0, 1.5]]), n, seed)
    if kind == "one":
        return torch.tensor([[2.5], [-1.25], [0.75]]).expand(3, n).contiguous()
    raise ValueError(kind)


ZERO_EXTENT = {"flat": (2,), "line": (1, 2), "half": (), "two": (), "one": (0, 1, 2)}      # axes of zero extent, by kind


def distinct_positions(p):
    return int(np.unique(p.numpy().T, axis=0).shape[0])


# ------------------------------------------------------------------------------------------------------------ planted shells
_S2, _S3 = 1 / math.sqrt(2), 1 / math.sqrt(3)
SHELL_DIRS = (("x", (1, 0, 0)), ("y", (0, 1, 0)), ("z", (0, 0, 1)), ("-x", (-1, 0, 0)),                 # axis-aligned
              ("xy", (_S2, _S2, 0)), ("x-y", (_S2, -_S2, 0)), ("xyz", (_S3, _S3, _S3)), ("xz", (_S2, 0, _S2)),     # diagonal
              ("345", (0.6, 0.8, 0)), ("g1", (0.36, -0.48, 0.8)))


def _generic_dirs(n):
    v = np.random.default_rng([SEED, 99]).standard_normal((n, 3))
    return tuple((f"r{i}", tuple((v[i] / np.linalg.norm(v[i])).tolist())) for i in range(n))


SHELL_DIRS = SHELL_DIRS + _generic_dirs(14)                     # generic directions: all three coordinates round on their own
AXIS_DIRS, DIAG_DIRS = ("x", "y", "z", "-x"), ("xy", "x-y", "xyz", "xz")


def shell_point(anchor, direction, r, cls, half=1 << 14):
    """A point a + t * direction whose canonical d2 to `anchor` is shell_values(r)[cls], or None: t walks the consecutive fp32
    values around r (nextafter, `half` steps each way), the sum is rounded to fp32 per coordinate, and a candidate is accepted
    by `P.canonical_d2` itself; the step nearest r wins."""
    if half > 1 << 9:                                 # (most walks end within a few hundred steps)
        q = shell_point(anchor, direction, r, cls, 1 << 9)
        if q is not None:
            return q
    want = shell_values(r)[cls]
    a = np.asarray(anchor, dtype=np.float64)
    t = f32_window(F32(r), half).astype(np.float64)
    cand = (a[None, :] + t[:, None] * np.asarray(direction, dtype=np.float64)[None, :]).astype(F32)
    d2 = P.canonical_d2(torch.from_numpy(cand), torch.from_numpy(a.astype(F32))).numpy()
    hit = np.nonzero(d2 == want)[0]
    if hit.size == 0:
        return None
    return cand[hit[np.argmin(np.abs(hit - half))]]


def plant_shells(plot, radii, n_anchor, per_cell, seed):
    """-> (plot' (3, N), anchors (A,) point indices, planted: list of (point index, anchor index, radius, class, direction name)).
    Anchors are ground points (z = 0) within 6 m of the centre, taken from the front of the plot; for every anchor, radius and
    class, `per_cell` shell points (directions tried in a seeded order until that many are found) overwrite the plot's tail."""
    g = np.random.default_rng([SEED, seed, 1])
    p = plot.numpy().copy()
    N = p.shape[1]
    budget = n_anchor * len(radii) * 3 * per_cell
    ok = np.nonzero((p[2, :N - budget] == 0) & (p[0, :N - budget] ** 2 + p[1, :N - budget] ** 2 < 36.0))[0]
    _, first = np.unique(p[:, ok].T, axis=0, return_index=True)                  # distinct anchors
    anchors = np.sort(g.choice(ok[np.sort(first)], n_anchor, replace=False))
    planted, at = [], N - budget
    for a in anchors:
        for r in radii:
            for cls in range(3):
                found = 0
                for d in g.permutation(len(SHELL_DIRS)):
                    name, vec = SHELL_DIRS[d]
                    q = shell_point(p[:, a], vec, r, cls)
                    if q is None:
                        continue
                    p[:, at] = q
                    planted.append((at, int(a), r, cls, name))
                    at += 1
                    found += 1
                    if found == per_cell:
                        break
    return torch.from_numpy(p), torch.from_numpy(anchors), planted


def shell_pair_counts(points, centroids, r):
    """points (n, 3), centroids (m, 3) -> the number of centroid-point pairs whose canonical d2 is (equal to, one fp32 below,
    one fp32 above) fp32(r*r)."""
    d2 = P.canonical_d2(points.unsqueeze(0), centroids.unsqueeze(1)).numpy()
    return tuple(int((d2 == v).sum()) for v in shell_values(r))


@functools.lru_cache(maxsize=None)
def planted_plot(n, seed=0):
    """The 0.25 m lattice plot of n points with shells planted for all four radii (what every batch below holds as its lattice
    plot): min(14, n // 160) anchors x 4 radii x 3 classes x 4 directions overwrite at most the last 672 points."""
    return plant_shells(lattice_plot(n, 0.25, seed), RADII, min(14, n // 160), 4, seed)


def shell_level1_set(n, m):
    """(3, m) fp32, (A,) indices: a level-1 point set made of the planted plot's anchors (first) and the first m - A of its planted
    shell points -- what the second ball-query level is run on besides the real FPS samples, in which planted pairs are rare
    (both ends of a pair must have been sampled)."""
    plot, anchors, planted = planted_plot(n)
    at = torch.tensor([p[0] for p in planted][:m - anchors.numel()])
    return torch.cat([plot[:, anchors], plot[:, at]], 1).contiguous(), torch.arange(anchors.numel())


# ------------------------------------------------------------------------------------------------------------ batches
KINDS5 = ("planted", "cm", "flat", "line", "half")
KINDS3 = ("one", "two", "planted")
KINDS8 = KINDS5 + ("one", "two", "cm")
# (points, level-1 samples) of the ball-query cases; level 2 takes a quarter of level 1.  The FPS start of every plot in them:
# index 2000 (a planted point of the lattice plot, a repeat in the padded ones) / 3.  With these the planted lattice plot has
# at least 8 (FPS centroid, point) pairs in every shell class at every radius (tests/test_boundary_plots_host.py counts them).
BALL_SIZES = ((2304, 576), (2048, 512))
BALL_START, BALL_START2 = 2000, 3


def make_plot(kind, n, seed=0):
    if kind == "planted":
        return planted_plot(n)[0]
    if kind == "cm":
        return lattice_plot(n, 0.01, seed + 100)
    return degenerate_plot(kind, n, seed + 200)


@functools.lru_cache(maxsize=None)
def batch(kinds, n):
    """(B, 3, n) fp32: one plot per kind, so that a per-plot quantity that leaks between plots shows."""
    return torch.stack([make_plot(k, n, seed=i) for i, k in enumerate(kinds)]).contiguous()


def repeated_and_fresh_starts(xyz):
    """(2, B) start indices: row 0 = for every plot a point that is a repeat of an earlier point (the last one that has an equal
    in front of it; plot-wise 0 if the plot has no repeats), row 1 = a point that is the first of its position."""
    B, _, n = xyz.shape
    rep, fresh = [], []
    for b in range(B):
        _, first, inv = np.unique(xyz[b].numpy().T, axis=0, return_index=True, return_inverse=True)
        is_rep = first[inv.reshape(-1)] != np.arange(n)
        rep.append(int(np.nonzero(is_rep)[0][-1]) if is_rep.any() else 0)
        fresh.append(int(np.sort(first)[min(len(first) - 1, 1)]))
    return torch.tensor([rep, fresh])


def gather_soa(xyz, idx):
    """xyz (B, 3, n), idx (B, m) -> (B, 3, m)."""
    return torch.gather(xyz, 2, idx.unsqueeze(1).expand(-1, 3, -1)).contiguous()


def oracle_ball_lists(xyz, cpos, r, cap):
    """P.radius on a regular batch: xyz (B, 3, N), cpos (B, 3, M) -> (count per centroid (B*M,), local source indices in the
    oracle's order: centroid-major, ascending source index)."""
    B, _, N = xyz.shape
    M = cpos.shape[2]
    bx, by = torch.arange(B).repeat_interleave(N), torch.arange(B).repeat_interleave(M)
    row, col = P.radius(xyz.permute(0, 2, 1).reshape(B * N, 3), cpos.permute(0, 2, 1).reshape(B * M, 3), r, bx, by,
                        max_num_neighbors=cap)
    return torch.bincount(row, minlength=B * M), col - bx[col] * N


def oracle_knn(src, dst, k):
    """P.knn and the interpolation weights on a regular batch: src (B, 3, S), dst (B, 3, T) -> (idx (B*T, kk) local, w (B*T, kk))
    with kk = min(k, S)."""
    B, _, S = src.shape
    T = dst.shape[2]
    ps, pd = src.permute(0, 2, 1).reshape(B * S, 3), dst.permute(0, 2, 1).reshape(B * T, 3)
    bs, bd = torch.arange(B).repeat_interleave(S), torch.arange(B).repeat_interleave(T)
    yi, xi = P.knn(ps, pd, k, bs, bd)
    kk = min(k, S)
    return (xi - bs[xi] * S).view(B * T, kk), (1.0 / torch.clamp(P.canonical_d2(ps[xi], pd[yi]), min=1e-16)).view(B * T, kk)


# ------------------------------------------------------------------------------------------------------------ planted 3-NN ties
def tie_classes(src, dst):
    """src (S, 3), dst (T, 3) -> bool (T, 4): target t has the same fp32 d2 to the sources of rank (1,2), (2,3), (3,4) of the
    oracle's order AND those two sources are different positions; column 3 = the target lies on a source (d2 = 0)."""
    d2 = P.canonical_d2(src.unsqueeze(0), dst.unsqueeze(1))
    order = torch.argsort(d2, dim=1, stable=True)[:, :4]
    d = torch.gather(d2, 1, order)
    out = torch.zeros(dst.shape[0], 4, dtype=torch.bool)
    for c in range(min(3, order.shape[1] - 1)):
        differ = (src[order[:, c]] != src[order[:, c + 1]]).any(1)
        out[:, c] = (d[:, c] == d[:, c + 1]) & differ
    out[:, 3] = d[:, 0] == 0
    return out


def tie_targets(src, per_class, seed):
    """src (3, S) on the 0.25 m lattice -> (3, 4 * per_class) targets: `per_class` for each column of `tie_classes`.  Candidates
    are points of the 0.125 m lattice around random sources (every coordinate difference is a multiple of 1/8 m below 32 m: d2 is
    exact, so equal distances are equal fp32 values); the oracle's own order classifies them."""
    g = torch.Generator().manual_seed(SEED * 77 + seed)
    s = src.t().contiguous()
    S = s.shape[0]
    base = s[torch.randint(0, S, (20000,), generator=g)]
    off = torch.randint(-12, 13, (20000, 3), generator=g).float() * 0.125
    off[:, 2] *= (torch.rand(20000, generator=g) < 0.4).float()                    # most candidates stay in the source's layer
    cand = base + off
    cls = tie_classes(s, cand)
    picks = []
    for c in range(3):
        only = torch.nonzero(cls[:, c])[:, 0]
        if only.numel() < per_class:
            raise ValueError(f"tie_targets: only {only.numel()} candidates tie at rank {c + 1}/{c + 2}")
        picks.append(cand[only[:per_class]])
    picks.append(s[torch.randint(0, S, (per_class,), generator=g)])              # on a source
    return torch.cat(picks).t().contiguous()


@functools.lru_cache(maxsize=None)
def tie_case(n, m, per_class=16):
    """Sources = the oracle's m FPS samples of the planted lattice plot of n points (start 0); targets = that plot with its first
    4 * per_class points replaced by `tie_targets`.  -> (src (3, m), dst (3, n), number of planted targets)."""
    plot = planted_plot(n)[0]
    idx = P.fps_batched(plot.t().unsqueeze(0).contiguous(), m, torch.zeros(1, dtype=torch.long))
    src = plot[:, idx[0]].contiguous()
    t = tie_targets(src, per_class, seed=n)
    dst = plot.clone()
    dst[:, :t.shape[1]] = t
    return src, dst, t.shape[1]


# ------------------------------------------------------------------------------------------------------------ pixel edges
P2_BOX_X, P2_BOX_Y = (F32(-0.987708), F32(0.7049583)), (F32(-0.91008645), F32(0.8268062))       # (min, max) of the bounding-box plots


def p1_id(v):
    """The oracle's fixed-grid id of a row of values (p1_pixel_ids on both rows of a (2, n) cloud, row 0 returned)."""
    v = torch.as_tensor(np.asarray(v, dtype=F32)).reshape(1, -1)
    return projection.p1_pixel_ids(torch.cat([v, v]), D_PIX, D_METERS)[0].numpy()


def p2_id(v, box):
    """The oracle's bounding-box id of a row of values that is extended by the box's min and max (so the normalisation is the
    box's whatever the values are, as long as they lie inside)."""
    v = np.asarray(v, dtype=F32).reshape(-1)
    row = torch.from_numpy(np.concatenate([v, np.asarray(box, dtype=F32)])).reshape(1, 1, -1)
    return projection.p2_pixel_ids(torch.cat([row, row], 1), D_PIX)[0, 0, :v.size].numpy()


def _flip_point(ident, lo, hi, k):
    """The smallest fp32 in [lo, hi] whose id is >= k (ids are monotone in the value: every operation of the formula is)."""
    a, b = int(f32_ord(lo)), int(f32_ord(hi))
    assert ident(f32_unord([a]))[0] < k <= ident(f32_unord([b]))[0]
    while b - a > 1:
        mid = (a + b) // 2
        if ident(f32_unord([mid]))[0] >= k:
            b = mid
        else:
            a = mid
    return f32_unord([b])[0]


@functools.lru_cache(maxsize=None)
def p1_edge_values(half=64):
    """(19, 2 * half + 1) fp32: for every interior edge k of the fixed grid the consecutive fp32 values around the value at
    which `p1_pixel_ids` steps from k - 1 to k."""
    return np.stack([f32_window(_flip_point(p1_id, F32(-0.999), F32(0.999), k), half) for k in range(1, D_PIX)])


@functools.lru_cache(maxsize=None)
def p2_edge_values(box, half=64):
    """The same for the bounding-box grid normalised by box = (min, max)."""
    ident = functools.partial(p2_id, box=box)
    return np.stack([f32_window(_flip_point(ident, box[0], box[1], k), half) for k in range(1, D_PIX)])


def _ordinary_rows(n, g, box=None):
    """(10, n) fp32 in the format of a prepared plot: x / 10, y / 10 in the unit disc (or uniformly inside `box` = ((xmin, xmax),
    (ymin, ymax)), both extremes included, so that the rows' bounding box is the box), z / z_max, seven features."""
    c = torch.rand(10, n, generator=g)
    if box is None:
        rad, th = torch.sqrt(c[0]), 2 * math.pi * c[1]
        c[0], c[1] = rad * torch.cos(th), rad * torch.sin(th)
    else:
        for a in range(2):
            lo, hi = float(box[a][0]), float(box[a][1])
            c[a] = (lo + (hi - lo) * (0.001 + 0.998 * c[a])).clamp(lo, hi)
            c[a, 0], c[a, 1] = lo, hi
    return c


@functools.lru_cache(maxsize=None)
def pixel_edge_batch(grid, n=2500):
    """(3, 10, n) fp32 clouds whose x row (plot 0), y row (plot 1) or both rows (plot 2, under different permutations) hold the
    2451 edge values of `grid` ("p1": fixed, "p2": bounding box P2_BOX_X / P2_BOX_Y, whose extremes the plots keep at points
    0 and 1) among otherwise ordinary points."""
    g = torch.Generator().manual_seed(SEED * 31 + (1 if grid == "p1" else 2))
    box = None if grid == "p1" else (P2_BOX_X, P2_BOX_Y)
    clouds = torch.stack([_ordinary_rows(n, g, box) for _ in range(3)])
    for b, rows in enumerate(((0,), (1,), (0, 1))):
        for a in rows:
            vals = p1_edge_values() if grid == "p1" else p2_edge_values(P2_BOX_X if a == 0 else P2_BOX_Y)
            vals = torch.from_numpy(vals.reshape(-1).copy())
            assert vals.numel() <= n - 2
            where = 2 + torch.randperm(n - 2, generator=g)[:vals.numel()]
            clouds[b, a, where] = vals
    return clouds.contiguous()


def cloud_from_xyz(xyz, seed):
    """xyz (B, 3, n) metres -> (B, 10, n) prepared clouds: x / 10, y / 10, z / z_max and seven features that are a function of the
    POSITION's first occurrence, so a repeated point is a repeat in every channel, as `sample_cloud` makes it."""
    B, _, n = xyz.shape
    g = torch.Generator().manual_seed(SEED * 13 + seed)
    out = torch.empty(B, 10, n)
    for b in range(B):
        _, first, inv = np.unique(xyz[b].numpy().T, axis=0, return_index=True, return_inverse=True)
        feats = torch.rand(7, n, generator=g)
        out[b, 3:] = feats[:, torch.from_numpy(first[inv.reshape(-1)])]
    out[:, 0], out[:, 1], out[:, 2] = xyz[:, 0] / 10.0, xyz[:, 1] / 10.0, xyz[:, 2] / Z_MAX
    return out.contiguous()


# ------------------------------------------------------------------------------------------------------------ wrong variants
def ball_mask(points, centroids, r, inclusive=False):
    """bool (m, n): the oracle's membership d2 < fp32(r*r) on a dense matrix; inclusive=True is the WRONG variant `<=`."""
    d2 = P.canonical_d2(points.unsqueeze(0), centroids.unsqueeze(1))
    thr = P.r2_threshold(r)
    return d2 <= thr if inclusive else d2 < thr


def knn_dense(src, dst, k, highest=False):
    """(T, k) source indices, nearest first: a stable argsort of the dense canonical d2 (lowest index on a tie, the oracle's
    rule); highest=True is the WRONG variant in which the highest index wins a tie."""
    d2 = P.canonical_d2(src.unsqueeze(0), dst.unsqueeze(1))
    if not highest:
        return torch.argsort(d2, dim=1, stable=True)[:, :k]
    S = src.shape[0]
    return S - 1 - torch.argsort(d2.flip(1), dim=1, stable=True)[:, :k]


def p1_id_fused(v):
    """WRONG variant of the fixed-grid id: floor(fma(v + 1e-4, sf, off)) -- the product exact (fp64 holds it), ONE rounding."""
    t = (np.asarray(v, dtype=F32) + F32(0.0001)).astype(np.float64)
    s = (t * float(F32(10 * (D_PIX / D_METERS))) + float(D_METERS // 2)).astype(F32)
    return np.clip(np.floor(s), 0, D_PIX - 1).astype(np.int32)


def p2_id_premultiplied(v, box):
    """WRONG variant of the bounding-box id: floor((v - min) * (D / (max - min + 1e-4))) -- the scale formed once."""
    v = np.asarray(v, dtype=F32)
    den = (F32(box[1]) - F32(box[0])) + F32(0.0001)
    return np.floor((v - F32(box[0])) * (F32(D_PIX) / den)).astype(np.int32)


def p2_id_without_epsilon(v, box):
    """WRONG variant of the bounding-box id without the reference's + 1e-4: an axis of zero extent divides 0 by 0 (id -1 here)."""
    v = np.asarray(v, dtype=F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = (v - F32(box[0])) / (F32(box[1]) - F32(box[0])) * F32(D_PIX)
    return np.where(np.isfinite(s), np.floor(s), -1).astype(np.int32)
