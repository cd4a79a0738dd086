"""Reference and cases for the projection and loss kernels alone (csrc/project.hip, csrc/loss.hip).  Host only, numpy.
tests/test_projection_loss_ref_host.py proves on the CPU what is stated here, tests/test_gpu_projection_loss.py runs the kernels
on it.

`reference` takes the pixel ids as an INPUT and restates everything downstream of them: per (plot, cell, channel 0/2/3) the
largest value and the lowest point index that attains it, the number of occupied cells, the mean over the occupied cells, the
three loss terms of oracle/losses.py, the seven per-plot columns of sn2_plot_losses, and the analytic gradients for an upstream
gradient g.  dtype = float64 is the reference; dtype = float32 is the same text with the kernels' types (fp32 maxima, sums and
entropy; the likelihood and the absolute term in fp64 from fp32 operands, as csrc/loss.hip documents) -- its distance from the
fp64 result is `e32`, what rounding alone costs.

Cases: a shape (table below) times a value family, built once per process and never written to (the arrays are read-only).

  name          B    N       D   what only this shape reaches
  one_point_d1  2    1       1   one point, one cell; zero-extent bounding box on the xy routes
  one_point_d3  2    1       3   the same with empty cells
  three_points  3    3       2   fewer points than a wave
  ragged_cells  3    1000    17  289 cells: ragged second round of the 256-thread finalisation; discs leave the corners empty
  full_grid     3    5000    45  the LDS limit (2025 cells); plot 0 ids over all cells, plot 1 every point in cell D*D-1,
                                 plot 2 one point in each of the 2025 cells and the rest in cell 0 (nocc = 2025)
  two_slices    2    4097    20  2 key parts (per = 2049), 3 plot_losses slices (per = 1366)
  many_plots    129  64      20  second round of the 3*B loop of the last workgroup; ticket over 129 workgroups
  clamped       2    262145  45  both slice clamps (64 slices, per = 4097), R = 524 290 rows: every grid-stride tail

xy cases (one_point_*, three_points, ragged_cells) carry a cloud -- a one-position plot, three corners of a square, two discs and
a square -- and their ids are oracle.projection.p2_pixel_ids / p1_pixel_ids of it.  The other cases plant their ids: drawn from a
subset of the cells (so cells stay empty), and in two_slices and clamped the last row of the first, second and last slice of
either slicing sits alone in a cell of its own (a loop that stops one row early, or a finalisation that skips the last slice,
changes nocc).  THE KERNELS DO NOT RANGE-CHECK IDS: `_checked` asserts 0 <= id < D*D on every case before it leaves this module.

Families: `uniform` fp32 in [0, 1); `dyadic` = floor(17 u)/8 - 1, multiples of 1/8 in [-1, 1] with exact +0.0, negatives, no -0.0
and no NaN, whose fp32 sums over <= 2025 cells are exact.  On the dyadic family ties are planted in every plot that has more than
one slice: for min(8, cells that hold points of the first AND the last slice of both slicings) cells the value 1.0 (the family's
maximum) goes, in all three channels, at a point of the first and at a point of the last slice (plots 1 and 2 of full_grid have one
such cell each, by their definition), and once more at a pair n, n + 1024 of one slice (same lane, next round).

Probabilities are fp32 softmax rows with planted (0,0,0,1), (0,0,1,0), (1,0,0,0): exact 0 and 1 in the med/high columns;
`proba_zero` also has all-zero rows, for the runs without the likelihood (m = 0).  Densities are 0.05 + U in fp64; some rows hold
1e-30 (1 + U), and some 1e-60 (1 + U): an fp32 product keeps the former to 6e-8 and flushes the latter to zero, so only the latter
prove that the likelihood is formed in fp64 (the host file shows it).  gt uniform fp64, g = 1.7.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from oracle import projection

EPS = 0.0001
G = 1.7
ME = ((0.1, 0.04), (0.0, 0.04), (0.1, 0.0), (0.0, 0.0))
FAMILIES = ("uniform", "dyadic")
SHAPES = {  # name: (B, N, D, xy)
    "one_point_d1": (2, 1, 1, True),
    "one_point_d3": (2, 1, 3, True),
    "three_points": (3, 3, 2, True),
    "ragged_cells": (3, 1000, 17, True),
    "full_grid": (3, 5000, 45, False),
    "two_slices": (2, 4097, 20, False),
    "many_plots": (129, 64, 20, False),
    "clamped": (2, 262145, 45, False),
}
ALL_ME = ("ragged_cells", "two_slices")          # the cases that run all four (m, e) pairs; the others run ME[0]
CHANNELS = (0, 2, 3)


def key_parts(N):
    """SN2_P2_KEY_PARTS of include/strata_hip.h"""
    return min(max(-(-N // 4096), 1), 64)


def loss_slices(N):
    """SN2_PLOT_LOSSES_SLICES of include/strata_hip.h"""
    return min(max(-(-N // 2048), 1), 64)


def slice_of(n, N, parts):
    return np.asarray(n) // (-(-N // parts))


def me_of(name):
    return ME if name in ALL_ME else ME[:1]


# ------------------------------------------------------------------------------------------------------------ reference
def project(cov, pix, B, N, D, dtype=np.float64):
    """-> mx (B, D*D, 3) fp32 maxima (-inf where empty), arg (B, D*D, 3) int32 (-1 where empty), nocc (B,) int32,
    pred (B, 4) `dtype`.  Maxima of fp32 values are exact in either type; the sums and the quotient are in `dtype`."""
    DD = D * D
    cell = (np.arange(B)[:, None] * DD + np.asarray(pix, np.int64).reshape(B, N)).reshape(-1)
    n = np.tile(np.arange(N, dtype=np.int64), B)
    mx = np.full((3, B * DD), -np.inf, np.float32)
    arg = np.full((3, B * DD), -1, np.int32)
    for k, ch in enumerate(CHANNELS):
        v = np.ascontiguousarray(cov[:, ch])
        np.maximum.at(mx[k], cell, v)
        hit = v == mx[k][cell]
        first = np.full(B * DD, N, np.int64)
        np.minimum.at(first, cell[hit], n[hit])
        arg[k] = np.where(first == N, -1, first)
    occ = (np.bincount(cell, minlength=B * DD) > 0).reshape(B, DD)
    nocc = occ.sum(1).astype(np.int32)
    m = np.where(occ[None], mx.reshape(3, B, DD).astype(dtype), dtype(0))
    soil = np.where(occ, dtype(1) - m[0], dtype(0))
    sums = np.stack([m[0].sum(1, dtype=dtype), soil.sum(1, dtype=dtype), m[1].sum(1, dtype=dtype), m[2].sum(1, dtype=dtype)], 1)
    pred = (sums / np.maximum(nocc, 1).astype(dtype)[:, None]).astype(dtype)
    return dict(mx=mx.reshape(3, B, DD).transpose(1, 2, 0).copy(), arg=arg.reshape(3, B, DD).transpose(1, 2, 0).copy(),
                nocc=nocc, pred=pred)


def raster(cov, cell, B, N, D):
    """P1: (B, 3, D, D) fp32 [low, med, high] maxima on cell = y_pix*D + x_pix, NaN where empty, rows flipped."""
    mx = project(cov, cell, B, N, D)["mx"]                       # (B, D*D, 3)
    img = np.where(np.isinf(mx), np.float32(np.nan), mx).transpose(0, 2, 1).reshape(B, 3, D, D)
    return img[:, :, ::-1, :].copy()


def _rows(proba, pdf, m, e, dtype):
    """per-row -log likelihood (R,) fp64 and entropy terms (R, 2) fp64, None where the term is off"""
    f32 = dtype == np.float32
    nll = ent = None
    if m != 0.0:
        pg = (proba[:, 0] + proba[:, 1]).astype(np.float64) if f32 else proba[:, 0].astype(np.float64) + proba[:, 1].astype(np.float64)
        lik = (pg * pdf[:, 0] + proba[:, 2].astype(np.float64) * pdf[:, 1]) + proba[:, 3].astype(np.float64) * pdf[:, 2]
        nll = -np.log(lik)
    if e != 0.0:
        p, eps, one = proba[:, 2:].astype(dtype), dtype(EPS), dtype(1)
        ent = (-(p * np.log(p + eps) + (one - p) * np.log(one - p + eps))).astype(np.float64)
    return nll, ent


def losses(pred, proba, pdf, gt, B, N, m, e, dtype=np.float64):
    """-> out (4,) = total, absolute, NLL, entropy over the batch; plots (B, 7) = total, absolute, NLL, entropy, abs_low, abs_med,
    abs_high of every plot alone.  A term whose weight is zero is exactly 0.0.  The entropy is an fp32 number when dtype is."""
    d = pred.astype(np.float64)[:, CHANNELS] - gt[:, CHANNELS]
    ab = np.sqrt(d * d + EPS)                                     # (B, 3)
    nll, ent = _rows(proba, pdf, m, e, dtype)
    R = B * N
    rnd = (lambda x: np.asarray(x, np.float64).astype(np.float32).astype(np.float64)) if dtype == np.float32 else np.asarray
    l_abs = ab.sum() / (3.0 * B)
    l_nll = nll.sum() / R if nll is not None else 0.0
    l_ent = float(rnd(ent.sum() / (2.0 * R))) if ent is not None else 0.0
    out = np.array([l_abs + m * l_nll + e * l_ent, l_abs, l_nll, l_ent])
    p_abs = ab.sum(1) / 3.0
    p_nll = nll.reshape(B, N).sum(1) / N if nll is not None else np.zeros(B)
    p_ent = rnd(ent.reshape(B, -1).sum(1) / (2.0 * N)) if ent is not None else np.zeros(B)
    plots = np.concatenate([(p_abs + m * p_nll + e * p_ent)[:, None], p_abs[:, None], p_nll[:, None], p_ent[:, None], ab], 1)
    return out, plots


def project_backward(dpred, arg, nocc, pix, B, N, D, dtype=np.float64):
    """d / d coverages (B*N, 4) of the projection for d / d pred (B, 4): a cell's gradient goes to its arg-max point only,
    (g0 - g1) / nocc on channel 0 (low vegetation also feeds bare soil = 1 - low), nothing on channel 1."""
    dpred = np.asarray(dpred, dtype)
    a = np.asarray(arg).reshape(B, D * D, 3)[np.arange(B)[:, None], np.asarray(pix, np.int64).reshape(B, N)]   # (B, N, 3)
    own = a == np.arange(N)[None, :, None]
    nn = np.maximum(nocc, 1).astype(dtype)
    g = np.stack([dpred[:, 0] - dpred[:, 1], dpred[:, 2], dpred[:, 3]], 1)
    per = g * (dtype(1) / nn)[:, None] if dtype == np.float32 else g / nn[:, None]
    out = np.zeros((B, N, 4), dtype)
    for k, ch in enumerate(CHANNELS):
        out[:, :, ch] = np.where(own[:, :, k], per[:, None, k], dtype(0))
    return out.reshape(B * N, 4)


def loss_backward(pred, proba, pdf, gt, B, N, m, e, g, dtype=np.float64):
    """-> dpred (B, 4), dproba (B*N, 4) of g * total at the GIVEN pred (fp64 arithmetic on it; the results are `dtype`)"""
    R = B * N
    d = pred.astype(np.float64) - gt
    dpred = g * d / np.sqrt(d * d + EPS) / (3.0 * B)
    dpred[:, 1] = 0.0
    dproba = np.zeros((R, 4))
    if m != 0.0:
        f32 = dtype == np.float32
        pg = (proba[:, 0] + proba[:, 1]).astype(np.float64) if f32 else proba[:, 0].astype(np.float64) + proba[:, 1].astype(np.float64)
        lik = (pg * pdf[:, 0] + proba[:, 2].astype(np.float64) * pdf[:, 1]) + proba[:, 3].astype(np.float64) * pdf[:, 2]
        il = -(g * m / R) / lik
        dproba[:, 0] = dproba[:, 1] = il * pdf[:, 0]
        dproba[:, 2] = il * pdf[:, 1]
        dproba[:, 3] = il * pdf[:, 2]
    if e != 0.0:
        p, eps, one = proba[:, 2:].astype(dtype), dtype(EPS), dtype(1)
        h = -(np.log(p + eps) + p / (p + eps) - np.log(one - p + eps) - (one - p) / (one - p + eps))
        dproba[:, 2:] += (g * e / (2.0 * R)) * h.astype(np.float64)
    return dpred.astype(dtype), dproba.astype(dtype)


def reference(cov, pix, proba, pdf, gt, B, N, D, m, e, g, dtype=np.float64):
    """Everything downstream of the pixel ids (module docstring).  -> dict: mx, arg, nocc, pred, out (4,), plots (B, 7), dpred,
    dcov, dproba."""
    r = project(cov, pix, B, N, D, dtype)
    r["out"], r["plots"] = losses(r["pred"], proba, pdf, gt, B, N, m, e, dtype)
    r["dpred"], r["dproba"] = loss_backward(r["pred"], proba, pdf, gt, B, N, m, e, g, dtype)
    r["dcov"] = project_backward(r["dpred"], r["arg"], r["nocc"], pix, B, N, D, dtype)
    return r


def backward_from(pred_in, arg, nocc, case, m, e, g, dtype=np.float64):
    """The backward entry points' reference: the gradients at a GIVEN fp32 pred (the absolute term's derivative has slope
    100 at pred = gt, so a backward is judged from the pred it is handed).  -> dpred, dcov, dproba."""
    c = case
    dpred, dproba = loss_backward(np.asarray(pred_in), c.proba_for(m), c.pdf, c.gt, c.B, c.N, m, e, g, dtype)
    return dpred, project_backward(dpred, arg, nocc, c.pix, c.B, c.N, c.D, dtype), dproba


def dist(a, b):
    """largest |a - b| over the largest |b| (b: the fp64 side); 0 for two all-zero tensors"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    s = float(np.abs(b).max()) if b.size else 0.0
    d = float(np.abs(a - b).max()) if b.size else 0.0
    return d / s if s > 0 else d


# ----------------------------------------------------------------------------------------------------------------- cases
def _values(rng, R, family):
    u = rng.random((R, 4), dtype=np.float32)
    return u if family == "uniform" else (np.floor(u * np.float32(17)) / np.float32(8) - np.float32(1)).astype(np.float32)


def _discs(rng, B, N, square=()):
    """(B, 3, N) fp32: x, y in the unit disc (plots in `square`: in [-1, 1]^2), z uniform"""
    cl = np.empty((B, 3, N), np.float32)
    for b in range(B):
        if b in square:
            xy = rng.random((2, N)) * 2 - 1
        else:
            r, t = np.sqrt(rng.random(N)), rng.random(N) * 2 * np.pi
            xy = np.stack([r * np.cos(t), r * np.sin(t)])
        cl[b, :2], cl[b, 2] = xy, rng.random(N)
    return cl


def _cloud(rng, name, B, N):
    if name.startswith("one_point"):
        cl = np.zeros((B, 3, 1), np.float32)
        cl[:, 0, 0], cl[:, 1, 0] = (0.25, -0.5), (0.75, 0.125)
        return cl
    if name == "three_points":
        cl = np.zeros((B, 3, 3), np.float32)
        cl[:, 0], cl[:, 1] = (-1.0, 1.0, 1.0), (-1.0, -1.0, 1.0)          # three corners of a square: one cell of four is empty
        cl[1, :2] *= 0.5
        cl[2, 0] += 0.25
        return cl
    return _discs(rng, B, N, square=(2,))


def _planted_ids(rng, name, B, N, D):
    DD = D * D
    pix = np.empty((B, N), np.int64)
    if name == "full_grid":
        pix[0] = rng.integers(0, DD, N)
        pix[0, 10 + 1024] = pix[0, 10]
        pix[1] = DD - 1
        pix[2, :DD], pix[2, DD:] = np.arange(DD), 0
        return pix
    for b in range(B):
        order = rng.permutation(DD)
        n_free = (DD * 4) // 5
        pix[b] = order[rng.integers(0, n_free, N)]
        if N > 1034:
            pix[b, 10 + 1024] = pix[b, 10]                               # same lane, next round of one slice
        if key_parts(N) > 1:
            last = set()
            for parts in (key_parts(N), loss_slices(N)):
                per = -(-N // parts)
                last |= {min(N, (q + 1) * per) - 1 for q in (0, 1, parts - 1)}
            for k, n in enumerate(sorted(last)):
                pix[b, n] = order[n_free + k]                            # alone in a cell nothing else is drawn from
    return pix


def _plant_ties(cov, pix, B, N):
    """value 1.0 in all three channels at a point of the first and a point of the last slice (of both slicings) of up to 8
    cells per plot, and at one pair n, n + 1024 inside one slice"""
    kp, ls = key_parts(N), loss_slices(N)
    n = np.arange(N)
    first = (slice_of(n, N, kp) == 0) & (slice_of(n, N, ls) == 0)
    last = (slice_of(n, N, kp) == kp - 1) & (slice_of(n, N, ls) == ls - 1)
    v = cov.reshape(B, N, 4)
    for b in range(B):
        in_last = {}
        for i in n[last][::-1]:
            in_last[int(pix[b, i])] = int(i)
        done = set()
        for i in n[first]:
            c = int(pix[b, i])
            if c in in_last and c not in done:
                v[b, i, :] = 1.0
                v[b, in_last[c], :] = 1.0
                done.add(c)
                if len(done) == 8:
                    break
        assert done, "no cell holds points of the first and of the last slice"
        i, j = n[:-1024], n[1024:]
        same = (pix[b, i] == pix[b, j]) & (slice_of(i, N, kp) == slice_of(j, N, kp)) & (slice_of(i, N, ls) == slice_of(j, N, ls))
        pair = int(np.flatnonzero(same)[0])
        v[b, pair, :] = 1.0
        v[b, pair + 1024, :] = 1.0


def _proba(rng, R, zeros):
    p = torch.softmax(torch.from_numpy(rng.standard_normal((R, 4)).astype(np.float32)), 1).numpy().copy()
    rows = ((0, 0, 0, 1), (0, 0, 1, 0), (1, 0, 0, 0)) + (((0, 0, 0, 0),) if zeros else ())
    for k, row in enumerate(rows):
        p[k::11][: max(1, R // 40)] = row                                # (with R = 2: row k of the first two kinds)
    return p


def _checked(c):
    assert c.pix.dtype == np.int32 and c.pix.shape == (c.B * c.N,)
    assert int(c.pix.min()) >= 0 and int(c.pix.max()) < c.D * c.D, "a pixel id outside the grid must never reach a kernel"
    if c.cell1 is not None:
        assert int(c.cell1.min()) >= 0 and int(c.cell1.max()) < c.D * c.D
    assert np.isfinite(c.cov).all() and not (np.signbit(c.cov) & (c.cov == 0)).any(), "the tie rule is stated for finite values, no -0.0"
    for a in (c.cov, c.pix, c.proba, c.proba_zero, c.pdf, c.gt) + ((c.cloud, c.cell1) if c.cloud is not None else ()):
        a.flags.writeable = False
    return c


@functools.lru_cache(maxsize=None)
def case(name, family):
    B, N, D, xy = SHAPES[name]
    R = B * N
    rng = np.random.default_rng([sorted(SHAPES).index(name), FAMILIES.index(family), 20])
    c = SimpleNamespace(name=name, family=family, B=B, N=N, D=D, R=R, cloud=None, cell1=None, diam_meters=D)
    c.cov = _values(rng, R, family)
    if xy:
        c.cloud = _cloud(rng, name, B, N)
        t = torch.from_numpy(c.cloud)
        p2 = projection.p2_pixel_ids(t, D).numpy().astype(np.int64)
        pix = p2[:, 0] * D + p2[:, 1]
        p1 = np.stack([projection.p1_pixel_ids(t[b], D, c.diam_meters).numpy().astype(np.int64) for b in range(B)])
        c.cell1 = (p1[:, 1] * D + p1[:, 0]).reshape(-1).astype(np.int32)
    else:
        pix = _planted_ids(rng, name, B, N, D)
    if family == "dyadic" and key_parts(N) > 1:
        _plant_ties(c.cov, pix, B, N)
    c.pix = pix.reshape(-1).astype(np.int32)
    c.proba, c.proba_zero = _proba(rng, R, False), _proba(rng, R, True)
    c.pdf = 0.05 + rng.random((R, 3))
    for start, tiny in ((5, 1e-30), (7, 1e-60)):
        rows = c.pdf[start::13][: max(1, R // 50)]                       # (a view: written in place)
        rows[:] = tiny * (1 + rng.random(rows.shape))
    c.gt = rng.random((B, 4))
    c.proba_for = lambda m: c.proba if m != 0.0 else c.proba_zero
    return _checked(c)


@functools.lru_cache(maxsize=None)
def ref(name, family, m=ME[0][0], e=ME[0][1], f32=False):
    """`reference` of a case, computed once per process and never changed"""
    c = case(name, family)
    return reference(c.cov, c.pix, c.proba_for(m), c.pdf, c.gt, c.B, c.N, c.D, m, e, G, np.float32 if f32 else np.float64)


@functools.lru_cache(maxsize=None)
def ref_backward(name, family, m=ME[0][0], e=ME[0][1], f32=False):
    """(pred32, dpred, dcov, dproba): the gradients at the fp64 pred rounded to fp32, from the reference's arg and nocc"""
    c, r = case(name, family), ref(name, family, m, e)
    pred32 = r["pred"].astype(np.float32)
    return (pred32,) + backward_from(pred32, r["arg"], r["nocc"], c, m, e, G, np.float32 if f32 else np.float64)


def case_ids():
    return [(n, f) for n in SHAPES for f in FAMILIES]
