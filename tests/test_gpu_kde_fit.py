"""Fitting the KDE mixture on the device (csrc/kde.hip: sn2_kde_fit; `hip_ops.kde_fit`, `losses.KdeTables.fit`, `sample_heights`).

The device tables are held to `fit_tables` of tests/test_kde_fit_host.py -- the fp64 numpy restatement of the estimator the header
writes out -- on the same fp32 heights.  There is no fixture from the reference: its fit needs KDEpy's `FFTKDE`
(`learning/kde_mixture.py:60-62`), which this project's tests cannot run, so no reference-fitted table can be recorded.

Tolerance: |Y_dev - Y_ref| <= 1e-9 * Y_ref + 1e-12, X equal to one ulp.  Both sides form the same terms (same bin indices, same
fractions: IEEE fp64 operations in the same order); they differ in the ORDER of fp64 sums of at most 2n non-negative terms, which
is worth <= 2n * 2^-53 relative (4.4e-11 at n = 200 000), and in a few ulp of `exp`.
"""
import functools

import numpy as np
import pytest
import torch
from scipy.interpolate import interp1d

from stratanet2_vegetation_coverage_maps_amd import PointNet2, evaluation as ev
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
from stratanet2_vegetation_coverage_maps_amd import losses as dev_losses
from stratanet2_vegetation_coverage_maps_amd._lib import StrataHipError
from stratanet2_vegetation_coverage_maps_amd.synthetic import Z_MAX, make_args, make_batch
from test_kde_fit_host import fit_tables, synthetic_heights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def heights(case):
    """the fp32 heights of a case (read-only: shared by every test that names the case)"""
    if case == "n1":
        z = np.array([0.0], np.float32)                                   # zm = 0: the grid is [-5 bw, 5 bw]
    elif case == "n2":
        z = np.array([0.3, 7.25], np.float32)
    elif case in ("n63", "n64", "n65"):
        z = synthetic_heights(int(case[1:]), 5)
    elif case == "equal":
        z = np.full(1000, 2.7182817, np.float32)
    elif case == "negmax":                                                # negative heights, one of them the largest |z|
        z = synthetic_heights(777, 6)
        z[::3] *= -1.0
        z[300] = -23.5
    elif case == "n20005":                                                # exact 0, 0.5, 1.5 and the maximum twice
        z = np.concatenate([synthetic_heights(20000, 7), np.array([0.0, 0.5, 1.5, 21.25, 21.25], np.float32)])
    elif case in ("n32768", "n32769"):                                    # the last n binned as one slice, the first as two
        z = synthetic_heights(int(case[1:]), 9)
    elif case == "n200000":                                               # seven slices, the last one short
        z = synthetic_heights(200000, 8)
    else:
        raise KeyError(case)
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def reference(case, K, bw):
    X, Y = fit_tables(heights(case), bw, K)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


def device_fit(case, K=5000, bw=0.1):
    X, Y = ops.kde_fit(torch.from_numpy(heights(case).copy()).to(DEV), bw, K)
    torch.cuda.synchronize()
    return X.cpu().numpy(), Y.cpu().numpy()


CASES = [(c, 5000, 0.1) for c in ("n1", "n2", "n63", "n64", "n65", "equal", "negmax", "n20005", "n32768", "n32769",
                                     "n200000")]
CASES += [("n20005", K, 0.1) for K in (2, 64, 512, 4999, 5001)]
CASES += [("n20005", 5000, 0.5), ("n20005", 64, 0.5), ("n65", 4999, 0.5), ("n1", 2, 0.1)]


@pytest.mark.parametrize("case,K,bw", CASES)
def test_device_tables_vs_the_restated_estimator(case, K, bw):
    Xr, Yr = reference(case, K, bw)
    X, Y = device_fit(case, K, bw)
    assert X.shape == Xr.shape and Y.shape == Yr.shape and X.dtype == np.float64 and Y.dtype == np.float64
    ex = float((np.abs(X - Xr) / np.spacing(np.abs(Xr))).max())
    excess = np.abs(Y - Yr) - (1e-9 * Yr + 1e-12)
    rel = float((np.abs(Y - Yr) / np.maximum(Yr, 1e-300))[Yr > 1e-3].max())
    print(f"\n{case} K={K} bw={bw}: X off by {ex:.1f} ulp at most; max |dY| {np.abs(Y - Yr).max():.3e}, "
          f"max |dY|/Y (Y > 1e-3) {rel:.3e}, worst excess over the bound {excess.max():.3e}")
    assert np.isfinite(Y).all() and ex <= 1.0
    assert (excess <= 0).all()
    assert Y.max() == 1.0 and X[0] <= -float(np.abs(heights(case)).max())


def test_same_bytes_every_call_and_from_a_replayed_graph():
    z = torch.from_numpy(heights("n200000").copy()).to(DEV)
    runs = [ops.kde_fit(z) for _ in range(3)]
    torch.cuda.synchronize()
    X0, Y0 = runs[0]
    for X, Y in runs[1:]:
        assert torch.equal(X, X0) and torch.equal(Y, Y0)
    graph = torch.cuda.CUDAGraph()
    with ops.graph_capture(graph, DEV):
        Xg, Yg = ops.kde_fit(z)
    for _ in range(2):
        Xg.zero_()
        Yg.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(Xg, X0) and torch.equal(Yg, Y0)


@pytest.mark.parametrize("case", ["n20005", "negmax", "n1"])
def test_fitted_heights_look_up_without_nan_and_as_scipy_does(case):
    """`kde_densities` over FITTED tables: the grid covers every fitted height, and the lookup keeps its contract (scipy's
    interp1d over the same tables, bit for bit)."""
    z = heights(case)
    tables = dev_losses.KdeTables.fit(z, DEV)
    cloud = torch.zeros(1, 3, z.size)
    cloud[0, 2] = torch.from_numpy(z.copy()) / Z_MAX                       # what the loader hands over: z rescaled
    pdf = dev_losses.kde_densities(cloud.to(DEV), Z_MAX, tables).cpu().numpy()
    assert pdf.shape == (z.size, 3) and not np.isnan(pdf).any()
    X, Y = tables.X.cpu().numpy(), tables.Y.cpu().numpy()
    zz = (cloud[0, 2] * Z_MAX).numpy().astype(np.float64)                  # fp32 product, widened: sn2_kde_lookup's height
    want = np.stack([interp1d(X, Y[k], kind="linear", assume_sorted=False)(zz) for k in range(3)], 1)
    assert np.array_equal(pdf, want)


def test_sample_heights():
    g = torch.Generator().manual_seed(9)
    plots = [torch.rand(10, n, generator=g) for n in (5000, 1, 7001, 3000)]
    off = 0
    for p in plots:                                                       # distinct heights: a value names its index
        p[2] = (off + torch.arange(p.shape[1], dtype=torch.float32)) * 0.25
        off += p.shape[1]
    allz = torch.cat([p[2] for p in plots])
    a = dev_losses.sample_heights(plots, size=4096, seed=11, device=DEV)
    b = dev_losses.sample_heights(plots, size=4096, seed=11, device=DEV)
    c = dev_losses.sample_heights(plots, size=4096, seed=12, device=DEV)
    assert a.is_cuda and a.dtype == torch.float32 and a.shape == (4096,)
    assert torch.equal(a, b) and not torch.equal(a, c)
    av = a.cpu().numpy()
    assert np.unique(av).size == 4096 and np.isin(av, allz.numpy()).all()
    assert np.isin(c.cpu().numpy(), allz.numpy()).all() and np.unique(c.cpu().numpy()).size == 4096
    # a uniform draw reaches every plot and is not a prefix
    assert av.max() > allz.numpy()[12000] and not np.array_equal(np.sort(av), allz.numpy()[:4096])
    # ONE resident (C, T) array with offsets is the same population: the same draw
    raw = torch.cat(plots, 1).to(DEV)
    offsets = torch.tensor([0, 5000, 5001, 12002, 15002], dtype=torch.int32, device=DEV)
    assert torch.equal(dev_losses.sample_heights(raw, size=4096, seed=11, offsets=offsets, device=DEV), a)
    # more candidates than sn2_subsample keeps in LDS (its four-launch form, what a real dataset takes)
    big = (torch.arange(40000, dtype=torch.float32) * 0.5).reshape(1, -1).repeat(3, 1)
    d1 = dev_losses.sample_heights(big, size=10000, seed=5, device=DEV).cpu().numpy()
    d2 = dev_losses.sample_heights([big[:, :123], big[:, 123:]], size=10000, seed=5, device=DEV).cpu().numpy()
    assert ops.subsample_form(40000, 10000) == ops.SUBSAMPLE_GLOBAL and ops.subsample_form(15002, 4096) == ops.SUBSAMPLE_LDS
    assert np.array_equal(d1, d2) and np.unique(d1).size == 10000 and np.isin(d1, big[2].numpy()).all() and d1.max() > 15000.0
    # fewer heights than `size`: all of them
    few = dev_losses.sample_heights(plots, size=500_000, seed=11, device=DEV)
    assert torch.equal(few.cpu(), allz)
    tables = dev_losses.KdeTables.from_plots(plots, DEV, size=4096, seed=11)
    direct = dev_losses.KdeTables.fit(a, DEV)
    assert torch.equal(tables.X, direct.X) and torch.equal(tables.Y, direct.Y)


def test_fitted_tables_through_evaluate():
    """`KdeTables.fit` -> `evaluate(model, batches, args, kde=...)` with args.m = 1 on 4 plots x 1024 points: finite losses, and
    the bytes of the same tables handed over through the plain constructor."""
    P, N = 4, 1024
    args = make_args(subsample_size=N, ratio1=0.25, r1=1.0, ratio2=0.25, r2=2.0, m=1.0)
    args.cuda = 0
    args.current_step_in_fold = 0
    torch.manual_seed(3)
    model = PointNet2(args).eval()
    d = make_batch(P, N, first_plot=40)

    fs = torch.stack([torch.arange(P) * 5 % N, torch.arange(P) * 3 % 40])   # fixed FPS starts: without them they are drawn

    def batches():
        return [{"cloud": d["cloud"][s:s + 2], "xyz": d["xyz"][s:s + 2], "coverages": d["coverages"][s:s + 2],
                 "plot_id": [f"plot_{s + i}" for i in range(2)], "fps_start": fs[:, s:s + 2]} for s in (0, 2)]

    tables = dev_losses.KdeTables.fit(d["xyz"][:, 2], DEV)                 # heights in metres, (4, 1024) on the host
    a, _ = ev.evaluate(model, batches(), args, kde=tables)
    X, Y = tables.X.cpu().numpy(), tables.Y.cpu().numpy()
    plain = dev_losses.KdeTables(X, Y[0], Y[1], Y[2], DEV)
    assert torch.equal(plain.X, tables.X) and torch.equal(plain.Y, tables.Y)
    b, _ = ev.evaluate(model, batches(), args, kde=plain)
    rows = a["per_plot"]["losses"]
    assert rows.shape == (P, 7) and np.isfinite(rows).all() and (rows[:, 2] != 0).all()
    assert np.array_equal(rows, b["per_plot"]["losses"]) and np.array_equal(a["per_plot"]["pred"], b["per_plot"]["pred"])


def test_invalid_input():
    z = torch.from_numpy(heights("n65").copy())
    for bad in (float("nan"), float("inf"), -float("inf")):
        zb = z.clone()
        zb[7] = bad
        with pytest.raises(ValueError, match="finite"):
            dev_losses.KdeTables.fit(zb, DEV)
        with pytest.raises(ValueError, match="finite"):
            dev_losses.KdeTables.fit(zb.to(DEV), DEV)
    with pytest.raises(StrataHipError, match="SN2_EINVAL"):                # the library's argument code, nothing launched
        ops.kde_fit(torch.empty(0, dtype=torch.float32, device=DEV))
    for K in (1, 0, -3):
        with pytest.raises(StrataHipError, match="SN2_EINVAL"):
            ops.kde_fit(z.to(DEV), 0.1, K)
    with pytest.raises(StrataHipError, match="SN2_EINVAL"):
        ops.kde_fit(z.to(DEV), 0.0)
    with pytest.raises(StrataHipError, match="SN2_ELIMIT"):
        ops.kde_fit(z.to(DEV), 0.1, ops.KDE_FIT_MAX_K + 1)
    with pytest.raises(ValueError):
        ops.kde_fit(z.to(DEV).double())
    with pytest.raises(ValueError):
        ops.kde_fit(z)                                                     # a host tensor
