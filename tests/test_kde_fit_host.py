"""The estimator behind `KdeTables.fit` (include/strata_hip.h: sn2_kde_fit), restated in fp64 numpy and checked on the CPU.

`fit_tables(z, bw, K)` is what the device tables are held to (tests/test_gpu_kde_fit.py).  It is a restatement of the header's
text, NOT a fixture from the reference: the reference fits with KDEpy's `FFTKDE` (`learning/kde_mixture.py:60-62`), KDEpy is not
available to this project's tests, so no table the reference fitted can be recorded.  What can be checked without it is checked
here: the weight rule against the values the reference's three lambdas give (`kde_mixture.py:54-58`, written out by hand), the
grid, and the binned-and-truncated estimate against the exact weighted Gaussian sum it approximates.
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from conftest import ROOT
from stratanet2_vegetation_coverage_maps_amd import _lib
from stratanet2_vegetation_coverage_maps_amd.hip_ops import KDE_FIT_MAX_K, kde_fit, kde_fit_ws_words          # noqa: F401
from stratanet2_vegetation_coverage_maps_amd.losses import KdeTables, sample_heights
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_plot

FIT_ARGTYPES = _lib.SIGNATURES["sn2_kde_fit"]
assert callable(KdeTables.fit) and callable(KdeTables.from_plots) and callable(sample_heights)


def synthetic_heights(n, seed=0):
    """n fp32 heights in metres from the mixture of synthetic.py (55 % ground, 25 % U(0,1.5), 20 % U(1.5,20))"""
    return make_plot(int(n), 20211007 + int(seed))[1][2].numpy().astype(np.float32).copy()


def strata_weights(a):
    """(3, m) weights of sample points with |z| = a (fp64): the rule of the header, strict inequalities"""
    a = np.asarray(a, dtype=np.float64)
    w1 = np.where(a < 0.5, 1.0, 0.05)
    w2 = np.where((0.5 < a) & (a < 1.5), 1.0, 0.05)
    w3 = np.where(1.5 < a, 1.0, np.where(0.5 < a, 0.5, 0.05))
    return np.stack([w1, w2, w3])


def fit_tables(z, bw=0.1, K=5000, details=False):
    """-> X (K), Y (3,K) fp64: symmetrise, weight, grid, linear binning, truncated Gaussian, one common maximum."""
    z32 = np.asarray(z, dtype=np.float32).reshape(-1)
    assert z32.size >= 1 and K >= 2 and np.isfinite(z32).all()
    z64 = z32.astype(np.float64)
    s = np.concatenate([-z64, z64])
    w = strata_weights(np.abs(s))
    zm = float(np.abs(z64).max())
    A = zm + max(0.05 * 2 * zm, 5 * bw)
    X = np.linspace(-A, A, K)
    dx = 2 * A / (K - 1)
    t = (s - X[0]) / dx
    j = np.minimum(np.floor(t).astype(np.int64), K - 2)
    f = t - j
    bins = np.stack([np.bincount(j, weights=wk * (1 - f), minlength=K) + np.bincount(j + 1, weights=wk * f, minlength=K) for wk in w])
    L = int(min(np.floor(5 * bw / dx), K - 1))
    u = np.arange(-L, L + 1) * dx
    g = np.exp(-u ** 2 / (2 * bw ** 2)) / (bw * np.sqrt(2 * np.pi))
    raw = np.stack([np.convolve(b, g)[L:L + K] for b in bins])          # "same" size as the grid, zero outside it
    Y = raw / raw.max()
    if details:
        return X, Y, dict(A=A, dx=dx, L=L, bins=bins, g=g, raw=raw)
    return X, Y


def exact_tables(z, X, bw=0.1, chunk=250):
    """the three weighted Gaussian sums at every grid point -- no binning, no truncation --, over their common maximum"""
    z64 = np.asarray(z, dtype=np.float32).astype(np.float64).reshape(-1)
    s = np.concatenate([-z64, z64])
    w = strata_weights(np.abs(s))
    Y = np.empty((3, X.size))
    for i in range(0, X.size, chunk):
        k = np.exp(-(X[i:i + chunk, None] - s[None, :]) ** 2 / (2 * bw ** 2)) / (bw * np.sqrt(2 * np.pi))
        Y[:, i:i + chunk] = w @ k.T
    return Y / Y.max()


def test_weight_rule_at_the_strata_limits():
    """a = 0, 0.5 -/+ one fp32 ulp, 0.5, 1.5 -/+ one fp32 ulp, 1.5 and 20: what `1 if abs(x) < 0.5 else 0.05`,
    `1 if 0.5 < abs(x) < 1.5 else 0.05` and `1 if 1.5 < abs(x) else 0.5 if 0.5 < abs(x) else 0.05` give there."""
    f32 = np.float32
    below = lambda v: np.nextafter(f32(v), f32(-np.inf))
    above = lambda v: np.nextafter(f32(v), f32(np.inf))
    a = np.array([0.0, below(0.5), 0.5, above(0.5), below(1.5), 1.5, above(1.5), 20.0], dtype=np.float32)
    want = np.array([[1, .05, .05], [1, .05, .05], [.05, .05, .05], [.05, 1, .5], [.05, 1, .5], [.05, .05, .5], [.05, .05, 1],
                     [.05, .05, 1]]).T
    assert np.array_equal(strata_weights(a.astype(np.float64)), want)
    # and through the whole fit: one height alone puts its weights' ratio into the tables' peaks
    for h, row in zip(a, want.T):
        _, Y = fit_tables([h])
        assert np.allclose(Y.max(1) / Y.max(), row / row.max(), rtol=1e-12)


def test_grid_covers_the_data_and_is_symmetric():
    for z in (synthetic_heights(3000, 1), np.array([0.0], np.float32), -synthetic_heights(100, 2), np.full(7, 3.25, np.float32)):
        for K in (2, 64, 4999, 5000):
            X, Y, d = fit_tables(z, K=K, details=True)
            zm = float(np.abs(z).max())
            assert X.shape == (K,) and Y.shape == (3, K)
            assert X[0] <= -zm and X[-1] >= zm and X[0] == -X[-1] and (np.diff(X) > 0).all()
            assert np.abs(X + X[::-1]).max() <= 4 * np.spacing(d["A"])          # i*dx, its sum with -A and dx: half an ulp of 2A each
            assert Y.max() == 1.0 and (Y >= 0).all()
            assert d["A"] >= zm + 0.5 - 1e-12


def test_binned_and_truncated_vs_exact():
    z = synthetic_heights(5000, 3)
    X, Y, d = fit_tables(z, 0.1, 5000, details=True)
    Ye = exact_tables(z, X, 0.1)
    err, bound = float(np.abs(Y - Ye).max()), (d["dx"] / 0.1) ** 2 / 8 + 1e-5
    print(f"\nbinned vs exact: max |dY| {err:.3e}, bound {bound:.3e} (dx {d['dx']:.4f}, L {d['L']})")
    assert err <= bound


def test_coarse_grid_is_the_scaled_histogram():
    z = synthetic_heights(3000, 4)
    X, Y, d = fit_tables(z, 0.1, 64, details=True)
    assert d["dx"] > 5 * 0.1 and d["L"] == 0 and d["g"].shape == (1,)
    assert np.allclose(Y, d["bins"] / d["bins"].max(), rtol=1e-14, atol=0)
    assert np.allclose(d["bins"].sum(1), strata_weights(np.abs(np.concatenate([-z, z]).astype(np.float64))).sum(1), rtol=1e-12)


def test_workspace_macro_matches_the_binding():
    src = ('#include <stdio.h>\n#include "strata_hip.h"\nint main(){printf("%zu %zu %zu %d\\n", (size_t)SN2_KDE_FIT_WS_WORDS(2),'
           '(size_t)SN2_KDE_FIT_WS_WORDS(5000), (size_t)SN2_KDE_FIT_WS_WORDS(65536), SN2_KDE_FIT_MAX_K);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [kde_fit_ws_words(2), kde_fit_ws_words(5000), kde_fit_ws_words(65536), KDE_FIT_MAX_K]


def test_argument_checks_return_before_any_device_work():
    lib = _lib.load()
    fake = 0x1000                                            # never dereferenced: every call below fails a check first
    fn = lib.sn2_kde_fit
    assert fn(fake, 0, 0.1, 5000, fake, fake, fake, None) == -1          # no heights
    assert fn(None, 10, 0.1, 5000, fake, fake, fake, None) == -1
    assert fn(fake, 10, 0.1, 1, fake, fake, fake, None) == -1            # a grid needs two points
    assert fn(fake, 10, 0.0, 5000, fake, fake, fake, None) == -1         # bandwidth
    assert fn(fake, 10, float("nan"), 5000, fake, fake, fake, None) == -1
    assert fn(fake, 10, 0.1, 5000, fake + 4, fake, fake, None) == -1     # workspace alignment
    assert fn(fake, 10, 0.1, KDE_FIT_MAX_K + 1, fake, fake, fake, None) == -2
    assert fn(fake, 2 ** 31, 0.1, 5000, fake, fake, fake, None) == -2
    assert FIT_ARGTYPES[1] is ctypes.c_long
