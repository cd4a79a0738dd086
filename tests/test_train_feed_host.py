"""The draws of sn2_train_batch, restated in numpy from the text of include/strata_hip.h -- not from the kernel -- with their
statistics, the entry point's argument checks and the bookkeeping of train_data.EpochFeeder (no device anywhere in this file).
tests/test_gpu_train_feed.py holds the kernel to `restate_batch`.  The generator is the restatement of tests/test_subsample_host.py.
"""
import ctypes
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_subsample_host import philox4x32_10, subsample_row

F32 = np.float32
SIGMA, CLIP_XY, CLIP_COLOUR = 0.01 * 10, 0.03 * 10, 0.03 * 65536          # as loader.py:180-208 writes them


def words(seed: int, key: int, i, c1: int):
    """The four output words for counter (i, c1, key.lo, key.hi) and key (seed.lo, seed.hi); i: an array of uint32 values."""
    i = np.asarray(i, dtype=np.uint64)
    key &= 2 ** 64 - 1
    z = np.zeros_like(i)
    return philox4x32_10((i, z + np.uint64(c1), z + np.uint64(key & 0xFFFFFFFF), z + np.uint64(key >> 32)),
                         (seed & 0xFFFFFFFF, seed >> 32))


def plot_key(epoch: int, P: int, plot_id: int) -> int:
    return epoch * P + plot_id


def plot_params(seed: int, key: int):
    """-> (flip_x, flip_y, angle in whole degrees)."""
    w = [int(v[0]) for v in words(seed, key, [0], 1)]
    return w[0] >> 31, w[1] >> 31, (w[2] * 360) >> 32


def fps_starts(seed: int, key: int, N: int, M1: int):
    w = [int(v[0]) for v in words(seed, key, [1], 1)]
    return (w[0] * N) >> 32, (w[1] * M1) >> 32


def box_muller(wa, wb):
    u1 = (wa.astype(np.float64) + 1.0) * 2.0 ** -32
    u2 = wb.astype(np.float64) * 2.0 ** -32
    r = np.sqrt(-2.0 * np.log(u1))
    t = 6.283185307179586 * u2
    return r * np.cos(t), r * np.sin(t)


def noise_terms(seed: int, key: int, src) -> np.ndarray:
    """(6, len(src)) fp32: the noise of x, y, red, green, blue, near_infrared for the points with SOURCE indices `src`."""
    a, b = words(seed, key, src, 2), words(seed, key, src, 3)
    gx, gy = box_muller(a[0], a[1])
    gr, gg = box_muller(a[2], a[3])
    gb, gn = box_muller(b[0], b[1])
    xy = [np.clip(SIGMA * g, -CLIP_XY, CLIP_XY).astype(F32) for g in (gx, gy)]
    col = [np.clip(SIGMA * g, -CLIP_COLOUR, CLIP_COLOUR).astype(F32) for g in (gr, gg, gb, gn)]
    return np.stack(xy + col)


def restate_plot(raw, center, fake, N, z_max, seed, key, cos_sin, train=True, noise=True):
    """One plot's rows: raw (10,n) fp32, center (2) fp32, fake (F,2) fp32 -> cloud (10,N), xyz (3,N) fp32, with the arithmetic of
    the header's sn2_prepare_plots (numpy 1.21 rules: fp32 stays fp32, the rotation is an fp64 product cast back)."""
    raw = np.asarray(raw, dtype=F32)
    n_raw, F = raw.shape[1], len(fake)
    src = subsample_row(n_raw + F, N, seed, key).astype(np.int64)
    v = np.zeros((10, N), dtype=F32)
    real = src < n_raw
    v[:, real] = raw[:, src[real]]
    v[0, real] -= F32(center[0])
    v[1, real] -= F32(center[1])
    v[0, ~real], v[1, ~real] = fake[src[~real] - n_raw, 0], fake[src[~real] - n_raw, 1]
    x, y, z = v[0].copy(), v[1].copy(), v[2].copy()
    if train:
        fx, fy, angle = plot_params(seed, key)
        cs, sn = cos_sin[angle]
        x64, y64 = v[0].astype(np.float64), v[1].astype(np.float64)
        x, y = (x64 * cs + y64 * sn).astype(F32), (x64 * (-sn) + y64 * cs).astype(F32)
        if fx:
            x = -x
        if fy:
            y = -y
        v[0], v[1] = x, y
        if noise:
            nz = noise_terms(seed, key, src)
            v[0] = v[0] + nz[0]
            v[1] = v[1] + nz[1]
            v[3:7] = v[3:7] + nz[2:6]
    v[0], v[1], v[2] = v[0] / F32(10), v[1] / F32(10), v[2] / F32(z_max)
    v[3:7] = v[3:7] / F32(65536)
    v[7] = v[7] / F32(32768)
    v[8:10] = (v[8:10] - F32(1)) / F32(6)
    return v, np.stack([x, y, z])


def restate_batch(raw_plots, centers, fake, ids, epoch, seed, N, M1, z_max, cos_sin, train=True, noise=True):
    P = len(raw_plots)
    rows = [restate_plot(raw_plots[p], centers[p], fake, N, z_max, seed, plot_key(epoch, P, p), cos_sin, train, noise) for p in ids]
    fs = np.array([fps_starts(seed, plot_key(epoch, P, p), N, M1) for p in ids], dtype=np.int32).T
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), fs


# ---- statistics of the restated draws -----------------------------------------------------------------------------------
SAMPLES = 10 ** 6


def _close(got, want, std_err):
    """within three standard errors or within 1 %, whichever is larger"""
    return abs(got - want) <= max(3 * std_err, 0.01 * abs(want))


def test_flips_are_fair_and_angles_uniform():
    seed = 0x1234_5678_9ABC_DEF0
    key = np.arange(SAMPLES, dtype=np.uint64)                   # one plot key per sample: counter (0, 1, key, 0)
    z = np.zeros_like(key)
    w = philox4x32_10((z, z + np.uint64(1), key, z), (seed & 0xFFFFFFFF, seed >> 32))
    assert [int(v) for v in (w[0][5], w[1][5], w[2][5], w[3][5])] == [int(v[0]) for v in words(seed, 5, [0], 1)]
    for flips in (w[0] >> np.uint64(31), w[1] >> np.uint64(31)):
        assert set(np.unique(flips).tolist()) == {0, 1}
        assert _close(float(flips.mean()), 0.5, 0.5 / math.sqrt(SAMPLES))
    angle = (w[2] * np.uint64(360)) >> np.uint64(32)
    counts = np.bincount(angle.astype(np.int64), minlength=360)
    assert counts.shape == (360,) and counts.min() > 0                      # 0 .. 359, every one drawn
    chi2 = float(((counts - SAMPLES / 360) ** 2 / (SAMPLES / 360)).sum())
    # chi-square with 359 degrees of freedom: mean 359, standard deviation sqrt(2 * 359) = 26.8; five of them
    assert chi2 < 359 + 5 * math.sqrt(2 * 359), chi2
    fs = [fps_starts(seed, k, 1000, 7) for k in range(200)]
    assert all(0 <= a < 1000 and 0 <= b < 7 for a, b in fs) and len({a for a, _ in fs}) > 150


def _clamped_normal_std(sigma: float, clip: float) -> float:
    """Standard deviation of X = clamp(sigma Z, -clip, clip), Z standard normal, a = clip / sigma (mean 0 by symmetry):
    E X^2 = sigma^2 [ int_{-a}^{a} z^2 phi(z) dz + 2 a^2 (1 - Phi(a)) ], and by parts int_{-a}^{a} z^2 phi = (2 Phi(a) - 1) - 2 a phi(a)."""
    a = clip / sigma
    Phi = 0.5 * (1.0 + math.erf(a / math.sqrt(2.0)))
    phi = math.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi)
    return sigma * math.sqrt((2.0 * Phi - 1.0) - 2.0 * a * phi + 2.0 * a * a * (1.0 - Phi))


def test_noise_is_the_clamped_normal():
    assert (SIGMA, CLIP_XY) == (0.1, 0.3)
    nz = noise_terms(0xC0FFEE, plot_key(3, 57, 11), np.arange(SAMPLES))
    assert nz.shape == (6, SAMPLES) and nz.dtype == F32
    assert abs(_clamped_normal_std(0.1, 0.3) - 0.1 * math.sqrt(0.9950073)) < 1e-8      # a = 3: the tabulated value
    for row, clip in zip(nz, [CLIP_XY] * 2 + [CLIP_COLOUR] * 4):
        std = _clamped_normal_std(SIGMA, clip)
        x = row.astype(np.float64)
        assert float(np.abs(x).max()) <= float(F32(clip))
        assert _close(float(x.mean()), 0.0, std / math.sqrt(SAMPLES)), float(x.mean())
        # standard error of a sample standard deviation: below std / sqrt(2 n) * sqrt(kurtosis - 1) ~ std / sqrt(n)
        assert _close(float(x.std()), std, std / math.sqrt(SAMPLES)), (float(x.std()), std)
    assert float((np.abs(nz[:2]) == F32(CLIP_XY)).mean()) > 0.002           # x, y ARE clamped at three sigma (2.7e-3 of them)
    c = np.corrcoef(nz.astype(np.float64))
    assert float(np.abs(c - np.eye(6)).max()) < 5 / math.sqrt(SAMPLES)      # the six channels are independent draws
    # duplicates of a source point share their noise; another key, seed or domain does not
    again = noise_terms(0xC0FFEE, plot_key(3, 57, 11), np.array([7, 7, 8]))
    assert np.array_equal(again[:, 0], again[:, 1]) and np.array_equal(again[:, 0], nz[:, 7]) and not np.array_equal(again[:, 0], again[:, 2])
    assert not np.array_equal(noise_terms(0xC0FFEE, plot_key(4, 57, 11), np.arange(8)), nz[:, :8])
    assert not np.array_equal(noise_terms(0xC0FFEF, plot_key(3, 57, 11), np.arange(8)), nz[:, :8])


def test_restated_plot_takes_both_subsample_branches():
    from stratanet2_vegetation_coverage_maps_amd.input_pipeline import fake_ground_xy
    from stratanet2_vegetation_coverage_maps_amd.train_data import cos_sin_table
    fake, cs = fake_ground_xy(20), cos_sin_table()
    assert fake.shape == (316, 2) and cs.shape == (360, 2) and cs[90, 1] == 1.0 and cs[0, 0] == 1.0
    rng = np.random.RandomState(1)
    for n in (60, 196, 700):
        raw = rng.rand(10, n).astype(F32) * 5 + 1
        a, xa = restate_plot(raw, (1.0, 2.0), fake, 512, 24.24, 9, 77, cs)
        b, xb = restate_plot(raw, (1.0, 2.0), fake, 512, 24.24, 9, 77, cs, noise=False)
        c, xc = restate_plot(raw, (1.0, 2.0), fake, 512, 24.24, 9, 77, cs, train=False)
        assert a.shape == (10, 512) and xa.shape == (3, 512) and np.array_equal(xa, xb)         # xyz never sees the noise
        assert np.array_equal(a[[2, 7, 8, 9]], b[[2, 7, 8, 9]]) and not np.array_equal(a[0], b[0]) and not np.array_equal(a[3], b[3])
        assert float(np.abs(a[:2] - b[:2]).max()) <= 0.03 + 1e-6
        np.testing.assert_allclose(np.hypot(xb[0], xb[1]), np.hypot(xc[0], xc[1]), rtol=1e-5, atol=1e-5)   # a rotation and flips
        assert np.array_equal(xb[2], xc[2])


# ---- the entry point's argument checks ----------------------------------------------------------------------------------
def test_c_abi_refuses_bad_arguments_before_any_device_work():
    from stratanet2_vegetation_coverage_maps_amd import _build, _lib
    raw = ctypes.CDLL(_lib.LIB_PATH if os.path.exists(_lib.LIB_PATH) else _build.build(verbose=False))
    fn = raw.sn2_train_batch
    fn.restype = ctypes.c_int
    fn.argtypes = _lib.SIGNATURES["sn2_train_batch"]
    wfn = raw.sn2_train_batch_ws_words
    wfn.restype = ctypes.c_int
    wfn.argtypes = _lib.SIGNATURES["sn2_train_batch_ws_words"]
    sub = raw.sn2_subsample_ws_words
    sub.restype = ctypes.c_size_t
    sub.argtypes = _lib.SIZE_HELPERS["sn2_subsample_ws_words"]
    EINVAL, ELIMIT = -1, -2
    nw = ctypes.c_size_t()
    assert wfn(3, 400, 512, ctypes.byref(nw)) == 0 and nw.value == 8 * 3                    # nobody is subsampled: keys, rotation, flips
    assert wfn(3, 1816, 512, ctypes.byref(nw)) == 0 and nw.value == 8 * 3 + 3 * 512         # + the index rows (LDS form: no more)
    assert wfn(3, 17316, 256, ctypes.byref(nw)) == 0 and nw.value == 8 * 3 + 3 * 256 + sub(3, 17316, 256, 0)
    assert wfn(3, 17316, 256, None) == EINVAL and wfn(0, 10, 10, ctypes.byref(nw)) == EINVAL
    assert wfn(3, 400, 512, ctypes.byref(nw)) == 0
    p = 0x1000                                                   # never dereferenced: every call below fails a check first
    good = dict(raw=p, T=5000, offsets=p, centers=p, coverages=p, P=5, ids=p, B=3, fake=p, n_fake=316, n_max=400, N=512, M1=64,
                z_max=24.24, seed=1, epoch=0, cos_sin=p, train=1, noise=1, ws=p, ws_words=nw.value, cloud=p, xyz=p, gt=p, fps=p,
                stream=None)

    def call(**kw):
        return fn(*{**good, **kw}.values())
    for name in ("raw", "offsets", "centers", "coverages", "ids", "cloud", "xyz", "gt", "fps", "fake", "cos_sin", "ws"):
        assert call(**{name: None}) == EINVAL, name
    for name in ("B", "N", "P", "M1", "n_max", "T"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -1}) == EINVAL, name
    assert call(n_fake=-1) == EINVAL and call(epoch=-1) == EINVAL and call(z_max=0.0) == EINVAL
    assert call(T=2 ** 31) == ELIMIT and call(B=65536, ws_words=10 ** 9) == ELIMIT
    assert call(ws_words=nw.value - 1) == EINVAL and call(ws=p + 4) == EINVAL
    assert call(n_max=1816, ws_words=nw.value) == EINVAL                                    # now the index rows do not fit
    assert _lib.SN2_VERSION == 102


def test_wrapper_validates_ids_on_the_host():
    from stratanet2_vegetation_coverage_maps_amd.train_data import ResidentPlots
    plots = ResidentPlots.__new__(ResidentPlots)
    plots.P = 5
    assert plots.check_ids([4, 0, 2]).dtype == torch.int32
    for bad in ([5, 0], [-1], [], [[1, 2]], [0.5]):
        with pytest.raises(ValueError):
            plots.check_ids(bad)


# ---- EpochFeeder's bookkeeping --------------------------------------------------------------------------------------------
def _feeder(P=7, B=2, seed=5, gen_seed=99):
    from stratanet2_vegetation_coverage_maps_amd.train_data import EpochFeeder
    return EpochFeeder(SimpleNamespace(P=P), None, B, seed, generator=torch.Generator().manual_seed(gen_seed))


def test_epoch_feeder_orders_are_the_samplers():
    f = _feeder()
    assert f.steps_per_epoch == 3
    g = torch.Generator().manual_seed(99)
    perms = [torch.randperm(7, generator=g) for _ in range(4)]
    for i in range(12):
        e, k = divmod(i, 3)
        assert f.locate(i) == (e, k)
        ids = f.batch_ids(i)
        assert ids.dtype == torch.int32 and ids.tolist() == perms[e][k * 2:(k + 1) * 2].tolist()
    for e in range(4):                                                       # every epoch: P // B batches of distinct ids
        seen = [int(v) for k in range(3) for v in f.batch_ids(3 * e + k)]
        assert len(seen) == 6 and len(set(seen)) == 6 and all(0 <= v < 7 for v in seen)
    assert f.batch_ids(1).tolist() == perms[0][2:4].tolist()                 # asking again (the capture's warm-up) draws nothing new
    assert f.batch_ids(12).tolist() == torch.randperm(7, generator=g)[0:2].tolist()
    with pytest.raises(ValueError):
        _feeder(P=3, B=4)
    with pytest.raises(ValueError):
        f.batch_ids(-1)


def test_epoch_feeder_state_dict_round_trip_continues_the_sequence():
    f = _feeder()
    want = [f.batch_ids(i).tolist() for i in range(20)]
    for cut in (0, 3, 7, 11):                                                # epoch boundaries and the middle of an epoch
        sd = f.state_dict(cut)
        assert sd["seed"] == 5 and sd["epoch"] == cut // 3 and sd["batch_in_epoch"] == cut % 3
        sd = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in sd.items()}
        g = _feeder(gen_seed=12345)                                          # another generator: the state brings its own
        g.load_state_dict(sd)
        assert g.seed == 5 and g.locate(0) == f.locate(cut)
        assert [g.batch_ids(i).tolist() for i in range(20 - cut)] == want[cut:]
    with pytest.raises(ValueError):
        _feeder(P=8).load_state_dict(f.state_dict(0))
