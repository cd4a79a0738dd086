"""The device subsampler's definition, restated in numpy from the text of include/strata_hip.h (sn2_subsample) -- not from
the kernel -- and the host-side checks around it.  tests/test_gpu_subsample.py holds the kernel to `subsample_rows`.

Known answers: the three Philox4x32-10 vectors of the Random123 distribution's `kat_vectors` (counter and key all zeros, all
ones, and the digits of pi).  They are quoted here; no copy of that file was found offline, so the generator is ALSO checked
against an independent scalar restatement in python integers and, on the GPU, by the distribution tests.
"""
import ctypes
import os

import numpy as np
import pytest

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars) c0..c3, key: (k0, k1) -> the four output words (uint64 arrays holding 32-bit
    values)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in counter)
    k0, k1 = (np.uint64(int(k) & 0xFFFFFFFF) for k in key)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                 # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def u_words(seed: int, key: int, i):
    """u(seed, key, i) for an array of candidate numbers i -> uint64."""
    i = np.asarray(i, dtype=np.uint64)
    key &= 2 ** 64 - 1
    z = np.zeros_like(i)
    o = philox4x32_10((i, z, z + np.uint64(key & 0xFFFFFFFF), z + np.uint64(key >> 32)), (seed & 0xFFFFFFFF, seed >> 32))
    return (o[0] << np.uint64(32)) | o[1]


def mulhi64(u, n: int):
    """floor(u * n / 2^64) for uint64 u and 0 < n < 2^31, without leaving uint64."""
    hi, lo = u >> np.uint64(32), u & MASK
    return (hi * np.uint64(n) + ((lo * np.uint64(n)) >> np.uint64(32))) >> np.uint64(32)


def subsample_row(n: int, N: int, seed: int, key: int) -> np.ndarray:
    """One plot's row: n candidates, subsample size N."""
    assert n > 0 and N > 0
    if n > N:
        u = u_words(seed, key, np.arange(n))
        return np.lexsort((np.arange(n), u))[:N].astype(np.int32)       # ascending (u, i)
    j = np.arange(n, N)
    return np.concatenate([np.arange(n), mulhi64(u_words(seed, key, j), n)]).astype(np.int32)


def subsample_rows(n_points, N: int, seed: int, keys) -> np.ndarray:
    return np.stack([subsample_row(int(n), N, seed, int(k)) for n, k in zip(n_points, keys)])


def _philox_scalar(c, k):
    """The same generator in python integers, written separately (key schedule BEFORE rounds 2..10, as the paper has it)."""
    c, k = list(c), list(k)
    for r in range(10):
        if r:
            k = [(k[0] + W0) % 2 ** 32, (k[1] + W1) % 2 ** 32]
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 % 2 ** 32, (p0 >> 32) ^ c[3] ^ k[1], p0 % 2 ** 32]
    return c


KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("c,k,want", KAT)
def test_philox_known_answers(c, k, want):
    assert tuple(int(v) for v in philox4x32_10(c, k)) == want
    assert tuple(_philox_scalar(c, k)) == want


def test_vector_and_scalar_restatements_agree():
    rng = np.random.RandomState(0)
    seed, key = int(rng.randint(0, 2 ** 63)) * 2 + 1, -int(rng.randint(1, 2 ** 62))     # a negative key: its 64 bits as unsigned
    i = np.concatenate([np.arange(50), rng.randint(0, 2 ** 31 - 1, 50)])
    u = u_words(seed, key, i)
    ku = key % 2 ** 64
    for ii, uu in zip(i, u):
        o = _philox_scalar((int(ii), 0, ku % 2 ** 32, ku >> 32), (seed % 2 ** 32, seed >> 32))
        assert int(uu) == o[0] << 32 | o[1]
    n = 12345
    assert [int(v) for v in mulhi64(u, n)] == [int(v) * n >> 64 for v in u]


def test_rows_have_the_two_branches_shapes_and_ranges():
    for n, N in ((300, 100), (101, 100), (5000, 1), (100, 100), (60, 100), (1, 7)):
        row = subsample_row(n, N, 42, 3)
        assert row.shape == (N,) and row.dtype == np.int32 and row.min() >= 0 and row.max() < n
        if n > N:
            assert len(set(row.tolist())) == N
            u = u_words(42, 3, row)
            assert all(int(a) <= int(b) for a, b in zip(u[:-1], u[1:]))            # listed in key order
            rest = np.setdiff1d(np.arange(n), row)
            assert int(u_words(42, 3, rest).min()) >= int(u[-1])                   # and no smaller key was left out
        else:
            assert row[:n].tolist() == list(range(n))
    assert not np.array_equal(subsample_row(300, 100, 42, 3), subsample_row(300, 100, 42, 4))
    assert not np.array_equal(subsample_row(300, 100, 42, 3), subsample_row(300, 100, 43, 3))
    # the first N draws of a longer subsample of the same plot are the shorter one: both list the same order
    assert np.array_equal(subsample_row(300, 100, 42, 3)[:40], subsample_row(300, 40, 42, 3))


def test_unknown_sampler_is_refused():
    import torch
    from stratanet2_vegetation_coverage_maps_amd import parcel
    from stratanet2_vegetation_coverage_maps_amd.input_pipeline import prepare_batch
    from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args
    args = make_args()
    plot = np.zeros((10, 60), dtype=np.float32)
    with pytest.raises(ValueError, match="sampler"):
        prepare_batch([plot], np.zeros((1, 2), np.float32), args, train=False, sampler="bogus")
    with pytest.raises(ValueError, match="sampler"):
        parcel._empty(torch.device("cpu")).batches(args, 8, sampler="bogus")
    with pytest.raises(ValueError, match="sampler"):
        parcel.predict_parcel_cloud(None, plot, args, sampler="bogus")
    with pytest.raises(ValueError, match="seed"):                                   # a seed without the sampler it belongs to
        prepare_batch([plot], np.zeros((1, 2), np.float32), args, train=False, seed=1)


def test_wrapper_refuses_bad_arguments_before_the_library():
    """hip_ops.subsample checks on the host first: tensors that are not on the device, wrong dtypes."""
    import torch
    from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
    with pytest.raises(ValueError):
        ops.subsample(torch.zeros(3, dtype=torch.int32), 0, 10, 1, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.subsample(np.zeros(3, dtype=np.int32), 0, 10, 1, np.zeros(2, dtype=np.int64))


def test_c_abi_refuses_bad_arguments_before_any_device_work():
    from stratanet2_vegetation_coverage_maps_amd import _build, _lib
    raw = ctypes.CDLL(_lib.LIB_PATH if os.path.exists(_lib.LIB_PATH) else _build.build(verbose=False))
    fn = raw.sn2_subsample
    fn.restype = ctypes.c_int
    fn.argtypes = _lib.SIGNATURES["sn2_subsample"]
    words = raw.sn2_subsample_ws_words
    words.restype = ctypes.c_size_t
    words.argtypes = _lib.SIZE_HELPERS["sn2_subsample_ws_words"]
    form = raw.sn2_subsample_form
    form.restype = ctypes.c_int
    form.argtypes = _lib.SIGNATURES["sn2_subsample_form"]
    p = 0x1000                                                   # never dereferenced: every call below fails a check first
    EINVAL, ELIMIT = -1, -2
    #           offsets extra n_max B  N  seed keys form ws ws_words idx stream
    assert fn(None, 0, 100, 2, 10, 1, p, 0, None, 0, p, None) == EINVAL
    assert fn(p, 0, 100, 2, 10, 1, None, 0, None, 0, p, None) == EINVAL
    assert fn(p, 0, 100, 2, 10, 1, p, 0, None, 0, None, None) == EINVAL
    assert fn(p, 0, 100, 0, 10, 1, p, 0, None, 0, p, None) == EINVAL            # no plot
    assert fn(p, 0, 100, 2, 0, 1, p, 0, None, 0, p, None) == EINVAL             # N <= 0
    assert fn(p, -1, 100, 2, 10, 1, p, 0, None, 0, p, None) == EINVAL           # extra < 0
    assert fn(p, 0, 0, 2, 10, 1, p, 0, None, 0, p, None) == EINVAL              # no candidates at all
    assert fn(p, 0, 100, 2, 10, 1, p, 3, None, 0, p, None) == EINVAL            # not a form
    assert fn(p, 0, 100, 2, 10, 1, p, 8, None, 0, p, None) == EINVAL
    lds_max = 16384
    assert form(lds_max, 10000) == 1 and form(lds_max + 1, 10000) == 2 and form(12316, 10000) == 1 and form(33084, 32768) == 2
    assert fn(p, 0, lds_max + 1, 2, 10, 1, p, 1, None, 0, p, None) == ELIMIT    # the LDS form beyond what LDS holds
    assert fn(p, 0, lds_max + 1, 2, 10, 1, p, 0, None, 0, p, None) == EINVAL    # the global form without its workspace
    need = words(2, lds_max + 1, 10, 0)
    assert need == words(2, lds_max + 1, 10, 2) and need >= 2 * 2 * (lds_max + 1)
    assert fn(p, 0, lds_max + 1, 2, 10, 1, p, 0, p, need - 1, p, None) == EINVAL    # ... or with too small a one
    assert fn(p, 0, lds_max + 1, 2, 10, 1, p, 0, p + 4, need, p, None) == EINVAL    # ... or a misaligned one
    assert words(2, 100, 10, 0) == 0 and words(2, 100, 10, 1) == 0 and words(2, 100, 10, 2) > 0
    assert words(0, 100, 10, 2) == 0
    assert _lib.SN2_VERSION == 102
