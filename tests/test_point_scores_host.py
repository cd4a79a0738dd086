"""The rule of the per-point scores (include/strata_hip.h, "Per-point scores") on the host: its numpy restatement
(tests/_point_scores_ref.py) is order-free, exact for a single contribution, and counts no repeat, fake ground point or
out-of-range index; header, binding and library agree; the C ABI refuses bad arguments before any device work."""
import ctypes
import os
import re

import numpy as np

import _point_scores_cases as cases
import _point_scores_ref as ref
from conftest import ROOT
from stratanet2_vegetation_coverage_maps_amd import _lib


def _contribs(plots):
    bt = cases.batch_of(plots)
    return ref.contributions(bt["cov"], bt["proba"], bt["xyz"], bt["idx"], bt["n_live"], bt["offsets"], bt["point_index"], cases.T,
                             cases.DIAM, bt["col_base"])


def _scores(col, terms):
    acc, hits = np.zeros((cases.T, 9), dtype=np.int64), np.zeros(cases.T, dtype=np.int32)
    ref.accumulate(acc, hits, col, terms)
    s, w = ref.finalize(acc, hits)
    return s.tobytes(), w.tobytes(), hits.tobytes()


def test_any_order_of_the_contributions_gives_the_same_bytes():
    plots = cases.planted()
    col, terms = _contribs(plots)
    want = _scores(col, terms)
    rng = np.random.default_rng(1)
    for _ in range(5):
        p = rng.permutation(len(col))
        assert _scores(col[p], terms[p]) == want
    assert _scores(col[::-1], terms[::-1]) == want
    # plot by plot, in reverse, is the same set of contributions
    parts = [_contribs([p]) for p in plots[::-1]]
    assert _scores(np.concatenate([c for c, _ in parts]), np.concatenate([t for _, t in parts])) == want


def test_a_single_contribution_returns_the_networks_value():
    """|num/den - v| <= 2^-32 (two roundings of at most half a unit over den >= 2^32), below the half-ulp 2^-31 of an fp32
    v >= 2^-7: the fp64 quotient rounds back to v.  10^5 random values, weights over the whole disc."""
    n = 100000
    rng = np.random.default_rng(2)
    v = np.concatenate([rng.uniform(2.0 ** -7, 1.0, (n - 2, 8)), np.full((1, 8), 2.0 ** -7), np.ones((1, 8))]).astype(np.float32)
    assert v.min() >= np.float32(2.0 ** -7)
    ang, rad = rng.random(n) * 2 * np.pi, 10.0 * np.sqrt(rng.random(n))
    xyz = np.stack([rad * np.cos(ang), rad * np.sin(ang), np.zeros(n)]).astype(np.float32)[None]
    col, terms = ref.contributions(v[:, :4], v[:, 4:], xyz, np.arange(n)[None], [n], [0, n], np.arange(n), n, cases.DIAM)
    assert np.array_equal(col, np.arange(n))
    acc, hits = np.zeros((n, 9), dtype=np.int64), np.zeros(n, dtype=np.int32)
    ref.accumulate(acc, hits, col, terms)
    s, w = ref.finalize(acc, hits)
    assert np.array_equal(np.ascontiguousarray(s.T).view(np.uint32), v.view(np.uint32))
    assert w.min() >= 1.0 - 1e-6 and w.max() <= 1.5


def test_repeats_fake_ground_and_out_of_range_samples_contribute_nothing():
    plots = cases.planted()
    col, terms = _contribs(plots)
    acc, hits = np.zeros((cases.T, 9), dtype=np.int64), np.zeros(cases.T, dtype=np.int32)
    ref.accumulate(acc, hits, col, terms)
    # by hand: the distinct live samples of real points whose column is inside the arena, per plot
    want = np.zeros(cases.T, dtype=np.int32)
    n_contrib = 0
    for p in plots:
        live = p["idx"][:p["n_live"]]
        real = live[(live >= 0) & (live < len(p["point_index"]))]
        assert len(np.unique(real)) == len(real)                       # a (plot, point) pair at most once
        c = p["col_base"] + p["point_index"][real].astype(np.int64)
        c = c[(c >= 0) & (c < cases.T)]
        n_contrib += len(c)
        np.add.at(want, c, 1)
    assert len(col) == n_contrib and np.array_equal(hits, want)
    assert hits[cases.SHARED] == 3 and hits[cases.NEVER] == 0 and hits.max() == 3 and (hits == 0).sum() > 50
    assert [hits[c] for c in (cases.CENTRE, cases.RIM, cases.ZERO, cases.ONE_)] == [1, 1, 1, 1]
    # plot 1 alone: its 100 real points once each, whatever the 76 repeats name
    c1, _ = _contribs(plots[1:2])
    assert len(c1) == 100 == len(np.unique(c1))
    # the planted weights and values
    s, w = ref.finalize(acc, hits)
    assert w[cases.CENTRE] == 1.5 and w[cases.RIM] == 1.0 and w[cases.NEVER] == 0.0
    assert np.isnan(s[:, cases.NEVER]).all() and (s[:, cases.ZERO] == 0.0).all() and (s[:, cases.ONE_] == 1.0).all()
    assert not np.isnan(s[:, hits > 0]).any()
    # nothing lands outside: naming a fake ground point instead of each bad index changes no byte
    good = [dict(p) for p in plots]
    for p in good:
        idx = p["idx"].copy()
        idx[(idx < 0) | (idx >= len(p["point_index"]) + 316)] = len(p["point_index"])
        p["idx"] = idx
    c2, t2 = _contribs(good)
    assert _scores(c2, t2) == _scores(col, terms)


def test_header_binding_and_exports_agree():
    txt = open(os.path.join(ROOT, "include", "strata_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("sn2_points_merge", "sn2_points_finalize"):
        assert re.search(r"^int\s+%s\s*\(" % name, txt, flags=re.M) and name in _lib.SIGNATURES
        assert hasattr(raw, name)
    assert re.search(r"^#define SN2_POINTS_ACC_WORDS 9\b", txt, flags=re.M) and _lib.SN2_POINTS_ACC_WORDS == 9
    sig = _lib.SIGNATURES["sn2_points_merge"]
    assert len(sig) == 16 and sig[7] is ctypes.c_long and sig[9:12] == [ctypes.c_int, ctypes.c_int, ctypes.c_double]
    assert sig[14] is ctypes.c_long and len(_lib.SIGNATURES["sn2_points_finalize"]) == 6
    from stratanet2_vegetation_coverage_maps_amd import _build
    assert "points.hip" in _build.SOURCES and "point_rules.h" in _build.HEADERS


def test_argument_checks_return_before_any_device_work():
    lib = _lib.load()
    fake = 0x1000                                            # never dereferenced: every call below fails a check first
    ok = dict(cov=fake, proba=fake, xyz=fake, idx=fake, n_live=fake, offsets=fake, point_index=fake, sum_n=430, col_base=None, B=3,
              N=256, diam=20.0, acc=fake, hits=fake, T=500, stream=None)

    def rc(**kw):
        return lib.sn2_points_merge(*{**ok, **kw}.values())
    for name in ("cov", "proba", "xyz", "idx", "n_live", "offsets", "point_index", "acc", "hits"):
        assert rc(**{name: None}) == _lib.SN2_EINVAL, name
    for bad in (dict(B=0), dict(B=-1), dict(N=0), dict(N=-256), dict(T=0), dict(T=-5), dict(sum_n=0), dict(diam=0.0), dict(diam=-20.0),
                dict(diam=float("nan"))):
        assert rc(**bad) == _lib.SN2_EINVAL, bad
        assert rc(col_base=fake, **bad) == _lib.SN2_EINVAL, bad
    for big in (dict(T=2 ** 31), dict(T=2 ** 40), dict(sum_n=2 ** 31), dict(B=65536, N=32768)):
        assert rc(**big) == _lib.SN2_ELIMIT, big

    okf = dict(acc=fake, hits=fake, T=500, scores=fake, weight=fake, stream=None)

    def rcf(**kw):
        return lib.sn2_points_finalize(*{**okf, **kw}.values())
    for name in ("acc", "hits", "scores", "weight"):
        assert rcf(**{name: None}) == _lib.SN2_EINVAL, name
    assert rcf(T=0) == _lib.SN2_EINVAL and rcf(T=-1) == _lib.SN2_EINVAL
    assert rcf(T=2 ** 31) == _lib.SN2_ELIMIT
