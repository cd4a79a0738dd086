"""sn2_fps_route without a device: the plan sn2_fps_live runs before its first launch, held to the routes written out BY HAND from
the dispatch ladder of the commit before it (sn2_fps_live, dispatch_fps_cluster, dispatch_fps_bucket16, launch_fps_cluster of
csrc/geometry.hip) -- one row per template rung of every ladder and per rewritten request."""
import ctypes
import os

import pytest


def _raw_lib():
    from stratanet2_vegetation_coverage_maps_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH if os.path.exists(_lib.LIB_PATH) else __import__(
        "stratanet2_vegetation_coverage_maps_amd._build", fromlist=["build"]).build(verbose=False))
    for name in ("sn2_fps_route", "sn2_fps_fills_ws", "sn2_fps_live", "sn2_fps_status"):
        fn = getattr(raw, name)
        fn.restype = ctypes.c_int
        fn.argtypes = _lib.SIGNATURES[name]
    return raw


def _route(raw, B, N, M, waves, have_ws=1, cus=256):
    """(form, nw, p, rung, lds_points, repair, fills_ws), or the negative code"""
    from stratanet2_vegetation_coverage_maps_amd import _lib
    r = _lib.FpsRoute(-9, -9, -9, -9, -9, -9, -9)
    rc = raw.sn2_fps_route(B, N, M, waves, have_ws, cus, ctypes.byref(r))
    return rc if rc != 0 else tuple(getattr(r, n) for n, _ in _lib.FpsRoute._fields_)


BRUTE, ROUND, SPEC, CLUSTER = 0, 1, 2, 3
EINVAL, ELIMIT = -1, -2


def brute(ppt, threads):
    return (BRUTE, threads // 64, 1, ppt, 0, 0, 0)


def single(nw, spw, form=SPEC):
    return (form, nw, 1, spw, 0, 0, 1)


def cluster(spw, nw, p, lp, repair):
    return (CLUSTER, nw, p, spw, lp, repair, 1)


# (B, N, M, waves, have_ws, cus) -> route.  buckets = ceil(N / 64); a cluster of P workgroups of NW waves fits where
# B * P <= cus and 2 * P * NW <= buckets <= 512 * P; its slots per wave hold ceil(ceil(buckets / P) / NW); its points stay in LDS
# where slots * NW <= 96; the repair launch is the 16-wave kernel of the plot size.
TABLE = {
    # ---- brute force (no workspace): fps_kernel<PPT, T>, every rung at its last size and the first size of the next
    (2, 256, 32, 0, 0, 256): brute(1, 256), (2, 257, 32, 0, 0, 256): brute(2, 256), (2, 512, 32, 0, 0, 256): brute(2, 256),
    (2, 513, 32, 0, 0, 256): brute(4, 256), (2, 1024, 32, 0, 0, 256): brute(4, 256), (2, 1025, 32, 0, 0, 256): brute(2, 1024),
    (2, 2048, 32, 0, 0, 256): brute(2, 1024), (2, 2049, 32, 0, 0, 256): brute(4, 1024), (2, 4096, 32, 0, 0, 256): brute(4, 1024),
    (2, 4097, 32, 0, 0, 256): brute(8, 1024), (2, 8192, 32, 0, 0, 256): brute(8, 1024), (2, 8193, 32, 0, 0, 256): brute(16, 1024),
    (2, 16384, 32, 0, 0, 256): brute(16, 1024), (2, 16385, 32, 0, 0, 256): brute(32, 1024), (2, 32768, 32, 0, 0, 256): brute(32, 1024),
    (2, 32769, 32, 0, 0, 256): ELIMIT, (2, 32772, 32, 8, 0, 256): ELIMIT,
    # with a workspace the kernels do not fill: 2048 points, 16 samples, B*N no multiple of 4
    (2, 2048, 32, 0, 1, 256): brute(2, 1024), (2, 4096, 16, 0, 1, 256): brute(4, 1024), (1, 2049, 100, 0, 1, 256): brute(4, 1024),
    (1, 2049, 100, 72, 1, 256): brute(4, 1024), (1, 2049, 100, 1, 1, 256): brute(4, 1024), (3, 16385, 64, 8, 1, 256): brute(32, 1024),
    # more than 32 plots of 2049 .. 4096 points: four waves per plot, with or without a workspace, whatever `waves`
    (33, 4096, 64, 0, 1, 256): brute(16, 256), (33, 4096, 64, 0, 0, 256): brute(16, 256), (40, 2500, 625, 4, 1, 256): brute(16, 256),
    (33, 2049, 64, 0, 0, 256): brute(16, 256), (33, 2048, 64, 0, 1, 256): brute(2, 1024), (32, 4096, 64, 0, 0, 256): brute(4, 1024),
    (33, 4097, 64, 0, 0, 256): brute(8, 1024),
    # ---- one workgroup of 16 waves: fps_spec_kernel<SPW, 16>, the rungs of dispatch_fps_bucket16
    (1, 2052, 32, 16, 1, 256): single(16, 4), (1, 4096, 32, 16, 1, 256): single(16, 4), (1, 4100, 32, 16, 1, 256): single(16, 8),
    (1, 8192, 32, 16, 1, 256): single(16, 8), (1, 8196, 32, 16, 1, 256): single(16, 16), (1, 16384, 32, 16, 1, 256): single(16, 16),
    (1, 16388, 32, 16, 1, 256): single(16, 32), (1, 32768, 32, 16, 1, 256): single(16, 32), (1, 32772, 32, 16, 1, 256): single(16, 64),
    (1, 65536, 32, 16, 1, 256): single(16, 64), (1, 65540, 32, 16, 1, 256): single(16, 128), (1, 131072, 32, 16, 1, 256): single(16, 128),
    # waves = 1: fps_bucket_kernel<SPW, 16>, the same rungs
    (1, 2052, 32, 1, 1, 256): single(16, 4, ROUND), (1, 4100, 32, 1, 1, 256): single(16, 8, ROUND),
    (1, 8196, 32, 1, 1, 256): single(16, 16, ROUND), (1, 16388, 32, 1, 1, 256): single(16, 32, ROUND),
    (1, 32772, 32, 1, 1, 256): single(16, 64, ROUND), (1, 65540, 32, 1, 1, 256): single(16, 128, ROUND),
    # waves = 8: <8, 8> .. <64, 8> up to 32 768 points, 16 waves above
    (1, 2052, 32, 8, 1, 256): single(8, 8), (1, 4096, 32, 8, 1, 256): single(8, 8), (1, 4100, 32, 8, 1, 256): single(8, 16),
    (1, 8192, 32, 8, 1, 256): single(8, 16), (1, 8196, 32, 8, 1, 256): single(8, 32), (1, 16384, 32, 8, 1, 256): single(8, 32),
    (1, 16388, 32, 8, 1, 256): single(8, 64), (1, 32768, 32, 8, 1, 256): single(8, 64),
    (1, 32772, 32, 8, 1, 256): single(16, 64), (1, 65540, 32, 8, 1, 256): single(16, 128),
    # waves = 4: <32, 4>, <64, 4> up to 16 384 points, 8 waves up to 32 768, 16 above
    (1, 2052, 32, 4, 1, 256): single(4, 32), (1, 8192, 32, 4, 1, 256): single(4, 32), (1, 8196, 32, 4, 1, 256): single(4, 64),
    (1, 16384, 32, 4, 1, 256): single(4, 64), (4, 16385, 32, 4, 1, 256): single(8, 64), (1, 16388, 32, 4, 1, 256): single(8, 64),
    (1, 32768, 32, 4, 1, 256): single(8, 64), (1, 32772, 32, 4, 1, 256): single(16, 64), (512, 10000, 2500, 4, 1, 256): single(4, 64),
    # ---- waves = 0 at the headline shape (512 buckets): 8 workgroups of 8 waves, 4 on 64 CUs (128 slots: no LDS points), none on 16
    (16, 32768, 1024, 0, 1, 256): cluster(8, 8, 8, 1, 32), (16, 32768, 1024, 0, 1, 128): cluster(8, 8, 8, 1, 32),
    (16, 32768, 1024, 0, 1, 127): cluster(16, 8, 4, 0, 32), (16, 32768, 1024, 0, 1, 64): cluster(16, 8, 4, 0, 32),
    (16, 32768, 1024, 0, 1, 63): cluster(32, 8, 2, 0, 32), (16, 32768, 1024, 0, 1, 32): cluster(32, 8, 2, 0, 32),
    (16, 32768, 1024, 0, 1, 31): single(16, 32), (16, 32768, 1024, 0, 1, 16): single(16, 32),
    (16, 32768, 1024, 0, 0, 256): brute(32, 1024), (16, 32768, 1024, 8, 1, 256): single(8, 64),
    # waves = 0 by the buckets: 33 (two workgroups), 63 / 64 (two / four), 127 / 128 (four / eight), 2048 (eight)
    (1, 2052, 32, 0, 1, 256): cluster(4, 8, 2, 1, 4), (1, 4032, 32, 0, 1, 256): cluster(4, 8, 2, 1, 4),
    (1, 4096, 32, 0, 1, 256): cluster(2, 8, 4, 1, 4), (1, 8128, 32, 0, 1, 256): cluster(4, 8, 4, 1, 8),
    (1, 8192, 32, 0, 1, 256): cluster(2, 8, 8, 1, 8), (1, 131072, 32, 0, 1, 256): cluster(32, 8, 8, 0, 128),
    (200, 8192, 32, 0, 1, 256): single(16, 8),
    # ---- the explicit codes at 79 buckets (3 x 5000): 34, 66, 68 fit; 36, 40, 72 need 128, 256, 128 buckets -> 16 waves
    (3, 5000, 1250, 34, 1, 256): cluster(4, 16, 2, 1, 8), (3, 5000, 1250, 66, 1, 256): cluster(8, 8, 2, 1, 8),
    (3, 5000, 1250, 68, 1, 256): cluster(4, 8, 4, 1, 8), (3, 5000, 1250, 36, 1, 256): single(16, 8),
    (3, 5000, 1250, 40, 1, 256): single(16, 8), (3, 5000, 1250, 72, 1, 256): single(16, 8),
    # 2304 points = 36 buckets: only two workgroups of 8 waves fit (two of 16 need 64)
    (6, 2304, 600, 66, 1, 256): cluster(4, 8, 2, 1, 4), (6, 2304, 600, 34, 1, 256): single(16, 4),
    # the smallest plot of each code (2 slots per wave), and one bucket less
    (1, 4096, 32, 34, 1, 256): cluster(2, 16, 2, 1, 4), (1, 4032, 32, 34, 1, 256): single(16, 4),
    (1, 8192, 32, 36, 1, 256): cluster(2, 16, 4, 1, 8), (1, 8128, 32, 36, 1, 256): single(16, 8),
    (1, 16384, 32, 40, 1, 256): cluster(2, 16, 8, 1, 16), (1, 16320, 32, 40, 1, 256): single(16, 16),
    (1, 2052, 32, 66, 1, 256): cluster(4, 8, 2, 1, 4), (1, 4096, 32, 68, 1, 256): cluster(2, 8, 4, 1, 4),
    (1, 4032, 32, 68, 1, 256): single(16, 4), (1, 8192, 32, 72, 1, 256): cluster(2, 8, 8, 1, 8), (1, 8128, 32, 72, 1, 256): single(16, 8),
    # all six at 2 x 32 768 (512 buckets), and on a chip too small for B * P workgroups
    (2, 32768, 1024, 34, 1, 256): cluster(16, 16, 2, 0, 32), (2, 32768, 1024, 36, 1, 256): cluster(8, 16, 4, 0, 32),
    (2, 32768, 1024, 40, 1, 256): cluster(4, 16, 8, 1, 32), (2, 32768, 1024, 66, 1, 256): cluster(32, 8, 2, 0, 32),
    (2, 32768, 1024, 68, 1, 256): cluster(16, 8, 4, 0, 32), (2, 32768, 1024, 72, 1, 256): cluster(8, 8, 8, 1, 32),
    (2, 32768, 1024, 72, 1, 15): single(16, 32), (2, 32768, 1024, 72, 1, 16): cluster(8, 8, 8, 1, 32),
    # the upper bound, 512 buckets per workgroup: 64 slots x 8 waves, 32 x 16; beyond it 16 waves
    (1, 65536, 32, 66, 1, 256): cluster(64, 8, 2, 0, 64), (1, 65540, 32, 66, 1, 256): single(16, 128),
    (1, 65536, 32, 34, 1, 256): cluster(32, 16, 2, 0, 64), (1, 65540, 32, 34, 1, 256): single(16, 128),
    (1, 131072, 32, 68, 1, 256): cluster(64, 8, 4, 0, 128), (1, 131072, 32, 36, 1, 256): cluster(32, 16, 4, 0, 128),
    (1, 131072, 32, 40, 1, 256): cluster(16, 16, 8, 0, 128), (1, 131072, 32, 72, 1, 256): cluster(32, 8, 8, 0, 128),
    (1, 100000, 257, 36, 1, 256): cluster(32, 16, 4, 0, 128), (1, 100000, 257, 72, 1, 256): cluster(32, 8, 8, 0, 128),
    # the give-up test's shape
    (4, 32768, 512, 72, 1, 256): cluster(8, 8, 8, 1, 32), (4, 32768, 512, 36, 1, 256): cluster(8, 16, 4, 0, 32),
    (4, 32768, 512, 0, 1, 256): cluster(8, 8, 8, 1, 32),
    # ---- beyond every kernel, and the argument checks (which come first)
    (1, 131076, 64, 0, 1, 256): ELIMIT, (1, 131076, 64, 0, 0, 256): ELIMIT, (1, 131076, 64, 72, 1, 256): ELIMIT,
    (1, 131076, 64, 16, 1, 256): ELIMIT, (1, 131076, 64, 3, 1, 256): EINVAL,
    (2, 4096, 512, 3, 1, 256): EINVAL, (2, 4096, 512, 35, 1, 256): EINVAL, (2, 4096, 512, -1, 1, 256): EINVAL,
    (2, 4096, 512, 3, 0, 256): EINVAL, (2, 4096, 512, 32, 1, 256): EINVAL, (2, 4096, 512, 64, 1, 256): EINVAL,
    (2, 4096, 512, 2, 1, 256): EINVAL, (2, 4096, 512, 38, 1, 256): EINVAL, (2, 4096, 512, 80, 1, 256): EINVAL,
    (0, 4096, 512, 0, 1, 256): EINVAL, (2, 0, 0, 0, 1, 256): EINVAL, (2, 4096, 0, 0, 1, 256): EINVAL, (2, 4096, 4097, 0, 1, 256): EINVAL,
}


def test_route_table_written_from_the_dispatch_before_the_plan():
    raw = _raw_lib()
    for args, want in TABLE.items():
        assert _route(raw, *args) == want, args
    # the rows the table must hold, spelled out
    assert TABLE[(16, 32768, 1024, 0, 1, 256)] == (CLUSTER, 8, 8, 8, 1, 32, 1)
    assert TABLE[(16, 32768, 1024, 0, 1, 64)][:3] == (CLUSTER, 8, 4) and TABLE[(16, 32768, 1024, 0, 1, 16)][:2] == (SPEC, 16)
    assert TABLE[(3, 5000, 1250, 36, 1, 256)][:2] == (SPEC, 16)
    assert TABLE[(4, 16385, 32, 4, 1, 256)][:2] == TABLE[(1, 16388, 32, 4, 1, 256)][:2] == (SPEC, 8)
    assert TABLE[(1, 32772, 32, 8, 1, 256)][:2] == (SPEC, 16)
    assert TABLE[(33, 4096, 64, 0, 1, 256)] == (BRUTE, 4, 1, 16, 0, 0, 0) and TABLE[(1, 2049, 100, 72, 1, 256)][0] == BRUTE
    # every template rung of every ladder is in the table
    got = {}
    for r in TABLE.values():
        if not isinstance(r, int):
            got.setdefault((r[0], r[1]), set()).add(r[3])
    assert got[(BRUTE, 4)] == {1, 2, 4, 16} and got[(BRUTE, 16)] == {2, 4, 8, 16, 32}
    assert got[(SPEC, 16)] == got[(ROUND, 16)] == {4, 8, 16, 32, 64, 128}
    assert got[(SPEC, 8)] == {8, 16, 32, 64} and got[(SPEC, 4)] == {32, 64}
    assert got[(CLUSTER, 8)] == {2, 4, 8, 16, 32, 64} and got[(CLUSTER, 16)] == {2, 4, 8, 16, 32}
    assert {(r[1], r[2]) for r in TABLE.values() if not isinstance(r, int) and r[0] == CLUSTER} == {
        (nw, p) for nw in (8, 16) for p in (2, 4, 8)}
    # a NULL result pointer; nothing is written on a refusal
    assert raw.sn2_fps_route(2, 4096, 512, 0, 1, 256, None) == EINVAL
    from stratanet2_vegetation_coverage_maps_amd import _lib
    r = _lib.FpsRoute(-9, -9, -9, -9, -9, -9, -9)
    assert raw.sn2_fps_route(2, 32769, 32, 0, 0, 256, ctypes.byref(r)) == ELIMIT and r.form == r.rung == -9


def test_fills_ws_is_the_exported_predicate_whatever_the_request():
    raw = _raw_lib()
    for B in (1, 2, 3, 32, 33):
        for N in (2048, 2049, 2052, 4096, 4097, 4100, 32768, 131072):
            for M in (16, 17, 64):
                want = raw.sn2_fps_fills_ws(B, N, M)
                for waves in (0, 1, 4, 8, 16, 34, 36, 40, 66, 68, 72):
                    for cus in (8, 256):
                        got = _route(raw, B, N, M, waves, 1, cus)
                        if want or N <= 32768:
                            assert got[6] == want and (got[0] == BRUTE) == (not want), (B, N, M, waves, cus)
                        else:
                            assert got == ELIMIT, (B, N, M, waves, cus)
                        none = _route(raw, B, N, M, waves, 0, cus)
                        assert none == ELIMIT if N > 32768 else none[6] == 0 and none[0] == BRUTE, (B, N, M, waves, cus)


def test_the_entry_point_refuses_what_the_plan_refuses():
    """The codes tests/test_cabi.py and tests/test_fps_live_host.py pin on sn2_fps_status / sn2_fps_live, from the plan and from the
    entry point (fake pointers: every call below fails a check before any device work); an unknown `waves` comes before the size
    limit, a NULL pointer before either."""
    raw = _raw_lib()
    fake = 0x1000
    for ws in (fake, None):
        assert raw.sn2_fps_status(fake, 1, 131076, 64, None, fake, fake, fake, ws, 0, None, None) == ELIMIT
        assert _route(raw, 1, 131076, 64, 0, int(ws is not None)) == ELIMIT
        for waves in (3, 35, -1):
            assert raw.sn2_fps_status(fake, 1, 131076, 64, None, fake, fake, fake, ws, waves, None, None) == EINVAL
            assert raw.sn2_fps_status(fake, 2, 4096, 512, None, fake, fake, fake, ws, waves, None, None) == EINVAL
            assert _route(raw, 1, 131076, 64, waves, int(ws is not None)) == EINVAL
        for B, N, M in ((0, 4096, 512), (2, 0, 512), (2, 4096, 0), (2, 4096, 4097)):
            assert raw.sn2_fps_live(fake, B, N, M, None, None, fake, fake, fake, ws, 3, None, None, None) == EINVAL
            assert raw.sn2_fps_live(fake, B, N, M, None, None, fake, fake, fake, ws, 0, None, None, None) == EINVAL
            assert _route(raw, B, N, M, 0, int(ws is not None)) == EINVAL
        assert raw.sn2_fps_live(None, 1, 131076, 64, None, None, fake, fake, fake, ws, 0, None, None, None) == EINVAL
    # a workspace that is not 16-byte aligned is no workspace
    assert raw.sn2_fps_status(fake, 1, 32772, 64, None, fake, fake, fake, fake + 4, 0, None, None) == ELIMIT


def test_hip_ops_fps_route_is_the_plan(monkeypatch):
    """hip_ops.fps_route: the device's compute units, bucketed=False = no workspace, a refusal raises."""
    import types
    import torch
    from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
    monkeypatch.setattr(torch.cuda, "get_device_properties", lambda d: types.SimpleNamespace(multi_processor_count=256))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    r = ops.fps_route(16, 32768, 1024)
    assert tuple(r) == TABLE[(16, 32768, 1024, 0, 1, 256)] and (r.form, r.nw, r.p, r.rung) == (ops.FPS_FORM_CLUSTER, 8, 8, 8)
    assert tuple(ops.fps_route(16, 32768, 1024, bucketed=False)) == TABLE[(16, 32768, 1024, 0, 0, 256)]
    assert ops.fps_route(3, 5000, 1250, waves=36).form == ops.FPS_FORM_SPEC and ops.fps_route(1, 2052, 32, waves=1).form == ops.FPS_FORM_ROUND
    with pytest.raises(ops.StrataHipError):
        ops.fps_route(1, 131076, 64)
