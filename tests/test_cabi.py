"""The C-ABI library builds in-tree, loads, and exports every symbol include/strata_hip.h declares (CPU only: no
compute call is made)."""
import ctypes
import os
import re

from conftest import ROOT


def _declared(ret="int"):
    txt = open(os.path.join(ROOT, "include", "strata_hip.h")).read()
    return sorted(set(re.findall(r"^%s\s+(sn2_\w+)\s*\(" % ret, txt, flags=re.M)))


def test_header_declares_the_hot_path():
    names = _declared()
    for must in ("sn2_fps", "sn2_ball_query", "sn2_three_nn", "sn2_sa_forward", "sn2_sa_backward", "sn2_fp_forward",
                 "sn2_fp_backward", "sn2_head_forward", "sn2_head_backward", "sn2_plot_project_forward",
                 "sn2_plot_project_backward", "sn2_raster_project", "sn2_version"):
        assert must in names


def test_library_builds_loads_and_exports_everything():
    from stratanet2_vegetation_coverage_maps_amd import _build, _lib
    path = _build.build(verbose=False)
    assert os.path.exists(path)
    raw = ctypes.CDLL(path)
    for name in _declared() + _declared("size_t"):
        assert hasattr(raw, name), f"{name} declared in strata_hip.h but not exported"
    lib = _lib.load()
    assert lib.sn2_version() == _lib.SN2_VERSION
    assert set(_lib.SIGNATURES) == set(_declared()), "ctypes binding and header disagree"
    assert set(_lib.SIZE_HELPERS) == set(_declared("size_t")), "ctypes binding and header disagree on the size helpers"


def test_build_lists_every_unit_and_header_of_csrc():
    """HEADERS drives the stale-object check of the build: a header missing from it means silently stale objects, a unit missing
    from SOURCES entry points that never reach the library."""
    from stratanet2_vegetation_coverage_maps_amd import _build
    files = os.listdir(_build.CSRC)
    assert sorted(f for f in files if f.endswith(".hip")) == sorted(_build.SOURCES)
    assert sorted(f for f in files if f.endswith(".h")) == sorted(h for h in _build.HEADERS if os.sep not in h)
    assert len(set(_build.SOURCES)) == len(_build.SOURCES) and len(set(_build.HEADERS)) == len(_build.HEADERS)
    assert {"ball_query.hip", "three_nn.hip", "znorm.hip"} <= set(_build.SOURCES) and "fps_ws.h" in _build.HEADERS


def test_struct_layouts_match_the_header_abi():
    """sizeof of the ctypes mirrors == what a C compiler computes for the header's structs."""
    import subprocess
    import tempfile
    from stratanet2_vegetation_coverage_maps_amd import _lib
    src = ('#include <stdio.h>\n#include "strata_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n",'
           'sizeof(sn2_block),sizeof(sn2_sa),sizeof(sn2_fp),sizeof(sn2_head),sizeof(sn2_net_layer),sizeof(sn2_net_model),'
           'sizeof(sn2_net_dims),sizeof(sn2_net_geo),sizeof(sn2_net_act),sizeof(sn2_net_bwd),sizeof(sn2_net_io),sizeof(sn2_fps_route_t));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    assert sizes == [ctypes.sizeof(c) for c in (_lib.Block, _lib.SA, _lib.FP, _lib.Head, _lib.NetLayer, _lib.NetModel, _lib.NetDims,
                                                _lib.NetGeo, _lib.NetAct, _lib.NetBwd, _lib.NetIO, _lib.FpsRoute)]


# (B, N, M1, M2): the metric's shape and a tiny batch
_SHAPES = [(16, 32768, 1024, 256), (2, 64, 16, 4)]


def _size_cases(B, N, M1, M2):
    """(helper of the library, its arguments, the header's macro call, the hip_ops function that wraps it or None)"""
    from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
    K, cells = (5000, 12345) if N > 1000 else (2, 4)
    return [
        ("sn2_fps_ws_words", (B, N), f"SN2_FPS_WS_WORDS({B},{N})", lambda: ops.fps_ws_words(B, N)),
        ("sn2_fps_ws_grid_offset", (B, N), f"SN2_FPS_WS_GRID_OFFSET({B},{N})", None),
        ("sn2_fps_ws_ctl_offset", (B, N), f"SN2_FPS_WS_CTL_OFFSET({B},{N})", None),
        ("sn2_fps_ws_rank_offset", (B, N), f"SN2_FPS_WS_RANK_OFFSET({B},{N})", None),
        ("sn2_three_nn_ws_words", (B, M1), f"SN2_THREE_NN_WS_WORDS({B},{M1})", lambda: ops.three_nn_ws_words(B, M1)),
        ("sn2_three_nn_xy_ws_words", (B, M1, N), f"SN2_THREE_NN_XY_WS_WORDS({B},{M1},{N})", lambda: ops.three_nn_ws_words(B, M1, N)),
        ("sn2_znorm_ws_words", (N, cells), f"SN2_ZNORM_WS_WORDS({N},{cells})", None),
        ("sn2_sa_order_words", (B, M1), f"SN2_SA_ORDER_WORDS({B},{M1})", lambda: ops.sa_order_len(B, M1)),
        ("sn2_interp_chunks", (N, M1), f"SN2_INTERP_CHUNKS({N},{M1})", lambda: ops.interp_chunks(N, M1)),
        ("sn2_interp_ws_words", (B, N, M1), f"SN2_INTERP_WS_WORDS({B},{N},{M1})", lambda: ops.interp_ws_words(B, N, M1)),
        ("sn2_interp_ws_words", (B, M2, 1), f"SN2_INTERP_WS_WORDS({B},{M2},1)", lambda: ops.interp_ws_words(B, M2, 1)),
        ("sn2_fp_src_ws_words", (B, N, M1, 34), f"SN2_FP_SRC_WS_WORDS({B},{N},{M1},34)", lambda: ops.fp_src_ws_words(B, N, M1, 34)),
        ("sn2_global_xchg_words", (B,), f"SN2_GLOBAL_XCHG_WORDS({B})", None),
        ("sn2_p2_key_parts", (N,), f"SN2_P2_KEY_PARTS({N})", lambda: ops.p2_key_parts(N)),
        ("sn2_kde_fit_ws_words", (K,), f"SN2_KDE_FIT_WS_WORDS({K})", lambda: ops.kde_fit_ws_words(K)),
    ]


def test_constants_and_size_helpers_match_the_header_macros():
    """Header -> library -> Python, closed: a C compiler prints every scalar macro that `_lib.CONSTANTS` names and every size
    macro at two shapes; the Python constants, the library's size helpers and the hip_ops functions over them must give
    those numbers.  Every size helper the binding knows (but the four whose rule is no macro) is covered."""
    import subprocess
    import tempfile
    from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
    from stratanet2_vegetation_coverage_maps_amd import _lib
    lib = _lib.load()
    names = sorted(_lib.CONSTANTS)
    cases = [c for shape in _SHAPES for c in _size_cases(*shape)]
    assert {c[0] for c in cases} == set(_lib.SIZE_HELPERS) - {"sn2_parcel_count_ws_words", "sn2_parcel_znorm_ws_words",
                                                              "sn2_subsample_ws_words", "sn2_plot_losses_ws_words"}
    exprs = names + [c[2] for c in cases]
    src = '#include <stdio.h>\n#include "strata_hip.h"\nint main(){\n' + "".join(
        f'printf("%lld\\n", (long long)({e}));\n' for e in exprs) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "m.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "m")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = [int(x) for x in subprocess.check_output([exe]).split()]
    assert len(vals) == len(exprs)
    for n, v in zip(names, vals):
        assert _lib.CONSTANTS[n] == v and getattr(_lib, n) == v, n
    for (helper, args, macro, py), v in zip(cases, vals[len(names):]):
        assert getattr(lib, helper)(*args) == v, macro
        if py is not None:
            assert py() == v, macro
    # the names the package and its tests have always used are those constants
    assert (ops.GL_MAX_PLOTS, ops.GL_BWD_MAX_ROWS, ops.GRAD_IMAGES, ops.SA_BWD_WS_WORDS, _lib.STAT_SLOTS, _lib.BN_FROZEN_KEEP) == tuple(
        _lib.CONSTANTS[n] for n in ("SN2_GLOBAL_MAX_PLOTS", "SN2_GLOBAL_BWD_MAX_ROWS", "SN2_NET_GRAD_IMAGES", "SN2_SA_BWD_WS_WORDS",
                                    "SN2_STAT_SLOTS", "SN2_BN_FROZEN_KEEP"))
    assert (ops.LOSS_BLOCKS, ops.PROJECTED_LOSS_WS, ops.KDE_FIT_MAX_K, ops.SUBSAMPLE_LDS_MAX) == tuple(
        _lib.CONSTANTS[n] for n in ("SN2_LOSS_BLOCKS", "SN2_PROJECTED_LOSS_WS", "SN2_KDE_FIT_MAX_K", "SN2_SUBSAMPLE_LDS_MAX"))
    assert (_lib.NET_FORK, _lib.NET_HAS_INVERTED) == (_lib.CONSTANTS["SN2_NET_FORK"], _lib.CONSTANTS["SN2_NET_HAS_INVERTED"])


def test_route_predicates_on_each_side_of_every_boundary():
    """The route rules of the library (include/strata_hip.h, "Routes") against the rules as the commit before them stated them
    in four languages, written out here as literals ON PURPOSE: this is the second statement that pins the first."""
    from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
    from stratanet2_vegetation_coverage_maps_amd import _lib
    lib = _lib.load()
    fps = {(1, 2048, 64): 0, (1, 2052, 64): 1, (1, 2052, 16): 0, (1, 2052, 17): 1, (1, 2049, 64): 0, (33, 4096, 64): 0,
           (32, 4096, 64): 1, (33, 4100, 64): 1, (1, 131072, 64): 1, (1, 131076, 64): 0}
    for a, want in fps.items():
        assert lib.sn2_fps_fills_ws(*a) == want and ops.fps_fills_ws(*a) is bool(want), a
    for a, want in {(127, 2049): 0, (128, 2049): 1, (128, 2048): 0, (8192, 2049): 1, (8193, 2049): 0}.items():
        assert lib.sn2_three_nn_uses_grid(*a) == want and ops.three_nn_uses_grid(*a) is bool(want), a
    assert lib.sn2_fp_rows_small(65536) == 1 and lib.sn2_fp_rows_small(65537) == 0
    assert ops.fp_rows_small(65536) is True and ops.fp_rows_small(65537) is False
    for cb, want in {0: 0, 3: 0, 20: 0, 4: 1, 8: 1, 16: 1}.items():
        assert lib.sn2_fp_source_side(65537, cb, 0) == want and ops.fp_source_side(65537, cb) is bool(want), cb
    assert lib.sn2_fp_source_side(65536, 8, 0) == 0 and lib.sn2_fp_source_side(65536, 8, 1) == 1
    assert ops.fp_source_side(65536, 8) is False and ops.fp_source_side(65536, 8, True) is True
    for a, want in {(28, 0): 1, (29, 0): 0, (28, 1): 0}.items():
        assert lib.sn2_global_level_forward_route(*a) == want, a
    for a, want in {(28, 256, 0, 0): 1, (28, 257, 0, 0): 0, (29, 256, 0, 0): 0, (28, 256, 1, 0): 0, (28, 256, 0, 1): 0}.items():
        assert lib.sn2_global_level_backward_route(*a) == want, a

    class Blk:
        def __init__(self, bf16):
            self.mma_bf16 = bf16
    f32, b16 = Blk(False), Blk(True)
    assert ops.global_level_forward_fused(28, f32, f32) is True and ops.global_level_forward_fused(29, f32, f32) is False
    assert ops.global_level_forward_fused(28, f32, b16) is False
    assert ops.global_level_backward_fused(28, 256, False, f32, f32) is True
    assert ops.global_level_backward_fused(28, 257, False, f32, f32) is False and ops.global_level_backward_fused(28, 256, True, f32, f32) is False
    assert ops.global_level_backward_fused(29, 256, False, f32, f32) is False and ops.global_level_backward_fused(28, 256, False, b16, f32) is False
    # sn2_three_nn_xy refuses source counts outside the grid search's range before any device work (fake pointers: never dereferenced)
    fake = 0x1000
    for S, want in ((127, -2), (8193, -2)):
        assert lib.sn2_three_nn_xy(fake, 1, S, fake, 4096, 3, fake, fake, fake, None) == want, S
    # plots beyond the largest bucketed kernel: SN2_ELIMIT with a workspace as without one, before any device work
    assert lib.sn2_fps_status(fake, 1, 131076, 64, None, fake, fake, fake, fake, 0, None, None) == -2
    assert lib.sn2_fps_status(fake, 1, 131076, 64, None, fake, fake, fake, None, 0, None, None) == -2
    # the plan behind those two refusals, and on each side of the workspace predicate (tests/test_fps_route_host.py: the whole table)
    r = _lib.FpsRoute()
    for ws in (1, 0):
        assert lib.sn2_fps_route(1, 131076, 64, 0, ws, 256, r) == -2 and lib.sn2_fps_route(1, 131072, 64, 3, ws, 256, r) == -1
    for a, want in fps.items():
        assert lib.sn2_fps_route(*a, 16, 1, 256, r) == (0 if a[1] <= 131072 else -2), a
        assert a[1] > 131072 or (r.fills_ws == want and (r.form != _lib.SN2_FPS_FORM_BRUTE) == bool(want)), a


def test_argument_checks_return_before_any_device_work():
    """The entry points validate their descriptors first and return SN2_EINVAL (-1) / SN2_ELIMIT (-2) without touching the
    device: checked here for the newest one, the fused global level (shapes other than the reference architecture's, bfloat16
    operands and NULL workspaces are refused -- the host then uses the separate calls)."""
    from stratanet2_vegetation_coverage_maps_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH if os.path.exists(_lib.LIB_PATH) else __import__(
        "stratanet2_vegetation_coverage_maps_amd._build", fromlist=["build"]).build(verbose=False))
    fn = raw.sn2_global_level_forward
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.POINTER(_lib.FP), ctypes.POINTER(_lib.FP)] + [ctypes.c_void_p] * 5
    sa3, fp3 = _lib.FP(), _lib.FP()
    assert fn(None, None, None, None, None, None, None) == -1
    fake = 0x1000                                            # never dereferenced: every call below fails a check first
    sa3.B = fp3.B = 4
    sa3.R_per_plot = fp3.R_per_plot = sa3.S_per_plot = 256
    fp3.S_per_plot = 1
    sa3.ca, sa3.cb, fp3.ca, fp3.cb = 32, 3, 64, 32
    sa3.blk.cin, sa3.blk.cout, fp3.blk.cin, fp3.blk.cout = 35, 64, 96, 48          # FP3 with 48 outputs: not the architecture
    assert fn(ctypes.byref(sa3), ctypes.byref(fp3), fake, fake, fake, fake, None) == -2
    fp3.blk.cout = 64
    fp3.blk.mma_bf16 = 1                                                            # bfloat16 operands: the separate kernels
    assert fn(ctypes.byref(sa3), ctypes.byref(fp3), fake, fake, fake, fake, None) == -2
    fp3.blk.mma_bf16 = 0
    fp3.S_per_plot = 256                                                            # FP3 must interpolate the plot's ONE source
    assert fn(ctypes.byref(sa3), ctypes.byref(fp3), fake, fake, fake, fake, None) == -1
    fp3.S_per_plot = 1
    assert fn(ctypes.byref(sa3), ctypes.byref(fp3), fake, fake, fake, fake, None) == -1   # no rows, tables or weights given


def _net_model_shell(max_neighbors=2000, n_flat=14997, source_side=1, fuse_eval_head=1):
    """A sn2_net_model with the reference architecture's layer shapes and no pointers: what the layout and the argument checks read."""
    from stratanet2_vegetation_coverage_maps_amd import _lib
    m = _lib.NetModel()
    for L, (ci, co) in zip([m.sa1[0], m.sa1[1], m.sa2, m.sa3, m.fp3, m.fp2, m.fp1],
                           [(11, 16), (16, 16), (19, 32), (35, 64), (96, 64), (80, 34), (42, 34)]):
        L.cin, L.cout = ci, co
    m.n_flat, m.max_neighbors, m.source_side, m.fuse_eval_head = n_flat, max_neighbors, source_side, fuse_eval_head
    return m


def _dims(B, N, M1, M2, maxn=2000, act_bf16=0, p2=0):
    from stratanet2_vegetation_coverage_maps_amd import _lib
    d = _lib.NetDims()
    d.B, d.N, d.M1, d.M2, d.cap1, d.cap2, d.act_bf16, d.p2_diam_pix = B, N, M1, M2, min(maxn, N), min(maxn, M1), act_bf16, p2
    return d


def test_network_executor_layouts_match_the_host_shape_tables():
    """sn2_net_geo_carve / sn2_net_act_carve (host-only arithmetic, no device): every buffer 256-byte aligned, no two overlap, each
    at least as large as the shape the host views it with (executor._geo_shapes / _act_shapes), everything inside the arena --
    for the metric's shape, the reference defaults, config 5's plots in bfloat16 and a tiny batch."""
    from ctypes import byref
    from stratanet2_vegetation_coverage_maps_amd import _lib
    from stratanet2_vegetation_coverage_maps_amd import executor as X
    lib = _lib.load()
    base = X._FAKE_BASE
    for (B, N, M1, M2, bf, p2) in [(16, 32768, 1024, 256, 0, 20), (20, 10000, 2500, 625, 0, 0), (8, 131072, 1024, 256, 1, 0),
                                   (2, 64, 16, 4, 0, 0), (512, 10000, 2500, 625, 0, 0)]:
        m, d = _net_model_shell(), _dims(B, N, M1, M2, act_bf16=bf, p2=p2)
        sz = ctypes.c_size_t()
        g = _lib.NetGeo()
        assert lib.sn2_net_geo_carve(byref(m), byref(d), base, byref(g), byref(sz)) == 0
        offs = X._offsets(g, X._geo_shapes(B, N, M1, M2, d.cap1, d.cap2))
        assert ("p2_pix" in offs) == (p2 > 0) and ("ws1" in offs) == (N > 2048 and not (N <= 4096 and B > 32))
        spans = sorted((o, o + X._ITEM[dt] * int(__import__("math").prod(sh))) for o, dt, sh in offs.values())
        assert all(o % 256 == 0 for o, _ in spans) and spans[-1][1] <= sz.value
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        for training in (0, 1):
            a = _lib.NetAct()
            assert lib.sn2_net_act_carve(byref(m), byref(d), training, base, byref(a), byref(sz)) == 0
            offs = X._offsets(a, X._act_shapes(B, N, M1, M2, bf))
            assert ("h1" in offs) == bool(training or bf)               # the fused eval pass keeps no per-point rows
            spans = sorted((o, o + X._ITEM[dt] * int(__import__("math").prod(sh))) for o, dt, sh in offs.values())
            assert all(o % 256 == 0 for o, _ in spans) and spans[-1][1] <= sz.value
            assert all(x[1] <= y[0] for x, y in zip(spans, spans[1:]))
        bw = _lib.NetBwd()
        sz2 = ctypes.c_size_t()
        assert lib.sn2_net_bwd_carve(byref(m), byref(d), base, base, byref(bw), byref(sz), byref(sz2)) == 0
        stride = (14997 + 63) // 64 * 64
        assert bw.images == 32 and bw.image_stride == stride and bw.arena_words * 4 == sz.value
        assert bw.dy2 - base == 32 * stride * 4 and bw.dy_sa3 - base + B * M2 * 64 * 4 <= sz.value


def test_network_executor_argument_checks_return_before_any_device_work():
    from ctypes import byref
    from stratanet2_vegetation_coverage_maps_amd import _lib
    lib = _lib.load()
    m, d = _net_model_shell(), _dims(4, 4096, 512, 128)
    g, a, b, io = _lib.NetGeo(), _lib.NetAct(), _lib.NetBwd(), _lib.NetIO()
    sz = ctypes.c_size_t()
    assert lib.sn2_net_geo_carve(None, byref(d), None, byref(g), byref(sz)) == -1
    assert lib.sn2_net_geometry(byref(m), byref(d), byref(g), byref(io), None) == -1          # no tables
    assert lib.sn2_net_forward(byref(m), byref(d), byref(g), byref(a), byref(io), None) == -1  # no parameters
    assert lib.sn2_net_backward(byref(m), byref(d), byref(g), byref(a), byref(b), None) == -1
    d.cap1 = 100                                                                                # not min(max_neighbors, N)
    assert lib.sn2_net_geo_carve(byref(m), byref(d), None, byref(g), byref(sz)) == -1
    d = _dims(4, 4096, 512, 128)
    m.fp2.cout = 48                                                                             # not the reference architecture
    assert lib.sn2_net_geo_carve(byref(m), byref(d), None, byref(g), byref(sz)) == -2
    assert lib.sn2_net_ctx_destroy(None) == -1


_FAKE = 0x1000                        # a non-NULL pointer value: sn2_fp_form launches nothing and dereferences nothing
_SPLIT, _SRC, _DENSE, _ELIMIT, _EINVAL = 0, 1, 2, -2, -1


def _fp_shell(name, B, N, M1, M2, src_ws=False, backward=False, act_bf16=0):
    """The sn2_fp of one of the six dense-row blocks as the network hands it out (csrc/net.hip, point_net2.py), every pointer
    fake.  backward: the buffers the backward pass adds (dsrc everywhere; du_scratch and the inverted index on the k-NN blocks;
    dskip where the skip input has a gradient: FP3, FP2, FP4)."""
    from stratanet2_vegetation_coverage_maps_amd import _lib
    M3 = max(M2 // 4, 1)              # the third ball-query level of the 3sa architecture
    ca, cb, cout, knn, Rp, Sp, src_stride, skip_stride, dskip = {
        "SA3": (32, 3, 64, False, M2, M2, 32, 4, False), "FP3": (64, 32, 64, True, M2, 1, 64, 32, True),
        "FP2": (64, 16, 34, True, M1, M2, 64, 16, True), "FP1": (34, 8, 34, True, N, M1, 36, 12, False),
        "GSA": (64, 3, 64, False, M3, M3, 64, 4, False), "FP4": (64, 64, 64, True, M3, 1, 64, 64, True)}[name]
    p = _lib.FP()
    p.B, p.R_per_plot, p.S_per_plot, p.ca, p.cb = B, Rp, Sp, ca, cb
    p.src, p.src_stride, p.skip, p.skip_stride = _FAKE, src_stride, _FAKE, skip_stride
    if knn:
        p.knn_idx = p.knn_w = _FAKE
    p.blk.cin, p.blk.cout, p.blk.W, p.blk.b = ca + cb, cout, _FAKE, _FAKE
    p.h, p.h_stride = _FAKE, (cout + 3) // 4 * 4
    p.dy = p.blk.dW = p.blk.db = p.blk.dgamma = p.blk.dbeta = _FAKE
    p.blk.grad_replicas = 1
    if src_ws and name in ("FP1", "FP2"):
        p.src_ws = _FAKE
    if name == "FP1":
        p.act_bf16 = act_bf16
    if backward:
        p.dsrc, p.dsrc_stride, p.bn_sums_done = _FAKE, src_stride, _FAKE
        if knn:
            p.du_scratch, p.scatter_ws, p.scatter_ready = _FAKE, _FAKE, 1
        if dskip:
            p.dskip, p.dskip_stride = _FAKE, skip_stride
    return p


def test_fp_form_table_of_the_six_blocks():
    """sn2_fp_form against the forms written out BY HAND from the dispatch of the commit before it (fp_forward_t / fp_backward_t
    of csrc/fp.hip), for the six blocks at four shapes.  Columns: passes 0, 1, 2, the backward with its buffers, the backward
    without dsrc / du_scratch / scatter_ws.  R = B * rows per plot; small = R <= 65 536."""
    from ctypes import byref
    from stratanet2_vegetation_coverage_maps_amd import _lib
    lib = _lib.load()
    S, Q, D, L = _SPLIT, _SRC, _DENSE, _ELIMIT
    small = (S, S, S, S, S)                      # at most 65 536 rows: the matrix-core kernels in every pass
    rows = (S, D, D, D, D)                       # more rows, no source-side form: only the eval pass stays on the matrix cores
    others = ("SA3", "FP3", "GSA", "FP4")
    table = {
        # every block small (FP1: 128 rows)
        (2, 64, 16, 4): {(n, ws): small for n in others + ("FP2", "FP1") for ws in (1, 0)},
        # FP1: 524 288 rows; FP2: 16 384
        (16, 32768, 1024, 256): {**{(n, ws): small for n in others + ("FP2",) for ws in (1, 0)},
                                 ("FP1", 1): (Q, Q, Q, Q, D), ("FP1", 0): rows},
        # SA3 / FP3: 320 000 rows, FP2: 1 280 000 (its backward writes dskip: no source-side backward), FP1: 5 120 000,
        # the 3sa blocks: 79 872
        (512, 10000, 2500, 625): {**{(n, ws): rows for n in others for ws in (1, 0)},
                                  ("FP2", 1): (Q, Q, Q, D, D), ("FP2", 0): rows,
                                  ("FP1", 1): (Q, Q, Q, Q, D), ("FP1", 0): rows},
        # bfloat16 rows on FP1 (1 048 576 rows): the source-side form or nothing
        (8, 131072, 1024, 256): {**{(n, ws): small for n in others + ("FP2",) for ws in (1, 0)},
                                 ("FP1", 1): (Q, Q, Q, Q, L), ("FP1", 0): (L, L, L, L, L)},
    }
    for shape, forms in table.items():
        bf = int(shape[1] == 131072)
        assert len(forms) == 12
        for (name, ws), want in forms.items():
            got = tuple(lib.sn2_fp_form(byref(_fp_shell(name, *shape, src_ws=bool(ws), backward=(col == 3), act_bf16=bf)), min(col, 3))
                        for col in range(5))
            assert got == want, (shape, name, ws, got)
    # the rows the form table must hold, spelled out
    assert table[(2, 64, 16, 4)][("FP1", 1)][:4] == table[(2, 64, 16, 4)][("FP1", 0)][:4] == (S, S, S, S)
    assert table[(16, 32768, 1024, 256)][("FP1", 1)][1:4] == (Q, Q, Q)
    no_ws = table[(16, 32768, 1024, 256)][("FP1", 0)]
    assert (no_ws[0], no_ws[1], no_ws[3]) == (S, D, D)
    assert set(table[(8, 131072, 1024, 256)][("FP1", 0)]) == {L}
    # the query's own argument checks
    p = _fp_shell("FP1", 2, 64, 16, 4)
    assert lib.sn2_fp_form(byref(p), 4) == _EINVAL and lib.sn2_fp_form(byref(p), -1) == _EINVAL and lib.sn2_fp_form(None, 0) == _EINVAL
    p.blk.cout, p.h_stride = 48, 48                                      # not a block of the architecture
    assert lib.sn2_fp_form(byref(p), 1) == _ELIMIT


def test_fp_backward_refusals_come_from_the_plan():
    """What fp_backward_t used to refuse only after its first launches, sn2_fp_form(p, 3) -- the plan sn2_fp_backward runs before
    any launch -- refuses with the same code; each descriptor is accepted without its one defect."""
    from ctypes import byref
    from stratanet2_vegetation_coverage_maps_amd import _lib
    lib = _lib.load()

    def form(p):
        return lib.sn2_fp_form(byref(p), 3)
    # a small-row block with row_perm (was: after the BatchNorm-sum and the split kernel)
    p = _fp_shell("FP1", 2, 64, 16, 4, src_ws=True, backward=True)
    assert form(p) == _SPLIT
    p.row_perm = _FAKE
    assert form(p) == _ELIMIT
    # a k-NN block with dsrc and du_scratch but no scatter_ws: small rows (after the split kernel) and many (after fp_bwd_main_kernel)
    for shape, want in (((2, 64, 16, 4), _SPLIT), ((16, 32768, 1024, 256), _DENSE)):
        p = _fp_shell("FP1", *shape, backward=True)
        assert form(p) == want
        p.scatter_ws = None
        assert form(p) == _EINVAL
        p.scatter_ready = -1                     # the caller transposes the interpolation itself: no index wanted
        assert form(p) == want
    # the source-side form with B * CM chunk slots out of range (was: after fp_bwd_rows_kernel)
    p = _fp_shell("FP1", 4096, 65536, 8192, 256, src_ws=True, backward=True)
    assert form(p) == _ELIMIT
    p.B = 2048
    assert form(p) == _SRC
    # more than 8192 sources per plot (was: after the BatchNorm-sum launch), source-side form and the shared gather
    for ws, want in ((True, _SRC), (False, _DENSE)):
        p = _fp_shell("FP1", 16, 32768, 8192, 256, src_ws=ws, backward=True)
        assert form(p) == want
        p.S_per_plot = 8193
        assert form(p) == _ELIMIT
    # a missing du_scratch beside dsrc, and the gradient buffers every backward needs
    p = _fp_shell("FP1", 2, 64, 16, 4, backward=True)
    p.du_scratch = None
    assert form(p) == _EINVAL
    p = _fp_shell("FP1", 2, 64, 16, 4, backward=True)
    p.dy = None
    assert form(p) == _EINVAL and lib.sn2_fp_form(byref(p), 1) == _SPLIT
