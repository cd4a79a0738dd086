"""The geometry and pixel-id kernels ON their decisions: lattice plots, degenerate plots (zero-extent axes, one or two positions),
points planted at d2 = fp32(r*r) and one fp32 to either side of it, 3-NN targets at exactly equal distances from two sources, and
coordinates at the values where the pixel id steps (tests/_boundary_plots.py builds them; tests/test_boundary_plots_host.py shows
on the CPU that they reach those decisions and that `<=`, highest-index-wins, a fused multiply-add, a pre-multiplied scale or a
dropped epsilon would each give another answer on them).  Everything is compared with `torch.equal` against the oracle; every
case asserts, with the library's own predicates, the route it means to test."""
import functools

import numpy as np
import pytest
import torch

from oracle import check, network, projection
from oracle import primitives as P
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops

import _boundary_plots as bp
from test_gpu_fps_live import FORMS, assert_form_route

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32
KINDS = {"five": bp.KINDS5, "three": bp.KINDS3}
N1, M1, M2 = 2304, 576, 144                      # the size at which tests/test_gpu_fps_live.py reaches the bucketed forms


def _dev(t, dtype=None):
    return torch.as_tensor(t).to(DEV, dtype) if dtype is not None else torch.as_tensor(t).to(DEV)


@functools.lru_cache(maxsize=None)
def _fps_ref(kinds, n, m, row):
    """The oracle's samples of a batch, computed once: (start (B,), idx (B, m), cpos (B, 3, m))."""
    xyz = bp.batch(kinds, n)
    start = bp.repeated_and_fresh_starts(xyz)[row] if row < 2 else torch.full((xyz.shape[0],), bp.BALL_START)
    idx = P.fps_batched(xyz.permute(0, 2, 1).contiguous(), m, start)
    return start, idx, bp.gather_soa(xyz, idx)


@functools.lru_cache(maxsize=None)
def _fps2_ref(kinds, n, m, row):
    """Level 2: a quarter of level 1's samples, start BALL_START2 (row 2) or alternating 0 / last."""
    _, _, cs = _fps_ref(kinds, n, m, row)
    B = cs.shape[0]
    start = torch.full((B,), bp.BALL_START2) if row == 2 else torch.tensor([(m - 1) * (b & 1) for b in range(B)])
    idx = P.fps_batched(cs.permute(0, 2, 1).contiguous(), m // 4, start)
    return start, idx, bp.gather_soa(cs, idx)


def _assert_fps(got, ref_idx, ref_cs, what):
    idx, cs, ca = got[:3]
    B, m = ref_idx.shape
    assert torch.equal(idx.cpu().long(), ref_idx), what
    assert torch.equal(cs.cpu(), ref_cs), what
    assert torch.equal(ca.cpu().view(B, m, 4)[..., :3], ref_cs.permute(0, 2, 1)), what


# ---------------------------------------------------------------------------------------------------- FPS
@pytest.mark.parametrize("waves,bucketed", FORMS)
@pytest.mark.parametrize("which", ["five", "three"])
def test_fps_every_form_on_mixed_batches(which, waves, bucketed):
    """2304 -> 576 -> 144 on the mixed batches, from a start that is a repeat of an earlier point and from one that is not.  On the
    one-position plot every running distance is 0 from the first round: the oracle's answer (index 0, the lowest on the tie) is
    the expected one."""
    kinds = KINDS[which]
    xyz = bp.batch(kinds, N1)
    B = xyz.shape[0]
    assert ops.fps_fills_ws(B, N1, M1) and not ops.fps_fills_ws(B, M1, M2)
    assert_form_route(B, N1, M1, waves, bucketed)
    assert ops.fps_route(B, M1, M2, waves=waves, bucketed=bucketed, device=DEV).form == ops.FPS_FORM_BRUTE       # level 2, every form
    dev = xyz.to(DEV)
    for row in (0, 1):
        start, ref, ref_cs = _fps_ref(kinds, N1, M1, row)
        got = ops.fps(dev, M1, _dev(start, I32), bucketed=bucketed, waves=waves, return_ws=True)
        _assert_fps(got, ref, ref_cs, (kinds, waves, bucketed, row))
        assert (got[3] is not None) == bucketed
        if got[3] is not None:
            assert int(ops.fps_ws_ctl(got[3], B, N1)[1]) == 0
        start2, ref2, ref2_cs = _fps2_ref(kinds, N1, M1, row)
        got2 = ops.fps(got[1], M2, _dev(start2, I32), bucketed=bucketed, waves=waves, return_ws=True)
        _assert_fps(got2, ref2, ref2_cs, (kinds, waves, bucketed, row, "level 2"))
        assert got2[3] is None
    if "one" in kinds:
        b = kinds.index("one")
        assert ref[b, 1:].abs().max() == 0


@pytest.mark.parametrize("which", ["five", "three"])
def test_fps_at_the_brute_force_limit(which):
    kinds = KINDS[which]
    n, m = bp.BALL_SIZES[1]
    xyz = bp.batch(kinds, n)
    assert not ops.fps_fills_ws(xyz.shape[0], n, m)
    for row in (0, 1):
        start, ref, ref_cs = _fps_ref(kinds, n, m, row)
        for bucketed in (True, False):
            got = ops.fps(xyz.to(DEV), m, _dev(start, I32), bucketed=bucketed, return_ws=True)
            _assert_fps(got, ref, ref_cs, (kinds, row, bucketed))
            assert got[3] is None


@functools.lru_cache(maxsize=None)
def _many_small():
    """40 plots x 2500 points (the eight kinds five times over; all but the planted plot with new draws each time) and the oracle's
    625 samples."""
    kinds = bp.KINDS8 * 5
    xyz = torch.stack([bp.make_plot(k, 2500, seed=i // 8 if k == "planted" else i) for i, k in enumerate(kinds)]).contiguous()
    start = torch.tensor([(977 * b + 13) % 2500 for b in range(40)])
    idx = P.fps_batched(xyz.permute(0, 2, 1).contiguous(), 625, start)
    return kinds, xyz, start, idx, bp.gather_soa(xyz, idx)


def test_fps_many_small_plots():
    """40 x 2500 -> 625: more than 32 plots of at most 4096 points take the brute-force kernel with 256 threads per plot."""
    kinds, xyz, start, ref, ref_cs = _many_small()
    assert not ops.fps_fills_ws(40, 2500, 625) and ops.fps_fills_ws(32, 2500, 625)
    assert tuple(ops.fps_route(40, 2500, 625, device=DEV))[:4] == (ops.FPS_FORM_BRUTE, 4, 1, 16)         # fps_kernel<16, 256>
    got = ops.fps(xyz.to(DEV), 625, _dev(start, I32), return_ws=True)
    _assert_fps(got, ref, ref_cs, "40 x 2500")
    assert got[3] is None


def test_fps_two_bucket_slots_per_lane():
    """65 540 points: the smallest plot for which the single-workgroup kernel keeps two bucket slots per lane (more than 64 slots
    per wave: above 65 536 points).  The centimetre lattice and the flat plot, 64 samples."""
    n, m = 65540, 64
    xyz = torch.stack([bp.lattice_plot(n, 0.01, 11), bp.degenerate_plot("flat", n, 12)]).contiguous()
    assert ops.fps_fills_ws(2, n, m)
    start = torch.tensor([n - 1, 7])
    ref = P.fps_batched(xyz.permute(0, 2, 1).contiguous(), m, start)
    # 16: fps_spec_kernel<128, 16>, the two-slots-per-lane kernel; 0: eight workgroups of 8 waves (1025 buckets), whose repair launch it is
    routes = {16: (ops.FPS_FORM_SPEC, 16, 1, 128, 0, 0, 1), 0: (ops.FPS_FORM_CLUSTER, 8, 8, 32, 0, 128, 1)}
    for waves in (16, 0):
        assert tuple(ops.fps_route(2, n, m, waves=waves, device=DEV)) == routes[waves]
        got = ops.fps(xyz.to(DEV), m, _dev(start, I32), waves=waves, return_ws=True)
        _assert_fps(got, ref, bp.gather_soa(xyz, ref), waves)
        assert got[3] is not None and int(ops.fps_ws_ctl(got[3], 2, n)[1]) == 0


# ---------------------------------------------------------------------------------------------------- ball query
def _assert_ball(got, want, cap, what):
    nbr, cnt, total = got
    cnt_ref, col = want
    assert torch.equal(cnt.cpu().long(), cnt_ref), what
    assert int(total.item()) == int(cnt_ref.sum()), what
    mask = torch.arange(nbr.shape[1]).unsqueeze(0) < cnt.cpu().unsqueeze(1)
    assert torch.equal(nbr.cpu()[mask].long(), col), what          # row-major over (centroid, slot) == the oracle's order


@pytest.mark.parametrize("r", bp.RADII)
@pytest.mark.parametrize("which", ["five", "three"])
@pytest.mark.parametrize("n,m", bp.BALL_SIZES)
def test_ball_query_on_planted_shells_and_degenerate_plots(n, m, which, r):
    """Both levels, both caps, the full scan and -- where FPS leaves its workspace -- the grid route, against `P.radius`: the
    planted lattice plot holds at least 8 (centroid, point) pairs at exactly fp32(r*r) (out: the test is strict), one fp32 below
    (in) and one above (out) for every radius; flat, line and one-position plots have axes of zero extent, over which the grid
    route's cell range runs with a scale of 16 / 1e-6."""
    kinds = KINDS[which]
    xyz = bp.batch(kinds, n)
    B = xyz.shape[0]
    _, _, cs = _fps_ref(kinds, n, m, 2)
    _, _, cs2 = _fps2_ref(kinds, n, m, 2)
    dev, cs_dev = xyz.to(DEV), cs.to(DEV)
    ws = ops.fps(dev, m, None, return_ws=True)[3]
    assert (ws is not None) == ops.fps_fills_ws(B, n, m) == (n > 2048)
    for cap in (2000, 64):
        want = bp.oracle_ball_lists(xyz, cs, r, cap)
        _assert_ball(ops.ball_query(dev, cs_dev, r, cap), want, cap, (kinds, r, cap, "full scan"))
        if ws is not None:
            _assert_ball(ops.ball_query(dev, cs_dev, r, cap, fps_ws=ws), want, cap, (kinds, r, cap, "grid"))
        if cap == 64 and r >= 2.0:
            assert int(want[0].max()) == 64                       # the cap bites: the first 64 in ascending index
        want2 = bp.oracle_ball_lists(cs, cs2, r, cap)
        _assert_ball(ops.ball_query(cs_dev, cs2.to(DEV), r, cap), want2, cap, (kinds, r, cap, "level 2"))


@pytest.mark.parametrize("n,m", bp.BALL_SIZES)
def test_ball_query_around_the_anchors(n, m):
    """The anchors themselves as centroids: every planted pair is a tested pair (at least 32 per class and radius at level 1, 40 at
    level 2, counted by the host test).  Level 2 runs on a level-1 set made of the anchors and planted points."""
    plot, anchors, _ = bp.planted_plot(n)
    xyz = plot.unsqueeze(0).contiguous()
    cen = bp.gather_soa(xyz, anchors.unsqueeze(0))
    s1, a1 = bp.shell_level1_set(n, m)
    s1 = s1.unsqueeze(0).contiguous()
    cen2 = bp.gather_soa(s1, a1.unsqueeze(0))
    dev = xyz.to(DEV)
    ws = ops.fps(dev, 64, None, return_ws=True)[3]
    assert (ws is not None) == ops.fps_fills_ws(1, n, 64) == (n > 2048)
    for r in bp.RADII:
        for cap in (2000, 64):
            want = bp.oracle_ball_lists(xyz, cen, r, cap)
            _assert_ball(ops.ball_query(dev, cen.to(DEV), r, cap), want, cap, (r, cap, "full scan"))
            if ws is not None:
                _assert_ball(ops.ball_query(dev, cen.to(DEV), r, cap, fps_ws=ws), want, cap, (r, cap, "grid"))
            _assert_ball(ops.ball_query(s1.to(DEV), cen2.to(DEV), r, cap), bp.oracle_ball_lists(s1, cen2, r, cap), cap, (r, cap, "level 2"))


def test_ball_query_many_small_plots():
    kinds, xyz, _, _, cs = _many_small()
    for r, cap in ((1.0, 2000), (2.0 ** 0.5, 64)):
        _assert_ball(ops.ball_query(xyz.to(DEV), cs.to(DEV), r, cap), bp.oracle_ball_lists(xyz, cs, r, cap), cap, (r, cap))


# ---------------------------------------------------------------------------------------------------- 3-NN
def _assert_knn(got, want, k, what):
    idx, w = got[0].cpu().long(), got[1].cpu()
    ref_idx, ref_w = want
    kk = ref_idx.shape[1]
    assert torch.equal(idx[:, :kk], ref_idx), what
    assert torch.equal(w[:, :kk], ref_w), what                     # the same canonical d2, IEEE division
    if kk < 3:
        assert torch.all(w[:, kk:] == 0) and torch.equal(idx[:, kk:], idx[:, :1].expand(-1, 3 - kk)), what


def _three_routes(src, dst, k, want, what, grid_expected):
    """grid=False, the default grid (sn2_three_nn_xy) and the walk over the targets' FPS order, where the sizes take the grid."""
    B, _, S = src.shape
    T = dst.shape[2]
    s, d = src.to(DEV), dst.to(DEV)
    assert ops.three_nn_uses_grid(S, T) == grid_expected, what
    _assert_knn(ops.three_nn(s, d, k, grid=False), want, k, (what, "full scan"))
    _assert_knn(ops.three_nn(s, d, k), want, k, (what, "grid" if grid_expected else "default"))
    if grid_expected and ops.fps_fills_ws(B, T, 64):
        ws = ops.fps(d, 64, None, return_ws=True)[3]
        assert ws is not None
        _assert_knn(ops.three_nn(s, d, k, dst_fps_ws=ws), want, k, (what, "grid over the FPS order"))


@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("n,m", [(2304, 576), (2500, 625)])
def test_three_nn_on_planted_ties(n, m, k):
    """Targets at the same fp32 distance from two different sources at rank 1/2, 2/3 and 3/4 (the lowest source index wins), and
    targets on a source (d2 = 0, weight 1 / 1e-16): at least 16 planted of each, hundreds more from the lattice itself."""
    src, dst, _ = bp.tie_case(n, m)
    src, dst = src.unsqueeze(0).contiguous(), dst.unsqueeze(0).contiguous()
    _three_routes(src, dst, k, bp.oracle_knn(src, dst, k), (n, m, k), True)


@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("which", ["five", "three"])
def test_three_nn_on_mixed_batches(which, k):
    """Points <- level-1 samples (the grid routes) and level-1 samples <- level-2 samples (the full scan) of the mixed batches: the
    sources of the line plot have zero extent in y, those of the one- and two-position plots are 576 copies of one or two points
    (every target ties: the lowest index wins)."""
    kinds = KINDS[which]
    xyz = bp.batch(kinds, N1)
    _, _, cs = _fps_ref(kinds, N1, M1, 2)
    _, _, cs2 = _fps2_ref(kinds, N1, M1, 2)
    _three_routes(cs, xyz, k, bp.oracle_knn(cs, xyz, k), (kinds, k, "level 1"), True)
    _three_routes(cs2, cs, k, bp.oracle_knn(cs2, cs, k), (kinds, k, "level 2"), False)


@pytest.mark.parametrize("k", [3, 1])
def test_three_nn_many_small_plots(k):
    """40 x (625 -> 2500): the grid route with more than 32 plots sorts its targets with 256 threads per plot."""
    kinds, xyz, _, _, cs = _many_small()
    _three_routes(cs, xyz, k, bp.oracle_knn(cs, xyz, k), ("40 x 2500", k), True)


@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("S", [2, 1])
def test_three_nn_with_one_and_two_sources(S, k):
    dst = bp.batch(bp.KINDS3, N1)
    src = torch.stack([dst[b][:, [0, N1 - 1][:S]] for b in range(3)]).contiguous()
    src[1] = dst[1][:, :1].expand(3, S)                          # the two-position plot: both sources at one position
    _three_routes(src, dst, k, bp.oracle_knn(src, dst, k), (S, k), False)


# ---------------------------------------------------------------------------------------------------- pixel ids
def _quantised(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, 4, generator=g) * 8).floor() / 8         # many exact ties: the first point wins


def test_bounding_box_grid_at_its_edges():
    """129 consecutive fp32 values around each of the 19 steps of the oracle's id, in x, in y and in both: ids bit for bit; arg-max
    points, occupied pixels and plot-wise coverages as the oracle's scatter_max gives them."""
    from types import SimpleNamespace
    D = bp.D_PIX
    clouds = bp.pixel_edge_batch("p2")
    B, _, N = clouds.shape
    pw = _quantised(B * N, 5)
    ref = projection.p2_pixel_ids(clouds, D)
    cell = (ref[:, 0].long() * D + ref[:, 1].long())
    mm, pix = ops.plot_pixels(clouds.to(DEV), D)
    assert torch.equal(pix.cpu(), cell.reshape(-1).int())
    assert torch.equal(mm.cpu(), torch.stack([clouds[:, 0].min(1).values, clouds[:, 0].max(1).values, clouds[:, 1].min(1).values,
                                              clouds[:, 1].max(1).values], 1))
    pred, pix0, arg, nocc = ops.plot_project_forward(pw.to(DEV), clouds.to(DEV), D)
    assert torch.equal(pix0, pix)
    pred1, _, arg1, nocc1 = ops.plot_project_forward_pix(pw.to(DEV), pix, B, N, D)
    assert torch.equal(arg1, arg) and torch.equal(nocc1, nocc) and torch.equal(pred1, pred)
    gcell = (cell + (torch.arange(B) * D * D).unsqueeze(1)).reshape(-1)
    _, a = P.scatter_max(pw.t().contiguous(), gcell, dim=-1, dim_size=B * D * D)            # (4, B*D*D): FIRST point at the maximum
    local = torch.where(a == B * N, torch.full_like(a, -1), a - (torch.arange(B) * N).repeat_interleave(D * D).unsqueeze(0))
    assert torch.equal(arg.cpu().view(B * D * D, 3).long(), local[[0, 2, 3]].t())
    assert torch.equal(nocc.cpu().long(), (a[0] != B * N).view(B, D * D).sum(1))
    want = projection.project_to_plotwise_coverages(pw, clouds, SimpleNamespace(diam_pix=D))
    np.testing.assert_allclose(pred.cpu().numpy(), want.numpy(), atol=1e-6, rtol=0)


def test_fixed_grid_at_its_edges():
    from types import SimpleNamespace
    D = bp.D_PIX
    clouds = bp.pixel_edge_batch("p1")
    B, _, N = clouds.shape
    pw = _quantised(B * N, 6)
    rasters, pix = ops.raster_project(pw.to(DEV), clouds.to(DEV), D, bp.D_METERS)
    args = SimpleNamespace(diam_pix=D, diam_meters=bp.D_METERS)
    for b in range(B):
        p = projection.p1_pixel_ids(clouds[b], D, bp.D_METERS)
        assert torch.equal(pix.cpu().view(B, N)[b], (p[1] * D + p[0]).int()), b
        ref = projection.project_to_2d_rasters(clouds[b], pw.view(B, N, 4)[b].t(), args)
        got = rasters[b].double().cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        assert np.array_equal(np.nan_to_num(got), np.nan_to_num(ref))         # maxima of identical fp32 values: exact


def test_bounding_box_grid_on_zero_extent_axes():
    """The line (y constant) and one-position (x and y constant) plots next to ordinary ones: the reference's + 1e-4 makes a zero
    extent well defined -- every id 0 on that axis --, and a plot's box does not leak into its neighbours."""
    D = bp.D_PIX
    xyz = bp.batch(bp.KINDS5 + ("one",), N1)
    clouds = bp.cloud_from_xyz(xyz, 3)
    ref = projection.p2_pixel_ids(clouds, D)
    assert int(ref[3, 1].abs().max()) == 0 and int(ref[5].abs().max()) == 0 and int(ref[3, 0].max()) == D - 1
    mm, pix = ops.plot_pixels(clouds.to(DEV), D)
    assert torch.equal(pix.cpu(), (ref[:, 0] * D + ref[:, 1]).reshape(-1).int())
    pw = _quantised(6 * N1, 7)
    _, pix0, _, nocc = ops.plot_project_forward(pw.to(DEV), clouds.to(DEV), D)
    assert torch.equal(pix0, pix) and int(nocc[5]) == 1 and int(nocc[3]) == D


# ---------------------------------------------------------------------------------------------------- through the network
NET_KINDS = ("planted", "flat", "half", "two")


@functools.lru_cache(maxsize=None)
def _net_case():
    from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args
    xyz = bp.batch(NET_KINDS, N1)
    B = xyz.shape[0]
    g = torch.Generator().manual_seed(17)
    d = {"xyz": xyz, "cloud": bp.cloud_from_xyz(xyz, 5), "coverages": torch.rand(B, 4, generator=g, dtype=torch.float64),
         "pdf_all": 0.05 + 0.95 * torch.rand(B * N1, 3, generator=g, dtype=torch.float64)}
    fs = torch.stack([torch.full((B,), bp.BALL_START), torch.full((B,), bp.BALL_START2)])
    d["fps_start"] = fs
    args = make_args(subsample_size=N1, ratio1=0.25, r1=1.0, ratio2=0.25, r2=2.0)
    sd = network.init_state_dict(3)
    ref64 = check.train_step(sd, d, args, fps_start=fs)
    ref32 = check.train_step(sd, d, args, fps_start=fs, dtype=torch.float32)
    with torch.no_grad():
        cov_e, proba_e, _ = network.forward({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, d["cloud"].double(),
                                            xyz, args, training=False, fps_start=(fs[0], fs[1]))
    # the oracle's index structures
    _, idx1, cs = _fps_ref(NET_KINDS, N1, M1, 2)
    _, idx2, cs2 = _fps2_ref(NET_KINDS, N1, M1, 2)
    tabs = dict(idx1=idx1, idx2=idx2, ball1=bp.oracle_ball_lists(xyz, cs, args.r1, 2000), ball2=bp.oracle_ball_lists(cs, cs2, args.r2, 2000),
                knn1=bp.oracle_knn(cs, xyz, 3), knn2=bp.oracle_knn(cs2, cs, 3))
    return args, sd, d, fs, ref64, ref32, (cov_e, proba_e), tabs


def _assert_tables(saved, tabs):
    assert torch.equal(saved.idx1.cpu().long().view(tabs["idx1"].shape), tabs["idx1"])
    assert torch.equal(saved.idx2.cpu().long().view(tabs["idx2"].shape), tabs["idx2"])
    for lvl in ("1", "2"):
        nbr, cnt = getattr(saved, "nbr" + lvl).cpu(), getattr(saved, "cnt" + lvl).cpu()
        cnt_ref, col = tabs["ball" + lvl]
        assert torch.equal(cnt.long(), cnt_ref), lvl
        mask = torch.arange(nbr.shape[1]).unsqueeze(0) < cnt.unsqueeze(1)
        assert torch.equal(nbr[mask].long(), col), lvl
        idx, w = getattr(saved, "knn" + lvl)
        assert torch.equal(idx.cpu().long(), tabs["knn" + lvl][0]) and torch.equal(w.cpu(), tabs["knn" + lvl][1]), lvl


@pytest.mark.parametrize("executor", [False, True])
def test_training_step_and_eval_forward_on_boundary_plots(executor):
    """One batch of the planted lattice plot, a flat bare-soil plot, a half disc and a two-position plot at 2304 points: forward,
    loss and backward in training mode and an eval forward, through the per-call path and the executor, against the fp64 oracle
    with `check.compare`'s defaults (1e-4 on outputs, 1e-3 of a gradient tensor's magnitude); the saved index structures equal
    the oracle's exactly.  Where the checker's own fp32-vs-fp64 distance on a tensor exceeds half the tolerance, that tensor's
    bound is max(tolerance, 2 x that distance) (the rule of tests/test_gpu_bf16.py); both numbers are printed per tensor.  The
    bound comes from the oracle in two precisions, never from the kernels.
    Measured on MI355X (the same to three digits on both paths): the checker's own distance is 1.4e-3 / 1.5e-3 / 5.3e-5 / 8.7e-6
    on coverages / probabilities / plot-wise coverages / loss and 8e-4 ... 1.2e-1 on the gradient tensors (largest on SA1's
    first layer) -- a quarter of every BatchNorm's rows are copies of two rows here, on top of the rarely active ReLU channels
    of default weights (oracle/check.py) --, so every tensor but the plot-wise coverages and the loss takes the second form of
    the bound.  HIP against the fp64 oracle: 1.17e-4 / 1.29e-4 / 5.6e-6 / 1.6e-8, gradients 4.5e-5 ... 2.0e-2 (the largest,
    sa1 layer 2's bias, where the checker's own distance is 4.9e-2): between 1.9 and 560 times closer to fp64 than the checker's
    fp32 run on every tensor.  The eval forward (no batch statistics) is within 6e-8 / 7.5e-8 at the flat 1e-4."""
    from stratanet2_vegetation_coverage_maps_amd import PointNet2, losses, project_to_plotwise_coverages
    args, sd, d, fs, ref64, ref32, (cov_e, proba_e), tabs = _net_case()
    args.cuda = 0
    m = PointNet2(args)
    m.load_state_dict({k: v.clone() for k, v in sd.items()})
    m.executor = executor
    m.train()
    cov, proba = m(d)
    saved = cov.grad_fn.saved
    _assert_tables(saved, tabs)
    pred = project_to_plotwise_coverages(cov, d["cloud"], args, model=m)
    loss, _ = losses.total_loss(pred, proba, d["coverages"].cuda(), d["pdf_all"].cuda(), args.m, args.e)
    loss.backward()
    torch.cuda.synchronize()
    tol_out, tol_grad = 1e-4, 1e-3
    fails, lines = [], []

    def bound(tol, own):
        return max(tol, 2.0 * own) if own > 0.5 * tol else tol

    for name, got, k in (("coverages_pointwise", cov, "cov"), ("proba_pointwise", proba, "proba"), ("pred_coverages", pred, "pred")):
        own = float((ref32[k].double() - ref64[k].double()).abs().max())
        err = float((got.detach().cpu().double() - ref64[k].double()).abs().max())
        lines.append(f"{name:42s} max abs err {err:.2e}  bound {bound(tol_out, own):.2e}  (checker fp32 vs fp64: {own:.2e})")
        if not err <= bound(tol_out, own):
            fails.append(lines[-1])
    own, err = abs(ref32["loss"] - ref64["loss"]), abs(loss.item() - ref64["loss"])
    lines.append(f"{'loss':42s} abs err {err:.2e}  bound {bound(tol_out, own):.2e}  (checker fp32 vs fp64: {own:.2e})")
    if not err <= bound(tol_out, own):
        fails.append(lines[-1])
    for k, p in m.named_parameters():
        g = ref64["grads"][k].double().numpy()
        scale = np.abs(g).max()
        own = float(np.abs(ref32["grads"][k].double().numpy() - g).max() / scale)
        err = float(np.abs(p.grad.detach().cpu().double().numpy() - g).max() / scale)
        lines.append(f"{k:42s} grad err {err:.2e}  bound {bound(tol_grad, own):.2e}  (checker fp32 vs fp64: {own:.2e})")
        if not err <= bound(tol_grad, own):
            fails.append(lines[-1])
    print(f"\n[boundary plots, executor={executor}] vs the fp64 oracle:\n  " + "\n  ".join(lines))
    assert not fails, "\n".join(fails)
    # eval forward (running statistics as loaded)
    m2 = PointNet2(args)
    m2.load_state_dict({k: v.clone() for k, v in sd.items()})
    m2.executor = executor
    m2.eval()
    with torch.no_grad():
        cov2, proba2 = m2(d)
    e_cov, e_proba = float((cov2.cpu().double() - cov_e).abs().max()), float((proba2.cpu().double() - proba_e).abs().max())
    print(f"  eval forward: coverages {e_cov:.2e}, probabilities {e_proba:.2e}  (tol {tol_out:.0e})")
    assert e_cov <= tol_out and e_proba <= tol_out
