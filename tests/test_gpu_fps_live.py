"""sn2_fps_live on the device (include/strata_hip.h): farthest point sampling that is told which points of a plot are repeats.
Every kernel form against full FPS on repeated tails, over two levels, the workspace it leaves, the definition where the tail is
NOT made of copies, the repair launch, and the callers: the network's two geometry paths, the batch producers and the pipeline."""
import numpy as np
import pytest
import torch

from oracle import primitives as P
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops

from _fps_live_ref import fps_live_ref, repeated_tail_plots

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32

# every kernel form at N = 2304: (waves, bucketed) -> the (form, waves per workgroup, workgroups per plot) sn2_fps_route names for it.
# 2304 points = 36 buckets: two workgroups of 8 waves are the widest split with two buckets per wave, which is also what 0 (sn2_fps)
# picks; two workgroups of 16 waves (34) would need 64 buckets, so that request runs the single workgroup of 16 waves, as 16 does.
# 1 = one sample per round, 4 / 8 / 16 = the speculative kernel, bucketed=False = the brute-force kernel (1024 threads at this size)
FORM_ROUTES = {(0, True): (ops.FPS_FORM_CLUSTER, 8, 2), (1, True): (ops.FPS_FORM_ROUND, 16, 1), (4, True): (ops.FPS_FORM_SPEC, 4, 1),
               (8, True): (ops.FPS_FORM_SPEC, 8, 1), (16, True): (ops.FPS_FORM_SPEC, 16, 1), (34, True): (ops.FPS_FORM_SPEC, 16, 1),
               (66, True): (ops.FPS_FORM_CLUSTER, 8, 2), (0, False): (ops.FPS_FORM_BRUTE, 16, 1)}
FORMS = list(FORM_ROUTES)


def assert_form_route(B, N, m, waves, bucketed):
    """The kernel this call launches is the one the form list claims (B plots of N = 2304 points)."""
    assert tuple(ops.fps_route(B, N, m, waves=waves, bucketed=bucketed, device=DEV))[:3] == FORM_ROUTES[(waves, bucketed)], (waves, bucketed)

NS = (2304, 1, 37, 365, 700, 600)
STARTS = (5, 0, 2000, 1999, 3, 11)              # two in the tail (plots 2 and 3)
N1, M1, M2 = 2304, 600, 150


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))


def _dev_i32(v):
    return torch.as_tensor(v).to(DEV, I32)


@pytest.fixture(scope="module")
def tails():
    """The shared case: positions, starts, the oracle's full FPS and the count of its early-exit restatement."""
    pos, start = repeated_tail_plots(N1, NS, STARTS, dup_plots=(0, 5), seed=0)
    ref = P.fps_batched(pos, M1, start)
    _, count = fps_live_ref(pos, M1, start)
    return pos, pos.permute(0, 2, 1).contiguous().to(DEV), start, ref, count


@pytest.mark.parametrize("waves,bucketed", FORMS)
def test_equals_full_fps_on_repeated_tails(tails, waves, bucketed):
    pos, xyz, start, ref, count = tails
    B = len(NS)
    st, nl = _dev_i32(start), _dev_i32(NS)
    out = torch.full((B,), -1, dtype=I32, device=DEV)
    assert_form_route(B, N1, M1, waves, bucketed)
    full = ops.fps(xyz, M1, st, bucketed=bucketed, waves=waves)
    live = ops.fps(xyz, M1, st, bucketed=bucketed, waves=waves, n_live=nl, n_live_out=out)
    assert torch.equal(full[0].cpu().long(), ref)
    assert _same(live, full)
    assert count.tolist() == [600, 1, 37, 365, 600, 598]
    assert out.cpu().tolist() == count.tolist()
    # n_live = NULL with a count asked for: the same samples and the same count (every form ends at a maximum of 0)
    out2 = torch.full((B,), -1, dtype=I32, device=DEV)
    assert _same(ops.fps(xyz, M1, st, bucketed=bucketed, waves=waves, n_live_out=out2), full) and torch.equal(out2, out)
    # clamped on the device: 0 and negative -> 1, beyond N -> N
    wild = _dev_i32([N1 + 7, 0, 37, 365, 1 << 30, 600])
    assert _same(ops.fps(xyz, M1, st, bucketed=bucketed, waves=waves, n_live=wild), full)


def test_two_levels(tails):
    pos, xyz, start, ref, count = tails
    B = len(NS)
    k = torch.empty(B, dtype=I32, device=DEV)
    _, cs, _ = ops.fps(xyz, M1, _dev_i32(start), n_live=_dev_i32(NS), n_live_out=k)
    st2 = _dev_i32([(7 * b + 3) % M1 for b in range(B)])
    st2[1] = M1 - 1                                   # a start in level 2's tail (plot 1: one live sample)
    for waves, bucketed in ((0, True), (0, False)):
        k2 = torch.empty(B, dtype=I32, device=DEV)
        assert _same(ops.fps(cs, M2, st2, waves=waves, bucketed=bucketed, n_live=k, n_live_out=k2),
                     ops.fps(cs, M2, st2, waves=waves, bucketed=bucketed))
    assert k2.cpu().tolist() == [150, 1, 37, 150, 150, 150]


def test_two_levels_at_the_parcel_loop_sizes():
    """10 000 -> 2500 -> 625 with four waves per plot: level 2 (2500 points) is on the bucketed path."""
    N, Ma, Mb, ns = 10000, 2500, 625, (367, 2600, 9000, 10000)
    pos, start = repeated_tail_plots(N, ns, (366, 9999, 17, 5), dup_plots=(1,), seed=3)
    xyz, st = pos.permute(0, 2, 1).contiguous().to(DEV), _dev_i32(start)
    assert ops.fps_fills_ws(4, Ma, Mb)
    k = torch.empty(4, dtype=I32, device=DEV)
    full1 = ops.fps(xyz, Ma, st, waves=4)
    live1 = ops.fps(xyz, Ma, st, waves=4, n_live=_dev_i32(ns), n_live_out=k)
    assert _same(live1, full1)
    assert k.cpu().tolist() == [367, 2500, 2500, 2500]
    st2 = _dev_i32([3, 2499, 1000, 7])
    for waves in (4, 0):
        assert _same(ops.fps(live1[1], Mb, st2, waves=waves, n_live=k), ops.fps(full1[1], Mb, st2, waves=waves)), waves


def test_workspace_still_covers_all_points(tails):
    """Repeated points are real neighbours: the ball query and the grid 3-NN that walk the workspace of a live call give the bytes
    of their forms without one."""
    pos, xyz, start, ref, count = tails
    B = len(NS)
    for waves in (0, 8):
        idx, cs, ca, ws = ops.fps(xyz, M1, _dev_i32(start), waves=waves, n_live=_dev_i32(NS), return_ws=True)
        assert ws is not None
        order = ws[:B * N1].view(B, N1).long()
        assert torch.equal(order.sort(1).values, torch.arange(N1, device=DEV).expand(B, N1))
        assert torch.equal(torch.gather(ops.fps_ws_rank(ws, B, N1).view(B, N1).long(), 1, order), torch.arange(N1, device=DEV).expand(B, N1))
        nbr_g, cnt_g, _ = ops.ball_query(xyz, cs, 0.4, 128, fps_ws=ws)
        nbr_f, cnt_f, _ = ops.ball_query(xyz, cs, 0.4, 128)
        mask = torch.arange(128, device=DEV)[None, :] < cnt_f[:, None]
        assert torch.equal(cnt_g, cnt_f) and torch.equal(nbr_g[mask], nbr_f[mask])
        assert int(cnt_f.view(B, M1)[1].min()) == 128          # the one-point plot: every repeat is a neighbour
        a_i, a_w = ops.three_nn(cs, xyz, 3, dst_fps_ws=ws)
        b_i, b_w = ops.three_nn(cs, xyz, 3, grid=False)
        assert torch.equal(a_i, b_i) and torch.equal(a_w, b_w)


def test_definition_when_the_tail_is_not_copies():
    """Distinct random points, n_live = 500 < N: every form samples points [0, 500) only, as fps_batched over that prefix does
    (the start inside it), and writes index 0 after the 500th sample."""
    B, n = 3, 500
    g = torch.Generator().manual_seed(11)
    pos = torch.rand(B, N1, 3, generator=g) * torch.tensor([2.0, 2.0, 0.5])
    start = torch.tensor([0, 499, 250])
    ref = P.fps_batched(pos[:, :n].contiguous(), n, start)
    ref = torch.cat([ref, torch.zeros(B, M1 - n, dtype=torch.long)], 1)
    xyz = pos.permute(0, 2, 1).contiguous().to(DEV)
    first = None
    for waves, bucketed in FORMS:
        assert_form_route(B, N1, M1, waves, bucketed)
        out = torch.empty(B, dtype=I32, device=DEV)
        got = ops.fps(xyz, M1, _dev_i32(start), bucketed=bucketed, waves=waves, n_live=_dev_i32([n] * B), n_live_out=out)
        assert torch.equal(got[0].cpu().long(), ref), (waves, bucketed)
        assert int(got[0].max()) < n and out.cpu().tolist() == [n] * B
        first = got if first is None else first
        assert _same(got, first), (waves, bucketed)
    assert torch.equal(first[1].cpu(), torch.gather(pos, 1, ref.unsqueeze(2).expand(-1, -1, 3)).permute(0, 2, 1))


def _lattice_plots(n, angles):
    """Short plots as the training feed makes them: 51 random points and the 316 ground points of the 1 m lattice, rotated by whole
    degrees (fp64 product cast back, as load_cloud's augmentation), then repeats up to n.  The lattice gives hundreds of DISTINCT
    points at nearly -- not exactly -- equal distances from one another."""
    from stratanet2_vegetation_coverage_maps_amd.input_pipeline import fake_ground_xy
    g = torch.Generator().manual_seed(4)
    fake = torch.from_numpy(fake_ground_xy(20)).double()
    plots = []
    for a in angles:
        c, s_ = np.cos(np.radians(a)), np.sin(np.radians(a))
        top = torch.rand(51, 3, generator=g, dtype=torch.float64) * torch.tensor([14.0, 14.0, 20.0], dtype=torch.float64) - torch.tensor([7.0, 7.0, 0.0], dtype=torch.float64)
        xy = torch.cat([top[:, :2], fake], 0)
        p = torch.stack([xy[:, 0] * c + xy[:, 1] * s_, -xy[:, 0] * s_ + xy[:, 1] * c, torch.cat([top[:, 2], torch.zeros(len(fake), dtype=torch.float64)])], 1).float()
        plots.append(torch.cat([p, p[torch.randint(0, len(p), (n - len(p),), generator=g)]], 0))
    return torch.stack(plots)


def test_nearly_equal_maxima_of_distinct_points():
    """Every form against the oracle where the largest running distances of DISTINCT points lie within a few ulp of each other:
    the multi-workgroup kernel publishes a workgroup's top buckets by 64-ulp keys, so its exact-tie search must run at the true
    maximum, which may be a value inside the top key's class that was left out of the published records."""
    n, m = 4096, 512
    pos = _lattice_plots(n, (17, 90, 200, 297))
    start = torch.tensor([400, 2460, 13, 366])
    ref = P.fps_batched(pos, m, start)
    xyz, st, nl = pos.permute(0, 2, 1).contiguous().to(DEV), _dev_i32(start), _dev_i32([367] * 4)
    # 4096 points = 64 buckets: four workgroups of 8 waves fit (68, and what 0 picks), two do (66); four of 16 waves (36) would need
    # 128 buckets and run the single workgroup of 16 waves
    C, S, R, F = ops.FPS_FORM_CLUSTER, ops.FPS_FORM_SPEC, ops.FPS_FORM_ROUND, ops.FPS_FORM_BRUTE
    routes = {(0, True): (C, 8, 4), (68, True): (C, 8, 4), (66, True): (C, 8, 2), (36, True): (S, 16, 1), (8, True): (S, 8, 1),
              (1, True): (R, 16, 1), (0, False): (F, 16, 1)}
    for (waves, bucketed), route in routes.items():
        assert tuple(ops.fps_route(4, n, m, waves=waves, bucketed=bucketed, device=DEV))[:3] == route, (waves, bucketed)
        assert torch.equal(ops.fps(xyz, m, st, waves=waves, bucketed=bucketed)[0].cpu().long(), ref), (waves, bucketed)
        assert torch.equal(ops.fps(xyz, m, st, waves=waves, bucketed=bucketed, n_live=nl)[0].cpu().long(), ref), (waves, bucketed, "live")


def test_repair_launch_honours_the_live_prefix():
    """The multi-workgroup pass made to give up (a wait limit of one sweep, as in tests/test_gpu_geometry.py) and repaired by the
    single-workgroup kernel: with n_live it equals the undisturbed result, count included."""
    from stratanet2_vegetation_coverage_maps_amd import _lib
    B, N, M, ns = 4, 32768, 512, (32768, 400, 20000, 511)
    pos, start = repeated_tail_plots(N, ns, (13, 30000, 990, 3), dup_plots=(2,), seed=5)
    xyz, st, nl = pos.permute(0, 2, 1).contiguous().to(DEV), _dev_i32(start), _dev_i32(ns)
    k0 = torch.empty(B, dtype=I32, device=DEV)
    assert tuple(ops.fps_route(B, N, M, waves=72, device=DEV))[:3] == (ops.FPS_FORM_CLUSTER, 8, 8)
    assert tuple(ops.fps_route(B, N, M, waves=16, device=DEV))[:3] == (ops.FPS_FORM_SPEC, 16, 1)
    want = ops.fps(xyz, M, st, waves=16)
    calm = ops.fps(xyz, M, st, waves=72, n_live=nl, n_live_out=k0, return_ws=True)
    assert _same(calm, want) and int(ops.fps_ws_ctl(calm[3], B, N)[1]) == 0
    assert k0.cpu().tolist() == [512, 400, 512, 511]
    before = ops.fps_gave_up(DEV, warn=False)
    lib = _lib.load()
    try:
        assert lib.sn2_debug_fps_spin_limit(1) == 0
        out = (torch.full((B, M), -7, dtype=I32, device=DEV), torch.full((B, 3, M), float("nan"), device=DEV),
               torch.full((B * M, 4), float("nan"), device=DEV), torch.empty(ops.fps_ws_words(B, N), dtype=I32, device=DEV))
        k = torch.full((B,), -1, dtype=I32, device=DEV)
        got = ops.fps(xyz, M, st, out=out, waves=72, n_live=nl, n_live_out=k, return_ws=True)
        torch.cuda.synchronize()
        assert int(ops.fps_ws_ctl(got[3], B, N)[1]) > 0, "the one-sweep limit did not make a wait give up"
        assert _same(got, want) and torch.equal(k, k0)
    finally:
        lib.sn2_debug_fps_spin_limit(0)
    assert ops.fps_gave_up(DEV, warn=False) > before


# ---------------------------------------------------------------------------------------------------- the network's geometry paths
def _short_plot_batch():
    """input_pipeline.prepare_batch on plots of 51, 400, 3000 and N + 200 raw points at N = 4096 (+ 316 fake ground points each)."""
    from stratanet2_vegetation_coverage_maps_amd.input_pipeline import prepare_batch
    from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_raw_plot
    n = 4096
    args = make_args(cuda=0, subsample_size=n, ratio1=0.125, r1=1.0, ratio2=0.25, r2=2.0)
    sizes = (51, 400, 3000, n + 200)
    centers = np.array([[100.0 + 25 * p, 300.0 - 25 * p] for p in range(len(sizes))], dtype=np.float32)
    raw = [make_raw_plot(m, 700 + p, centers[p]) for p, m in enumerate(sizes)]
    batch = prepare_batch(raw, centers, args, train=False, rs=np.random.RandomState(3), device=DEV)
    assert batch["n_live"].cpu().tolist() == [367, 716, 3316, n]
    off = prepare_batch(raw, centers, args, train=False, rs=np.random.RandomState(3), device=DEV, n_live=False)
    assert "n_live" not in off and torch.equal(off["xyz"], batch["xyz"]) and torch.equal(off["cloud"], batch["cloud"])
    batch["fps_start"] = torch.tensor([[5, 4000, 17, 9], [0, 511, 3, 100]], dtype=I32, device=DEV)      # plot 1: both starts in the tails
    return args, batch


def _model(args, executor):
    from oracle import network
    from stratanet2_vegetation_coverage_maps_amd import PointNet2
    m = PointNet2(args)
    m.load_state_dict(network.init_state_dict(5))
    m = m.cuda()
    m.executor = executor
    return m


def _tables(g):
    out = {k: getattr(g, k).clone() for k in ("idx1", "idx2", "cnt1", "cnt2")}
    for k, c in (("nbr1", "cnt1"), ("nbr2", "cnt2")):                 # the first cnt entries of a list are defined
        nbr = getattr(g, k)
        out[k] = nbr.masked_fill(torch.arange(nbr.shape[1], device=nbr.device)[None, :] >= getattr(g, c)[:, None].long(), -1)
    for k in ("knn1", "knn2", "knn3"):
        out[k + "_idx"], out[k + "_w"] = (t.clone() for t in getattr(g, k))
    return out


@pytest.mark.parametrize("executor", [True, False])
def test_network_forward_with_n_live_equals_the_forward_without(executor):
    from stratanet2_vegetation_coverage_maps_amd import losses
    from stratanet2_vegetation_coverage_maps_amd.project_to_2d import project_to_plotwise_coverages
    args, batch = _short_plot_batch()
    plain = {k: v for k, v in batch.items() if k != "n_live"}
    model = _model(args, executor).eval()
    res = {}
    with torch.no_grad():
        for name, cd in (("live", batch), ("plain", plain)):
            geo = model.prefetch_geometry(cd)
            cov, proba = model(dict(cd, geometry=geo))
            torch.cuda.synchronize()
            res[name] = (cov.clone(), proba.clone(), _tables(geo))
            cov2, proba2 = model(dict(cd))                            # the forward that runs its own geometry pass
            assert torch.equal(cov2, cov) and torch.equal(proba2, proba), name
    assert torch.equal(res["live"][0], res["plain"][0]) and torch.equal(res["live"][1], res["plain"][1])
    for k, v in res["plain"][2].items():
        assert torch.equal(res["live"][2][k], v), k
    assert int(res["plain"][2]["idx1"][0].max()) < 367                # the 51-point plot: its samples are prefix points
    # a training step's loss
    model.train()
    B, n = batch["cloud"].shape[0], batch["cloud"].shape[2]
    g = torch.Generator().manual_seed(2)
    gt = torch.rand(B, 4, generator=g, dtype=torch.float64).to(DEV)
    pdf = (0.1 + torch.rand(B * n, 3, generator=g, dtype=torch.float64)).to(DEV)
    keep = (torch.rand(B * n, 16, generator=g) > args.drop).to(DEV)
    loss = {}
    for name, cd in (("live", batch), ("plain", plain)):
        model.zero_grad()
        cov, proba = model(dict(cd, dropout_mask=keep))
        pred = project_to_plotwise_coverages(cov, cd["cloud"], args)
        l, _ = losses.total_loss(pred, proba, gt, pdf, args.m, args.e)
        l.backward()
        loss[name] = float(l.detach())
    assert np.isfinite(loss["live"]) and loss["live"] == loss["plain"]


# ---------------------------------------------------------------------------------------------------- the producers
def test_parcel_batches_deliver_n_live():
    from stratanet2_vegetation_coverage_maps_amd import parcel
    from stratanet2_vegetation_coverage_maps_amd.input_pipeline import fake_ground_xy
    from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_parcel
    args = make_args(cuda=0, subsample_size=2048)
    plots = parcel.prepare_parcel(make_parcel(seed=11), args)
    want = np.minimum(plots.n_points + len(fake_ground_xy(args.diam_meters)), args.subsample_size)
    assert (want < args.subsample_size).any() and (want == args.subsample_size).any()
    for kw in ({"sampler": "numpy", "rs": np.random.RandomState(1)}, {"sampler": "device", "seed": 9}):
        got = [d["n_live"] for d in plots.batches(args, 8, **kw)]
        assert all(t.dtype == I32 and t.is_cuda for t in got)
        assert np.array_equal(torch.cat(got).cpu().numpy(), want), kw["sampler"]
        assert all("n_live" not in d for d in plots.batches(args, 8, n_live=False, **kw))
        # what the key promises of the rows: the first n_live points are followed by bit-identical copies of them
        d = next(iter(plots.batches(args, 8, **kw)))
        xyz, nl = d["xyz"].cpu(), d["n_live"].cpu()
        for b in range(xyz.shape[0]):
            head = {tuple(p) for p in xyz[b, :, :nl[b]].T.tolist()}
            assert all(tuple(p) in head for p in xyz[b, :, nl[b]:].T.tolist()), (kw["sampler"], b)


def test_train_batch_live_writes_n_live_and_the_bytes_of_train_batch():
    from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args
    from stratanet2_vegetation_coverage_maps_amd.train_data import ResidentPlots
    from test_gpu_train_feed import SIZES, _out, _raw_set
    n, ids = 512, [4, 0, 2, 3, 1]
    args = make_args(cuda=0, subsample_size=n, ratio1=0.125)
    raw, centers, cov = _raw_set(SIZES)
    plots = ResidentPlots.from_plots(raw, centers, cov, DEV)
    a = plots.fill(ids, 3, 1234, args, _out(len(ids), n))
    b = _out(len(ids), n)
    b["n_live"] = torch.full((len(ids),), -1, dtype=I32, device=DEV)
    plots.fill(ids, 3, 1234, args, b)
    torch.cuda.synchronize()
    assert b["n_live"].cpu().tolist() == [min(SIZES[p] + 316, n) for p in ids] == [512, 376, 512, 512, 512]
    for k in ("cloud", "xyz", "gt", "fps_start"):
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k


# ---------------------------------------------------------------------------------------------------- the pipeline
@pytest.mark.parametrize("pair", [False, True])
def test_pipeline_with_n_live_slots_matches_plain_loop(pair):
    """tests/test_gpu_train_feed.py::test_pipeline_with_epoch_feeder_matches_plain_loop on a set with short plots, the pipelined
    loop's slots carrying "n_live" (written by the feeder, read by the geometry passes), the plain loop's not.  (The short plots'
    rotated ground lattice also needs what `test_nearly_equal_maxima_of_distinct_points` checks of the plain loop's FPS kernel.)"""
    from test_gpu_pipeline import _setup
    from test_gpu_train_feed import _out
    from stratanet2_vegetation_coverage_maps_amd import losses
    from stratanet2_vegetation_coverage_maps_amd.pipeline import TrainPipeline
    from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_raw_plot
    from stratanet2_vegetation_coverage_maps_amd.train_data import EpochFeeder, ResidentPlots
    from oracle import network
    n, B, depth, P = 4096, 2, 2, 7
    n_slots = 2 * depth + 2 if pair else depth + 1
    steps = 2 * n_slots + 3
    args = make_args(cuda=0, subsample_size=n, ratio1=0.125, r1=1.0, ratio2=0.25, r2=2.0)
    sizes = (51, 400, 3000, 5000, n - 316, 2500, 3900)
    centers = np.array([[100.0 + 25 * p, 300.0 - 25 * p] for p in range(P)], dtype=np.float32)
    raw = [make_raw_plot(m, 900 + p, centers[p]) for p, m in enumerate(sizes)]
    cov = np.random.RandomState(4).rand(P, 4)
    plots = ResidentPlots.from_plots(raw, centers, cov, DEV)
    tables = losses.KdeTables(np.linspace(-1.0, 30.0, 64), *[np.linspace(0.1, 1.0, 64) ** k for k in (1, 2, 3)], DEV)
    seed = 77

    model, opt, slots, fstep = _setup(n, B, depth, n_slots, lr=0.0)
    order = EpochFeeder(plots, args, B, seed, generator=torch.Generator().manual_seed(11))
    assert order.steps_per_epoch == 3
    ref = []
    for i in range(steps):
        inp = plots.fill(order.batch_ids(i).tolist(), order.locate(i)[0], seed, args, _out(B, n, pdf=True), kde=tables)
        assert "n_live" not in inp
        l = fstep(inp)
        opt.step()
        ref.append(float(l.detach()))

    model2, opt2, slots2, fstep2 = _setup(n, B, depth, n_slots, lr=0.0)
    for sl in slots2:
        sl["n_live"] = torch.full((B,), n, dtype=I32, device=DEV)
    pipe = TrainPipeline(model2, opt2, fstep2, slots2, depth=depth, use_graph=True)
    assert pipe.pair == pair and pipe.has_live
    pipe.capture()
    for sl in slots2:                                   # wipe the resident copies: the feeder must bring the data
        for k in ("cloud", "xyz", "gt", "pdf", "fps_start", "n_live"):
            sl[k].zero_()
    model2.load_state_dict(network.init_state_dict(5))
    opt2.reset()
    pipe.issued = pipe.done = 0
    pipe.set_feeder(EpochFeeder(plots, args, B, seed, kde=tables, generator=torch.Generator().manual_seed(11)))
    issue = pipe.issue_geometry

    def delayed(i=None):
        for st in pipe.side:
            with torch.cuda.stream(st):
                torch.cuda._sleep(2_000_000)            # ~1 ms in front of whatever that side stream does next
        return issue(i)
    pipe.issue_geometry = delayed
    pipe.prime()
    out = torch.zeros(steps, dtype=torch.float64, device="cuda")
    for i in range(steps):                              # no host synchronisation inside the loop
        out[i] = pipe.step().detach()
    pipe.drain()
    torch.cuda.synchronize()
    got = out.cpu().tolist()
    assert all(np.isfinite(got)), got
    assert len(set(np.round(ref, 6))) > steps // 2      # the batches differ: equal losses are no accident
    assert sorted({int(v) for sl in slots2 for v in sl["n_live"].cpu()} - {n}) != []          # the feeder wrote short plots' counts
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-6)
    assert int(opt2.step_dev.item()) == steps
