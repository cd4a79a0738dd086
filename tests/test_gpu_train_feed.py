"""sn2_train_batch (csrc/feed.hip) through train_data.ResidentPlots.fill and train_data.EpochFeeder: a training batch written from a
device-resident plot set, every draw made on the device.  Held to `hip_ops.prepare_plots` fed the restated draws (that path is held
to the reference's load_cloud golden), to the numpy restatement of tests/test_train_feed_host.py for the noise, and inside a
TrainPipeline to the plain loop over standalone `fill` calls.

Shapes: N = 512 with 316 fake ground points and plots of 60, 196 (n == N exactly), 700, 1500 and 300 raw points reach both
subsample branches and the boundary between them; 17 000 points reach the subsample's GLOBAL form."""
import numpy as np
import pytest
import torch

from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
from stratanet2_vegetation_coverage_maps_amd import losses
from stratanet2_vegetation_coverage_maps_amd.input_pipeline import fake_ground_xy
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_raw_plot
from stratanet2_vegetation_coverage_maps_amd.train_data import EpochFeeder, ResidentPlots, cos_sin_table
from test_train_feed_host import fps_starts, plot_key, plot_params, restate_batch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, SEED, EPOCH = 512, 0xA5A5_0123_4567_89AB, 3
SIZES = (60, 196, 700, 1500, 300)
ID_LISTS = ([4, 0, 2], [3, 1, 4])


def _raw_set(sizes, seed=0):
    """Raw plots with distinct values in every channel (equal clouds then mean equal subsample rows), absolute coordinates."""
    rng = np.random.RandomState(seed)
    plots, centers = [], []
    for n in sizes:
        c = np.array([1000.5 + 40 * len(plots), 2000.25 - 30 * len(plots)], dtype=np.float32)
        r, a = 10 * np.sqrt(rng.rand(n)), 2 * np.pi * rng.rand(n)
        p = np.stack([c[0] + r * np.cos(a), c[1] + r * np.sin(a), 20 * rng.rand(n)] + [np.floor(65536 * rng.rand(n)) for _ in range(4)]
                     + [np.floor(32768 * rng.rand(n)), 1.0 + rng.randint(0, 4, n), 1.0 + rng.randint(0, 4, n)]).astype(np.float32)
        plots.append(p)
        centers.append(c)
    cov = rng.rand(len(sizes), 4)
    return plots, np.stack(centers), cov


@pytest.fixture(scope="module")
def small():
    args = make_args(cuda=0, subsample_size=N, ratio1=0.125)
    plots, centers, cov = _raw_set(SIZES)
    return {"args": args, "plots": plots, "centers": centers, "cov": cov, "fake": fake_ground_xy(args.diam_meters),
            "set": ResidentPlots.from_plots(plots, centers, cov, DEV), "M1": ops.fps_num_samples(N, args.ratio1)}


def _out(B, n=N, pdf=False):
    o = {"cloud": torch.full((B, 10, n), float("nan"), device=DEV), "xyz": torch.full((B, 3, n), float("nan"), device=DEV),
         "gt": torch.full((B, 4), float("nan"), dtype=torch.float64, device=DEV),
         "fps_start": torch.full((2, B), -1, dtype=torch.int32, device=DEV)}
    if pdf:
        o["pdf"] = torch.full((B * n, 3), float("nan"), dtype=torch.float64, device=DEV)
    return o


def _fill(s, ids, epoch=EPOCH, seed=SEED, **kw):
    out = s["set"].fill(ids, epoch, seed, s["args"], _out(len(ids), s["args"].subsample_size, "kde" in kw), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _packed(plots, centers, ids):
    """The plots `ids` side by side, as hip_ops.prepare_plots / hip_ops.subsample take them."""
    raw = torch.from_numpy(np.concatenate([plots[p] for p in ids], 1)).to(DEV)
    offs = torch.tensor(np.concatenate([[0], np.cumsum([plots[p].shape[1] for p in ids])]), dtype=torch.int32, device=DEV)
    return raw, offs, torch.from_numpy(np.ascontiguousarray(centers[ids])).to(DEV)


def _by_prepare_plots(s, ids, train, n=N, epoch=EPOCH, seed=SEED):
    P = len(s["plots"])
    keys = [plot_key(epoch, P, p) for p in ids]
    raw, offs, cen = _packed(s["plots"], s["centers"], ids)
    idx = ops.subsample(offs, len(s["fake"]), n, seed, torch.tensor(keys, dtype=torch.int64, device=DEV))
    rot = flips = None
    if train:
        par = [plot_params(seed, k) for k in keys]
        rot = torch.from_numpy(np.stack([cos_sin_table()[a] for _, _, a in par])).to(DEV)
        flips = torch.tensor([[fx, fy] for fx, fy, _ in par], dtype=torch.int32, device=DEV)
    cloud, xyz = ops.prepare_plots(raw, offs, cen, torch.from_numpy(s["fake"]).to(DEV), idx, s["args"].z_max, rot, flips)
    torch.cuda.synchronize()
    return cloud.cpu().numpy(), xyz.cpu().numpy()


@pytest.mark.parametrize("ids", ID_LISTS)
@pytest.mark.parametrize("train", [True, False])
def test_without_noise_equals_prepare_plots_fed_the_restated_draws(small, ids, train):
    got = _fill(small, ids, train=train, noise=False)
    cloud, xyz = _by_prepare_plots(small, ids, train)
    assert np.array_equal(got["cloud"].view(np.uint32), cloud.view(np.uint32))
    assert np.array_equal(got["xyz"].view(np.uint32), xyz.view(np.uint32))
    assert np.array_equal(got["gt"], small["cov"][ids])
    P = len(SIZES)
    assert got["fps_start"].T.tolist() == [list(fps_starts(SEED, plot_key(EPOCH, P, p), N, small["M1"])) for p in ids]
    if train:                                                                     # the draws did something
        eval_cloud, _ = _by_prepare_plots(small, ids, False)
        assert not np.array_equal(cloud[:, :2], eval_cloud[:, :2]) and np.array_equal(cloud[:, 2:], eval_cloud[:, 2:])


def test_with_noise_equals_the_numpy_restatement(small):
    """Every element equals the restatement or its fp32 neighbour, and at most 1 in 10^4 differs at all: the device's fp64 log /
    cos / sin may differ from numpy's in the last bit, and an error of 2 ulp in fp64 moves an fp32 rounding with probability about
    2^-27 per element -- about 1e-3 expected differences here, against the roughly 100 % a wrong word order or counter gives."""
    differ = total = 0
    for ids in ID_LISTS:
        got = _fill(small, ids)
        cloud, xyz, fs = restate_batch(small["plots"], small["centers"], small["fake"], ids, EPOCH, SEED, N, small["M1"],
                                       small["args"].z_max, cos_sin_table())
        assert np.array_equal(got["fps_start"], fs)
        for g, w in ((got["cloud"], cloud), (got["xyz"], xyz)):
            near = (g == w) | (g == np.nextafter(w, np.float32(np.inf))) | (g == np.nextafter(w, np.float32(-np.inf)))
            assert near.all(), f"{int((~near).sum())} elements are further than one fp32 step from the restatement"
            differ += int((g != w).sum())
            total += g.size
        quiet = _fill(small, ids, noise=False)["cloud"]
        assert not np.array_equal(got["cloud"][:, 0], quiet[:, 0]) and not np.array_equal(got["cloud"][:, 3:7], quiet[:, 3:7])
        assert np.array_equal(got["cloud"][:, [2, 7, 8, 9]], quiet[:, [2, 7, 8, 9]])
    print(f"noise=True against the numpy restatement: {differ} of {total} elements differ (by one fp32 step)")
    assert differ * 10 ** 4 <= total, (differ, total)


def test_rows_depend_on_seed_epoch_and_plot_alone(small):
    tables = losses.KdeTables(np.linspace(-1.0, 30.0, 64), *[np.linspace(0.1, 1.0, 64) ** k for k in (1, 2, 3)], DEV)
    a, b = _fill(small, ID_LISTS[0], kde=tables), _fill(small, ID_LISTS[1], kde=tables)
    one, again = _fill(small, [4]), _fill(small, ID_LISTS[0], kde=tables)
    for k in ("cloud", "xyz", "gt"):
        assert np.array_equal(a[k][0], b[k][2]) and np.array_equal(a[k][0], one[k][0]), k         # plot 4: first of three, last of three, alone
        assert np.array_equal(a[k], again[k]), k                                                   # and in two calls
    assert np.array_equal(a["fps_start"][:, 0], b["fps_start"][:, 2]) and np.array_equal(a["fps_start"][:, 0], one["fps_start"][:, 0])
    for other in (_fill(small, [4], epoch=EPOCH + 1), _fill(small, [4], seed=SEED + 1)):
        assert not np.array_equal(other["cloud"][0, :2], one["cloud"][0, :2]) and not np.array_equal(other["cloud"][0, 3], one["cloud"][0, 3])
        assert np.array_equal(other["gt"], one["gt"])
    cloud = torch.from_numpy(a["cloud"]).to(DEV)
    want = losses.kde_densities(cloud, small["args"].z_max, tables)
    torch.cuda.synchronize()
    assert np.array_equal(a["pdf"].view(np.uint64), want.cpu().numpy().view(np.uint64)) and np.isfinite(a["pdf"]).all()
    with pytest.raises(ValueError):
        small["set"].fill([0, 5], 0, 1, small["args"], _out(2))                                    # an id outside the set: refused on the host


def test_global_subsample_form_with_an_id_table():
    """One plot beyond what the LDS form holds beside two small ones, ids not ascending: the four-launch form reads plot b's range
    through the id table.  Bytes of hip_ops.subsample + hip_ops.prepare_plots on the same plots packed side by side."""
    n = 256
    plots, centers, cov = _raw_set((17000, 100, 50), seed=1)
    s = {"args": make_args(cuda=0, subsample_size=n, ratio1=0.125), "plots": plots, "centers": centers, "cov": cov,
         "fake": fake_ground_xy(20), "set": ResidentPlots.from_plots(plots, centers, cov, DEV)}
    assert ops.subsample_form(17000 + 316, n) == ops.SUBSAMPLE_GLOBAL
    ids = [2, 0, 1]
    for train in (False, True):
        got = _fill(s, ids, train=train, noise=False)
        cloud, xyz = _by_prepare_plots(s, ids, train, n=n)
        assert np.array_equal(got["cloud"].view(np.uint32), cloud.view(np.uint32))
        assert np.array_equal(got["xyz"].view(np.uint32), xyz.view(np.uint32))
    assert np.array_equal(got["gt"], cov[ids])


@pytest.mark.parametrize("pair", [False, True])
def test_pipeline_with_epoch_feeder_matches_plain_loop(pair):
    """tests/test_gpu_pipeline.py::test_pipeline_with_host_feeder_matches_plain_loop with the batches made on the device: hipGraph
    replays, slots zeroed after the capture, a spin kernel in front of every geometry pass, learning rate 0.  P = 7 plots and B = 2
    make epochs of 3 steps, so the 2 n_slots + 3 steps cross several epoch boundaries and refill every slot.  The plain loop's
    batches come from the standalone `fill` with the feeder's ids."""
    from test_gpu_pipeline import _setup
    from stratanet2_vegetation_coverage_maps_amd.pipeline import TrainPipeline
    from oracle import network
    n, B, depth, P = 4096, 2, 2, 7
    n_slots = 2 * depth + 2 if pair else depth + 1
    steps = 2 * n_slots + 3
    args = make_args(cuda=0, subsample_size=n, ratio1=0.125, r1=1.0, ratio2=0.25, r2=2.0)
    sizes = (3000, 5000, n - 316, 6000, 2500, 4500, 3900)
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
        l = fstep(inp)
        opt.step()
        ref.append(float(l.detach()))

    model2, opt2, slots2, fstep2 = _setup(n, B, depth, n_slots, lr=0.0)
    pipe = TrainPipeline(model2, opt2, fstep2, slots2, depth=depth, use_graph=True)
    assert pipe.pair == pair
    pipe.capture()
    for sl in slots2:                                   # wipe the resident copies: the feeder must bring the data
        for k in ("cloud", "xyz", "gt", "pdf", "fps_start"):
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
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-6)
    assert int(opt2.step_dev.item()) == steps
