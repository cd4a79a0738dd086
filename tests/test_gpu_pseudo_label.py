"""Pseudo-labelling end to end on the device (pseudo_label.py, train_data.ResidentPlots.append / eval_batches,
EpochFeeder(plot_subset=...)): synthetic parcels -> prepared plots -> labels of an untrained seeded model -> a resident set, held
bit for bit to the plain loops and to the host route (`ResidentPlots.from_plots` on plots read back).  Nothing here computes a new
floating-point quantity, so every comparison is of bytes."""
import numpy as np
import pytest
import torch

from oracle import network
from stratanet2_vegetation_coverage_maps_amd import PointNet2, evaluation, losses, parcel, project_to_plotwise_coverages
from stratanet2_vegetation_coverage_maps_amd.inference import predict_parcel
from stratanet2_vegetation_coverage_maps_amd.pseudo_label import label_plots, pretrain_split, pseudo_label_parcel
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_parcel
from stratanet2_vegetation_coverage_maps_amd.train_data import EpochFeeder, ResidentPlots

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N = 1024
KW = dict(batch_size=16, fps_start=0, sampler="device", seed=5)
MIN_POINTS = 1000                      # of the set-building tests: the dense half of a parcel (plots of about 2000 points)


def _bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype != torch.float64 else t.contiguous().view(torch.int64)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def world():
    args = make_args(cuda=0, subsample_size=N)
    model = PointNet2(args)
    model.load_state_dict(network.init_state_dict(3))
    model.eval()
    clouds = [make_parcel(seed=s) for s in (11, 12)]
    plots = [parcel.prepare_parcel(c, args) for c in clouds]
    tables = losses.KdeTables(np.linspace(-1.0, 30.0, 64), *[np.linspace(0.1, 1.0, 64) ** k for k in (1, 2, 3)], DEV)
    return {"args": args, "model": model, "clouds": clouds, "plots": plots, "kde": tables}


@pytest.fixture(scope="module")
def built(world):
    """The set of two pseudo_label_parcel calls (capacity larger than needed) and its host-built twin."""
    args, model = world["args"], world["model"]
    keep = [p.n_points[p.n_points > MIN_POINTS] for p in world["plots"]]
    assert all(len(k) >= 8 for k in keep) and all(len(k) < len(p) for k, p in zip(keep, world["plots"]))
    ds = ResidentPlots.empty(int(sum(k.sum() for k in keep)) + 1001, sum(len(k) for k in keep) + 5, DEV)
    raw, centers, labels, counts = [], [], [], []
    for cloud, k in zip(world["clouds"], keep):
        pl, n = pseudo_label_parcel(model, cloud, args, ds, min_points=MIN_POINTS, **KW)
        assert n == len(k) == len(pl) and pl.n_points.tolist() == k.tolist()
        lab = label_plots(model, pl, args, **KW).cpu().numpy()          # the host route: everything read back, plot by plot
        off = np.concatenate([[0], np.cumsum(pl.n_points)])
        host_raw = pl.raw.cpu().numpy()
        raw += [host_raw[:, off[j]:off[j + 1]] for j in range(len(pl))]
        centers.append(pl.centers_host)
        labels.append(lab.astype(np.float64))
        counts.append(n)
    host = ResidentPlots.from_plots(raw, np.concatenate(centers), np.concatenate(labels), DEV)
    torch.cuda.synchronize()
    return ds, host, counts


def _fill(s, ids, args, kde=None, **kw):
    B = len(ids)
    out = {"cloud": torch.full((B, 10, N), float("nan"), device=DEV), "xyz": torch.full((B, 3, N), float("nan"), device=DEV),
           "gt": torch.full((B, 4), float("nan"), dtype=torch.float64, device=DEV),
           "fps_start": torch.full((2, B), -1, dtype=torch.int32, device=DEV), "n_live": torch.full((B,), -1, dtype=torch.int32, device=DEV)}
    if kde is not None:
        out["pdf"] = torch.full((B * N, 3), float("nan"), dtype=torch.float64, device=DEV)
    return s.fill(ids, kw.pop("epoch", 2), kw.pop("seed", 77), args, out, kde=kde, **kw)


# ---- labels ---------------------------------------------------------------------------------------------------------------
def test_labels_equal_the_plain_loop_and_the_mosaic_equals_predict_parcel(world):
    args, model, plots = world["args"], world["model"], world["plots"][0]
    KW = dict(globals()["KW"], batch_size=next(b for b in (16, 15, 14) if len(plots) % b))      # the last batch is short
    model.train()                                                       # label_plots must put this back
    labels = label_plots(model, plots, args, **KW)
    assert model.training and "p2_diam_pix" not in model.__dict__
    assert labels.shape == (len(plots), 4) and labels.dtype == torch.float32 and labels.is_cuda
    model.eval()
    ref = []
    with torch.no_grad():
        for b in plots.batches(args, **KW):
            ref.append(project_to_plotwise_coverages(model(b)[0], b["cloud"], args))
    assert len(ref) == -(-len(plots) // KW["batch_size"]) > 2 and len(plots) % KW["batch_size"] != 0     # several batches, a short one
    assert _same(labels, torch.cat(ref)) and torch.isfinite(labels).all()
    # one pass, both products
    mosaic = parcel.parcel_mosaic(plots.centers_host, args, DEV)
    again = label_plots(model, plots, args, mosaic=mosaic, **KW)
    want = parcel.parcel_mosaic(plots.centers_host, args, DEV)
    assert predict_parcel(model, plots.batches(args, **KW), want, args) == len(plots)
    assert _same(again, labels) and _same(mosaic.mean, want.mean) and _same(mosaic.wsum, want.wsum)
    assert bool(torch.isfinite(mosaic.mean).any())

    class Boom:
        def add(self, *a):
            raise RuntimeError("boom")
    model.train()
    with pytest.raises(RuntimeError, match="boom"):
        label_plots(model, plots, args, mosaic=Boom(), **KW)
    assert model.training and "p2_diam_pix" not in model.__dict__       # restored when a batch raises, too
    model.eval()
    torch.cuda.synchronize()


# ---- the filter -----------------------------------------------------------------------------------------------------------
def test_filter_is_strict_and_prepare_parcel_keeps_the_same_bytes(world):
    """A parcel in which one plot has exactly one point more than another: points that lie in plot A alone are taken out of the
    cloud until A has B's count + 1 (the lattice is passed explicitly, so it does not move)."""
    args, model, cloud, base = world["args"], world["model"], world["clouds"][0], world["plots"][0]
    lattice = parcel.parcel_plot_centers(cloud[0].min(), cloud[0].max(), cloud[1].min(), cloud[1].max(), args)
    off, pidx = base.offsets.cpu().numpy(), base.point_index.cpu().numpy()
    ja = int(np.argmax(base.n_points))
    far = np.hypot(*(base.centers_host - base.centers_host[ja]).T) > 25.0
    jb = int(np.nonzero(far & (base.n_points < base.n_points[ja] - 1) & (base.n_points > 500))[0][0])
    in_a, in_b = pidx[off[ja]:off[ja + 1]], pidx[off[jb]:off[jb + 1]]
    assert not np.intersect1d(in_a, in_b).size
    drop = in_a[:int(base.n_points[ja] - base.n_points[jb] - 1)]
    cloud2 = np.ascontiguousarray(np.delete(cloud, drop, axis=1))
    full = parcel.prepare_parcel(cloud2, args, centers=lattice)
    m = int(base.n_points[jb])
    ia, ib = int(base.plot_index[ja]), int(base.plot_index[jb])
    count = dict(zip(full.plot_index.tolist(), full.n_points.tolist()))
    assert count[ib] == m and count[ia] == m + 1

    # prepare_parcel(min_points=m): the default call's plots with n_points >= m, the same bytes
    some = parcel.prepare_parcel(cloud2, args, centers=lattice, min_points=m)
    kept = np.nonzero(full.n_points >= m)[0]
    assert 0 < len(kept) < len(full) and some.plot_index.tolist() == full.plot_index[kept].tolist()
    assert some.n_points.tolist() == full.n_points[kept].tolist() and some.plot_ids == [full.plot_ids[j] for j in kept]
    assert np.array_equal(some.centers_host, full.centers_host[kept])
    assert _same(some.centers, full.centers[torch.from_numpy(kept).to(DEV)])
    f_off = full.offsets.cpu().numpy()
    cols = torch.from_numpy(np.concatenate([np.arange(f_off[j], f_off[j + 1]) for j in kept])).to(DEV)
    assert _same(some.raw, full.raw[:, cols]) and _same(some.point_index, full.point_index[cols])
    assert some.offsets.cpu().tolist() == np.concatenate([[0], np.cumsum(full.n_points[kept])]).tolist()
    with pytest.raises(ValueError):
        parcel.prepare_parcel(cloud2, args, centers=lattice, min_points=0)

    # pseudo-labelling with min_points = m: the plot of m points is absent, the plot of m + 1 is there
    ds = ResidentPlots.empty(int(full.n_points.sum()), len(full), DEV)
    pl, n = pseudo_label_parcel(model, cloud2, args, ds, min_points=m, centers=lattice, **KW)
    assert ib not in pl.plot_index.tolist() and ia in pl.plot_index.tolist()
    assert n == int((full.n_points > m).sum()) == ds.P and int(ds.n_points.min()) == m + 1
    assert pl.plot_index.tolist() == full.plot_index[full.n_points > m].tolist()
    # a parcel with nothing to keep: 0, and the set is untouched; a parcel that does not fit: refused before anything is appended
    version = ds.version
    assert pseudo_label_parcel(model, cloud2, args, ds, min_points=10 ** 6, centers=lattice, **KW)[1] == 0 and ds.version == version
    tiny = ResidentPlots.empty(1000, 2, DEV)
    with pytest.raises(ValueError, match="need a capacity"):
        pseudo_label_parcel(model, cloud2, args, tiny, min_points=m, centers=lattice, **KW)
    assert tiny.P == 0 and tiny.version == 0
    torch.cuda.synchronize()


# ---- set building ---------------------------------------------------------------------------------------------------------
def test_set_of_two_parcels_equals_the_host_built_set(world, built):
    ds, host, counts = built
    args = world["args"]
    assert ds.P == host.P == sum(counts) and ds.n_filled == host.n_filled == host.raw.shape[1] < ds.point_capacity
    assert ds.plot_capacity > ds.P and ds.n_points_max == host.n_points_max and ds.n_points.tolist() == host.n_points.tolist()
    assert _same(ds.raw[:, :ds.n_filled], host.raw)
    assert _same(ds.offsets, host.offsets) and _same(ds.centers, host.centers) and _same(ds.coverages, host.coverages)
    assert ds.offsets.is_contiguous() and ds.centers.is_contiguous() and ds.coverages.is_contiguous()
    assert ds.coverages.dtype == torch.float64 and tuple(ds.coverages.shape) == (ds.P, 4)
    ids = [ds.P - 1, 0, counts[0], counts[0] - 1, 3]                     # both parcels, the seam between them
    a = _fill(ds, ids, args, train=True, noise=True)
    b = _fill(host, ids, args, train=True, noise=True)
    for k in ("cloud", "xyz", "gt", "fps_start", "n_live"):
        assert _same(a[k], b[k]), k
    assert torch.isfinite(a["cloud"]).all() and int(a["n_live"].min()) > 0
    # the mixture is fitted from the arena as it lies: no copy
    za = losses.sample_heights(ds.raw, size=4096, seed=1, offsets=ds.offsets, device=DEV)
    zb = losses.sample_heights(host.raw, size=4096, seed=1, offsets=host.offsets, device=DEV)
    assert _same(za, zb)


# ---- staleness ------------------------------------------------------------------------------------------------------------
def test_a_feeder_built_before_an_append_is_refused_and_fill_gets_a_new_workspace(world):
    args, plots = world["args"], world["plots"][0]
    cov = torch.rand(len(plots), 4, generator=torch.Generator().manual_seed(1)).to(DEV)
    order = np.argsort(plots.n_points, kind="stable")
    small, big = order[:6].tolist(), order[-1:].tolist()
    ds = ResidentPlots.empty(int(plots.n_points[small + big].sum()) + 64, 8, DEV)
    assert ds.append(plots, cov, select=small) == 6
    before = ds.n_points_max
    first = _fill(ds, [5, 0, 2], args)                                   # caches a workspace sized for the small plots
    feeder = EpochFeeder(ds, args, 2, 1)
    feeder.batch_ids(0)
    assert ds.append(plots, cov, select=big) == 1 and ds.n_points_max == int(plots.n_points.max()) > before
    assert ds.n_points_max + 316 > N                                     # the new plot is subsampled: index rows in the workspace
    assert not ds._ws
    with pytest.raises(RuntimeError, match="changed"):
        feeder.batch_ids(1)
    with pytest.raises(RuntimeError, match="changed"):
        feeder.fill_slot(0, {})
    off = np.concatenate([[0], np.cumsum(plots.n_points)])
    host_raw = plots.raw.cpu().numpy()
    sel = small + big
    host = ResidentPlots.from_plots([host_raw[:, off[j]:off[j + 1]] for j in sel], plots.centers_host[sel],
                                    cov.cpu().numpy().astype(np.float64)[sel], DEV)
    a, b = _fill(ds, [6, 5, 0], args), _fill(host, [6, 5, 0], args)
    for k in ("cloud", "xyz", "gt", "fps_start", "n_live"):
        assert _same(a[k], b[k]), k
    fresh = EpochFeeder(ds, args, 2, 1)                                  # a feeder built on the completed set runs
    assert fresh.P == 7 and fresh.batch_ids(0).numel() == 2
    assert _same(first["gt"][0], a["gt"][1])                             # plot 5 kept its row through the append
    torch.cuda.synchronize()


# ---- training on a subset, validating on the rest -------------------------------------------------------------------------
def test_training_draws_only_the_subset_and_eval_batches_feed_evaluate(world, built):
    from test_gpu_pipeline import _setup
    from stratanet2_vegetation_coverage_maps_amd.pipeline import TrainPipeline
    ds, host, counts = built
    kde = world["kde"]
    train_ids, val_ids = pretrain_split(ds.P)
    assert len(val_ids) == min(int(0.2 * ds.P), 100) >= 3 and len(train_ids) + len(val_ids) == ds.P
    B, depth, steps = 2, 2, 3
    pargs = make_args(cuda=0, subsample_size=N, ratio1=0.125, r1=1.0, ratio2=0.25, r2=2.0)      # the network _setup builds
    model, opt, slots, fstep = _setup(N, B, depth)
    feeder = EpochFeeder(ds, pargs, B, 9, kde=kde, plot_subset=train_ids, generator=torch.Generator().manual_seed(4))
    assert feeder.steps_per_epoch == len(train_ids) // B and feeder.P == ds.P
    seen = []
    fill_slot = feeder.fill_slot

    def recording(i, slot):
        seen.extend(feeder.batch_ids(i).tolist())
        return fill_slot(i, slot)
    feeder.fill_slot = recording
    pipe = TrainPipeline(model, opt, fstep, slots, depth=depth, use_graph=False)
    pipe.capture()
    pipe.issued = pipe.done = 0
    pipe.set_feeder(feeder)
    pipe.prime()
    out = torch.zeros(steps, dtype=torch.float64, device=DEV)
    for i in range(steps):
        out[i] = pipe.step().detach()
    pipe.drain()
    torch.cuda.synchronize()
    got = out.cpu().tolist()
    assert all(np.isfinite(got)), got
    assert len(seen) >= steps * B and set(seen) <= set(train_ids.tolist()) and not set(seen) & set(val_ids.tolist())

    # validation on the held-out plots: eval_batches against hand-built dicts from fill(train=False)
    args, emodel = world["args"], world["model"]
    batches = list(ds.eval_batches(val_ids, args, 4, seed=3, kde=kde))
    assert [b["cloud"].shape[0] for b in batches] == [4] * (len(val_ids) // 4) + ([len(val_ids) % 4] if len(val_ids) % 4 else [])
    assert len({b["cloud"].data_ptr() for b in batches}) == len(batches)                    # tensors of their own
    by_hand = []
    for b0 in range(0, len(val_ids), 4):
        ids = val_ids[b0:b0 + 4].tolist()
        o = _fill(ds, ids, args, kde=kde, epoch=0, seed=3, train=False)
        by_hand.append({"cloud": o["cloud"], "xyz": o["xyz"], "coverages": o["gt"], "plot_id": ids, "fps_start": o["fps_start"],
                        "n_live": o["n_live"], "pdf_all": o["pdf"]})
    for b, h in zip(batches, by_hand):
        for k in ("cloud", "xyz", "coverages", "fps_start", "n_live", "pdf_all"):
            assert _same(b[k], h[k]), k
        assert b["plot_id"].tolist() == h["plot_id"]
    res, summ = evaluation.evaluate(emodel, ds.eval_batches(val_ids, args, 4, seed=3, kde=kde), args, kde=kde)
    want, wsumm = evaluation.evaluate(emodel, by_hand, args, kde=kde)
    assert [s["pl_id"] for s in summ] == val_ids.tolist() == [s["pl_id"] for s in wsumm]
    assert res["per_plot"]["losses"].tobytes() == want["per_plot"]["losses"].tobytes()
    assert res["per_plot"]["pred"].tobytes() == want["per_plot"]["pred"].tobytes() and res["total_loss"] == want["total_loss"]
    assert np.isfinite(res["per_plot"]["losses"]).all()
    gt = ds.coverages[torch.from_numpy(val_ids).to(DEV)].cpu().numpy()
    assert [[s[k] for k in ("vt_veg_b", "vt_sol_nu", "vt_veg_moy", "vt_veg_h")] for s in summ] == gt.tolist()


# ---- no host reads --------------------------------------------------------------------------------------------------------
def test_labelling_and_appending_read_nothing_back(world, monkeypatch):
    args, model, cloud = world["args"], world["model"], world["clouds"][1]
    plots = parcel.prepare_parcel(cloud, args, min_points=MIN_POINTS + 1)
    cap = (int(plots.n_points.sum()) * 2 + 8, 2 * len(plots) + 2)
    ds = ResidentPlots.empty(*cap, DEV)
    ds.append(plots, label_plots(model, plots, args, **KW))              # warm-up: lazy loads, allocator
    pseudo_label_parcel(model, cloud, args, ResidentPlots.empty(*cap, DEV), min_points=MIN_POINTS, **KW)
    torch.cuda.synchronize()
    counts, current = {}, [None]

    def counted(name, fn, tensor_method):
        def wrapper(*a, **kw):
            if not tensor_method or a[0].is_cuda:                        # a device-to-host read (or a synchronize)
                counts[current[0]][name] += 1
            return fn(*a, **kw)
        return wrapper
    for name in ("item", "cpu", "tolist", "numpy"):
        monkeypatch.setattr(torch.Tensor, name, counted(name, getattr(torch.Tensor, name), True))
    monkeypatch.setattr(torch.cuda, "synchronize", counted("synchronize", torch.cuda.synchronize, False))

    def run(key, fn):
        current[0] = key
        counts[key] = {"item": 0, "cpu": 0, "tolist": 0, "numpy": 0, "synchronize": 0}
        return fn()
    n = run("label+append", lambda: ds.append(plots, label_plots(model, plots, args, **KW)))
    run("prepare", lambda: parcel.prepare_parcel(cloud, args, min_points=MIN_POINTS + 1))
    fresh = ResidentPlots.empty(*cap, DEV)
    _, n2 = run("parcel", lambda: pseudo_label_parcel(model, cloud, args, fresh, min_points=MIN_POINTS, **KW))
    monkeypatch.undo()
    print(f"\nhost reads: {counts}")
    assert n == n2 == len(plots) and ds.P == 2 * len(plots)
    assert sum(counts["label+append"].values()) == 0
    assert sum(counts["prepare"].values()) >= 1
    assert all(counts["parcel"][k] <= counts["prepare"][k] for k in counts["prepare"])
    torch.cuda.synchronize()
    assert _same(ds.coverages[:len(plots)], ds.coverages[len(plots):]) and _same(fresh.coverages, ds.coverages[:len(plots)])
