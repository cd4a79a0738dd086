"""The 3sa-arch variant (three ball-query levels; not in the reference) against the oracle's generalisation."""
import numpy as np
import pytest
import torch

from oracle import check, network
from stratanet2_vegetation_coverage_maps_amd import losses, project_to_plotwise_coverages
from stratanet2_vegetation_coverage_maps_amd.point_net2_3sa import PointNet2ThreeSA
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_batch

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.mark.parametrize("B,N,ratio1", [(2, 4096, 0.125), (1, 8192, 0.125)])
def test_3sa_forward_backward_vs_oracle(B, N, ratio1):
    args = make_args(cuda=0, subsample_size=N, ratio1=ratio1, r1=1.0, ratio2=0.25, r2=2.0, ratio3=0.25, r3=4.0)
    d = make_batch(B, N, first_plot=500)
    sd = network.init_state_dict_3sa(2)
    fs = torch.stack([torch.arange(B) * 5 % N, torch.arange(B) % 7, torch.zeros(B, dtype=torch.long)])
    d["fps_start"] = fs
    m = PointNet2ThreeSA(args)
    m.load_state_dict(sd)
    m.train()
    assert sorted(m.state_dict().keys()) == sorted(sd.keys())
    cov, proba = m(d)
    pred = project_to_plotwise_coverages(cov, d["cloud"], args, model=m)
    loss, _ = losses.total_loss(pred, proba, d["coverages"].cuda(), d["pdf_all"].cuda(), args.m, args.e)
    loss.backward()
    ref = check.train_step(sd, d, args, fps_start=fs, arch="3sa")           # the oracle's generalisation, in fp64
    # gradients 2e-3: the one-plot case has 64-row BatchNorms at the third level, where a single ReLU decision next to zero
    # moves the gradients behind it by ~1e-3 (measured 1.4e-3 on fp2's bias; everything in front of it agrees to 3e-6)
    fails, report = check.compare(m, cov, proba, loss.item(), ref, pred=pred, tol_grad=2e-3)
    print(f"\n[3sa {B} x {N}] vs the fp64 oracle:\n  {report}")
    assert not fails, "\n".join(fails)


def test_3sa_backward_through_an_eval_forward_vs_oracle():
    """model.eval() with autograd on (tests/test_gpu_network.py::test_backward_through_an_eval_forward_vs_oracle), the variant."""
    B, N = 2, 4096
    args = make_args(cuda=0, subsample_size=N, ratio1=0.125, r1=1.0, ratio2=0.25, r2=2.0, ratio3=0.25, r3=4.0)
    d = make_batch(B, N, first_plot=520)
    g = torch.Generator().manual_seed(4)
    sd = network.init_state_dict_3sa(2)
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = 0.2 * torch.randn(sd[k].shape, generator=g)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(sd[k].shape, generator=g)
    fs = torch.stack([torch.arange(B) * 5 % N, torch.arange(B) % 7, torch.zeros(B, dtype=torch.long)])
    d["fps_start"] = fs
    m = PointNet2ThreeSA(args)
    m.load_state_dict(sd)
    m.eval()
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    cov, proba = m(d)
    pred = project_to_plotwise_coverages(cov, d["cloud"], args, model=m)
    loss, _ = losses.total_loss(pred, proba, d["coverages"].cuda(), d["pdf_all"].cuda(), args.m, args.e)
    loss.backward()
    ref = check.train_step(sd, d, args, fps_start=fs, arch="3sa", training=False)
    fails, report = check.compare(m, cov, proba, loss.item(), ref, pred=pred, tol_grad=2e-3)
    print(f"\n[3sa {B} x {N}] eval-mode step vs the fp64 oracle:\n  {report}")
    assert not fails, "\n".join(fails)
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), f"{k} changed in an eval-mode step"


@pytest.mark.parametrize("pair", [False, True, 4])
def test_3sa_in_the_pipelined_loop_matches_the_plain_loop(pair):
    """`bench.py --arch 3sa` drives this model through TrainPipeline (geometry passes on side streams -- one per batch, or one
    per two batches in pair mode --, feature graphs per slot): the same losses as the plain loop."""
    from stratanet2_vegetation_coverage_maps_amd.optim import FlatAdam, flatten_parameters
    from stratanet2_vegetation_coverage_maps_amd.pipeline import TrainPipeline
    G = int(pair) if pair not in (False, True) else (2 if pair else 1)          # batches per geometry pass
    pair = G > 1
    N, B, depth, steps = 4096, 2, 2, (2 * G + 4) if pair else 6
    n_slots = G * depth + G

    def setup():
        args = make_args(cuda=0, subsample_size=N, ratio1=0.125, r1=1.0, ratio2=0.25, r2=2.0, ratio3=0.25, r3=4.0)
        model = PointNet2ThreeSA(args)
        model.load_state_dict(network.init_state_dict_3sa(2))
        model = model.cuda().train()
        flatten_parameters(model)
        opt = FlatAdam(model, lr=0.0, eps=1e-3)          # lr 0: every step must reproduce the plain loop's loss
        slots = []
        for j in range(n_slots):
            h = make_batch(B, N, first_plot=300 + j * B)
            slots.append({"cloud": h["cloud"].cuda(), "xyz": h["xyz"].cuda(),
                          "fps_start": torch.full((3, B), j, dtype=torch.int32, device="cuda"),
                          "gt": h["coverages"].cuda(), "pdf": h["pdf_all"].cuda()})

        def fstep(inp, geo=None):
            opt.zero_grad()
            cd = {"cloud": inp["cloud"], "xyz": inp["xyz"], "fps_start": inp["fps_start"]}
            if geo is not None:
                cd["geometry"] = geo
            cov, proba = model(cd)
            pred = project_to_plotwise_coverages(cov, inp["cloud"], args)
            loss, _ = losses.total_loss(pred, proba, inp["gt"], inp["pdf"], args.m, args.e)
            loss.backward()
            return loss
        return model, opt, slots, fstep

    model, opt, slots, fstep = setup()
    ref = []
    for i in range(steps):
        ref.append(float(fstep(slots[i % len(slots)]).detach()))
        opt.step()
    model2, opt2, slots2, fstep2 = setup()
    pipe = TrainPipeline(model2, opt2, fstep2, slots2, depth=depth, group=G)
    assert pipe.pair == pair and pipe.group == G
    pipe.capture()
    pipe.prime()
    got = [float(pipe.step().detach()) for _ in range(steps)]
    pipe.drain()
    torch.cuda.synchronize()
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-6)


def test_3sa_prefetched_geometry_and_parcel_loop():
    """`prefetch_geometry` (inherited) and `inference.predict_parcel` drive the 3sa model too: an eval-mode pass skips the
    inverted 3-NN tables (`inverted=False`), a training-mode forward on the same handle builds them; the prefetched
    forward returns the bits of the plain one."""
    from stratanet2_vegetation_coverage_maps_amd import inference
    N, B = 4096, 2
    args = make_args(cuda=0, subsample_size=N, ratio1=0.125, r1=1.0, ratio2=0.25, r2=2.0, ratio3=0.25, r3=4.0)
    model = PointNet2ThreeSA(args)
    model.load_state_dict(network.init_state_dict_3sa(2))
    d = make_batch(B, N, first_plot=40)
    d["fps_start"] = torch.zeros(3, B, dtype=torch.long)
    model.eval()
    with torch.no_grad():
        cov0, proba0 = model(d)
        geo = model.prefetch_geometry(d)
        assert geo.has_inverted is False
        cov1, proba1 = model(dict(d, geometry=geo))
    assert torch.equal(cov0, cov1) and torch.equal(proba0, proba1)
    # eval-prefetched tables under a training-mode forward + backward
    model.train()
    geo = model.eval().prefetch_geometry(d)
    model.train()
    cov, proba = model(dict(d, geometry=geo))
    assert geo.has_inverted is True
    (cov.sum() + proba.sum()).backward()
    g_pre = [p.grad.clone() for p in model.parameters()]
    model.zero_grad(set_to_none=True)
    cov2, proba2 = model(d)
    (cov2.sum() + proba2.sum()).backward()
    assert torch.equal(cov, cov2)
    for a, b in zip(g_pre, (p.grad for p in model.parameters())):
        # the backward adds its weight gradients with float atomics: two runs agree to ~1e-6 of a tensor's magnitude
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-12
    # the parcel loop with its default prefetch of 3 passes
    batches = []
    for s in range(3):
        h = make_batch(B, N, first_plot=60 + s * B)
        c = torch.tensor([[10.0 + 5 * (s * B + i), 10.0] for i in range(B)], dtype=torch.float64)
        batches.append({"cloud": h["cloud"], "xyz": h["xyz"], "plot_center": c, "fps_start": torch.zeros(3, B, dtype=torch.long)})
    H, W = 20, 20 + 5 * (3 * B - 1)
    mos = inference.ParcelMosaic(0.0, float(H), H, W, args, torch.device("cuda:0"))
    assert inference.predict_parcel(model, batches, mos, args) == 3 * B
    mos0 = inference.ParcelMosaic(0.0, float(H), H, W, args, torch.device("cuda:0"))
    assert inference.predict_parcel(model, batches, mos0, args, prefetch=0) == 3 * B
    assert torch.equal(torch.nan_to_num(mos0.result()), torch.nan_to_num(mos.result()))


def test_3sa_grouped_geometry_pass_matches_the_per_batch_passes():
    """`_geometry_pair` of the variant (the base class's grouped pass: `*_group` launches into strided buffers, the group's cloud
    in one tensor) against one `_geometry(..., cloud=)` call per batch: the same bits in every table, and a training step through a
    grouped handle gives the outputs of a step through the per-batch handle.  M = 512 / 128 / 32 on 4096 points: the level-1 FPS
    fills its workspace and the per-point 3-NN table takes its grid form."""
    from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
    B, N, L = 2, 4096, 3
    dev = torch.device("cuda:0")
    args = make_args(cuda=0, subsample_size=N, ratio1=0.125, r1=1.0, ratio2=0.25, r2=2.0, ratio3=0.25, r3=4.0)
    model = PointNet2ThreeSA(args)
    model.load_state_dict(network.init_state_dict_3sa(2))
    model.train()
    model.p2_diam_pix = int(args.diam_pix)
    Ms = (N,) + tuple(model._sizes(N))
    assert Ms == (4096, 512, 128, 32)
    assert ops.fps_fills_ws(B, N, Ms[1]) and ops.three_nn_uses_grid(Ms[1], N)

    def tables(g, with_cloud):
        t = {}
        for l in range(1, L + 1):
            cnt = getattr(g, f"cnt{l}")
            nbr = getattr(g, f"nbr{l}")
            live = torch.arange(nbr.shape[1], device=dev)[None, :] < cnt[:, None]         # the first cnt entries of a list are defined
            t[f"nbr{l}"] = torch.where(live, nbr, -1)
            for name in (f"idx{l}", f"pos{l}_aos", f"pos{l}_soa", f"cnt{l}", f"tot{l}", f"ord{l}"):
                t[name] = getattr(g, name)
        for j in range(1, L + 2):
            t[f"knn{j}_idx"], t[f"knn{j}_w"] = getattr(g, f"knn{j}")
        if with_cloud:
            assert g.has_rows0 and g.p2_diam_pix == int(args.diam_pix)
            t["rows0"], t["p2_pix"], t["p2_mm"] = g.rows0, g.p2_pix, g.p2_mm
        return t

    step = None
    for G, group_cloud in ((2, True), (3, False)):
        hosts = [make_batch(B, N, first_plot=700 + 10 * G + h * B) for h in range(G)]
        xyz2 = torch.cat([h["xyz"] for h in hosts]).to(dev, torch.float32).contiguous()
        cloud2 = torch.cat([h["cloud"] for h in hosts]).to(dev, torch.float32).contiguous()
        fs2 = (torch.arange(L * G * B, dtype=torch.int32).view(L, G * B) * 3 % 32).to(dev)
        gp, halves = model.alloc_geometry_pair(B, N, dev, group=G)
        model._geometry_pair(xyz2, fs2, gp, halves, **({"cloud2": cloud2} if group_cloud else {}))
        for h, g in enumerate(halves):
            sl = slice(h * B, (h + 1) * B)
            ref = model._geometry(xyz2[sl], fs2[:, sl].contiguous(), cloud=cloud2[sl])
            got, want = tables(g, group_cloud), tables(ref, group_cloud)
            for name in want:
                assert torch.equal(got[name], want[name]), f"G={G}, batch {h}: {name}"
            if step is None and h == 1:
                step = (hosts[h], fs2[:, sl].contiguous(), g, ref)
    # a training forward and backward through the grouped handle and through the per-batch handle
    d, fs, g_grp, g_one = step
    out = []
    for geo in (g_grp, g_one):
        model.zero_grad(set_to_none=True)
        cov, proba = model({"cloud": d["cloud"], "xyz": d["xyz"], "fps_start": fs, "geometry": geo})
        (cov.sum() + proba.sum()).backward()
        out.append((cov, proba, [p.grad.clone() for p in model.parameters()]))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    for a, b in zip(out[0][2], out[1][2]):
        # the backward adds its weight gradients with float atomics: two runs agree to ~1e-6 of a tensor's magnitude
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-12
