"""The weight update of every training mode against fp64 Adam over the fp64 oracle's gradients.

The parity tests elsewhere check the forward pass and the gradient of one backward; the pipeline tests compare two loops that
run the same kernels with the same optimiser.  Here the update a mode actually APPLIES is checked against an independent
reference -- the gradient the optimiser consumed, the Adam moments and the new weights:

* probe (learning rate 0, weight decay 0): the weights stay bit-identical, so every step's gradient is a function of that
  step's batch alone and the moments after K steps must equal the fp64 recurrences over the oracle's gradients of the batches
  in the order the mode consumed them.  A partial fold of the gradient images, a stale or misplaced slot, a missed or doubled
  step shows as an O(1) error; every step's loss is checked against its batch's oracle loss as well;
* update leg: one step with bench.py's lr / weight decay / eps from a known state (the probe's moments at step K): moments
  against the oracle gradient + wd * w, weights against the fp64 Adam update from the kernel's own moments (no eps cliff on
  near-zero gradients: the comparison does not depend on how those moments rounded);
* the two Adam kernels alone against fp64 torch.optim.Adam;
* `bench.py --dump-outputs` as typed, mode by mode, against the oracle.
"""
import multiprocessing as mp
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import check, network
from stratanet2_vegetation_coverage_maps_amd import PointNet2, losses, project_to_plotwise_coverages
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
from stratanet2_vegetation_coverage_maps_amd.optim import FlatAdam, flatten_parameters
from stratanet2_vegetation_coverage_maps_amd.pipeline import TrainPipeline
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, B = 4096, 2
B1, B2 = 0.9, 0.999
LR, WD, EPS = 1e-3, 1e-3, 1e-8                   # bench.py's optimiser (config.py:84,97 of the reference) and Adam's eps
TOL_GRAD = 1e-3                                  # oracle.check.compare's gradient tolerance
f32 = lambda x: float(np.float32(x))             # noqa: E731  (the kernels take their hyperparameters as fp32)

# rows of the issue's table: loop kind, gradient images folded by the Adam kernel, pipeline shape, exchange, variant
ROWS = {
    "a_eager_nofold": dict(loop="eager", fold=False),
    "b_eager_fold": dict(loop="eager"),
    "c_serial_graph": dict(loop="serial", fused=True),
    "d_pipe_g1_graph": dict(loop="pipe", G=1, depth=2, graph=True),
    "e_pipe_g1_graph_split": dict(loop="pipe", G=1, depth=2, graph=True, split=True),
    "f_pipe_g1_eager_split": dict(loop="pipe", G=1, depth=2, graph=False, split=True),
    "g_pipe_g2_graph_split": dict(loop="pipe", G=2, depth=2, graph=True, split=True),
    "h_headline": dict(loop="pipe", G=8, depth=3, graph=True, phase=3, fused=True),
    "i_headline_feeder": dict(loop="pipe", G=8, depth=3, graph=True, phase=3, fused=True, feeder=True),
    "j_headline_rccl": dict(loop="pipe", G=8, depth=3, graph=True, phase=3, fused=True, rccl=True),
    "k_headline_3sa": dict(loop="pipe", G=8, depth=3, graph=True, phase=3, fused=True, arch="3sa"),
    "l_headline_bf16": dict(loop="pipe", G=8, depth=3, graph=True, phase=3, fused=True, dtype="bf16"),
}


def _args(arch="ref", dtype="f32", cuda=0):
    kw = dict(ratio3=0.25, r3=4.0) if arch == "3sa" else {}
    args = make_args(cuda=cuda, subsample_size=N, ratio1=0.125, r1=1.0, ratio2=0.25, r2=2.0, **kw)
    args.mma_dtype = "bf16" if dtype == "bf16" else "fp32"
    return args


def _state_dict(arch):
    return network.init_state_dict_3sa(5) if arch == "3sa" else network.init_state_dict(5)


def _host_batch(j, n_fps):
    """Batch number j of this module: plots [40 + 2j, +2), FPS start indices j % 3 (every batch its own loss)."""
    h = make_batch(B, N, first_plot=40 + j * B)
    h["fps_start"] = torch.full((n_fps, B), j % 3, dtype=torch.int32)
    return h


def _dev_batch(h):
    return {"cloud": h["cloud"].cuda(), "xyz": h["xyz"].cuda(), "fps_start": h["fps_start"].cuda(),
            "gt": h["coverages"].cuda(), "pdf": h["pdf_all"].cuda()}


def _layout(model):
    """(name, offset, numel) of every parameter in the flat buffer (the parameters are views of it)."""
    base, es = model._flat_params.data_ptr(), model._flat_params.element_size()
    return [(k, (p.data_ptr() - base) // es, p.numel()) for k, p in model.named_parameters()]


def _flat(layout, n, tensors):
    out = np.zeros(n, dtype=np.float64)
    for k, o, m in layout:
        out[o:o + m] = tensors[k].detach().double().reshape(-1).numpy()
    return out


def _errs(got, want, layout):
    """Per parameter tensor: max |got - want| / max |want|."""
    out = {}
    for k, o, m in layout:
        w, g = want[o:o + m], got[o:o + m]
        scale = np.abs(w).max()
        out[k] = float(np.abs(g - w).max() / scale) if scale > 0 else float(np.abs(g).max())
    return out


def _worst(got, want, layout, tol):
    """-> (worst ratio of a tensor's error (_errs) to its bound, that error, that bound, tensor name); `tol`: one bound for
    every tensor or {tensor: bound}."""
    worst = (-1.0, 0.0, 0.0, "")
    for k, err in _errs(got, want, layout).items():
        t = tol[k] if isinstance(tol, dict) else tol
        if np.isnan(err):
            return float("nan"), err, t, k
        if err / t > worst[0]:
            worst = (err / t, err, t, k)
    return worst


def _checker_bounds(want, want32, layout, tol):
    """Per tensor max(tol, 2 x the fp32 checker's own distance from the fp64 one) -- tests/test_gpu_bf16.py's rule.  At
    default-initialised weights a few batches of this size have BatchNorm channels next to zero variance or ReLU decisions
    next to zero (oracle/check.py): the fp32 oracle itself lands up to ~1e-1 away from the fp64 one on some tensors there
    (measured on batches 4, 5, 26 and 31 of this module), and the HIP gradient, better than the fp32 oracle, still shows
    ~1e-2.  A partial, stale or doubled gradient is an O(1) error on every tensor."""
    return {k: max(tol, 2.0 * e) for k, e in _errs(want32, want, layout).items()}


def _adam_weights(w_before, m, v, t, lr):
    """fp64 Adam update from given moments (fp32 hyperparameters, as the kernel is handed them)."""
    b1, b2, eps = f32(B1), f32(B2), f32(EPS)
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    return w_before - (f32(lr) / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))


def _ulp_bound(p_ref, lr):
    return 2.0 * np.spacing(np.abs(p_ref).astype(np.float32)).astype(np.float64) + 1e-5 * lr


# ---------------------------------------------------------------------------------------------------------------- oracle
@pytest.fixture(scope="module")
def oracle():
    """fp64 oracle step per (arch, dtype, batch number), computed once per module: {loss, grads, new_stats} + the fp32
    checker's gradients ("grads32", for _checker_bounds)."""
    cache, spent = {}, [0.0, 0]

    def get(arch, dtype, j, act_bf16=False):
        key = (arch, dtype, j)
        if key not in cache:
            t0 = time.perf_counter()
            h = _host_batch(j, 3 if arch == "3sa" else 2)
            fs = h["fps_start"].long()
            kw = dict(use_kdtree=True, bf16_layers=PointNet2.BF16_BLOCKS, act_bf16=act_bf16) if dtype == "bf16" else {}
            cache[key] = check.train_step(_state_dict(arch), h, _args(arch, dtype), fps_start=fs, arch=arch, **kw)
            cache[key]["grads32"] = check.train_step(_state_dict(arch), h, _args(arch, dtype), fps_start=fs, arch=arch,
                                                     dtype=torch.float32, **kw)["grads"]
            spent[0] += time.perf_counter() - t0
            spent[1] += 1
        return cache[key]
    get.spent = spent
    yield get
    if spent[1]:
        print(f"\n[oracle] {spent[1]} fp64 + fp32 steps of {B} x {N} in {spent[0]:.1f} s ({spent[0] / spent[1]:.2f} s per batch)")


# ---------------------------------------------------------------------------------------------------------------- modes
def _build(cfg, lr, wd, n_batches):
    """Model, optimiser and the loop of one row; returns run(K) -> (losses (K,) fp64 device tensor, batch numbers consumed)."""
    arch, dtype = cfg.get("arch", "ref"), cfg.get("dtype", "f32")
    args = _args(arch, dtype)
    if arch == "3sa":
        from stratanet2_vegetation_coverage_maps_amd.point_net2_3sa import PointNet2ThreeSA
        model = PointNet2ThreeSA(args)
        model.set_mma_dtype(args.mma_dtype)
    else:
        model = PointNet2(args)
    sd = _state_dict(arch)
    model.load_state_dict(sd)
    model = model.cuda().train()
    fused = cfg.get("fused", False)
    if fused:
        model.p2_diam_pix = args.diam_pix            # bench.build_training: the geometry passes also compute the pixel ids
    flatten_parameters(model)
    comm = None
    if cfg.get("rccl"):
        from stratanet2_vegetation_coverage_maps_amd import rccl
        comm = rccl.comm_from_torch_group("cuda:0")
        assert rccl.self_test(comm, graph=True)
    opt = FlatAdam(model, lr=lr, weight_decay=wd, eps=EPS, comm=comm, fold_gradient_images=cfg.get("fold", True))
    assert opt.fold_gradient_images == (cfg.get("fold", True) and comm is None)
    n_fps = 3 if arch == "3sa" else 2
    host = [_host_batch(j, n_fps) for j in range(n_batches)]
    seed = torch.ones((), dtype=torch.float64, device="cuda")

    def feature_step(inp, geo=None):
        opt.zero_grad()
        cd = {"cloud": inp["cloud"], "xyz": inp["xyz"], "fps_start": inp["fps_start"]}
        if geo is not None:
            cd["geometry"] = geo
        cov, proba = model(cd)
        if fused:                                    # bench.build_training's feature step
            loss, _, _ = losses.projected_total_loss(cov, proba, inp["cloud"], inp["gt"], inp["pdf"], args, geometry=geo, model=model)
            loss.backward(gradient=seed)
        else:                                        # tests/test_gpu_pipeline.py's
            pred = project_to_plotwise_coverages(cov, inp["cloud"], args)
            loss, _ = losses.total_loss(pred, proba, inp["gt"], inp["pdf"], args.m, args.e)
            loss.backward()
        return loss

    def restart(state):
        model.load_state_dict(sd)
        if state is None:
            opt.reset()
        else:
            opt.load_state_dict(state)

    loop = cfg["loop"]
    if loop == "eager":
        dev = [_dev_batch(h) for h in host]

        def run(K, state=None):
            restart(state)
            out = torch.zeros(K, dtype=torch.float64, device="cuda")
            for i in range(K):
                out[i] = feature_step(dev[i % n_batches]).detach()
                opt.step()
            return out, [i % n_batches for i in range(K)]
    elif loop == "serial":
        # bench.py --serial: the whole step (geometry on its forked branches, features, Adam) as ONE hipGraph on a static batch
        dev = [_dev_batch(h) for h in host]
        data = {k: v.clone() for k, v in dev[0].items()}

        def step():
            loss = feature_step(data)
            opt.step()
            return loss
        for _ in range(3):                           # bench.py: eager steps before the capture
            step()
        fork = model.geometry_fork
        model.geometry_fork = True
        try:
            torch.cuda.synchronize()
            side = ops.shared_stream("cuda:0", "capture")
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step()                               # allocator warm-up on the capture stream
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with ops.graph_capture(graph, "cuda:0", allowed_forks=("fork_b", "fork_c", "pack")):
                loss_static = step()
        finally:
            model.geometry_fork = fork

        def run(K, state=None):
            restart(state)
            out = torch.zeros(K, dtype=torch.float64, device="cuda")
            for i in range(K):
                for k, v in dev[i % n_batches].items():
                    data[k].copy_(v)
                graph.replay()
                out[i].copy_(loss_static.detach())
            return out, [i % n_batches for i in range(K)]
    else:
        G, depth = cfg["G"], cfg["depth"]
        n_slots = G * depth + G
        slots = [_dev_batch(host[j]) for j in range(n_slots)]
        pipe = TrainPipeline(model, opt, feature_step, slots, depth=depth, use_graph=cfg["graph"],
                             split_exchange=cfg.get("split", False), group=G, phase=cfg.get("phase", 0))
        assert pipe.slots == n_slots
        pipe.capture()
        feeder = None
        if cfg.get("feeder"):
            # batches from pinned host memory, more distinct ones than slots (tests/test_gpu_pipeline.py's host feeder)
            feeder = [{"cloud": h["cloud"].pin_memory(), "xyz": h["xyz"].pin_memory(), "fps_start": h["fps_start"].pin_memory(),
                       "gt": h["coverages"].pin_memory(), "pdf": h["pdf_all"].pin_memory()} for h in host]
            pipe.set_feeder(lambda i: feeder[i % n_batches])
        runs = [0]

        def run(K, state=None):
            assert runs[0] == 0, "one run per captured pipeline"
            runs[0] += 1
            restart(state)
            pipe.issued = pipe.done = 0
            pipe.prime()
            out = torch.zeros(K, dtype=torch.float64, device="cuda")
            for i in range(K):                       # no host synchronisation inside the loop
                out[i] = pipe.step().detach()
            pipe.drain(check=True)
            return out, [i % (n_batches if feeder else n_slots) for i in range(K)]
    # feature_step and `seed` ride along: a captured graph reads `seed` (the backward's d loss / d loss) by address, and the serial
    # row's run() does not reach them -- freed, the seed's block went to the next small allocation (run()'s loss buffer) and the
    # replays scaled their gradients by whatever that held (0, then the previous step's loss)
    return SimpleNamespace(model=model, opt=opt, run=run, comm=comm, sd=sd, arch=arch, dtype=dtype, args=args,
                           feature_step=feature_step, seed=seed)


def _shape(cfg):
    """(number of distinct batches, K probe steps): K exceeds the slots (every slot reused) and covers every batch."""
    if cfg["loop"] in ("eager", "serial"):
        return 3, 5
    n_slots = cfg["G"] * cfg["depth"] + cfg["G"]
    n_batches = n_slots + 3 if cfg.get("feeder") else n_slots
    return n_batches, n_slots + cfg["G"] + 3


@pytest.mark.parametrize("row", list(ROWS))
def test_training_mode_update_matches_fp64_adam(row, oracle):
    cfg = ROWS[row]
    n_batches, K = _shape(cfg)
    bf16 = cfg.get("dtype") == "bf16"
    tol_g = 2e-2 if bf16 else TOL_GRAD                # tests/test_gpu_bf16.py's gradient bound
    tol_loss = 1e-3 if bf16 else 1e-4                 # ... and its output bound
    t0 = time.perf_counter()

    # ---- probe: lr = 0, wd = 0
    w = _build(cfg, 0.0, 0.0, n_batches)
    act_bf16 = bf16 and w.model._act_dtype(B * N) == torch.bfloat16
    w0 = w.opt.flat.detach().clone()
    out, order = w.run(K)
    torch.cuda.synchronize()
    got_loss = out.cpu().numpy()
    layout, n = _layout(w.model), w.opt.flat.numel()
    refs = {j: oracle(w.arch, w.dtype, j, act_bf16) for j in set(order)}
    g = {j: _flat(layout, n, r["grads"]) for j, r in refs.items()}
    g32 = {j: _flat(layout, n, r["grads32"]) for j, r in refs.items()}
    m_ref, v_ref, m32, v32 = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for j in order:
        m_ref = B1 * m_ref + (1 - B1) * g[j]
        v_ref = B2 * v_ref + (1 - B2) * g[j] ** 2
        m32 = B1 * m32 + (1 - B1) * g32[j]
        v32 = B2 * v32 + (1 - B2) * g32[j] ** 2
    m = w.opt.exp_avg.double().cpu().numpy()
    v = w.opt.exp_avg_sq.double().cpu().numpy()
    em = _worst(m, m_ref, layout, _checker_bounds(m_ref, m32, layout, tol_g))
    ev = _worst(v, v_ref, layout, _checker_bounds(v_ref, v32, layout, 2 * tol_g))
    dloss = np.abs(got_loss - np.array([refs[j]["loss"] for j in order]))
    steps = int(w.opt.step_words[0].item())
    unchanged = torch.equal(w.opt.flat, w0)
    probe_state = {"exp_avg": w.opt.exp_avg.clone(), "exp_avg_sq": w.opt.exp_avg_sq.clone(), "step": steps}
    if w.comm is not None:
        w.comm.destroy()
    del w

    # ---- update leg: one step with bench.py's lr / wd / eps from the probe's state (step K)
    u = _build(cfg, LR, WD, n_batches)
    u0 = _flat(layout, n, u.sd)                      # the start every run() restores
    out1, order1 = u.run(1, state=probe_state)
    torch.cuda.synchronize()
    gp, gp32 = g[order1[0]] + WD * u0, g32[order1[0]] + WD * u0
    m_prev, v_prev = probe_state["exp_avg"].double().cpu().numpy(), probe_state["exp_avg_sq"].double().cpu().numpy()
    mu_ref, mu32 = B1 * m_prev + (1 - B1) * gp, B1 * m_prev + (1 - B1) * gp32
    vu_ref, vu32 = B2 * v_prev + (1 - B2) * gp ** 2, B2 * v_prev + (1 - B2) * gp32 ** 2
    mu, vu = u.opt.exp_avg.double().cpu().numpy(), u.opt.exp_avg_sq.double().cpu().numpy()
    emu = _worst(mu, mu_ref, layout, _checker_bounds(mu_ref, mu32, layout, tol_g))
    evu = _worst(vu, vu_ref, layout, _checker_bounds(vu_ref, vu32, layout, 2 * tol_g))
    p = u.opt.flat.double().cpu().numpy()
    p_ref = _adam_weights(u0, mu, vu, K + 1, LR)
    sel = np.concatenate([np.arange(o, o + c) for _, o, c in layout])
    bound = _ulp_bound(p_ref, LR)
    ep = float((np.abs(p - p_ref)[sel] / bound[sel]).max())
    steps1 = int(u.opt.step_words[0].item())
    dloss1 = abs(float(out1[0]) - refs[order1[0]]["loss"])
    if u.comm is not None:
        u.comm.destroy()

    print(f"\n[{row}] K = {K} steps over {n_batches} batches, {time.perf_counter() - t0:.1f} s (oracle so far: "
          f"{oracle.spent[1]} batches, {oracle.spent[0]:.1f} s)\n"
          f"  probe: exp_avg err {em[1]:.2e} bound {em[2]:.1e} ({em[3]}); exp_avg_sq err {ev[1]:.2e} bound {ev[2]:.1e} ({ev[3]}); "
          f"max |d loss| {dloss.max():.2e} bound {tol_loss:.0e}; steps {steps}; weights unchanged {unchanged}\n"
          f"  update: exp_avg err {emu[1]:.2e} bound {emu[2]:.1e} ({emu[3]}); exp_avg_sq err {evu[1]:.2e} bound {evu[2]:.1e} "
          f"({evu[3]}); weights {ep:.3f} x "
          f"(2 ulp + 1e-5 lr); |d loss| {dloss1:.2e}; steps {steps1}")
    assert unchanged, "lr = 0 moved the weights"
    assert steps == K, f"step count {steps} after {K} steps"
    assert dloss.max() <= tol_loss, f"losses off the oracle's by {dloss.max():.2e} (per step: {dloss})"
    assert em[0] <= 1.0, f"exp_avg off the fp64 recurrence over the oracle's gradients: {em[1]:.2e} on {em[3]}"
    assert ev[0] <= 1.0, f"exp_avg_sq off the fp64 recurrence over the oracle's gradients: {ev[1]:.2e} on {ev[3]}"
    assert steps1 == K + 1
    assert dloss1 <= tol_loss
    assert emu[0] <= 1.0, f"update leg: exp_avg off the oracle gradient + wd w by {emu[1]:.2e} on {emu[3]}"
    assert evu[0] <= 1.0, f"update leg: exp_avg_sq off by {evu[1]:.2e} on {evu[3]}"
    assert ep <= 1.0, f"update leg: weights off the fp64 Adam update from the kernel's own moments: {ep:.3f} x the bound"


# ------------------------------------------------------------------------------------------------------ Adam kernels alone
def _grad_values(n, gen):
    """Magnitudes 1e-12 .. 1 (log-uniform), random signs, exact zeros and values next to eps."""
    g = torch.rand(n, generator=gen, dtype=torch.float64) * 12 - 12
    g = torch.sign(torch.rand(n, generator=gen, dtype=torch.float64) - 0.5) * 10 ** g
    k = torch.randint(0, 8, (n,), generator=gen)
    g[k == 0] = 0.0
    near = k == 1
    g[near] = EPS * (0.25 + 4 * torch.rand(int(near.sum()), generator=gen, dtype=torch.float64))
    return g.float()


@pytest.mark.parametrize("replicas", [None, 1, 2, 5, 32])
def test_adam_kernels_match_fp64_torch_adam(replicas):
    """sn2_adam_step (replicas None) and sn2_adam_step_images (gradient spread over `replicas` images) against fp64
    torch.optim.Adam on the CPU, from states loaded with FlatAdam.load_state_dict at step 0, 1, 999 and 10^6.  The reference
    is handed the fp32 values of lr / betas / eps / weight decay the kernels are handed.  Bounds: weights 2 ulp + 1e-5 lr,
    moments 4e-6 of the larger of their inputs, element by element."""
    gen = torch.Generator().manual_seed(11 + (replicas or 0))
    worst = {"p": 0.0, "m": 0.0, "v": 0.0, "fold": 0.0}
    cases = 0
    for n in (1, 255, 257, 14997):
        for start in (0, 1, 999, 10 ** 6):
            for wd in (0.0, WD):
                for scale in (1.0, 0.5):
                    p0 = (torch.rand(n, generator=gen) * 2 - 1).float()
                    g = _grad_values(n, gen)
                    if start == 0:
                        m0, v0 = torch.zeros(n), torch.zeros(n)
                    else:
                        s = 10 ** (torch.rand(n, generator=gen) * 12 - 12)
                        m0 = (s * (torch.rand(n, generator=gen) * 2 - 1)).float()
                        v0 = (s * s * (0.5 + torch.rand(n, generator=gen))).float()
                    flat = p0.cuda()
                    holder = SimpleNamespace(_flat_params=flat, _last_flat_grad=None, _grad_images_pending=None)
                    opt = FlatAdam(holder, lr=LR, weight_decay=wd, eps=EPS, fold_gradient_images=replicas is not None)
                    opt.step_words.copy_(torch.tensor([123, 7], dtype=torch.int32))     # a stale ticket
                    opt.load_state_dict({"exp_avg": m0.cuda(), "exp_avg_sq": v0.cuda(), "step": start})
                    assert opt.step_words.tolist() == [start, 0], "load_state_dict must reset the ticket word"
                    if replicas is None:
                        gsum = g.double()
                        grad = g.cuda()
                        holder._last_flat_grad = grad
                        if scale == 1.0:
                            opt.step()
                        else:
                            ops.adam_step(flat, grad, opt.exp_avg, opt.exp_avg_sq, LR, B1, B2, EPS, wd, opt.step_words, scale)
                    else:
                        stride = (n + 127) // 128 * 128 + 64
                        arena = torch.full((replicas * stride,), float("nan"))          # padding between images: never read
                        w = torch.rand(replicas, n, generator=gen) + 0.05
                        parts = (g[None, :] * (w / w.sum(0, keepdim=True))).float()     # same-sign parts of g
                        for r in range(replicas):
                            arena[r * stride:r * stride + n] = parts[r]
                        gsum = parts.double().sum(0)
                        arena = arena.cuda()
                        holder._last_flat_grad = arena[:n]
                        holder._grad_images_pending = (arena, replicas, stride)
                        if scale == 1.0:
                            opt.step()
                        else:
                            ops.adam_step_images(flat, arena, replicas, stride, opt.exp_avg, opt.exp_avg_sq, LR, B1, B2, EPS, wd,
                                                 opt.step_words, scale)
                        folded = arena[:n].double().cpu()
                        fe = float(((folded - gsum).abs() / (parts.double().abs().sum(0) * 1e-6 * replicas + 1e-45)).max())
                        worst["fold"] = max(worst["fold"], fe)
                        assert fe <= 1.0, f"folded gradient written back to image 0 off by {fe:.2f} x its bound"
                        assert torch.isnan(arena.view(replicas, stride)[:, n:]).all(), "a write between the images"
                    torch.cuda.synchronize()
                    assert opt.step_words.tolist() == [start + 1, 0]
                    # the fp64 reference
                    pr = torch.nn.Parameter(p0.double().clone())
                    ref = torch.optim.Adam([pr], lr=f32(LR), betas=(f32(B1), f32(B2)), eps=f32(EPS), weight_decay=f32(wd),
                                           foreach=False)
                    ref.state[pr] = {"step": torch.tensor(float(start), dtype=torch.float64),
                                     "exp_avg": m0.double().clone(), "exp_avg_sq": v0.double().clone()}
                    pr.grad = gsum * f32(scale)
                    ref.step()
                    st = ref.state[pr]
                    p_ref = pr.detach()
                    p = flat.double().cpu()
                    bound = torch.from_numpy(_ulp_bound(p_ref.numpy(), LR))
                    e = float(((p - p_ref).abs() / bound).max())
                    gp = (gsum * f32(scale)).abs() + f32(wd) * p0.double().abs()    # (rounding: of the terms, not their sum)
                    em = float(((opt.exp_avg.double().cpu() - st["exp_avg"]).abs() /
                                (4e-6 * torch.maximum(m0.double().abs(), gp) + 1e-45)).max())
                    ev = float(((opt.exp_avg_sq.double().cpu() - st["exp_avg_sq"]).abs() /
                                (4e-6 * torch.maximum(v0.double(), gp * gp) + 1e-45)).max())
                    worst["p"], worst["m"], worst["v"] = max(worst["p"], e), max(worst["m"], em), max(worst["v"], ev)
                    cases += 1
                    assert e <= 1.0, f"n {n} step {start} wd {wd} scale {scale}: weights {e:.2f} x (2 ulp + 1e-5 lr) off fp64 Adam"
                    assert em <= 1.0 and ev <= 1.0, f"n {n} step {start} wd {wd} scale {scale}: moments {em:.2f} / {ev:.2f} x bound"
    print(f"\n[adam {'plain' if replicas is None else f'{replicas} images'}] {cases} cases; worst as a fraction of the bound: "
          f"weights {worst['p']:.3f} (2 ulp + 1e-5 lr), exp_avg {worst['m']:.3f}, exp_avg_sq {worst['v']:.3f}"
          + ("" if replicas is None else f", fold {worst['fold']:.3f}"))


# ------------------------------------------------------------------------------------------------ bench.py as typed
BENCH_MODES = {
    "default": ([], {}),
    "split_exchange": (["--split-exchange"], {}),
    "serial": (["--serial"], {}),
    "exchange_torch": (["--exchange", "torch"], {}),
    "two_ranks_gloo": (["--gpus", "2"], {"SN2_BENCH_ONE_DEVICE": "1", "SN2_BENCH_BACKEND": "gloo"}),
}
BENCH_STEPS, BENCH_WARMUP, BENCH_PLOTS = 8, 2, 2


@pytest.mark.parametrize("mode", list(BENCH_MODES))
def test_bench_dump_outputs_match_fp64_oracle(mode, tmp_path):
    """`bench.py --dump-outputs DIR`: the timed path's own step once more from the seeded start, on the batch of the next
    slot, against the fp64 oracle: loss, flat gradient (two ranks: the SUM over the ranks' shards), exp_avg = 0.1 (g / world
    + wd w0), step 1, the weights from the dumped moments, BatchNorm running statistics."""
    import bench
    from _dist_gpu_worker import run_command
    flags, env = BENCH_MODES[mode]
    world = 2 if "--gpus" in flags else 1
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--plots", str(BENCH_PLOTS), "--points", str(N), "--steps",
           str(BENCH_STEPS), "--warmup", str(BENCH_WARMUP), "--dump-outputs", str(tmp_path)] + flags
    t0 = time.perf_counter()
    ctx = mp.get_context("forkserver")              # started clean in conftest.pytest_configure: never a fork of this process
    q = ctx.Queue()
    proc = ctx.Process(target=run_command, args=(cmd, env, q, 300))
    proc.start()
    rc, out, err = q.get(timeout=330)
    proc.join(60)
    t_bench = time.perf_counter() - t0
    assert rc == 0, err
    dump = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path) if f.endswith(".npy")}

    # the seeded start and the dumped step's batch, from bench's own arithmetic
    pipelined = "--serial" not in flags
    G = bench.pipe_group_for(BENCH_STEPS)
    n_slots = G * 3 + G if pipelined else 1
    j = (BENCH_WARMUP + BENCH_STEPS) % n_slots if pipelined else 0
    args = make_args(cuda=0, subsample_size=N, ratio1=bench.M1 / N, r1=1.0, ratio2=0.25, r2=2.0)
    torch.manual_seed(0)                             # bench.build_training: the model right after the seed
    m0 = PointNet2(args)
    sd0 = {k: v.detach().cpu().clone() for k, v in m0.state_dict().items()}
    flatten_parameters(m0)                           # bench's flat layout
    layout, n_flat = _layout(m0), m0._flat_params.numel()
    refs, refs32 = [], []
    for r in range(world):
        h = make_batch(BENCH_PLOTS, N, first_plot=(j * world + r) * BENCH_PLOTS)
        fs = torch.zeros(2, BENCH_PLOTS, dtype=torch.long)
        refs.append(check.train_step(sd0, h, args, fps_start=fs))
        refs32.append(check.train_step(sd0, h, args, fps_start=fs, dtype=torch.float32))
    t_all = time.perf_counter() - t0

    keys = [k for k, _, _ in layout]
    g_sum = sum(_flat(layout, n_flat, r["grads"]) for r in refs)
    w0 = _flat(layout, n_flat, sd0)
    gd = dump["grad"].astype(np.float64)
    g32 = sum(_flat(layout, n_flat, r["grads"]) for r in refs32)
    eg = _worst(gd, g_sum, layout, _checker_bounds(g_sum, g32, layout, TOL_GRAD))
    gp, gp32 = g_sum / world + WD * w0, g32 / world + WD * w0
    em = _worst(dump["adam.exp_avg"].astype(np.float64), (1 - B1) * gp, layout, _checker_bounds(gp, gp32, layout, TOL_GRAD))
    ev = _worst(dump["adam.exp_avg_sq"].astype(np.float64), (1 - B2) * gp ** 2, layout,
                _checker_bounds(gp ** 2, gp32 ** 2, layout, 2 * TOL_GRAD))
    p = _flat(layout, n_flat, {k: torch.from_numpy(dump["state." + k]) for k in keys})
    p_ref = _adam_weights(w0, dump["adam.exp_avg"].astype(np.float64), dump["adam.exp_avg_sq"].astype(np.float64), 1, LR)
    sel = np.concatenate([np.arange(off, off + c) for _, off, c in layout])
    ep = float((np.abs(p - p_ref)[sel] / _ulp_bound(p_ref, LR)[sel]).max())
    dl = abs(float(dump["loss"].reshape(-1)[0]) - refs[0]["loss"])
    es = 0.0
    for k, ref in refs[0]["new_stats"].items():
        got = dump["state." + k].astype(np.float64)
        es = max(es, float(np.abs(got - ref.double().numpy()).max() / max(1.0, float(ref.abs().max()))))
    print(f"\n[bench {' '.join(flags) or 'default'}] batch {j}, bench {t_bench:.1f} s, with the oracle {t_all:.1f} s\n"
          f"  loss err {dl:.2e} (1e-4); grad err {eg[1]:.2e} on {eg[3]} (bound {eg[2]:.1e}); exp_avg {em[1]:.2e} "
          f"(bound {em[2]:.1e}); exp_avg_sq {ev[1]:.2e} (bound {ev[2]:.1e}); weights {ep:.3f} x (2 ulp + 1e-5 lr); running stats {es:.2e} (1e-4); "
          f"step {int(dump['adam.step'].reshape(-1)[0])}")
    assert dl <= 1e-4, f"loss off the oracle's by {dl:.2e}"
    assert eg[0] <= 1.0, f"dumped gradient off the oracle's by {eg[1]:.2e} on {eg[3]}"
    assert int(dump["adam.step"].reshape(-1)[0]) == 1
    assert em[0] <= 1.0, f"exp_avg off 0.1 (g / world + wd w0) by {em[1]:.2e} on {em[3]}"
    assert ev[0] <= 1.0, f"exp_avg_sq off by {ev[1]:.2e} on {ev[3]}"
    assert ep <= 1.0, f"weights off the fp64 Adam update from the dumped moments: {ep:.3f} x the bound"
    assert es <= 1e-4, f"BatchNorm running statistics off the oracle's by {es:.2e}"
