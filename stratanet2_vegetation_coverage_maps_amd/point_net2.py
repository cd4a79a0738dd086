"""PointNet2 -- drop-in for the reference `model/point_net2.py` (IGNF/StrataNet2), MI355X-native underneath.

Same public surface as the reference class (`/root/reference/model/point_net2.py:70-220`): constructor fields read
from `args`, `forward(cloud_data) -> (coverages_pointwise, proba_pointwise)`, `get_long_form`, `get_batch_format`,
early-stopping / checkpoint helpers, and a `state_dict()` with the reference's exact keys and shapes
(`sa1_module.conv.local_nn.0.0.weight`, ..., `lin2.bias`), so reference checkpoints load and the reference training
and inference drivers (`learning/train.py:53-56`, `predict.py:103-114`) can call it unchanged.

Underneath, `forward` is ONE autograd node whose forward and backward are sequences of hand-written HIP kernels
(libstrata_hip.so via ctypes, raw device pointers, torch's current stream): FPS -> ball query -> fused
gather+MLP+BN+max (SA1, SA2) -> global SA -> 3-NN interpolation + MLP (FP3..FP1) -> head.  No torch_cluster /
torch_scatter / torch_geometric, no per-edge tensors, no host synchronisation anywhere in a step.

Additive extensions: `cloud_data["fps_start"]` -- int tensor (2,B) of LOCAL start indices for the two FPS calls ((L,B) for L levels)
(the reference's `fps` starts at a C `rand()` point and is unseeded).  Absent: random starts
drawn with torch's generator in training mode... the reference draws them in eval mode too, so does this class.
`cloud_data["n_live"]` -- int tensor (B): plot b's points [n_live[b], N) are bit-identical copies of earlier ones, which is how
every sampler lays out a plot with fewer candidates than `subsample_size` (input_pipeline.live_counts).  The FPS kernels then skip
the copies (include/strata_hip.h: sn2_fps_live); outputs and tables are the same bytes as without the key.  Absent: all N points.
"""
import os
from collections import OrderedDict

import torch
import torch.nn as nn
from torch.nn import BatchNorm1d as BN
from torch.nn import Linear as Lin
from torch.nn import ReLU
from torch.nn import Sequential as Seq

from . import executor as X
from . import hip_ops as ops
from ._lib import BN_FROZEN_KEEP, MAX_NEIGHBORS as _MAXN, STAT_SLOTS, StrataHipError

MAX_NEIGHBORS = _MAXN      # radius(..., max_num_neighbors=2000), model/point_net2.py:24 (tests lower it by monkeypatching)

F32, I32, I64, F64 = torch.float32, torch.int32, torch.int64, torch.float64


def MLP(channels):
    """(Linear -> ReLU -> BatchNorm1d) blocks with the reference's module nesting, hence its state-dict keys
    `<i>.0.*` (Linear) and `<i>.2.*` (BatchNorm)  -- model/point_net2.py:45-53."""
    return Seq(*[Seq(Lin(channels[i - 1], channels[i]), ReLU(), BN(channels[i])) for i in range(1, len(channels))])


class PointConv(nn.Module):
    """Parameter holder named like torch_geometric's PointConv (`.local_nn`); the computation is sn2_sa_forward."""

    def __init__(self, local_nn):
        super().__init__()
        self.local_nn = local_nn


class SAModule(nn.Module):
    def __init__(self, ratio, r, nn_):
        super().__init__()
        self.ratio, self.r = ratio, r
        self.conv = PointConv(nn_)


class GlobalSAModule(nn.Module):
    def __init__(self, nn_):
        super().__init__()
        self.nn = nn_


class FPModule(nn.Module):
    def __init__(self, k, nn_):
        super().__init__()
        self.k = k
        self.nn = nn_


def _at(o, stem, l, tail=""):
    """The level-numbered attribute `<stem><l><tail>` of a geometry handle or a saved set: idx1, pos2_soa, knn3, ..."""
    return getattr(o, f"{stem}{l}{tail}")


def _put(o, stem, l, value, tail=""):
    setattr(o, f"{stem}{l}{tail}", value)


def _pad4(c):
    return (c + 3) // 4 * 4


class _Saved:
    """Everything the backward pass needs from one forward (device tensors + sizes)."""
    pass


def _blocks_of(seq, aux_arena, stats_arena, cursor, mma_bf16=False):
    out = []
    for blk in seq:
        lin, bn = blk[0], blk[2]
        c = lin.out_features
        aux = aux_arena[cursor[0]:cursor[0] + 4 * c].view(4, c)
        ns = STAT_SLOTS * 2 * c
        st = stats_arena[cursor[1]:cursor[1] + ns]
        cursor[0] += 4 * c
        cursor[1] += ns
        out.append(ops.BlockBuffers(lin, bn, aux, st))
        out[-1].mma_bf16 = mma_bf16
    return out


class _PointNet2Fn(torch.autograd.Function):
    """forward/backward of the whole network as one autograd node; `params` are passed so autograd routes their
    gradients, the kernels read them through the modules (same storage)."""

    @staticmethod
    def forward(ctx, model, xyz, cloud, fps_start, geo, drop_keep, *params):
        training = model.training
        # will a backward pass follow?  Grad mode is off inside Function.forward, and ctx.needs_input_grad reports the inputs'
        # requires_grad flags WHATEVER the caller's grad mode (round 5: under torch.no_grad() it said yes, and an eval forward
        # took the everything-kept path of the eval-mode backward): the callers record torch.is_grad_enabled() in front of apply
        need_grad = bool(getattr(model, "_grad_mode_at_call", True)) and any(ctx.needs_input_grad[6:])
        # (the batch's live prefixes, cloud_data["n_live"], ride the same way: only a forward that runs its own geometry pass reads them)
        n_live = model.__dict__.pop("_n_live_at_call", None)
        cov, proba, saved = model._forward_impl(xyz, cloud, fps_start, training, geo, drop_keep, need_grad=need_grad,
                                                **({} if n_live is None else {"n_live": n_live}))
        ctx.model = model
        if not isinstance(saved, X.NetSaved):
            saved.training = training
        ctx.saved = saved if need_grad else None
        ctx.n_params = len(params)
        return cov, proba

    @staticmethod
    def backward(ctx, dcov, dproba):
        if ctx.saved is None:
            raise RuntimeError("PointNet2: backward through a forward that recorded no graph")
        # (after an eval-mode forward -- BatchNorm on its running statistics, model/point_net2.py:45-53 -- the gradient is the
        # running-statistics one, gamma * invstd * dy: the forward kept what a training forward keeps and marked its blocks
        # `frozen`, sn2_block.frozen_stats; round 5)
        # the loss node may have left its gradient as a descriptor (losses.PendingLossGrad) and two placeholders: if BOTH incoming
        # gradients are exactly those, the head backward computes them itself; otherwise cov or proba had another consumer and
        # autograd summed something onto a placeholder (a zero): the descriptor is materialised and added.  Cleared either way.
        pending = ctx.__dict__.pop("loss_grad", None)
        loss = None
        if pending is not None:
            if pending.is_placeholder(dcov) and pending.is_placeholder(dproba):
                loss, dcov, dproba = pending.desc(), None, None
            else:
                gc, gp = pending.materialize()
                dcov = gc if (dcov is None or pending.is_placeholder(dcov)) else dcov + gc
                dproba = gp if (dproba is None or pending.is_placeholder(dproba)) else dproba + gp
        grads = ctx.model._backward_impl(ctx.saved, dcov, dproba) if loss is None else ctx.model._backward_impl(ctx.saved, None, None, loss=loss)
        ctx.saved = None
        return (None, None, None, None, None, None) + tuple(grads)


class PointNet2(nn.Module):
    def __init__(self, args):
        super().__init__()
        self._init_fields(args)
        ndim = 3
        mlp1 = [self.n_input_feats + ndim, 16, 16]
        mlp2 = [mlp1[-1] + ndim, 32]
        mlp3 = [mlp2[-1] + ndim, 64]
        # construction order = the reference's (point_net2.py:84-96): same RNG stream => same default weights
        self.sa1_module = SAModule(args.ratio1, args.r1, MLP(mlp1))
        self.sa2_module = SAModule(args.ratio2, args.r2, MLP(mlp2))
        self.sa3_module = GlobalSAModule(MLP(mlp3))
        mlp3_fp = [mlp3[-1] + mlp2[-1], 64]
        mlp2_fp = [mlp3_fp[-1] + mlp1[-1], 34]
        mlp1_fp = [mlp2_fp[-1] + self.n_input_feats, 34]
        self.fp3_module = FPModule(1, MLP(mlp3_fp))
        self.fp2_module = FPModule(3, MLP(mlp2_fp))
        self.fp1_module = FPModule(3, MLP(mlp1_fp))
        self.lin1 = nn.Linear(mlp1_fp[-1], 16)
        self.lin2 = nn.Linear(16, self.n_class + 1)
        self.lin2.bias = nn.Parameter(torch.tensor([0.733, 0.266, 0.235, 0.358, 0.500]))  # point_net2.py:97-99
        self.softmax = nn.Softmax(dim=1)
        self.sigmoid = nn.Sigmoid()
        if self.cuda_device is not None:
            self.cuda(self.cuda_device)

    def _init_fields(self, args):
        """Everything of the constructor that is not the architecture (shared with point_net2_3sa.PointNet2ThreeSA); draws nothing
        from the RNG."""
        self.cuda_device = args.cuda
        self.subsample_size = args.subsample_size
        self.n_class = args.n_class
        self.drop = args.drop
        self.n_input_feats = args.n_input_feats - 2  # x and y are not fed to the network (point_net2.py:77)
        self.set_patience_attributes(args)
        self.log_embeddings = args.log_embeddings
        self.last_G_tensor = None
        self._last_flat_grad = None
        self._last_cloud_dev = None
        # additive extension (not a reference flag): "bf16" = bfloat16 operands on the matrix cores (BASELINE.json
        # configs[4]); default "fp32" = the reference's precision
        self.set_mma_dtype(getattr(args, "mma_dtype", "fp32"))
        if self.n_class != 4 or self.n_input_feats not in self.SUPPORTED_FEATS:
            raise ValueError("the HIP kernels cover the reference architecture with n_class=4 and n_input_feats - 2 in {"
                             f"{', '.join(str(f) for f in sorted(self.SUPPORTED_FEATS))}}} point features "
                             f"(got n_class={self.n_class}, n_input_feats={args.n_input_feats})")

    # Point features the kernels are instantiated for (`args.n_input_feats - 2`; model/point_net2.py:77): the reference's eight
    # (z, red, green, blue, nir, intensity, return_num, num_returns) and four (z, intensity, return_num, num_returns: LiDAR that was
    # never colourised).  A four-feature model takes `cloud (B,6,N)` -- or the reference's `(B,10,N)`, whose colour rows 3..6 it
    # never reads (include/strata_hip.h: sn2_pack_rows_feat), so every producer of ten-row clouds serves it as it is.
    SUPPORTED_FEATS = (4, 8)

    # the blocks `mma_dtype = "bf16"` applies to: everything that runs on the matrix cores -- the set-abstraction levels and
    # the dense layers over centroids (SA3, FP3, FP2).  The two per-point layers (FP1 in its source-side form, the head)
    # are VALU streaming kernels bound by HBM, not by arithmetic: they stay fp32.
    BF16_BLOCKS = ("sa1_module.conv.local_nn", "sa2_module.conv.local_nn", "sa3_module.nn", "fp3_module.nn", "fp2_module.nn")
    mma_dtype = "fp32"
    # the level-1 FPS kernel when its pass shares the chip with feature kernels (sn2_fps_waves: 8 = one workgroup of 8 waves per plot)
    fps_waves_shared = int(os.environ.get("SN2_FPS_WAVES_SHARED", "8"))
    # ... and with MANY plots in the pass (more than 32: the parcel loop's 512 per launch = two FPS workgroups per CU) 4 waves per
    # plot where the kernel has that form (plots of at most 16 384 points; larger ones take 8): under that much concurrency the pass
    # itself is shorter with fewer waves (4.1 against 5.1 ms per 512 plots of 10 000 points) and the loop 2.6 % faster
    fps_waves_many = int(os.environ.get("SN2_FPS_WAVES_MANY", "4"))
    geometry_fork = True       # `_geometry`: the three independent chains behind the level-1 FPS on three streams
    # One C-ABI call per pass (executor.py; include/strata_hip.h: sn2_net_geometry / sn2_net_forward / sn2_net_backward) instead of
    # ~25 + ~10 calls issued from Python: same entry points, same descriptors, same order, same bits -- the host time between the
    # launches is what bounded the reference's loop as written (learning/train.py:44-71).  False: the per-call path below (also
    # taken while hip_ops.timing measures single entry points).
    executor = os.environ.get("SN2_EXECUTOR", "1") == "1"
    # True (set by optim.FlatAdam(fold_gradient_images=True) where no exchange sits between backward and update): the backward
    # pass leaves the 32 images of the flat gradient unfolded and the optimiser's kernel folds them (sn2_adam_step_images: one
    # launch less per step); until that step `p.grad` holds image 0 only.
    defer_grad_reduce = False
    _grad_images_pending = None
    geometry_pair_takes_group_cloud = True      # `_geometry_pair(..., cloud2=)`: the input-only pieces once per group of batches
    fuse_eval_head = os.environ.get("SN2_FUSE_EVAL_HEAD", "1") == "1"     # eval: FP1 + head in one kernel (sn2_fp_head_eval)
    # training: SA3, its BatchNorm, the plot max, FP3 and its BatchNorm in one launch (sn2_global_level_forward) instead of five;
    # its workgroups exchange the batch statistics among themselves -- False where other processes share the device
    fuse_global_level = os.environ.get("SN2_FUSE_GLOBAL_LEVEL", "1") == "1"
    # training: `losses.projected_total_loss` hands this model's backward pass the loss gradient as a descriptor and the head
    # backward computes d loss / d coverages and d loss / d proba itself (sn2_head.loss) -- no sn2_projected_loss_backward launch
    fuse_loss_backward = os.environ.get("SN2_FUSE_LOSS_BACKWARD", "1") == "1"
    # additive: a geometry pass that is handed the batch's `cloud` also does the two INPUT-only pieces of the feature pass --
    # the level-0 rows (`sn2_pack_rows`: 12 us of the step's critical path at C2) and, when `p2_diam_pix` is set (to
    # args.diam_pix), the pixel ids of `project_to_plotwise_coverages` (project_to_2d.py:16-22: a function of x, y only; 10 us) --
    # so that a loop which runs its geometry passes ahead (pipeline.TrainPipeline, prefetch_geometry) takes them off the
    # feature pass.  Same kernels, same results.
    p2_diam_pix = None

    def set_mma_dtype(self, dtype: str):
        """"fp32" (default: exact fp32 products, the reference's precision) or "bf16": the dense contractions of
        `BF16_BLOCKS` -- forward, input gradient, weight gradient -- take bfloat16 operands on v_mfma_f32_16x16x32_bf16 /
        16x16x16 with fp32 accumulation; ReLU, BatchNorm, statistics, every arg-max and all position-only kernels stay
        fp32, so the index structures are the same bits in both modes.  A dense block with more rows than
        `hip_ops.fp_rows_small` takes -- FP2 at the reference's default ratio1 = 0.5 on 32 768-point plots -- has no bfloat16
        kernel and runs in fp32 (`hip_ops.fp_desc`)."""
        if dtype not in ("fp32", "bf16"):
            raise ValueError("mma_dtype must be 'fp32' or 'bf16'")
        self.mma_dtype = dtype
        return self

    # ------------------------------------------------------------------------------------------ forward
    def forward(self, cloud_data):
        cloud, xyz = cloud_data["cloud"], cloud_data["xyz"]
        dev = self.lin1.weight.device
        if dev.type != "cuda":
            raise StrataHipError("PointNet2.forward needs a HIP device (args.cuda): the product path has no CPU "
                                 "fallback; the CPU restatement lives in oracle/ and is test infrastructure")
        if cloud.dim() != 3 or cloud.shape[1] not in self._cloud_rows() or xyz.shape != (cloud.shape[0], 3, cloud.shape[2]):
            raise ValueError(f"expected cloud {' or '.join(f'(B,{c},N)' for c in self._cloud_rows())} and xyz (B,3,N), got "
                             f"{tuple(cloud.shape)} and {tuple(xyz.shape)}")
        with torch.cuda.device(dev):
            geo = cloud_data.get("geometry", None) if isinstance(cloud_data, dict) else None
            if geo is None and not cloud.is_cuda and not xyz.is_cuda and self.host_upload_overlap:
                return self._forward_from_host(cloud_data, cloud, dev)
            cloud_d = cloud.to(device=dev, dtype=F32, non_blocking=True).contiguous()
            if geo is not None:
                if getattr(geo, "ready", None) is not None:
                    # position-only kernels already ran (or are running) on the side stream: wait for them here
                    cs = torch.cuda.current_stream()
                    cs.wait_event(geo.ready)
                    for v in geo.__dict__.values():          # allocated on the side stream, consumed on this one
                        for t in (v if isinstance(v, tuple) else (v,)):
                            if isinstance(t, torch.Tensor):
                                t.record_stream(cs)
                # ready is None: persistent buffers (alloc_geometry); the caller orders the streams itself
                xyz_d, fs = geo.xyz, None
            else:
                xyz_d, fs = self._stage_positions(cloud_data, dev)
                self._n_live_at_call = self._stage_live(cloud_data, dev, xyz_d.shape[0])
            self._last_cloud_dev = (cloud, cloud_d)  # lets project_to_plotwise_coverages skip a second H2D copy
            params = self._params()
            self._grad_mode_at_call = torch.is_grad_enabled()
            cov, proba = _PointNet2Fn.apply(self, xyz_d, cloud_d, fs, geo, self._dropout_keep(cloud_data, cloud_d), *params)
        return cov, proba

    # CPU inputs (the reference's calling convention, learning/train.py:46-56): upload `xyz` (6 MB at C2) first through a pinned
    # ring, launch the position-only kernels on it, and let `cloud` (21 MB) follow on a copy stream while they run
    host_upload_overlap = os.environ.get("SN2_HOST_UPLOAD_OVERLAP", "1") == "1"

    def _forward_from_host(self, cloud_data, cloud, dev):
        """`forward` for CPU-resident inputs: same kernels, same results; only the order of uploads and launches differs."""
        ring = ops.pinned_ring(dev)
        cur = torch.cuda.current_stream(dev)
        # the device copy of `cloud` is allocated HERE, on the stream that consumes it, before anything of this forward is
        # launched: whatever used the block before lies in front of `start` on this stream
        cloud_d = torch.empty(cloud.shape, dtype=F32, device=dev)
        start = torch.cuda.Event()
        start.record(cur)
        xyz_d, fs = self._stage_positions(cloud_data, dev, ring=ring)
        # (the inverted tables: whenever a backward pass may follow -- training, or eval mode under autograd)
        g = self._geometry(xyz_d, fs, defer_join=True, inverted=self.training or torch.is_grad_enabled(),     # launched: the device is busy from here on
                           **self._live_kw(self._stage_live(cloud_data, dev, xyz_d.shape[0])))
        up = ops.shared_stream(dev, "upload")
        up.wait_event(start)                                                          # not for the geometry pass: only for the block's past
        ring.upload(cloud, stream=up, dtype=F32, out=cloud_d, consumer=cur)            # host memcpy + DMA beside the geometry pass
        self._last_cloud_dev = (cloud, cloud_d)
        from .project_to_2d import remember_upload
        remember_upload(cloud, cloud_d)              # `project_to_plotwise_coverages(pred, clouds, args)` as the reference calls it
        params = self._params()
        self._grad_mode_at_call = torch.is_grad_enabled()
        return _PointNet2Fn.apply(self, xyz_d, cloud_d, None, g, self._dropout_keep(cloud_data, cloud_d), *params)

    def _cloud_rows(self):
        """The row counts `forward` accepts for `cloud`: F + 2, and for a four-feature model also the reference's ten."""
        F = self.n_input_feats
        return (F + 2,) if F == 8 else (F + 2, 10)

    def _params(self):
        """The module's parameters in `parameters()` order, walked once (the walk was 0.1 ms of host time per forward and per
        backward) and VALIDATED per use: the direct children and every cached leaf's Parameter / buffer objects must still be the
        ones the walk saw -- a swapped `lin2`, `to_empty()`, `load_state_dict(assign=True)` or a Parameter assigned by hand
        rebuild the list (and with it the executor's model struct) instead of routing gradients to stale objects.  (A module
        replaced deeper in the tree, e.g. `fp1_module.nn[0] = ...`, is not seen by the cheap check: call `invalidate_caches()`.)"""
        c = self.__dict__.get("_leafs")
        if c is not None:
            mods = self._modules
            ok = all(mods.get(k) is v for k, v in c[0]) and all(m._parameters.get(n) is p for m, n, p in c[1]) and \
                all(m._buffers.get(n) is b for m, n, b in c[2])
            if ok:
                return self.__dict__["_param_list"]
        self.invalidate_caches()
        ps = list(self.parameters())
        leaf_p, leaf_b = [], []
        for mod in self.modules():
            leaf_p += [(mod, n, p) for n, p in mod._parameters.items() if p is not None]
            leaf_b += [(mod, n, b) for n, b in mod._buffers.items() if b is not None]
        self.__dict__["_param_list"] = ps
        self.__dict__["_leafs"] = (tuple(self._modules.items()), leaf_p, leaf_b)
        return ps

    def invalidate_caches(self):
        """Forget everything derived from the module tree (parameter list, the executor's model struct and plans)."""
        for k in ("_param_list", "_leafs", "_net_ms"):
            self.__dict__.pop(k, None)

    def _apply(self, fn, *a, **kw):          # .to() / .cuda() / .float() / to_empty(): tensors may move or be replaced
        self.invalidate_caches()
        return super()._apply(fn, *a, **kw)

    def load_state_dict(self, *a, **kw):
        self.invalidate_caches()
        return super().load_state_dict(*a, **kw)

    def _use_executor(self):
        return bool(self.executor) and ops._timing is None

    def _net_model(self):
        """The executor's view of this model (executor.ModelStruct), rebuilt when a parameter / buffer object or address or one
        of the settings it carries changed."""
        params = self._params()                       # (validates the module tree, drops `_net_ms` when it changed)
        ms = self.__dict__.get("_net_ms")
        if ms is None or not ms.current(self, MAX_NEIGHBORS):
            ms = self.__dict__["_net_ms"] = X.ModelStruct(self, params, MAX_NEIGHBORS)
        return ms

    def _net_ctx(self):
        c = self.__dict__.get("_net_ctx_obj")
        if c is None:
            c = self.__dict__["_net_ctx_obj"] = X.NetCtx()
        return c

    def _dropout_keep(self, cloud_data, cloud_d):
        """F.dropout(x, p=self.drop, training=self.training) between lin1 and lin2 (model/point_net2.py:142): the (B*N) words
        of kept hidden channels for the head kernels, or None (eval mode, p = 0).  The mask is drawn on the device from
        torch's generator (Bernoulli(1-p) per element, as F.dropout draws it; torch's own CUDA dropout stream is not
        reproducible across devices either); additive extension for parity tests: `cloud_data["dropout_mask"]`, a
        (B*N,16) tensor, non-zero = keep."""
        if not (self.training and self.drop > 0):
            return None
        R = cloud_d.shape[0] * cloud_d.shape[2]
        keep = cloud_data.get("dropout_mask", None) if isinstance(cloud_data, dict) else None
        if keep is None:
            keep = torch.empty(R, 16, dtype=F32, device=cloud_d.device).bernoulli_(max(0.0, 1.0 - float(self.drop)))
        else:
            keep = torch.as_tensor(keep).to(device=cloud_d.device)
            if tuple(keep.shape) != (R, 16):
                raise ValueError(f"dropout_mask must have shape ({R},16)")
        return ops.dropout_mask_words(keep)

    # Keep FP1's d pre-activation rows in the plots' Morton order (sn2_fp.row_perm).  OFF: measured at 16 x 32 768, the source
    # pass's gather did not get faster (45.2 against 46.8 us: neighbouring sources already share an XCD's L2, and the pass is
    # bound by the number of cache lines its gather instructions touch, not by where they come from), while the row pass's
    # permuted stores cost 7.8 us (57.9 against 50.1).  The path stays tested (tests/test_gpu_network.py).
    fp1_morton_rows = os.environ.get("SN2_FP1_MORTON_ROWS", "0") == "1"

    @staticmethod
    def _fp1_source_side(rows):
        """Whether the per-point layer FP1 runs in its source-side form (hip_ops.fp_desc hands out `src_ws`): only that form
        keeps bfloat16 rows (`_act_dtype`) and a permuted d pre-activation buffer (`rank1`)."""
        return bool(ops.SOURCE_SIDE) and ops.fp_source_side(rows, 8)      # (the rule is the same for FP1's 4 or 8 skip columns)

    def _act_dtype(self, rows):
        """Storage type of the three per-point activation buffers (FP1's output h1, the head's gradient dy1, FP1's
        d pre-activation): bfloat16 under `mma_dtype = "bf16"` where the per-point layer takes its source-side form
        (`_fp1_source_side`), else fp32.  These 75 MB buffers are what the per-point kernels stream."""
        return torch.bfloat16 if (self.mma_dtype == "bf16" and self._fp1_source_side(rows)) else F32

    # ------------------------------------------------------------------------------------------ the architecture as data
    # The per-call path below is written ONCE over these, for L = len(sa_levels) ball-query levels (2 in the reference
    # architecture, 3 in point_net2_3sa.PointNet2ThreeSA).  They read the registered submodules in construction order -- the SA
    # levels bottom up, the FP levels top down, as the reference constructs them -- and register nothing.  Handles and saved sets
    # number their attributes by level: idx/pos/ws/nbr/cnt/tot/ord/ext/arg/x/M 1..L, knn/inv/h 1..L+1; the global level is L+1.
    @property
    def sa_levels(self):
        """The ball-query set-abstraction modules in order: (sa1_module, sa2_module, ...)."""
        return tuple(m for m in self._modules.values() if isinstance(m, SAModule))

    @property
    def global_sa(self):
        """The global set-abstraction module: level L+1 (`sa3_module` of the reference architecture)."""
        return next(m for m in self._modules.values() if isinstance(m, GlobalSAModule))

    @property
    def fp_levels(self):
        """The feature-propagation modules from the top (k = 1, out of the global feature) down to `fp1_module`."""
        return tuple(m for m in self._modules.values() if isinstance(m, FPModule))

    def _fp_by_level(self):
        """{j: the FP module that writes level j-1's rows}: j = L+1 (top) .. 1."""
        fps = self.fp_levels
        return dict(zip(range(len(fps), 0, -1), fps))

    def _block_seqs(self):
        """(state-dict prefix, Sequential of blocks) in the order of the BatchNorm side-buffer arena: the SA levels, the global
        level, FP top down to FP1."""
        sa = [(f"sa{l}_module.conv.local_nn", m.conv.local_nn) for l, m in enumerate(self.sa_levels, 1)]
        fp = self._fp_by_level()
        return sa + [(f"sa{len(sa) + 1}_module.nn", self.global_sa.nn)] + [(f"fp{j}_module.nn", m.nn) for j, m in fp.items()]

    def _sizes(self, N):
        """(M1, ..., ML): the sample count of every ball-query level for plots of N points."""
        out = []
        for m in self.sa_levels:
            N = ops.fps_num_samples(N, m.ratio)
            out.append(N)
        return tuple(out)

    def _level_sizes(self, N):
        """[N, M1, ..., ML]: points per plot at level 0 (the input) .. L."""
        return [N, *self._sizes(N)]

    @staticmethod
    def _dims(g, L):
        return (g.B, g.N) + tuple(_at(g, "M", l) for l in range(1, L + 1))

    # ------------------------------------------------------------------------------------------ geometry
    def alloc_geometry(self, B, N, device=None):
        """Persistent result buffers for `_geometry(..., out=)`: what a software-pipelined training loop hands to the
        position-only kernels of the batches in flight (pipeline.TrainPipeline)."""
        dev = torch.device(device if device is not None else self.lin1.weight.device)
        if self._use_executor():
            with torch.cuda.device(dev):
                return X.ArenaGeometry(self._net_model().plan(self, B, N), dev, self)      # one allocation, views on demand
        Ms = self._level_sizes(N)
        L = len(Ms) - 1
        e = lambda *shape, dt=F32: torch.empty(*shape, dtype=dt, device=dev)          # noqa: E731
        g = _Saved()
        g.B, g.N = B, N
        g.totals = torch.zeros(L, dtype=I64, device=dev)
        for l in range(1, L + 1):
            S, M = Ms[l - 1], Ms[l]
            _put(g, "M", l, M)
            _put(g, "idx", l, e(B, M, dt=I32))
            _put(g, "pos", l, e(B, 3, M), "_soa")
            _put(g, "pos", l, e(B * M, 4), "_aos")
            _put(g, "ws", l, e(ops.fps_ws_words(B, S), dt=I32) if ops.fps_fills_ws(B, S, M) else None)
            _put(g, "nbr", l, e(B * M, min(MAX_NEIGHBORS, S), dt=I32))
            _put(g, "cnt", l, e(B * M, dt=I32))
            _put(g, "tot", l, g.totals[l - 1:l])
            _put(g, "ord", l, e(ops.sa_order_len(B, M), dt=I32))
            if l < L:       # level l's count of live samples = level l+1's n_live (hip_ops.fps), when a batch has one
                _put(g, "fps_live", l, e(B, dt=I32))
        # every point's position along the plot's Morton curve (the level-1 FPS leaves it in its workspace): the order FP1's
        # backward keeps its d pre-activation rows in (hip_ops.fp_desc: row_perm)
        g.rank1 = ops.fps_ws_rank(g.ws1, B, N) if (self.fp1_morton_rows and g.ws1 is not None and self._fp1_source_side(B * N)) else None
        _put(g, "pos", L + 1, torch.zeros(B, 3, 1, dtype=F32, device=dev))        # the plots' global feature sits at the origin
        for j in range(L + 1, 0, -1):
            R = B * Ms[j - 1]
            _put(g, "knn", j, (e(R, 3, dt=I32), e(R, 3)))
            _put(g, "inv", j, e(ops.interp_ws_words(B, Ms[j - 1], Ms[j] if j <= L else 1)))
        # nn_ws[k]: the grid workspace of knn{L-k}
        g.nn_ws = tuple(e(ops.three_nn_ws_words(B, Ms[j], Ms[j - 1]), dt=I32) if ops.three_nn_uses_grid(Ms[j], Ms[j - 1]) else None
                        for j in range(L, 0, -1))
        self._alloc_input_only(g, B, N, dev)
        g.ready = None
        return g

    def _alloc_input_only(self, g, B, N, dev):
        """Buffers of the input-only pieces a geometry pass may produce (see `p2_diam_pix`)."""
        g.rows0 = torch.empty(B * N, self.n_input_feats + 4, dtype=F32, device=dev)
        g.has_rows0 = False
        g.p2_pix, g.p2_mm, g.p2_diam_pix = None, None, None
        if self.p2_diam_pix is not None:
            g.p2_pix = torch.empty(B * N, dtype=I32, device=dev)
            g.p2_mm = torch.empty(B, 4, dtype=F32, device=dev)

    def _input_only(self, g, cloud, xyz):
        """The input-only pieces of the feature pass, run with the geometry pass when it is handed the batch's `cloud` (device)."""
        ops.pack_rows(cloud, xyz, out=g.rows0, feats=self.n_input_feats)
        g.has_rows0 = True
        if g.p2_pix is not None and self.p2_diam_pix is not None:
            ops.plot_pixels(cloud, self.p2_diam_pix, out=(g.p2_mm, g.p2_pix))
            g.p2_diam_pix = int(self.p2_diam_pix)

    geometry_takes_n_live = True          # `_geometry(n_live=)` / `_geometry_pair(n_live2=)`: what TrainPipeline asks before passing it

    # ---- the position-only launches of one level / one 3-NN table, as `_geometry`, `_geometry_pair` and `_forward_impl` issue them
    @staticmethod
    def _positions(g, xyz, L):
        """[xyz, pos1_soa, ..., posL_soa, pos{L+1}]: the positions of level 0 .. L+1 (the last: the origin, one per plot)."""
        return [xyz] + [_at(g, "pos", l, "_soa") for l in range(1, L + 1)] + [_at(g, "pos", L + 1)]

    @staticmethod
    def _fps_level(g, pos, l, m, start, n_live=None, waves=0):
        """Level l's m samples of level l-1's points.  -> the live count of its samples (the next level's n_live), or None."""
        live_out = getattr(g, f"fps_live{l}", None) if n_live is not None else None
        ops.fps(pos[l - 1], m, start, out=(_at(g, "idx", l), pos[l], _at(g, "pos", l, "_aos"), _at(g, "ws", l)), waves=waves,
                n_live=n_live, n_live_out=live_out)
        return live_out

    @staticmethod
    def _ball_level(g, pos, l, r, total):
        ops.ball_query(pos[l - 1], pos[l], r, MAX_NEIGHBORS, total, fps_ws=_at(g, "ws", l), out=(_at(g, "nbr", l), _at(g, "cnt", l)))

    @staticmethod
    def _nn_table(g, pos, j, k, inverted=False):
        """knn{j}: for every point of level j-1 its k nearest of level j (FP module j's k: 1 from the plot's global feature).
        inverted: `_search_order` follows (the grid search then leaves its rows in its own order too)."""
        L = len(pos) - 2
        ops.three_nn(pos[j], pos[j - 1], k, out=_at(g, "knn", j), **({"ws": g.nn_ws[L - j], "sorted_copy": inverted} if j <= L else {}))

    @staticmethod
    def _search_order(g, Ms, j):
        """The order (and the sorted rows) that knn{j}'s search left in its workspace, as keywords of `ops.interp_index*`; nothing
        where the full scan ran.  Only right behind `_nn_table(..., inverted=True)` of the same level, on the same stream: the
        next search with that workspace overwrites them."""
        L = len(Ms) - 1
        if j > L or g.nn_ws is None or g.nn_ws[L - j] is None or not ops.three_nn_uses_grid(Ms[j], Ms[j - 1]):
            return {}
        order, si, sw = ops.three_nn_order(g.nn_ws[L - j], g.B, Ms[j], Ms[j - 1])
        return {"row_order": order, "sorted_table": (si, sw)}

    @staticmethod
    def _inverted_table(g, Ms, j, ordered=False):
        """inv{j}: the inverted index of knn{j} that the backward pass gathers through.  ordered: in the search's order
        (`_search_order`: the geometry pass itself; a late build takes the rows' own order)."""
        B, L = g.B, len(Ms) - 1
        kw = {"src_pos": g.pos1_aos, "row_perm": getattr(g, "rank1", None)} if j == 1 else {}
        if ordered:
            kw.update(PointNet2._search_order(g, Ms, j))
        ops.interp_index(_at(g, "knn", j), B, Ms[j - 1], Ms[j] if j <= L else 1, out=_at(g, "inv", j), **kw)

    def _geometry(self, xyz, fps_start, out=None, fork=None, shared=False, defer_join=False, inverted=True, cloud=None, n_live=None):
        """Everything that depends on the point POSITIONS only (no weights, no features): the FPS levels, their ball
        queries, the 3-NN tables.  In the reference these are the torch_cluster calls inside SAModule / FPModule
        (point_net2.py:22-25, 63).  Because they need no parameters they can run ahead of the feature kernels: see
        `prefetch_geometry`.  `out`: buffers from `alloc_geometry` to write into (no allocation, same addresses every
        time: what a hipGraph-replayed feature pass needs).
        `fork` (default `self.geometry_fork`): after the level-1 FPS the three independent chains -- (a) ball query 1 +
        its work items, (b) the levels above (FPS, ball query, work items), every 3-NN table but the per-point one and their
        inverted indices, (c) the per-point 3-NN table + its inverted index -- run on three streams and join before returning
        (captured into a hipGraph they become parallel branches): the level-2 FPS is 16 workgroups for 0.15 ms, chains (a) and
        (c) fill the chip beside it.
        `defer_join` (with `fork`): return without joining; `g._join = (stream of chain b, stream of chain c)` for the caller
        to wait on where it first needs them (`_forward_impl`: the first set-abstraction level starts beside chain b).
        `inverted=False`: skip the inverted 3-NN tables and the message totals (only the backward pass reads them: an eval-mode
        forward does not need them -- a tenth of the geometry pass of the parcel loop); `g.has_inverted` records it.
        `shared`: the pass runs beside other batches' feature kernels (a pipelined loop, `prefetch_geometry`): the level-1
        FPS takes `fps_waves_shared` waves per plot (include/strata_hip.h: sn2_fps_waves).
        `cloud` (B,F+2,N) on the device ((B,10,N) too for F = 4): also run the input-only pieces of the feature pass here (`_input_only`).
        `n_live` (B) int32 on the device or None: the plots' live prefixes (`cloud_data["n_live"]`; include/strata_hip.h:
        sn2_fps_live) -- level 1 samples over them and counts its samples up to a maximum of 0, the next level takes that count.
        Same tables with or without it."""
        if self._use_executor():
            return X.geometry(self, self._net_model(), xyz, fps_start, out=out, fork=fork, shared=shared, defer_join=defer_join,
                              inverted=inverted, cloud=cloud, n_live=n_live)
        dev = xyz.device
        B, _, N = xyz.shape
        Ms = self._level_sizes(N)
        L = len(Ms) - 1
        g = out if out is not None else self.alloc_geometry(B, N, dev)
        if self._dims(g, L) != (B, *Ms):
            raise ValueError("geometry buffers do not match this batch")
        g.xyz = xyz
        fork = self.geometry_fork if fork is None else fork
        cur = torch.cuda.current_stream(dev)
        pos, sa, fp = self._positions(g, xyz, L), self.sa_levels, self._fp_by_level()
        # (the message totals: only where a backward may follow -- `inverted`; sn2_net_geometry)
        total = (lambda l: _at(g, "tot", l)) if inverted else (lambda l: False)
        live = self._fps_level(g, pos, 1, Ms[1], fps_start[0], n_live,
                               waves=(self.fps_waves_many if B > 32 else self.fps_waves_shared) if shared else 0)
        if fork:
            sb, sc = ops.shared_stream(dev, "fork_b"), ops.shared_stream(dev, "fork_c")
            sb.wait_stream(cur)
            sc.wait_stream(cur)
        else:
            sb = sc = cur
        with torch.cuda.stream(sb):                                        # (b) the chain of the levels above
            for l in range(2, L + 1):
                live = self._fps_level(g, pos, l, Ms[l], fps_start[l - 1], live)
                self._ball_level(g, pos, l, sa[l - 1].r, total(l))
                ops.sa_order(_at(g, "cnt", l), B, Ms[l], out=_at(g, "ord", l))
            for j in range(L + 1, 1, -1):
                self._nn_table(g, pos, j, fp[j].k, inverted)
            # the inverted 3-NN tables the backward pass gathers through: positions only, so they belong here
            if inverted:
                for j in range(L + 1, 1, -1):
                    self._inverted_table(g, Ms, j, ordered=True)
        with torch.cuda.stream(sc):                                        # (c) the per-point table
            self._nn_table(g, pos, 1, fp[1].k, inverted)
            if inverted:
                self._inverted_table(g, Ms, 1, ordered=True)
        g.has_inverted = bool(inverted)
        g.has_rows0 = False
        if cloud is not None:
            self._input_only(g, cloud, xyz)
        # (a)
        self._ball_level(g, pos, 1, sa[0].r, total(1))
        ops.sa_order(g.cnt1, B, Ms[1], out=g.ord1)
        g._join = None
        if fork and defer_join:
            g._join = (sb, sc)
        elif fork:
            cur.wait_stream(sb)
            cur.wait_stream(sc)
        return g

    def alloc_geometry_pair(self, B, N, device=None, group=2):
        """Buffers for `_geometry_pair`: the position-only kernels of `group` (2, or more) batches of B plots launched together
        (FPS is one workgroup per plot and M sequential rounds: several batches take as long as one), plus the per-batch views
        the feature passes read.  -> (combined buffers, (geometry of the first batch, of the second, ...))."""
        dev = torch.device(device if device is not None else self.lin1.weight.device)
        Ms = self._level_sizes(N)
        L = len(Ms) - 1
        gp = self.alloc_geometry(group * B, N, dev)
        e = lambda *shape, dt=F32: torch.empty(*shape, dtype=dt, device=dev)          # noqa: E731
        # the per-batch products -- message totals, SA work items, inverted 3-NN indices -- of all `group` batches live in ONE
        # strided buffer each, so that the pass builds them with one (set of) launch(es) per kind instead of one per batch
        # (hip_ops.*_group; round 5: 18 small launches per pass of eight batches instead of 144); a batch's slice is an ordinary
        # per-batch table
        up4 = lambda n: (n + 3) // 4 * 4          # noqa: E731
        inv_words = {j: ops.interp_ws_words(B, Ms[j - 1], Ms[j] if j <= L else 1) for j in range(L + 1, 0, -1)}
        grp = _Saved()
        grp.G = group
        grp.so = {l: ops.sa_order_len(B, Ms[l]) for l in range(1, L + 1)}          # strides of the batches' tables in ord / inv
        grp.si = {j: up4(w) for j, w in inv_words.items()}
        grp.ord = {l: e(group * n, dt=I32) for l, n in grp.so.items()}
        grp.inv = {j: e(group * n) for j, n in grp.si.items()}
        grp.totals = torch.zeros(group, L, dtype=I64, device=dev)
        gp._grp = grp
        halves = []
        for h in range(group):
            g = _Saved()
            g.B, g.N = B, N
            pl = slice(h * B, (h + 1) * B)
            rows = [slice(h * B * M, (h + 1) * B * M) for M in Ms]          # batch h's rows at level 0 .. L
            g.totals = grp.totals[h]
            for l in range(1, L + 1):
                _put(g, "M", l, Ms[l])
                _put(g, "idx", l, _at(gp, "idx", l)[pl])
                _put(g, "pos", l, _at(gp, "pos", l, "_soa")[pl], "_soa")
                for stem, tail in (("pos", "_aos"), ("nbr", ""), ("cnt", "")):
                    _put(g, stem, l, _at(gp, stem, l, tail)[rows[l]], tail)
                _put(g, "tot", l, grp.totals[h, l - 1:l])
                _put(g, "ord", l, grp.ord[l][h * grp.so[l]:(h + 1) * grp.so[l]])
                _put(g, "ws", l, None)
            for j in range(L + 1, 0, -1):
                idx, w = _at(gp, "knn", j)
                _put(g, "knn", j, (idx[rows[j - 1]], w[rows[j - 1]]))
                _put(g, "inv", j, grp.inv[j][h * grp.si[j]:h * grp.si[j] + inv_words[j]])
            g.nn_ws = None
            g.rank1 = gp.rank1[rows[0]] if (gp.rank1 is not None and self._fp1_source_side(B * N)) else None
            # the input-only pieces of the feature pass: the batch's slices of the GROUP's buffers (one launch each for the whole
            # group when the pass is handed the group's clouds in one tensor: `_geometry_pair(..., cloud2=)`)
            g.rows0, g.has_rows0 = gp.rows0[rows[0]], False
            g.p2_pix = gp.p2_pix[rows[0]] if gp.p2_pix is not None else None
            g.p2_mm = gp.p2_mm[pl] if gp.p2_mm is not None else None
            g.p2_diam_pix = None
            g.ready = None
            halves.append(g)
        return gp, tuple(halves)

    def _geometry_pair(self, xyz2, fps_start2, gp, halves, clouds=None, cloud2=None, n_live2=None):
        """`_geometry` for len(halves) batches at once: xyz2 (G B,3,N), fps_start2 (L,G B); FPS, ball queries and 3-NN tables
        run on all plots in one launch each (into `gp`), the per-batch products (message totals, SA work items, inverted 3-NN
        indices) per batch.  Same tables as G `_geometry` calls.  clouds: the G batches' (B,10,N) device tensors -> also the
        input-only pieces of their feature passes (`_input_only`), batch by batch; cloud2 (G B,10,N): the same for the whole group
        in one launch each (the batches' clouds live in one tensor: what TrainPipeline arranges).  n_live2 (G B) int32 or None:
        the plots' live prefixes, as `_geometry`'s n_live."""
        B2, _, N = xyz2.shape
        G = len(halves)
        B = B2 // G
        Ms = self._level_sizes(N)
        L = len(Ms) - 1
        if (gp.B, gp.N) != (B2, N):
            raise ValueError("geometry buffers do not match this batch pair")
        pos, sa, fp = self._positions(gp, xyz2, L), self.sa_levels, self._fp_by_level()
        live = n_live2
        for l in range(1, L + 1):
            # 8 waves per plot at level 1: this pass runs beside other batches' feature kernels (sn2_fps_waves)
            live = self._fps_level(gp, pos, l, Ms[l], fps_start2[l - 1], live, waves=self.fps_waves_shared if l == 1 else 0)
            # (no message total of the GROUP: the batches' totals come from count_sum_group below)
            self._ball_level(gp, pos, l, sa[l - 1].r, False)
        # (the per-point table's targets in the FPS pass's existing Morton order -- `dst_fps_ws=gp.ws1`, no target sort -- made the
        # pipelined step SLOWER, 0.739 against 0.718 ms: the search's query boxes grow more than the sort costs; round 5)
        for j in range(L + 1, 0, -1):
            self._nn_table(gp, pos, j, fp[j].k, True)
        grp = gp._grp
        tot_flat = grp.totals.view(-1)                       # (G,L): [h][l-1] = level-l messages of batch h
        for l in range(1, L + 1):
            ops.count_sum_group(_at(gp, "cnt", l), G, B * Ms[l], tot_flat[l - 1:], L)
        for l in range(1, L + 1):
            ops.sa_order_group(_at(gp, "cnt", l), G, B, Ms[l], grp.ord[l], grp.so[l])
        rank = gp.rank1 if halves[0].rank1 is not None else None
        for j in range(L + 1, 0, -1):
            kw = {"src_pos": gp.pos1_aos, "row_perm": rank} if j == 1 else {}
            kw.update(self._search_order(gp, Ms, j))        # (every level has a workspace of its own: all still hold their orders)
            ops.interp_index_group(_at(gp, "knn", j), G, B, Ms[j - 1], Ms[j] if j <= L else 1, grp.inv[j], grp.si[j], **kw)
        if cloud2 is not None:
            self._input_only(gp, cloud2, xyz2)                    # one launch each over the whole group
        for h, g in enumerate(halves):
            g.xyz = xyz2[h * B:(h + 1) * B]
            g.has_rows0 = cloud2 is not None
            g.p2_diam_pix = gp.p2_diam_pix if cloud2 is not None else None
            g.has_inverted = True
            if clouds is not None and cloud2 is None:
                self._input_only(g, clouds[h], g.xyz)
        return halves

    def prefetch_geometry(self, cloud_data, lane: int = 0):
        """Run the position-only kernels of a batch on a side stream, ahead of time (typically for batch k+1 while
        batch k is in its backward pass: the FPS rounds are sequential and occupy one CU per plot, the feature kernels
        fill the rest of the chip).  Returns a handle to put into `cloud_data["geometry"]` for the forward call.
        `lane` selects one of several side streams, so that the passes of several batches can be in flight at once."""
        dev = self.lin1.weight.device
        if dev.type != "cuda":
            raise StrataHipError("prefetch_geometry needs a HIP device")
        with torch.cuda.device(dev):
            xyz_d, fs = self._stage_positions(cloud_data, dev)
            side = ops.shared_stream(dev, f"side{lane}")
            side.wait_stream(torch.cuda.current_stream())
            # staged on the current stream, read by kernels of the side stream long after this function has returned:
            # without this the allocator may hand the start indices' memory to the next forward while FPS level 2 still
            # has to read them
            xyz_d.record_stream(side)
            fs.record_stream(side)
            nl = self._stage_live(cloud_data, dev, xyz_d.shape[0])
            if nl is not None:
                nl.record_stream(side)
            with torch.cuda.stream(side):
                # one stream per pass: several passes are in flight on their own lanes already, and a fork inside each
                # (three more streams + their events) cost the parcel loop 18 % (33 300 -> 27 100 plots/s)
                cl = cloud_data.get("cloud", None) if isinstance(cloud_data, dict) else None
                cl = cl if (isinstance(cl, torch.Tensor) and cl.is_cuda and cl.dtype == F32 and cl.is_contiguous()) else None
                g = self._geometry(xyz_d, fs, shared=True, fork=False, inverted=self.training, cloud=cl, **self._live_kw(nl))
                g.fps_start = fs
                g.ready = torch.cuda.Event()
                g.ready.record(side)
            g.stream = side
        return g

    def _stage_positions(self, cloud_data, dev, ring=None):
        xyz = cloud_data["xyz"]
        if ring is not None and not xyz.is_cuda:
            xyz_d = ring.upload(xyz, dtype=F32)
        else:
            xyz_d = xyz.to(device=dev, dtype=F32, non_blocking=True).contiguous()
        B, _, N = xyz_d.shape
        Ms = self._level_sizes(N)
        L = len(Ms) - 1
        fs = cloud_data.get("fps_start", None) if isinstance(cloud_data, dict) else None
        if fs is None:
            # reference behaviour: an independent random start per plot and per FPS call
            fs = torch.stack([torch.randint(0, S, (B,)) for S in Ms[:L]])
        fs = torch.as_tensor(fs).to(device=dev, dtype=I32, non_blocking=True).contiguous()
        if fs.shape != (L, B):
            raise ValueError(f"fps_start must have shape ({L},{B})")
        return xyz_d, fs

    def _stage_live(self, cloud_data, dev, B):
        """`cloud_data["n_live"]` (B) on the device as int32, or None: the additive key of the module docstring (a host tensor is
        uploaded with the batch)."""
        nl = cloud_data.get("n_live", None) if isinstance(cloud_data, dict) else None
        if nl is None or not self.geometry_takes_n_live:         # (a subclass with its own geometry pass ignores the key)
            return None
        nl = torch.as_tensor(nl).to(device=dev, dtype=I32, non_blocking=True).contiguous()
        if nl.shape != (B,):
            raise ValueError(f"n_live must have shape ({B},)")
        return nl

    @staticmethod
    def _live_kw(n_live):
        return {} if n_live is None else {"n_live": n_live}

    def _forward_impl(self, xyz, cloud, fps_start, training, geo=None, drop_keep=None, need_grad=True, n_live=None):
        if self._use_executor():
            cov, proba, s = X.forward(self, self._net_model(), xyz, cloud, fps_start, training, geo, drop_keep, need_grad=need_grad,
                                      n_live=n_live)
            if self.log_embeddings:
                self.last_G_tensor = s.x3
            return cov, proba, s
        dev = xyz.device
        B, _, N = xyz.shape
        Ms = self._level_sizes(N)
        L = len(Ms) - 1
        G = L + 1                                # the global level
        cur_stream = torch.cuda.current_stream(dev)
        # eval mode with gradients wanted: everything a training forward keeps, on the running statistics (SN2_BN_FROZEN_KEEP)
        frozen = (not training) and bool(need_grad)
        keep = bool(training) or frozen
        mode = 1 if training else (BN_FROZEN_KEEP if frozen else 0)
        rows0, packed = None, None
        if geo is not None and getattr(geo, "has_rows0", False) and geo.rows0.shape[0] == B * N:
            rows0 = geo.rows0                    # packed by the geometry pass (`_input_only`)
        if geo is None:
            if self.geometry_fork:
                # the row packing needs the inputs only: beside the level-1 FPS (16 workgroups) instead of behind it
                rows0 = torch.empty(B * N, self.n_input_feats + 4, dtype=F32, device=dev)
                pack_stream = ops.shared_stream(dev, "pack")
                pack_stream.wait_stream(cur_stream)
                with torch.cuda.stream(pack_stream):
                    ops.pack_rows(cloud, xyz, out=rows0, feats=self.n_input_feats)
                    packed = torch.cuda.Event()
                    packed.record(pack_stream)
            geo = self._geometry(xyz, fps_start, defer_join=True, inverted=keep, n_live=n_live)
        elif self._dims(geo, L) != (B, *Ms):
            raise ValueError("prefetched geometry does not match this batch")
        join = getattr(geo, "_join", None)
        geo._join = None
        if join == "ctx":
            raise StrataHipError("a geometry pass launched by the executor with a deferred join must be consumed by the executor")
        if keep and not getattr(geo, "has_inverted", True):
            # tables prefetched in eval mode, forward in training mode: the backward pass needs the inverted indices -- of 3-NN
            # tables that a pass with a deferred join is still writing on its side streams (round 5: joined here first; at the
            # metric's size the indices were built from tables half written)
            if join is not None:
                cur_stream.wait_stream(join[0])
                cur_stream.wait_stream(join[1])
                join = None
            for l in range(1, L + 1):          # (the message totals an eval-mode geometry pass did not make)
                ops.count_sum(_at(geo, "cnt", l), _at(geo, "tot", l))
            for j in range(G, 0, -1):
                self._inverted_table(geo, Ms, j)
            geo.has_inverted = True
        s = _Saved()
        s.__dict__.update({k: v for k, v in geo.__dict__.items()
                           if k not in ("ready", "stream", "totals", "nn_ws", "fps_start", "_join", "has_rows0")
                           and not k.startswith(("ws", "fps_live"))})
        s.xyz = xyz
        # per-forward arenas for the BN side buffers of all blocks: a,c,mean,invstd and the per-workgroup statistics
        # slots (written before they are read: no zero fill)
        seqs = self._block_seqs()
        width = sum(blk[0].out_features for _, seq in seqs for blk in seq)
        aux = torch.empty(4 * width, dtype=F32, device=dev)
        stats = torch.empty(STAT_SLOTS * 2 * width, dtype=F32, device=dev)
        cur = [0, 0]
        blocks = [_blocks_of(seq, aux, stats, cur, self.mma_dtype == "bf16" and prefix in self.BF16_BLOCKS) for prefix, seq in seqs]
        # b_sa[l]: the blocks of ball-query level l; b_glob: the global level's block; b_fp[j]: FP level j's, j = L+1 .. 1
        s.b_sa = dict(enumerate(blocks[:L], 1))
        s.b_glob = blocks[L][0]
        s.b_fp = dict(zip(range(G, 0, -1), (b[0] for b in blocks[G:])))
        s.blocks = [bb for b in blocks for bb in b]
        s.aux, s.stats = aux, stats
        for bb in s.blocks:
            bb.frozen = frozen
        e = lambda *shape, dt=F32: torch.empty(*shape, dtype=dt, device=dev)          # noqa: E731

        # ---- level 0 rows: [F features | x y z 0]
        if packed is not None:
            cur_stream.wait_event(packed)
            s.rows0 = rows0
        elif rows0 is not None:
            s.rows0 = rows0
        else:
            s.rows0 = ops.pack_rows(cloud, xyz, feats=self.n_input_feats)
        # ---- SA1 .. SAL: gather + MLP + BN + max over the ball-query lists        (point_net2.py:131-132, 21-29)
        for l in range(1, L + 1):
            R, C = B * Ms[l], s.b_sa[l][-1].cout
            _put(s, "ext", l, e(R, C))
            _put(s, "arg", l, e(R, C, dt=I32))
            _put(s, "x", l, e(R, C))
            ops.sa_forward(self._sa_desc(s, l), mode)
            if l == 1 and join is not None:
                cur_stream.wait_stream(join[0])      # chain b of the forked geometry pass: the tables of the levels above, small 3-NN tables
        # ---- the global level: MLP on cat[x_L, pos_L] -> per-plot max             (:133, 37-42)
        R, C = B * Ms[L], s.b_glob.cout
        _put(s, "h_sa", G, e(R, _pad4(C)))
        _put(s, "h", G, e(R, _pad4(s.b_fp[G].cout)))
        if training and self.fuse_global_level and ops.global_level_forward_fused(B, s.b_glob, s.b_fp[G]):
            # ... and its max, the top FP level (k=1 from the plot's global feature) and both BatchNorms: one launch  (:133-137)
            _put(s, "x", G, e(B, C))
            _put(s, "arg", G, e(B, C, dt=I32))
            ops.global_level_forward(self._global_sa_desc(s), self._fp_desc(s, G), _at(s, "x", G), _at(s, "arg", G), owner=self)
        else:
            ops.fp_forward(self._global_sa_desc(s), mode)
            x, arg = ops.plot_max_forward(_at(s, "h_sa", G), s.b_glob.a, s.b_glob.c, B, Ms[L], C)
            _put(s, "x", G, x)
            _put(s, "arg", G, arg)
            # ---- FP from the top (k=1 from the plot's global feature at the origin) down (k=3)   (:137-139, 62-67)
            ops.fp_forward(self._fp_desc(s, G), mode)
        if self.log_embeddings:
            self.last_G_tensor = _at(s, "x", G)
        for j in range(L, 1, -1):
            _put(s, "h", j, e(B * Ms[j - 1], _pad4(s.b_fp[j].cout)))
            ops.fp_forward(self._fp_desc(s, j), mode)
        if join is not None:
            cur_stream.wait_stream(join[1])      # chain c: the per-point 3-NN table and its inverted index
        cov, proba = e(B * N, 4), e(B * N, 4)
        s.drop_keep = drop_keep
        b1 = s.b_fp[1]
        if not keep and self.fuse_eval_head and self._act_dtype(B * N) == F32 and ops.SOURCE_SIDE:
            # EVAL: FP1 and the head (:139-151) in one pass, the (B*N,36) rows of h1 never reach memory (nothing is kept for a backward)
            s.h1 = None
            ops.fp_head_eval(self._fp_desc(s, 1, force_src_ws=True),
                             ops.head_desc(None, b1.a, b1.c, self.lin1, self.lin2, cov, proba, rows=B * N))
            return cov, proba, s
        s.h1 = torch.empty(B * N, _pad4(b1.cout), dtype=self._act_dtype(B * N), device=dev)
        ops.fp_forward(self._fp_desc(s, 1), mode)
        # ---- head                                                                  (:141-151)
        ops.head_forward(ops.head_desc(s.h1, b1.a, b1.c, self.lin1, self.lin2, cov, proba, drop_mask=drop_keep, drop_p=self.drop))
        return cov, proba, s

    # ---- descriptors (shared by forward and backward; gradient views are attached for the backward call); channel widths are the
    # blocks' own (Linear.in_features / out_features)
    def _sa_desc(self, s, l, dout=None, dfeat=None, g=False, bwd_ws=None):
        """Ball-query level l (1..L): its sources are the level-0 rows (l = 1) or level l-1's features and positions."""
        blocks = s.b_sa[l]
        cf = blocks[0].cin - 3
        if l == 1:
            feat, spos, S = s.rows0[:, 0:cf], s.rows0[:, cf:cf + 4], s.N
        else:
            feat, spos, S = _at(s, "x", l - 1), _at(s, "pos", l - 1, "_aos"), _at(s, "M", l - 1)
        return ops.sa_desc(blocks, feat, cf, spos, _at(s, "pos", l, "_aos"), _at(s, "nbr", l), _at(s, "cnt", l), _at(s, "tot", l), s.B, S,
                           _at(s, "M", l), _at(s, "ext", l), _at(s, "arg", l), _at(s, "x", l), dout=dout, dfeat=dfeat, with_grads=g,
                           order=getattr(s, f"ord{l}", None), bwd_ws=bwd_ws)

    def _global_sa_desc(self, s, **kw):
        """The global level (L+1): a dense block over cat[x_L, pos_L]; its per-plot max is a launch of its own."""
        L = len(s.b_sa)
        M = _at(s, "M", L)
        return ops.fp_desc(s.b_glob, s.B, M, M, s.b_glob.cin - 3, 3, _at(s, "x", L), _at(s, "h_sa", L + 1), skip=_at(s, "pos", L, "_aos"), **kw)

    def _fp_desc(self, s, j, **kw):
        """FP level j (L+1 = the top .. 1): level j's features (the plot's global feature at the top, else FP level j+1's output
        behind its BatchNorm affine) interpolated through knn{j} onto level j-1's rows, beside that level's own features."""
        L, blk = len(s.b_sa), s.b_fp[j]
        if j == L + 1:
            src, S, ca, affine = _at(s, "x", j), 1, s.b_glob.cout, None
        else:
            up = s.b_fp[j + 1]
            src, S, ca, affine = _at(s, "h", j + 1), _at(s, "M", j), up.cout, (up.a, up.c)
        if j == 1:
            R, skip = s.N, s.rows0[:, 0:blk.cin - ca]
            kw["row_perm"] = getattr(s, "rank1", None)
        else:
            R, skip = _at(s, "M", j - 1), _at(s, "x", j - 1)
        return ops.fp_desc(blk, s.B, R, S, ca, blk.cin - ca, src, _at(s, "h", j), src_affine=affine, knn=_at(s, "knn", j), skip=skip, **kw)

    # ------------------------------------------------------------------------------------------ backward
    def _backward_impl(self, s, dcov, dproba, loss=None):
        """loss: a `hip_ops.loss_grad_desc` in place of both gradients (the fused route of `losses.projected_total_loss`)"""
        if isinstance(s, X.NetSaved):
            return X.backward(self, s, dcov, dproba, loss=loss)
        dev = s.xyz.device
        B, N, L = s.B, s.N, len(s.b_sa)
        G = L + 1
        Ms = [N] + [_at(s, "M", l) for l in range(1, G)]
        params = self._params()
        # one zero-filled arena: flat parameter gradient + every accumulate-into buffer of the backward chain --
        # dy{j}: d (FP level j's output), dx{l}: d x{l}, dy_sa{L+1}: d (the global level's rows)
        shapes = OrderedDict((f"dy{j}", (B * Ms[j - 1], _pad4(s.b_fp[j].cout))) for j in range(2, G + 1))
        shapes.update((f"dx{l}", (B * Ms[l], s.b_sa[l][-1].cout)) for l in range(1, G))
        shapes[f"dx{G}"] = (B, s.b_glob.cout)
        shapes[f"dy_sa{G}"] = (B * Ms[L], _pad4(s.b_glob.cout))
        sizes = OrderedDict((k, r * c) for k, (r, c) in shapes.items())
        sizes["sa1_ws"] = ops.SA_BWD_WS_WORDS
        flat, buf, views, images, arena = self._grad_arena(params, sizes, dev)
        dy = {j: buf[f"dy{j}"].view(shapes[f"dy{j}"]) for j in range(2, G + 1)}
        dx = {l: buf[f"dx{l}"].view(shapes[f"dx{l}"]) for l in range(1, G + 1)}
        for bb in s.blocks:
            bb.grads = (views[id(bb.lin.weight)], views[id(bb.lin.bias)], views[id(bb.bn.weight)], views[id(bb.bn.bias)])
            bb.grad_images = images
        dcov = None if dcov is None else dcov.contiguous()
        dproba = None if dproba is None else dproba.contiguous()
        e = lambda *shape, dt=F32: torch.empty(*shape, dtype=dt, device=dev)          # noqa: E731
        bn_ok = e(L + 2, dt=I32)      # per BatchNorm: did the shortcut apply (else the same kernel's row pass)

        def bn_sums(fn, d, blk, k):
            """The gradients of `blk`'s BatchNorm from the weight gradients of the layer `d` that consumes its output."""
            fn(d, blk.bn.weight.detach(), blk.bn.bias.detach(), blk.aux[2], blk.aux[3], views[id(blk.bn.weight)], views[id(blk.bn.bias)],
               bn_ok[k:k + 1])

        # head
        b1 = s.b_fp[1]
        dy[1] = e(B * N, _pad4(b1.cout), dt=s.h1.dtype)
        hg = (views[id(self.lin1.weight)], views[id(self.lin1.bias)], views[id(self.lin2.weight)], views[id(self.lin2.bias)])
        hd = ops.head_desc(s.h1, b1.a, b1.c, self.lin1, self.lin2, dcov=dcov, dproba=dproba, dy=dy[1], grads=hg,
                           grad_images=images, drop_mask=getattr(s, "drop_keep", None), drop_p=self.drop, loss=loss)
        ops.head_backward(hd)
        # FP1's BatchNorm gradients fall out of lin1's (hip_ops.head_bn_sums): no extra pass over the B*N rows
        bn_sums(ops.head_bn_sums, hd, b1, 0)
        # FP1 .. FPL: FP level j -> d (FP level j+1's output) and d x{j-1}; FP level j+1's BatchNorm feeds level j's
        # interpolation: its gradients from level j's dW, db
        for j in range(1, G):
            blk, ca = s.b_fp[j], s.b_fp[j + 1].cout
            du = e(B * Ms[j - 1], max(ca, _pad4(blk.cout)), dt=dy[j].dtype)
            d = self._fp_desc(s, j, dy=dy[j], dsrc=dy[j + 1], du_scratch=du, with_grads=True, interp_index=_at(s, "inv", j),
                              bn_sums_done=bn_ok[j - 1:j], **({"dskip": dx[j - 1]} if j > 1 else {}))
            ops.fp_backward(d)
            if j < L:
                bn_sums(ops.fp_bn_sums, d, s.b_fp[j + 1], j)
        top, gb = s.b_fp[G], s.b_glob
        if self.fuse_global_level and ops.global_level_backward_fused(B, Ms[L], getattr(top, "frozen", False), gb, top):
            # the top FP level's BatchNorm sums, that level, the pool under it, the global level's BatchNorm sums and the global
            # level in one launch
            ops.global_level_backward(self._global_sa_desc(s, dsrc=dx[L], with_grads=True),
                                      self._fp_desc(s, G, dy=dy[G], dsrc=dx[G], dskip=dx[L], with_grads=True), _at(s, "arg", G), owner=self)
        else:
            bn_sums(ops.fp_bn_sums, d, top, L)
            # top FP level -> d x_L and the per-row gradients of its interpolated part (left in du: scatter_ready = -1); then the
            # pool under it in one launch (hip_ops.global_pool_backward): d x{L+1}, its routing to the global level's rows that
            # attained the maximum, and that level's BatchNorm sums over those B x C entries
            du = e(B * Ms[L], max(gb.cout, _pad4(top.cout)))
            ops.fp_backward(self._fp_desc(s, G, dy=dy[G], dsrc=dx[G], dskip=dx[L], du_scratch=du, with_grads=True,
                                          interp_index=_at(s, "inv", G), bn_sums_done=bn_ok[L:L + 1], gather=False))
            dy_sa = buf[f"dy_sa{G}"].view(shapes[f"dy_sa{G}"])
            ops.global_pool_backward(du, _at(s, "arg", G), _at(s, "h_sa", G), gb.aux[2], gb.aux[3], B, Ms[L], dx[G], dy_sa,
                                     views[id(gb.bn.weight)], views[id(gb.bn.bias)])
            ops.fp_backward(self._global_sa_desc(s, dy=dy_sa, dsrc=dx[L], with_grads=True, bn_sums_done=bn_ok[L + 1:L + 2]))
        # SAL -> d x{L-1} ; ... ; SA1
        for l in range(L, 1, -1):
            ops.sa_backward(self._sa_desc(s, l, dout=dx[l], dfeat=dx[l - 1], g=True))
        ops.sa_backward(self._sa_desc(s, 1, dout=dx[1], g=True, bwd_ws=buf["sa1_ws"]))      # (both blocks in one message pass)
        if getattr(self, "defer_grad_reduce", False):
            self._grad_images_pending = (arena,) + tuple(images)       # FlatAdam folds the images inside its own kernel
        else:
            ops.grad_reduce(arena, flat.numel(), images)      # the images of (dW, db) -> image 0 = `flat`
            self._grad_images_pending = None
        s.flat_grad = flat
        self._last_flat_grad = flat
        return [views[id(p)] for p in params]

    @staticmethod
    def _grad_arena(params, sizes, dev):
        """One zero-filled arena per backward: the images of the flat parameter gradient (hip_ops.grad_images_alloc) and
        every accumulate-into buffer of the backward chain.  -> (flat = image 0, buffers, per-parameter views of image
        0, (replicas, stride), arena)."""
        poffs, n_flat = ops.flat_layout(params)
        offs, tot = {}, 0
        for k, n in sizes.items():
            offs[k] = tot
            tot += (n + 3) // 4 * 4
        arena, flat, images, extra = ops.grad_images_alloc(n_flat, dev, tot)
        buf = {k: extra[offs[k]:offs[k] + n] for k, n in sizes.items()}
        views = {id(p): flat[o:o + p.numel()].view(p.shape) for p, o in zip(params, poffs)}
        return flat, buf, views, images, arena

    # ------------------------------------------------------------------------------------------ layout helpers
    @staticmethod
    def get_long_form(data):
        """(B,f,N) -> (B*N,f), plot-major (point_net2.py:155-158)."""
        B, f, N = data.shape
        return data.permute(1, 0, 2).reshape(f, B * N).transpose(1, 0)

    def get_batch_format(self, data):
        """(B*N,f) -> (B,f,N) (point_net2.py:160-163)."""
        n = self.subsample_size
        return data.view(-1, n, data.shape[1]).transpose(1, 2)

    # ------------------------------------------------------------------------------------------ early stopping / ckpt
    def set_patience_attributes(self, args):
        self.stopped_early = False
        self.best_metric_value = 10 ** 6
        self.best_metric_epoch = 1
        self.patience_in_epochs = args.patience_in_epochs

    def stop_early(self, val_metric, epoch, args):
        """Keep the best state so far (by a metric to minimise); True once patience is exhausted
        (point_net2.py:172-184)."""
        if val_metric < self.best_metric_value:
            self.best_metric_value, self.best_metric_epoch = val_metric, epoch
            self.save_state(args)
            return False
        if epoch < args.epoch_to_start_early_stop:
            return False
        if epoch >= self.best_metric_epoch + self.patience_in_epochs:
            self.stopped_early = True
            return True
        return False

    @staticmethod
    def _checkpoint_path(args):
        tag = f"fold_n={args.current_fold_id}" if args.current_fold_id > 0 else "full"
        return os.path.join(args.stats_path, f"PCC_model_{tag}.pt")

    def save_state(self, args):
        torch.save({"best_metric_epoch": self.best_metric_epoch, "state_dict": self.state_dict(),
                    "best_metric_value": self.best_metric_value}, self._checkpoint_path(args))

    def load_state(self, save_path):
        checkpoint = torch.load(save_path, map_location=None if self.cuda_device is not None else torch.device("cpu"))
        self.load_state_dict(checkpoint["state_dict"])
        self.best_metric_epoch = checkpoint["best_metric_epoch"]
        self.best_metric_value = checkpoint["best_metric_value"]
        return self

    def load_best_state(self, args):
        return self.load_state(self._checkpoint_path(args))
