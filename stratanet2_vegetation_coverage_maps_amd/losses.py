"""Device-side loss block of the timed training step -- mirror of the reference's
`learning/loss_functions.py:9-57` as used by `learning/train.py:58-62`:

    loss = get_absolute_loss(pred, gt) + m * get_NLL_loss(proba, pdf_all) + e * get_entropy_loss(proba)

`total_loss` is ONE autograd node over three HIP kernels (csrc/loss.hip: pointwise partial sums, finalize, backward)
instead of the ~75 elementwise launches torch needs for the same expression and its gradient -- at 2.5 ms per step
those launches were a fifth of the step.  `total_loss_torch` and the three `get_*_torch` functions keep the plain torch-op form
(same as the reference, usable on any device); the tests hold the fused kernels to them.  The three `get_*` functions the
reference's loop calls are that node with two terms switched off on a HIP device, the torch forms elsewhere.

Difference from the reference signature: `get_NLL_loss` takes the KDE-mixture densities `pdf_all (B*N,3)` directly
instead of evaluating `args.kde_mixture` on the CPU each step (`loss_functions.py:30-42`): `kde_densities` looks them up in
`KdeTables`, which `KdeTables.fit` / `from_plots` fit on the device (`learning/kde_mixture.py:16-100`) or `from_mixture` copies
from a mixture the reference fitted.
"""
import weakref

import torch

from . import hip_ops as ops
from ._lib import StrataHipError

EPS = 0.0001


def get_absolute_loss_torch(pred_pl, gt):
    # strata [low, med, high] = columns 0, 2, 3; sliced (not list-indexed: a python index list costs a host-to-device
    # copy per step and cannot be captured into a hipGraph)
    d = torch.cat((pred_pl[:, 0:1], pred_pl[:, 2:4]), 1) - torch.cat((gt[:, 0:1], gt[:, 2:4]), 1)
    return (d.pow(2) + EPS).pow(0.5).mean(0).mean()


def get_entropy_loss_torch(pred_pixels):
    p = pred_pixels[:, 2:]
    return -(p * torch.log(p + EPS) + (1 - p) * torch.log(1 - p + EPS)).mean()


def get_NLL_loss_torch(pred_pointwise, pdf_all):
    p_ground = pred_pointwise[:, 0] + pred_pointwise[:, 1]
    lik = p_ground * pdf_all[:, 0] + pred_pointwise[:, 2] * pdf_all[:, 1] + pred_pointwise[:, 3] * pdf_all[:, 2]
    return -torch.log(lik).mean()


def total_loss_torch(pred_coverages, proba_pointwise, gt, pdf_all, m=0.10, e=0.2 / 5):
    l_abs = get_absolute_loss_torch(pred_coverages, gt)
    l_log = get_NLL_loss_torch(proba_pointwise, pdf_all)
    l_e = get_entropy_loss_torch(proba_pointwise)
    return l_abs + m * l_log + e * l_e, (l_abs, l_log, l_e)


# The reference's loop calls the three terms one by one (learning/train.py:58-62).  On a HIP device each of them is ONE autograd
# node over the fused loss kernels with the other two terms SKIPPED (csrc/loss.hip: a switched-off term is not computed and its
# inputs need not exist) -- one or two launches forward and one backward per term instead of ~20 elementwise torch launches
# and their autograd graph (the eager drop-in loop is bound by its host time: DESIGN.md section 5) --, the values in fp64 as
# `total_loss`.  FUSED_TERMS = False (SN2_FUSED_LOSS_TERMS=0), CPU tensors: the plain torch forms above.
import os as _os
FUSED_TERMS = _os.environ.get("SN2_FUSED_LOSS_TERMS", "1") == "1"


def _fused_ok(*tensors):
    return FUSED_TERMS and all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors)


class _LossTerm(torch.autograd.Function):
    """ONE term of the training loss: kind 1 = absolute (x = plot-wise predictions (B,4), y = ground truth (B,4) fp64),
    2 = NLL (x = pointwise probabilities (R,4), y = densities (R,3) fp64), 3 = entropy (x = (R,4), y = None)."""

    @staticmethod
    def forward(ctx, kind, x, y):
        out = ops.loss_term_forward(kind, x, y)
        ctx.kind = kind
        ctx.save_for_backward(x, y) if y is not None else ctx.save_for_backward(x)
        return out[kind]

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None
        saved = ctx.saved_tensors
        x, y = saved[0], (saved[1] if len(saved) > 1 else None)
        return None, ops.loss_term_backward(ctx.kind, x, y, g.to(torch.float64).contiguous()), None


def get_absolute_loss(pred_pl, gt):
    if not _fused_ok(pred_pl, gt):
        return get_absolute_loss_torch(pred_pl, gt)
    with torch.cuda.device(pred_pl.device):
        return _LossTerm.apply(1, pred_pl.float().contiguous(), gt.to(torch.float64).contiguous())


def get_NLL_loss(pred_pointwise, pdf_all):
    if FUSED_TERMS and isinstance(pred_pointwise, torch.Tensor) and pred_pointwise.is_cuda and not pdf_all.is_cuda:
        # the reference evaluates its KDE mixture on the CPU and moves the densities to the device inside this function
        # (loss_functions.py:30-42): through the pinned ring, asynchronously (12.6 MB at C2: a pageable `.cuda()` blocks 0.4 ms),
        # on the upload stream -- the copy runs beside whatever the current stream still has queued (the forward pass: in the
        # reference's loop the device is 0.8 ms behind the host here), not behind it
        dev = pred_pointwise.device
        with torch.cuda.device(dev):
            pdf_all = ops.pinned_ring(dev).upload(pdf_all, stream=ops.shared_stream(dev, "upload"), dtype=torch.float64,
                                                  consumer=torch.cuda.current_stream(dev))
    if not _fused_ok(pred_pointwise, pdf_all):
        return get_NLL_loss_torch(pred_pointwise, pdf_all)
    with torch.cuda.device(pred_pointwise.device):
        return _LossTerm.apply(2, pred_pointwise.float().contiguous(), pdf_all.to(torch.float64).contiguous())


def get_entropy_loss(pred_pixels):
    if not _fused_ok(pred_pixels):
        return get_entropy_loss_torch(pred_pixels)
    with torch.cuda.device(pred_pixels.device):
        return _LossTerm.apply(3, pred_pixels.float().contiguous(), None)


class KdeTables:
    """The three linear-interpolation tables of the reference's `KdeMixture` (`learning/kde_mixture.py:62-70`: X and
    y1, y2, y3 from `evaluate_kdes`, what `interp1d` holds) on the device.  `KdeTables.fit(z, device)` fits them from heights on
    the device (csrc/kde.hip: the estimator behind KDEpy's FFTKDE, written out in include/strata_hip.h), `from_plots` from a
    dataset's plots; `KdeTables.from_mixture(args.kde_mixture, device)` copies the tables of a mixture the reference fitted."""

    def __init__(self, X, y1, y2, y3, device):
        import numpy as np
        X = np.asarray(X, dtype=np.float64)
        order = np.argsort(X, kind="stable")                      # interp1d(assume_sorted=False) sorts its knots
        Y = np.stack([np.asarray(y, dtype=np.float64)[order] for y in (y1, y2, y3)])
        self.X = torch.from_numpy(np.ascontiguousarray(X[order])).to(device)
        self.Y = torch.from_numpy(np.ascontiguousarray(Y)).to(device)

    @classmethod
    def from_mixture(cls, kde_mixture, device):
        return cls(kde_mixture.f1.x, kde_mixture.f1.y, kde_mixture.f2.y, kde_mixture.f3.y, device)


    @classmethod
    def fit(cls, z, device, bw=0.1, grid_points=5000):
        """`KdeMixture.fit` + `evaluate_kdes` (`learning/kde_mixture.py:50-100`) on the device: z = heights in metres (`cloud[2]`
        before rescaling), a host or device array of any shape, taken as fp32.  One finiteness check (the call's only
        synchronisation): ValueError on a NaN or Inf.  The grid comes out ascending, so there is no host `argsort` as in
        `__init__`.  The same heights give the same table bytes."""
        if not isinstance(z, torch.Tensor):
            import numpy as np
            z = torch.from_numpy(np.array(z, dtype=np.float32))
        z = z.detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous()
        if not z.is_cuda:
            raise StrataHipError("losses.KdeTables.fit runs on the HIP device")
        if not bool(torch.isfinite(z).all()):
            raise ValueError("KdeTables.fit: the heights must be finite (found NaN or Inf)")
        self = cls.__new__(cls)
        with torch.cuda.device(z.device):
            self.X, self.Y = ops.kde_fit(z, bw, grid_points)
        return self

    @classmethod
    def from_plots(cls, plots, device, size=500_000, seed=0, bw=0.1, grid_points=5000, offsets=None):
        """`get_fitted_kde_mixture_from_dataset` (`learning/kde_mixture.py:31-34`): `sample_heights` then `fit`."""
        return cls.fit(sample_heights(plots, size=size, seed=seed, offsets=offsets, device=device), device, bw, grid_points)


def sample_heights(plots, size=500_000, seed=0, offsets=None, device="cuda:0"):
    """The counterpart of `sample_z_from_dataset` (`learning/kde_mixture.py:16-21`: concatenate every plot's `cloud[2]`, shuffle,
    keep `size`): a uniform subset without replacement of all plots' heights, as (min(size, total),) fp32 on the device.
    plots: a list of (C >= 3, n_i) arrays or tensors (host or device; row 2 = z in metres), or ONE (C, T) array of plots side by
    side -- the resident `raw` of `input_pipeline.prepare_batch` -- with `offsets` (B+1) or None (all of it): the heights are
    raw[2, offsets[0]:offsets[-1]].  Fewer than `size` heights: all of them, in their order, nothing drawn.
    Drawn on the device with `hip_ops.subsample` (sn2_subsample) over ONE "plot" of key 0 spanning every height: the `size`
    heights with the smallest Philox4x32-10 keys u(seed, 0, i), in key order -- distinct indices, integer arithmetic only, so
    the same seed gives the same bytes (the distribution of the reference's shuffle, not numpy's draws).  Its limit is
    total < 2^31 heights."""
    dev = torch.device(device)
    if isinstance(plots, (list, tuple)):
        if offsets is not None:
            raise ValueError("sample_heights: offsets go with ONE (C, T) array, not with a list of plots")
        rows = [torch.as_tensor(p)[2].to(device=dev, dtype=torch.float32).reshape(-1) for p in plots]
        z = torch.cat(rows) if rows else torch.empty(0, dtype=torch.float32, device=dev)
    else:
        z = torch.as_tensor(plots)[2].to(device=dev, dtype=torch.float32).reshape(-1)
        if offsets is not None:
            z = z[int(offsets[0]):int(offsets[-1])]
    z = z.contiguous()
    if not z.is_cuda:
        raise StrataHipError("losses.sample_heights draws on the HIP device")
    total, size = z.numel(), int(size)
    if size <= 0:
        raise ValueError("sample_heights: size must be positive")
    if total <= size:
        return z
    if total >= 2 ** 31:
        raise ValueError("sample_heights: sn2_subsample numbers a plot's candidates with int32: fewer than 2^31 heights")
    with torch.cuda.device(dev):
        span = torch.tensor([0, total], dtype=torch.int32, device=dev)
        idx = ops.subsample(span, 0, size, int(seed), torch.zeros(1, dtype=torch.int64, device=dev), n_max=total)
        return z[idx[0].long()]


def kde_densities(clouds_dev, z_max, tables: KdeTables):
    """pdf_all (B*N,3) fp64 of `get_NLL_loss` (`learning/loss_functions.py:30-42`): the three KDE densities at every
    point's height z = cloud[2] * z_max, looked up on the device instead of through scipy on the CPU each step."""
    if not clouds_dev.is_cuda:
        raise StrataHipError("losses.kde_densities runs on the HIP device")
    with torch.cuda.device(clouds_dev.device):
        return ops.kde_lookup(clouds_dev.float().contiguous(), z_max, tables.X, tables.Y)


class _TotalLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, proba, gt, pdf, m, e):
        out = ops.loss_forward(pred, gt, proba, pdf, m, e)
        ctx.save_for_backward(pred, proba, gt, pdf)
        ctx.me = (m, e)
        ctx.set_materialize_grads(False)     # no zero tensors (= three fill launches per step) for the unused component outputs
        total, l_abs, l_log, l_e = out[0], out[1], out[2], out[3]
        ctx.mark_non_differentiable(l_abs, l_log, l_e)
        return total, l_abs, l_log, l_e

    @staticmethod
    def backward(ctx, g, *_):
        if g is None:
            return None, None, None, None, None, None
        pred, proba, gt, pdf = ctx.saved_tensors
        m, e = ctx.me
        dpred, dproba = ops.loss_backward(pred, gt, proba, pdf, m, e, g.to(torch.float64).contiguous())
        return dpred, dproba, None, None, None, None


def total_loss(pred_coverages, proba_pointwise, gt, pdf_all, m=0.10, e=0.2 / 5):
    """-> (total, (absolute, NLL, entropy)), fp64 scalars on the device; differentiable w.r.t. the first two arguments."""
    if not (pred_coverages.is_cuda and proba_pointwise.is_cuda):
        raise StrataHipError("losses.total_loss runs on the HIP device (total_loss_torch is the plain torch form)")
    with torch.cuda.device(pred_coverages.device):
        gt = gt.to(device=pred_coverages.device, dtype=torch.float64).contiguous()
        pdf_all = pdf_all.to(device=pred_coverages.device, dtype=torch.float64).contiguous()
        total, l_abs, l_log, l_e = _TotalLoss.apply(pred_coverages.float().contiguous(), proba_pointwise.float().contiguous(),
                                                    gt, pdf_all, float(m), float(e))
    return total, (l_abs, l_log, l_e)


_ZERO = {}      # device index -> a zero fp32 scalar that nothing ever writes (the fused route's placeholders are views of it)


def _zero_scalar(dev):
    """The cached zero of a device, made at the first fused backward pass.  If that pass runs under a stream capture (no eager
    warm-up step in front of it, unlike bench.py and the training loops here) the scalar is memory of the capture's pool and is
    NOT cached: that graph carries one fill node per replay and the next capture makes its own."""
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    z = _ZERO.get(idx)
    if z is None:
        z = torch.zeros((), dtype=torch.float32, device=dev)
        if torch.cuda.is_current_stream_capturing():
            return z                    # memory of the capture's pool: not kept beyond it
        _ZERO[idx] = z
    return z


class PendingLossGrad:
    """What `_ProjectedLoss.backward` leaves on the network's autograd node on the fused route instead of two (R,4) gradients: the
    inputs of `ops.projected_loss_backward` -- for the head backward, which computes both gradients itself (sn2_head.loss) -- and
    the two placeholders it returned to autograd in their place: views of ONE zero scalar, expanded to (R,4), no memory of their
    own.  If the network's node receives exactly those, nothing else consumed cov / proba and the descriptor is the whole
    incoming gradient; if autograd summed something onto one of them, `materialize` gives the two gradients as tensors.
    Who may see a placeholder instead of a gradient, and what is done about it:
      * a second loss node on the same cov / proba: a network node is claimed by ONE fused loss node (`_fused_net_node`), every
        further `projected_total_loss` over it returns real gradients, which autograd sums onto the placeholder: materialised;
      * `cov.retain_grad()` / `cov.register_hook(...)` (or on proba), set at any time before the backward pass:
        `_ProjectedLoss.backward` looks and returns real gradients;
      * NOT covered: `torch.autograd.grad(total, cov)` (the network's node never runs: the caller receives the zero placeholder)
        and hooks registered on the autograd NODE (`cov.grad_fn.register_prehook`).  Set `model.fuse_loss_backward = False` for
        such uses."""

    def __init__(self, saved, dims, g):
        self.saved, self.dims, self.g = saved, dims, g
        B, N = dims[0], dims[1]
        z = _zero_scalar(g.device)
        self.zero = z
        self.placeholders = (z.expand(B * N, 4), z.expand(B * N, 4))

    def is_placeholder(self, t):
        return (t is not None and t.dtype == torch.float32 and t.dim() == 2 and t.stride() == (0, 0) and
                t.shape == self.placeholders[0].shape and t.device == self.zero.device and t.data_ptr() == self.zero.data_ptr())

    def materialize(self):
        pred, proba, gt, pdf, arg, nocc, pix = self.saved
        B, N, D, m, e = self.dims
        return ops.projected_loss_backward(pred, gt, proba, pdf, B, N, D, m, e, self.g, arg, nocc, pix)

    def desc(self):
        """-> hip_ops.LossGrad (sn2_loss_grad) over the saved tensors"""
        pred, proba, gt, pdf, arg, nocc, pix = self.saved
        B, N, D, m, e = self.dims
        return ops.loss_grad_desc(pred, gt, proba, pdf if m != 0.0 else None, self.g, arg, nocc, pix, B, N, D, m, e)


class _ProjectedLoss(torch.autograd.Function):
    """`project_to_plotwise_coverages` + `total_loss` as ONE autograd node over three launches (csrc/project.hip:
    sn2_projected_loss_forward / _backward) instead of two nodes over seven.  net_node: the `_PointNet2Fn` node that produced cov
    and proba where the fused route applies (`projected_total_loss`), else None: the backward pass then launches nothing and
    hands that node a `PendingLossGrad`."""

    @staticmethod
    def forward(ctx, cov, proba, pix, gt, pdf, B, N, D, m, e, net_node=None):
        out, pred, arg, nocc = ops.projected_loss_forward(cov, pix, proba, pdf, gt, B, N, D, m, e)
        ctx.save_for_backward(pred, proba, gt, pdf, arg, nocc, pix)
        ctx.dims = (B, N, D, m, e)
        ctx.net_node = net_node
        # (weak: the loss node must not keep the network's outputs alive; looked at in backward for hooks / retain_grad)
        ctx.outs = (weakref.ref(cov), weakref.ref(proba)) if net_node is not None else None
        ctx.set_materialize_grads(False)
        total, l_abs, l_log, l_e = out[0], out[1], out[2], out[3]
        ctx.mark_non_differentiable(l_abs, l_log, l_e, pred)
        return total, l_abs, l_log, l_e, pred

    @staticmethod
    def backward(ctx, g, *_):
        if g is None:
            return (None,) * 11
        pred, proba, gt, pdf, arg, nocc, pix = ctx.saved_tensors
        B, N, D, m, e = ctx.dims
        g = g.to(torch.float64).contiguous()
        if ctx.net_node is not None and not any(_observed(r()) for r in ctx.outs):
            # (one loss node per network node, `_fused_net_node`: a descriptor found here is this node's own from a backward pass
            # that never reached the network, e.g. torch.autograd.grad w.r.t. cov alone -- replaced)
            pending = PendingLossGrad((pred, proba, gt, pdf, arg, nocc, pix), ctx.dims, g)
            ctx.net_node.loss_grad = pending
            return pending.placeholders + (None,) * 9
        dcov, dproba = ops.projected_loss_backward(pred, gt, proba, pdf, B, N, D, m, e, g, arg, nocc, pix)
        return (dcov, dproba) + (None,) * 9


def _observed(t):
    """Does anything look at this tensor's gradient (retain_grad, a tensor hook)?  It must then be the real one."""
    return t is not None and (bool(t.retains_grad) or bool(getattr(t, "_backward_hooks", None)))


def _fused_net_node(cov, proba, cov32, proba32, B, N, D):
    """The autograd node whose backward pass can take the loss gradient as a descriptor, or None: cov and proba are outputs 0 and
    1 of ONE `_PointNet2Fn` node, untouched by the casts above (the very same tensors), that node's model has
    `fuse_loss_backward` on, no other loss node has claimed it (two descriptors cannot both be the whole incoming gradient: the
    second and later loss nodes over one forward return real gradients) and the library takes the sizes."""
    from .point_net2 import _PointNet2Fn
    node = cov.grad_fn
    if node is None or node is not proba.grad_fn or not isinstance(node, _PointNet2Fn._backward_cls):
        return None
    if cov32 is not cov or proba32 is not proba or cov.output_nr != 0 or proba.output_nr != 1:
        return None
    if tuple(cov.shape) != (B * N, 4) or tuple(proba.shape) != (B * N, 4):
        return None
    if not getattr(getattr(node, "model", None), "fuse_loss_backward", False) or getattr(node, "saved", None) is None:
        return None
    if getattr(node, "loss_node_claimed", False) or not ops.head_loss_route(B, N, D):
        return None
    node.loss_node_claimed = True
    return node


def projected_total_loss(coverages_pointwise, proba_pointwise, clouds, gt, pdf_all, args, geometry=None, model=None):
    """`pred = project_to_plotwise_coverages(coverages_pointwise, clouds, args)` followed by `total_loss(pred, proba_pointwise, gt,
    pdf_all, args.m, args.e)` (learning/train.py:54-62) -> (total, (absolute, NLL, entropy), pred).  With the pixel ids of a
    geometry pass at hand (`geometry.p2_pix`: `model.p2_diam_pix = args.diam_pix`) the two are ONE autograd node over three
    launches -- the scatter of the coverages beside the pointwise loss sums, the per-plot finalisation whose last workgroup adds
    the loss up, and one backward pass that writes both gradients; same pred, same gradients (bits), the loss to fp64
    re-association.  Without them: the two calls.
    Where cov and proba are the two outputs of ONE network node whose model has `fuse_loss_backward` on, and the library takes the
    sizes (`ops.head_loss_route`), that backward pass is no launch at all: the head backward computes both gradients from the
    loss's inputs (`PendingLossGrad`; the same gradient bits, csrc/loss_rules.h)."""
    from .project_to_2d import project_to_plotwise_coverages
    pix = getattr(geometry, "p2_pix", None) if geometry is not None else None
    B = clouds.shape[0]
    N = clouds.shape[2]
    ok = (pix is not None and getattr(geometry, "p2_diam_pix", None) == int(args.diam_pix) and pix.numel() == B * N and
          coverages_pointwise.is_cuda and proba_pointwise.is_cuda)
    if not ok:
        pred = project_to_plotwise_coverages(coverages_pointwise, clouds, args, model=model, geometry=geometry)
        total, parts = total_loss(pred, proba_pointwise, gt, pdf_all, args.m, args.e)
        return total, parts, pred
    dev = coverages_pointwise.device
    with torch.cuda.device(dev):
        gt = gt.to(device=dev, dtype=torch.float64).contiguous()
        pdf_all = pdf_all.to(device=dev, dtype=torch.float64).contiguous()
        cov32, proba32 = coverages_pointwise.float().contiguous(), proba_pointwise.float().contiguous()
        total, l_abs, l_log, l_e, pred = _ProjectedLoss.apply(cov32, proba32, pix, gt, pdf_all, B, N, int(args.diam_pix), float(args.m),
                                                              float(args.e), _fused_net_node(coverages_pointwise, proba_pointwise, cov32,
                                                                                             proba32, B, N, int(args.diam_pix)))
    return total, (l_abs, l_log, l_e), pred
