"""Flat-buffer optimiser and data-parallel gradient exchange for the timed training step.

The reference's harness builds `optim.Adam(model.parameters(), lr=args.lr, weight_decay=args.wd)`
(`/root/reference/learning/train.py:180-185`).  `FlatAdam` is the same update rule (amsgrad off, L2 decay folded into
the gradient, bias correction) as ONE kernel over the model's 14 997 parameters, which `flatten_parameters` re-homes
into a single contiguous buffer (every nn.Parameter becomes a view of it, so `state_dict()` / `load_state_dict()` and
any torch optimiser keep working).  The backward pass already writes all gradients into one flat buffer
(`PointNet2._last_flat_grad`), so data parallelism is exactly one `all_reduce` of 60 KB per step.
"""
import torch

from . import hip_ops as ops


def shard_of_rank(rank: int, plots_per_rank: int):
    """(first plot, number of plots) of a rank: the global batch of `world * plots_per_rank` plots is cut into contiguous
    shards; plots are independent units (per-GPU BatchNorm statistics, as torch DDP without SyncBN)."""
    return rank * plots_per_rank, plots_per_rank


def allreduce_flat_grad(flat_grad: torch.Tensor, world_size: int, group=None, comm=None, force: bool = False) -> float:
    """The only exchange step of the data-parallel path: one SUM all-reduce of the flat gradient buffer (14 997 fp32 =
    60 KB, latency-bound on xGMI).  Returns the 1/world scale the optimiser kernel applies afterwards.
    comm: an `rccl.RcclComm` -- `ncclAllReduce` on torch's CURRENT stream ("on the compute stream"; inside a
    graph capture it becomes a node of the step's hipGraph), run at ANY world size including 1; None: torch's process group
    (its own stream and event hand-offs; skipped at world 1 unless `force`: a one-rank process group then runs the call, which
    is how bench.py times this path on a one-GPU box)."""
    if comm is not None:
        comm.all_reduce_sum_(flat_grad)
        return 1.0 / comm.world
    if world_size > 1 or force:
        torch.distributed.all_reduce(flat_grad, op=torch.distributed.ReduceOp.SUM, group=group)
    return 1.0 / world_size


def broadcast_bn_buffers(model, world_size: int, src: int = 0, group=None) -> int:
    """Optional second exchange of the data-parallel path (torch DDP's `broadcast_buffers`): every rank takes
    rank `src`'s BatchNorm running statistics -- 520 floats + 7 counters, one small broadcast.  The training step does not
    need it (batch statistics are per GPU, as DDP without SyncBN; the weights stay identical through the all-reduced
    gradient), but without it the replicas' EVAL-mode outputs drift apart, because each rank's running statistics follow
    its own shard.  Call it every K steps or before evaluating / checkpointing from a rank other than `src`.
    Returns the number of floats exchanged."""
    bufs = [b for n, b in model.named_buffers() if n.endswith("running_mean") or n.endswith("running_var")]
    cnts = [b for n, b in model.named_buffers() if n.endswith("num_batches_tracked")]
    if world_size <= 1 or not bufs:
        return 0
    flat = torch.cat([b.reshape(-1).float() for b in bufs])
    torch.distributed.broadcast(flat, src=src, group=group)
    o = 0
    for b in bufs:
        b.copy_(flat[o:o + b.numel()].view_as(b))
        o += b.numel()
    n = int(flat.numel())
    if cnts:
        # the int64 `num_batches_tracked` counters travel as int64 (a float32 carries integers only up to 2^24)
        ic = torch.stack([c.reshape(()).to(torch.int64) for c in cnts])
        torch.distributed.broadcast(ic, src=src, group=group)
        for c, v in zip(cnts, ic):
            c.copy_(v.to(c.dtype))
        n += int(ic.numel())
    return n


def flatten_parameters(model) -> torch.Tensor:
    params = list(model.parameters())
    offs, n = ops.flat_layout(params)
    flat = torch.zeros(n, dtype=params[0].dtype, device=params[0].device)
    for p, o in zip(params, offs):
        flat[o:o + p.numel()].copy_(p.detach().reshape(-1))
        p.data = flat[o:o + p.numel()].view(p.shape)
    model._flat_params = flat
    return flat


class FlatAdam:
    """Adam over the model's flat parameter buffer, one launch per step (sn2_adam_step_dev / sn2_adam_step_images_dev).

    Everything a step needs beside its gradient lives on the DEVICE, because every fast training mode captures the launch into
    a hipGraph once and replays it: the step count (`step_words`), the learning rate (`lr_dev`, one fp32 word) and the epoch
    meter (`meter`).  `opt.lr = x` writes the word with a fill on the current stream, so an assignment between two steps --
    eager calls or graph replays on that stream -- holds from the next step on; no re-capture.  `StepLR` below is the
    reference's schedule over that attribute.

    Epoch meter (`learning/train.py:68-79` reports the epoch means of the total, absolute and NLL loss): a feature step calls
    `opt.track(total, l_abs, l_log, l_e)` with the loss's own device scalars; the update launch that follows adds them to
    `meter` -- inside the Adam kernel, no launch and no host read per step.  Per epoch: `meter_reset()`, the steps, ONE
    `meter_read()`.  With several ranks the meter holds the sums of THIS rank's shard (the losses are never exchanged; the
    mean over ranks is the mean of the ranks' `meter_read()["means"]`, taken by whoever wants it)."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, process_group=None,
                 world_size=1, comm=None, fold_gradient_images=False):
        """fold_gradient_images: with no exchange between backward and update (one rank, no communicator) let THIS step's kernel
        fold the 32 images of the flat gradient (sn2_adam_step_images) instead of a launch of its own at the end of the backward
        pass: `model.defer_grad_reduce = True`; the parameters' `.grad` views hold the whole gradient after `step()` (before
        it: image 0 only).  Ignored when an exchange needs the folded gradient first."""
        self.model = model
        self.flat = getattr(model, "_flat_params", None)
        if self.flat is None:
            self.flat = flatten_parameters(model)
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)
        self.betas, self.eps, self.weight_decay = betas, eps, weight_decay
        # on the device (graph-replay safe): {steps taken so far, the kernel's arrival ticket}
        self.step_words = torch.zeros(2, dtype=torch.int32, device=self.flat.device)
        self.step_dev = self.step_words[:1]
        # ... the learning rate the kernel reads (the fp32 of the host value, as a by-value float argument would be) ...
        self._lr = float(lr)
        self.lr_dev = torch.full((1,), self._lr, dtype=torch.float32, device=self.flat.device)
        # ... and the epoch meter: METER_TERMS sums of tracked loss terms, then the number of steps added
        self.meter = torch.zeros(ops.METER_TERMS + 1, dtype=torch.float64, device=self.flat.device)
        self._tracked = None                  # terms registered by track(), consumed by the next update launch
        self._terms_eager = None              # the terms buffer of the last eager launch
        self._terms_captured = []             # every terms buffer a CAPTURED launch reads: a graph holds addresses, not tensors
        self.world_size = world_size
        self.process_group = process_group
        self.comm = comm                      # rccl.RcclComm: the exchange as ncclAllReduce on the step's own stream (graph-capturable)
        self.force_exchange = False           # torch's all_reduce even at world 1 (needs an initialised one-rank process group)
        if comm is not None and comm.world != world_size:
            raise ValueError("FlatAdam: the RCCL communicator and world_size disagree")
        self.fold_gradient_images = bool(fold_gradient_images) and world_size == 1 and comm is None
        if self.fold_gradient_images:
            model.defer_grad_reduce = True

    def _capturing(self):
        if not self.flat.is_cuda:
            return False
        with torch.cuda.device(self.flat.device):
            return torch.cuda.is_current_stream_capturing()

    @property
    def lr(self):
        """The learning rate as last assigned (host value; the kernel reads its fp32 from `lr_dev`)."""
        return self._lr

    @lr.setter
    def lr(self, value):
        """Stream-ordered: a fill of `lr_dev` on the CURRENT stream -- assign on the stream the steps run on (or one ordered with
        it); steps issued afterwards, graph replays included, use the new rate.  Refused inside a stream capture: the fill would
        become a node of the graph and pin the rate at every replay."""
        if self._capturing():
            raise RuntimeError("FlatAdam.lr: assigned while the current stream is capturing -- the write would be replayed with "
                               "the graph and pin the learning rate; assign between replays")
        self._lr = float(value)
        self.lr_dev.fill_(self._lr)

    def reset(self):
        """Forget the optimiser state: moments, step count, the Adam kernel's arrival ticket (`step_words[1]`: the last
        workgroup of a launch advances `step_words[0]` and zeroes the ticket; a ticket left non-zero -- state restored by
        hand, a launch that was aborted -- would keep the count from ever advancing again) AND the epoch meter.  The learning
        rate stays."""
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        self.step_words.zero_()
        self.meter.zero_()

    def state_dict(self):
        """What to save: the moments, the step count (`step_words[0]`; the ticket word is not state) and the learning rate."""
        return {"exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(), "step": int(self.step_words[0].item()),
                "lr": self._lr}

    def load_state_dict(self, sd):
        """(a dictionary without "lr" -- saved before the rate was state -- keeps the current rate)"""
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.step_words.copy_(torch.tensor([int(sd["step"]), 0], dtype=torch.int32))   # ticket zeroed whatever it was
        if "lr" in sd:
            self.lr = sd["lr"]

    def zero_grad(self, set_to_none=True):
        for p in self.model.parameters():
            p.grad = None
        self.model._last_flat_grad = None
        self.model._grad_images_pending = None

    # ---- epoch meter
    def track(self, *scalars):
        """Register this step's loss terms for the epoch meter: 1 to METER_TERMS fp64 device scalars that lie one after another
        in ONE buffer -- what `losses.total_loss` / `projected_total_loss` return: `opt.track(total, *parts)`.  The next update
        launch (`step()` / `update()`) consumes the registration and adds the terms to `meter[0 .. n)`; a later `track` before
        that launch replaces it (warm-up feature steps that no update follows do not pile up).  Inside a capture the launch is
        recorded with the buffer's ADDRESS: every replay adds what the replayed loss kernels wrote there."""
        n = len(scalars)
        if not 1 <= n <= ops.METER_TERMS:
            raise ValueError(f"FlatAdam.track: 1 to {ops.METER_TERMS} scalars, got {n}")
        first = scalars[0]
        for j, t in enumerate(scalars):
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.numel() == 1 and t.device == self.flat.device):
                raise ValueError(f"FlatAdam.track: scalar {j} is not one fp64 value on {self.flat.device}")
            if (t.untyped_storage().data_ptr() != first.untyped_storage().data_ptr() or
                    t.data_ptr() != first.data_ptr() + 8 * j):
                raise ValueError(f"FlatAdam.track: scalar {j} does not lie right behind scalar {j - 1} in the same buffer "
                                 "(pass the views of one loss output, in order)")
        self._tracked = first.detach().as_strided((n,), (1,))

    def meter_reset(self):
        """Zero the meter, in stream order on the current stream (refused inside a capture, like an `lr` assignment)."""
        if self._capturing():
            raise RuntimeError("FlatAdam.meter_reset inside a stream capture: the zero fill would be replayed with the graph")
        self.meter.zero_()

    def meter_read(self):
        """ONE device-to-host read (it waits for the steps issued so far on the current stream) -> {"steps": steps added since
        the last reset, "sums": their METER_TERMS sums in the order tracked, "means": sums / steps (NaN with no step)}."""
        vals = self.meter.cpu().tolist()
        steps = int(vals[ops.METER_TERMS])
        sums = vals[:ops.METER_TERMS]
        return {"steps": steps, "sums": sums, "means": [s / steps if steps else float("nan") for s in sums]}

    # ---- the update
    def update(self, grad, grad_scale=1.0, images=None):
        """THE update launch, stated once (`step()` and TrainPipeline's split capture come here): Adam on `grad` (the folded flat
        gradient), or with images = (arena, replicas, stride) on the arena's unfolded images; learning rate from `lr_dev`, the
        terms registered by `track()` into the meter."""
        terms, self._tracked = self._tracked, None
        if terms is not None:
            # the launch reads `terms` by address: kept alive here -- for a captured launch as long as the optimiser (the graph
            # replays it), for an eager one until the next (stream order makes an earlier buffer's reuse safe)
            if self._capturing():
                self._terms_captured.append(terms)
            else:
                self._terms_eager = terms
        if images is not None:
            arena, replicas, stride = images
            ops.adam_step_images_dev(self.flat, arena, replicas, stride, self.exp_avg, self.exp_avg_sq, self.lr_dev, self.betas[0],
                                     self.betas[1], self.eps, self.weight_decay, self.step_words, grad_scale, terms, self.meter)
        else:
            ops.adam_step_dev(self.flat, grad, self.exp_avg, self.exp_avg_sq, self.lr_dev, self.betas[0], self.betas[1], self.eps,
                              self.weight_decay, self.step_words, grad_scale, terms, self.meter)

    def step(self):
        g = self.model._last_flat_grad
        if g is None:
            raise RuntimeError("FlatAdam.step: no gradient (run backward through PointNet2 first)")
        pending = getattr(self.model, "_grad_images_pending", None)
        if pending is not None and not (self.world_size > 1 or self.force_exchange or self.comm is not None):
            self.model._grad_images_pending = None
            self.update(g, 1.0, images=pending)
            return
        if pending is not None:                # an exchange was switched on after the backward pass: fold first
            arena, replicas, stride = pending
            self.model._grad_images_pending = None
            ops.grad_reduce(arena, g.numel(), (replicas, stride))
        scale = allreduce_flat_grad(g, self.world_size, self.process_group, self.comm, self.force_exchange)   # RCCL over xGMI when world > 1
        self.update(g, scale)


class StepLR:
    """`torch.optim.lr_scheduler.StepLR(optimizer, step_size, gamma)` as the reference steps it, once per epoch
    (`learning/train.py:152,185`; main_SSL.py: step_size 1, gamma 0.75), over ANY object with an `lr` attribute -- for a `FlatAdam`
    the assignment is the stream-ordered write of its device word.  torch's recursive rule, so the floats are torch's:
    lr <- lr * gamma whenever the epoch count reaches a multiple of step_size.  Call `step()` between steps of the optimiser, on
    the stream they run on."""

    def __init__(self, opt, step_size, gamma=0.1):
        if int(step_size) < 1:
            raise ValueError("StepLR: step_size must be a positive number of epochs")
        self.opt, self.step_size, self.gamma = opt, int(step_size), float(gamma)
        self.last_epoch = 0
        self._last_lr = [opt.lr]

    def step(self):
        self.last_epoch += 1
        if self.last_epoch % self.step_size == 0:
            self.opt.lr = self.opt.lr * self.gamma
        self._last_lr = [self.opt.lr]

    def get_last_lr(self):
        """[the rate set by the last `step()`] (a list, as torch's: one parameter group)"""
        return list(self._last_lr)

    def state_dict(self):
        return {"step_size": self.step_size, "gamma": self.gamma, "last_epoch": self.last_epoch, "_last_lr": list(self._last_lr)}

    def load_state_dict(self, sd):
        """As torch's: restores the schedule's own counters; the rate itself is the optimiser's state (`FlatAdam.state_dict`)."""
        self.step_size, self.gamma, self.last_epoch = int(sd["step_size"]), float(sd["gamma"]), int(sd["last_epoch"])
        self._last_lr = list(sd["_last_lr"])
