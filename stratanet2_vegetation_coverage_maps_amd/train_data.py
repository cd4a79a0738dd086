"""Training from a plot set that lives on the device: the reference's `train()` loop (`learning/train.py:29-79`) builds every
batch afresh through `load_cloud(train=True)` (`data_loader/loader.py:73-87`) -- a new shuffle per epoch, a new rotation and flips
per plot, new clipped gaussian noise per point, a new subsample.  Here the set is uploaded once (`ResidentPlots`), and each step's
batch is written straight into the caller's buffers -- a `TrainPipeline` slot -- by `sn2_train_batch` (csrc/feed.hip): every draw
comes from a counter-based generator on the device, keyed by (seed, epoch, plot id), so a plot's rows do not depend on the batch
size, its place in the batch or the slot, and a resumed run draws the same batches.  The only per-step host work left is the
upload of the batch's B plot ids; the only per-epoch host work is `torch.randperm(P)`, drawn as the DataLoader's RandomSampler
draws it.

    plots = ResidentPlots.from_dataset(dataset, device)            # or .from_plots(raw_plots, centers, coverages, device)
    feeder = EpochFeeder(plots, args, batch_size, seed=1234, kde=tables)
    pipe.set_feeder(feeder)                                        # fills slot i % slots before batch i's geometry pass

A set may also be grown on the device: `ResidentPlots.empty(point_capacity, plot_capacity, device)` is an arena with spare room,
`append(plots, coverages, ...)` moves selected plots of a `parcel.ParcelPlots` (or of another set) into it with one
`sn2_plots_append` launch and no host read (`pseudo_label.py` labels parcels that way).  Complete the set first, then build its
feeder: a feeder built on an older state of the set refuses to run.  `EpochFeeder(..., plot_subset=ids)` trains on a part of a set,
`ResidentPlots.eval_batches(ids, ...)` hands the rest to `evaluation.evaluate`.

Generator layout and contract: include/strata_hip.h, sn2_train_batch; the append: sn2_plots_append.
"""
import numpy as np
import torch

from . import hip_ops as ops
from .input_pipeline import fake_ground_xy

_COS_SIN = None


def cos_sin_table() -> np.ndarray:
    """(360,2) fp64: cos and sin of the whole-degree angles as the reference computes them (`np.radians(np.random.choice(360))`,
    loader.py:217-230).  The kernel reads the rotation from this table, so it is numpy's bit for bit."""
    global _COS_SIN
    if _COS_SIN is None:
        a = np.radians(np.arange(360))
        _COS_SIN = np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], 1))
    return _COS_SIN


def plan_append(n_points, select, min_points, P0: int, T0: int, point_capacity: int, plot_capacity: int):
    """The host side of `ResidentPlots.append`, from counts the host already has (no device anywhere): n_points (Ps) the source
    plots' point counts, select a sequence of source plot numbers (any order, repeats allowed) or None (all, in order), min_points
    None or the count a plot must EXCEED to be kept (`filter_dataset` of the reference keeps `N_points_in_cloud > 2000`), P0 / T0
    the plots / points the destination holds ->
        (kept (K) int64 source plot numbers, dst_start (K+1) int64 = T0 + the running sum of the kept plots' points,
         the largest kept plot's points (0 when K = 0)).
    A selection outside [0, Ps), or one that does not fit the capacities, raises ValueError; the message names the capacity needed."""
    n = np.asarray(n_points, dtype=np.int64).reshape(-1)
    if n.size and int(n.min()) < 0:
        raise ValueError("plan_append: point counts cannot be negative")
    if select is None:
        sel = np.arange(n.size, dtype=np.int64)
    else:
        sel = np.asarray(select)
        if sel.size == 0:
            sel = np.zeros(0, dtype=np.int64)
        if sel.ndim != 1 or sel.dtype.kind not in "iu":
            raise ValueError("plan_append: select must be a 1-D integer sequence")
        sel = sel.astype(np.int64)
        if sel.size and (int(sel.min()) < 0 or int(sel.max()) >= n.size):
            raise ValueError(f"plan_append: every selected plot must be in [0, {n.size})")
    if min_points is not None:
        sel = sel[n[sel] > int(min_points)]
    K = int(sel.size)
    dst_start = int(T0) + np.concatenate([[0], np.cumsum(n[sel])]).astype(np.int64)
    if K and (int(P0) + K > int(plot_capacity) or int(dst_start[-1]) > int(point_capacity)):
        raise ValueError(f"ResidentPlots.append: {K} plots with {int(dst_start[-1]) - int(T0)} points need a capacity of "
                         f"{int(P0) + K} plots and {int(dst_start[-1])} points; the set has room for {int(plot_capacity)} plots "
                         f"and {int(point_capacity)} points (reserve() grows it)")
    return sel, dst_start, (int(n[sel].max()) if K else 0)


class ResidentPlots:
    """A set of P raw plots on the device: raw (10,T) fp32 side by side (channel order of `hip_ops.prepare_plots`), offsets (P+1)
    int32, centers (P,2) fp32, coverages (P,4) fp64.

    A set made by `empty` is an arena: raw (10, point_capacity) of which the first `n_filled` columns hold plots, and tables with
    room for `plot_capacity` plots, of which `offsets`, `centers`, `coverages` are the contiguous views of the filled part -- what
    `fill`, `hip_ops.train_batch` and `losses.sample_heights(raw, offsets=...)` take, with raw.shape[1] as the row stride.
    `append` fills it, `reserve` is the only call that reallocates.  COMPLETE THE SET BEFORE BUILDING A FEEDER ON IT: `version`
    counts the appends and reserves, and an `EpochFeeder` built on an older version raises instead of running with workspaces
    sized for smaller plots and generator keys of another P."""

    def __init__(self, raw, offsets, centers, coverages, n_points_max: int, n_points=None):
        self.raw, self.offsets, self.centers, self.coverages = raw, offsets, centers, coverages
        self.P = int(offsets.numel()) - 1
        self.n_points_max = int(n_points_max)               # the largest plot's raw points: known on the host, never read back
        self.n_points = None if n_points is None else np.asarray(n_points, dtype=np.int64).reshape(-1)   # per plot, on the host
        self.n_filled = int(raw.shape[1])                   # columns of raw that hold plots (an arena: fewer than raw.shape[1])
        self.version = 0                                    # bumped by append / reserve
        self._arena = (offsets, centers, coverages)         # the whole tables; offsets / centers / coverages view their filled part
        self.device = raw.device
        self._consts = {}                                   # diam_meters -> fake ground points on the device
        self._cos_sin = torch.from_numpy(cos_sin_table()).to(self.device)
        self._ws = {}                                       # (stream, B, N, extra) -> workspace of standalone `fill` calls

    @property
    def point_capacity(self) -> int:
        return int(self.raw.shape[1])

    @property
    def plot_capacity(self) -> int:
        return int(self._arena[1].shape[0])

    @classmethod
    def empty(cls, point_capacity: int, plot_capacity: int, device):
        """An arena for `point_capacity` points and `plot_capacity` plots holding no plot yet (P = 0): `append` fills it.  Using it
        while it is empty (`fill`, a feeder) raises ValueError."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ops.StrataHipError("train_data.ResidentPlots lives on the HIP device")
        point_capacity, plot_capacity = int(point_capacity), int(plot_capacity)
        if not 1 <= point_capacity < 2 ** 31 or not 1 <= plot_capacity < 2 ** 31 - 1:
            raise ValueError("ResidentPlots.empty: capacities of 1 .. 2^31 - 1 points and at least one plot")
        raw = torch.empty(10, point_capacity, dtype=torch.float32, device=dev)
        arena = (torch.zeros(plot_capacity + 1, dtype=torch.int32, device=dev),
                 torch.empty(plot_capacity, 2, dtype=torch.float32, device=dev),
                 torch.empty(plot_capacity, 4, dtype=torch.float64, device=dev))
        self = cls(raw, arena[0][:1], arena[1][:0], arena[2][:0], 0, n_points=np.zeros(0, dtype=np.int64))
        self._arena, self.n_filled = arena, 0
        return self

    def _rebind(self):
        o, c, g = self._arena
        self.offsets, self.centers, self.coverages = o[:self.P + 1], c[:self.P], g[:self.P]

    def append(self, plots, coverages, select=None, min_points=None) -> int:
        """Appends plots of `plots` -- anything with raw (10,T), offsets, centers on this device and the per-plot point counts
        `n_points` on the host: a `parcel.ParcelPlots`, another `ResidentPlots` -- with `coverages` (len(plots),4) fp32 on the
        device as their ground truth (the plot-wise predictions of `pseudo_label.label_plots`; widened to fp64 exactly) ->
        the number of plots appended.  select: a host sequence of plot numbers of `plots` (any order) or None (all); min_points: a
        plot is kept iff n_points > min_points (the reference's strict test).
        All bookkeeping comes from the host's counts (`plan_append`); the upload is one small int32 table, the work one
        `sn2_plots_append` launch on the current stream; nothing is read back.  A selection that does not fit raises ValueError
        before any launch (the arena never reallocates on its own: `reserve`); nothing kept returns 0 without a launch.
        Drops the cached `fill` workspaces and bumps `version`: feeders built before are stale."""
        if plots is self:
            raise ValueError("ResidentPlots.append: a set cannot be appended to itself")
        n_src = getattr(plots, "n_points", None)
        if n_src is None:
            raise ValueError("ResidentPlots.append: the source needs its per-plot point counts `n_points` on the host")
        sel, dst_start, n_max = plan_append(n_src, select, min_points, self.P, self.n_filled, self.point_capacity, self.plot_capacity)
        K = int(sel.size)
        if K == 0:
            return 0
        if plots.raw.device != self.device or coverages.device != self.device:
            raise ValueError(f"ResidentPlots.append: the source plots and coverages must be on {self.device}")
        table = torch.from_numpy(np.concatenate([sel, dst_start]).astype(np.int32)).to(self.device)
        with torch.cuda.device(self.device):
            ops.plots_append(plots.raw, plots.offsets, plots.centers, coverages, table[:K], self.raw, *self._arena, self.P,
                             self.n_filled, table[K:], int(dst_start[-1]))
        if self.n_points is not None:
            self.n_points = np.concatenate([self.n_points, np.asarray(n_src, dtype=np.int64).reshape(-1)[sel]])
        self.P += K
        self.n_filled = int(dst_start[-1])
        self.n_points_max = max(self.n_points_max, n_max)
        self._rebind()
        self._ws = {}                                       # sized by n_points_max
        self.version += 1
        return K

    def reserve(self, point_capacity: int, plot_capacity: int):
        """Reallocates the arena to the given capacities (at least what is filled) and copies the filled part, with torch ops on
        the current stream.  Bumps `version`."""
        point_capacity, plot_capacity = int(point_capacity), int(plot_capacity)
        if point_capacity < max(1, self.n_filled) or plot_capacity < max(1, self.P) or point_capacity >= 2 ** 31:
            raise ValueError(f"ResidentPlots.reserve: the set holds {self.P} plots with {self.n_filled} points (and at most "
                             "2^31 - 1 points fit)")
        with torch.cuda.device(self.device):
            raw = torch.empty(10, point_capacity, dtype=torch.float32, device=self.device)
            raw[:, :self.n_filled].copy_(self.raw[:, :self.n_filled])
            arena = (torch.zeros(plot_capacity + 1, dtype=torch.int32, device=self.device),
                     torch.empty(plot_capacity, 2, dtype=torch.float32, device=self.device),
                     torch.empty(plot_capacity, 4, dtype=torch.float64, device=self.device))
            for new, old in zip(arena, (self.offsets, self.centers, self.coverages)):
                new[:old.shape[0]].copy_(old)
        self.raw, self._arena = raw, arena
        self._rebind()
        self._ws = {}
        self.version += 1

    @classmethod
    def from_plots(cls, raw_plots, centers, coverages, device):
        """raw_plots: P arrays / tensors (10, n_i) float32; centers (P,2); coverages (P,4).  One upload."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ops.StrataHipError("train_data.ResidentPlots lives on the HIP device")
        plots = [torch.as_tensor(np.asarray(p) if not isinstance(p, torch.Tensor) else p, dtype=torch.float32) for p in raw_plots]
        P = len(plots)
        if P == 0 or any(p.dim() != 2 or p.shape[0] != 10 for p in plots):
            raise ValueError("ResidentPlots: need at least one plot, each of shape (10, n)")
        n = [int(p.shape[1]) for p in plots]
        if sum(n) >= 2 ** 31 or sum(n) == 0:
            raise ValueError("ResidentPlots: the set must hold between 1 and 2^31 - 1 points")
        centers = np.asarray(centers, dtype=np.float32).reshape(P, 2)
        coverages = np.asarray(coverages, dtype=np.float64).reshape(P, 4)
        raw = torch.cat([p.cpu() for p in plots], 1).contiguous().to(dev)
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(n)]).astype(np.int32)).to(dev)
        return cls(raw, offsets, torch.from_numpy(centers).to(dev), torch.from_numpy(coverages).to(dev), max(n), n_points=n)

    @classmethod
    def from_dataset(cls, dataset, device):
        """dataset: the reference's dict {plot_id: cloud_data} (`utils/load_data.py:52-85`); the plots are ordered by their "index"
        as `get_index_sorted_plot_ids` (loader.py:46-54) orders them, so plot number p here is entry p of the reference's list."""
        items = sorted(dataset.values(), key=lambda cd: cd["index"])
        return cls.from_plots([cd["cloud"] for cd in items], [cd["plot_center"] for cd in items],
                              [np.asarray(cd["coverages"], dtype=np.float64).reshape(4) for cd in items], device)

    def _fake(self, diam_meters: int):
        f = self._consts.get(diam_meters)
        if f is None:
            f = self._consts[diam_meters] = torch.from_numpy(fake_ground_xy(diam_meters)).to(self.device)
        return f

    def workspace(self, B: int, N: int, diam_meters: int) -> torch.Tensor:
        """A workspace for `fill` calls of this shape (int32, 16-byte aligned: torch's allocations are)."""
        n_max = self.n_points_max + int(self._fake(diam_meters).shape[0])
        return torch.empty(max(4, ops.train_batch_ws_words(B, n_max, N)), dtype=torch.int32, device=self.device)

    def check_ids(self, ids) -> torch.Tensor:
        """plot ids on the HOST -> (B) int32 host tensor; an id outside [0, P) never reaches a kernel."""
        ids = torch.as_tensor(ids, device="cpu")
        if ids.dim() != 1 or ids.numel() == 0 or ids.dtype.is_floating_point:
            raise ValueError("plot_ids: expected a non-empty 1-D integer sequence")
        if int(ids.min()) < 0 or int(ids.max()) >= self.P:
            raise ValueError(f"plot_ids: every id must be in [0, {self.P})")
        return ids.to(torch.int32)

    def fill(self, plot_ids, epoch: int, seed: int, args, out, train: bool = True, noise: bool = True, kde=None, ws=None):
        """One batch into out = {"cloud" (B,10,N), "xyz" (B,3,N), "gt" (B,4) f64, "fps_start" (2,B) i32 [, "pdf" (B N,3) f64]
        [, "n_live" (B) i32: the plots' live prefixes, `cloud_data["n_live"]` of PointNet2 -- written when `out` has it]} on the
        current stream.  plot_ids: a host sequence (checked and uploaded here), or an int32 DEVICE tensor whose host source the
        caller has put through `check_ids` (EpochFeeder).  kde: a `losses.KdeTables` -> out["pdf"] = the densities of the cloud
        just written, the bytes of `losses.kde_densities(cloud, z_max, kde)`."""
        if self.P == 0:
            raise ValueError("ResidentPlots.fill: the set is empty")
        with torch.cuda.device(self.device):
            if not (isinstance(plot_ids, torch.Tensor) and plot_ids.is_cuda):
                plot_ids = self.check_ids(plot_ids).to(self.device)
            cloud = out["cloud"]
            B, _, N = cloud.shape
            fake = self._fake(args.diam_meters)
            n_max = self.n_points_max + int(fake.shape[0])
            if ws is None:
                key = (torch.cuda.current_stream(self.device).cuda_stream, B, N, int(fake.shape[0]))
                ws = self._ws.get(key)
                if ws is None:
                    ws = self._ws[key] = self.workspace(B, N, args.diam_meters)
            M1 = ops.fps_num_samples(N, args.ratio1)
            ops.train_batch(self.raw, self.offsets, self.centers, self.coverages, plot_ids, fake, n_max, M1, args.z_max, seed, epoch,
                            self._cos_sin, cloud, out["xyz"], out["gt"], out["fps_start"], ws, train=train, noise=noise,
                            n_live=out.get("n_live"))
            if kde is not None:
                ops.kde_lookup(cloud, args.z_max, kde.X, kde.Y, out=out["pdf"])
        return out

    def eval_batches(self, ids, args, batch_size: int, seed: int = 0, kde=None):
        """The plots `ids` (a host sequence, checked here) as the batches `evaluation.evaluate` takes, `batch_size` plots each (the
        last one may be short), made by `fill(train=False)` on the current stream: "cloud", "xyz", "coverages" (the fp64 ground
        truth rows), "plot_id" (the ids as an int32 device tensor: `evaluate` reads them back with its table, at the end),
        "fps_start", "n_live", and "pdf_all" when `kde` (a `losses.KdeTables`) is given.  Every batch has tensors of its own
        (`evaluate` keeps several batches in flight).  The subsample of a plot larger than subsample_size is keyed by (seed, plot
        id): epoch 0 of `fill`."""
        ids = self.check_ids(ids)
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("eval_batches: batch_size must be at least 1")
        return self._eval_batches(ids, args, batch_size, int(seed), kde)

    def _eval_batches(self, ids, args, batch_size, seed, kde):
        N, dev = int(args.subsample_size), self.device
        for b0 in range(0, ids.numel(), batch_size):
            chunk = ids[b0:b0 + batch_size].to(dev)
            B = chunk.numel()
            out = {"cloud": torch.empty(B, 10, N, dtype=torch.float32, device=dev),
                   "xyz": torch.empty(B, 3, N, dtype=torch.float32, device=dev),
                   "gt": torch.empty(B, 4, dtype=torch.float64, device=dev),
                   "fps_start": torch.empty(2, B, dtype=torch.int32, device=dev),
                   "n_live": torch.empty(B, dtype=torch.int32, device=dev)}
            if kde is not None:
                out["pdf"] = torch.empty(B * N, 3, dtype=torch.float64, device=dev)
            self.fill(chunk, 0, seed, args, out, train=False, noise=False, kde=kde)
            d = {"cloud": out["cloud"], "xyz": out["xyz"], "coverages": out["gt"], "plot_id": chunk, "fps_start": out["fps_start"],
                 "n_live": out["n_live"]}
            if kde is not None:
                d["pdf_all"] = out["pdf"]
            yield d


class EpochFeeder:
    """Feeds a `TrainPipeline` (set_feeder) from a `ResidentPlots`: batch number i is batch i % steps_per_epoch of epoch
    i // steps_per_epoch, the order of an epoch is `torch.randperm(P, generator=generator)` drawn on the host once per epoch in
    epoch order (the DataLoader's RandomSampler), the last incomplete batch is dropped (`drop_last`).

    plot_subset: None (all P plots: the orders above) or a host sequence of plot ids (checked once, here): an epoch's order is
    `subset[torch.randperm(len(subset), generator=generator)]`, steps_per_epoch = len(subset) // batch_size.  The generator key of a
    plot stays epoch * P + plot id with the SET's P: a plot's draws do not depend on the subset it is trained in.
    The set must be complete: after a `ResidentPlots.append` or `reserve` this feeder raises on its next use.

    The geometry passes run ahead of training, across epoch boundaries, and with `slot_wait="device"` the host can be many batches
    ahead of the device: every epoch's order is a FRESH pinned tensor, the batch's ids are uploaded from a slice of it, and torch's
    pinned allocator keeps that memory from being handed out again before the copies that read it have run."""

    KEEP_EPOCHS = 64          # orders (and the generator states in front of them) remembered behind the newest one

    def __init__(self, plots, args, batch_size: int, seed: int, kde=None, train: bool = True, noise: bool = True, generator=None,
                 plot_subset=None):
        self.plots, self.args, self.B = plots, args, int(batch_size)
        self.P = int(plots.P)
        self._version = getattr(plots, "version", 0)
        self.subset = None if plot_subset is None else ResidentPlots.check_ids(plots, plot_subset)     # (n) int32 on the host
        self.n_draw = self.P if self.subset is None else int(self.subset.numel())
        self.steps_per_epoch = self.n_draw // self.B if self.B >= 1 else 0
        if self.B < 1 or self.steps_per_epoch < 1:
            raise ValueError("EpochFeeder: need 1 <= batch_size <= number of plots")
        if not 0 <= int(seed) < 2 ** 64:
            raise ValueError("EpochFeeder: seed must fit 64 unsigned bits")
        self.seed, self.kde, self.train, self.noise = int(seed), kde, bool(train), bool(noise)
        self.generator = generator if generator is not None else torch.Generator().manual_seed(self.seed % 2 ** 63)
        self.epoch0 = 0                   # epoch of batch number 0 (load_state_dict moves it)
        self.batch0 = 0                   # ... and that batch's place in its epoch
        self._orders = {}                 # epoch -> (generator state in front of its draw, order (P) int32, pinned where possible)
        self._next_epoch = 0              # the next epoch to draw
        self._slot_ids = {}               # id(slot dict) -> (B) int32 device tensor owned by that slot
        self._slot_ws = {}

    # ---- host bookkeeping (no device)
    def _check_fresh(self):
        if getattr(self.plots, "version", 0) != self._version:
            raise RuntimeError("EpochFeeder: the plot set has changed (append / reserve) since this feeder was built -- its "
                               "workspaces and generator keys belong to the older set; build the feeder after the set is complete")

    def _order(self, epoch: int):
        while self._next_epoch <= epoch:
            state = self.generator.get_state()
            order = torch.randperm(self.n_draw, generator=self.generator)
            order = order.to(torch.int32) if self.subset is None else self.subset[order]
            if torch.cuda.is_available():
                order = order.pin_memory()
            self._orders[self._next_epoch] = (state, order)
            self._orders.pop(self._next_epoch - self.KEEP_EPOCHS, None)
            self._next_epoch += 1
        if epoch not in self._orders:
            raise ValueError(f"EpochFeeder: epoch {epoch} lies more than {self.KEEP_EPOCHS} epochs behind the newest one drawn")
        return self._orders[epoch][1]

    def locate(self, i: int):
        """batch number i -> (epoch, batch of that epoch)."""
        j = int(i) + self.batch0
        if i < 0:
            raise ValueError("EpochFeeder: batch numbers start at 0")
        return self.epoch0 + j // self.steps_per_epoch, j % self.steps_per_epoch

    def batch_ids(self, i: int) -> torch.Tensor:
        """The B plot ids of batch number i: a slice of its epoch's (pinned) order on the host."""
        self._check_fresh()
        epoch, k = self.locate(i)
        return self._order(epoch)[k * self.B:(k + 1) * self.B]

    def state_dict(self, batch: int = 0):
        """What a resumed run needs to draw batch number `batch` and everything after it again: load it into a feeder built with
        the same set, batch size and flags, and that feeder's batch 0 is this one's batch `batch`."""
        epoch, k = self.locate(batch)
        self._order(epoch)
        return {"seed": self.seed, "epoch": epoch, "batch_in_epoch": k, "generator_state": self._orders[epoch][0].clone(),
                "plots": self.P, "batch_size": self.B, "subset": None if self.subset is None else self.n_draw}

    def load_state_dict(self, sd):
        if int(sd["plots"]) != self.P or int(sd["batch_size"]) != self.B:
            raise ValueError("EpochFeeder: the state belongs to another set or batch size")
        if sd.get("subset") != (None if self.subset is None else self.n_draw):
            raise ValueError("EpochFeeder: the state belongs to another plot subset")
        self.seed = int(sd["seed"])
        self.epoch0 = self._next_epoch = int(sd["epoch"])
        self.batch0 = int(sd["batch_in_epoch"])
        self.generator.set_state(sd["generator_state"])
        self._orders = {}

    # ---- the device side
    def fill_slot(self, i: int, slot):
        """Batch number i into `slot` (a TrainPipeline slot dict) on the CURRENT stream: B ids up, one `ResidentPlots.fill`.  The
        slot's tensors are written through, never rebound (in group mode they are views of the pass group's tensors)."""
        self._check_fresh()
        epoch, _ = self.locate(i)
        host_ids = self.batch_ids(i)      # a permutation of 0 .. P-1 or of the checked subset: in range by construction
        key = id(slot)
        ids = self._slot_ids.get(key)
        if ids is None:
            B, _, N = slot["cloud"].shape
            if B != self.B:
                raise ValueError(f"EpochFeeder: the slot holds batches of {B}, the feeder makes batches of {self.B}")
            ids = self._slot_ids[key] = torch.empty(self.B, dtype=torch.int32, device=self.plots.device)
            self._slot_ws[key] = self.plots.workspace(B, N, self.args.diam_meters)
        ids.copy_(host_ids, non_blocking=True)
        self.plots.fill(ids, epoch, self.seed, self.args, slot, train=self.train, noise=self.noise, kde=self.kde,
                        ws=self._slot_ws[key])
