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

Generator layout and contract: include/strata_hip.h, sn2_train_batch.
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


class ResidentPlots:
    """A set of P raw plots on the device: raw (10,T) fp32 side by side (channel order of `hip_ops.prepare_plots`), offsets (P+1)
    int32, centers (P,2) fp32, coverages (P,4) fp64."""

    def __init__(self, raw, offsets, centers, coverages, n_points_max: int):
        self.raw, self.offsets, self.centers, self.coverages = raw, offsets, centers, coverages
        self.P = int(offsets.numel()) - 1
        self.n_points_max = int(n_points_max)               # the largest plot's raw points: known on the host, never read back
        self.device = raw.device
        self._consts = {}                                   # diam_meters -> fake ground points on the device
        self._cos_sin = torch.from_numpy(cos_sin_table()).to(self.device)
        self._ws = {}                                       # (stream, B, N, extra) -> workspace of standalone `fill` calls

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
        return cls(raw, offsets, torch.from_numpy(centers).to(dev), torch.from_numpy(coverages).to(dev), max(n))

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


class EpochFeeder:
    """Feeds a `TrainPipeline` (set_feeder) from a `ResidentPlots`: batch number i is batch i % steps_per_epoch of epoch
    i // steps_per_epoch, the order of an epoch is `torch.randperm(P, generator=generator)` drawn on the host once per epoch in
    epoch order (the DataLoader's RandomSampler), the last incomplete batch is dropped (`drop_last`).

    The geometry passes run ahead of training, across epoch boundaries, and with `slot_wait="device"` the host can be many batches
    ahead of the device: every epoch's order is a FRESH pinned tensor, the batch's ids are uploaded from a slice of it, and torch's
    pinned allocator keeps that memory from being handed out again before the copies that read it have run."""

    KEEP_EPOCHS = 64          # orders (and the generator states in front of them) remembered behind the newest one

    def __init__(self, plots, args, batch_size: int, seed: int, kde=None, train: bool = True, noise: bool = True, generator=None):
        self.plots, self.args, self.B = plots, args, int(batch_size)
        self.P = int(plots.P)
        self.steps_per_epoch = self.P // self.B
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
    def _order(self, epoch: int):
        while self._next_epoch <= epoch:
            state = self.generator.get_state()
            order = torch.randperm(self.P, generator=self.generator).to(torch.int32)
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
        epoch, k = self.locate(i)
        return self._order(epoch)[k * self.B:(k + 1) * self.B]

    def state_dict(self, batch: int = 0):
        """What a resumed run needs to draw batch number `batch` and everything after it again: load it into a feeder built with
        the same set, batch size and flags, and that feeder's batch 0 is this one's batch `batch`."""
        epoch, k = self.locate(batch)
        self._order(epoch)
        return {"seed": self.seed, "epoch": epoch, "batch_in_epoch": k, "generator_state": self._orders[epoch][0].clone(),
                "plots": self.P, "batch_size": self.B}

    def load_state_dict(self, sd):
        if int(sd["plots"]) != self.P or int(sd["batch_size"]) != self.B:
            raise ValueError("EpochFeeder: the state belongs to another set or batch size")
        self.seed = int(sd["seed"])
        self.epoch0 = self._next_epoch = int(sd["epoch"])
        self.batch0 = int(sd["batch_in_epoch"])
        self.generator.set_state(sd["generator_state"])
        self._orders = {}

    # ---- the device side
    def fill_slot(self, i: int, slot):
        """Batch number i into `slot` (a TrainPipeline slot dict) on the CURRENT stream: B ids up, one `ResidentPlots.fill`.  The
        slot's tensors are written through, never rebound (in group mode they are views of the pass group's tensors)."""
        epoch, _ = self.locate(i)
        host_ids = self.batch_ids(i)      # a permutation of 0 .. P-1: in range by construction
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
