"""Host-side wrappers of the C ABI (include/strata_hip.h): PyTorch-ROCm tensors in, raw device pointers across
`ctypes`, torch's current stream.  Every wrapper validates dtype / device / contiguity / shape on the host before a
kernel is launched (a kernel that faults can take the whole node down) and raises on a non-zero return code.

Names follow the reference's third-party call sites (model/point_net2.py:9): fps, radius -> ball_query,
knn_interpolate -> three_nn + the interpolation inside `fp_forward`, PointConv -> `sa_forward`.
"""
import collections
import ctypes
import functools
import math
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import FP, SA, Block, Head, LossGrad, StrataHipError, check

I32, F32, F64, I64, BF16 = torch.int32, torch.float32, torch.float64, torch.int64, torch.bfloat16


# ---- optional per-entry-point timing with HIP events on torch's current stream (the stream every kernel is launched
# on).  bench.py switches it on for the entry points whose roofline it reports; None = off (no overhead).
_timing = None


class timing:
    """with timing({"sn2_fps", ...}) as t: ... ; t.summary() -> {name: (calls, total_ms)} after a device sync."""

    def __init__(self, names=None):
        self.names = None if names is None else set(names)
        self.events = []

    def __enter__(self):
        global _timing
        self._prev, _timing = _timing, self
        return self

    def __exit__(self, *exc):
        global _timing
        _timing = self._prev

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, a, b in self.events:
            c, t = out.get(name, (0, 0.0))
            out[name] = (c + 1, t + a.elapsed_time(b))
        return out


def _call(name, *args, tag=None, key=None):
    fn = getattr(_lib.load(), name)
    t = _timing
    key = key or name                       # the name the entry point is reported under
    if tag is not None:
        key = f"{key}:{tag}"
    if t is not None and (t.names is None or key in t.names):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = fn(*args)
        b.record()
        t.events.append((key, a, b))
    else:
        rc = fn(*args)
    check(rc, name)


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    """The raw handle of torch's current stream on the current device (every entry point launches there).  Through torch's
    own raw accessor where it exists: `torch.cuda.current_stream()` builds a Stream object per call, ~2 us x 60 calls per
    eager step."""
    if _RAW_STREAM is not None:
        return _RAW_STREAM(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


_SHARED_STREAMS = {}      # (device index, name) -> stream


def shared_stream(dev, name: str) -> torch.cuda.Stream:
    """The process-wide side stream `name` of a device ("side0".."sideK": geometry passes of pipelined loops and prefetch
    lanes; "fork_b", "fork_c", "pack": the branches of an unpipelined geometry pass; "capture").  Created ONCE: HIP deals
    streams onto a few hardware queues round-robin as they are created, so a second pipeline (or model) that created its own
    streams could find two of them -- or one and the main stream -- on one queue, where the passes it meant to overlap run
    back to back (seen: +25 % per step for a pipeline built after another one in the same process).
    SINGLE OWNER AT A TIME: the streams are shared by everything in the process that asks for them by name -- a TrainPipeline,
    an eval model's prefetch lanes, bench.py's serial capture.  Two such users that are LIVE at once serialise on them (a pass
    meant to overlap another runs behind it), and a hipGraph capture on "capture" would record foreign work enqueued on it
    meanwhile: run one pipelined loop / one capture at a time per device (what bench.py and the tests do: legs run one after
    the other), or give a second concurrent user its own names."""
    dev = torch.device(dev)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), name)
    if key not in _SHARED_STREAMS:
        _SHARED_STREAMS[key] = torch.cuda.Stream(device=dev)
    return _SHARED_STREAMS[key]


def forked_streams(dev, exclude=None):
    """Names of the process's shared streams of `dev` that are part of a stream capture RIGHT NOW (hipStreamIsCapturing):
    streams a capture forked into (`side.wait_stream(capture stream)` + work on `side`)."""
    dev = torch.device(dev)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    out = []
    for (di, name), s in list(_SHARED_STREAMS.items()):
        if di != idx or (exclude is not None and s == exclude):
            continue
        with torch.cuda.stream(s):
            if torch.cuda.is_current_stream_capturing():
                out.append(name)
    return out


import contextlib as _contextlib
import gc as _gc


@_contextlib.contextmanager
def graph_capture(graph, dev, pool=None, allowed_forks=()):
    """`torch.cuda.graph(graph, pool=pool)` with the two rules this package's captures live by ENFORCED (round 5; DESIGN.md
    section 4, "the capture_end crash of round 4"):
      * a capture starts with none of the process's shared streams inside another capture (two live users of `shared_stream`
        names) -- refused with StrataHipError before anything is captured;
      * a capture ENDS with every stream it forked into joined back.  ROCm 7.2's hipStreamEndCapture does not return
        hipErrorStreamCaptureUnjoined for a stream that is still forked: it crashed the process (round 4: a loss-value branch
        on a fourth stream whose autograd node the engine ran -- and left work -- on that stream after the step's join).
        Here every shared stream found capturing at the end of the block is joined first (so the runtime never sees the
        state), and unless its name is in `allowed_forks` (streams the captured code forks into and joins itself: the
        unpipelined step's geometry branches) the graph is dropped and StrataHipError raised.
    A third rule: Python's cyclic garbage collector is OFF while the capture is open (and restored afterwards).  A collection can
    start in any thread at any allocation -- the autograd thread of a captured backward pass included -- and whatever dead cycle
    it finds is destroyed there and then: an earlier pipeline's hipGraphs with their memory pool, for one.  Destroying those while
    a capture in the global error mode is open aborted the process (the whole GPU suite, in the capture that follows `del w` in
    tests/test_gpu_train_modes.py, whenever the collector's counters happened to fire inside it).  torch.cuda.graph collected
    garbage itself BEFORE every capture up to torch 2.8; since 2.9 it does not (`torch.compiler.config.force_cudagraph_gc`), so
    dead cycles now survive into the capture.  Reference-counted frees are not affected; the cycles are collected after the capture."""
    dev = torch.device(dev)
    busy = forked_streams(dev)
    if busy:
        raise StrataHipError(f"graph_capture: shared stream(s) {busy} are already part of a stream capture: one capture at a time "
                             "per device (hip_ops.shared_stream: single owner at a time)")
    stray = []
    kw = {} if pool is None else {"pool": pool}
    gc_was_on = _gc.isenabled()
    _gc.disable()
    try:
        with torch.cuda.graph(graph, **kw):
            cap = torch.cuda.current_stream(dev)
            try:
                yield cap
            finally:
                for name in forked_streams(dev, exclude=cap):
                    cap.wait_stream(shared_stream(dev, name))  # joined: hipStreamEndCapture sees a legal graph whatever happened
                    if name not in allowed_forks:
                        stray.append(name)
    finally:
        if gc_was_on:
            _gc.enable()
    if stray:
        graph.reset()
        raise StrataHipError(f"graph_capture: the captured code left work on shared stream(s) {stray} that nothing joined back "
                             "into the capture stream (an autograd node created on a side stream runs its backward there); "
                             "the graph was dropped")


_UPLOAD_TRACE = None       # scripts/profile_dropin_host.py sets a list: (what, host ms) of every wait / copy inside PinnedRing.upload


class PinnedRing:
    """Host-to-device uploads of pageable tensors through a small ring of PINNED staging buffers.

    The reference hands `PointNet2.forward` CPU tensors from a DataLoader without `pin_memory` (`learning/train.py:33-44`,
    `model/point_net2.py:119-124` moves them with `.cuda()`): a copy from pageable memory is staged by the runtime chunk by chunk
    and blocks the host for its whole length (40 MB per step at C2: 5 of the eager loop's 5.8 ms).  Here the host copies into a
    pinned buffer itself (a multi-threaded memcpy) and the DMA runs asynchronously on the stream it is given, so the kernels
    that need only the first tensor (the geometry pass needs `xyz` only) start while the rest is still on its way.
    A slot is reused only after the DMA that read it has finished (an event per slot, waited for on the host)."""

    def __init__(self, dev, slots: int = 4):
        self.dev = torch.device(dev)
        self.bufs = [None] * slots
        self.events = [None] * slots
        self.k = 0

    def upload(self, t: torch.Tensor, stream=None, dtype=None, out=None, consumer=None) -> torch.Tensor:
        """CPU tensor -> device tensor of `dtype` (default: its own) with the same shape, copied asynchronously on `stream`
        (default: torch's current stream).  The result is safe to use on that stream; events for others are the caller's
        business.  out: the device tensor to fill -- allocate it on the stream that will CONSUME it (a 21 MB block allocated on
        a side stream and handed to the main stream with record_stream kept the caching allocator from reusing it: a fresh
        hipMalloc per step, 80 ms instead of 5), and make `stream` wait for whatever last used the block.
        consumer: the stream that will read `out` when that is not `stream`: it is made to wait for the copy here, and the
        slot's reuse event is recorded on IT.  (An event that is the last thing ever submitted to an otherwise idle side stream
        was only seen as complete by a later `event.synchronize()` after ~86 ms on ROCm 7.2 -- every third step of the eager
        loop; an event on the busy main stream completes when the stream gets there.)"""
        dtype = dtype or t.dtype
        src = t.detach()
        if src.dtype != dtype:
            src = src.to(dtype)
        src = src.contiguous()
        n = src.numel() * src.element_size()
        i = self.k
        self.k = (self.k + 1) % len(self.bufs)
        if self.events[i] is not None:
            if _UPLOAD_TRACE is not None:
                import time as _t
                a = _t.perf_counter()
                self.events[i].synchronize()
                _UPLOAD_TRACE.append(("event", (_t.perf_counter() - a) * 1e3))
            else:
                self.events[i].synchronize()                  # the DMA that last read this slot
        if self.bufs[i] is None or self.bufs[i].numel() < n:
            self.bufs[i] = torch.empty(max(n, 1 << 20), dtype=torch.uint8).pin_memory()
        stage = self.bufs[i][:n].view(dtype).view(src.shape)
        if _UPLOAD_TRACE is not None:
            import time as _t
            a = _t.perf_counter()
            stage.copy_(src)
            _UPLOAD_TRACE.append(("memcpy", (_t.perf_counter() - a) * 1e3))
        else:
            stage.copy_(src)                                  # host memcpy into pinned memory
        st = torch.cuda.current_stream(self.dev) if stream is None else stream
        allocated_here = out is None
        with torch.cuda.stream(st):
            if out is None:
                out = torch.empty(src.shape, dtype=dtype, device=self.dev)
            elif out.shape != src.shape or out.dtype != dtype or not out.is_contiguous():
                raise ValueError("PinnedRing.upload: `out` does not match the source")
            out.copy_(stage, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(st)
        if consumer is not None and consumer != st:
            consumer.wait_event(ev)
            ev = torch.cuda.Event()
            ev.record(consumer)
            if allocated_here:
                # allocated on the copy stream, read on the consumer's: the caching allocator must not hand the block to a later
                # allocation of the copy stream before the consumer is done with it.  (Two blocks then alternate from step to
                # step -- scripts/debug_side_alloc.py: no hipMalloc after the second iteration.)
                out.record_stream(consumer)
        self.events[i] = ev
        return out


_RINGS = {}


def pinned_ring(dev) -> PinnedRing:
    """The process-wide upload ring of a device."""
    dev = torch.device(dev)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _RINGS:
        _RINGS[key] = PinnedRing(dev)
    return _RINGS[key]


def create_shared_streams(dev, lanes: int = 4):
    """Create the process's side streams NOW ("side0".."side<lanes-1>", the fork / pack / capture streams), in a fixed order.
    Call it before anything else creates streams on the device (RCCL communicators, torch.distributed process groups): the
    hardware queues go to the first streams created, and a loop whose side streams come late shares queues with the
    communicator's streams (measured: 0.905 instead of 0.787 ms per step)."""
    for name in [f"side{j}" for j in range(lanes)] + ["fork_b", "fork_c", "pack", "capture", "upload"]:
        shared_stream(dev, name)


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _chk(t: torch.Tensor, dtype, shape=None, name="tensor"):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name}: expected a tensor on the HIP device")
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _chk_rows(t: torch.Tensor, dtype, rows: int, cols: int, name="rows", align: int = 4) -> int:
    """A 2-D row view (rows, >=cols) with unit inner stride; returns the row stride in elements.  Row starts must be
    16-byte aligned when align == 4 (the kernels read rows with 16-byte loads)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or t.dim() != 2:
        raise ValueError(f"{name}: expected a 2-D {dtype} tensor on the HIP device")
    if t.shape[0] != rows or t.shape[1] < cols or t.stride(1) != 1:
        raise ValueError(f"{name}: expected ({rows}, >={cols}) with unit inner stride, got {tuple(t.shape)} {t.stride()}")
    st = t.stride(0) if rows > 1 else max(t.stride(0), t.shape[1])
    if align > 1 and (st % align or (t.data_ptr() % (4 * align))):
        raise ValueError(f"{name}: rows must be {4 * align}-byte aligned")
    return st


def fps_num_samples(n: int, ratio: float) -> int:
    """ceil(fp32(n) * fp32(ratio)) -- torch-cluster 1.5.9 `fps` sample count (see oracle/primitives.py)."""
    return int(math.ceil(float(np.float32(n) * np.float32(ratio))))


def r2_threshold(r: float) -> float:
    """fp32(r*r) with r*r evaluated in double: what `radius` compares squared distances with."""
    return float(np.float32(float(r) * float(r)))


# ---------------------------------------------------------------------------------------------- geometry
def pack_rows(cloud: torch.Tensor, xyz: torch.Tensor, out: Optional[torch.Tensor] = None, feats: int = 8) -> torch.Tensor:
    """include/strata_hip.h: sn2_pack_rows_feat.  cloud (B,C,N), xyz (B,3,N) -> rows0 (B*N, feats+4) = [feats features | x y z 0];
    (C, feats) = (10, 8), (6, 4) or (10, 4) -- a ten-row cloud whose colour rows a four-feature model never reads."""
    B, C, N = cloud.shape
    _chk(cloud, F32, (B, C, N), "cloud")
    _chk(xyz, F32, (B, 3, N), "xyz")
    W = int(feats) + 4
    rows0 = torch.empty(B * N, W, dtype=F32, device=cloud.device) if out is None else _chk(out, F32, (B * N, W), "out")
    _call("sn2_pack_rows_feat", _ptr(cloud), _ptr(xyz), B, C, N, int(feats), _ptr(rows0), _stream())
    return rows0


_host = _lib.host_value      # route predicates and size helpers of the library, remembered per argument tuple


def fps_ws_words(B: int, N: int) -> int:
    """SN2_FPS_WS_WORDS of include/strata_hip.h."""
    return _host("sn2_fps_ws_words", int(B), int(N))


def fps_ws_grid(ws: torch.Tensor, B: int, N: int) -> torch.Tensor:
    """The B cell-grid headers of a filled FPS workspace (cell starts, bounding boxes, pad words)."""
    o = _host("sn2_fps_ws_grid_offset", int(B), int(N))
    return ws[o:o + _lib.SN2_FPS_WS_GRID_WORDS * B]


def fps_ws_ctl(ws: torch.Tensor, B: int, N: int) -> torch.Tensor:
    """The 32 control words of a filled FPS workspace ([1] = exchange waits of the multi-workgroup kernel that gave up in the LAST
    pass over this workspace; the process-wide running total is `fps_gave_up`)."""
    o = _host("sn2_fps_ws_ctl_offset", int(B), int(N))
    return ws[o:o + _lib.SN2_FPS_WS_CTL_WORDS]


def fps_ws_rank(ws: torch.Tensor, B: int, N: int) -> torch.Tensor:
    """The (B*N) int32 view of a filled FPS workspace that holds every point's position in the plot's spatial (Morton) order."""
    return ws[_host("sn2_fps_ws_rank_offset", int(B), int(N)):]


def fps_fills_ws(B: int, N: int, m: int) -> bool:
    """Whether sn2_fps takes its bucketed path for these sizes, i.e. FILLS the workspace (Morton order, sorted table, cell
    starts) that ball_query / three_nn may then walk (sn2_fps_fills_ws, the test sn2_fps_status itself makes): handing those
    kernels a workspace nobody filled would send them through garbage cell lists."""
    return bool(_host("sn2_fps_fills_ws", int(B), int(N), int(m)))


FPS_FORM_BRUTE, FPS_FORM_ROUND, FPS_FORM_SPEC, FPS_FORM_CLUSTER = (_lib.SN2_FPS_FORM_BRUTE, _lib.SN2_FPS_FORM_ROUND, _lib.SN2_FPS_FORM_SPEC,
                                                                   _lib.SN2_FPS_FORM_CLUSTER)
FpsRoute = collections.namedtuple("FpsRoute", [n for n, _ in _lib.FpsRoute._fields_])


@functools.lru_cache(maxsize=4096)
def _fps_route(B, N, m, waves, have_ws, cus) -> FpsRoute:
    r = _lib.FpsRoute()
    check(_lib.load().sn2_fps_route(B, N, m, waves, have_ws, cus, r), "sn2_fps_route")
    return FpsRoute(*(getattr(r, n) for n in FpsRoute._fields))


def fps_route(B: int, N: int, m: int, waves: int = 0, bucketed: bool = True, device=None) -> FpsRoute:
    """sn2_fps_route: the kernel `fps(pos_soa (B,3,N), m, waves=waves, bucketed=bucketed)` launches on `device` (None: the current
    one) -- form (FPS_FORM_*), waves per workgroup, workgroups per plot, template rung, whether the multi-workgroup kernel keeps its
    points in LDS, the repair launch's rung, whether the workspace is filled.  The plan sn2_fps_live itself runs: host arithmetic,
    nothing is launched.  bucketed=False = no workspace handed over, which is how `fps` forces the brute-force kernel."""
    cus = torch.cuda.get_device_properties(device if device is not None else torch.cuda.current_device()).multi_processor_count
    return _fps_route(int(B), int(N), int(m), int(waves), int(bool(bucketed)), int(cus))


_FPS_STATUS = {}          # device index -> [status word (1,) int32 on the device, count already reported]


class StrataHipWarning(RuntimeWarning):
    pass


def fps_status_word(dev) -> torch.Tensor:
    """The device word every `fps` call of this process hands to sn2_fps_status (include/strata_hip.h): it accumulates the
    waits of the multi-workgroup FPS kernel that gave up (each such pass is repeated by the single-workgroup kernel inside
    the same call: the samples are right either way)."""
    dev = torch.device(dev)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _FPS_STATUS:
        _FPS_STATUS[key] = [torch.zeros(1, dtype=I32, device=dev), 0]
    return _FPS_STATUS[key][0]


def fps_gave_up(dev, warn: bool = True) -> int:
    """Waits of the multi-workgroup FPS that gave up on this device since the process started.  Reads one word from the
    device: call it where the host synchronises anyway (TrainPipeline.drain, the end of predict_parcel, after a test).
    A count that grew since the last call means FPS passes are being run twice (the workgroups of the multi-workgroup
    kernel were not resident together -- another stream or process held the CUs): results are unaffected, the pass takes
    its bounded wait + the single-workgroup kernel longer; `warn` reports that once per growth as a StrataHipWarning."""
    dev = torch.device(dev)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _FPS_STATUS:
        return 0
    word, seen = _FPS_STATUS[key]
    n = int(word.item())
    if n > seen:
        _FPS_STATUS[key][1] = n
        if warn:
            import warnings
            warnings.warn(f"multi-workgroup FPS: {n - seen} exchange wait(s) gave up on {dev} and the passes were repeated by "
                          "the single-workgroup kernel (results unaffected, the passes took longer); ask for one workgroup "
                          "per plot (fps(..., waves=8 or 16)) where other kernels or processes share the device",
                          StrataHipWarning, stacklevel=2)
    return n


def fps(pos_soa: torch.Tensor, m: int, start: Optional[torch.Tensor] = None, bucketed: bool = True,
        return_ws: bool = False, out=None, waves: int = 0, n_live: Optional[torch.Tensor] = None,
        n_live_out: Optional[torch.Tensor] = None):
    """pos_soa (B,3,N) -> idx (B,m) int32 local indices, cpos_soa (B,3,m), cpos_aos (B*m,4).
    waves: which bucketed kernel (include/strata_hip.h: sn2_fps_waves): 0 = the shortest pass (several workgroups per plot
    where the batch fits the chip), 16 / 8 / 4 = one workgroup of 16 / 8 / 4 waves per plot (8 = the pass that shares its CUs with
    concurrent kernels, what the pipelined training loop asks for; 4 = the same for passes over hundreds of small plots, the
    parcel loop; plots of more than 16 384 points take 8), 32 + P / 64 + P = P workgroups of 16 / 8 waves per plot,
    1 = the one-sample-per-round kernel; same indices whichever runs.
    bucketed=False forces the brute-force kernel (same result; kept for cross-checks).  return_ws=True also returns
    the spatial-order workspace (or None), which `ball_query` over the same points can reuse.
    out = (idx, cpos_soa, cpos_aos, workspace-or-None): caller-owned result buffers (persistent pipelines).
    n_live (B) int32 on the device: the plot's live prefix (include/strata_hip.h: sn2_fps_live) -- points [n_live[b], N) of plot b
    are bit-identical copies of earlier ones, as every sampler of this package lays a short plot out; same bytes as without it,
    minus the all-ties rounds.  n_live_out (B) int32: receives the samples emitted before the maximum reached 0 (m if never),
    which is the n_live of an FPS over the returned positions."""
    B, three, N = pos_soa.shape
    _chk(pos_soa, F32, (B, 3, N), "pos_soa")
    if not (1 <= m <= N):
        raise ValueError(f"fps: need 1 <= m <= N, got m={m}, N={N}")
    if start is not None:
        _chk(start, I32, (B,), "start")
    dev = pos_soa.device
    use_ws = bucketed and fps_fills_ws(B, N, m)
    if out is not None:
        idx, cs, ca, order = out
        _chk(idx, I32, (B, m), "out idx")
        _chk(cs, F32, (B, 3, m), "out cpos_soa")
        _chk(ca, F32, (B * m, 4), "out cpos_aos")
        if order is not None:
            _chk(order, I32, (fps_ws_words(B, N),), "out workspace")
        if not use_ws:
            order = None                      # the kernel would not fill it: nobody may read it
    else:
        idx = torch.empty(B, m, dtype=I32, device=dev)
        cs = torch.empty(B, 3, m, dtype=F32, device=dev)
        ca = torch.empty(B * m, 4, dtype=F32, device=dev)
        order = torch.empty(fps_ws_words(B, N), dtype=I32, device=dev) if use_ws else None
    if n_live is None and n_live_out is None:
        _call("sn2_fps_status", _ptr(pos_soa), B, N, m, _ptr(start), _ptr(idx), _ptr(cs), _ptr(ca), _ptr(order), int(waves),
              _ptr(fps_status_word(dev)), _stream(), tag=f"N={N}", key="sn2_fps")
    else:
        if n_live is not None:
            _chk(n_live, I32, (B,), "n_live")
        if n_live_out is not None:
            _chk(n_live_out, I32, (B,), "n_live_out")
        _call("sn2_fps_live", _ptr(pos_soa), B, N, m, _ptr(start), _ptr(n_live), _ptr(idx), _ptr(cs), _ptr(ca), _ptr(order),
              int(waves), _ptr(n_live_out), _ptr(fps_status_word(dev)), _stream(), tag=f"N={N}", key="sn2_fps")
    if return_ws:
        return idx, cs, ca, order
    return idx, cs, ca


def ball_query(src_soa: torch.Tensor, cpos_soa: torch.Tensor, r: float, cap: int = _lib.MAX_NEIGHBORS,
               total: Optional[torch.Tensor] = None, fps_ws: Optional[torch.Tensor] = None, out=None):
    """-> nbr (B*M,cap) int32 (first cnt entries valid, ascending source index), cnt (B*M) int32, total (1) int64.
    out = (nbr, cnt): caller-owned result buffers."""
    B, _, N = src_soa.shape
    M = cpos_soa.shape[2]
    _chk(src_soa, F32, (B, 3, N), "src_soa")
    _chk(cpos_soa, F32, (B, 3, M), "cpos_soa")
    cap = min(cap, N)
    dev = src_soa.device
    if out is not None:
        nbr, cnt = out
        _chk(nbr, I32, (B * M, cap), "out nbr")
        _chk(cnt, I32, (B * M,), "out cnt")
    else:
        nbr = torch.empty(B * M, cap, dtype=I32, device=dev)
        cnt = torch.empty(B * M, dtype=I32, device=dev)
    if total is False:
        total = None                          # no message total wanted (a grouped pass sums the counts per batch: count_sum_group)
    elif total is None:
        total = torch.zeros(1, dtype=I64, device=dev)
    else:
        _chk(total, I64, (1,), "total")
    if fps_ws is not None:
        _chk(fps_ws, I32, (fps_ws_words(B, N),), "fps_ws")
    _call("sn2_ball_query", _ptr(src_soa), B, N, _ptr(cpos_soa), M, r2_threshold(r), cap, _ptr(nbr), _ptr(cnt), _ptr(total),
          _ptr(fps_ws), _stream(), tag=f"N={N}")
    return nbr, cnt, total


def count_sum(cnt: torch.Tensor, total: torch.Tensor):
    """include/strata_hip.h: sn2_count_sum -- total (1,) int64 = sum of the neighbour counts cnt (n,) int32."""
    _chk(cnt, I32, None, "cnt")
    _chk(total, I64, (1,), "total")
    _call("sn2_count_sum", _ptr(cnt), cnt.numel(), _ptr(total), _stream())


def count_sum_group(cnt: torch.Tensor, G: int, n: int, totals: torch.Tensor, stride: int):
    """include/strata_hip.h: sn2_count_sum_group -- totals[h * stride] = sum of cnt[h*n : (h+1)*n], h < G, in one launch."""
    _chk(cnt, I32, (G * n,), "cnt")
    _chk(totals, I64, None, "totals")
    if totals.numel() < (G - 1) * stride + 1:
        raise ValueError("count_sum_group: totals too small")
    _call("sn2_count_sum_group", _ptr(cnt), G, n, _ptr(totals), stride, _stream(), key="sn2_count_sum")


def three_nn_ws_words(B: int, S: int, T: int = 0) -> int:
    """SN2_THREE_NN_XY_WS_WORDS (T > 0) / SN2_THREE_NN_WS_WORDS (T = 0) of include/strata_hip.h."""
    return _host("sn2_three_nn_xy_ws_words", int(B), int(S), int(T)) if T else _host("sn2_three_nn_ws_words", int(B), int(S))


def three_nn_uses_grid(S: int, T: int) -> bool:
    """The grid search of sn2_three_nn_xy applies (otherwise the full scan runs): sn2_three_nn_uses_grid."""
    return bool(_host("sn2_three_nn_uses_grid", int(S), int(T)))


@functools.lru_cache(maxsize=256)
def _three_nn_order_offsets(B: int, S: int, T: int):
    order, copy = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _lib.check(_lib.load().sn2_three_nn_xy_order_offset(B, S, T, ctypes.byref(order), ctypes.byref(copy)), "sn2_three_nn_xy_order_offset")
    return order.value, copy.value


def three_nn_order(ws: torch.Tensor, B: int, S: int, T: int, sorted_copy: bool = True):
    """What the grid search `three_nn(..., ws=ws)` left in its workspace (include/strata_hip.h: sn2_three_nn_xy_order_offset):
    -> (order (B*T,) int32, idx_sorted (B*T,3) int32 or None, w_sorted (B*T,3) float32 or None), views of `ws` -- valid until the
    next search with the same workspace.  The sorted copy only where the search was asked for it (`sorted_copy=True` there)."""
    o, c = _three_nn_order_offsets(int(B), int(S), int(T))
    n = B * T
    order = ws[o:o + n]
    if not sorted_copy:
        return order, None, None
    return order, ws[c:c + 3 * n].view(n, 3), ws[c + 3 * n:c + 6 * n].view(torch.float32).view(n, 3)


def three_nn(src_soa: torch.Tensor, dst_soa: torch.Tensor, k: int, out=None, grid: bool = True, ws=None,
             dst_fps_ws: Optional[torch.Tensor] = None, sorted_copy: bool = False):
    """-> idx (B*T,3) int32 local source indices, w (B*T,3) = 1/max(d2,1e-16) (0 on unused slots).
    out = (idx, w): caller-owned result buffers.
    grid=True: where `three_nn_uses_grid(S, T)` the search walks a per-plot x,y grid of the sources, a wave taking
    64 targets of adjacent grid cells (sn2_three_nn_xy sorts the targets by cell itself; same result as the full scan, bit
    for bit); ws: caller-owned workspace of three_nn_ws_words(B, S, T) int32 for it (allocated here when None).
    sorted_copy: the grid search also leaves its result rows in its own order in `ws`, for the inverted index that follows
    (`three_nn_order`, `interp_index(..., row_order=)`); ignored where the full scan runs.
    dst_fps_ws (with grid=True): use the order `fps(..., return_ws=True)` left for the TARGET points instead of the
    cell sort (the first form of the grid search, kept for cross-checks); grid=False forces the full scan."""
    B, _, S = src_soa.shape
    T = dst_soa.shape[2]
    _chk(src_soa, F32, (B, 3, S), "src_soa")
    _chk(dst_soa, F32, (B, 3, T), "dst_soa")
    dev = src_soa.device
    if out is not None:
        idx, w = out
        _chk(idx, I32, (B * T, 3), "out idx")
        _chk(w, F32, (B * T, 3), "out w")
    else:
        idx = torch.empty(B * T, 3, dtype=I32, device=dev)
        w = torch.empty(B * T, 3, dtype=F32, device=dev)
    if grid and three_nn_uses_grid(S, T) and dst_fps_ws is None:
        n = three_nn_ws_words(B, S, T)
        if ws is None:
            ws = torch.empty(n, dtype=I32, device=dev)
        else:
            _chk(ws, I32, (n,), "ws")
        _call("sn2_three_nn_xy_copy", _ptr(src_soa), B, S, _ptr(dst_soa), T, k, _ptr(idx), _ptr(w), _ptr(ws), int(bool(sorted_copy)),
              _stream(), tag=f"T={T}", key="sn2_three_nn_xy")
        return idx, w
    if grid and dst_fps_ws is not None and three_nn_uses_grid(S, T):
        if ws is None:
            ws = torch.empty(three_nn_ws_words(B, S), dtype=I32, device=dev)
        elif ws.numel() < three_nn_ws_words(B, S):
            raise ValueError("three_nn: workspace too small")
        _chk(dst_fps_ws, I32, (fps_ws_words(B, T),), "dst_fps_ws")
    else:
        ws = dst_fps_ws = None
    _call("sn2_three_nn", _ptr(src_soa), B, S, _ptr(dst_soa), T, k, _ptr(idx), _ptr(w), _ptr(ws), _ptr(dst_fps_ws), _stream(),
          tag=f"T={T}")
    return idx, w


# ---------------------------------------------------------------------------------------------- blocks
class BlockBuffers:
    """Device-side companions of one (Linear -> ReLU -> BatchNorm1d) block: affine (a, c), saved batch statistics,
    fp64 accumulators.  `params` = (W, b, gamma, beta, running_mean, running_var) tensors of the nn modules."""

    def __init__(self, lin: torch.nn.Linear, bn: torch.nn.BatchNorm1d, aux: Optional[torch.Tensor] = None,
                 stats: Optional[torch.Tensor] = None):
        self.lin, self.bn = lin, bn
        self.cin, self.cout = lin.in_features, lin.out_features
        dev = lin.weight.device
        # aux rows: a, c, mean, invstd (fp32);  stats: per-workgroup batch-statistics slots (no initialisation needed)
        self.aux = torch.empty(4, self.cout, dtype=F32, device=dev) if aux is None else aux
        self.stats = torch.empty(_lib.STAT_SLOTS * 2 * self.cout, dtype=F32, device=dev) if stats is None else stats
        _chk(self.aux, F32, (4, self.cout), "aux")
        _chk(self.stats, F32, (_lib.STAT_SLOTS * 2 * self.cout,), "stat_slots")
        self.grads = None                                                 # (dW, db, dgamma, dbeta) views, set per backward
        self.grad_images = (1, 0)                                         # (replicas, stride in floats) of dW / db
        self.mma_bf16 = False                                             # bfloat16 operands on the matrix cores (sn2_block.mma_bf16)
        self.frozen = False                                               # the forward ran on the running statistics (sn2_block.frozen_stats)

    def fill(self, blk: Block, with_grads: bool = False):
        for t, n in ((self.lin.weight, "weight"), (self.lin.bias, "bias"), (self.bn.weight, "bn.weight"),
                     (self.bn.bias, "bn.bias"), (self.bn.running_mean, "running_mean"),
                     (self.bn.running_var, "running_var")):
            _chk(t, F32, None, n)
        blk.cin, blk.cout = self.cin, self.cout
        blk.mma_bf16 = int(bool(self.mma_bf16))
        blk.frozen_stats = int(bool(self.frozen))
        blk.W, blk.b = _ptr(self.lin.weight), _ptr(self.lin.bias)
        blk.gamma, blk.beta = _ptr(self.bn.weight), _ptr(self.bn.bias)
        blk.running_mean, blk.running_var = _ptr(self.bn.running_mean), _ptr(self.bn.running_var)
        blk.a, blk.c, blk.mean, blk.invstd = (_ptr(self.aux[i]) for i in range(4))
        blk.stat_slots = _ptr(self.stats)
        nbt = self.bn.num_batches_tracked
        if nbt is not None:
            _chk(nbt, I64, None, "num_batches_tracked")
        blk.num_batches_tracked = _ptr(nbt) if nbt is not None else None
        if with_grads:
            dW, db, dg, dbeta = self.grads
            for t, ref in ((dW, self.lin.weight), (db, self.lin.bias), (dg, self.bn.weight), (dbeta, self.bn.bias)):
                _chk(t, F32, ref.shape, "grad view")
            blk.dW, blk.db, blk.dgamma, blk.dbeta = _ptr(dW), _ptr(db), _ptr(dg), _ptr(dbeta)
            blk.grad_replicas, blk.grad_replica_stride = self.grad_images
        else:
            blk.dW = blk.db = blk.dgamma = blk.dbeta = None
            blk.grad_replicas, blk.grad_replica_stride = 1, 0

    @property
    def a(self):
        return self.aux[0]

    @property
    def c(self):
        return self.aux[1]


def prepare_plots(raw, offsets, centers, fake_xy, idx, z_max: float, rot=None, flips=None, noise=None, noise_offsets=None):
    """include/strata_hip.h: sn2_prepare_plots.  raw (10,T) f32, offsets (B+1) i32, centers (B,2) f32, fake_xy (F,2) f32,
    idx (B,N) i32; train iff rot (B,2) f64 and flips (B,2) i32 are given; noise (6,Tn) f32 + noise_offsets (B) i64 optional.
    -> cloud (B,10,N), xyz (B,3,N)."""
    C, T = raw.shape
    B, N = idx.shape
    _chk(raw, F32, (10, T), "raw")
    _chk(offsets, I32, (B + 1,), "offsets")
    _chk(centers, F32, (B, 2), "centers")
    F = fake_xy.shape[0]
    _chk(fake_xy, F32, (F, 2), "fake_xy")
    _chk(idx, I32, (B, N), "idx")
    train = rot is not None
    if train:
        _chk(rot, F64, (B, 2), "rot")
        _chk(flips, I32, (B, 2), "flips")
    Tn = 0
    if noise is not None:
        Tn = noise.shape[1]
        _chk(noise, F32, (6, Tn), "noise")
        _chk(noise_offsets, I64, (B,), "noise_offsets")
    dev = raw.device
    cloud = torch.empty(B, 10, N, dtype=F32, device=dev)
    xyz = torch.empty(B, 3, N, dtype=F32, device=dev)
    _call("sn2_prepare_plots", _ptr(raw), T, _ptr(offsets), _ptr(centers), _ptr(fake_xy), F, _ptr(idx), B, N, int(train),
          _ptr(rot), _ptr(flips), _ptr(noise), _ptr(noise_offsets), Tn, float(z_max), _ptr(cloud), _ptr(xyz), _stream())
    return cloud, xyz


SUBSAMPLE_LDS, SUBSAMPLE_GLOBAL, SUBSAMPLE_COARSE = _lib.SN2_SUBSAMPLE_LDS, _lib.SN2_SUBSAMPLE_GLOBAL, _lib.SN2_SUBSAMPLE_COARSE
SUBSAMPLE_LDS_MAX = _lib.SN2_SUBSAMPLE_LDS_MAX


def subsample_form(n_max: int, N: int) -> int:
    """The form sn2_subsample takes for plots of at most n_max candidates when none is forced (sn2_subsample_form):
    SUBSAMPLE_LDS (one workgroup per plot, pairs in LDS) or SUBSAMPLE_GLOBAL (four launches over a workspace)."""
    return int(_lib.load().sn2_subsample_form(int(n_max), int(N)))


def subsample_ws_words(B: int, n_max: int, N: int, form: int = 0) -> int:
    """sn2_subsample_ws_words of include/strata_hip.h (0: the LDS form needs no workspace)."""
    return int(_lib.load().sn2_subsample_ws_words(int(B), int(n_max), int(N), int(form)))


def subsample(offsets, extra: int, N: int, seed: int, plot_keys, n_max: Optional[int] = None, form: int = 0):
    """include/strata_hip.h: sn2_subsample.  offsets (B+1) i32, plot_keys (B) i64 -> idx (B,N) i32 for prepare_plots: per plot
    the N candidates (of its offsets[b+1] - offsets[b] + extra) with the smallest Philox keys u(seed, plot_keys[b], i) in key
    order, or all of them followed by draws with replacement.  n_max: the caller's host-side bound on a plot's candidates
    (None: read from `offsets`, one small sync).  form: 0, or a SUBSAMPLE_* form for the tests (same bytes)."""
    _chk(offsets, I32, None, "offsets")
    if offsets.dim() != 1 or offsets.numel() < 2:
        raise ValueError("offsets: expected (B+1,) with B >= 1")
    B = offsets.numel() - 1
    _chk(plot_keys, I64, (B,), "plot_keys")
    extra, N, seed, form = int(extra), int(N), int(seed), int(form)
    if N <= 0 or extra < 0:
        raise ValueError("subsample: N must be positive and extra non-negative")
    if not 0 <= seed < 2 ** 64:
        raise ValueError("subsample: seed must fit 64 unsigned bits")
    if n_max is None:
        n_max = int((offsets[1:] - offsets[:-1]).max()) + extra
    n_max = int(n_max)
    if n_max <= 0 or n_max >= 2 ** 31:
        raise ValueError("subsample: n_max must be in 1 .. 2^31 - 1 (a plot needs at least one candidate)")
    if form not in (0, 1, 2, 5, 6):
        raise ValueError("subsample: form must be 0, SUBSAMPLE_LDS or SUBSAMPLE_GLOBAL (| SUBSAMPLE_COARSE)")
    if form & 3 == SUBSAMPLE_LDS and n_max > SUBSAMPLE_LDS_MAX:
        raise ValueError(f"subsample: the LDS form takes at most {SUBSAMPLE_LDS_MAX} candidates per plot")
    dev = offsets.device
    nw = subsample_ws_words(B, n_max, N, form)
    ws = torch.empty(nw + 4, dtype=I32, device=dev) if nw else None
    idx = torch.empty(B, N, dtype=I32, device=dev)
    _call("sn2_subsample", _ptr(offsets), extra, n_max, B, N, seed, _ptr(plot_keys), form, _ptr(ws), nw, _ptr(idx), _stream())
    return idx


def train_batch_ws_words(B: int, n_max: int, N: int) -> int:
    """sn2_train_batch_ws_words of include/strata_hip.h: the 32-bit words of sn2_train_batch's workspace."""
    words = ctypes.c_size_t()
    check(_lib.load().sn2_train_batch_ws_words(int(B), int(n_max), int(N), ctypes.byref(words)), "sn2_train_batch_ws_words")
    return int(words.value)


def train_batch(raw, offsets, centers, coverages, plot_ids, fake_xy, n_max: int, M1: int, z_max: float, seed: int, epoch: int,
                cos_sin, cloud, xyz, gt, fps_start, ws, train: bool = True, noise: bool = True, n_live=None):
    """include/strata_hip.h: sn2_train_batch.  The resident set raw (10,T) f32, offsets (P+1) i32, centers (P,2) f32, coverages
    (P,4) f64; plot_ids (B) i32 ON THE DEVICE -- the caller has checked 0 <= id < P on the host copy it uploaded (no kernel does);
    cos_sin (360,2) f64; ws: i32, at least train_batch_ws_words(B, n_max, N) elements.  Writes cloud (B,10,N), xyz (B,3,N), gt (B,4)
    f64 and fps_start (2,B) i32 in place, on the current stream, without a host read.  n_live (B) i32 or None: also the plots'
    live prefixes min(points + fake points, N) (sn2_train_batch_live: what `fps(..., n_live=)` takes)."""
    _, T = raw.shape
    P = offsets.numel() - 1
    B, _, N = cloud.shape
    _chk(raw, F32, (10, T), "raw")
    _chk(offsets, I32, (P + 1,), "offsets")
    _chk(centers, F32, (P, 2), "centers")
    _chk(coverages, F64, (P, 4), "coverages")
    _chk(plot_ids, I32, (B,), "plot_ids")
    F = fake_xy.shape[0]
    _chk(fake_xy, F32, (F, 2), "fake_xy")
    _chk(cos_sin, F64, (360, 2), "cos_sin")
    _chk(cloud, F32, (B, 10, N), "cloud")
    _chk(xyz, F32, (B, 3, N), "xyz")
    _chk(gt, F64, (B, 4), "gt")
    _chk(fps_start, I32, (2, B), "fps_start")
    _chk(ws, I32, None, "ws")
    seed, epoch, n_max, M1 = int(seed), int(epoch), int(n_max), int(M1)
    if not 0 <= seed < 2 ** 64 or not 0 <= epoch < 2 ** 31:
        raise ValueError("train_batch: seed must fit 64 unsigned bits and epoch 31")
    if P < 1 or B < 1 or N < 1 or not 0 < n_max < 2 ** 31 or not 0 < M1 <= N:
        raise ValueError("train_batch: need P, B, N >= 1, 0 < n_max < 2^31 and 0 < M1 <= N")
    need = train_batch_ws_words(B, n_max, N)
    if ws.dim() != 1 or ws.numel() < need or ws.data_ptr() % 16:
        raise ValueError(f"train_batch: ws must be a 16-byte aligned 1-D int32 tensor of at least {need} elements")
    args = (_ptr(raw), T, _ptr(offsets), _ptr(centers), _ptr(coverages), P, _ptr(plot_ids), B, _ptr(fake_xy), F,
            n_max, N, M1, float(z_max), seed, epoch, _ptr(cos_sin), int(bool(train)), int(bool(noise)), _ptr(ws), ws.numel(),
            _ptr(cloud), _ptr(xyz), _ptr(gt), _ptr(fps_start))
    if n_live is None:
        _call("sn2_train_batch", *args, _stream())
    else:
        _chk(n_live, I32, (B,), "n_live")
        _call("sn2_train_batch_live", *args, _ptr(n_live), _stream())


def plots_append(src_raw, src_offsets, src_centers, src_cov, sel, dst_raw, dst_offsets, dst_centers, dst_cov, P0: int, T0: int,
                 dst_start, new_T: int):
    """include/strata_hip.h: sn2_plots_append.  Source plot list src_raw (10,src_T) f32, src_offsets (Ps+1) i32, src_centers (Ps,2)
    f32, src_cov (Ps,4) f32; sel (K) i32 ON THE DEVICE -- the caller has checked 0 <= sel < Ps on the host copy it uploaded (no
    kernel does); the destination arena dst_raw (10,cap_T) f32, dst_offsets (cap_P+1) i32, dst_centers (cap_P,2) f32, dst_cov
    (cap_P,4) f64 holds P0 plots / T0 points; dst_start (K+1) i32 on the device, dst_start[0] = T0 and dst_start[K] = new_T.
    Appends in place, on the current stream, without a host read."""
    _, src_T = src_raw.shape
    Ps = src_offsets.numel() - 1
    K = sel.numel()
    _, cap_T = dst_raw.shape
    cap_P = dst_offsets.numel() - 1
    _chk(src_raw, F32, (10, src_T), "src_raw")
    _chk(src_offsets, I32, (Ps + 1,), "src_offsets")
    _chk(src_centers, F32, (Ps, 2), "src_centers")
    _chk(src_cov, F32, (Ps, 4), "src_cov")
    _chk(sel, I32, (K,), "sel")
    _chk(dst_raw, F32, (10, cap_T), "dst_raw")
    _chk(dst_offsets, I32, (cap_P + 1,), "dst_offsets")
    _chk(dst_centers, F32, (cap_P, 2), "dst_centers")
    _chk(dst_cov, F64, (cap_P, 4), "dst_cov")
    _chk(dst_start, I32, (K + 1,), "dst_start")
    P0, T0, new_T = int(P0), int(T0), int(new_T)
    if K < 1 or Ps < 1 or P0 < 0 or P0 + K > cap_P or not 0 <= T0 <= new_T <= cap_T:
        raise ValueError("plots_append: need K, Ps >= 1, 0 <= P0, P0 + K <= the plot capacity and 0 <= T0 <= new_T <= the point "
                         "capacity")
    _call("sn2_plots_append", _ptr(src_raw), src_T, _ptr(src_offsets), _ptr(src_centers), _ptr(src_cov), _ptr(sel), K, _ptr(dst_raw),
          cap_T, _ptr(dst_offsets), _ptr(dst_centers), _ptr(dst_cov), cap_P, P0, T0, _ptr(dst_start), new_T, _stream())


def znorm(xyz: torch.Tensor, radius: float):
    """xyz (3,n) fp32 of ONE raw plot on the device -> (zmin (n), z - zmin (n)): the local-minimum z-normalisation of
    `normalize_z_with_minz_in_a_radius` (utils/load_data.py:237-249)."""
    _, n = xyz.shape
    _chk(xyz, F32, (3, n), "xyz")
    if not radius > 0:
        raise ValueError("znorm: radius must be positive")
    lo = xyz[:2].min(1).values.tolist()          # the caller usually has the bounding box already; here one small sync
    hi = xyz[:2].max(1).values.tolist()
    cells = (int((hi[0] - lo[0]) / radius) + 2) * (int((hi[1] - lo[1]) / radius) + 2)
    ws = torch.empty(_host("sn2_znorm_ws_words", n, cells), dtype=I32, device=xyz.device)
    zmin = torch.empty(n, dtype=F32, device=xyz.device)
    zout = torch.empty(n, dtype=F32, device=xyz.device)
    _call("sn2_znorm", _ptr(xyz[0]), _ptr(xyz[1]), _ptr(xyz[2]), n, float(radius), lo[0], lo[1], hi[0], hi[1], _ptr(ws),
          _ptr(zmin), _ptr(zout), _stream())
    return zmin, zout


# ---------------------------------------------------------------------------------------------- parcel plots
def parcel_count_ws_words(P: int, rows: int) -> int:
    """sn2_parcel_count_ws_words of include/strata_hip.h."""
    return int(_lib.load().sn2_parcel_count_ws_words(int(P), int(rows)))


def parcel_znorm_ws_words(T: int, radius: float, x_min: float, y_min: float, x_max: float, y_max: float) -> int:
    """sn2_parcel_znorm_ws_words of include/strata_hip.h (0: the z-norm grid would exceed 2^26 cells)."""
    return int(_lib.load().sn2_parcel_znorm_ws_words(int(T), float(radius), float(x_min), float(y_min), float(x_max),
                                                     float(y_max)))


def _chk_center_grid(grid, P: int):
    """grid: (cell_start (GX*GY+1) i32, cell_items i32, GX, GY, gx0, gy0, cell_inv) -- the CSR of the plot centres over
    square cells (parcel.center_grid)."""
    start, items, GX, GY, gx0, gy0, inv = grid
    _chk(start, I32, (GX * GY + 1,), "cell_start")
    _chk(items, I32, None, "cell_items")
    if items.dim() != 1 or items.numel() < 1 or items.numel() > P:
        raise ValueError("cell_items: expected 1..P centre ids")
    return start, items, int(GX), int(GY), float(gx0), float(gy0), float(inv)


def parcel_count(cloud: torch.Tensor, centers: torch.Tensor, grid, radius: float, L: int, rows: int):
    """include/strata_hip.h: sn2_parcel_count.  cloud (10,T) f32, centers (P,2) f32 -> (prefix (P*rows+1) i32: exclusive
    starts of the (plot, row) counts, plot-major; total (1) i64: all hits)."""
    _, T = cloud.shape
    _chk(cloud, F32, (10, T), "cloud")
    P = centers.shape[0]
    _chk(centers, F32, (P, 2), "centers")
    start, items, GX, GY, gx0, gy0, inv = _chk_center_grid(grid, P)
    dev = cloud.device
    nw = parcel_count_ws_words(P, rows)
    ws = torch.empty(nw + 4, dtype=I32, device=dev)
    prefix = torch.empty(P * rows + 1, dtype=I32, device=dev)
    total = torch.empty(1, dtype=I64, device=dev)
    _call("sn2_parcel_count", _ptr(cloud), T, int(L), int(rows), _ptr(centers), P, _ptr(start), _ptr(items), GX, GY, gx0, gy0,
          inv, float(radius), _ptr(ws), nw, _ptr(prefix), _ptr(total), _stream())
    return prefix, total


def parcel_fill(cloud: torch.Tensor, centers: torch.Tensor, grid, radius: float, L: int, rows: int, prefix: torch.Tensor,
                plot_base: torch.Tensor, sum_n: int):
    """include/strata_hip.h: sn2_parcel_fill.  prefix: parcel_count's (consumed); plot_base (P) i32, INT_MIN = plot dropped.
    -> raw (10,sum_n) f32 (z row not written: parcel_znorm), point_index (sum_n) i32."""
    _, T = cloud.shape
    _chk(cloud, F32, (10, T), "cloud")
    P = centers.shape[0]
    _chk(centers, F32, (P, 2), "centers")
    start, items, GX, GY, gx0, gy0, inv = _chk_center_grid(grid, P)
    _chk(prefix, I32, (P * rows + 1,), "prefix")
    _chk(plot_base, I32, (P,), "plot_base")
    dev = cloud.device
    raw = torch.empty(10, sum_n, dtype=F32, device=dev)
    pidx = torch.empty(sum_n, dtype=I32, device=dev)
    _call("sn2_parcel_fill", _ptr(cloud), T, int(L), int(rows), _ptr(centers), P, _ptr(start), _ptr(items), GX, GY, gx0, gy0,
          inv, float(radius), _ptr(prefix), _ptr(plot_base), int(sum_n), _ptr(raw), _ptr(pidx), _stream())
    return raw, pidx


def parcel_znorm(cloud: torch.Tensor, bbox, radius: float, disc_radius: float, offsets: torch.Tensor, centers: torch.Tensor,
                 point_index: torch.Tensor, raw: torch.Tensor):
    """include/strata_hip.h: sn2_parcel_znorm.  Writes raw's z row (in place): each plot point's z minus the least z within
    `radius` among the points of its own disc.  bbox = (x_min, y_min, x_max, y_max) of the parcel (fp32 values)."""
    _, T = cloud.shape
    _chk(cloud, F32, (10, T), "cloud")
    P = centers.shape[0]
    _chk(centers, F32, (P, 2), "centers")
    _chk(offsets, I32, (P + 1,), "offsets")
    sum_n = point_index.shape[0]
    _chk(point_index, I32, (sum_n,), "point_index")
    _chk(raw, F32, (10, sum_n), "raw")
    nw = parcel_znorm_ws_words(T, radius, *bbox)
    if nw == 0:
        raise ValueError("parcel_znorm: the parcel's extent needs more than 2^26 cells of the z-norm radius")
    ws = torch.empty(nw + 4, dtype=I32, device=cloud.device)
    _call("sn2_parcel_znorm", _ptr(cloud), T, *[float(v) for v in bbox], float(radius), float(disc_radius), _ptr(offsets),
          _ptr(centers), P, _ptr(point_index), sum_n, _ptr(ws), nw, _ptr(raw), _stream())
    return raw


# ---- K parcels at once (include/strata_hip.h, "the plots of K parcels in one pass"; csrc/parcels.hip) --------------------------
def pack_upload(arrays, device):
    """Host arrays -> their device copies through ONE host-to-device copy: the arrays' bytes laid end to end at 16-byte
    boundaries, uploaded, and viewed again with each array's dtype and shape."""
    arrays = [np.ascontiguousarray(a) for a in arrays]
    offs, n = [], 0
    for a in arrays:
        offs.append(n)
        n += (a.nbytes + 15) // 16 * 16
    blob = np.zeros(max(n, 16), dtype=np.uint8)
    for a, o in zip(arrays, offs):
        blob[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    dev = torch.from_numpy(blob).to(device)
    return [dev[o:o + a.nbytes].view(torch.from_numpy(a).dtype).view(a.shape) for a, o in zip(arrays, offs)]


def parcels_bbox_starts(T) -> np.ndarray:
    """The (2, K+1) int64 `starts` of sn2_parcels_bbox for clouds of T[k] points: point_start, then the workgroup prefix."""
    T = np.asarray(T, dtype=np.int64).reshape(-1)
    chunk = _lib.SN2_PARCELS_BBOX_CHUNK
    return np.stack([np.concatenate([[0], np.cumsum(T)]), np.concatenate([[0], np.cumsum((T + chunk - 1) // chunk)])]).astype(np.int64)


def parcels_bbox_identity(K: int) -> np.ndarray:
    """(K,4) uint32: the state sn2_parcels_bbox starts from (nothing folded in yet), as int32 words."""
    return np.tile(np.array([-1, -1, 0, 0], dtype=np.int32), (int(K), 1))


def parcels_bbox_decode(state: np.ndarray) -> np.ndarray:
    """The order-preserving integers of sn2_parcels_bbox's state -> (K,4) float32 x_min, y_min, x_max, y_max."""
    u = np.ascontiguousarray(state).view(np.uint32)
    return np.where(u >> 31 == 1, u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32).view(np.float32)


def parcels_bbox(arena: torch.Tensor, starts_host: np.ndarray, starts_dev: torch.Tensor, state: torch.Tensor) -> torch.Tensor:
    """include/strata_hip.h: sn2_parcels_bbox.  arena (10,T_all) f32; starts as `parcels_bbox_starts`, on the host and on the
    device; state (K,4) i32 words, folded into in place (one launch) and returned: `parcels_bbox_decode` its host copy."""
    _, T_all = arena.shape
    _chk(arena, F32, (10, T_all), "arena")
    K = starts_host.shape[1] - 1
    _chk(starts_dev, I64, (2, K + 1), "starts")
    _chk(state, I32, (K, 4), "state")
    starts_host = np.ascontiguousarray(starts_host, dtype=np.int64)
    _call("sn2_parcels_bbox", _ptr(arena), T_all, K, starts_host.ctypes.data, _ptr(starts_dev), _ptr(state), _stream())
    return state


class ParcelTable:
    """The parcel table of K clouds in one arena on the host (`host`, numpy (K+1, SN2_PARCELS_COLS) int64) and, once uploaded, on
    the device (`dev`): what the sn2_parcels_* entry points take.  T, P: points and plot centres per parcel; grids: per parcel
    `parcel.center_grid`'s tuple or None (P[k] = 0); boxes (K,4) fp32; radius, zradius: disc and z-norm radius.  Host arithmetic
    (sn2_parcels_table); SN2_EINVAL / SN2_ELIMIT raise.  L, count_ws_words, znorm_ws_words as the library states them."""

    def __init__(self, T, P, grids, boxes, radius: float, zradius: float):
        T = np.ascontiguousarray(np.asarray(T, dtype=np.int64).reshape(-1))
        K = len(T)
        P = np.ascontiguousarray(np.asarray(P, dtype=np.int64).reshape(-1))
        boxes = np.ascontiguousarray(np.asarray(boxes, dtype=np.float32).reshape(-1, 4))
        if len(P) != K or len(grids) != K or len(boxes) != K:
            raise ValueError("ParcelTable: T, P, grids and boxes need one entry per parcel")
        if K and (P.max() >= 2 ** 31 or P.min() < 0):
            raise ValueError("ParcelTable: P must fit a non-negative int32")
        gxy = np.zeros((K, 2), dtype=np.int32)
        geo = np.zeros((K, 3), dtype=np.float64)
        for k, g in enumerate(grids):
            if (g is None) != (P[k] == 0):
                raise ValueError("ParcelTable: a parcel has a centre grid iff it has centres")
            if g is not None:
                gxy[k] = g[2:4]
                geo[k] = g[4:7]
        GX, GY = np.ascontiguousarray(gxy[:, 0]), np.ascontiguousarray(gxy[:, 1])
        self.host = np.zeros((K + 1, _lib.SN2_PARCELS_COLS), dtype=np.int64)
        L, cw, zw = ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
        p32 = P.astype(np.int32)
        check(_lib.load().sn2_parcels_table(K, T.ctypes.data, p32.ctypes.data, GX.ctypes.data, GY.ctypes.data, geo.ctypes.data,
                                            boxes.ctypes.data, float(radius), float(zradius), self.host.ctypes.data, ctypes.byref(L),
                                            ctypes.byref(cw), ctypes.byref(zw)), "sn2_parcels_table")
        self.K, self.L, self.count_ws_words, self.znorm_ws_words = K, L.value, cw.value, zw.value
        self.radius, self.zradius = float(radius), float(zradius)
        last = self.host[K]
        self.T_all, self.rows, self.P_all, self.entries, self.csr_words, self.zcells = (int(last[c]) for c in (0, 2, 3, 5, 6, 12))
        self.dev = None


def _chk_parcels(arena, table: ParcelTable):
    _chk(arena, F32, (10, table.T_all), "arena")
    _chk(table.dev, I64, (table.K + 1, _lib.SN2_PARCELS_COLS), "table.dev")


def parcels_count(arena: torch.Tensor, table: ParcelTable, centers: torch.Tensor, cell_start: torch.Tensor, cell_items: torch.Tensor):
    """include/strata_hip.h: sn2_parcels_count.  centers (P_all,2) f32, cell_start (csr_words) i32, cell_items i32: the parcels'
    centres and centre grids end to end -> (prefix (entries+1) i32, plot_start (P_all+1) i64 with the total last)."""
    _chk_parcels(arena, table)
    _chk(centers, F32, (table.P_all, 2), "centers")
    _chk(cell_start, I32, (table.csr_words,), "cell_start")
    _chk(cell_items, I32, None, "cell_items")
    dev = arena.device
    ws = torch.empty(table.count_ws_words + 4, dtype=I32, device=dev)
    prefix = torch.empty(table.entries + 1, dtype=I32, device=dev)
    starts = torch.empty(table.P_all + 2, dtype=I64, device=dev)           # plot_start, then the scan's own total word
    _call("sn2_parcels_count", _ptr(arena), table.K, table.host.ctypes.data, _ptr(table.dev), _ptr(centers), _ptr(cell_start),
          _ptr(cell_items), table.radius, _ptr(ws), table.count_ws_words, _ptr(prefix), _ptr(starts[table.P_all + 1:]), _ptr(starts),
          _stream())
    return prefix, starts[:table.P_all + 1]


def parcels_fill(arena: torch.Tensor, table: ParcelTable, centers: torch.Tensor, cell_start: torch.Tensor, cell_items: torch.Tensor,
                 prefix: torch.Tensor, plot_base: torch.Tensor, sum_n: int):
    """include/strata_hip.h: sn2_parcels_fill.  prefix: parcels_count's (consumed); plot_base (P_all) i32, INT_MIN = plot dropped
    -> raw (10,sum_n) f32 (z row not written: parcels_znorm), point_index (sum_n) i32, relative to the plot's own parcel."""
    _chk_parcels(arena, table)
    _chk(centers, F32, (table.P_all, 2), "centers")
    _chk(cell_start, I32, (table.csr_words,), "cell_start")
    _chk(cell_items, I32, None, "cell_items")
    _chk(prefix, I32, (table.entries + 1,), "prefix")
    _chk(plot_base, I32, (table.P_all,), "plot_base")
    raw = torch.empty(10, sum_n, dtype=F32, device=arena.device)
    pidx = torch.empty(sum_n, dtype=I32, device=arena.device)
    _call("sn2_parcels_fill", _ptr(arena), table.K, table.host.ctypes.data, _ptr(table.dev), _ptr(centers), _ptr(cell_start),
          _ptr(cell_items), table.radius, _ptr(prefix), _ptr(plot_base), int(sum_n), _ptr(raw), _ptr(pidx), _stream())
    return raw, pidx


def parcels_znorm(arena: torch.Tensor, table: ParcelTable, offsets: torch.Tensor, centers: torch.Tensor, plot_parcel: torch.Tensor,
                  point_index: torch.Tensor, raw: torch.Tensor):
    """include/strata_hip.h: sn2_parcels_znorm.  offsets (P+1) i32, centers (P,2) f32, plot_parcel (P) i32 of the KEPT plots.
    Writes raw's z row in place, plot by plot as `parcel_znorm` does for the plot's own parcel."""
    _chk_parcels(arena, table)
    P = centers.shape[0]
    _chk(centers, F32, (P, 2), "centers")
    _chk(offsets, I32, (P + 1,), "offsets")
    _chk(plot_parcel, I32, (P,), "plot_parcel")
    sum_n = point_index.shape[0]
    _chk(point_index, I32, (sum_n,), "point_index")
    _chk(raw, F32, (10, sum_n), "raw")
    ws = torch.empty(table.znorm_ws_words + 4, dtype=I32, device=arena.device)
    _call("sn2_parcels_znorm", _ptr(arena), table.K, table.host.ctypes.data, _ptr(table.dev), table.zradius, table.radius, _ptr(offsets),
          _ptr(centers), _ptr(plot_parcel), P, _ptr(point_index), sum_n, _ptr(ws), table.znorm_ws_words, _ptr(raw), _stream())
    return raw


def sa_order_len(B: int, M: int) -> int:
    """SN2_SA_ORDER_WORDS of include/strata_hip.h."""
    return _host("sn2_sa_order_words", int(B), int(M))


def sa_order(cnt: torch.Tensor, B: int, M: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cnt (B*M) from ball_query -> the work items of the SA passes (include/strata_hip.h: sn2_sa_order): solo centroids
    with long lists, quads of centroids with medium ones, and eight / sixteen centroids with at most 8 / 4 neighbours packed into
    one step, heaviest first."""
    _chk(cnt, I32, (B * M,), "cnt")
    n = sa_order_len(B, M)
    if out is None:
        out = torch.empty(n, dtype=I32, device=cnt.device)
    else:
        _chk(out, I32, (n,), "out order")
    _call("sn2_sa_order", _ptr(cnt), B, M, _ptr(out), _stream())
    return out


def sa_order_group(cnt: torch.Tensor, G: int, B: int, M: int, out_all: torch.Tensor, stride: int):
    """include/strata_hip.h: sn2_sa_order_group -- the work items of G consecutive batches of B plots in one launch pair; batch h's
    table = out_all[h * stride : h * stride + sa_order_len(B, M)]."""
    _chk(cnt, I32, (G * B * M,), "cnt")
    if stride < sa_order_len(B, M):
        raise ValueError("sa_order_group: stride smaller than a table")
    _chk(out_all, I32, (G * stride,), "out order tables")
    _call("sn2_sa_order_group", _ptr(cnt), G, B, M, _ptr(out_all), stride, _stream(), key="sn2_sa_order")


SA_BWD_WS_WORDS = _lib.SN2_SA_BWD_WS_WORDS


def sa_desc(blocks, feat, cf, spos, cpos_aos, nbr, cnt, total, B, Nsrc, M, ext, arg, out, dout=None, dfeat=None,
            with_grads=False, order=None, bwd_ws=None) -> SA:
    """feat: (B*Nsrc, >=cf) row view; spos: (B*Nsrc, >=4) row view holding x,y,z,.
    bwd_ws: (SA_BWD_WS_WORDS) f32, ZERO on entry -- sn2_sa.bwd_ws: a two-block module's backward without `dfeat` then takes
    one message pass for both blocks' weight gradients instead of two."""
    cap = nbr.shape[1]
    cl = blocks[-1].cout
    feat_stride = _chk_rows(feat, F32, B * Nsrc, cf, "feat")
    spos_stride = _chk_rows(spos, F32, B * Nsrc, 4, "spos")
    _chk(cpos_aos, F32, (B * M, 4), "cpos_aos")
    _chk(nbr, I32, (B * M, cap), "nbr")
    _chk(cnt, I32, (B * M,), "cnt")
    _chk(total, I64, (1,), "total")
    _chk(ext, F32, (B * M, cl), "ext")
    _chk(arg, I32, (B * M, cl), "arg")
    _chk(out, F32, (B * M, cl), "out")
    d = SA()
    d.B, d.Nsrc, d.M, d.cap, d.cf, d.nl = B, Nsrc, M, cap, cf, len(blocks)
    d.feat, d.feat_stride, d.spos, d.spos_stride = _ptr(feat), feat_stride, _ptr(spos), spos_stride
    d.cpos, d.nbr, d.cnt, d.total = _ptr(cpos_aos), _ptr(nbr), _ptr(cnt), _ptr(total)
    if order is not None:
        _chk(order, I32, (sa_order_len(B, M),), "order")
    d.order = _ptr(order)
    for i, bb in enumerate(blocks):
        bb.fill(d.blk[i], with_grads)
    d.ext, d.arg, d.out = _ptr(ext), _ptr(arg), _ptr(out)
    if dout is not None:
        _chk(dout, F32, (B * M, cl), "dout")
    if dfeat is not None:
        _chk(dfeat, F32, (B * Nsrc, cf), "dfeat")
    if bwd_ws is not None:
        _chk(bwd_ws, F32, (SA_BWD_WS_WORDS,), "bwd_ws")
    d.dout, d.dfeat, d.bwd_ws = _ptr(dout), _ptr(dfeat), _ptr(bwd_ws)
    return d


def sa_forward(d: SA, training: bool):
    _call("sn2_sa_forward", d, int(training), _stream(), tag=f"cf={d.cf}")


def sa_backward(d: SA):
    _call("sn2_sa_backward", d, _stream(), tag=f"cf={d.cf}")


def interp_ws_words(B: int, R_per_plot: int, S_per_plot: int) -> int:
    """SN2_INTERP_WS_WORDS of include/strata_hip.h."""
    return _host("sn2_interp_ws_words", int(B), int(R_per_plot), int(S_per_plot))


def interp_chunks(R_per_plot: int, S_per_plot: int) -> int:
    """SN2_INTERP_CHUNKS of include/strata_hip.h: slots of the per-plot chunk table of an inverted index."""
    return _host("sn2_interp_chunks", int(R_per_plot), int(S_per_plot))


def fp_src_ws_words(B: int, R_per_plot: int, S_per_plot: int, cout: int) -> int:
    """SN2_FP_SRC_WS_WORDS of include/strata_hip.h: floats of the source-side workspace of a dense-row block (sn2_fp.src_ws)."""
    return _host("sn2_fp_src_ws_words", int(B), int(R_per_plot), int(S_per_plot), int(cout))


def fp_rows_small(R: int) -> bool:
    """sn2_fp_rows_small: a training pass over R rows takes the 64-row matrix-core kernels, the only ones with bfloat16 operands."""
    return bool(_host("sn2_fp_rows_small", int(R)))


def fp_source_side(R: int, cb: int, force: bool = False) -> bool:
    """sn2_fp_source_side: a k-NN block of R rows with cb skip channels takes the source-side form where it is handed a workspace."""
    return bool(_host("sn2_fp_source_side", int(R), int(cb), int(bool(force))))


def interp_index(knn, B: int, R_per_plot: int, S_per_plot: int, out: Optional[torch.Tensor] = None,
                 src_pos: Optional[torch.Tensor] = None, row_perm: Optional[torch.Tensor] = None,
                 row_order: Optional[torch.Tensor] = None, sorted_table=None) -> torch.Tensor:
    """Inverted index of a 3-NN table (source -> list of (target row, normalised weight)): what the backward of the
    interpolation gathers through.  Position-only, so it can be built in the geometry pass.  src_pos (B*S,4): the
    source positions; given, the index also orders every plot's sources along a Morton curve (L2 locality of the
    source-side backward).  row_perm (B*R_per_plot) int32, a permutation of 0..R-1 per plot: the lists name row_perm[row]
    instead of row -- where `fp_desc(..., row_perm=)` keeps the row's d pre-activation (include/strata_hip.h: sn2_fp.row_perm).
    row_order (B*R_per_plot) int32, a permutation of 0..R-1 per plot: the order the rows are walked in (same lists, other order
    inside a list) -- the order the grid search of `three_nn` left (`three_nn_order`) makes the list writes dense;
    sorted_table = (idx_sorted, w_sorted): the table's rows in that order, read instead of a gather (sn2_interp_index_ordered)."""
    if row_order is not None or sorted_table is not None:
        n = interp_ws_words(B, R_per_plot, S_per_plot)
        if out is None:
            out = torch.empty(n, dtype=F32, device=knn[0].device)
        interp_index_group(knn, 1, B, R_per_plot, S_per_plot, out, n, src_pos=src_pos, row_perm=row_perm, row_order=row_order,
                           sorted_table=sorted_table)
        return out
    if src_pos is not None:
        _chk(src_pos, F32, (B * S_per_plot, 4), "src_pos")
    if row_perm is not None:
        _chk(row_perm, I32, (B * R_per_plot,), "row_perm")
    R = B * R_per_plot
    _chk(knn[0], I32, (R, 3), "knn_idx")
    _chk(knn[1], F32, (R, 3), "knn_w")
    n = interp_ws_words(B, R_per_plot, S_per_plot)
    if out is None:
        out = torch.empty(n, dtype=F32, device=knn[0].device)
    else:
        _chk(out, F32, (n,), "out index")
    _call("sn2_interp_index_perm", _ptr(knn[0]), _ptr(knn[1]), _ptr(src_pos), _ptr(row_perm), B, R_per_plot, S_per_plot, _ptr(out),
          _stream(), key="sn2_interp_index")
    return out


def interp_index_group(knn, G: int, B: int, R_per_plot: int, S_per_plot: int, out_all: torch.Tensor, stride: int,
                       src_pos: Optional[torch.Tensor] = None, row_perm: Optional[torch.Tensor] = None,
                       row_order: Optional[torch.Tensor] = None, sorted_table=None):
    """include/strata_hip.h: sn2_interp_index_group -- the inverted indices of G consecutive batches of B plots in ONE set of four
    launches; knn / src_pos / row_perm: the group's arrays; batch h's index = out_all[h * stride : h * stride + interp_ws_words(...)].
    row_order / sorted_table (the group's arrays, as `interp_index`): sn2_interp_index_ordered."""
    R = G * B * R_per_plot
    _chk(knn[0], I32, (R, 3), "knn_idx")
    _chk(knn[1], F32, (R, 3), "knn_w")
    if src_pos is not None:
        _chk(src_pos, F32, (G * B * S_per_plot, 4), "src_pos")
    if row_perm is not None:
        _chk(row_perm, I32, (R,), "row_perm")
    if G == 1:
        stride = interp_ws_words(B, R_per_plot, S_per_plot)          # (one batch: no stride)
    elif stride % 4 or stride < interp_ws_words(B, R_per_plot, S_per_plot):
        raise ValueError("interp_index_group: stride must be a multiple of 4 words and hold one index")
    _chk(out_all, F32, (G * stride,), "out indices")
    if row_order is not None or sorted_table is not None:
        if row_order is None:
            raise ValueError("interp_index_group: sorted_table needs its row_order")
        _chk(row_order, I32, (R,), "row_order")
        si, sw = sorted_table if sorted_table is not None else (None, None)
        if si is not None:
            _chk(si, I32, (R, 3), "idx_sorted")
            _chk(sw, F32, (R, 3), "w_sorted")
        _call("sn2_interp_index_ordered", _ptr(knn[0]), _ptr(knn[1]), _ptr(src_pos), _ptr(row_perm), _ptr(row_order), _ptr(si), _ptr(sw),
              G, B, R_per_plot, S_per_plot, _ptr(out_all), stride, _stream(), key="sn2_interp_index")
        return
    _call("sn2_interp_index_group", _ptr(knn[0]), _ptr(knn[1]), _ptr(src_pos), _ptr(row_perm), G, B, R_per_plot, S_per_plot, _ptr(out_all),
          stride, _stream(), key="sn2_interp_index")


SOURCE_SIDE = True     # False: never hand out src_ws, i.e. every row rebuilds its interpolated input (tests compare both)


def fp_desc(block: BlockBuffers, B, R_per_plot, S_per_plot, ca, cb, src, h, src_affine=None, knn=None, skip=None,
            dy=None, dsrc=None, dskip=None, du_scratch=None, with_grads=False, interp_index=None,
            bn_sums_done=None, row_perm=None, force_src_ws=False, gather=True) -> FP:
    """src: (B*S_per_plot, >=ca) rows when knn is given, else (B*R_per_plot, >=ca); skip: (B*R_per_plot, >=cb) row view.
    h of dtype bfloat16 (then dy and du_scratch too): the per-point layer stores its three activation buffers in bfloat16
    (include/strata_hip.h: sn2_fp.act_bf16; BASELINE config 5) -- only the source-side form (`fp_source_side`) has those
    kernels."""
    R = B * R_per_plot
    hs = (block.cout + 3) // 4 * 4
    AT = BF16 if (h is not None and h.dtype == BF16) else F32         # the storage type of h / dy / du_scratch
    n_src_rows = R if knn is None else B * S_per_plot
    src_stride = _chk_rows(src, F32, n_src_rows, ca, "src")
    if src.shape[1] < (ca + 3) // 4 * 4 and src_stride < (ca + 3) // 4 * 4:
        raise ValueError("fp: src rows must be padded to a multiple of 4 floats")
    if h is not None or not force_src_ws:
        _chk(h, AT, (R, hs), "h")
    d = FP()
    d.B, d.R_per_plot, d.S_per_plot, d.ca, d.cb = B, R_per_plot, S_per_plot, ca, cb
    d.src, d.src_stride = _ptr(src), src_stride
    if src_affine is not None:
        _chk(src_affine[0], F32, (ca,), "src_a")
        _chk(src_affine[1], F32, (ca,), "src_c")
        d.src_a, d.src_c = _ptr(src_affine[0]), _ptr(src_affine[1])
    else:
        d.src_a = d.src_c = None
    if knn is not None:
        _chk(knn[0], I32, (R, 3), "knn_idx")
        _chk(knn[1], F32, (R, 3), "knn_w")
        d.knn_idx, d.knn_w = _ptr(knn[0]), _ptr(knn[1])
    else:
        d.knn_idx = d.knn_w = None
    if cb > 0:
        d.skip_stride = _chk_rows(skip, F32, R, cb, "skip", align=4 if cb % 4 == 0 else 1)
        d.skip = _ptr(skip)
    else:
        d.skip, d.skip_stride = None, 0
    block.fill(d.blk, with_grads)
    if not fp_rows_small(R):
        # bfloat16 operands exist on the matrix-core kernels of the layers over centroids only;
        # a block with more rows (FP2 at the reference's default ratio1 = 0.5: 262 144 rows) runs its fp32 row kernels
        d.blk.mma_bf16 = 0
    d.h, d.h_stride = _ptr(h), hs
    if dy is not None:
        _chk(dy, AT, (R, hs), "dy")
    d.dsrc_stride = d.dskip_stride = 0
    if dsrc is not None:
        d.dsrc_stride = _chk_rows(dsrc, F32, n_src_rows, ca, "dsrc", align=1)
    if dskip is not None:
        d.dskip_stride = _chk_rows(dskip, F32, R, cb, "dskip", align=1)
    d.scatter_ws, d.scatter_ready = None, 0
    if bn_sums_done is not None:
        _chk(bn_sums_done, I32, (1,), "bn_sums_done")
    d.bn_sums_done = _ptr(bn_sums_done)
    # source-side workspace of the per-point layer (include/strata_hip.h: src_ws); scratch, so one per descriptor
    d._src_ws = None
    if SOURCE_SIDE and knn is not None and fp_source_side(R, cb, force_src_ws):
        d._src_ws = torch.empty(fp_src_ws_words(B, R_per_plot, S_per_plot, block.cout), dtype=F32, device=src.device)
    d.src_ws = _ptr(d._src_ws)
    d.row_perm = None
    if row_perm is not None and d._src_ws is not None and du_scratch is not None:
        # the backward pass keeps its d pre-activation rows in this order; the interp_index handed in must have been built
        # with the same permutation
        _chk(row_perm, I32, (R,), "row_perm")
        d.row_perm = _ptr(row_perm)
    d.act_bf16 = int(AT == BF16)
    if d.act_bf16 and d._src_ws is None:
        raise ValueError("fp: bfloat16 activation rows need the source-side form (hip_ops.fp_source_side)")
    if du_scratch is not None:
        _chk(du_scratch, AT, (R, max(ca, hs)), "du_scratch")
        if knn is not None and dsrc is not None:
            # inverted index of the 3-NN table: prebuilt by interp_index (geometry pass) or built by the backward call
            words = interp_ws_words(B, R_per_plot, S_per_plot)
            if interp_index is not None:
                _chk(interp_index, F32, (words,), "interp_index")
                d._scatter_ws, d.scatter_ready = interp_index, 1
            else:
                d._scatter_ws = torch.empty(words, dtype=F32, device=src.device)
            d.scatter_ws = _ptr(d._scatter_ws)
            if not gather:
                d.scatter_ready = -1          # the per-row input gradients stay in du_scratch: the caller transposes (global_pool_backward)
    d.dy, d.dsrc, d.dskip, d.du_scratch = _ptr(dy), _ptr(dsrc), _ptr(dskip), _ptr(du_scratch)
    return d


def fp_bn_sums(d: FP, gamma, beta, mean, invstd, dgamma, dbeta, ok):
    """After fp_backward(d): dgamma/dbeta (ACCUMULATED, complete) of the BatchNorm whose output block d interpolates, from d's
    own weight and bias gradients -- or, where a |gamma| is too small for that, summed over the rows by the same kernel
    (include/strata_hip.h: sn2_fp_bn_sums).  mean, invstd: the BatchNorm's saved batch statistics."""
    for t, n in ((gamma, "gamma"), (beta, "beta"), (mean, "mean"), (invstd, "invstd"), (dgamma, "dgamma"), (dbeta, "dbeta")):
        _chk(t, F32, (d.ca,), n)
    _chk(ok, I32, (1,), "ok")
    _call("sn2_fp_bn_sums", d, _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(invstd), _ptr(dgamma), _ptr(dbeta), _ptr(ok), _stream())


def fp_forward(d: FP, training: bool):
    _call("sn2_fp_forward", d, int(training), _stream(), tag=f"{d.ca}+{d.cb}->{d.blk.cout}")


def fp_backward(d: FP):
    _call("sn2_fp_backward", d, _stream(), tag=f"{d.ca}+{d.cb}->{d.blk.cout}")


FP_FORM_SPLIT, FP_FORM_SOURCE_SIDE, FP_FORM_DENSE = _lib.SN2_FP_FORM_SPLIT, _lib.SN2_FP_FORM_SOURCE_SIDE, _lib.SN2_FP_FORM_DENSE


def fp_form(d: FP, fp_pass: int) -> int:
    """sn2_fp_form: the kernel form (FP_FORM_*) that fp_forward(d, training = fp_pass) takes for fp_pass 0 / 1 / 2 and
    fp_backward(d) for fp_pass 3, or the negative code the call would return.  Host arithmetic: nothing is launched."""
    return _lib.load().sn2_fp_form(d, int(fp_pass))


def plot_max_forward(h, a, c, B, R_per_plot, C):
    hs = (C + 3) // 4 * 4
    _chk(h, F32, (B * R_per_plot, hs), "h")
    _chk(a, F32, (C,), "a")
    _chk(c, F32, (C,), "c")
    out = torch.empty(B, C, dtype=F32, device=h.device)
    arg = torch.empty(B, C, dtype=I32, device=h.device)
    _call("sn2_plot_max_forward", _ptr(h), _ptr(a), _ptr(c), B, R_per_plot, C, _ptr(out), _ptr(arg), _stream())
    return out, arg


GL_MAX_PLOTS = _lib.SN2_GLOBAL_MAX_PLOTS        # sn2_global_level_forward's and _backward's limit
_GLOBAL_WS = {}          # device index -> workspace of callers that name no owner
_GLOBAL_WS_ALL = []      # weak references to every live workspace (global_level_gave_up looks at all of them)


class _GlobalWs(list):
    """[exchange granules (int64), control words (int32), give-ups already reported, the backward's granules, its control words]"""
    __slots__ = ("__weakref__",)


def global_level_ws(dev, B: int = GL_MAX_PLOTS, owner=None):
    """The exchange areas and control words of `global_level_forward` (ws[0], ws[1]) and `global_level_backward` (ws[3], ws[4]:
    its own), zero-filled once, then the library's.
    owner: the object whose training forwards use it (a PointNet2): the workspace lives on it, so two models that train on two
    streams of one process never share an exchange area; without an owner there is one per device.  Launches that share a
    workspace must be on one stream at a time.  Allocated ONCE at the largest size the kernels take (GL_MAX_PLOTS plots: 229 KB
    for the forward's granules, 57 KB for the backward's, 8 + 64 control words) and
    never again: hipGraphs captured earlier hold its raw address and its launch epoch (round 4 reallocated it when a later call
    had more plots, under the feet of the graphs captured before)."""
    dev = torch.device(dev)
    if B > GL_MAX_PLOTS:
        raise ValueError(f"global_level_forward takes at most {GL_MAX_PLOTS} plots")
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    store = _GLOBAL_WS if owner is None else owner.__dict__.setdefault("_gl_ws", {})
    ws = store.get(key)
    if ws is None:
        if torch.cuda.is_current_stream_capturing():
            # zero fills captured into a graph would run at every replay and reset the launch epoch under the other graphs
            raise StrataHipError("global_level_forward: its exchange area must exist before a stream capture starts -- run one "
                                 "eager training forward first (TrainPipeline.capture does) or call hip_ops.global_level_ws(dev, owner=model)")
        ws = _GlobalWs([torch.zeros(_host("sn2_global_xchg_words", GL_MAX_PLOTS), dtype=I64, device=dev),
                        torch.zeros(_lib.SN2_GLOBAL_CTL_WORDS, dtype=I32, device=dev), 0,
                        torch.zeros(_lib.SN2_GLOBAL_BWD_XCHG_WORDS, dtype=I64, device=dev),
                        torch.zeros(_lib.SN2_GLOBAL_BWD_CTL_WORDS, dtype=I32, device=dev)])
        store[key] = ws
        import weakref
        _GLOBAL_WS_ALL[:] = [r for r in _GLOBAL_WS_ALL if r() is not None]
        _GLOBAL_WS_ALL.append(weakref.ref(ws))
    return ws


def global_level_forward_fused(B: int, *blocks) -> bool:
    """Does a training forward of the global level take `global_level_forward`?  (sn2_global_level_forward_route, the rule of
    sn2_net_forward: at most GL_MAX_PLOTS plots and fp32 operands in `blocks`; the caller ANDs in its own setting.)"""
    return bool(_host("sn2_global_level_forward_route", int(B), int(any(b.mma_bf16 for b in blocks))))


def global_level_forward(d_sa3: FP, d_fp3: FP, x3: torch.Tensor, arg3: torch.Tensor, owner=None):
    """SA3 -> BatchNorm -> plot max -> FP3 -> BatchNorm in one launch (training mode; include/strata_hip.h).  d_fp3 must have
    been built with src = x3.  owner: see `global_level_ws`."""
    B = d_sa3.B
    _chk(x3, F32, (B, 64), "x3")
    _chk(arg3, I32, (B, 64), "arg3")
    ws = global_level_ws(x3.device, B, owner=owner)
    _call("sn2_global_level_forward", d_sa3, d_fp3, _ptr(x3), _ptr(arg3), _ptr(ws[0]), _ptr(ws[1]), _stream())


GL_BWD_MAX_ROWS = _lib.SN2_GLOBAL_BWD_MAX_ROWS


def global_level_backward_fused(B: int, M2: int, frozen: bool, *blocks) -> bool:
    """Does the backward of the global level take `global_level_backward`?  (sn2_global_level_backward_route, the rule of
    sn2_net_backward: at most GL_MAX_PLOTS plots, batch statistics, fp32 operands, and at most GL_BWD_MAX_ROWS rows per plot --
    the one-block-per-group instance of the kernel, the one measured against the four launches; the entry point itself takes
    more rows.)"""
    return bool(_host("sn2_global_level_backward_route", int(B), int(M2), int(bool(frozen)), int(any(b.mma_bf16 for b in blocks))))


def global_level_backward(d_sa3: FP, d_fp3: FP, arg3: torch.Tensor, owner=None):
    """FP3's BatchNorm sums, FP3 backward, the pool's backward, SA3's BatchNorm sums and SA3 backward in one launch (include/
    strata_hip.h).  d_fp3: dy, dsrc = d x3, dskip = d x2; d_sa3: dsrc = the same d x2; both with_grads.  owner: see
    `global_level_ws`."""
    B = d_sa3.B
    _chk(arg3, I32, (B, 64), "arg3")
    ws = global_level_ws(arg3.device, B, owner=owner)
    _call("sn2_global_level_backward", d_sa3, d_fp3, _ptr(arg3), _ptr(ws[3]), _ptr(ws[4]), _stream())


def global_level_gave_up(dev, warn: bool = True) -> int:
    """Exchange waits of `global_level_forward` and `global_level_backward` that gave up on this device since the process
    started (a workgroup of a launch was not resident within the spin limit: another stream or process held the CUs), over
    every live workspace.  Each such launch was REPAIRED inside itself by the workgroup that left it last (the forward
    recomputes the level, the backward finishes the plots whose workgroups had committed nothing: include/strata_hip.h),
    so the results are unaffected; a count that grew since the last call is reported once as a StrataHipWarning (the passes took
    longer; `PointNet2.fuse_global_level = False` runs the level as separate launches).  Reads device words: call it where the
    host synchronises anyway (TrainPipeline.drain, after a test)."""
    dev = torch.device(dev)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    total = 0
    for r in list(_GLOBAL_WS_ALL):
        ws = r()
        if ws is None or ws[1].device.index != key:
            continue
        n = int(ws[1][1].item()) + int(ws[4][1].item())
        total += n
        if n > ws[2]:
            seen, ws[2] = ws[2], n
            if warn:
                import warnings
                warnings.warn(f"global_level_forward / backward: {n - seen} exchange wait(s) gave up on {dev}; those launches were finished "
                              "by their last workgroup alone (results unaffected, the passes took longer); set "
                              "PointNet2.fuse_global_level = False where other kernels or processes share the device",
                              StrataHipWarning, stacklevel=2)
    return total


def plot_max_backward(dout, arg, B, R_per_plot, C, dy):
    hs = (C + 3) // 4 * 4
    _chk(dout, F32, (B, C), "dout")
    _chk(arg, I32, (B, C), "arg")
    _chk(dy, F32, (B * R_per_plot, hs), "dy")
    _call("sn2_plot_max_backward", _ptr(dout), _ptr(arg), B, R_per_plot, C, _ptr(dy), _stream())


def global_pool_backward(du, arg, h, mean, invstd, B, R_per_plot, dx, dy, dgamma, dbeta):
    """include/strata_hip.h: sn2_global_pool_backward -- the backward of the pool between FP3 and SA3 in one launch."""
    _chk(du, F32, (B * R_per_plot, 64), "du")
    _chk(arg, I32, (B, 64), "arg")
    _chk(h, F32, (B * R_per_plot, 64), "h")
    for t, n in ((mean, "mean"), (invstd, "invstd"), (dgamma, "dgamma"), (dbeta, "dbeta")):
        _chk(t, F32, (64,), n)
    _chk(dx, F32, (B, 64), "dx")
    _chk(dy, F32, (B * R_per_plot, 64), "dy")
    _call("sn2_global_pool_backward", _ptr(du), 64, _ptr(arg), _ptr(h), _ptr(mean), _ptr(invstd), B, R_per_plot, 64, _ptr(dx), _ptr(dy),
          _ptr(dgamma), _ptr(dbeta), _stream())


def dropout_mask_words(keep: torch.Tensor) -> torch.Tensor:
    """keep (R,16) bool / 0-1 values (True = the hidden channel survives F.dropout) -> (R) int32 words, bit j = channel j."""
    if keep.dim() != 2 or keep.shape[1] != 16:
        raise ValueError("dropout mask must be (rows, 16)")
    pow2 = (2 ** torch.arange(16, device=keep.device, dtype=torch.int32))
    return ((keep != 0).to(torch.int32) * pow2).sum(1, dtype=torch.int32).contiguous()


def head_loss_route(B: int, N: int, diam_pix: int) -> bool:
    """include/strata_hip.h: sn2_head_loss_route -- the head backward takes a loss-gradient descriptor at these sizes."""
    return bool(_host("sn2_head_loss_route", int(B), int(N), int(diam_pix)))


def loss_grad_desc(pred, gt, proba, pdf, grad_total, arg, nocc, pix, B: int, N: int, diam_pix: int, m: float, e: float) -> LossGrad:
    """include/strata_hip.h: sn2_loss_grad -- what `projected_loss_backward` takes, for `head_desc(loss=)` / the executor's
    backward: the head backward computes d loss / d coverages and d loss / d proba itself.  pdf may be None when m == 0.  The
    descriptor keeps its tensors alive (`.tensors`)."""
    R, D = B * N, int(diam_pix)
    _chk(pred, F32, (B, 4), "pred")
    _chk(gt, F64, (B, 4), "gt")
    _chk(proba, F32, (R, 4), "proba")
    if pdf is not None:
        _chk(pdf, F64, (R, 3), "pdf")
    _chk(grad_total, F64, None, "grad_total")
    _chk(arg, I32, (B * D * D * 3,), "arg")
    _chk(nocc, I32, (B,), "nocc")
    _chk(pix, I32, (R,), "pix")
    if grad_total.numel() != 1:
        raise ValueError("loss_grad_desc: grad_total is ONE fp64 scalar on the device")
    g = LossGrad()
    g.pred, g.gt, g.proba, g.pdf, g.grad_total = _ptr(pred), _ptr(gt), _ptr(proba), _ptr(pdf), _ptr(grad_total)
    g.arg, g.nocc, g.pix = _ptr(arg), _ptr(nocc), _ptr(pix)
    g.B, g.N, g.D, g.m, g.e = int(B), int(N), D, float(m), float(e)
    g.tensors = (pred, gt, proba, pdf, grad_total, arg, nocc, pix)
    return g


def head_desc(f, fa, fc, lin1, lin2, coverages=None, proba=None, dcov=None, dproba=None, dy=None, grads=None,
              grad_images=(1, 0), drop_mask=None, drop_p: float = 0.0, rows: Optional[int] = None, loss: Optional[LossGrad] = None) -> Head:
    """f (R,36): the rows the head reads -- or None with `rows` = R for `fp_head_eval`, whose rows never reach memory.
    loss (`loss_grad_desc`, where `head_loss_route` says yes): `head_backward` computes the incoming gradients itself; dcov and
    dproba must then be None."""
    if f is None:
        if rows is None or coverages is None:
            raise ValueError("head_desc: without f the row count and the outputs must be given")
        R, AT = int(rows), F32
    else:
        R = f.shape[0]
        AT = BF16 if f.dtype == BF16 else F32         # bfloat16 rows of f (and dy): sn2_head.act_bf16
        _chk(f, AT, (R, 36), "f")
    _chk(fa, F32, (34,), "fa")
    _chk(fc, F32, (34,), "fc")
    _chk(lin1.weight, F32, (16, 34), "lin1.weight")
    _chk(lin1.bias, F32, (16,), "lin1.bias")
    _chk(lin2.weight, F32, (5, 16), "lin2.weight")
    _chk(lin2.bias, F32, (5,), "lin2.bias")
    d = Head()
    d.R, d.cin, d.f_stride = R, 34, 36
    d.f, d.fa, d.fc = _ptr(f), _ptr(fa), _ptr(fc)
    d.W1, d.b1, d.W2, d.b2 = _ptr(lin1.weight), _ptr(lin1.bias), _ptr(lin2.weight), _ptr(lin2.bias)
    for t, n in ((coverages, "coverages"), (proba, "proba"), (dcov, "dcoverages"), (dproba, "dproba")):
        if t is not None:
            _chk(t, F32, (R, 4), n)
    d.coverages, d.proba, d.dcoverages, d.dproba = _ptr(coverages), _ptr(proba), _ptr(dcov), _ptr(dproba)
    if dy is not None:
        _chk(dy, AT, (R, 36), "dy")
    d.dy = _ptr(dy)
    d.act_bf16 = int(AT == BF16)
    if grads is not None:
        for t, ref in zip(grads, (lin1.weight, lin1.bias, lin2.weight, lin2.bias)):
            _chk(t, F32, ref.shape, "head grad view")
        d.dW1, d.db1, d.dW2, d.db2 = (_ptr(t) for t in grads)
        d.grad_replicas, d.grad_replica_stride = grad_images
    else:
        d.dW1 = d.db1 = d.dW2 = d.db2 = None
        d.grad_replicas, d.grad_replica_stride = 1, 0
    if drop_mask is not None:
        _chk(drop_mask, I32, (R,), "drop_mask")
        d.drop_mask, d.drop_scale = _ptr(drop_mask), (1.0 / (1.0 - drop_p) if drop_p < 1.0 else 0.0)
    else:
        d.drop_mask, d.drop_scale = None, 1.0
    if loss is not None:
        if dcov is not None or dproba is not None:
            raise ValueError("head_desc: a loss-gradient descriptor takes the place of dcov and dproba")
        d.loss = ctypes.pointer(loss)
        d._loss = loss                          # (the pointer does not keep the descriptor, nor that its tensors, alive)
    return d


GRAD_IMAGES = _lib.SN2_NET_GRAD_IMAGES       # images of the flat parameter gradient the backward kernels spread their atomics over


def flat_layout(params):
    """Offsets of the parameters inside the flat parameter / gradient vectors (back to back, in model.parameters() order)
    and the vectors' length."""
    offs, o = [], 0
    for p in params:
        offs.append(o)
        o += p.numel()
    return offs, o


def grad_images_alloc(n_flat: int, device, extra_words: int = 0):
    """One zero-filled arena: GRAD_IMAGES images of the flat gradient (image stride = n_flat rounded up to 64 floats)
    followed by `extra_words` floats.  Returns (arena, image 0 view (n_flat), (replicas, stride), extra view)."""
    stride = (n_flat + 63) // 64 * 64
    arena = torch.zeros(GRAD_IMAGES * stride + extra_words, dtype=F32, device=device)
    return arena, arena[:n_flat], (GRAD_IMAGES, stride), arena[GRAD_IMAGES * stride:]


def grad_reduce(arena, n_flat: int, images):
    """include/strata_hip.h: sn2_grad_reduce -- fold the images into image 0 (arena[:n_flat])."""
    replicas, stride = images
    _chk(arena, F32, None, "arena")
    if arena.numel() < replicas * stride:
        raise ValueError("grad_reduce: arena smaller than its images")
    _call("sn2_grad_reduce", _ptr(arena), n_flat, replicas, stride, _stream())


def fp_head_eval(d: FP, hd: Head):
    """include/strata_hip.h: sn2_fp_head_eval -- EVAL: the per-point layer and the head in one pass, no (B*N,36) buffer between."""
    _call("sn2_fp_head_eval", d, hd, _stream())


def head_forward(d: Head):
    _call("sn2_head_forward", d, _stream())


def head_backward(d: Head):
    _call("sn2_head_backward", d, _stream())


def head_bn_sums(d: Head, gamma, beta, mean, invstd, dgamma, dbeta, ok):
    """After head_backward: dgamma/dbeta (ACCUMULATED, complete) of the BatchNorm feeding lin1, from lin1's gradients (or by
    the kernel's own pass over the rows where a |gamma| is too small)."""
    for t, n in ((gamma, "gamma"), (beta, "beta"), (mean, "mean"), (invstd, "invstd"), (dgamma, "dgamma"), (dbeta, "dbeta")):
        _chk(t, F32, (d.cin,), n)
    _chk(ok, I32, (1,), "ok")
    _call("sn2_head_bn_sums", d, _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(invstd), _ptr(dgamma), _ptr(dbeta), _ptr(ok), _stream())


# ---------------------------------------------------------------------------------------------- projections
def _xy_rows(clouds_dev: torch.Tensor):
    """clouds (B,C>=2,N) on device -> (pointer tensor, plot stride in floats)."""
    B, C, N = clouds_dev.shape
    _chk(clouds_dev, F32, (B, C, N), "clouds")
    if C < 2:
        raise ValueError("clouds needs at least the x and y rows")
    return clouds_dev, C * N


def plot_project_forward(pred_pointwise: torch.Tensor, clouds_dev: torch.Tensor, diam_pix: int):
    B, C, N = clouds_dev.shape
    _chk(pred_pointwise, F32, (B * N, 4), "pred_pointwise")
    t, stride = _xy_rows(clouds_dev)
    dev = pred_pointwise.device
    D = int(diam_pix)
    keys = torch.empty(B * D * D * 3, dtype=I64, device=dev)
    pix = torch.empty(B * N, dtype=I32, device=dev)
    arg = torch.empty(B * D * D * 3, dtype=I32, device=dev)
    nocc = torch.empty(B, dtype=I32, device=dev)
    pred = torch.empty(B, 4, dtype=F32, device=dev)
    _call("sn2_plot_project_forward", _ptr(pred_pointwise), _ptr(t), stride, B, N, D, _ptr(keys), _ptr(pix),
                                               _ptr(arg), _ptr(nocc), _ptr(pred), _stream())
    return pred, pix, arg, nocc


def p2_key_parts(N: int) -> int:
    """SN2_P2_KEY_PARTS of include/strata_hip.h."""
    return _host("sn2_p2_key_parts", int(N))


def plot_pixels(clouds_dev: torch.Tensor, diam_pix: int, out=None):
    """clouds (B,C,N) on the device -> (mm (B,4) bounding boxes, pix (B*N) int32): the pixel ids of
    `project_to_plotwise_coverages` (project_to_2d.py:16-22), computed from the positions alone -- what a pipelined loop runs
    ahead of the feature pass (include/strata_hip.h: sn2_plot_pixels).  out = (mm, pix): caller-owned buffers."""
    B, C, N = clouds_dev.shape
    t, stride = _xy_rows(clouds_dev)
    if out is None:
        mm = torch.empty(B, 4, dtype=F32, device=clouds_dev.device)
        pix = torch.empty(B * N, dtype=I32, device=clouds_dev.device)
    else:
        mm, pix = out
        _chk(mm, F32, (B, 4), "out mm")
        _chk(pix, I32, (B * N,), "out pix")
    _call("sn2_plot_pixels", _ptr(t), stride, B, N, int(diam_pix), _ptr(mm), _ptr(pix), _stream())
    return mm, pix


def plot_project_forward_pix(pred_pointwise: torch.Tensor, pix: torch.Tensor, B: int, N: int, diam_pix: int):
    """`plot_project_forward` from pixel ids that `plot_pixels` computed ahead of time: two launches, no key table to clear."""
    _chk(pred_pointwise, F32, (B * N, 4), "pred_pointwise")
    _chk(pix, I32, (B * N,), "pix")
    dev = pred_pointwise.device
    D = int(diam_pix)
    keys = torch.empty(p2_key_parts(N) * B * D * D * 3, dtype=I64, device=dev)
    arg = torch.empty(B * D * D * 3, dtype=I32, device=dev)
    nocc = torch.empty(B, dtype=I32, device=dev)
    pred = torch.empty(B, 4, dtype=F32, device=dev)
    _call("sn2_plot_project_forward_pix", _ptr(pred_pointwise), _ptr(pix), B, N, D, _ptr(keys), _ptr(arg), _ptr(nocc), _ptr(pred),
          _stream(), key="sn2_plot_project_forward")
    return pred, pix, arg, nocc


def plot_project_backward(dpred, arg, nocc, pix, B, N, diam_pix):
    D = int(diam_pix)
    _chk(dpred, F32, (B, 4), "dpred")
    _chk(arg, I32, (B * D * D * 3,), "arg")
    _chk(nocc, I32, (B,), "nocc")
    _chk(pix, I32, (B * N,), "pix")
    dpw = torch.empty(B * N, 4, dtype=F32, device=dpred.device)
    _call("sn2_plot_project_backward", _ptr(dpred), _ptr(arg), _ptr(nocc), _ptr(pix), B, N, D, _ptr(dpw), _stream())
    return dpw


def raster_project(coverages: torch.Tensor, clouds_dev: torch.Tensor, diam_pix: int, diam_meters: int):
    """coverages (B*N,4), clouds (B,C,N) -> rasters (B,3,D,D) fp32 with NaN, pix (B*N) int32."""
    B, C, N = clouds_dev.shape
    _chk(coverages, F32, (B * N, 4), "coverages")
    t, stride = _xy_rows(clouds_dev)
    dev = coverages.device
    D = int(diam_pix)
    keys = torch.empty(B * D * D * 3, dtype=I64, device=dev)
    pix = torch.empty(B * N, dtype=I32, device=dev)
    rasters = torch.empty(B, 3, D, D, dtype=F32, device=dev)
    _call("sn2_raster_project", _ptr(coverages), _ptr(t), stride, B, N, D, int(diam_meters), _ptr(keys),
                                         _ptr(pix), _ptr(rasters), _stream())
    return rasters, pix


def mosaic_merge(rasters, weights, offsets, mean, wsum, window=None):
    """Fold plots 0..B-1 (in order) into the running mosaic (mean, wsum) (3,H,W), NaN = no data."""
    B, _, D, _ = rasters.shape
    _, H, W = mean.shape
    _chk(rasters, F32, (B, 3, D, D), "rasters")
    _chk(weights, F32, (D, D), "weights")
    _chk(offsets, I32, (B, 2), "offsets")
    _chk(mean, F32, (3, H, W), "mean")
    _chk(wsum, F32, (3, H, W), "wsum")
    y0, x0, wh, ww = (0, 0, H, W) if window is None else [int(v) for v in window]
    _call("sn2_mosaic_merge", _ptr(rasters), _ptr(weights), _ptr(offsets), B, D, H, W, _ptr(mean), _ptr(wsum),
          y0, x0, wh, ww, _stream())


def mosaic_finalize(mean: torch.Tensor, wsum: torch.Tensor, thr: Optional[torch.Tensor] = None):
    """mean (3,H,W), wsum (H,W) -> out (5,H,W) = [Vb, Vm_soft, Vh, Vm_hard, weights], thr (2,) = threshold, its index (written
    into `thr` when one is given)."""
    _, H, W = mean.shape
    _chk(mean, F32, (3, H, W), "mean")
    _chk(wsum, F32, (H, W), "wsum")
    dev = mean.device
    hist = torch.empty(_lib.SN2_MOSAIC_HIST_WORDS, dtype=I32, device=dev)
    acc = torch.empty(1, dtype=F64, device=dev)
    thr = torch.empty(2, dtype=F32, device=dev) if thr is None else _chk(thr, F32, (2,), "thr")
    out = torch.empty(5, H, W, dtype=F32, device=dev)
    _call("sn2_mosaic_finalize", _ptr(mean), _ptr(wsum), H, W, _ptr(hist), _ptr(acc), _ptr(thr), _ptr(out), _stream())
    return out, thr


MOSAIC_CROP_MAX_BANDS, MOSAIC_CROP_MAX_EDGES = _lib.SN2_MOSAIC_CROP_MAX_BANDS, _lib.SN2_MOSAIC_CROP_MAX_EDGES


def mosaic_crop_ws_words(C: int, H: int, W: int) -> int:
    """SN2_MOSAIC_CROP_WS_WORDS of include/strata_hip.h (32-bit words)."""
    return _host("sn2_mosaic_crop_ws_words", int(C), int(H), int(W))


def mosaic_crop_stats(bands: torch.Tensor, x_min: float, y_max: float, pix: float, edges=None, out=None):
    """include/strata_hip.h: sn2_mosaic_crop_stats.  bands (C,H,W) fp32 on the device, CHANGED IN PLACE: every pixel whose centre
    (x_min + pix (c + 0.5), y_max - pix (r + 0.5)) is not inside the polygon of `edges` ((E,4) fp64 = ax, ay, bx, by: numpy or a
    device tensor, `parcel.polygon_edges`) becomes NaN in every band -> (mean (C) fp64, count (C) int64) on the device: the
    band-wise mean and number of the pixels that are not NaN after the crop.  edges=None: no crop, `bands` is not written, the
    statistics alone.  out: a (mean, count) pair of device tensors to write into.  Two launches on the current stream and no
    read-back; the same input gives the same bytes.  The limits (C <= MOSAIC_CROP_MAX_BANDS, H W < 2^31, 3 <= E <=
    MOSAIC_CROP_MAX_EDGES, pix > 0, finite geometry) are the library's: SN2_EINVAL / SN2_ELIMIT."""
    _chk(bands, F32, None, "bands")
    if bands.dim() != 3:
        raise ValueError(f"bands: expected (C,H,W), got {tuple(bands.shape)}")
    C, H, W = bands.shape
    dev = bands.device
    E = 0
    if edges is not None:
        if not isinstance(edges, torch.Tensor):
            edges = torch.from_numpy(np.ascontiguousarray(np.asarray(edges, dtype=np.float64).reshape(-1, 4)))
        edges = edges.to(dev)
        E = edges.shape[0]
        _chk(edges, F64, (E, 4), "edges")
        if E == 0:
            raise ValueError("edges: no edge (edges=None asks for the statistics alone)")
    ws = torch.empty(max(mosaic_crop_ws_words(C, H, W), 2) // 2, dtype=F64, device=dev)
    if out is None:
        mean, count = torch.empty(C, dtype=F64, device=dev), torch.empty(C, dtype=I64, device=dev)
    else:
        mean, count = _chk(out[0], F64, (C,), "out[0]"), _chk(out[1], I64, (C,), "out[1]")
    _call("sn2_mosaic_crop_stats", _ptr(bands), C, H, W, float(x_min), float(y_max), float(pix), _ptr(edges) if E else None, E,
          _ptr(ws), _ptr(mean), _ptr(count), _stream())
    return mean, count


# ---- the mosaic atlas (include/strata_hip.h, "Mosaic atlas"; csrc/atlas.hip): the canvases of K parcels in one arena ----------
def atlas_canvas_table(H, W, x_min=None, y_max=None) -> np.ndarray:
    """sn2_atlas_canvas_table: the (K+1, SN2_ATLAS_CANVAS_COLS) int64 canvas table of K canvases of H[k] x W[k] pixels with the
    geotransforms (x_min[k], y_max[k]) (None: zeros).  Host arithmetic, no device.  SN2_EINVAL / SN2_ELIMIT raise."""
    H = np.ascontiguousarray(np.asarray(H, dtype=np.int64).reshape(-1))
    W = np.ascontiguousarray(np.asarray(W, dtype=np.int64).reshape(-1))
    K = len(H)
    if len(W) != K or (x_min is None) != (y_max is None):
        raise ValueError("atlas_canvas_table: H, W (and x_min, y_max) need one entry per canvas")
    if K and (np.abs(H).max() >= 2 ** 31 or np.abs(W).max() >= 2 ** 31):
        raise ValueError("atlas_canvas_table: H, W must fit an int32")
    h32, w32 = H.astype(np.int32), W.astype(np.int32)
    geo = [None, None]
    if x_min is not None:
        geo = [np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1)) for v in (x_min, y_max)]
        if len(geo[0]) != K or len(geo[1]) != K:
            raise ValueError("atlas_canvas_table: x_min, y_max need one entry per canvas")
    table = np.zeros((K + 1, _lib.SN2_ATLAS_CANVAS_COLS), dtype=np.int64)
    check(_lib.load().sn2_atlas_canvas_table(K, h32.ctypes.data, w32.ctypes.data, *(None if g is None else g.ctypes.data for g in geo),
                                             table.ctypes.data), "sn2_atlas_canvas_table")
    return table


class AtlasTable:
    """The canvas table of a mosaic atlas on the host (`host`, numpy) and, with a device, on the device (`dev`): what the atlas
    entry points take.  K canvases; `pixels` = the sum of H W; base(k), shape(k) = (H, W), geo(k) = (x_min, y_max);
    view(arena, C, k): canvas k's zero-copy (C,H,W) view of a C-band arena."""

    def __init__(self, H, W, x_min=None, y_max=None, device=None):
        self.host = atlas_canvas_table(H, W, x_min, y_max)
        self.K = len(self.host) - 1
        self.pixels = int(self.host[self.K, 0])
        self.dev = None if device is None else torch.from_numpy(self.host).to(device)

    def base(self, k: int) -> int:
        return int(self.host[k, 0])

    def shape(self, k: int):
        return int(self.host[k, 1]), int(self.host[k, 2])

    def geo(self, k: int):
        g = self.host[k, 5:7].view(np.float64)
        return float(g[0]), float(g[1])

    def view(self, arena: torch.Tensor, C: int, k: int) -> torch.Tensor:
        (H, W), b = self.shape(k), self.base(k)
        return arena[C * b:C * (b + H * W)].view(C, H, W)


def atlas_segments(place, D: int, table: np.ndarray) -> np.ndarray:
    """The segment table of sn2_atlas_merge for one batch: place (B,3) = (canvas, row, col) per plot on the host, the canvases
    NON-DECREASING (else ValueError) -> (S+1, SN2_ATLAS_SEG_COLS) int32: per run of equal canvas [canvas, first plot, last plot + 1,
    y0, x0, h, w, first workgroup]; the window is the run's bounding window clipped to the canvas (h = w = 0 when nothing is left);
    row S holds the number of workgroups."""
    place = np.asarray(place).reshape(-1, 3).astype(np.int64)
    B, K = len(place), len(table) - 1
    if B == 0:
        raise ValueError("atlas_segments: no plot")
    c = place[:, 0]
    if (np.diff(c) < 0).any():
        raise ValueError("atlas_segments: the plots of a batch must come in non-decreasing canvas order")
    if c[0] < 0 or c[-1] >= K:
        raise ValueError(f"atlas_segments: canvas index outside [0, {K})")
    first = np.flatnonzero(np.concatenate([[True], c[1:] != c[:-1]]))
    canvas = c[first]
    H, W = table[canvas, 1], table[canvas, 2]
    y0 = np.clip(np.minimum.reduceat(place[:, 1], first), 0, H)
    y1 = np.clip(np.maximum.reduceat(place[:, 1], first) + D, 0, H)
    x0 = np.clip(np.minimum.reduceat(place[:, 2], first), 0, W)
    x1 = np.clip(np.maximum.reduceat(place[:, 2], first) + D, 0, W)
    some = (y1 > y0) & (x1 > x0)
    h, w = np.where(some, y1 - y0, 0), np.where(some, x1 - x0, 0)
    wg = -(-w // 64) * -(-h // 4)
    S = len(first)
    seg = np.zeros((S + 1, _lib.SN2_ATLAS_SEG_COLS), dtype=np.int64)
    seg[:S, 0], seg[:S, 1], seg[:S, 2] = canvas, first, np.concatenate([first[1:], [B]])
    seg[:S, 3], seg[:S, 4], seg[:S, 5], seg[:S, 6] = np.where(some, y0, 0), np.where(some, x0, 0), h, w
    seg[1:, 7] = np.cumsum(wg)
    if seg[S, 7] >= 2 ** 31:
        raise StrataHipError("atlas_segments: more than 2^31 - 1 workgroups (SN2_ELIMIT)")
    return seg.astype(np.int32)


def _arena(t, bands, table, name):
    return _chk(t, F32, (bands * table.pixels,), name)


def atlas_merge(rasters, weights, place, table: AtlasTable, mean, wsum):
    """include/strata_hip.h: sn2_atlas_merge.  Fold the plots of a batch, in order, each into ITS canvas of the atlas, in one
    launch.  rasters (B,3,D,D), weights (D,D) on the device; place (B,3) int = (canvas, row, col) on the HOST, canvases
    non-decreasing (ValueError otherwise); mean, wsum: the (3 pixels,) arenas, changed in place.  place and the segment table go
    to the device in one copy."""
    B, _, D, _ = rasters.shape
    _chk(rasters, F32, (B, 3, D, D), "rasters")
    _chk(weights, F32, (D, D), "weights")
    _arena(mean, 3, table, "mean")
    _arena(wsum, 3, table, "wsum")
    place = np.ascontiguousarray(np.asarray(place).reshape(-1, 3).astype(np.int32))
    if len(place) != B:
        raise ValueError(f"place: expected ({B},3), got {place.shape}")
    seg = np.ascontiguousarray(atlas_segments(place, D, table.host))
    S = len(seg) - 1
    both = torch.from_numpy(np.concatenate([place.reshape(-1), seg.reshape(-1)])).to(rasters.device)
    _call("sn2_atlas_merge", _ptr(rasters), _ptr(weights), _ptr(both), B, D, table.K, table.host.ctypes.data, _ptr(table.dev),
          seg.ctypes.data, both.data_ptr() + 4 * 3 * B, S, _ptr(mean), _ptr(wsum), _stream())


def atlas_finalize_ws_words(K: int) -> int:
    """SN2_ATLAS_FINALIZE_WS_WORDS of include/strata_hip.h (32-bit words)."""
    words = ctypes.c_size_t()
    check(_lib.load().sn2_atlas_finalize_ws_words(int(K), ctypes.byref(words)), "sn2_atlas_finalize_ws_words")
    return int(words.value)


def atlas_finalize(mean, wsum, table: AtlasTable, thr: Optional[torch.Tensor] = None):
    """include/strata_hip.h: sn2_atlas_finalize.  The arenas mean, wsum (3 pixels,) -> bands (5 pixels,): canvas k's (5,H,W) =
    [Vb, Vm_soft, Vh, Vm_hard, weights]; thr (K,2) = threshold, its index (written into `thr` when one is given)."""
    _arena(mean, 3, table, "mean")
    _arena(wsum, 3, table, "wsum")
    dev, K = mean.device, table.K
    ws = torch.empty(atlas_finalize_ws_words(K) // 2, dtype=F64, device=dev)
    thr = torch.empty(K, 2, dtype=F32, device=dev) if thr is None else _chk(thr, F32, (K, 2), "thr")
    bands = torch.empty(5 * table.pixels, dtype=F32, device=dev)
    _call("sn2_atlas_finalize", _ptr(mean), _ptr(wsum), K, table.host.ctypes.data, _ptr(table.dev), _ptr(ws), _ptr(thr), _ptr(bands),
          _stream())
    return bands, thr


def atlas_edges(edges, K: int):
    """edges: None, or K entries, each None or the (E,4) fp64 edges of that canvas's polygon (`parcel.polygon_edges`) ->
    (all edges (sum E,4) fp64 or None, edge_start (K+1) int32), on the host."""
    start = np.zeros(K + 1, dtype=np.int64)
    parts = []
    if edges is not None:
        if len(edges) != K:
            raise ValueError(f"edges: expected one entry per canvas ({K}), got {len(edges)}")
        for k, e in enumerate(edges):
            n = 0
            if e is not None:
                e = np.asarray(e, dtype=np.float64).reshape(-1, 4)
                n = len(e)
                if n == 0:
                    raise ValueError("edges: a canvas without a crop is given as None, not as an empty array")
                parts.append(e)
            start[k + 1] = start[k] + n
    if start[K] >= 2 ** 31:
        raise StrataHipError("atlas_edges: more than 2^31 - 1 edges (SN2_ELIMIT)")
    return (np.ascontiguousarray(np.concatenate(parts, 0)) if parts else None), start.astype(np.int32)


def atlas_crop_stats(bands, C: int, table: AtlasTable, pix: float, edges=None, out=None):
    """include/strata_hip.h: sn2_atlas_crop_stats.  bands: the (C pixels,) arena, CHANGED IN PLACE canvas by canvas as
    `mosaic_crop_stats` changes a single one, with the table's geotransforms; edges: as `atlas_edges` takes them (None, or None
    for a canvas: no crop, the statistics alone) -> (mean (K,C) fp64, count (K,C) int64) on the device.  Two launches, one
    host-to-device copy (the edges and their starts), no read-back."""
    _arena(bands, C, table, "bands")
    dev, K = bands.device, table.K
    e, start = atlas_edges(edges, K)
    n0 = (K + 2) // 2                                             # the int32 starts in front, padded to fp64 words
    buf = np.zeros(n0 + (0 if e is None else e.size), dtype=np.float64)
    buf[:n0].view(np.int32)[:K + 1] = start
    if e is not None:
        buf[n0:] = e.reshape(-1)
    both = torch.from_numpy(buf).to(dev)
    ws = torch.empty(max(2 * C * int(table.host[K, 4]), 1), dtype=F64, device=dev)
    if out is None:
        mean, count = torch.empty(K, C, dtype=F64, device=dev), torch.empty(K, C, dtype=I64, device=dev)
    else:
        mean, count = _chk(out[0], F64, (K, C), "out[0]"), _chk(out[1], I64, (K, C), "out[1]")
    _call("sn2_atlas_crop_stats", _ptr(bands), int(C), K, table.host.ctypes.data, _ptr(table.dev), float(pix),
          None if e is None else both.data_ptr() + 8 * n0, start.ctypes.data, both.data_ptr(), _ptr(ws), _ptr(mean), _ptr(count),
          _stream())
    return mean, count


# ---- the admissibility band (include/strata_hip.h, "Admissibility band"; csrc/admissibility.hip) --------------------------------
def admissibility_ws_words(pixels: int) -> int:
    """SN2_ADM_WS_WORDS of include/strata_hip.h (32-bit words) for a canvas, or an atlas, of `pixels` pixels."""
    words = ctypes.c_size_t()
    check(_lib.load().sn2_admissibility_ws_words(int(pixels), ctypes.byref(words)), "sn2_admissibility_ws_words")
    return int(words.value)


def _sieve_size(sieve_size) -> int:
    if isinstance(sieve_size, bool) or int(sieve_size) != sieve_size:
        raise ValueError(f"sieve_size: expected an integer >= 0, got {sieve_size!r}")
    return int(sieve_size)


def mosaic_admissibility(bands5: torch.Tensor, sieve_size: int, out=None):
    """include/strata_hip.h: sn2_mosaic_admissibility.  bands5 (5,H,W) fp32 = [Vb, Vm_soft, Vh, Vm_hard, weights] as
    `mosaic_finalize` leaves them, BEFORE any crop -> (bands6 (6,H,W) = [Vb, Vm_soft, Vh, Vm_hard, Adm, weights], stats (4) int64 =
    regions, regions smaller than sieve_size, sieved pixels, valid inaccessible pixels), both on the device.  The rule is the
    header's -- ours, not a pinned reference output.  sieve_size has NO default: 5 is the reading by the reference's comment
    ("Eliminate zones < 5 pixels"), 0 the reading by its call as written (the mask excludes the valid pixels: nothing is sieved).
    out: a (bands6, stats) pair of device tensors to write into.  A few launches on the current stream, no read-back; the same
    input gives the same bytes."""
    _chk(bands5, F32, None, "bands5")
    if bands5.dim() != 3 or bands5.shape[0] != 5:
        raise ValueError(f"bands5: expected (5,H,W), got {tuple(bands5.shape)}")
    _, H, W = bands5.shape
    s, dev = _sieve_size(sieve_size), bands5.device
    ws = torch.empty(admissibility_ws_words(H * W) // 2, dtype=F64, device=dev)
    if out is None:
        bands6, stats = torch.empty(6, H, W, dtype=F32, device=dev), torch.empty(4, dtype=I64, device=dev)
    else:
        bands6, stats = _chk(out[0], F32, (6, H, W), "out[0]"), _chk(out[1], I64, (4,), "out[1]")
    _call("sn2_mosaic_admissibility", _ptr(bands5), H, W, s, _ptr(ws), _ptr(bands6), _ptr(stats), _stream())
    return bands6, stats


def atlas_admissibility(bands5, table: AtlasTable, sieve_size: int, out=None):
    """include/strata_hip.h: sn2_atlas_admissibility.  bands5: the (5 pixels,) arena of `atlas_finalize` -> (bands6: the
    (6 pixels,) arena, canvas k's (6,H_k,W_k) = `table.view(bands6, 6, k)`; stats (K,4) int64), on the device: canvas by canvas
    the bytes `mosaic_admissibility` gives on that canvas's view.  out: a (bands6, stats) pair to write into."""
    _arena(bands5, 5, table, "bands5")
    s, dev, K = _sieve_size(sieve_size), bands5.device, table.K
    ws = torch.empty(admissibility_ws_words(table.pixels) // 2, dtype=F64, device=dev)
    if out is None:
        bands6, stats = torch.empty(6 * table.pixels, dtype=F32, device=dev), torch.empty(K, 4, dtype=I64, device=dev)
    else:
        bands6, stats = _arena(out[0], 6, table, "out[0]"), _chk(out[1], I64, (K, 4), "out[1]")
    _call("sn2_atlas_admissibility", _ptr(bands5), K, table.host.ctypes.data, _ptr(table.dev), s, _ptr(ws), _ptr(bands6), _ptr(stats),
          _stream())
    return bands6, stats


# ---- the per-point scores of a parcel cloud (include/strata_hip.h, "Per-point scores"; csrc/points.hip) -------------------------
POINTS_ACC_WORDS = _lib.SN2_POINTS_ACC_WORDS


def points_merge(cov, proba, xyz, idx, n_live, offsets, point_index, acc, hits, diam_meters: float, col_base=None):
    """include/strata_hip.h: sn2_points_merge.  cov, proba (B*N,4) fp32 of the eval forward, xyz (B,3,N) fp32 centred metres,
    idx (B,N) int32 the batch's subsample, n_live (B) int32, offsets (B+1) int32 the plots' positions in point_index (sum_n)
    int32, col_base (B) int32 or None -> the contributions of the batch added into acc (T, POINTS_ACC_WORDS) int64 and hits (T)
    int32 (both zeroed once by the caller).  One launch on the current stream, no read-back; 64-bit integer atomics, so the sums
    do not depend on batching or order."""
    _chk(idx, I32, None, "idx")
    if idx.dim() != 2:
        raise ValueError(f"idx: expected (B,N), got {tuple(idx.shape)}")
    B, N = idx.shape
    _chk(cov, F32, (B * N, 4), "cov")
    _chk(proba, F32, (B * N, 4), "proba")
    _chk(xyz, F32, (B, 3, N), "xyz")
    _chk(n_live, I32, (B,), "n_live")
    _chk(offsets, I32, (B + 1,), "offsets")
    _chk(point_index, I32, None, "point_index")
    if point_index.dim() != 1:
        raise ValueError(f"point_index: expected (sum_n,), got {tuple(point_index.shape)}")
    _chk(hits, I32, None, "hits")
    if hits.dim() != 1:
        raise ValueError(f"hits: expected (T,), got {tuple(hits.shape)}")
    T = hits.shape[0]
    _chk(acc, I64, (T, POINTS_ACC_WORDS), "acc")
    if col_base is not None:
        _chk(col_base, I32, (B,), "col_base")
    _call("sn2_points_merge", _ptr(cov), _ptr(proba), _ptr(xyz), _ptr(idx), _ptr(n_live), _ptr(offsets), _ptr(point_index),
          point_index.shape[0], _ptr(col_base), B, N, float(diam_meters), _ptr(acc), _ptr(hits), T, _stream())


def points_finalize(acc, hits, out=None):
    """include/strata_hip.h: sn2_points_finalize.  acc (T, POINTS_ACC_WORDS) int64 and hits (T) int32 of `points_merge` (left as
    they are) -> (scores (8,T) fp32 = the four coverages then the four class probabilities, weight (T) fp32): NaN scores and
    weight 0 where hits == 0.  out: a (scores, weight) pair to write into."""
    _chk(hits, I32, None, "hits")
    if hits.dim() != 1:
        raise ValueError(f"hits: expected (T,), got {tuple(hits.shape)}")
    T = hits.shape[0]
    _chk(acc, I64, (T, POINTS_ACC_WORDS), "acc")
    if out is None:
        scores, weight = torch.empty(8, T, dtype=F32, device=acc.device), torch.empty(T, dtype=F32, device=acc.device)
    else:
        scores, weight = _chk(out[0], F32, (8, T), "out[0]"), _chk(out[1], F32, (T,), "out[1]")
    _call("sn2_points_finalize", _ptr(acc), _ptr(hits), T, _ptr(scores), _ptr(weight), _stream())
    return scores, weight


# ---- the LAS decoder (include/strata_hip.h, "LAS point records"; csrc/las.hip) ---------------------------------------------------
LAS_COORDS = {"reference": _lib.SN2_LAS_COORDS_REFERENCE, "header": _lib.SN2_LAS_COORDS_HEADER}


def las_record_min_length(point_format: int) -> int:
    """sn2_las_record_min_length: the least record length of a LAS point format (ValueError for a format the decoder refuses)."""
    n = _lib.host_value("sn2_las_record_min_length", int(point_format))
    if n <= 0:
        raise ValueError(f"LAS point format {point_format}: not an uncompressed format 0..10")
    return n


def las_decode(raw, point_format: int, record_length: int, T: int, coords: str = "reference", xform=None, raw0=None, out=None,
               col0: int = 0, classification=None):
    """include/strata_hip.h: sn2_las_decode.  raw: uint8 device tensor that starts at the first record (16-byte aligned, at least
    T * record_length bytes) -> out (10, >= col0 + T) fp32, columns col0 .. col0 + T written (a new (10,T) tensor when None).
    coords "reference": raw0 = (X0, Y0, Z0) integers or None; "header": xform = 9 floats, scale xyz, offset xyz, origin xyz.
    classification: a uint8 tensor of out's row length (column col0 + i written) or None.  One launch on the current stream."""
    _chk(raw, torch.uint8, None, "raw")
    if raw.dim() != 1:
        raise ValueError(f"raw: expected a 1-D byte tensor, got {tuple(raw.shape)}")
    if coords not in LAS_COORDS:
        raise ValueError(f"coords: expected 'reference' or 'header', got {coords!r}")
    T, col0 = int(T), int(col0)
    if out is None:
        out = torch.empty(_lib.SN2_LAS_ROWS, T, dtype=F32, device=raw.device)
    row_stride = _chk_rows(out, F32, _lib.SN2_LAS_ROWS, col0 + T, "out", align=1)
    if out.device != raw.device:
        raise ValueError("out: must be on raw's device")
    if classification is not None:
        _chk(classification, torch.uint8, None, "classification")
        if classification.dim() != 1 or classification.shape[0] < col0 + T or classification.device != raw.device:
            raise ValueError(f"classification: expected (>= {col0 + T},) uint8 on raw's device")
    if T == 0:
        return out
    xf = None if xform is None else (ctypes.c_double * 9)(*[float(v) for v in xform])
    r0 = None if raw0 is None else (ctypes.c_longlong * 3)(*[int(v) for v in raw0])
    _call("sn2_las_decode", _ptr(raw), raw.numel(), int(point_format), int(record_length), T, LAS_COORDS[coords], xf, r0, _ptr(out),
          row_stride, col0, _ptr(classification), _stream())
    return out


# ---- the LAS encoder (include/strata_hip.h, "LAS point records, written"; csrc/las_write.hip) -----------------------------------
LAS_FIELDS = ("cov_low_veg", "cov_bare_soil", "cov_medium_veg", "cov_high_veg", "p_low_veg", "p_bare_soil", "p_medium_veg", "p_high_veg",
              "weight", "hits")          # bit k of field_mask; all fp32 but hits, a uint16


def las_field_mask(fields) -> int:
    """names out of LAS_FIELDS (any order, or "all") -> the 10-bit field_mask of sn2_las_encode"""
    if fields == "all":
        return _lib.SN2_LAS_FIELD_MASK_ALL
    if isinstance(fields, str):
        fields = (fields,)
    mask = 0
    for f in fields:
        if f not in LAS_FIELDS:
            raise ValueError(f"fields: {f!r} is none of {', '.join(LAS_FIELDS)}")
        mask |= 1 << LAS_FIELDS.index(f)
    return mask


def las_extra_bytes(field_mask: int) -> int:
    """E of the rule: four bytes per fp32 field, two for hits"""
    return 4 * bin(field_mask & 0x1FF).count("1") + 2 * ((field_mask >> 9) & 1)


def las_encode_stage_max() -> int:
    """sn2_las_encode_stage_max: the longest output record the encoder composes in LDS"""
    return _lib.host_value("sn2_las_encode_stage_max")


class LasEncodeStats:
    """The statistics block of sn2_las_encode on the device (`buf`, SN2_LAS_STATS_BYTES uint8), initialised here -- min = INT32_MAX,
    max = INT32_MIN, the counts 0 -- so that several launches can accumulate into it.  `read()` is ONE device-to-host copy and
    fills mins, maxs (raw integer X, Y, Z; None when nothing was written), by_return (15), n_bad, n_scored."""
    _LAYOUT = "<3i3i15QQQ"

    def __init__(self, device):
        import struct
        assert struct.calcsize(self._LAYOUT) == _lib.SN2_LAS_STATS_BYTES
        init = struct.pack(self._LAYOUT, *([2 ** 31 - 1] * 3), *([-2 ** 31] * 3), *([0] * 17))
        self.buf = torch.from_numpy(np.frombuffer(init, dtype=np.uint8).copy()).to(device)
        self.mins = self.maxs = self.by_return = self.n_bad = self.n_scored = None

    def read(self) -> "LasEncodeStats":
        import struct
        v = struct.unpack(self._LAYOUT, self.buf.cpu().numpy().tobytes())
        some = all(lo <= hi for lo, hi in zip(v[0:3], v[3:6]))
        self.mins, self.maxs = (tuple(v[0:3]), tuple(v[3:6])) if some else (None, None)
        self.by_return, self.n_bad, self.n_scored = tuple(v[6:21]), v[21], v[22]
        return self


def las_encode(raw, point_format: int, record_length: int, T_src: int, point_index=None, n_out=None, scores=None, weight=None,
               hits=None, col0: int = 0, field_mask: int = 0, class_codes=None, unscored: int = -1, out=None, stats=None):
    """include/strata_hip.h: sn2_las_encode.  raw: uint8 device tensor that starts at the first source record (16-byte aligned, at
    least T_src * record_length bytes).  point_index: int32 (T_out) source record of every output record, or None = record i.
    n_out: T_out (default: len(point_index), else T_src).  scores (8, >= col0 + T_out) fp32 with unit inner stride, weight fp32 and
    hits int32 (>= col0 + T_out): output record i takes column col0 + i; all three None for a pure copy.  class_codes: None = the
    classification stays, else the four codes of the classes (and `unscored`: the code of a point with hits == 0, -1 = its byte
    stays).  out: uint8 (>= T_out * L_dst), 16-byte aligned, or None.  stats: a `LasEncodeStats` to accumulate into, or None = a
    fresh one.  One launch on the current stream, no read-back.  -> (out[:T_out * L_dst], stats)"""
    _chk(raw, torch.uint8, None, "raw")
    if raw.dim() != 1:
        raise ValueError(f"raw: expected a 1-D byte tensor, got {tuple(raw.shape)}")
    T_src, col0, mask = int(T_src), int(col0), int(field_mask)
    if point_index is not None:
        _chk(point_index, I32, None, "point_index")
        if point_index.dim() != 1 or point_index.device != raw.device:
            raise ValueError("point_index: expected (T_out,) int32 on raw's device")
    T_out = int(n_out) if n_out is not None else (point_index.shape[0] if point_index is not None else T_src)
    if point_index is not None and point_index.shape[0] < T_out:
        raise ValueError(f"point_index: {point_index.shape[0]} entries for {T_out} records")
    if mask < 0 or mask > _lib.SN2_LAS_FIELD_MASK_ALL:
        raise ValueError(f"field_mask: expected 10 bits, got {mask:#x}")
    L_dst = int(record_length) + las_extra_bytes(mask)
    given = [t is not None for t in (scores, weight, hits)]
    if any(given) and not all(given):
        raise ValueError("scores, weight, hits: all three or none")
    if not any(given) and (mask or class_codes is not None):
        raise ValueError("fields or a classification need scores, weight and hits")
    stride = col0 + max(T_out, 1)
    if all(given):
        stride = _chk_rows(scores, F32, 8, col0 + T_out, "scores", align=1)
        for t, dt, name in ((weight, F32, "weight"), (hits, I32, "hits")):
            if (not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1 or t.shape[0] < col0 + T_out or t.stride(0) != 1
                    or t.device != raw.device):
                raise ValueError(f"{name}: expected (>= {col0 + T_out},) {dt} with unit stride on raw's device")
        if scores.device != raw.device:
            raise ValueError("scores: must be on raw's device")
    if out is None:
        out = torch.empty(max(T_out * L_dst, 16), dtype=torch.uint8, device=raw.device)
    _chk(out, torch.uint8, None, "out")
    if out.dim() != 1 or out.device != raw.device:
        raise ValueError("out: expected a 1-D byte tensor on raw's device")
    if stats is None:
        stats = LasEncodeStats(raw.device)
    if stats.buf.device != raw.device:
        raise ValueError("stats: must be on raw's device")
    if T_out == 0:
        return out[:0], stats
    codes = None if class_codes is None else (ctypes.c_int * 4)(*[int(c) for c in class_codes])
    _call("sn2_las_encode", _ptr(raw), raw.numel(), int(point_format), int(record_length), T_src, _ptr(point_index), T_out,
          _ptr(scores), _ptr(weight), _ptr(hits), stride, col0, mask, 0 if class_codes is None else 1, codes, int(unscored),
          _ptr(out), out.numel(), _ptr(stats.buf), _stream())
    return out[:T_out * L_dst], stats


# ---- the GeoTIFF band packer (include/strata_hip.h, "GeoTIFF image data"; csrc/tiff_pack.hip) --------------------------------------
TIFF_LAYOUTS = {"band": _lib.SN2_TIFF_LAYOUT_BAND, "pixel": _lib.SN2_TIFF_LAYOUT_PIXEL}


def tiff_pack_stage_max() -> int:
    """sn2_tiff_pack_stage_max: the longest row, in bytes (4 wc), the packer stages in LDS"""
    return _lib.host_value("sn2_tiff_pack_stage_max")


def tiff_layout(interleave) -> int:
    if interleave not in TIFF_LAYOUTS:
        raise ValueError(f"interleave: expected 'band' or 'pixel', got {interleave!r}")
    return TIFF_LAYOUTS[interleave]


def tiff_place_table(canvas_table: np.ndarray, C: int, layout: int, skip=None) -> np.ndarray:
    """sn2_tiff_place_table: the (K+1, SN2_TIFF_PLACE_COLS) int64 place table of the K canvases of a canvas table (host) for C bands
    in `layout`; skip: None or K flags, True = no file.  Host arithmetic, no device.  SN2_EINVAL / SN2_ELIMIT raise."""
    canvas_table = np.ascontiguousarray(canvas_table, dtype=np.int64)
    K = len(canvas_table) - 1
    flags = None
    if skip is not None:
        flags = np.ascontiguousarray(np.asarray(skip, dtype=bool).reshape(-1).astype(np.uint8))
        if len(flags) != K:
            raise ValueError(f"skip: expected one flag per canvas ({K}), got {len(flags)}")
    place = np.zeros((K + 1, _lib.SN2_TIFF_PLACE_COLS), dtype=np.int64)
    check(_lib.load().sn2_tiff_place_table(int(C), K, canvas_table.ctypes.data, int(layout), None if flags is None else flags.ctypes.data,
                                           place.ctypes.data), "sn2_tiff_place_table")
    return place


def tiff_key_bits(key: np.ndarray) -> np.ndarray:
    """the fp32 bit pattern of a statistics key (csrc/tiff_rules.h: tiff_key_bits)"""
    key = np.asarray(key, dtype=np.uint32)
    return key ^ np.where(key >> 31, np.uint32(0x80000000), np.uint32(0xFFFFFFFF)).astype(np.uint32)


class TiffPacked:
    """What sn2_tiff_pack leaves on the device: `buf` (uint8) holds every canvas's image data block at place[k, 0] and then the
    statistics.  `read()` is the ONE device-to-host copy; after it block(k) is canvas k's bytes (a uint8 view of the host copy, None
    without a file), counts (K,C) uint64, min_bits / max_bits (K,C) uint32 the fp32 bit patterns of the extrema (meaningless where
    the count is 0) and minimum / maximum (K,C) fp32 (NaN where the count is 0)."""

    def __init__(self, buf, place, C, K, layout, predictor):
        self.buf, self.place, self.C, self.K, self.layout, self.predictor = buf, place, C, K, layout, predictor
        self.total = int(place[K, 3])
        self.host = self.counts = self.min_bits = self.max_bits = self.minimum = self.maximum = None

    def read(self) -> "TiffPacked":
        if self.host is None:
            self.host = self.buf[:self.total].cpu().numpy()
            s = self.host[int(self.place[self.K, 0]):self.total].view(np.uint32).reshape(self.K, self.C, 4)
            self.counts = np.ascontiguousarray(s[:, :, 0:2]).view(np.uint64).reshape(self.K, self.C)
            self.min_bits, self.max_bits = tiff_key_bits(s[:, :, 2]), tiff_key_bits(s[:, :, 3])
            some = self.counts > 0
            self.minimum = np.where(some, self.min_bits.view(np.float32), np.float32(np.nan))
            self.maximum = np.where(some, self.max_bits.view(np.float32), np.float32(np.nan))
        return self

    def block(self, k: int):
        if self.host is None:
            raise ValueError("TiffPacked.block: read() first")
        if self.place[k, 1]:
            return None
        b = int(self.place[k, 0])
        return self.host[b:b + int(self.place[k, 3])]


def tiff_pack(band_arena, C: int, table: AtlasTable, layout: int = 0, predictor: int = 1, skip=None, out=None) -> TiffPacked:
    """include/strata_hip.h: sn2_tiff_pack.  band_arena: the (C pixels,) fp32 arena of `table`'s canvases, left as it is.  skip: None or
    K flags, True = that canvas gets no file.  out: None or a 1-D uint8 device tensor, 16-byte aligned, of at least the place
    table's total.  The statistics block is initialised here, on the stream; then ONE launch, no read-back."""
    C = int(C)
    _arena(band_arena, C, table, "band_arena")
    if table.dev is None or table.dev.device != band_arena.device:
        raise ValueError("table: needs its device copy on the arena's device")
    if predictor not in (1, 3):
        raise ValueError(f"predictor: expected 1 or 3, got {predictor!r}")
    place = tiff_place_table(table.host, C, layout, skip)
    K = table.K
    total, stats_off = int(place[K, 3]), int(place[K, 0])
    if out is None:
        out = torch.empty(total, dtype=torch.uint8, device=band_arena.device)
    _chk(out, torch.uint8, None, "out")
    if out.dim() != 1 or out.device != band_arena.device or out.numel() < total:
        raise ValueError(f"out: expected a 1-D byte tensor of at least {total} bytes on the arena's device")
    stats = out[stats_off:total].view(torch.int32).view(K * C, 4)            # count (two words), key of the minimum, of the maximum
    stats.zero_()
    stats[:, 2].fill_(-1)
    place_dev = torch.from_numpy(place).to(band_arena.device)
    _call("sn2_tiff_pack", _ptr(band_arena), C, K, table.host.ctypes.data, _ptr(table.dev), place.ctypes.data, _ptr(place_dev),
          int(layout), int(predictor), _ptr(out), out.numel(), _stream())
    packed = TiffPacked(out, place, C, K, int(layout), int(predictor))
    packed._place_dev = place_dev                                            # alive until the launch has run
    return packed


# ---- the dBase record annotator (include/strata_hip.h, "dBase records, annotated"; csrc/dbf.hip) ------------------------------------
class DbfAnnotated:
    """What sn2_dbf_annotate leaves on the device: `buf` (uint8) holds the K records of Ld bytes and, on the next multiple of 8, the
    uint64 overflow count.  `read()` is the ONE device-to-host copy; after it `records` is the (K, Ld) uint8 view of the host copy
    and `overflow` the number of fields filled with '*'."""

    def __init__(self, buf, K, Ld):
        self.buf, self.K, self.Ld = buf, K, Ld
        self.counter_at = (K * Ld + 7) // 8 * 8
        self.total = self.counter_at + 8
        self.host = self.records = self.overflow = None

    def read(self) -> "DbfAnnotated":
        if self.host is None:
            self.host = self.buf[:self.total].cpu().numpy()
            self.records = self.host[:self.K * self.Ld].reshape(self.K, self.Ld)
            self.overflow = int(self.host[self.counter_at:self.total].view(np.uint64)[0])
        return self


def dbf_annotate(records, values, row_of, cols, size: int = 50, decimal: int = 10, missing: float = -1.0, out=None) -> DbfAnnotated:
    """include/strata_hip.h: sn2_dbf_annotate.  records (K,L) uint8, values (R,C) fp64, row_of (K,) int32 (-1 = no row: `missing`),
    all contiguous on one device; cols: n host ints, the column of `values` each appended field is formatted from.  out: None or a
    1-D uint8 device tensor, 16-byte aligned, of at least K (L + n size) rounded up to 8, plus 8 bytes.  The overflow count is
    zeroed here, on the stream; then ONE launch, no read-back."""
    _chk(records, torch.uint8, None, "records")
    if records.dim() != 2 or records.shape[0] < 1 or records.shape[1] < 1:
        raise ValueError(f"records: expected (K,L) uint8 with K, L >= 1, got {tuple(records.shape)}")
    _chk(values, torch.float64, None, "values")
    if values.dim() != 2 or values.shape[0] < 1 or values.shape[1] < 1 or values.device != records.device:
        raise ValueError(f"values: expected (R,C) fp64 with R, C >= 1 on the records' device, got {tuple(values.shape)}")
    K, L = records.shape
    R, C = values.shape
    _chk(row_of, I32, (K,), "row_of")
    if row_of.device != records.device:
        raise ValueError("row_of: must be on the records' device")
    cols = [int(c) for c in cols]
    n, size, decimal = len(cols), int(size), int(decimal)
    Ld = L + n * size
    counter_at = (K * Ld + 7) // 8 * 8
    if out is None:
        out = torch.empty(counter_at + 8, dtype=torch.uint8, device=records.device)
    _chk(out, torch.uint8, None, "out")
    if out.dim() != 1 or out.device != records.device or out.numel() < counter_at + 8:
        raise ValueError(f"out: expected a 1-D byte tensor of at least {counter_at + 8} bytes on the records' device")
    out[counter_at:counter_at + 8].zero_()
    _call("sn2_dbf_annotate", _ptr(records), K, L, _ptr(values), R, C, _ptr(row_of), (ctypes.c_int * max(n, 1))(*cols), n, size, decimal,
          float(missing), _ptr(out), out.numel(), _stream())
    return DbfAnnotated(out, K, Ld)


# ---- the parcel cut (include/strata_hip.h, "Parcel cut"; csrc/cut.hip) -------------------------------------------------------------
CUT_ROW_POINTS = 2048         # points per wave of the count / fill passes (parcel.ROW_POINTS)
CUT_MAX_TABLE = 1 << 26       # (parcel, row) entries of the count table before rows get longer (parcel.MAX_TABLE)
CUT_CELL_SIDE = 32.0          # metres: the least cell side of the candidate grid


def cut_boxes(edge_lists, buffer_m: float) -> np.ndarray:
    """(K,4) fp64 = x_lo, y_lo, x_hi, y_hi: the bounding box of every parcel's vertices expanded by STRICTLY more than buffer_m --
    by buffer_m + 2^-40 (A + buffer_m + 1) with A the largest |coordinate| of the set, 4096 ulps of the largest quantity the rule
    or the differences `min - reach`, `max + reach` round.  A point the rule keeps lies inside."""
    b = float(buffer_m)
    lo = np.array([[e[:, 0].min(), e[:, 1].min()] for e in edge_lists], dtype=np.float64).reshape(-1, 2)
    hi = np.array([[e[:, 0].max(), e[:, 1].max()] for e in edge_lists], dtype=np.float64).reshape(-1, 2)
    amax = max(float(np.abs(lo).max()), float(np.abs(hi).max())) if len(lo) else 0.0
    reach = b + 2.0 ** -40 * (amax + b + 1.0)
    return np.concatenate([lo - reach, hi + reach], axis=1)


def cut_cell(v, g0: float, inv: float):
    """The cell of a coordinate along one axis, the kernels' floor((v - g0) * inv) in fp64 (monotonic in v)."""
    return np.floor((np.asarray(v, dtype=np.float64) - np.float64(g0)) * np.float64(inv))


class CutTable:
    """The candidate table of sn2_cut_count / sn2_cut_fill for K parcels and a cloud of T points, built on the host.
    edge_lists: per parcel its (E_k,4) fp64 edges (`parcel.polygon_edges`); buffer_m: b.  A uniform grid over the union of the
    expanded boxes (`cut_boxes`), parcel k listed in every cell from cell(lo_k) to cell(hi_k), ids ascending inside a cell; the
    cell side starts at max(cell_side, extent / 2048) and doubles until the grid has at most SN2_CUT_MAX_CELLS cells and
    SN2_CUT_MAX_ITEMS list entries (StrataHipError SN2_ELIMIT where one cell per axis still lists too many).  L: points per row,
    max(2048, ceil(K T / max_table) rounded up to 64).  `host`: the numpy arrays, `dev`: their device copies once `upload` ran;
    `struct()`: the sn2_cut_table.  The library checks the table before every launch; `ws_words` asks it once here."""

    def __init__(self, edge_lists, T: int, buffer_m: float, max_table: int = CUT_MAX_TABLE, cell_side: float = CUT_CELL_SIDE):
        edge_lists = [np.ascontiguousarray(np.asarray(e, dtype=np.float64).reshape(-1, 4)) for e in edge_lists]
        K, T, b = len(edge_lists), int(T), float(buffer_m)
        if K < 1 or any(len(e) == 0 for e in edge_lists):
            raise ValueError("CutTable: at least one parcel, and every parcel needs edges")
        if T < 1:
            raise ValueError("CutTable: the cloud holds no point")
        if not (math.isfinite(b) and b >= 0.0):
            raise ValueError(f"CutTable: buffer_m must be finite and >= 0, got {buffer_m}")
        if int(max_table) < 1 or not float(cell_side) > 0.0:
            raise ValueError("CutTable: max_table and cell_side must be positive")
        edges = np.concatenate(edge_lists, axis=0)
        if not np.isfinite(edges).all():
            raise ValueError("CutTable: a polygon vertex is not finite")
        boxes = cut_boxes(edge_lists, b)
        gx0, gy0 = float(boxes[:, 0].min()), float(boxes[:, 1].min())
        extent = max(float(boxes[:, 2].max()) - gx0, float(boxes[:, 3].max()) - gy0)
        side = max(float(cell_side), extent / 2048)
        while True:
            inv = 1.0 / side
            ix0, ix1 = cut_cell(boxes[:, 0], gx0, inv).astype(np.int64), cut_cell(boxes[:, 2], gx0, inv).astype(np.int64)
            iy0, iy1 = cut_cell(boxes[:, 1], gy0, inv).astype(np.int64), cut_cell(boxes[:, 3], gy0, inv).astype(np.int64)
            GX, GY = int(ix1.max()) + 1, int(iy1.max()) + 1
            per = (ix1 - ix0 + 1) * (iy1 - iy0 + 1)
            if GX * GY <= _lib.SN2_CUT_MAX_CELLS and int(per.sum()) <= _lib.SN2_CUT_MAX_ITEMS:
                break
            if GX == 1 and GY == 1:
                raise StrataHipError(f"CutTable failed: SN2_ELIMIT {_lib.SN2_ELIMIT} ({K} parcels in one cell)")
            side *= 2.0
        # parcel k's cells, parcel after parcel; the stable sort by cell keeps the ids ascending inside a cell
        ids = np.repeat(np.arange(K, dtype=np.int64), per)
        first = np.concatenate([[0], np.cumsum(per)])[:-1]
        j = np.arange(int(per.sum()), dtype=np.int64) - np.repeat(first, per)
        w = np.repeat(ix1 - ix0 + 1, per)
        cell = (np.repeat(iy0, per) + j // w) * GX + np.repeat(ix0, per) + j % w
        order = np.argsort(cell, kind="stable")
        cell_start = np.zeros(GX * GY + 1, dtype=np.int64)
        np.cumsum(np.bincount(cell, minlength=GX * GY), out=cell_start[1:])
        edge_start = np.concatenate([[0], np.cumsum([len(e) for e in edge_lists])])
        if edge_start[-1] >= 2 ** 31:
            raise StrataHipError(f"CutTable failed: SN2_ELIMIT {_lib.SN2_ELIMIT} ({edge_start[-1]} edges)")
        L = max(CUT_ROW_POINTS, (-(-(K * T) // int(max_table)) + 63) // 64 * 64)
        if L >= 2 ** 31:
            raise StrataHipError(f"CutTable failed: SN2_ELIMIT {_lib.SN2_ELIMIT} (row length {L})")
        self.K, self.T, self.buffer, self.L, self.GX, self.GY = K, T, b, int(L), GX, GY
        self.gx0, self.gy0, self.inv = gx0, gy0, inv
        self.rows = -(-T // self.L)
        self.boxes = boxes
        self.host = [cell_start.astype(np.int32), ids[order].astype(np.int32), edge_start.astype(np.int32), np.ascontiguousarray(edges)]
        self.dev = None
        self.ws_words = self._ws_words()

    def struct(self) -> "_lib.CutTable":
        t = _lib.CutTable()
        t.K, t.GX, t.GY, t.L, t.T = self.K, self.GX, self.GY, self.L, self.T
        t.n_items, t.n_edges = len(self.host[1]), len(self.host[3])
        t.gx0, t.gy0, t.inv, t.buffer = self.gx0, self.gy0, self.inv, self.buffer
        t.cell_start, t.cell_items, t.edge_start, t.edges = (a.ctypes.data for a in self.host)
        if self.dev is not None:
            t.cell_start_dev, t.cell_items_dev, t.edge_start_dev, t.edges_dev = (_ptr(d) for d in self.dev)
        return t

    def _ws_words(self) -> int:
        n = ctypes.c_size_t()
        check(_lib.load().sn2_cut_ws_words(ctypes.byref(self.struct()), ctypes.byref(n)), "sn2_cut_ws_words")
        return n.value

    def upload(self, device):
        """the four arrays to `device` in one copy"""
        self.dev = pack_upload(self.host, device)
        return self


def cut_drop_words(drop_classes) -> np.ndarray:
    """The 256-bit drop set of sn2_cut_count / _fill as 8 uint32 words: bit c of word c // 32 for every class c in 0..255."""
    w = np.zeros(8, dtype=np.uint32)
    for c in drop_classes:
        if int(c) != c or not 0 <= int(c) <= 255:
            raise ValueError(f"drop_classes: a LAS class is an integer in 0..255, got {c!r}")
        w[int(c) >> 5] |= np.uint32(1 << (int(c) & 31))
    return w


def _chk_cut(cloud, table: CutTable, classification, drop):
    _chk(cloud, F32, (10, table.T), "cloud")
    if table.dev is None:
        raise ValueError("table: not uploaded (CutTable.upload)")
    for d, a, name in zip(table.dev, table.host, ("cell_start", "cell_items", "edge_start", "edges")):
        _chk(d, torch.from_numpy(a).dtype, a.shape, f"table.{name}")
        if d.device != cloud.device:
            raise ValueError(f"table.{name}: must be on the cloud's device")
    if (classification is None) != (drop is None):
        raise ValueError("classification and drop: both or neither")
    if classification is not None:
        _chk(classification, torch.uint8, (table.T,), "classification")
        if classification.device != cloud.device:
            raise ValueError("classification: must be on the cloud's device")
        drop = np.ascontiguousarray(drop, dtype=np.uint32)
        if drop.shape != (8,):
            raise ValueError("drop: expected 8 uint32 words (cut_drop_words)")
    return drop


def cut_count(cloud: torch.Tensor, table: CutTable, classification: Optional[torch.Tensor] = None, drop=None):
    """include/strata_hip.h: sn2_cut_count.  cloud (10,T) f32; classification (T) u8 and drop (8 words, `cut_drop_words`) or neither
    -> (prefix (K rows + 1) i32, parcel_start (K+1) i64 with the total last)."""
    drop = _chk_cut(cloud, table, classification, drop)
    dev = cloud.device
    ws = torch.empty(table.ws_words + 4, dtype=I32, device=dev)
    prefix = torch.empty(table.K * table.rows + 1, dtype=I32, device=dev)
    starts = torch.empty(table.K + 2, dtype=I64, device=dev)               # parcel_start, then the scan's own total word
    _call("sn2_cut_count", _ptr(cloud), _ptr(classification), None if drop is None else drop.ctypes.data, ctypes.byref(table.struct()),
          _ptr(ws), table.ws_words, _ptr(prefix), _ptr(starts), _stream())
    return prefix, starts[:table.K + 1]


def cut_fill(cloud: torch.Tensor, table: CutTable, prefix: torch.Tensor, parcel_base: torch.Tensor, sum_n: int,
             classification: Optional[torch.Tensor] = None, drop=None):
    """include/strata_hip.h: sn2_cut_fill.  prefix: cut_count's (consumed); parcel_base (K) i32, INT_MIN = parcel skipped
    -> out (10,sum_n) f32, point_index (sum_n) i32: the cloud's column of every column of out."""
    drop = _chk_cut(cloud, table, classification, drop)
    _chk(prefix, I32, (table.K * table.rows + 1,), "prefix")
    _chk(parcel_base, I32, (table.K,), "parcel_base")
    sum_n = int(sum_n)
    if not 0 < sum_n < 2 ** 31:
        raise ValueError(f"sum_n: expected 1 .. 2^31 - 1, got {sum_n}")
    out = torch.empty(10, sum_n, dtype=F32, device=cloud.device)
    pidx = torch.empty(sum_n, dtype=I32, device=cloud.device)
    _call("sn2_cut_fill", _ptr(cloud), _ptr(classification), None if drop is None else drop.ctypes.data, ctypes.byref(table.struct()),
          _ptr(prefix), _ptr(parcel_base), sum_n, _ptr(out), _ptr(pidx), _stream())
    return out, pidx


# ---- the orthoimage colours (include/strata_hip.h, "Orthoimage colours"; csrc/ortho.hip) -------------------------------------------
ORTHO_DTYPES = {"uint8": (_lib.SN2_ORTHO_U8, 1), "uint16": (_lib.SN2_ORTHO_U16, 2), "float32": (_lib.SN2_ORTHO_F32, 4)}
ORTHO_LAYOUTS = {"chunky": _lib.SN2_ORTHO_CHUNKY, "planar": _lib.SN2_ORTHO_PLANAR}


def ortho_check_mapping(C: int, bands, rows, scale):
    """The (band, row) pairs of one call, checked before the library: 1 to SN2_ORTHO_MAX_MAP pairs, bands in [0, C), rows
    distinct and in 3..9 (0 and 1 are the call's input), a finite scale."""
    bands, rows = tuple(bands), tuple(rows)
    if len(bands) != len(rows) or not 1 <= len(bands) <= _lib.SN2_ORTHO_MAX_MAP:
        raise ValueError(f"bands, rows: 1 to {_lib.SN2_ORTHO_MAX_MAP} (band, row) pairs, got {len(bands)} bands and {len(rows)} rows")
    for b in bands:
        if int(b) != b or not 0 <= b < C:
            raise ValueError(f"bands: band {b!r} of an image of {C}")
    for r in rows:
        if int(r) != r or not 3 <= r <= 9:
            raise ValueError(f"rows: row {r!r}; the rows a call may write are 3..9 (0 and 1 are read)")
    if len(set(rows)) != len(rows):
        raise ValueError(f"rows: {rows} are not distinct")
    if not math.isfinite(float(scale)):
        raise ValueError(f"scale: expected a finite number, got {scale!r}")


def ortho_set_struct(images, dtype: str, C: int, layout: str, bands, rows, scale: float, nodata=None) -> "_lib.OrthoSet":
    """The sn2_ortho_set of one call.  images: up to SN2_ORTHO_MAX_IMAGES tuples (pixels: device address, x0, y0, px, py, W, H);
    dtype: a key of ORTHO_DTYPES, layout: a key of ORTHO_LAYOUTS.  What can be refused without the library is refused here."""
    images = list(images)
    if dtype not in ORTHO_DTYPES:
        raise ValueError(f"dtype: expected one of {tuple(ORTHO_DTYPES)}, got {dtype!r}")
    if layout not in ORTHO_LAYOUTS:
        raise ValueError(f"layout: expected one of {tuple(ORTHO_LAYOUTS)}, got {layout!r}")
    if not 1 <= len(images) <= _lib.SN2_ORTHO_MAX_IMAGES:
        raise ValueError(f"images: 1 to {_lib.SN2_ORTHO_MAX_IMAGES}, got {len(images)}")
    if int(C) < 1:
        raise ValueError(f"C: at least one band, got {C}")
    ortho_check_mapping(C, bands, rows, scale)
    if nodata is not None and math.isnan(float(nodata)):
        raise ValueError("nodata: must not be NaN")
    s = _lib.OrthoSet()
    s.S, s.C, s.dtype, s.layout, s.n_map = len(images), int(C), ORTHO_DTYPES[dtype][0], ORTHO_LAYOUTS[layout], len(tuple(bands))
    s.has_nodata, s.nodata, s.scale = int(nodata is not None), 0.0 if nodata is None else float(nodata), float(scale)
    for k, (b, r) in enumerate(zip(bands, rows)):
        s.band[k], s.row[k] = int(b), int(r)
    for im, (ptr, x0, y0, px, py, W, H) in zip(s.image, images):
        im.pixels, im.x0, im.y0, im.px, im.py, im.W, im.H = ptr, float(x0), float(y0), float(px), float(py), int(W), int(H)
    return s


def ortho_colorize(cloud: torch.Tensor, oset: "_lib.OrthoSet", col0: int = 0, T: Optional[int] = None, covered: Optional[torch.Tensor] = None,
                   missing: Optional[torch.Tensor] = None) -> torch.Tensor:
    """include/strata_hip.h: sn2_ortho_colorize.  cloud (10, n) fp32 with unit stride along n (its row stride may be larger: a
    column view of an arena); the columns col0 .. col0 + T (T None: all from col0) are coloured in place.  covered (T) u8 or None;
    missing (1) i64, ADDED to (None: a fresh zero) -> missing.  The images' pixel buffers are the caller's to keep alive and to
    size (W H C samples each)."""
    if not isinstance(cloud, torch.Tensor) or not cloud.is_cuda or cloud.dtype != F32 or cloud.dim() != 2 or cloud.shape[0] != 10:
        raise ValueError("cloud: expected a (10,T) fp32 tensor on the HIP device")
    n = cloud.shape[1]
    if n > 1 and cloud.stride(1) != 1:
        raise ValueError("cloud: unit stride along the points")
    row_stride = max(cloud.stride(0), n)
    col0 = int(col0)
    T = n - col0 if T is None else int(T)
    if col0 < 0 or T < 0 or col0 + T > n:
        raise ValueError(f"col0, T: columns {col0} .. {col0 + T} of a cloud of {n}")
    if covered is not None:
        _chk(covered, torch.uint8, (T,), "covered")
    if missing is None:
        missing = torch.zeros(1, dtype=I64, device=cloud.device)
    _chk(missing, I64, (1,), "missing")
    for t, name in ((covered, "covered"), (missing, "missing")):
        if t is not None and t.device != cloud.device:
            raise ValueError(f"{name}: must be on the cloud's device")
    _call("sn2_ortho_colorize", _ptr(cloud), row_stride, col0, T, ctypes.byref(oset), _ptr(covered), _ptr(missing), _stream())
    return missing


LOSS_BLOCKS = _lib.SN2_LOSS_BLOCKS


def kde_lookup(clouds_dev: torch.Tensor, z_max: float, X: torch.Tensor, Y: torch.Tensor, z_channel: int = 2,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """clouds (B,C,N) fp32 on the device, X (K) / Y (3,K) fp64 interpolation tables -> pdf_all (B*N,3) fp64 (into `out` when
    one is given)."""
    B, C, N = clouds_dev.shape
    _chk(clouds_dev, F32, (B, C, N), "clouds")
    K = X.shape[0]
    _chk(X, F64, (K,), "X")
    _chk(Y, F64, (3, K), "Y")
    if K < 2 or not (0 <= z_channel < C):
        raise ValueError("kde_lookup: need K >= 2 knots and a valid z channel")
    pdf = torch.empty(B * N, 3, dtype=F64, device=clouds_dev.device) if out is None else _chk(out, F64, (B * N, 3), "out")
    _call("sn2_kde_lookup", _ptr(clouds_dev), B, C, N, int(z_channel), float(z_max), _ptr(X), _ptr(Y), K, _ptr(pdf), _stream())
    return pdf


KDE_FIT_MAX_K = _lib.SN2_KDE_FIT_MAX_K


def kde_fit_ws_words(K: int) -> int:
    """SN2_KDE_FIT_WS_WORDS of include/strata_hip.h (32-bit words)."""
    return _host("sn2_kde_fit_ws_words", max(int(K), 2))


def kde_fit(z_dev: torch.Tensor, bw: float = 0.1, grid_points: int = 5000):
    """include/strata_hip.h: sn2_kde_fit.  z (n) fp32 FINITE heights in metres on the device -> (X (K), Y (3,K)) fp64, the tables
    `kde_lookup` takes: the reference's `KdeMixture.fit` + `evaluate_kdes`.  Four launches on the current stream and no read-back
    (the finiteness check is the caller's: `losses.KdeTables.fit` makes it); the same input gives the same bytes.  n = 0, K < 2
    and bw <= 0 are refused by the library (SN2_EINVAL), K > KDE_FIT_MAX_K too (SN2_ELIMIT)."""
    _chk(z_dev, F32, None, "z")
    if z_dev.dim() != 1:
        raise ValueError(f"z: expected a 1-D tensor of heights, got {tuple(z_dev.shape)}")
    K = int(grid_points)
    dev = z_dev.device
    ws = torch.empty(kde_fit_ws_words(K) // 2 + 1, dtype=F64, device=dev)
    X = torch.empty(max(K, 2), dtype=F64, device=dev)
    Y = torch.empty(3, max(K, 2), dtype=F64, device=dev)
    _call("sn2_kde_fit", _ptr(z_dev) or None, z_dev.numel(), float(bw), K, _ptr(ws), _ptr(X), _ptr(Y), _stream())
    return X, Y


def loss_forward(pred, gt, proba, pdf, m: float, e: float):
    """-> out (4,) fp64 = [total, absolute, NLL, entropy] (include/strata_hip.h: sn2_loss_forward)."""
    B, R = pred.shape[0], proba.shape[0]
    _chk(pred, F32, (B, 4), "pred")
    _chk(gt, F64, (B, 4), "gt")
    _chk(proba, F32, (R, 4), "proba")
    _chk(pdf, F64, (R, 3), "pdf")
    partials = torch.empty(2 * LOSS_BLOCKS, dtype=F64, device=pred.device)
    out = torch.empty(4, dtype=F64, device=pred.device)
    _call("sn2_loss_forward", _ptr(pred), _ptr(gt), B, _ptr(proba), _ptr(pdf), R, float(m), float(e), _ptr(partials),
          _ptr(out), _stream())
    return out


def loss_backward(pred, gt, proba, pdf, m: float, e: float, grad_total):
    B, R = pred.shape[0], proba.shape[0]
    _chk(grad_total, F64, None, "grad_total")
    dpred = torch.empty(B, 4, dtype=F32, device=pred.device)
    dproba = torch.empty(R, 4, dtype=F32, device=pred.device)
    _call("sn2_loss_backward", _ptr(pred), _ptr(gt), B, _ptr(proba), _ptr(pdf), R, float(m), float(e), _ptr(grad_total),
          _ptr(dpred), _ptr(dproba), _stream())
    return dpred, dproba


PROJECTED_LOSS_WS = _lib.SN2_PROJECTED_LOSS_WS


def projected_loss_forward(cov, pix, proba, pdf, gt, B: int, N: int, diam_pix: int, m: float, e: float):
    """include/strata_hip.h: sn2_projected_loss_forward -> (out (4,) fp64 = total, absolute, NLL, entropy; pred (B,4); arg, nocc)."""
    R, D = B * N, int(diam_pix)
    _chk(cov, F32, (R, 4), "coverages")
    _chk(pix, I32, (R,), "pix")
    _chk(proba, F32, (R, 4), "proba")
    _chk(pdf, F64, (R, 3), "pdf")
    _chk(gt, F64, (B, 4), "gt")
    dev = cov.device
    keys = torch.empty(p2_key_parts(N) * B * D * D * 3, dtype=I64, device=dev)
    arg = torch.empty(B * D * D * 3, dtype=I32, device=dev)
    nocc = torch.empty(B, dtype=I32, device=dev)
    pred = torch.empty(B, 4, dtype=F32, device=dev)
    partials = torch.empty(PROJECTED_LOSS_WS, dtype=F64, device=dev)
    out = torch.empty(4, dtype=F64, device=dev)
    _call("sn2_projected_loss_forward", _ptr(cov), _ptr(pix), _ptr(proba), _ptr(pdf), _ptr(gt), B, N, D, float(m), float(e), _ptr(keys),
          _ptr(arg), _ptr(nocc), _ptr(pred), _ptr(partials), _ptr(out), _stream())
    return out, pred, arg, nocc


def projected_loss_backward(pred, gt, proba, pdf, B: int, N: int, diam_pix: int, m: float, e: float, grad_total, arg, nocc, pix):
    """include/strata_hip.h: sn2_projected_loss_backward -> (d loss / d coverages, d loss / d proba), (B*N,4) each."""
    R = B * N
    _chk(grad_total, F64, None, "grad_total")
    dcov = torch.empty(R, 4, dtype=F32, device=pred.device)
    dproba = torch.empty(R, 4, dtype=F32, device=pred.device)
    _call("sn2_projected_loss_backward", _ptr(pred), _ptr(gt), B, _ptr(proba), _ptr(pdf), N, int(diam_pix), float(m), float(e),
          _ptr(grad_total), _ptr(arg), _ptr(nocc), _ptr(pix), _ptr(dcov), _ptr(dproba), _stream())
    return dcov, dproba


def plot_losses_ws_words(B: int, N: int, diam_pix: int) -> int:
    """32-bit words of `plot_losses`' workspace (include/strata_hip.h: sn2_plot_losses_ws_words); 0 = beyond what the kernels cover."""
    return int(_lib.load().sn2_plot_losses_ws_words(int(B), int(N), int(diam_pix)))


def plot_losses(cov, pix, proba, pdf, gt, B: int, N: int, diam_pix: int, m: float, e: float, out=None, ws=None):
    """include/strata_hip.h: sn2_plot_losses -> (out (B,7) fp64 = per plot total, absolute, NLL, entropy, abs_low, abs_med,
    abs_high; pred (B,4) fp32).  pdf may be None when m == 0.  out = (out, pred): caller-owned buffers (rows of a larger table);
    ws: caller-owned workspace of at least `plot_losses_ws_words` int32 words."""
    R, D = B * N, int(diam_pix)
    m, e = float(m), float(e)
    _chk(cov, F32, (R, 4), "coverages")
    _chk(pix, I32, (R,), "pix")
    _chk(proba, F32, (R, 4), "proba")
    if m != 0.0 or pdf is not None:
        _chk(pdf, F64, (R, 3), "pdf")
    _chk(gt, F64, (B, 4), "gt")
    dev = cov.device
    words = plot_losses_ws_words(B, N, D)
    if words == 0:
        raise StrataHipError(f"plot_losses: B={B}, N={N}, diam_pix={D} is outside what the kernels cover (SN2_ELIMIT)")
    if ws is None:
        ws = torch.empty(words, dtype=I32, device=dev)
    else:
        _chk(ws, I32, None, "ws")
        if ws.numel() < words or ws.data_ptr() % 8:
            raise ValueError(f"ws: need {words} int32 words, 8-byte aligned")
    if out is None:
        o, pred = torch.empty(B, 7, dtype=F64, device=dev), torch.empty(B, 4, dtype=F32, device=dev)
    else:
        o, pred = out
        _chk(o, F64, (B, 7), "out")
        _chk(pred, F32, (B, 4), "out pred")
    _call("sn2_plot_losses", _ptr(cov), _ptr(pix), _ptr(proba), _ptr(pdf) if m != 0.0 else None, _ptr(gt), B, N, D, m, e, _ptr(ws),
          _ptr(pred), _ptr(o), _stream())
    return o, pred


CV_COLUMNS, CV_STATS_DOUBLES, CV_MAX_PLOTS = (_lib.CONSTANTS[n] for n in ("SN2_CV_COLUMNS", "SN2_CV_STATS_DOUBLES", "SN2_CV_MAX_PLOTS"))


def cv_indicators_ws_words(P: int) -> int:
    """32-bit words of `cv_indicators`' workspace (include/strata_hip.h: sn2_cv_indicators_ws_words); 0 = more plots than the
    kernels cover."""
    words = ctypes.c_size_t()
    rc = _lib.load().sn2_cv_indicators_ws_words(int(P), ctypes.byref(words))
    if rc not in (0, _lib.SN2_ELIMIT):
        check(rc, "sn2_cv_indicators_ws_words")
    return int(words.value)


def cv_indicators(pred, gt, relabel: bool, ws=None):
    """include/strata_hip.h: sn2_cv_indicators -> (rows (P,30) fp64, cls (P,9) int32, stats (SN2_CV_STATS_DOUBLES) fp64) on the
    device, two launches on the current stream: the indicators of `learning/accuracy.py` per plot (V1, V2, V3), the true / predicted /
    margin-adjusted classes, and the column sums, non-NaN counts, confusion counts and the number of continuous rows.  pred (P,4)
    fp32, gt (P,4) fp64; relabel: the ground truths are first moved to their closest class centres.  The reference's two oddities are
    kept as written: acc_all is the mean of TWO strata, error3_all takes error2 of the medium stratum.
    ws: caller-owned workspace of at least `cv_indicators_ws_words(P)` int32 words (None: allocated here)."""
    if not isinstance(pred, torch.Tensor) or pred.dim() != 2:
        raise ValueError("pred: expected a (P,4) tensor")
    P = int(pred.shape[0])
    _chk(pred, F32, (P, 4), "pred")
    _chk(gt, F64, (P, 4), "gt")
    if P < 1:
        raise ValueError("cv_indicators: no plots")
    words = cv_indicators_ws_words(P)
    if words == 0:
        raise StrataHipError(f"cv_indicators: P={P} is more than the kernels cover ({CV_MAX_PLOTS}: SN2_ELIMIT)")
    dev = pred.device
    if ws is None:
        ws = torch.empty(words, dtype=I32, device=dev)
    else:
        _chk(ws, I32, None, "ws")
        if ws.numel() < words or ws.data_ptr() % 8:
            raise ValueError(f"ws: need {words} int32 words, 8-byte aligned")
    rows = torch.empty(P, CV_COLUMNS, dtype=F64, device=dev)
    cls = torch.empty(P, 9, dtype=I32, device=dev)
    stats = torch.empty(CV_STATS_DOUBLES, dtype=F64, device=dev)
    if pred.data_ptr() % 16 or rows.data_ptr() % 16:
        raise ValueError("cv_indicators: pred and rows must be 16-byte aligned")
    _call("sn2_cv_indicators", _ptr(pred), _ptr(gt), P, int(bool(relabel)), _ptr(rows), _ptr(cls), _ptr(stats), _ptr(ws), _stream())
    return rows, cls, stats


def adam_step_images(param, arena, replicas, stride, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step_dev, grad_scale=1.0):
    """include/strata_hip.h: sn2_adam_step_images -- fold the gradient's images and take the Adam step in one launch."""
    n = param.numel()
    for t, nme in ((param, "param"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _chk(t, F32, (n,), nme)
    _chk(arena, F32, None, "arena")
    if arena.numel() < replicas * stride or stride < n:
        raise ValueError("adam_step_images: arena smaller than its images")
    _chk(step_dev, I32, (2,), "step_dev")
    _call("sn2_adam_step_images", _ptr(param), _ptr(arena), int(replicas), int(stride), _ptr(exp_avg), _ptr(exp_avg_sq), n, lr, beta1,
          beta2, eps, weight_decay, _ptr(step_dev), grad_scale, _stream())


METER_TERMS = _lib.SN2_METER_TERMS           # sums of the optimiser's epoch meter (followed by the number of steps added)


def _chk_lr_meter(lr_dev, terms, meter, who):
    """The arguments sn2_adam_step_dev / sn2_adam_step_images_dev add: lr_dev fp32 (1,); terms None or fp64, contiguous, 1 to
    METER_TERMS elements, then meter fp64 (METER_TERMS + 1,).  -> n_terms"""
    _chk(lr_dev, F32, (1,), "lr_dev")
    if terms is None:
        return 0
    _chk(terms, F64, None, "terms")
    if not 1 <= terms.numel() <= METER_TERMS:
        raise ValueError(f"{who}: terms holds {terms.numel()} values, the meter takes 1 to {METER_TERMS}")
    _chk(meter, F64, (METER_TERMS + 1,), "meter")
    return terms.numel()


def adam_step_images_dev(param, arena, replicas, stride, exp_avg, exp_avg_sq, lr_dev, beta1, beta2, eps, weight_decay, step_dev,
                         grad_scale=1.0, terms=None, meter=None):
    """include/strata_hip.h: sn2_adam_step_images_dev -- adam_step_images with the learning rate read from the device word
    `lr_dev` when the kernel runs, and `terms` (this step's loss terms) added to `meter` by the launch's last thread."""
    n = param.numel()
    for t, nme in ((param, "param"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _chk(t, F32, (n,), nme)
    _chk(arena, F32, None, "arena")
    if arena.numel() < replicas * stride or stride < n:
        raise ValueError("adam_step_images_dev: arena smaller than its images")
    _chk(step_dev, I32, (2,), "step_dev")
    n_terms = _chk_lr_meter(lr_dev, terms, meter, "adam_step_images_dev")
    _call("sn2_adam_step_images_dev", _ptr(param), _ptr(arena), int(replicas), int(stride), _ptr(exp_avg), _ptr(exp_avg_sq), n,
          _ptr(lr_dev), beta1, beta2, eps, weight_decay, _ptr(step_dev), grad_scale, _ptr(terms), n_terms,
          _ptr(meter) if n_terms else None, _stream())


def loss_term_forward(kind: int, x: torch.Tensor, y: Optional[torch.Tensor]):
    """ONE term of the loss (the reference's loop calls them one by one, learning/train.py:58-60) -> out (4,) fp64 with
    out[kind] = the term: kind 1 = absolute (x = pred (B,4), y = gt (B,4) fp64), 2 = NLL (x = proba (R,4), y = pdf (R,3) fp64),
    3 = entropy (x = proba (R,4)).  The other terms are skipped inside sn2_loss_forward (their inputs are not passed)."""
    out = torch.empty(4, dtype=F64, device=x.device)
    if kind == 1:
        B = x.shape[0]
        _chk(x, F32, (B, 4), "pred")
        _chk(y, F64, (B, 4), "gt")
        _call("sn2_loss_forward", _ptr(x), _ptr(y), B, None, None, 0, 0.0, 0.0, None, _ptr(out), _stream())
        return out
    R = x.shape[0]
    _chk(x, F32, (R, 4), "proba")
    partials = torch.empty(2 * LOSS_BLOCKS, dtype=F64, device=x.device)
    if kind == 2:
        _chk(y, F64, (R, 3), "pdf")
        _call("sn2_loss_forward", None, None, 0, _ptr(x), _ptr(y), R, 1.0, 0.0, _ptr(partials), _ptr(out), _stream())
    elif kind == 3:
        _call("sn2_loss_forward", None, None, 0, _ptr(x), None, R, 0.0, 1.0, _ptr(partials), _ptr(out), _stream())
    else:
        raise ValueError("loss term kind must be 1, 2 or 3")
    return out


def loss_term_backward(kind: int, x: torch.Tensor, y: Optional[torch.Tensor], grad: torch.Tensor):
    """d term / d x for the upstream gradient `grad` (fp64 device scalar) of that one term."""
    _chk(grad, F64, None, "grad")
    dx = torch.empty_like(x)
    if kind == 1:
        _call("sn2_loss_backward", _ptr(x), _ptr(y), x.shape[0], None, None, 0, 0.0, 0.0, _ptr(grad), _ptr(dx), None, _stream())
    elif kind == 2:
        _call("sn2_loss_backward", None, None, 0, _ptr(x), _ptr(y), x.shape[0], 1.0, 0.0, _ptr(grad), None, _ptr(dx), _stream())
    else:
        _call("sn2_loss_backward", None, None, 0, _ptr(x), None, x.shape[0], 0.0, 1.0, _ptr(grad), None, _ptr(dx), _stream())
    return dx


def adam_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step_dev, grad_scale=1.0):
    """step_dev: int32 device tensor (2,) = {number of steps taken so far (incremented by the call), 0}."""
    n = param.numel()
    for t, nme in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _chk(t, F32, (n,), nme)
    _chk(step_dev, I32, (2,), "step_dev")
    _call("sn2_adam_step", _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), n, lr, beta1, beta2, eps,
          weight_decay, _ptr(step_dev), grad_scale, _stream())


def adam_step_dev(param, grad, exp_avg, exp_avg_sq, lr_dev, beta1, beta2, eps, weight_decay, step_dev, grad_scale=1.0, terms=None,
                  meter=None):
    """include/strata_hip.h: sn2_adam_step_dev -- adam_step with the learning rate read from the device word `lr_dev` (fp32 (1,))
    when the kernel runs: a launch captured into a hipGraph follows whatever is written there between replays.  terms (fp64, 1 to
    METER_TERMS values written earlier on the stream) are added to meter (fp64 (METER_TERMS + 1,): sums, then steps)."""
    n = param.numel()
    for t, nme in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _chk(t, F32, (n,), nme)
    _chk(step_dev, I32, (2,), "step_dev")
    n_terms = _chk_lr_meter(lr_dev, terms, meter, "adam_step_dev")
    _call("sn2_adam_step_dev", _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), n, _ptr(lr_dev), beta1, beta2, eps,
          weight_decay, _ptr(step_dev), grad_scale, _ptr(terms), n_terms, _ptr(meter) if n_terms else None, _stream())
