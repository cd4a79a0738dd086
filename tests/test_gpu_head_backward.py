"""sn2_head_backward alone (csrc/head.hip: head_bwd_mfma_kernel<BF>, through hip_ops.head_desc / head_backward with 32 gradient
images) against the head in fp64 on the CPU.  tests/_head_ref.py builds the cases and the reference; tests/test_head_ref_host.py
proves on the CPU what this file rests on (the reference against central differences, the ReLU masks, the edge inputs, e32).

Shapes: R = 1; 63, 64, 65 (a tile short by one, one tile, one row into a second); 255, 256, 257 (a workgroup's four waves short by
one row, full, a second workgroup of one row); 805 (a ragged end); and 2 x CUs x 256 + 65 (131 137 on 256 CUs), the smallest
shape at which a wave takes a second turn: the prefetch `request(r0 + stride)`, accumulators carried across turns, a second turn
that is a partial tile, and waves with none.  Every small R with fp32 and bfloat16 rows x with / without dropout words at p = 0.5
x dcov only, dproba only, both; the large R with dropout and both gradients, fp32 and bfloat16 rows.

What is looked at: dy, and dW1, db1, dW2, db2 folded over the 32 images in fp64 on the host and once more through
hip_ops.grad_reduce.  Exact: 64 sentinel rows behind dy; dy[:, 34:36] == 0; the dead channel's row of dW1, its db1 and its column
of dW2, and the zero column of dy; with neither gradient the arena and dy stay zero; with p = 1 (drop_scale 0) dy, dW1, db1, dW2 are
zero and db2 is the reference's; the rows' padding filled with 777.25 and with NaN gives the bits of zero padding in every
output; a second call into the same arena doubles the folded gradients and leaves dy's bits.

Tolerances (the project's: ATOM, FACTOR, BOUND of tests/test_gpu_fp_blocks.py; every figure is printed next to its bound):
  * gradients, fp32 rows: distance from fp64 relative to the tensor's largest element at most max(1e-5, 8 e32), never above 1e-3;
    e32 is the same distance of the reference restated in fp32 on the CPU;
  * bfloat16 rows: the weight gradients by the same rule against the reference from the rows as stored; dy per element within one
    bfloat16 step (the spacing at the fp64 value) plus that rule's bound times the tensor's largest element.
Every live pre-activation keeps 2^-15 from zero (tests/_head_ref.py: _separate), so the kernel's ReLU mask is the reference's.

Measured on an MI355X ("Head backward and consumer-side BatchNorm sums alone"; 108 tests in under 3 s, the
slowest 0.4 s: the 131 137-row case with its fp64 reference), distance from fp64 relative to the largest element [e32]:
                 small R, fp32 rows                 small R, bfloat16 rows             131 137 rows, fp32 / bfloat16
  dW1            4.4e-8 ... 7.3e-5 [7.8e-8 ... 7.3e-5]   1.0e-7 ... 1.1e-5 [8.2e-8 ... 1.1e-5]   1.9e-7 / 2.0e-7 [6.0e-7 / 4.3e-7]
  db1            4.7e-8 ... 2.8e-7 [4.7e-8 ... 3.0e-7]   7.4e-8 ... 4.6e-7 [6.3e-8 ... 2.8e-7]   1.4e-7 / 1.5e-7 [1.4e-7 / 2.7e-7]
  dW2            5.2e-8 ... 1.0e-4 [4.8e-8 ... 1.0e-4]   3.3e-8 ... 3.6e-5 [8.2e-8 ... 3.6e-5]   2.3e-7 / 2.0e-7 [2.9e-7 / 3.2e-7]
  db2            3.6e-8 ... 3.0e-7 [3.6e-8 ... 5.7e-7]   3.0e-8 ... 2.8e-7 [3.3e-8 ... 3.4e-7]   1.6e-7 / 1.7e-7 [2.6e-7 / 2.1e-7]
  dy             7.9e-8 ... 7.7e-7 [5.6e-8 ... 3.3e-7]   0 ... 7.3e-8 beyond one bfloat16 step   1.9e-7 / 2.2e-8 beyond one step
  The figures above 1e-5 (R = 64, 255, 257) are the kernel's and the fp32 restatement's ALIKE, to two digits (7.29e-5 against
  e32 7.29e-5): on a scaled row the sigmoid saturates, 1 - sigmoid is one fp32 rounding step where fp64 has e^-30, and the
  row's |y| of a few hundred carries that into dW1 and dW2; the bound follows e32 there.  The largest error is 77 % of its bound
  (dW1, R = 65, fp32 rows, no dropout, dproba only: 7.8e-6 of 1.01e-5, e32 1.3e-6); everything at 131 137 rows is at 2 % of
  it.  No change to
  head_bwd_mfma_kernel was needed.
Two deliberately wrong kernels, built once and not kept (neither indexes outside its buffers): without the ninth lin1 step (k = 32 +
kq: columns 32, 33) 102 of these 108 tests fail (dW1 7e-2 ... 2.4e2, dW2 0.17 ... 3.6e2 of the largest element) -- and so do 59
existing whole-network tests (test_gpu_network.py, test_gpu_train_modes.py, ...): that step was covered; with
`request(r0 + stride)` loading the current turn again only `test_a_second_turn_per_wave_matches_float64` fails here (dW1 3.3e-2, dW2
2.9e-2, both row types), beside three existing tests at the workload's own sizes (test_more_than_one_turn_per_wave, whose two sides
differ in which buffer the repeated turn reads, and test_metric_size_forward_loss_backward_vs_oracle[ref / 3sa]).
"""
import functools

import numpy as np
import pytest
import torch

import _head_ref as H
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATOM, BOUND, FACTOR = 1e-5, 1e-3, 8
GUARD = 64
DY_SENT = -768.0                              # (exact in bfloat16)
GRADS = {"both": (True, True), "dcov": (True, False), "dproba": (False, True)}
NAMES = [n for n, _ in H.GRAD_SHAPES]


@functools.lru_cache(maxsize=None)
def _large_rows():
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count * 256 + 65


def _split(flat):
    out, o = {}, 0
    for n, shape in H.GRAD_SHAPES:
        k = int(np.prod(shape))
        out[n] = flat[o:o + k].reshape(shape)
        o += k
    return out


def _run(R, rows, drop, dcov, dproba, drop_p=H.DROP_P, pad=None, calls=1):
    """`calls` x sn2_head_backward of case R into one zeroed arena and a dy pre-filled with DY_SENT (GUARD rows behind it) ->
    dy_full (R + GUARD, 36) fp32 on the CPU, images (32, N_FLAT) fp32, fold = the images summed in fp64 on the host,
    reduced = image 0 after hip_ops.grad_reduce, each split into the four gradients"""
    c = H.make_case(R)
    dt = H.ROWS[rows]
    f = c.f.clone()
    if pad is not None:
        f[:, H.C:] = pad
    f = f.to(DEV).to(dt)
    lin1, lin2 = torch.nn.Linear(H.C, H.HID).to(DEV), torch.nn.Linear(H.HID, H.OUT).to(DEV)
    with torch.no_grad():
        lin1.weight.copy_(c.W1), lin1.bias.copy_(c.b1), lin2.weight.copy_(c.W2), lin2.bias.copy_(c.b2)
    arena, flat, images, _ = ops.grad_images_alloc(H.N_FLAT, DEV)
    views, o = [], 0
    for _, shape in H.GRAD_SHAPES:
        k = int(np.prod(shape))
        views.append(flat[o:o + k].view(shape))
        o += k
    dy_full = torch.full((R + GUARD, H.STRIDE), DY_SENT, dtype=dt, device=DEV)
    # (the descriptor holds addresses only: every buffer stays referenced here until the last call has been read back)
    fa, fc, keep = c.fa.to(DEV), c.fc.to(DEV), c.keep.to(DEV) if drop else None
    gc, gp = c.dcov.to(DEV) if dcov else None, c.dproba.to(DEV) if dproba else None
    hd = ops.head_desc(f, fa, fc, lin1, lin2, dcov=gc, dproba=gp, dy=dy_full[:R], grads=views, grad_images=images, drop_mask=keep,
                       drop_p=drop_p if drop else 0.0)
    assert hd.grad_replicas == 32
    dys = []
    for _ in range(calls):
        ops.head_backward(hd)
        torch.cuda.synchronize()
        dys.append(dy_full.float().cpu().numpy())
    img = arena[:images[0] * images[1]].view(images[0], images[1])[:, :H.N_FLAT].cpu().numpy().copy()
    ops.grad_reduce(arena, H.N_FLAT, images)
    torch.cuda.synchronize()
    out = {"dy_full": dys[-1], "dys": dys, "images": img, "fold": _split(img.astype(np.float64).sum(0)),
           "reduced": _split(flat.cpu().numpy().copy())}
    del fa, fc, keep, gc, gp
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _bf16_step(x):
    """the spacing of bfloat16 at |x| (8 significant bits; the smallest normal's below it)"""
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126)))
    return 2.0 ** (e - 7)


def _check(got, R, rows, ref, r32, tag, factor=1.0):
    """Exact properties first, then every figure is printed, then all are asserted.  factor: the reference's multiple (2 after a
    second call into the same arena)."""
    dy_full = got["dy_full"]
    assert np.array_equal(dy_full[R:], np.full((GUARD, H.STRIDE), DY_SENT, np.float32)), "rows behind dy were written"
    dy = dy_full[:R]
    assert np.isfinite(dy).all() and all(np.isfinite(got["fold"][n]).all() for n in NAMES)
    assert not dy[:, H.C:].any(), "dy's padding columns are not exactly 0"
    assert not dy[:, H.ZERO_COL].any(), "the zero column's dy is not exactly 0"
    for src in ("fold", "reduced"):
        g = got[src]
        assert not g["dW1"][H.DEAD].any() and g["db1"][H.DEAD] == 0 and not g["dW2"][:, H.DEAD].any(), f"{src}: the dead channel has a gradient"
    bad = []
    for n in NAMES:
        scale = np.abs(ref[n]).max()
        assert scale > 0, n
        e32 = H.rel(r32[n], ref[n])
        bound = min(max(ATOM, FACTOR * e32), BOUND)
        for src in ("fold", "reduced"):
            err = float(np.abs(got[src][n] / factor - ref[n]).max()) / scale
            print(f"{tag} {n} ({src}): vs fp64 {err:.2e}, bound {bound:.2e} (e32 {e32:.2e})")
            if not err <= bound:
                bad.append((n, src, err, bound))
    scale = np.abs(ref["dy"]).max()
    e32 = H.rel(r32["dy"], ref["dy"])
    bound = min(max(ATOM, FACTOR * e32), BOUND)
    diff = np.abs(dy[:, :H.C].astype(np.float64) - ref["dy"])
    if rows == "bf16":
        over = float((diff - _bf16_step(ref["dy"])).max()) / scale
        print(f"{tag} dy: beyond one bfloat16 step of fp64 {max(over, 0.0):.2e}, bound {bound:.2e} (e32 {e32:.2e}); plain {diff.max() / scale:.2e}")
        if not over <= bound:
            bad.append(("dy", over, bound))
    else:
        err = float(diff.max()) / scale
        print(f"{tag} dy: vs fp64 {err:.2e}, bound {bound:.2e} (e32 {e32:.2e})")
        if not err <= bound:
            bad.append(("dy", err, bound))
    assert not bad, bad


@pytest.mark.parametrize("grads", list(GRADS))
@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("rows", list(H.ROWS))
@pytest.mark.parametrize("R", H.SMALL_ROWS)
def test_small_shapes_match_float64(R, rows, drop, grads):
    dcov, dproba = GRADS[grads]
    got = _run(R, rows, drop, dcov, dproba)
    _check(got, R, rows, H.reference(R, rows, drop, dcov, dproba), H.reference_fp32(R, rows, drop, dcov, dproba),
           f"R {R} {rows} {'drop' if drop else 'nodrop'} {grads}")


@pytest.mark.parametrize("rows", list(H.ROWS))
def test_a_second_turn_per_wave_matches_float64(rows):
    """2 x CUs x 256 + 65 rows: the grid is capped at 2 x CUs workgroups, so wave 0 of workgroup 0 takes a second turn of 64 rows
    and wave 1 one of a single row, behind the prefetch issued in the middle of their first turn; every other wave has none."""
    R = _large_rows()
    got = _run(R, rows, True, True, True)
    _check(got, R, rows, H.reference(R, rows, True), H.reference_fp32(R, rows, True), f"R {R} {rows} drop both")


@pytest.mark.parametrize("rows", list(H.ROWS))
@pytest.mark.parametrize("R", (65, 805))
def test_no_incoming_gradient_leaves_everything_zero(R, rows):
    got = _run(R, rows, True, False, False)
    assert not got["images"].any(), "the gradient arena moved"
    assert not got["dy_full"][:R].any(), "dy is not zero"
    assert np.array_equal(got["dy_full"][R:], np.full((GUARD, H.STRIDE), DY_SENT, np.float32))


@pytest.mark.parametrize("rows", list(H.ROWS))
@pytest.mark.parametrize("R", (65, 805))
def test_dropout_of_everything(R, rows):
    """p = 1: drop_scale 0.  Nothing reaches lin1 or the rows; the scores are lin2's bias, and db2 is the reference's."""
    got = _run(R, rows, True, True, True, drop_p=1.0)
    ref, r32 = H.reference(R, rows, True, True, True, 1.0), H.reference_fp32(R, rows, True, True, True, 1.0)
    assert not ref["dW1"].any() and not ref["dW2"].any() and not ref["dy"].any()
    assert not got["dy_full"][:R].any()
    for src in ("fold", "reduced"):
        assert not got[src]["dW1"].any() and not got[src]["db1"].any() and not got[src]["dW2"].any(), src
        e32 = H.rel(r32["db2"], ref["db2"])
        err, bound = H.rel(got[src]["db2"], ref["db2"]), min(max(ATOM, FACTOR * e32), BOUND)
        print(f"R {R} {rows} p = 1 db2 ({src}): vs fp64 {err:.2e}, bound {bound:.2e} (e32 {e32:.2e})")
        assert err <= bound


@pytest.mark.parametrize("rows", list(H.ROWS))
@pytest.mark.parametrize("R", (65, 805))
def test_the_rows_padding_is_never_used(R, rows):
    """Columns 34, 35 of f filled with 0, with 777.25 and with NaN: the same bits in dy and in all 32 images (at these shapes an
    image receives one add per call, so the sums do not depend on an order)."""
    base = _run(R, rows, True, True, True, pad=0.0)
    assert np.abs(base["dy_full"][:R]).max() > 0
    for pad in (H.PAD, float("nan")):
        got = _run(R, rows, True, True, True, pad=pad)
        assert np.array_equal(_bits(got["dy_full"]), _bits(base["dy_full"])), f"padding {pad}: dy differs"
        assert np.array_equal(_bits(got["images"]), _bits(base["images"])), f"padding {pad}: the weight gradients differ"


@pytest.mark.parametrize("rows", list(H.ROWS))
@pytest.mark.parametrize("R", (257, 805))
def test_a_second_call_accumulates_the_gradients_and_overwrites_dy(R, rows):
    got = _run(R, rows, True, True, True, calls=2)
    assert np.array_equal(_bits(got["dys"][1]), _bits(got["dys"][0])), "dy was accumulated, not overwritten"
    _check(got, R, rows, H.reference(R, rows, True), H.reference_fp32(R, rows, True), f"R {R} {rows} drop both, two calls", factor=2.0)
