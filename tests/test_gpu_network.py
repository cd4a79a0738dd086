"""GPU parity of the full path through the drop-in Python API (which calls the C ABI): goldens produced by the
reference glue, the oracle at other sizes, projections, backward.  Tolerances: 1e-4 absolute on probabilities /
coverages / rasters (BASELINE.json north_star), pixel indices and NaN masks bit-exact; gradients 1e-3 of the
tensor's max magnitude."""
import numpy as np
import pytest
import torch

from conftest import GOLDEN_CASES, golden_args, golden_state_dict, load_golden
from oracle import check, losses, network, projection
from stratanet2_vegetation_coverage_maps_amd import (PointNet2, project_to_2d_rasters, project_to_plotwise_coverages)
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops
from stratanet2_vegetation_coverage_maps_amd.synthetic import make_args, make_batch

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _model(args, sd):
    args.cuda = 0
    m = PointNet2(args)
    m.load_state_dict(sd)
    return m


def _data(g):
    return {"cloud": torch.from_numpy(g["in/cloud"]), "xyz": torch.from_numpy(g["in/xyz"]),
            "fps_start": torch.from_numpy(g["in/fps_start"])}


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_eval_forward_and_projections_vs_reference_golden(name):
    g, args = load_golden(name), golden_args(name)
    m = _model(args, golden_state_dict(g)).eval()
    data = _data(g)
    with torch.no_grad():
        cov, proba = m(data)
        pred = project_to_plotwise_coverages(cov, data["cloud"], args, model=m)
    np.testing.assert_allclose(cov.cpu().numpy(), g["eval/coverages_pointwise"], atol=TOL, rtol=0)
    np.testing.assert_allclose(proba.cpu().numpy(), g["eval/proba_pointwise"], atol=TOL, rtol=0)
    np.testing.assert_allclose(pred.cpu().numpy(), g["eval/pred_coverages"], atol=TOL, rtol=0)
    cov_b = m.get_batch_format(cov)
    for b in range(cov_b.shape[0]):
        r = project_to_2d_rasters(data["cloud"][b], cov_b[b], args)
        ref = g["eval/rasters"][b]
        assert r.dtype == np.float64 and r.shape == ref.shape
        assert np.array_equal(np.isnan(r), np.isnan(ref))
        np.testing.assert_allclose(np.nan_to_num(r), np.nan_to_num(ref), atol=TOL, rtol=0)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_train_step_vs_reference_golden(name):
    g, args = load_golden(name), golden_args(name)
    m = _model(args, golden_state_dict(g)).train()
    data = _data(g)
    cov, proba = m(data)
    pred = project_to_plotwise_coverages(cov, data["cloud"], args, model=m)
    gt = torch.from_numpy(g["in/coverages"]).cuda()
    pdf = torch.from_numpy(g["in/pdf_all"]).cuda()
    loss, parts = losses.total_loss(pred, proba, gt, pdf, args.m, args.e)   # the loss block is harness code (torch ops)
    loss.backward()
    np.testing.assert_allclose(cov.detach().cpu().numpy(), g["train/coverages_pointwise"], atol=TOL, rtol=0)
    np.testing.assert_allclose(proba.detach().cpu().numpy(), g["train/proba_pointwise"], atol=TOL, rtol=0)
    np.testing.assert_allclose(pred.detach().cpu().numpy(), g["train/pred_coverages"], atol=TOL, rtol=0)
    np.testing.assert_allclose([loss.item()] + [p.item() for p in parts], g["train/losses"], atol=TOL, rtol=0)
    # gradients: against the reference run with fp64 features/weights (same fp32 geometry and pixel ids) = the yardstick:
    # a flat 1e-3 of each tensor's magnitude.  (The reference's OWN fp32 run is further from it than that on the N = 4096
    # cases -- `self_err`, printed: rarely active ReLU channels get BatchNorm outputs of ~100 sigma and torch's fp32 CPU
    # batch statistics are good to ~1e-5 relative; the HIP statistics are finalised in fp64.)  Only the single-plot case
    # c1_ref_defaults (256-row BatchNorms; a 1e-8 relative weight perturbation moves its fp64 gradients by 3e-3,
    # scripts/cond_probe.py) gets max(1e-3, self_err).  Every measured error is printed.
    report, worst = [], 0.0
    for k, p in m.named_parameters():
        ref32, ref64 = g[f"grad/{k}"], g[f"grad64/{k}"]
        assert p.grad is not None, k
        scale = np.abs(ref64).max()
        self_err = np.abs(ref32 - ref64).max() / scale
        tol = max(1e-3, 1.0 * self_err) if name == "c1_ref_defaults" else 1e-3
        err = np.abs(p.grad.cpu().numpy() - ref64).max() / scale
        report.append(f"{k:42s} err {err:.2e}  tol {tol:.2e}  reference fp32-vs-fp64 {self_err:.2e}{'  <-- FAIL' if err > tol else ''}")
        worst = max(worst, err / tol)
    print(f"\n[{name}] parameter gradients vs the reference's fp64 run (relative to max |grad|):\n  " + "\n  ".join(report))
    assert worst <= 1.0, "\n".join(report)
    sd = m.state_dict()
    for k in sd:
        if "running_" in k:
            np.testing.assert_allclose(sd[k].cpu().numpy(), g[f"sd_after/{k}"], atol=1e-5, rtol=1e-4, err_msg=k)
        if "num_batches" in k:
            assert int(sd[k]) == int(g[f"sd_after/{k}"])


def test_pixel_indices_bit_exact_and_p2_gradient():
    """P1 / P2 pixel ids against the oracle's fp32 index arithmetic, and P2's backward against autograd of the oracle,
    on values with many exact ties (quantised) so the first-point-wins rule is exercised."""
    B, N = 3, 5000
    args = make_args(subsample_size=N)
    d = make_batch(B, N, first_plot=40)
    g = torch.Generator().manual_seed(5)
    pw = (torch.rand(B * N, 4, generator=g) * 8).floor() / 8
    clouds_dev = d["cloud"].cuda()
    pw_dev = pw.cuda().requires_grad_(True)
    pred = project_to_plotwise_coverages(pw_dev, clouds_dev, args)
    pix2 = projection.p2_pixel_ids(d["cloud"], args.diam_pix)
    ref_cell = (pix2[:, 0] * args.diam_pix + pix2[:, 1]).reshape(-1)
    _, pix, _, _ = ops.plot_project_forward(pw.cuda(), clouds_dev, args.diam_pix)
    assert torch.equal(pix.cpu(), ref_cell.int())
    pw_ref = pw.clone().requires_grad_(True)
    pred_ref = projection.project_to_plotwise_coverages(pw_ref, d["cloud"], args)
    np.testing.assert_allclose(pred.detach().cpu().numpy(), pred_ref.detach().numpy(), atol=1e-6, rtol=0)
    wgt = torch.rand(B, 4, generator=g)
    (pred * wgt.cuda()).sum().backward()
    (pred_ref * wgt).sum().backward()
    np.testing.assert_allclose(pw_dev.grad.cpu().numpy(), pw_ref.grad.numpy(), atol=1e-7, rtol=1e-5)
    # P1 (fixed grid, clipped)
    rasters, pix1 = ops.raster_project(pw.cuda(), clouds_dev, args.diam_pix, args.diam_meters)
    for b in range(B):
        p = projection.p1_pixel_ids(d["cloud"][b], args.diam_pix, args.diam_meters)
        assert torch.equal(pix1.cpu().view(B, N)[b], (p[1] * args.diam_pix + p[0]).int())
        ref = projection.project_to_2d_rasters(d["cloud"][b], pw.view(B, N, 4)[b].t(), args)
        got = rasters[b].double().cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        assert np.array_equal(np.nan_to_num(got), np.nan_to_num(ref))     # maxima of identical fp32 values: exact


def test_projection_from_precomputed_pixel_ids_is_the_same_projection():
    """sn2_plot_pixels + sn2_plot_project_forward_pix (the ids computed ahead, per-slice key tables, no atomics across
    workgroups) == sn2_plot_project_forward, bit for bit: pixel ids, arg-max points, occupied-pixel counts, plot-wise
    coverages and the gradient -- on quantised values (many exact ties: first point wins) and several plot sizes."""
    for B, N in ((3, 5000), (2, 32768), (5, 700)):
        args = make_args(subsample_size=N)
        d = make_batch(B, N, first_plot=40)
        g = torch.Generator().manual_seed(5)
        pw = ((torch.rand(B * N, 4, generator=g) * 8).floor() / 8).cuda()
        clouds_dev = d["cloud"].cuda()
        pred0, pix0, arg0, nocc0 = ops.plot_project_forward(pw, clouds_dev, args.diam_pix)
        mm, pix = ops.plot_pixels(clouds_dev, args.diam_pix)
        pred1, pix1, arg1, nocc1 = ops.plot_project_forward_pix(pw, pix, B, N, args.diam_pix)
        assert torch.equal(pix, pix0) and torch.equal(arg1, arg0) and torch.equal(nocc1, nocc0) and torch.equal(pred1, pred0)
        ref = projection.p2_pixel_ids(d["cloud"], args.diam_pix)
        assert torch.equal(pix.cpu(), (ref[:, 0] * args.diam_pix + ref[:, 1]).reshape(-1).int())
        # through the autograd node, with a geometry handle that carries the ids
        from types import SimpleNamespace
        geo = SimpleNamespace(p2_pix=pix, p2_diam_pix=args.diam_pix)
        a = pw.clone().requires_grad_(True)
        b = pw.clone().requires_grad_(True)
        wgt = torch.rand(B, 4, generator=g).cuda()
        (project_to_plotwise_coverages(a, clouds_dev, args, geometry=geo) * wgt).sum().backward()
        (project_to_plotwise_coverages(b, clouds_dev, args) * wgt).sum().backward()
        assert torch.equal(a.grad, b.grad)
        geo_other = SimpleNamespace(p2_pix=pix, p2_diam_pix=args.diam_pix + 1)        # ids of another grid: ignored
        assert torch.equal(project_to_plotwise_coverages(pw, clouds_dev, args, geometry=geo_other), pred0)


@pytest.mark.parametrize("B,N,ratio1,r1,r2", [(2, 3000, 0.1, 1.0, 2.0), (1, 8192, 0.125, 1.0, 2.0),
                                               (1, 10000, 0.25, 2 ** 0.5, 8 ** 0.5)])
def test_forward_backward_vs_oracle_other_sizes(B, N, ratio1, r1, r2):
    """Sizes outside the goldens (N not a multiple of 64, C2-style radii, the reference defaults at N = 10000 where
    level 2 also takes the bucketed FPS + cell-list ball query): oracle restatement as the checker."""
    args = make_args(subsample_size=N, ratio1=ratio1, r1=r1, ratio2=0.25, r2=r2)
    d = make_batch(B, N, first_plot=200)
    sd = network.init_state_dict(3)
    fs = torch.stack([torch.arange(B) * 7 % N, torch.arange(B) * 3 % 50])
    d["fps_start"] = fs
    m = _model(args, sd).train()
    cov, proba = m(d)
    pred = project_to_plotwise_coverages(cov, d["cloud"], args, model=m)
    loss, _ = losses.total_loss(pred, proba, d["coverages"].cuda(), d["pdf_all"].cuda(), args.m, args.e)
    loss.backward()
    ref = check.train_step(sd, d, args, fps_start=fs)                  # the oracle in fp64: see oracle/check.py
    fails, report = check.compare(m, cov, proba, loss.item(), ref, pred=pred)
    print(f"\n[{B} x {N}] vs the fp64 oracle:\n  {report}")
    assert not fails, "\n".join(fails)


def test_eval_is_batch_independent_and_deterministic():
    """Plots never interact in eval mode: a plot's outputs do not depend on its batch neighbours; two runs agree
    bit for bit (no atomics on the eval path's values)."""
    N = 2048
    args = make_args(subsample_size=N, ratio1=0.125, r1=1.0, ratio2=0.25, r2=2.0)
    d = make_batch(3, N, first_plot=77)
    fs = torch.zeros(2, 3, dtype=torch.long)
    m = _model(args, network.init_state_dict(1)).eval()
    with torch.no_grad():
        cov_all, _ = m({"cloud": d["cloud"], "xyz": d["xyz"], "fps_start": fs})
        cov_again, _ = m({"cloud": d["cloud"], "xyz": d["xyz"], "fps_start": fs})
        cov_1, _ = m({"cloud": d["cloud"][1:2], "xyz": d["xyz"][1:2], "fps_start": fs[:, :1]})
    assert torch.equal(cov_all, cov_again)
    assert torch.equal(cov_all.view(3, N, 4)[1], cov_1.view(N, 4))


def test_flat_adam_matches_torch_adam():
    """FlatAdam (one HIP kernel over the flat parameter buffer, device-side step counter) against torch.optim.Adam with
    the reference's settings (learning/train.py:180-185: lr, weight_decay as L2), identical gradients, three steps."""
    from stratanet2_vegetation_coverage_maps_amd.optim import FlatAdam, flatten_parameters
    args = make_args(cuda=0, subsample_size=1024)
    torch.manual_seed(0)
    m1, m2 = PointNet2(args), PointNet2(args)
    m2.load_state_dict(m1.state_dict())
    flat = flatten_parameters(m1)
    o1 = FlatAdam(m1, lr=1e-3, weight_decay=1e-3)
    o2 = torch.optim.Adam(m2.parameters(), lr=1e-3, weight_decay=1e-3)
    gen = torch.Generator().manual_seed(3)
    for _ in range(3):
        g = (torch.randn(flat.numel(), generator=gen) * 10 ** torch.randint(-6, 1, (flat.numel(),), generator=gen).float()).cuda()
        m1._last_flat_grad = g.clone()
        o1.step()
        offs, _ = ops.flat_layout(list(m2.parameters()))
        for p, o in zip(m2.parameters(), offs):
            p.grad = g[o:o + p.numel()].view(p.shape).clone()
        o2.step()
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        if a.is_floating_point():
            np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), atol=1e-6, rtol=1e-5, err_msg=k)


def test_losses_match_oracle():
    """Fused loss kernels (product, hipGraph-capturable) vs the oracle's restatement of learning/loss_functions.py and vs
    the plain torch-op form on the device: values 1e-6, gradients 1e-6 relative to the largest entry."""
    from stratanet2_vegetation_coverage_maps_amd import losses as dev_losses
    g = torch.Generator().manual_seed(0)
    for B, R in ((6, 3000), (16, 70001)):
        pred = torch.rand(B, 4, generator=g)
        proba = torch.softmax(torch.randn(R, 4, generator=g), 1) * torch.rand(R, 1, generator=g)
        gt = torch.rand(B, 4, generator=g, dtype=torch.float64)
        pdf = torch.rand(R, 3, generator=g, dtype=torch.float64) + 0.05
        pd, qd = pred.cuda().requires_grad_(True), proba.cuda().requires_grad_(True)
        a, pa = dev_losses.total_loss(pd, qd, gt.cuda(), pdf.cuda(), 0.1, 0.04)
        (3.0 * a).backward()                                        # a non-unit upstream gradient
        pt, qt = pred.cuda().requires_grad_(True), proba.cuda().requires_grad_(True)
        t, _ = dev_losses.total_loss_torch(pt, qt, gt.cuda(), pdf.cuda(), 0.1, 0.04)
        (3.0 * t).backward()
        pr, qr = pred.clone().requires_grad_(True), proba.clone().requires_grad_(True)
        b, pb = losses.total_loss(pr, qr, gt, pdf, 0.1, 0.04)
        (3.0 * b).backward()
        assert abs(a.item() - b.item()) < 1e-6 and abs(a.item() - t.item()) < 1e-6
        for x, y in zip(pa, pb):
            assert abs(x.item() - y.item()) < 1e-6
        for got, ref in ((pd.grad, pr.grad), (qd.grad, qr.grad), (pd.grad, pt.grad.cpu()), (qd.grad, qt.grad.cpu())):
            ref = ref.cpu().numpy()
            np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-5, atol=1e-6 * np.abs(ref).max())


def test_the_three_loss_terms_one_by_one_are_the_fused_node():
    """The reference's loop calls `get_absolute_loss`, `get_NLL_loss`, `get_entropy_loss` one by one (learning/train.py:58-62): on
    a HIP device each is the fused node with the other two terms switched off.  Values against the plain torch forms (1e-6)
    and the oracle's, gradients of their weighted sum 1e-5; CPU tensors take the torch forms."""
    from stratanet2_vegetation_coverage_maps_amd import losses as dev_losses
    g = torch.Generator().manual_seed(1)
    B, R = 5, 40001
    pred = torch.rand(B, 4, generator=g)
    proba = torch.softmax(torch.randn(R, 4, generator=g), 1) * torch.rand(R, 1, generator=g)
    gt = torch.rand(B, 4, generator=g, dtype=torch.float64)
    pdf = torch.rand(R, 3, generator=g, dtype=torch.float64) + 0.05
    res = {}
    for fused in (True, False):
        dev_losses.FUSED_TERMS = fused
        try:
            pd, qd = pred.cuda().requires_grad_(True), proba.cuda().requires_grad_(True)
            la = dev_losses.get_absolute_loss(pd, gt.cuda())
            ll = dev_losses.get_NLL_loss(qd, pdf.cuda())
            le = dev_losses.get_entropy_loss(qd)
            (2.0 * (la + 0.1 * ll + 0.04 * le)).backward()
            res[fused] = (la.item(), ll.item(), le.item(), pd.grad.clone(), qd.grad.clone())
        finally:
            dev_losses.FUSED_TERMS = True
    _, (oa, ol, oe) = losses.total_loss(pred, proba, gt, pdf, 0.1, 0.04)
    for k, o in enumerate((oa, ol, oe)):
        assert abs(res[True][k] - res[False][k]) < 1e-6 * max(1.0, abs(res[False][k])) and abs(res[True][k] - o.item()) < 1e-6 * max(1.0, abs(o.item()))
    for k in (3, 4):
        ref = res[False][k].cpu().numpy()
        np.testing.assert_allclose(res[True][k].cpu().numpy(), ref, rtol=1e-5, atol=1e-6 * np.abs(ref).max())
    assert dev_losses.get_absolute_loss(pred, gt).dtype == dev_losses.get_absolute_loss_torch(pred, gt).dtype      # CPU: torch form
    #  a switched-off term is SKIPPED, not multiplied by zero: the entropy of rows that are no probability vectors
    # (the reference's docstring says "coverage raster"; all-zero rows included) is finite, value and gradient, as in torch
    rows = torch.rand(1000, 4, generator=g) * 0.3
    rows[::7] = 0.0
    out = {}
    for fused in (True, False):
        dev_losses.FUSED_TERMS = fused
        try:
            q = rows.cuda().requires_grad_(True)
            le = dev_losses.get_entropy_loss(q)
            le.backward()
            out[fused] = (le.item(), q.grad.clone())
        finally:
            dev_losses.FUSED_TERMS = True
    assert np.isfinite(out[True][0]) and torch.isfinite(out[True][1]).all()
    assert abs(out[True][0] - out[False][0]) < 1e-6 * max(1.0, abs(out[False][0]))
    np.testing.assert_allclose(out[True][1].cpu().numpy(), out[False][1].cpu().numpy(), rtol=1e-5, atol=1e-9)


def test_prefetched_geometry_gives_identical_results():
    """`prefetch_geometry` (position-only kernels on a side stream) + forward == plain forward, bit for bit in eval."""
    N = 4096
    args = make_args(subsample_size=N, ratio1=0.125, r1=1.0, ratio2=0.25, r2=2.0)
    d = make_batch(2, N, first_plot=9)
    d["fps_start"] = torch.tensor([[5, 77], [3, 1]])
    m = _model(args, network.init_state_dict(2)).eval()
    with torch.no_grad():
        cov_a, proba_a = m(d)
        geo = m.prefetch_geometry(d)
        cov_b, proba_b = m({"cloud": d["cloud"], "xyz": d["xyz"], "geometry": geo})
    assert torch.equal(cov_a, cov_b) and torch.equal(proba_a, proba_b)


def test_geometry_prefetched_in_eval_mode_serves_a_training_step():
    """An eval-mode geometry pass skips the inverted 3-NN tables (only the backward gathers through them); a training
    forward over such a handle builds them itself: same gradients as the plain training step."""
    N = 4096
    args = make_args(subsample_size=N, ratio1=0.125, r1=1.0, ratio2=0.25, r2=2.0)
    d = make_batch(2, N, first_plot=9)
    d["fps_start"] = torch.tensor([[5, 77], [3, 1]])
    grads = []
    for prefetch_in_eval in (False, True):
        m = _model(args, network.init_state_dict(2))
        cd = {"cloud": d["cloud"], "xyz": d["xyz"], "fps_start": d["fps_start"]}
        if prefetch_in_eval:
            m.eval()
            geo = m.prefetch_geometry(d)
            assert geo.has_inverted is False
            cd["geometry"] = geo
        m.train()
        cov, proba = m(cd)
        (cov.sum() + (proba * proba).sum()).backward()
        torch.cuda.synchronize()
        grads.append(torch.cat([p.grad.reshape(-1) for p in m.parameters()]).cpu().numpy())
    scale = np.abs(grads[0]).max()
    np.testing.assert_allclose(grads[1], grads[0], rtol=0, atol=1e-5 * scale)     # float atomics in the weight gradients


def test_kde_lookup_matches_scipy_interp1d():
    """Device lookup of the KDE-mixture densities vs the reference's way (scipy interp1d on the CPU): fp64, same operation
    order -> equal to the last bit on equidistant knots (FFTKDE's grid) and on irregular, unsorted ones."""
    from stratanet2_vegetation_coverage_maps_amd import losses as dev_losses
    rng = np.random.default_rng(3)
    d = make_batch(3, 5000, first_plot=11)
    z_max = 24.24
    for irregular in (False, True):
        K = 5000
        X = np.linspace(-30.0, 30.0, K)
        if irregular:
            X = np.sort(X + rng.uniform(-0.004, 0.004, K))
            perm = rng.permutation(K)
        ys = [np.exp(-0.5 * ((np.abs(X) - c) / s) ** 2) + 0.01 for c, s in ((0.2, 0.3), (1.0, 0.5), (8.0, 5.0))]
        Xin, yin = (X[perm], [y[perm] for y in ys]) if irregular else (X, ys)
        want = losses.kde_predict(Xin, yin, d["cloud"], z_max)
        tab = dev_losses.KdeTables(Xin, *yin, device="cuda:0")
        got = dev_losses.kde_densities(d["cloud"].cuda(), z_max, tab).cpu().numpy()
        assert got.shape == want.shape == (3 * 5000, 3)
        np.testing.assert_array_equal(got, want)
    # out of the table's range: scipy raises, the device marks the point
    tab = dev_losses.KdeTables(np.linspace(0.0, 1.0, 10), *[np.ones(10)] * 3, device="cuda:0")
    out = dev_losses.kde_densities(d["cloud"].cuda(), z_max, tab)
    assert torch.isnan(out).any() and not torch.isnan(out).all()


def test_dense_plot_128k_points_vs_oracle():
    """BASELINE config 5's plot size through the whole network (fp32; the bf16 variant of this size: tests/test_gpu_bf16.py): one 131 072-point
    plot, forward + loss + backward against the oracle (kd-tree candidate search, canonical fp32 tests)."""
    N = 131072
    args = make_args(subsample_size=N, ratio1=1024 / N, r1=1.0, ratio2=0.25, r2=2.0)
    d = make_batch(1, N, first_plot=77)
    sd = network.init_state_dict(1)
    fs = torch.tensor([[123], [7]])
    d["fps_start"] = fs
    m = _model(args, sd).train()
    cov, proba = m(d)
    pred = project_to_plotwise_coverages(cov, d["cloud"], args, model=m)
    from stratanet2_vegetation_coverage_maps_amd import losses as dev_losses
    loss, _ = dev_losses.total_loss(pred, proba, d["coverages"].cuda(), d["pdf_all"].cuda(), args.m, args.e)
    loss.backward()
    ref = check.train_step(sd, d, args, fps_start=fs, use_kdtree=True)      # the oracle in fp64 (oracle/check.py)
    fails, report = check.compare(m, cov, proba, loss.item(), ref, pred=pred, tol_grad=2e-3)     # one plot: 256-row BatchNorms
    print(f"\n[1 x {N}] vs the fp64 oracle:\n  {report}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("N", [24001, 24004])
def test_per_point_layer_source_side_form(N):
    """FP1 above 65 536 rows runs in the source-side form (include/strata_hip.h: sn2_fp.src_ws): several plots, a plot
    size that is no multiple of the 7 rows a load instruction covers.  Checked against the oracle and against the
    row-per-lane form of the same library on the same inputs (fp32 re-association only: 2e-5).
    N = 24004 (3 N a multiple of 4: the bucketed FPS fills its workspace): the backward pass also keeps its d pre-activation
    rows in the plots' Morton order (sn2_fp.row_perm, the inverted index built over the permuted rows); N = 24001: it does not."""
    B = 3
    args = make_args(subsample_size=N, ratio1=1024 / N, r1=1.0, ratio2=0.25, r2=2.0)
    d = make_batch(B, N, first_plot=31)
    sd = network.init_state_dict(5)
    fs = torch.stack([torch.arange(B) * 11 % N, torch.arange(B) * 5 % 100])
    d["fps_start"] = fs
    from stratanet2_vegetation_coverage_maps_amd import losses as dev_losses

    def run(source_side):
        ops.SOURCE_SIDE = source_side
        try:
            m = _model(args, sd).train()
            m.fp1_morton_rows = True               # (off by default: slower at the metric's size, point_net2.py)
            cov, proba = m(d)
            assert (getattr(cov.grad_fn.saved, "rank1", None) is not None) == (source_side and N % 4 == 0)
            pred = project_to_plotwise_coverages(cov, d["cloud"], args, model=m)
            loss, _ = dev_losses.total_loss(pred, proba, d["coverages"].cuda(), d["pdf_all"].cuda(), args.m, args.e)
            loss.backward()
            torch.cuda.synchronize()
        finally:
            ops.SOURCE_SIDE = True
        return cov.detach().cpu().numpy(), proba.detach().cpu().numpy(), loss.item(), \
            {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}, \
            {k: v.cpu().numpy() for k, v in m.state_dict().items() if "running" in k}

    cov, proba, loss, grads, running = run(True)
    cov0, proba0, loss0, grads0, running0 = run(False)
    np.testing.assert_allclose(cov, cov0, atol=2e-5, rtol=0)
    np.testing.assert_allclose(proba, proba0, atol=2e-5, rtol=0)
    assert abs(loss - loss0) < 2e-5
    for k in grads:
        np.testing.assert_allclose(grads[k], grads0[k], atol=1e-7 + 2e-4 * np.abs(grads0[k]).max(), rtol=0, err_msg=k)
    for k in running:
        np.testing.assert_allclose(running[k], running0[k], atol=1e-6, rtol=1e-5, err_msg=k)

    ref = check.train_step(sd, d, args, fps_start=fs, use_kdtree=True)      # the oracle in fp64 (oracle/check.py)
    assert np.abs(cov - ref["cov"].numpy()).max() <= TOL and np.abs(proba - ref["proba"].numpy()).max() <= TOL
    assert abs(loss - ref["loss"]) <= TOL
    for k in grads:
        g = ref["grads"][k].numpy()
        err = np.abs(grads[k] - g).max() / np.abs(g).max()
        assert err <= 1e-3, f"{k}: {err:.2e}"


def _fp1_form(B, N, M1, fp_pass):
    """The kernel form (ops.FP_FORM_*) the per-point layer's forward takes at this shape, asked of the library for the
    descriptor the host would hand it (uninitialised buffers: nothing is launched)."""
    dev = torch.device("cuda:0")

    def e(*shape):
        return torch.empty(*shape, device=dev)
    blk = ops.BlockBuffers(torch.nn.Linear(42, 34).to(dev), torch.nn.BatchNorm1d(34).to(dev))
    knn = (torch.empty(B * N, 3, dtype=torch.int32, device=dev), e(B * N, 3))
    return ops.fp_form(ops.fp_desc(blk, B, N, M1, 34, 8, e(B * M1, 36), e(B * N, 36), src_affine=(e(34), e(34)), knn=knn,
                                   skip=e(B * N, 12)[:, 0:8]), fp_pass)


@pytest.mark.parametrize("defect,want", [("row_perm", -2), ("no_scatter_ws", -1), (None, 0)])
def test_fp_backward_refuses_a_descriptor_before_its_first_launch(defect, want):
    """sn2_fp_backward validates first (include/strata_hip.h: SN2_EINVAL / SN2_ELIMIT come back with the device untouched).  The
    64 + 16 -> 34 k-NN block on 2 x 64 rows over 2 x 16 sources (the Split form), every buffer really allocated:
    row_perm -- an identity permutation -- belongs to the source-side form only (SN2_ELIMIT), and dsrc with du_scratch but no
    scatter_ws has nothing to gather through (SN2_EINVAL).  The dispatch once returned both codes after the BatchNorm-sum kernel
    and fp_bwd_split_kernel had run -- the latter adds into dW / db with atomics.  The gradient arena, du_scratch and dsrc must
    hold the same int32 words as before the call; the same descriptor without a defect returns 0 and changes dW."""
    from stratanet2_vegetation_coverage_maps_amd import _lib
    dev = torch.device("cuda:0")
    B, Rp, Sp, ca, cb, co = 2, 64, 16, 64, 16, 34
    g = torch.Generator(device="cpu").manual_seed(11)

    def r(*shape):
        return torch.randn(*shape, generator=g).to(dev)
    knn = ops.three_nn(r(B, 3, Sp), r(B, 3, Rp), 3)
    blk = ops.BlockBuffers(torch.nn.Linear(ca + cb, co).to(dev), torch.nn.BatchNorm1d(co).to(dev))
    n_w = co * (ca + cb)
    arena, flat, images, _ = ops.grad_images_alloc(n_w + 3 * co, dev)
    blk.grads = (flat[:n_w].view(co, ca + cb),) + tuple(flat[n_w + i * co:n_w + (i + 1) * co] for i in range(3))
    blk.grad_images = images
    src, skip, h, dy = r(B * Sp, ca), r(B * Rp, cb), torch.empty(B * Rp, 36, device=dev), r(B * Rp, 36)
    dsrc, du = torch.empty(B * Sp, ca, device=dev), torch.empty(B * Rp, ca, device=dev)
    ops.fp_forward(ops.fp_desc(blk, B, Rp, Sp, ca, cb, src, h, knn=knn, skip=skip), 1)
    before = []
    for t in (arena, du, dsrc):
        t.view(-1).copy_((torch.arange(t.numel(), device=dev) % 251) * 0.25 + 1.0)           # the sentinel pattern
        before.append(t.view(torch.int32).clone())
    d = ops.fp_desc(blk, B, Rp, Sp, ca, cb, src, h, knn=knn, skip=skip, dy=dy, dsrc=dsrc, du_scratch=du, with_grads=True)
    perm = torch.arange(Rp, dtype=torch.int32, device=dev).repeat(B)
    if defect == "row_perm":
        d.row_perm = perm.data_ptr()
    elif defect == "no_scatter_ws":
        d.scatter_ws = None
    assert ops.fp_form(d, 3) == (want if want < 0 else ops.FP_FORM_SPLIT)
    rc = _lib.load().sn2_fp_backward(d, ops._stream())
    torch.cuda.synchronize()
    assert rc == want
    same = [torch.equal(t.view(torch.int32), b) for t, b in zip((arena, du, dsrc), before)]
    if want < 0:
        assert same == [True, True, True], dict(zip(("gradient arena", "du_scratch", "dsrc"), same))
    else:
        dW = sum(arena[i * images[1]:i * images[1] + n_w] - before[0].view(torch.float32)[i * images[1]:i * images[1] + n_w]
                 for i in range(images[0]))
        assert not same[0] and bool(torch.isfinite(dW).all()) and float(dW.abs().max()) > 0


@pytest.mark.parametrize("B,N,M1", [(3, 24001, 1024), (16, 32768, 1024), (72, 1024, 8), (5, 14001, 3500), (20, 10000, 3300)])
def test_the_two_row_passes_of_the_source_side_forward_give_the_same_bits(B, N, M1):
    """fp_fwd_rows2_kernel (round 5: a wave fetches an iteration's indices, weights and skip quads one element per lane, four
    iterations ahead, and hands them to the (row, quad) lanes through LDS; the next iteration's table rows are asked for before
    the current one is computed) against fp_fwd_rows_kernel (every lane of a row loads the row's inputs itself, one iteration
    ahead): same rows per wave, same arithmetic in the same order -- the activations, BatchNorm statistics and running statistics
    must be the same BITS, row counts that are no multiple of the 14 rows of an iteration and plots of a few rows included."""
    from stratanet2_vegetation_coverage_maps_amd import _lib
    dev = torch.device("cuda:0")
    torch.manual_seed(B * N)
    d = make_batch(B, N, first_plot=3)
    xyz = d["xyz"].to(dev).float().contiguous()
    _, pos1_soa, _ = ops.fps(xyz, M1, torch.zeros(B, dtype=torch.int32, device=dev))[:3]
    knn = ops.three_nn(pos1_soa, xyz, 3)
    h2 = torch.randn(B * M1, 36, device=dev)
    a2, c2 = torch.rand(34, device=dev) + 0.5, torch.randn(34, device=dev) * 0.1
    rows0 = torch.randn(B * N, 12, device=dev)
    out = {}
    try:
        # (form of the row pass, form of the source-table kernel: on the matrix cores -- round 5, where there are at least 65 536
        # sources: the last case -- or one row per lane)
        for form, table in ((1, 1), (0, 1), (1, 0)):
            _lib.load().sn2_debug_fp_rows_form(form)
            _lib.load().sn2_debug_fp_table_form(table)
            lin, bn = torch.nn.Linear(42, 34).to(dev), torch.nn.BatchNorm1d(34).to(dev)
            with torch.no_grad():
                g = torch.Generator(device="cpu").manual_seed(5)
                lin.weight.copy_(torch.randn(34, 42, generator=g) * 0.2)
                lin.bias.copy_(torch.randn(34, generator=g) * 0.1)
            blk = ops.BlockBuffers(lin, bn)
            h1 = torch.full((B * N, 36), 7.0, device=dev)
            desc = ops.fp_desc(blk, B, N, M1, 34, 8, h2, h1, src_affine=(a2, c2), knn=knn, skip=rows0[:, 0:8])
            assert ops.fp_form(desc, 1) == ops.FP_FORM_SOURCE_SIDE
            ops.fp_forward(desc, 1)
            torch.cuda.synchronize()
            out[(form, table)] = (h1.clone(), blk.aux.clone(), bn.running_mean.clone(), bn.running_var.clone())
    finally:
        _lib.load().sn2_debug_fp_rows_form(1)
        _lib.load().sn2_debug_fp_table_form(1)
    assert B * N > 64 * _lib.STAT_SLOTS, "the case must take the source-side form"
    assert float(out[(1, 1)][0][:, :34].abs().max()) > 0 and not (out[(1, 1)][0][:, :34] == 7.0).any()
    for other in ((0, 1), (1, 0)):
        for a, b, what in zip(out[(1, 1)], out[other], ("rows", "a | c | mean | invstd", "running_mean", "running_var")):
            assert torch.equal(a, b), (other, what)


def test_source_side_form_with_many_tiny_plots():
    """72 plots of 1024 points with 8 level-1 centroids each: more than 65 536 rows, so the per-point layer takes its
    source-side form, but a plot's chunk table has only 57 slots (< 64 = the slots one wave of fp_bwd_src_chunk_kernel owns):
    a wave's range starts in one plot's padding, covers the next plot's chunks and ends in that plot's padding.  (The
    kernel's "padding only" early return once looked at the first and the last slot only and skipped such waves, and the
    merge then summed partial rows nobody had written.)  The allocator is poisoned with NaN first, so unwritten scratch
    shows.  Checked against the row-per-lane form and against the fp64 oracle."""
    B, N = 72, 1024
    args = make_args(subsample_size=N, ratio1=8 / N, r1=6.0, ratio2=0.5, r2=12.0)
    assert ops.interp_chunks(N, 8) < 64 and B * N > 65536
    assert _fp1_form(B, N, 8, 1) == ops.FP_FORM_SOURCE_SIDE
    d = make_batch(B, N, first_plot=400)
    sd = network.init_state_dict(6)
    fs = torch.stack([torch.arange(B) * 11 % N, torch.arange(B) % 8])
    d["fps_start"] = fs
    from stratanet2_vegetation_coverage_maps_amd import losses as dev_losses

    def run(source_side):
        ops.SOURCE_SIDE = source_side
        try:
            junk = [torch.full((n,), float("nan"), device="cuda") for n in (1 << 16, 1 << 18, 1 << 20, 1 << 22, 1 << 24) for _ in range(4)]
            del junk                                   # the caching allocator hands these blocks to the next torch.empty calls
            m = _model(args, sd).train()
            cov, proba = m(d)
            assert (cov.grad_fn.saved.h1.shape[0] == B * N)
            pred = project_to_plotwise_coverages(cov, d["cloud"], args, model=m)
            loss, _ = dev_losses.total_loss(pred, proba, d["coverages"].cuda(), d["pdf_all"].cuda(), args.m, args.e)
            loss.backward()
            torch.cuda.synchronize()
        finally:
            ops.SOURCE_SIDE = True
        return cov.detach().cpu().numpy(), loss.item(), {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}

    cov, loss, grads = run(True)
    cov0, loss0, grads0 = run(False)
    assert np.isfinite(cov).all() and all(np.isfinite(g).all() for g in grads.values())
    np.testing.assert_allclose(cov, cov0, atol=2e-5, rtol=0)
    for k in grads:
        np.testing.assert_allclose(grads[k], grads0[k], atol=1e-7 + 2e-4 * np.abs(grads0[k]).max(), rtol=0, err_msg=k)
    ref = check.train_step(sd, d, args, fps_start=fs)
    assert np.abs(cov - ref["cov"].numpy()).max() <= TOL and abs(loss - ref["loss"]) <= TOL
    worst = max(np.abs(grads[k] - ref["grads"][k].numpy()).max() / np.abs(ref["grads"][k].numpy()).max() for k in grads)
    print(f"\n[72 x 1024, 8 sources per plot] worst gradient error vs the fp64 oracle {worst:.2e} (tol 2e-3)")
    assert worst <= 2e-3


@pytest.mark.parametrize("B,N", [(3, 24001), (2, 4096), (5, 10000), (14, 10000)])
def test_eval_fused_per_point_layer_and_head(B, N):
    """Eval mode runs FP1 and the head as ONE kernel (sn2_fp_head_eval: the rows of h1 stay in LDS).  Against the two separate
    kernels: the same bits where those take the same (source-side) form of FP1 -- more than 65 536 rows --, and equal to
    rounding (2e-6) below, where the separate path runs FP1 row by row on the matrix cores; the oracle pins both (1e-4).
    N = 24001 and 10000: a last turn of fewer than 63 rows, plots that are no multiple of 7 rows."""
    args = make_args(subsample_size=N, ratio1=0.03, r1=1.0, ratio2=0.25, r2=2.0)
    d = make_batch(B, N, first_plot=11)
    d["fps_start"] = torch.zeros(2, B, dtype=torch.long)
    sd = network.init_state_dict(7)
    m = _model(args, sd).train()
    with torch.no_grad():
        m(d)                                            # running statistics that are not (0, 1)
    m.eval()
    sd_now = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    out = {}
    for fused in (True, False):
        m.fuse_eval_head = fused
        with torch.no_grad():
            cov, proba = m(d)
        torch.cuda.synchronize()
        out[fused] = (cov.clone(), proba.clone())
    m.fuse_eval_head = True
    if B * N >= 63 * 4 * 512:
        # enough turns for the pipelined form of the fused kernel (fp_head_eval2_kernel, round 5: a turn's inputs fetched one
        # element per lane a turn ahead, table rows asked for a batch ahead): the first form on the same inputs, the same bits
        from stratanet2_vegetation_coverage_maps_amd import _lib
        try:
            _lib.load().sn2_debug_fp_rows_form(0)
            with torch.no_grad():
                cov0, proba0 = m(d)
            torch.cuda.synchronize()
        finally:
            _lib.load().sn2_debug_fp_rows_form(1)
        assert torch.equal(cov0, out[True][0]) and torch.equal(proba0, out[True][1])
    if B * N > 65536:
        assert _fp1_form(B, N, ops.fps_num_samples(N, 0.03), 0) == ops.FP_FORM_SOURCE_SIDE
        assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])
    else:
        assert _fp1_form(B, N, ops.fps_num_samples(N, 0.03), 0) == ops.FP_FORM_SPLIT
        assert float((out[True][0] - out[False][0]).abs().max()) < 2e-6 and float((out[True][1] - out[False][1]).abs().max()) < 2e-6
    with torch.no_grad():
        cov_r, proba_r, _ = network.forward(sd_now, d["cloud"], d["xyz"], args, training=False, use_kdtree=True)
    np.testing.assert_allclose(out[True][0].cpu().numpy(), cov_r.numpy(), atol=TOL, rtol=0)
    np.testing.assert_allclose(out[True][1].cpu().numpy(), proba_r.numpy(), atol=TOL, rtol=0)


def test_last_G_tensor_holds_the_plot_embeddings():
    """`args.log_embeddings` (model/point_net2.py:134-135; read by learning/test.py:105-107): after a forward
    `model.last_G_tensor` is the (B,64) output of the global set-abstraction level -- against the oracle's x3."""
    B, N = 3, 4096
    args = make_args(subsample_size=N, ratio1=0.125, r1=1.0, ratio2=0.25, r2=2.0, log_embeddings=True)
    d = make_batch(B, N, first_plot=60)
    d["fps_start"] = torch.zeros(2, B, dtype=torch.long)
    sd = network.init_state_dict(2)
    m = _model(args, sd).eval()
    assert m.last_G_tensor is None
    with torch.no_grad():
        m(d)
        _, _, ex = network.forward(sd, d["cloud"], d["xyz"], args, training=False, details=True)
    assert tuple(m.last_G_tensor.shape) == (B, 64)
    np.testing.assert_allclose(m.last_G_tensor.cpu().numpy(), ex["x3"].numpy(), atol=TOL, rtol=0)
    args2 = make_args(subsample_size=N, ratio1=0.125, r1=1.0, ratio2=0.25, r2=2.0, log_embeddings=False)
    m2 = _model(args2, sd).eval()
    with torch.no_grad():
        m2(d)
    assert m2.last_G_tensor is None                       # only kept when asked for, as in the reference


@pytest.mark.parametrize("B,N", [(2, 4096), (3, 24001)])
def test_training_forward_is_bit_reproducible(B, N):
    """The training-mode forward pass (batch statistics included) gives the same bits on every run, for the small-layer
    kernels and for the per-point layer's source-side form.  It has to: statistics that move by 1e-7 (waves adding their
    sums in arrival order) now and then change the sign of a pre-activation next to zero, and one flipped ReLU mask moved
    weight gradients of the same step by 1-2 % (scripts/debug_grad_images.py)."""
    args = make_args(subsample_size=N, ratio1=min(0.125, 1024 / N), r1=1.0, ratio2=0.25, r2=2.0)
    d = make_batch(B, N, first_plot=40)
    d["fps_start"] = torch.zeros(2, B, dtype=torch.int64)
    m = _model(args, network.init_state_dict(5)).train()
    ref = None
    for _ in range(6):
        cov, proba = m(d)
        got = (cov.detach().clone(), proba.detach().clone())
        if ref is None:
            ref = got
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


@pytest.mark.parametrize("p_drop", [0.3, 0.5])
def test_dropout_in_the_head_vs_oracle_with_the_same_mask(p_drop):
    """F.dropout between lin1 and lin2 (/root/reference/model/point_net2.py:142, args.drop, config.py:76): with the keep-mask
    handed in (`cloud_data["dropout_mask"]`, additive extension) forward, loss and gradients equal the oracle's; eval mode
    ignores it; without a mask the kernel draws Bernoulli(1-p) per element from torch's generator."""
    B, N = 2, 3000
    args = make_args(subsample_size=N, ratio1=0.1, r1=1.0, ratio2=0.25, r2=2.0, drop=p_drop)
    d = make_batch(B, N, first_plot=200)
    sd = network.init_state_dict(3)
    fs = torch.zeros(2, B, dtype=torch.long)
    keep = torch.rand(B * N, 16, generator=torch.Generator().manual_seed(9)) >= p_drop
    d["fps_start"], d["dropout_mask"] = fs, keep
    m = _model(args, sd).train()
    cov, proba = m(d)
    pred = project_to_plotwise_coverages(cov, d["cloud"], args, model=m)
    loss, _ = losses.total_loss(pred, proba, d["coverages"].cuda(), d["pdf_all"].cuda(), args.m, args.e)
    loss.backward()
    ref = check.train_step(sd, d, args, fps_start=fs, dropout_mask=keep)   # the oracle in fp64 with the same mask
    fails, report = check.compare(m, cov, proba, loss.item(), ref, pred=pred)
    print(f"\n[dropout p = {p_drop}] vs the fp64 oracle:\n  {report}")
    assert not fails, "\n".join(fails)
    # the mask matters (the no-dropout outputs differ), eval mode ignores it, and the built-in draw keeps ~(1-p)
    no_drop = _model(make_args(subsample_size=N, ratio1=0.1, r1=1.0, ratio2=0.25, r2=2.0, drop=0.0), sd).train()
    cov0, _ = no_drop({k: v for k, v in d.items() if k != "dropout_mask"})
    assert (cov0 - cov).abs().max() > 1e-3
    m2 = _model(args, sd).eval()
    m3 = _model(make_args(subsample_size=N, ratio1=0.1, r1=1.0, ratio2=0.25, r2=2.0, drop=0.0), sd).eval()
    with torch.no_grad():
        c_eval, _ = m2(d)
        c_eval0, _ = m3({k: v for k, v in d.items() if k != "dropout_mask"})
    assert torch.equal(c_eval, c_eval0)
    words = m.train()._dropout_keep({"cloud": d["cloud"]}, d["cloud"].cuda())
    kept = sum(int(((words >> j) & 1).sum()) for j in range(16)) / (16 * B * N)
    assert abs(kept - (1 - p_drop)) < 0.01
    torch.manual_seed(1)
    a, _ = m(dict(cloud=d["cloud"], xyz=d["xyz"], fps_start=fs))
    torch.manual_seed(1)
    b, _ = m(dict(cloud=d["cloud"], xyz=d["xyz"], fps_start=fs))
    assert torch.equal(a, b) and torch.isfinite(a).all()          # reproducible under torch's seed


def _with_running_statistics(sd, seed):
    """a state dict whose BatchNorms carry running statistics that are NOT the batch's (as after some epochs of training)"""
    g = torch.Generator().manual_seed(seed)
    sd = {k: v.clone() for k, v in sd.items()}
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = 0.2 * torch.randn(sd[k].shape, generator=g)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(sd[k].shape, generator=g)
        elif k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(7)
    return sd


@pytest.mark.parametrize("executor", [True, False])
@pytest.mark.parametrize("B,N,ratio1", [(2, 3000, 0.1), (1, 10000, 0.25), (16, 32768, 1024 / 32768)])
def test_backward_through_an_eval_forward_vs_oracle(B, N, ratio1, executor):
    """`model.eval()` with autograd on -- torch's BatchNorm in eval mode under autograd (model/point_net2.py:45-53; the
    reference's drivers never do it, its autograd allows it; rounds 1-4 refused): the forward runs every BatchNorm on its RUNNING
    statistics and keeps what a training forward keeps (SN2_BN_FROZEN_KEEP), the backward has no batch-mean / batch-variance
    terms (sn2_block.frozen_stats): d pre-BN = gamma * invstd * dy.  Against the oracle's eval-mode step in fp64; the running
    statistics and counters stay as they were; the outputs are those of the no-grad eval path (other kernels: the fused eval
    head, the SA kernels without arg-max slots) to rounding."""
    args = make_args(subsample_size=N, ratio1=ratio1, r1=1.0, ratio2=0.25, r2=2.0)
    d = make_batch(B, N, first_plot=31)
    sd = _with_running_statistics(network.init_state_dict(5), 11)
    fs = torch.stack([torch.arange(B) * 5 % N, torch.arange(B) * 3 % 40])
    d["fps_start"] = fs
    m = _model(args, sd).eval()
    m.executor = executor
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    cov, proba = m(d)
    pred = project_to_plotwise_coverages(cov, d["cloud"], args, model=m)
    loss, _ = losses.total_loss(pred, proba, d["coverages"].cuda(), d["pdf_all"].cuda(), args.m, args.e)
    loss.backward()
    if B * N <= 40000:
        ref = check.train_step(sd, d, args, fps_start=fs, training=False)
        fails, report = check.compare(m, cov, proba, loss.item(), ref, pred=pred)
        print(f"\n[{B} x {N}, executor {executor}] eval-mode step vs the fp64 oracle:\n  {report}")
        assert not fails, "\n".join(fails)
    else:
        # the metric's size (the oracle takes minutes there): the two host paths against each other
        assert all(torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0 for p in m.parameters())
        m2 = _model(args, sd).eval()
        m2.executor = not executor
        cov2, proba2 = m2(d)
        pred2 = project_to_plotwise_coverages(cov2, d["cloud"], args, model=m2)
        loss2, _ = losses.total_loss(pred2, proba2, d["coverages"].cuda(), d["pdf_all"].cuda(), args.m, args.e)
        loss2.backward()
        assert torch.equal(cov2, cov) and torch.equal(proba2, proba)
        for (k, p), p2 in zip(m.named_parameters(), m2.parameters()):
            err = float((p.grad - p2.grad).abs().max() / p.grad.abs().max())
            assert err <= 2e-5, (k, err)
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), f"{k} changed in an eval-mode step"
    with torch.no_grad():
        cov0, proba0 = m(d)
    assert float((cov0 - cov).abs().max()) <= 2e-6 and float((proba0 - proba).abs().max()) <= 2e-6
    # a training step right after it is an ordinary training step (nothing of the frozen mode sticks to the model)
    m.train()
    m.zero_grad(set_to_none=True)
    cov, proba = m(d)
    pred = project_to_plotwise_coverages(cov, d["cloud"], args, model=m)
    loss, _ = losses.total_loss(pred, proba, d["coverages"].cuda(), d["pdf_all"].cuda(), args.m, args.e)
    loss.backward()
    if B * N <= 40000:
        ref = check.train_step(sd, d, args, fps_start=fs)
        fails, report = check.compare(m, cov, proba, loss.item(), ref, pred=pred)
        assert not fails, "\n".join(fails)


def _gl_count(m):
    """the sticky give-up count of a model's own exchange area (hip_ops.global_level_ws(owner=model))"""
    ws = m.__dict__.get("_gl_ws", {}).get(0)
    return int(ws[1][1].item()) if ws else 0


def _gl_step(m, d, args):
    cov, proba = m(d)
    pred = project_to_plotwise_coverages(cov, d["cloud"], args, model=m)
    (pred.square().sum() + proba[:, 1].sum() * 1e-3).backward()
    torch.cuda.synchronize()
    return dict(cov=cov.detach().clone(), proba=proba.detach().clone(), G=m.last_G_tensor.clone(),
                grads={k: p.grad.detach().clone() for k, p in m.named_parameters()},
                state={k: v.detach().clone() for k, v in m.state_dict().items()})


@pytest.mark.parametrize("B,N,ratio1", [(3, 4096, 0.125), (16, 32768, 1024 / 32768), (5, 10000, 0.25)])
def test_global_level_in_one_launch_is_the_five_launches(B, N, ratio1):
    """Training forward + backward with SA3 / plot max / FP3 and their BatchNorms in ONE launch (sn2_global_level_forward: the
    workgroups exchange the batch statistics among themselves) against the same step with the five separate launches: the
    rows of SA3 are the same tiles, the statistics are the same sums added in another grouping (1e-6), FP3 adds its
    interpolated part once per plot (outputs to 1e-5, a tenth of the oracle's tolerance),
    the running statistics and the counters move the same way, and the gradients agree to 2e-4 of their scale (the step against
    the oracle: test_forward_backward_vs_oracle_other_sizes, which runs the one launch).
    Then the give-up path (round 5): with a wait limit of one sweep the workgroups' waits run out -- and the step is STILL the
    undisturbed fused step, BIT FOR BIT (outputs, plot features, running statistics, counters; hence also the five launches'
    to the tolerances above): the gated repair launch behind the fused one recomputed the level.  The count is sticky and
    `global_level_gave_up` reports it once, as a warning."""
    args = make_args(subsample_size=N, ratio1=ratio1, r1=1.0, ratio2=0.25, r2=2.0, log_embeddings=True)
    d = make_batch(B, N, first_plot=90)
    d["fps_start"] = torch.zeros(2, B, dtype=torch.int64)
    sd = network.init_state_dict(9)
    res = {}
    for fused in (True, False):
        m = _model(args, {k: v.clone() for k, v in sd.items()}).train()
        m.fuse_global_level = fused
        res[fused] = _gl_step(m, d, args)
        assert _gl_count(m) == 0                                            # nothing gave up
    a, b = res[True], res[False]
    assert float((a["G"] - b["G"]).abs().max()) <= 2e-6 * max(1.0, float(b["G"].abs().max()))
    assert float((a["cov"] - b["cov"]).abs().max()) <= 1e-5 and float((a["proba"] - b["proba"]).abs().max()) <= 1e-5
    for k, v in b["state"].items():
        if v.dtype.is_floating_point:
            assert float((a["state"][k] - v).abs().max()) <= 1e-6 * max(1.0, float(v.abs().max())), k
        else:
            assert torch.equal(a["state"][k], v), k                      # num_batches_tracked
    for k, g in b["grads"].items():
        scale = max(float(g.abs().max()), 1e-12)
        # (statistics that differ in the 7th digit flip a few ReLU masks next to zero: 5e-5 of the scale observed at 16 x 32 768)
        assert float((a["grads"][k] - g).abs().max()) <= 2e-4 * scale + 1e-9, (k, float((a["grads"][k] - g).abs().max()), scale)
    # ---- the give-up path: every wait gives up after one sweep, the repair launch recomputes the level
    import warnings
    from stratanet2_vegetation_coverage_maps_amd import _lib
    lib = _lib.load()
    m = _model(args, {k: v.clone() for k, v in sd.items()}).train()
    m.fuse_global_level = True
    m(d)                                          # allocates the model's exchange area (and is one undisturbed step: the state
    m.load_state_dict({k: v.clone() for k, v in sd.items()})             # ... is put back)
    lib.sn2_debug_global_spin_limit(1)
    try:
        r1 = _gl_step(m, d, args)
        gave_up = _gl_count(m)
    finally:
        lib.sn2_debug_global_spin_limit(0)
    print(f"  global level B={B}: {gave_up} workgroup(s) gave up under a one-sweep wait limit")
    for k in ("cov", "proba", "G"):
        assert torch.equal(r1[k], a[k]), k                                # the bits of the undisturbed fused step
    for k, v in a["state"].items():
        assert torch.equal(r1["state"][k], v), k                          # running statistics and counters: updated exactly once
    if gave_up:
        with pytest.warns(ops.StrataHipWarning, match="gave up"):
            assert ops.global_level_gave_up(DEV_T) >= gave_up
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            ops.global_level_gave_up(DEV_T)                               # reported once
    # and the launches after it are undisturbed again (the repair moved the epoch past every stale tag)
    m.load_state_dict({k: v.clone() for k, v in sd.items()})
    r2 = _gl_step(m, d, args)
    assert _gl_count(m) == gave_up
    for k in ("cov", "proba", "G"):
        assert torch.equal(r2[k], a[k]), k


def test_global_level_give_up_is_repaired_with_one_workgroup_held_back():
    """The give-up that can really happen: ONE workgroup of the fused launch is not resident in time (here: every workgroup
    gives up at once is the other test; this one makes the waits short and runs a chip-filling idle kernel in front, so that
    some workgroups start late).  Whatever subset gives up, the step's results are the undisturbed step's."""
    B, N = 16, 8192
    args = make_args(subsample_size=N, ratio1=0.125, r1=1.0, ratio2=0.25, r2=2.0, log_embeddings=True)
    d = make_batch(B, N, first_plot=7)
    d["fps_start"] = torch.zeros(2, B, dtype=torch.int64)
    sd = network.init_state_dict(3)
    from stratanet2_vegetation_coverage_maps_amd import _lib
    lib = _lib.load()
    m = _model(args, {k: v.clone() for k, v in sd.items()}).train()
    ref = _gl_step(m, d, args)
    for limit in (2, 8, 64):
        m.load_state_dict({k: v.clone() for k, v in sd.items()})
        lib.sn2_debug_global_spin_limit(limit)
        try:
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):        # 2048 one-wave workgroups idling ~0.5 ms beside the step
                ops._call("sn2_debug_spin", 2048, 1000000, None, side.cuda_stream)
            r = _gl_step(m, d, args)
        finally:
            lib.sn2_debug_global_spin_limit(0)
        for k in ("cov", "proba", "G"):
            assert torch.equal(r[k], ref[k]), (limit, k)
        for k, v in ref["state"].items():
            assert torch.equal(r["state"][k], v), (limit, k)
    print(f"  give-ups provoked in total: {_gl_count(m)}")


DEV_T = torch.device("cuda:0")


def test_global_level_exchange_area_is_not_allocated_inside_a_capture():
    """The exchange area of the fused global level holds the launch epoch: zero fills captured into a graph would reset it at
    every replay, under the other graphs' feet.  `hip_ops.global_level_ws` refuses to allocate while a stream is capturing
    (TrainPipeline warms every slot eagerly first; this is for hosts that capture on their own)."""
    saved = dict(ops._GLOBAL_WS)
    ops._GLOBAL_WS.clear()
    try:
        g = torch.cuda.CUDAGraph()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            with pytest.raises(Exception, match="before a stream capture"):
                with torch.cuda.graph(g, stream=st):
                    ops.global_level_ws(DEV_T, 4)
        torch.cuda.synchronize()
        ws = ops.global_level_ws(DEV_T, 4)                                          # outside a capture: fine
        assert ws[0].numel() == 2 * ops.GL_MAX_PLOTS * 4 * 128 and ops.global_level_ws(DEV_T, 20) is ws    # one size, never reallocated
    finally:
        ops._GLOBAL_WS.clear()
        ops._GLOBAL_WS.update(saved)


def test_per_plot_rasters_of_a_batch_come_from_one_launch_and_are_the_same_bits():
    """The reference's inference loop (predict.py:103-126) calls `project_to_2d_rasters(clouds[idx], coverages_pointwise[idx], args)`
    per plot of the batch it just sent through the model.  The drop-in answers those calls from ONE batched launch + ONE
    device-to-host read per batch (both arguments are views of the batch's tensors): same arrays as plot-by-plot launches, for
    consecutive batches (a new batch is recognised by tensor identity, not by address), with autograd on as in the reference."""
    from stratanet2_vegetation_coverage_maps_amd import project_to_2d as p2d
    B, N = 5, 4096
    args = make_args(subsample_size=N, ratio1=0.25, r1=1.0, ratio2=0.25, r2=2.0)
    m = _model(args, network.init_state_dict(7)).eval()
    calls = []
    orig = ops.raster_project
    ops.raster_project = lambda *a, **k: (calls.append(a[0].shape[0]), orig(*a, **k))[1]
    try:
        for first in (0, 50, 0):                              # the third batch has the first one's data in new tensors
            d = make_batch(B, N, first_plot=first)
            cloud_data = {"cloud": d["cloud"], "xyz": d["xyz"], "fps_start": torch.zeros(2, B, dtype=torch.int64)}
            clouds = cloud_data["cloud"]
            cov, _ = m(cloud_data)
            cov_b = m.get_batch_format(cov)
            calls.clear()
            got = [project_to_2d_rasters(clouds[i], cov_b[i], args) for i in range(B)]
            assert calls == [B * N]                           # one launch over the whole batch
            p2d.BATCH_RASTERS = False
            try:
                calls.clear()
                want = [project_to_2d_rasters(clouds[i], cov_b[i], args) for i in range(B)]
                assert calls == [N] * B
            finally:
                p2d.BATCH_RASTERS = True
            for a, b in zip(got, want):
                assert a.dtype == np.float64 and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
            # a call that is NOT a plot of a batch (its own tensors) takes the single-plot path
            calls.clear()
            one = project_to_2d_rasters(clouds[1].clone(), cov_b[1].clone(), args)
            assert calls == [N] and np.array_equal(one, want[1], equal_nan=True)
    finally:
        ops.raster_project = orig


def test_projection_and_loss_as_one_node_is_the_two_nodes():
    """`losses.projected_total_loss` (three launches: the scatter beside the pointwise loss sums, the finalisation whose last
    workgroup adds the loss up, one backward pass for both gradients) against `project_to_plotwise_coverages` + `total_loss`
    (seven): the plot-wise predictions and BOTH gradients are the same bits, the loss terms agree to fp64 re-association --
    with all terms on, and with the NLL or the entropy switched off; a geometry handle without pixel ids falls back."""
    B, N = 6, 10000
    args = make_args(subsample_size=N)
    d = make_batch(B, N, first_plot=31)
    clouds = d["cloud"].cuda()
    g = torch.Generator().manual_seed(3)
    gt, pdf = d["coverages"].cuda(), d["pdf_all"].cuda()
    from types import SimpleNamespace
    mm, pix = ops.plot_pixels(clouds, args.diam_pix)
    geo = SimpleNamespace(p2_pix=pix, p2_diam_pix=int(args.diam_pix))
    for m_, e_ in ((0.1, 0.04), (0.0, 0.04), (0.1, 0.0)):
        args.m, args.e = m_, e_
        res = []
        for fused in (True, False):
            cov = torch.rand(B * N, 4, generator=g).cuda().requires_grad_(True) if not res else res[0][5].detach().clone().requires_grad_(True)
            proba = (torch.softmax(torch.randn(B * N, 4, generator=g), 1).cuda() if not res else res[0][6].detach().clone()).requires_grad_(True)
            if fused:
                total, parts, pred = losses_dev().projected_total_loss(cov, proba, clouds, gt, pdf, args, geometry=geo)
            else:
                pred = project_to_plotwise_coverages(cov, clouds, args, geometry=geo)
                total, parts = losses_dev().total_loss(pred, proba, gt, pdf, args.m, args.e)
            (3.0 * total).backward()
            res.append((total.item(), [p.item() for p in parts], pred.detach().clone(), cov.grad.clone(), proba.grad.clone(), cov, proba))
        a, b = res
        assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4]), (m_, e_)
        assert abs(a[0] - b[0]) <= 1e-12 * max(1.0, abs(b[0]))
        for x, y in zip(a[1], b[1]):
            assert abs(x - y) <= 1e-12 * max(1.0, abs(y))
    args.m, args.e = 0.1, 0.04
    cov = torch.rand(B * N, 4, generator=g).cuda().requires_grad_(True)
    proba = torch.softmax(torch.randn(B * N, 4, generator=g), 1).cuda()
    total, _, pred = losses_dev().projected_total_loss(cov, proba, clouds, gt, pdf, args, geometry=None)      # no ids: the two calls
    ref = project_to_plotwise_coverages(cov, clouds, args)
    assert torch.equal(pred, ref)


def losses_dev():
    from stratanet2_vegetation_coverage_maps_amd import losses as dev_losses
    return dev_losses
