"""The projection and loss kernels alone (csrc/project.hip, csrc/loss.hip, csrc/loss_grad.h) against fp64 at their edges, through
hip_ops, on the cases of tests/_projection_loss_ref.py (tests/test_projection_loss_ref_host.py proves on the CPU what this file
rests on).  Every entry point is run alone: the forward routes sn2_plot_project_forward, sn2_plot_pixels +
sn2_plot_project_forward_pix, sn2_projected_loss_forward, sn2_plot_losses, sn2_raster_project and sn2_loss_forward; the backward
entries sn2_plot_project_backward, sn2_loss_backward and sn2_projected_loss_backward, each fed the REFERENCE's arg, nocc and
fp32-rounded pred, so that each is judged on its own arithmetic.

Exact, on both value families: the pixel ids of the xy routes (the oracle's), arg (-1 on empty cells), nocc, the P1 rasters and
the places of their NaNs, the bits of pred / arg / nocc between the P2 routes, the bytes of a second call, the zero pattern of
the coverage gradient (non-zero exactly at the arg-max point of an occupied cell, per channel; column 1 all zero; every row
written -- the output block is poisoned with NaN before the call), terms that are switched off (0.0).
Bounded (none invented here):
  * pred, dyadic family: one fp32 ulp of the fp64 mean (the sums are exact, the quotient is rounded once);
  * pred, uniform family: 1e-6 absolute (test_pixel_indices_bit_exact_and_p2_gradient);
  * the four outputs of the one-node forward and of sn2_loss_forward, the seven per plot of sn2_plot_losses:
    1e-6 max(1, |ref|) (TOL_FORMS of tests/test_gpu_eval.py);
  * dcov, dproba, dpred: the distance from fp64 over the tensor's largest element is at most max(1e-6, 8 e32), never above 1e-5
    (atol and rtol of test_losses_match_oracle; factor and rule of tests/test_gpu_sa_modules.py); e32 is the same distance of the
    reference restated with the kernels' types on the CPU.
Limits: diam_pix = 46 is refused by every forward route before any launch, 45 is accepted.
Every figure is printed beside its bound before anything is asserted (run with -s); the largest per output are printed at the
end.
Measured on an MI355X, largest over all cases ("Projection and loss kernels alone"):
  pred 7.3e-8 (uniform), 0.50 ulp (dyadic); one-node forward and loss_forward outputs 2.7e-8, plot_losses columns 7.0e-8;
  loss_backward dpred 5.3e-8 (e32 5.3e-8), dproba 1.15e-7 (e32 <= 7.0e-8, kernel / e32 <= 1.82); plot_project_backward dcov
  1.30e-7 (e32 1.30e-7); projected_loss_backward dcov 1.28e-7 (e32 1.28e-7), dproba 1.15e-7 (kernel / e32 <= 1.82);
  kernel / e32 = 1.00 on dpred and dcov; the gradient bound never exceeded 1.04e-6.  No test failed on the kernels as they are;
  five deliberately wrong kernels (DESIGN.md lists them) each failed at least five tests.
"""
import numpy as np
import pytest
import torch

import _projection_loss_ref as R
from stratanet2_vegetation_coverage_maps_amd import _lib, hip_ops as ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64, F32 = np.float64, np.float32
PRED_TOL, TOL_FORMS = 1e-6, 1e-6
ATOM, FACTOR, BOUND = 1e-6, 8, 1e-5
CASES = R.case_ids()
IDS = [f"{n}-{f}" for n, f in CASES]
XY = [(n, f) for n, f in CASES if R.SHAPES[n][3]]
_DEV, _WORST = {}, {}


def _dev(name, family):
    """the case on the device, uploaded once"""
    key = (name, family)
    if key not in _DEV:
        c = R.case(name, family)
        d = {k: torch.tensor(getattr(c, k), device=DEV) for k in ("cov", "pix", "proba", "proba_zero", "pdf", "gt")}
        d["cloud"] = None if c.cloud is None else torch.tensor(c.cloud, device=DEV)
        d["g"] = torch.tensor([R.G], dtype=torch.float64, device=DEV)
        _DEV[key] = d
    return _DEV[key]


def _proba(d, m):
    return d["proba"] if m != 0.0 else d["proba_zero"]


def _np(t):
    return t.detach().cpu().numpy()


def _fig(what, label, value, bound, e32=None):
    """print a figure beside its bound, keep the largest per output; -> within the bound"""
    w = _WORST.setdefault(what, dict(value=0.0, bound=bound, label=label, e32=0.0, ratio=0.0))
    if value >= w["value"]:
        w.update(value=value, bound=bound, label=label)
    tail = ""
    if e32 is not None:
        w["e32"] = max(w["e32"], e32)
        if e32 > 0:
            w["ratio"] = max(w["ratio"], value / e32)
        tail = f"  e32 {e32:.2e}"
    print(f"{label} {what}: {value:.3e} (bound {bound:.1e}){tail}")
    return value <= bound


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\nlargest figure per output (tests/test_gpu_projection_loss.py):")
    for what, w in sorted(_WORST.items()):
        print(f"  {what}: {w['value']:.3e} of {w['bound']:.1e} at {w['label']}" +
              (f"; largest e32 {w['e32']:.2e}, largest kernel/e32 {w['ratio']:.2f}" if w["e32"] else ""))


def _grad_bound(e32):
    return min(max(ATOM, FACTOR * e32), BOUND)


def _poison(rows):
    """fill the block the next (rows, 4) fp32 output is carved from with NaN: the caching allocator hands the block freed last
    to the next request of its size, so a row the kernel does not write shows"""
    t = torch.full((rows, 4), float("nan"), device=DEV)
    del t


def _same_bytes(a, b):
    return all(torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)) for x, y in zip(a, b))


def _check_projection(label, c, r, pred, arg, nocc):
    """arg, nocc exact; pred within its family's bound"""
    assert np.array_equal(_np(arg).reshape(c.B, c.D * c.D, 3), r["arg"]), f"{label}: arg"
    assert np.array_equal(_np(nocc), r["nocc"]), f"{label}: nocc"
    got = _np(pred).astype(F64)
    if c.family == "dyadic":
        ulp = np.spacing(np.abs(r["pred"]).astype(F32)).astype(F64)
        ok = _fig("pred (dyadic, in ulp)", label, float((np.abs(got - r["pred"]) / ulp).max()), 1.0)
    else:
        ok = _fig("pred (uniform)", label, float(np.abs(got - r["pred"]).max()), PRED_TOL)
    assert ok, f"{label}: pred"


# ---------------------------------------------------------------------------------------------------------- forward routes
@pytest.mark.parametrize("name,family", CASES, ids=IDS)
def test_p2_routes_alone(name, family):
    c, r, d = R.case(name, family), R.ref(name, family), _dev(name, family)
    B, N, D = c.B, c.N, c.D
    m, e = R.ME[0]
    routes = {}
    if c.cloud is not None:
        pred, pix, arg, nocc = ops.plot_project_forward(d["cov"], d["cloud"], D)
        assert torch.equal(pix, d["pix"]), "plot_project_forward: pixel ids"
        routes["atomic"] = (pred, arg, nocc)
        again = ops.plot_project_forward(d["cov"], d["cloud"], D)
        assert _same_bytes((pred, pix, arg, nocc), again)
        _, pix = ops.plot_pixels(d["cloud"], D)
        assert torch.equal(pix, d["pix"]), "plot_pixels: pixel ids"
        assert torch.equal(ops.plot_pixels(d["cloud"], D)[1], pix)
    pred, _, arg, nocc = ops.plot_project_forward_pix(d["cov"], d["pix"], B, N, D)
    routes["pix"] = (pred, arg, nocc)
    again = ops.plot_project_forward_pix(d["cov"], d["pix"], B, N, D)
    assert _same_bytes(routes["pix"], (again[0], again[2], again[3]))
    out, pred, arg, nocc = ops.projected_loss_forward(d["cov"], d["pix"], d["proba"], d["pdf"], d["gt"], B, N, D, m, e)
    routes["one_node"] = (pred, arg, nocc)
    again = ops.projected_loss_forward(d["cov"], d["pix"], d["proba"], d["pdf"], d["gt"], B, N, D, m, e)
    assert _same_bytes((out, pred, arg, nocc), again)
    plots, pred_l = ops.plot_losses(d["cov"], d["pix"], d["proba"], d["pdf"], d["gt"], B, N, D, m, e)
    again = ops.plot_losses(d["cov"], d["pix"], d["proba"], d["pdf"], d["gt"], B, N, D, m, e)
    assert _same_bytes((plots, pred_l), again)
    torch.cuda.synchronize()
    for route, (pred, arg, nocc) in routes.items():
        _check_projection(f"{name}-{family} {route}", c, r, pred, arg, nocc)
    first = routes["pix"]
    for route, other in routes.items():
        assert _same_bytes(first, other), f"{route}: the P2 routes give each other's pred / arg / nocc bits"
    assert _same_bytes((first[0],), (pred_l,)), "plot_losses: the same pred bits"


@pytest.mark.parametrize("name,family", CASES, ids=IDS)
def test_loss_outputs_alone(name, family):
    c, d = R.case(name, family), _dev(name, family)
    B, N, D = c.B, c.N, c.D
    for m, e in R.me_of(name):
        r, label = R.ref(name, family, m, e), f"{name}-{family} m={m} e={e}"
        q = _proba(d, m)
        out = _np(ops.projected_loss_forward(d["cov"], d["pix"], q, d["pdf"], d["gt"], B, N, D, m, e)[0])
        plots = _np(ops.plot_losses(d["cov"], d["pix"], q, d["pdf"], d["gt"], B, N, D, m, e)[0])
        pred32 = R.ref_backward(name, family, m, e)[0]
        alone = _np(ops.loss_forward(torch.tensor(pred32, device=DEV), d["gt"], q, d["pdf"], m, e))
        want_alone, _ = R.losses(pred32, c.proba_for(m), c.pdf, c.gt, B, N, m, e)
        ok = _fig("one-node forward, 4 outputs", label, float((np.abs(out - r["out"]) / np.maximum(1.0, np.abs(r["out"]))).max()), TOL_FORMS)
        ok &= _fig("plot_losses, 7 columns", label, float((np.abs(plots - r["plots"]) / np.maximum(1.0, np.abs(r["plots"]))).max()), TOL_FORMS)
        ok &= _fig("loss_forward, 4 outputs", label, float((np.abs(alone - want_alone) / np.maximum(1.0, np.abs(want_alone))).max()), TOL_FORMS)
        assert ok, label
        for col, w in ((2, m), (3, e)):
            if w == 0.0:
                assert out[col] == 0.0 and alone[col] == 0.0 and not plots[:, col].any(), f"{label}: a term that is off is exactly 0.0"
        if m == 0.0:
            bare = _np(ops.plot_losses(d["cov"], d["pix"], q, None, d["gt"], B, N, D, m, e)[0])
            assert bare.tobytes() == plots.tobytes(), "plot_losses without densities when m = 0"


@pytest.mark.parametrize("name,family", XY, ids=[f"{n}-{f}" for n, f in XY])
def test_raster_route_alone(name, family):
    c, d = R.case(name, family), _dev(name, family)
    want = R.raster(c.cov, c.cell1, c.B, c.N, c.D)
    rasters, pix = ops.raster_project(d["cov"], d["cloud"], c.D, c.diam_meters)
    again = ops.raster_project(d["cov"], d["cloud"], c.D, c.diam_meters)
    assert np.array_equal(_np(pix), c.cell1), "raster_project: pixel ids"
    got = _np(rasters)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN exactly where no point falls"
    assert np.array_equal(np.nan_to_num(got), np.nan_to_num(want)), "maxima of fp32 values: exact"
    assert _same_bytes((rasters, pix), again)


# --------------------------------------------------------------------------------------------------------- backward entries
def _check_grad(what, label, got, ref64, ref32):
    e32 = R.dist(ref32, ref64)
    return _fig(what, label, R.dist(got, ref64), _grad_bound(e32), e32)


def _check_pattern(label, dcov, ref64):
    assert not np.isnan(dcov).any(), f"{label}: every row is written"
    assert np.array_equal(dcov != 0, ref64 != 0), f"{label}: non-zero exactly at the arg-max points"
    assert not dcov[:, 1].any(), f"{label}: column 1"


@pytest.mark.parametrize("name,family", CASES, ids=IDS)
def test_backward_entries_alone(name, family):
    c, d = R.case(name, family), _dev(name, family)
    B, N, D = c.B, c.N, c.D
    r = R.ref(name, family)
    arg = torch.tensor(r["arg"].reshape(-1), device=DEV)
    nocc = torch.tensor(r["nocc"], device=DEV)
    # the projection's backward: a d / d pred whose column 1 is not zero (the g0 - g1 of the low channel)
    up = np.random.default_rng(3).standard_normal((B, 4)).astype(F32)
    label = f"{name}-{family}"
    _poison(c.R)
    got = _np(ops.plot_project_backward(torch.tensor(up, device=DEV), arg, nocc, d["pix"], B, N, D))
    want = [R.project_backward(up, r["arg"], r["nocc"], c.pix, B, N, D, t) for t in (F64, F32)]
    ok = _check_grad("plot_project_backward dcov", label, got, *want)
    _check_pattern(label + " plot_project_backward", got, want[0])
    assert ok, label
    for m, e in R.me_of(name):
        label = f"{name}-{family} m={m} e={e}"
        pred32, dpred64, dcov64, dproba64 = R.ref_backward(name, family, m, e)
        _, dpred32, dcov32, dproba32 = R.ref_backward(name, family, m, e, f32=True)
        pred, q = torch.tensor(pred32, device=DEV), _proba(d, m)
        dpred, dproba = ops.loss_backward(pred, d["gt"], q, d["pdf"], m, e, d["g"])
        ok = _check_grad("loss_backward dpred", label, _np(dpred), dpred64, dpred32)
        ok &= _check_grad("loss_backward dproba", label, _np(dproba), dproba64, dproba32)
        assert not _np(dpred)[:, 1].any()
        _poison(c.R)
        dcov, dproba = ops.projected_loss_backward(pred, d["gt"], q, d["pdf"], B, N, D, m, e, d["g"], arg, nocc, d["pix"])
        dcov = _np(dcov)
        ok &= _check_grad("projected_loss_backward dcov", label, dcov, dcov64, dcov32)
        ok &= _check_grad("projected_loss_backward dproba", label, _np(dproba), dproba64, dproba32)
        _check_pattern(label + " projected_loss_backward", dcov, dcov64)
        assert ok, label


# ------------------------------------------------------------------------------------------------------------------- limits
def _tiny(D):
    B, N = 1, 4
    g = torch.Generator().manual_seed(0)
    cloud = torch.rand(B, 3, N, generator=g).to(DEV)
    cov = torch.rand(B * N, 4, generator=g).to(DEV)
    pix = torch.tensor([0, 1 % (D * D), D * D - 1, 0], dtype=torch.int32, device=DEV)
    proba = torch.softmax(torch.randn(B * N, 4, generator=g), 1).to(DEV)
    pdf = (torch.rand(B * N, 3, generator=g, dtype=torch.float64) + 0.05).to(DEV)
    gt = torch.rand(B, 4, generator=g, dtype=torch.float64).to(DEV)
    return B, N, {
        "plot_project_forward": lambda: ops.plot_project_forward(cov, cloud, D),
        "plot_pixels": lambda: ops.plot_pixels(cloud, D),
        "plot_project_forward_pix": lambda: ops.plot_project_forward_pix(cov, pix, B, N, D),
        "projected_loss_forward": lambda: ops.projected_loss_forward(cov, pix, proba, pdf, gt, B, N, D, 0.1, 0.04),
        "plot_losses": lambda: ops.plot_losses(cov, pix, proba, pdf, gt, B, N, D, 0.1, 0.04),
        "raster_project": lambda: ops.raster_project(cov, cloud, D, 20),
    }


def test_diam_pix_46_is_refused_and_45_is_accepted():
    """return codes only: a refusal comes before any launch, and the accepted calls use ids inside the 45 x 45 grid"""
    B, N, routes = _tiny(46)
    assert ops.plot_losses_ws_words(B, N, 46) == 0 and ops.plot_losses_ws_words(B, N, 45) > 0
    for name, call in routes.items():
        with pytest.raises((_lib.StrataHipError, ValueError)) as err:
            call()
        assert "SN2_ELIMIT" in str(err.value), name
    B, N, routes = _tiny(45)
    for name, call in routes.items():
        call()
    torch.cuda.synchronize()
