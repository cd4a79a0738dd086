"""The inputs of tests/test_gpu_boundary_geometry.py reach the decisions they are built for -- shown here on the CPU with the
oracle alone, so that the GPU tests cannot be vacuous: every condition below is a condition on the INPUTS (counted, printed and
asserted), and each deliberately wrong restatement of the oracle (tests/_boundary_plots.py) differs from the oracle on the input
set that the corresponding GPU assertion uses.  Also: the oracle's own `radius` and `knn` against their dense definitions."""
import numpy as np
import pytest
import torch

from oracle import primitives as P
from oracle import projection

import _boundary_plots as bp

CLASSES = ("d2 == fp32(r*r)", "one fp32 below", "one fp32 above")


def _centroids(xyz, m, start):
    pos = xyz.permute(0, 2, 1).contiguous()
    idx = P.fps_batched(pos, m, start)
    return idx, bp.gather_soa(xyz, idx)


@pytest.mark.parametrize("n,m", bp.BALL_SIZES)
def test_shell_classes_are_reached_by_the_fps_centroids(n, m):
    """Per planted plot and radius: each class has >= 8 (FPS centroid, point) pairs, with the centroids the oracle's FPS picks on
    the FINAL plot (planting changes FPS: counted after planting), and the anchors themselves reach every planted pair."""
    plot, anchors, planted = bp.planted_plot(n)
    xyz = plot.unsqueeze(0)
    idx, cs = _centroids(xyz, m, torch.tensor([bp.BALL_START]))
    _, cs2 = _centroids(cs, m // 4, torch.tensor([bp.BALL_START2]))
    pts = plot.t().contiguous()
    dirs = {d for *_, d in planted}
    assert dirs & set(bp.AXIS_DIRS) and dirs & set(bp.DIAG_DIRS) and any(d.startswith("r") for d in dirs)
    for r in bp.RADII:
        c1 = bp.shell_pair_counts(pts, cs[0].t().contiguous(), r)
        ca = bp.shell_pair_counts(pts, plot[:, anchors].t().contiguous(), r)
        c2 = bp.shell_pair_counts(cs[0].t().contiguous(), cs2[0].t().contiguous(), r)
        print(f"\n[{n} -> {m} -> {m // 4}, r = {r:.4f}] pairs (equal, below, above): FPS centroids x points {c1}, anchors x points {ca}, "
              f"level-2 centroids x level-1 centroids {c2}")
        assert min(c1) >= 8, (r, c1)
        want = [sum(1 for _, _, rr, cls, _ in planted if rr == r and cls == k) for k in range(3)]
        assert all(a >= w >= 8 for a, w in zip(ca, want)), (r, ca, want)
        # level 2: among real FPS samples planted pairs are rare (printed above, not asserted), so the second level also runs on
        # a level-1 set made of the anchors and planted points, the anchors as centroids
        s1, a1 = bp.shell_level1_set(n, m)
        cb = bp.shell_pair_counts(s1.t().contiguous(), s1[:, a1].t().contiguous(), r)
        print(f"    level-1 set of anchors + planted points ({s1.shape[1]}), anchors as centroids: {cb}")
        assert min(cb) >= 8, (r, cb)
    # every planted point is where it was meant to be
    for at, a, r, cls, _ in planted:
        assert P.canonical_d2(plot[:, at], plot[:, a]).item() == bp.shell_values(r)[cls]


@pytest.mark.parametrize("n,m", bp.BALL_SIZES)
def test_inclusive_ball_differs_from_the_oracle_and_radius_is_the_dense_definition(n, m):
    for kinds in (bp.KINDS5, bp.KINDS3):
        xyz = bp.batch(kinds, n)
        B = xyz.shape[0]
        idx, cs = _centroids(xyz, m, torch.full((B,), bp.BALL_START))
        for r, cap in ((1.0, 2000), (2.0 ** 0.5, 64), (2.0, 2000), (8.0 ** 0.5, 64)):
            cnt, col = bp.oracle_ball_lists(xyz, cs, r, cap)
            differ = 0
            at = 0
            for b in range(B):
                pts, cen = xyz[b].t().contiguous(), cs[b].t().contiguous()
                strict = bp.ball_mask(pts, cen, r)
                differ += int((bp.ball_mask(pts, cen, r, inclusive=True) != strict).sum()) if kinds[b] == "planted" else 0
                # P.radius == the dense matrix compared with `<`, ascending index, first `cap`
                for q in range(m):
                    want = torch.nonzero(strict[q])[:, 0][:cap]
                    k = int(cnt[b * m + q])
                    assert k == want.numel() and torch.equal(col[at:at + k], want)
                    at += k
            print(f"\n[{'+'.join(kinds)} x {n}, r = {r:.4f}] `<=` differs from `<` on {differ} (centroid, point) pairs of the planted plot")
            assert differ >= 8


def test_degenerate_plots_are_degenerate():
    for n in (2304, 2048, 2500):
        for kind, axes in bp.ZERO_EXTENT.items():
            p = bp.make_plot(kind, n, seed=3)
            ext = (p.max(1).values - p.min(1).values).tolist()
            assert [a for a in range(3) if ext[a] == 0.0] == list(axes), (kind, ext)
            d = bp.distinct_positions(p)
            print(f"\n[{kind} x {n}] extent {ext}, {d} distinct positions")
            assert d == {"one": 1, "two": 2}.get(kind, d) and d < n
            if kind in ("flat", "line", "half"):
                k = {"flat": 3 * n // 4, "line": n // 3, "half": 7 * n // 8}[kind]
                head = {tuple(v) for v in p[:, :k].t().tolist()}
                assert all(tuple(v) in head for v in p[:, k:].t().tolist())            # the tail repeats earlier points
        for step in (0.25, 0.01):
            p = bp.lattice_plot(n, step, 0)
            assert 0.5 < float((p[2] == 0).float().mean()) < 0.6
            assert float((p[0] ** 2 + p[1] ** 2).max()) <= 100.0
            q = p.double() / step
            assert float((q - q.round()).abs().max()) < 1e-4
    s = bp.repeated_and_fresh_starts(bp.batch(bp.KINDS5, 2304))
    xyz = bp.batch(bp.KINDS5, 2304)
    for b in range(2, 5):                                 # (flat, line, half disc: the padded plots)
        r, f = int(s[0, b]), int(s[1, b])
        assert (xyz[b, :, :r] == xyz[b, :, r:r + 1]).all(0).any() and not (xyz[b, :, :f] == xyz[b, :, f:f + 1]).all(0).any()


def test_tie_targets_tie_and_the_highest_index_variant_differs():
    for n, m in ((2304, 576), (2500, 625)):
        src, dst, planted = bp.tie_case(n, m)
        s, d = src.t().contiguous(), dst.t().contiguous()
        cls = bp.tie_classes(s, d)
        counts = cls.sum(0).tolist()
        print(f"\n[{m} sources, {n} targets] targets that tie at rank 1/2, 2/3, 3/4 between distinct sources: {counts[:3]}; on a source: {counts[3]}"
              f" ({planted} planted)")
        assert min(counts) >= 8 and min(cls[:planted].sum(0).tolist()) >= 8
        for k in (3, 1):
            lo, hi = bp.knn_dense(s, d, k), bp.knn_dense(s, d, k, highest=True)
            differ = int((lo != hi).any(1).sum())
            print(f"  k = {k}: highest-index-wins differs from the oracle on {differ} targets")
            assert differ >= 8 if k == 3 else differ >= 1
            idx, w = bp.oracle_knn(src.unsqueeze(0), dst.unsqueeze(0), k)                 # P.knn == the stable argsort
            assert torch.equal(idx, lo)
            assert float(w.max()) == float(np.float32(1.0) / np.float32(1e-16))            # a target on a source: 1 / clamp(0, 1e-16)
    # the degenerate plots: sources = their FPS samples, many of them one position
    xyz = bp.batch(bp.KINDS3, 2304)
    idx, cs = _centroids(xyz, 576, torch.zeros(3, dtype=torch.long))
    for b, kind in enumerate(bp.KINDS3[:2]):
        assert bp.distinct_positions(cs[b]) == {"one": 1, "two": 2}[kind]
        lo, hi = bp.knn_dense(cs[b].t().contiguous(), xyz[b].t().contiguous(), 3), bp.knn_dense(cs[b].t().contiguous(), xyz[b].t().contiguous(), 3, True)
        assert int((lo != hi).any(1).sum()) == 2304                                       # every target ties


@pytest.mark.parametrize("grid", ["p1", "p2"])
def test_pixel_edges_are_straddled_and_the_fused_forms_differ(grid):
    boxes = (None,) if grid == "p1" else (bp.P2_BOX_X, bp.P2_BOX_Y)
    for box in boxes:
        vals = bp.p1_edge_values() if grid == "p1" else bp.p2_edge_values(box)
        assert vals.shape == (19, 129) and np.all(np.diff(bp.f32_ord(vals), axis=1) == 1)        # consecutive fp32 values
        ident = bp.p1_id if grid == "p1" else (lambda v: bp.p2_id(v, box))
        for k in range(1, bp.D_PIX):
            assert set(ident(vals[k - 1]).tolist()) == {k - 1, k}, k                         # the oracle takes both ids at edge k
        want = ident(vals.reshape(-1))
        wrong = {"p1": {"multiply-add fused": bp.p1_id_fused}, "p2": {"scale pre-multiplied": lambda v: bp.p2_id_premultiplied(v, box)}}[grid]
        for name, fn in wrong.items():
            differ = int((fn(vals.reshape(-1)) != want).sum())
            print(f"\n[{grid} {'' if box is None else tuple(float(v) for v in box)}] {name}: differs from the oracle on {differ} of {vals.size} values")
            assert differ >= 1
    # the plots hold every one of these values in the stated rows, and (p2) keep the box
    clouds = bp.pixel_edge_batch(grid)
    for b, rows in enumerate(((0,), (1,), (0, 1))):
        for a in rows:
            vals = bp.p1_edge_values() if grid == "p1" else bp.p2_edge_values(bp.P2_BOX_X if a == 0 else bp.P2_BOX_Y)
            assert set(vals.reshape(-1).tolist()) <= set(clouds[b, a].tolist())
    if grid == "p2":
        for a, box in enumerate((bp.P2_BOX_X, bp.P2_BOX_Y)):
            assert torch.all(clouds[:, a].min(1).values == float(box[0])) and torch.all(clouds[:, a].max(1).values == float(box[1]))
        # through the oracle's own function on the whole batch: the ids at the planted values are the ids of `p2_id`
        pix = projection.p2_pixel_ids(clouds, bp.D_PIX)
        assert np.array_equal(pix[2, 0].numpy(), bp.p2_id(clouds[2, 0].numpy(), bp.P2_BOX_X))


def test_zero_extent_ids_are_zero_and_need_the_epsilon():
    """The bounding-box grid on the line and one-position plots: the reference's + 1e-4 makes a zero extent well defined (every id 0
    on that axis); without it the ids are not (0 / 0)."""
    for kind in ("line", "one"):
        p = bp.make_plot(kind, 2304, seed=3)
        clouds = (p[:2] / 10.0).unsqueeze(0)
        pix = projection.p2_pixel_ids(clouds, bp.D_PIX)[0]
        for a in (0, 1):
            if a in bp.ZERO_EXTENT[kind]:
                assert int(pix[a].abs().max()) == 0
                box = (clouds[0, a].min().item(), clouds[0, a].max().item())
                wrong = bp.p2_id_without_epsilon(clouds[0, a].numpy(), box)
                differ = int((wrong != pix[a].numpy()).sum())
                print(f"\n[{kind}, axis {a}] without the epsilon {differ} of 2304 ids differ from the oracle's 0")
                assert differ == 2304
            else:
                assert int(pix[a].max()) == bp.D_PIX - 1
