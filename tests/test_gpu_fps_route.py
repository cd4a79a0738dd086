"""Every rung of every FPS ladder launches and samples like the oracle: for each template rung of the brute-force, one-sample,
speculative and multi-workgroup kernels one call of 32 samples at the smallest size that takes it, with the route
(sn2_fps_route: form, waves per workgroup, workgroups per plot, rung) written out here and asserted before the launch.  A quarter
of every plot's points are duplicates of others, so exact ties are sampled too."""
import functools

import pytest
import torch

from oracle import primitives as P
from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M = 32
BRUTE, ROUND, SPEC, CLUSTER = ops.FPS_FORM_BRUTE, ops.FPS_FORM_ROUND, ops.FPS_FORM_SPEC, ops.FPS_FORM_CLUSTER

# (B, N, waves, bucketed) -> (form, waves per workgroup, workgroups per plot, rung)
CASES = {}
# fps_kernel<PPT, T>: PPT = rung points per thread on T = 64 * nw threads; 33 plots of 4096 points: the many-small rung <16, 256>
for n, nw, ppt in ((256, 4, 1), (257, 4, 2), (512, 4, 2), (513, 4, 4), (1024, 4, 4), (1025, 16, 2), (2048, 16, 2), (2052, 16, 4),
                   (4100, 16, 8), (8196, 16, 16), (16388, 16, 32)):
    CASES[(2, n, 0, False)] = (BRUTE, nw, 1, ppt)
CASES[(33, 4096, 0, False)] = (BRUTE, 4, 1, 16)
# fps_spec_kernel<SPW, NW> / fps_bucket_kernel<SPW, 16> (waves = 1): SPW = rung bucket slots per wave.  Four waves exist up to
# 16 384 points and become eight above, eight exist up to 32 768 and become sixteen
for n, s16, r8, r4 in ((2052, 4, (8, 8), (4, 32)), (4100, 8, (8, 16), (4, 32)), (8196, 16, (8, 32), (4, 64)),
                       (16388, 32, (8, 64), (8, 64)), (32772, 64, (16, 64), (16, 64)), (65540, 128, (16, 128), None)):
    CASES[(1, n, 16, True)] = (SPEC, 16, 1, s16)
    CASES[(1, n, 1, True)] = (ROUND, 16, 1, s16)
    CASES[(1, n, 8, True)] = (SPEC,) + (r8[0], 1, r8[1])
    if r4 is not None:
        CASES[(1, n, 4, True)] = (SPEC,) + (r4[0], 1, r4[1])
# fps_cluster_kernel<SPW, NW, P>: each code at the smallest plot (a multiple of 4 points) that holds two buckets per wave -- 64, 128,
# 256 buckets for 2, 4, 8 workgroups of 16 waves; 33 (the smallest bucketed plot: 2052 points), 64, 128 for those of 8 waves
CLUSTERS = {34: (4036, 16, 2, 2), 36: (8132, 16, 4, 2), 40: (16324, 16, 8, 2), 66: (2052, 8, 2, 4), 68: (4036, 8, 4, 2), 72: (8132, 8, 8, 2)}
for w, (n, nw, p, spw) in CLUSTERS.items():
    CASES[(1, n, w, True)] = (CLUSTER, nw, p, spw)


@functools.lru_cache(maxsize=None)
def _plots(B, N):
    """Positions (B, N, 3) whose last quarter repeats the first, the starts, and the oracle's 32 samples: once per size."""
    g = torch.Generator().manual_seed(1000 * B + N)
    pos = torch.rand(B, N, 3, generator=g) * torch.tensor([20.0, 20.0, 8.0])
    q = N // 4
    pos[:, N - q:] = pos[:, :q]
    start = torch.tensor([(977 * b + 13) % N for b in range(B)])
    return pos.permute(0, 2, 1).contiguous().to(DEV), start.to(DEV, torch.int32), P.fps_batched(pos, M, start)


@pytest.mark.parametrize("B,N,waves,bucketed", list(CASES), ids=lambda v: str(int(v)))
def test_every_rung_launches_and_samples_like_the_oracle(B, N, waves, bucketed):
    want = CASES[(B, N, waves, bucketed)]
    route = ops.fps_route(B, N, M, waves=waves, bucketed=bucketed, device=DEV)
    assert tuple(route)[:4] == want
    assert bool(route.fills_ws) == (want[0] != BRUTE) and (route.repair > 0) == (want[0] == CLUSTER)
    if want[0] == CLUSTER:            # the smallest such plot: four points fewer and the request runs another kernel
        assert ops.fps_route(B, N - 4, M, waves=waves, device=DEV).form != CLUSTER
    xyz, start, ref = _plots(B, N)
    idx, cs, ca, ws = ops.fps(xyz, M, start, bucketed=bucketed, waves=waves, return_ws=True)
    assert torch.equal(idx.cpu().long(), ref)
    assert torch.equal(cs, torch.gather(xyz, 2, idx.long().unsqueeze(1).expand(-1, 3, -1)))
    assert torch.equal(ca.view(B, M, 4)[..., :3], cs.permute(0, 2, 1))
    assert (ws is not None) == bool(route.fills_ws)
    if ws is not None:
        assert torch.equal(ws[:B * N].view(B, N).long().sort(1).values, torch.arange(N, device=DEV).expand(B, N))
        assert int(ops.fps_ws_ctl(ws, B, N)[1]) == 0          # no wait of the multi-workgroup exchange gave up
