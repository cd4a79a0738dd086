"""The live-set rule of sn2_fps_live (include/strata_hip.h) restated on the CPU with the oracle's distance, for
tests/test_fps_live_host.py and tests/test_gpu_fps_live.py.  Not a test module."""
import torch

from oracle import primitives as P


def fps_live_ref(pos, m, start, n_live=None):
    """pos (B,N,3), start (B), n_live (B) or None (= N) -> (idx (B,m) int64, count (B) int64).
    Plot b: the arg-max (lowest index on ties) runs over points [0, n_live[b]) only, the start is emitted as itself; once the
    largest running distance is 0 every remaining sample is index 0; count = samples emitted before that, m if never.
    With n_live = None this is oracle.primitives.fps_batched plus the count."""
    B, N, _ = pos.shape
    idx = torch.zeros(B, m, dtype=torch.long)
    count = torch.full((B,), m, dtype=torch.long)
    for b in range(B):
        n = N if n_live is None else min(max(int(n_live[b]), 1), N)
        live = pos[b:b + 1, :n]
        s = int(start[b])
        idx[b, 0] = s
        dist = P.canonical_d2(live, pos[b:b + 1, s].unsqueeze(1))
        for i in range(1, m):
            if float(dist.max()) == 0.0:
                count[b] = i
                break
            a = int(torch.argmax(dist, dim=1))
            idx[b, i] = a
            dist = torch.minimum(dist, P.canonical_d2(live, pos[b:b + 1, a].unsqueeze(1)))
    return idx, count


def repeated_tail_plots(N, ns, starts, dup_plots=(), seed=0):
    """(B,N,3) positions: plot b has ns[b] distinct random points in front (in `dup_plots`: two of them are true duplicates of
    earlier prefix points) and copies drawn with randint(0, n) behind them, as sample_cloud pads a short plot."""
    g = torch.Generator().manual_seed(seed)
    B = len(ns)
    pos = torch.empty(B, N, 3)
    for b, n in enumerate(ns):
        p = torch.rand(n, 3, generator=g) * torch.tensor([2.0, 2.0, 0.5])
        if b in dup_plots and n >= 8:
            p[n // 2] = p[3]
            p[n - 1] = p[5]
        tail = torch.randint(0, n, (N - n,), generator=g)
        pos[b] = torch.cat([p, p[tail]], 0)
    return pos, torch.tensor(list(starts), dtype=torch.long)
