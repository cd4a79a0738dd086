"""Planted inputs of the per-point score tests (host arrays only): three plots of N = 256 samples over T = 500 parcel points,
diam_meters = 20, at the smallest shapes that hold every case of the rule (include/strata_hip.h, "Per-point scores")."""
import numpy as np

B, N, T, DIAM = 3, 256, 500, 20
N_REAL = (180, 100, 150)            # real points per plot
COL_BASE = (0, 0, 200)              # plot 2 lies in a second parcel whose cloud starts at column 200
SHARED = 250                        # the column all three plots sample
CENTRE, RIM = 7, 11                 # columns only plot 0 reaches: sampled once at the plot centre (w = 1.5), once at r = 10 m (w = 1.0)
ZERO, ONE_ = 13, 17                 # columns only plot 0 reaches: all eight values 0.0, all eight values 1.0
NEVER = 499                         # a column nobody samples
LIVE1 = 180                         # plot 1: 100 real + 80 appended candidates, then repeats


def planted(seed=0):
    """-> list of three per-plot dicts: point_index (n_b) int32, idx (N) int32, n_live, col_base, xyz (3,N) fp32, cov / proba (N,4)
    fp32.  Plot 0: more candidates than samples (no repeats), samples that name fake ground points, an idx beyond the
    candidates, a negative idx, a point_index entry that gives a negative column.  Plot 1: 100 real points in order, 80 fake ones,
    then 76 repeats of live samples (real points among them) that must not count.  Plot 2: col_base 200 and a point_index entry
    whose column is >= T."""
    rng = np.random.default_rng(seed)
    only0 = np.array([CENTRE, RIM, ZERO, ONE_])
    pool01 = np.setdiff1d(np.arange(20, 330), [SHARED])
    p0 = np.sort(np.concatenate([only0, [SHARED], rng.choice(pool01, N_REAL[0] - 5, replace=False)])).astype(np.int32)
    p1 = np.sort(np.concatenate([[SHARED], rng.choice(pool01, N_REAL[1] - 1, replace=False)])).astype(np.int32)
    p2 = np.sort(np.concatenate([[SHARED - COL_BASE[2]], rng.choice(np.setdiff1d(np.arange(0, 299), [SHARED - COL_BASE[2]]),
                                                                     N_REAL[2] - 1, replace=False)])).astype(np.int32)
    assert NEVER - COL_BASE[2] not in p2
    # plot 0: 256 distinct candidates of 180 + 316; the planted columns among them
    need0 = [int(np.nonzero(p0 == c)[0][0]) for c in (CENTRE, RIM, ZERO, ONE_, SHARED)]
    rest0 = rng.choice(np.setdiff1d(np.arange(N_REAL[0] + 316), need0), N - len(need0), replace=False)
    idx0 = rng.permutation(np.concatenate([need0, rest0])).astype(np.int32)
    assert (idx0 >= N_REAL[0]).sum() > 20                                   # samples that name fake ground points
    free = [j for j in range(N) if idx0[j] >= N_REAL[0]][:2]                # two fake-ground samples become the bad ones
    idx0[free[0]] = N_REAL[0] + 316 + 5                                     # beyond the plot's candidates
    idx0[free[1]] = -4                                                      # negative
    p0 = p0.copy()
    victim = int(idx0[[j for j in range(N) if 0 <= idx0[j] < N_REAL[0] and idx0[j] not in need0][0]])
    p0[victim] = -3                                                         # column -3: ignored
    # plot 1: candidates 0..179 in order, then repeats of them
    idx1 = np.concatenate([np.arange(LIVE1), rng.integers(0, LIVE1, N - LIVE1)]).astype(np.int32)
    assert (idx1[LIVE1:] < N_REAL[1]).sum() > 10                            # repeats of REAL points: they must not count
    # plot 2: 256 distinct candidates of 150 + 316, the shared point among them; one entry points past the arena
    s2 = int(np.nonzero(p2 == SHARED - COL_BASE[2])[0][0])
    idx2 = rng.permutation(np.concatenate([[s2], rng.choice(np.setdiff1d(np.arange(N_REAL[2] + 316), [s2]), N - 1, replace=False)])).astype(np.int32)
    p2 = p2.copy()
    far = int(idx2[[j for j in range(N) if 0 <= idx2[j] < N_REAL[2] and idx2[j] != s2][0]])
    p2[far] = 320                                                           # column 520 >= T: ignored
    plots = []
    for b, (p, idx, live) in enumerate(((p0, idx0, N), (p1, idx1, LIVE1), (p2, idx2, N))):
        ang, rad = rng.random(N) * 2 * np.pi, 10.0 * np.sqrt(rng.random(N))
        xyz = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.random(N) * 20]).astype(np.float32)
        plots.append(dict(point_index=p, idx=idx, n_live=live, col_base=COL_BASE[b], xyz=xyz,
                          cov=rng.random((N, 4), dtype=np.float32), proba=rng.random((N, 4), dtype=np.float32)))
    j = {c: int(np.nonzero(idx0 == need0[k])[0][0]) for k, c in enumerate((CENTRE, RIM, ZERO, ONE_))}
    plots[0]["xyz"][:2, j[CENTRE]] = (0.0, 0.0)
    plots[0]["xyz"][:2, j[RIM]] = (6.0, 8.0)
    plots[0]["cov"][j[ZERO]] = plots[0]["proba"][j[ZERO]] = 0.0
    plots[0]["cov"][j[ONE_]] = plots[0]["proba"][j[ONE_]] = 1.0
    plots[0]["planted_samples"] = j
    return plots


def batch_of(plots):
    """the plots, in the order given, as one batch of the arrays `_point_scores_ref.contributions` and `hip_ops.points_merge` take"""
    n = [len(p["point_index"]) for p in plots]
    return dict(cov=np.concatenate([p["cov"] for p in plots]), proba=np.concatenate([p["proba"] for p in plots]),
                xyz=np.stack([p["xyz"] for p in plots]), idx=np.stack([p["idx"] for p in plots]),
                n_live=np.array([p["n_live"] for p in plots], dtype=np.int32),
                offsets=np.concatenate([[0], np.cumsum(n)]).astype(np.int32),
                point_index=np.concatenate([p["point_index"] for p in plots]).astype(np.int32),
                col_base=np.array([p["col_base"] for p in plots], dtype=np.int32))
