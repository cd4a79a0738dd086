"""The per-point scores of a parcel cloud (include/strata_hip.h, "Per-point scores"), restated in numpy: int64 sums in units of
2^-32, np.rint (round to nearest even), fp64 weight and division.  Every function is plain array arithmetic; nothing here knows
the kernels."""
import numpy as np

ONE = 2.0 ** 32


def contributions(cov, proba, xyz, idx, n_live, offsets, point_index, T, diam_meters, col_base=None):
    """The contributions of one batch -> (col (C) int64, terms (C,9) int64): per contribution its parcel column and the nine
    fixed-point terms [w, w v_1 .. w v_8].  cov, proba (B*N,4) fp32; xyz (B,3,N) fp32; idx (B,N); n_live (B); offsets (B+1) into
    point_index; col_base (B) or None."""
    cov, proba = np.asarray(cov, dtype=np.float32), np.asarray(proba, dtype=np.float32)
    xyz = np.asarray(xyz, dtype=np.float32)
    idx, n_live, offsets = np.asarray(idx, dtype=np.int64), np.asarray(n_live, dtype=np.int64), np.asarray(offsets, dtype=np.int64)
    point_index = np.asarray(point_index, dtype=np.int64)
    B, N = idx.shape
    base = np.zeros(B, dtype=np.int64) if col_base is None else np.asarray(col_base, dtype=np.int64)
    n_b = offsets[1:] - offsets[:-1]
    j = np.arange(N, dtype=np.int64)[None, :]
    ok = (j < n_live[:, None]) & (idx >= 0) & (idx < n_b[:, None])
    ok &= ((offsets[:-1] >= 0) & (n_b >= 0) & (offsets[1:] <= len(point_index)))[:, None]
    b, jj = np.nonzero(ok)
    col = base[b] + point_index[offsets[b] + idx[b, jj]]
    inside = (col >= 0) & (col < T)
    b, jj, col = b[inside], jj[inside], col[inside]
    dx, dy = xyz[b, 0, jj].astype(np.float64), xyz[b, 1, jj].astype(np.float64)
    w = 1.5 - np.sqrt(dx * dx + dy * dy) / float(diam_meters)
    v = np.concatenate([cov.reshape(B, N, 4)[b, jj], proba.reshape(B, N, 4)[b, jj]], 1).astype(np.float64)     # (C,8)
    terms = np.empty((len(col), 9), dtype=np.int64)
    terms[:, 0] = np.rint(w * ONE).astype(np.int64)
    terms[:, 1:] = np.rint(w[:, None] * v * ONE).astype(np.int64)
    return col, terms


def accumulate(acc, hits, col, terms):
    """acc (T,9) int64 and hits (T) int32, in place: the integer sums of the contributions, in the order given."""
    np.add.at(acc, col, terms)
    np.add.at(hits, col, 1)


def finalize(acc, hits):
    """-> (scores (8,T) fp32, weight (T) fp32): fp64 quotients cast to fp32; NaN scores and weight 0 where hits == 0."""
    T = len(hits)
    hit = hits > 0
    scores = np.full((8, T), np.nan, dtype=np.float32)
    den = acc[hit, 0].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        scores[:, hit] = (acc[hit, 1:].astype(np.float64) / den[:, None]).T.astype(np.float32)
    weight = np.zeros(T, dtype=np.float32)
    weight[hit] = (den / ONE).astype(np.float32)
    return scores, weight


def point_scores(batches, T, diam_meters):
    """batches: dicts with cov, proba, xyz, idx, n_live, offsets, point_index and optionally col_base -> (scores, weight, hits)."""
    acc, hits = np.zeros((T, 9), dtype=np.int64), np.zeros(T, dtype=np.int32)
    for bt in batches:
        accumulate(acc, hits, *contributions(bt["cov"], bt["proba"], bt["xyz"], bt["idx"], bt["n_live"], bt["offsets"],
                                             bt["point_index"], T, diam_meters, bt.get("col_base")))
    return finalize(acc, hits) + (hits,)
