"""sn2_plots_append restated in numpy from the text of include/strata_hip.h -- not from the kernel: plot by plot, with slices.
tests/test_gpu_plotset.py holds the kernel to it; tests/test_pseudo_label_host.py holds it to hand-written cases."""
import numpy as np

SENTINEL_F32 = np.uint32(0x7FC5A5A5)           # a NaN with a payload no copy of real data produces
SENTINEL_F64 = np.uint64(0x7FF8A5A55A5AA5A5)
SENTINEL_I32 = np.int32(-0x5A5A5A5B)


def dst_start_of(n_points, sel, T0):
    """The host-made table: dst_start[0] = T0, dst_start[k+1] = dst_start[k] + the points of plot sel[k]."""
    n = np.asarray(n_points, dtype=np.int64)
    return (int(T0) + np.concatenate([[0], np.cumsum(n[np.asarray(sel, dtype=np.int64)])])).astype(np.int64)


def sentinel_destination(cap_T, cap_P):
    """A destination arena in which every word is a sentinel: (raw (10,cap_T) f32, offsets (cap_P+1) i32, centers (cap_P,2) f32,
    cov (cap_P,4) f64)."""
    raw = np.full((10, cap_T), SENTINEL_F32, dtype=np.uint32).view(np.float32)
    offsets = np.full(cap_P + 1, SENTINEL_I32, dtype=np.int32)
    centers = np.full((cap_P, 2), SENTINEL_F32, dtype=np.uint32).view(np.float32)
    cov = np.full((cap_P, 4), SENTINEL_F64, dtype=np.uint64).view(np.float64)
    return raw, offsets, centers, cov


def plots_append_ref(src_raw, src_offsets, src_centers, src_cov, sel, dst_raw, dst_offsets, dst_centers, dst_cov, P0, T0, dst_start):
    """The writes of the header, on COPIES of the destination arrays -> (raw, offsets, centers, cov).  Word moves go through
    integer views, so NaN payloads survive."""
    raw, offsets = dst_raw.copy(), dst_offsets.copy()
    centers, cov = dst_centers.copy(), dst_cov.copy()
    raw_w, src_w = raw.view(np.uint32), np.ascontiguousarray(src_raw).view(np.uint32)
    K = len(sel)
    assert len(dst_start) == K + 1 and int(dst_start[0]) == T0
    for k, p in enumerate(sel):
        lo, hi = int(src_offsets[p]), int(src_offsets[p + 1])
        d = int(dst_start[k])
        assert int(dst_start[k + 1]) - d == hi - lo
        raw_w[:, d:d + hi - lo] = src_w[:, lo:hi]
        offsets[P0 + k] = d
        centers[P0 + k] = src_centers[p]
        cov[P0 + k] = src_cov[p].astype(np.float64)
    offsets[P0 + K] = int(dst_start[K])
    return raw, offsets, centers, cov
