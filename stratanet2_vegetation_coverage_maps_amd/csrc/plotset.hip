// plotset.hip -- growing a plot set that lives on the device: K plots picked out of a source plot list (a parcel's prepared plots
// with their plot-wise predictions, or another set) are appended behind the P0 plots / T0 points a destination arena already
// holds.  Host side: hip_ops.plots_append, train_data.ResidentPlots.append.
//
// Contract: include/strata_hip.h, sn2_plots_append.  One launch, a plain copy: one thread per destination column in [T0, new_T)
// finds its plot in the host-made table of destination starts (a binary search per wave, then a short walk per lane) and moves
// the column's ten channels, one dword per lane and row: a wave reads and writes 256 contiguous bytes per row wherever it lies
// inside one plot.  The starts of a plot in the source and in the destination are arbitrary, so nothing wider than a dword is
// assumed aligned.  The first K + 1 threads also write the per-plot rows.  40 B read and 40 B written per point; no atomics, no
// workspace, and every output word has exactly one writer, so the bytes do not depend on the order in which the waves run.
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void plots_append_kernel(const float* __restrict__ src_raw, long src_T,
                                                           const int* __restrict__ src_offsets,
                                                           const float* __restrict__ src_centers,
                                                           const float* __restrict__ src_cov, const int* __restrict__ sel, int K,
                                                           float* __restrict__ dst_raw, long cap_T, int* __restrict__ dst_offsets,
                                                           float* __restrict__ dst_centers, double* __restrict__ dst_cov, int P0,
                                                           int T0, const int* __restrict__ dst_start, int n_cols) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g <= K) {                                                 // the per-plot rows: K + 1 offsets, K centres and coverages
        dst_offsets[P0 + g] = dst_start[g];
        if (g < K) {
            const int p = sel[g];
            const size_t d = (size_t)P0 + g;
            dst_centers[2 * d] = src_centers[2 * (size_t)p];
            dst_centers[2 * d + 1] = src_centers[2 * (size_t)p + 1];
#pragma unroll
            for (int c = 0; c < 4; ++c) dst_cov[4 * d + c] = (double)src_cov[4 * (size_t)p + c];
        }
    }
    if (g >= n_cols) return;
    const int col = T0 + (int)g;
    // The plot k with dst_start[k] <= col < dst_start[k + 1]: of equal neighbours (empty plots) the LAST start at or below col.
    // The lanes of a wave hold consecutive columns, so the binary search runs once per wave, for its first column (the first
    // active lane's: lanes only drop out at the high end) -- wave-uniform loads instead of ten dependent loads per lane; each
    // lane then steps over the few plot starts between that column and its own (none, for most waves).
    const int col0 = __builtin_amdgcn_readfirstlane(col);
    int lo = 0, hi = K;                                           // dst_start[lo] <= col0 < dst_start[hi] throughout
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (dst_start[mid] <= col0) lo = mid; else hi = mid;
    }
    int k = lo;
    while (k + 1 < K && dst_start[k + 1] <= col) ++k;
    const int p = sel[k];
    const int s0 = src_offsets[p], i = col - dst_start[k];
    if (i >= src_offsets[p + 1] - s0) return;                     // a start table that is not the plots' running sum: no read past the plot
    const size_t s = (size_t)s0 + i;
#pragma unroll
    for (int c = 0; c < 10; ++c) dst_raw[(size_t)c * cap_T + col] = src_raw[(size_t)c * src_T + s];
}

}  // namespace

extern "C" int sn2_plots_append(const float* src_raw, long src_T, const int* src_offsets, const float* src_centers,
                                const float* src_cov, const int* sel, int K, float* dst_raw, long cap_T, int* dst_offsets,
                                float* dst_centers, double* dst_cov, int cap_P, int P0, long T0, const int* dst_start, long new_T,
                                void* stream) {
    if (!src_raw || !src_offsets || !src_centers || !src_cov || !sel || !dst_raw || !dst_offsets || !dst_centers || !dst_cov ||
        !dst_start)
        return SN2_EINVAL;
    if (K <= 0 || P0 < 0 || T0 < 0 || src_T < 0 || cap_T < 0 || cap_P < 0) return SN2_EINVAL;
    if ((long)P0 + K > cap_P || new_T > cap_T || new_T < T0) return SN2_EINVAL;
    if (cap_T >= (1L << 31) || src_T >= (1L << 31)) return SN2_ELIMIT;
    const long n_cols = new_T - T0, threads = n_cols > (long)K + 1 ? n_cols : (long)K + 1;
    hipLaunchKernelGGL(plots_append_kernel, dim3(sn2_cdiv(threads, 256)), dim3(256), 0, (hipStream_t)stream, src_raw, src_T,
                       src_offsets, src_centers, src_cov, sel, K, dst_raw, cap_T, dst_offsets, dst_centers, dst_cov, P0, (int)T0,
                       dst_start, (int)n_cols);
    SN2_RETURN_LAUNCH();
}
