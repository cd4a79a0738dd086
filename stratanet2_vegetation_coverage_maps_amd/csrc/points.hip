// points.hip -- the per-point scores of a parcel cloud: the network's pointwise coverages and class probabilities of every batch
// scattered back onto the parcel's own points and merged over the overlapping plots by the mosaic's radial weight.  Host side:
// inference.PointScores.
//
// Contract (include/strata_hip.h, "Per-point scores"; the rule's functions: point_rules.h):
//   - a sample contributes once per (plot, parcel point): repeats past n_live and fake ground points do not;
//   - the sums are 64-bit INTEGERS in units of 2^-32 (vector global atomics, no result read back), so they do not depend on the
//     order of arrival: any batching, plot order or launch split gives the same bytes.  No floating-point atomic anywhere;
//   - nothing is written for a sample whose index or column is out of range.
#include "point_rules.h"

namespace {

// PT_LANES lanes per sample: each reads its own value and adds its own word, so the adds of a sample are one contiguous run
__global__ __launch_bounds__(256) void points_merge_kernel(const float* __restrict__ cov, const float* __restrict__ proba,
                                                           const float* __restrict__ xyz, const int* __restrict__ idx,
                                                           const int* __restrict__ n_live, const int* __restrict__ offsets,
                                                           const int* __restrict__ point_index, long sum_n,
                                                           const int* __restrict__ col_base, int B, int N, double diam_meters,
                                                           unsigned long long* __restrict__ acc, int* __restrict__ hits, long T) {
    const long s = ((long)blockIdx.x * 256 + threadIdx.x) / PT_LANES;          // sample = b * N + j
    const int k = threadIdx.x % PT_LANES;
    if (s >= (long)B * N || k > PT_WORDS) return;
    const int b = (int)(s / N), j = (int)(s % N);
    const long col = pt_column(b, j, idx, N, n_live, offsets, point_index, sum_n, col_base, T);
    if (col < 0) return;
    if (k == PT_WORDS) {
        atomicAdd(&hits[col], 1);
        return;
    }
    const float* p = xyz + (size_t)b * 3 * N + j;
    const double w = pt_weight(p[0], p[N], diam_meters);
    const long long t = k == 0 ? pt_fix_weight(w) : pt_fix_value(w, k <= 4 ? cov[(size_t)s * 4 + (k - 1)] : proba[(size_t)s * 4 + (k - 5)]);
    atomicAdd(&acc[pt_word(col, k, T)], (unsigned long long)t);
}

__global__ __launch_bounds__(256) void points_finalize_kernel(const long long* __restrict__ acc, const int* __restrict__ hits, long T,
                                                              float* __restrict__ scores, float* __restrict__ weight) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    const bool hit = hits[i] > 0;
    const long long den = acc[pt_word(i, 0, T)];
#pragma unroll
    for (int k = 1; k < PT_WORDS; ++k)
        scores[(size_t)(k - 1) * T + i] = hit ? pt_score(acc[pt_word(i, k, T)], den) : __builtin_nanf("");
    weight[i] = hit ? pt_total_weight(den) : 0.f;
}
}  // namespace

extern "C" int sn2_points_merge(const float* cov, const float* proba, const float* xyz, const int* idx, const int* n_live,
                                const int* offsets, const int* point_index, long sum_n, const int* col_base, int B, int N,
                                double diam_meters, long long* acc, int* hits, long T, void* stream) {
    if (!cov || !proba || !xyz || !idx || !n_live || !offsets || !point_index || !acc || !hits || B <= 0 || N <= 0 || T <= 0 ||
        sum_n <= 0 || !(diam_meters > 0.0))
        return SN2_EINVAL;
    if (T >= (1L << 31) || sum_n >= (1L << 31) || (long)B * N >= (1L << 31)) return SN2_ELIMIT;
    hipLaunchKernelGGL(points_merge_kernel, dim3(sn2_cdiv((long)B * N * PT_LANES, 256)), dim3(256), 0, (hipStream_t)stream, cov, proba,
                       xyz, idx, n_live, offsets, point_index, sum_n, col_base, B, N, diam_meters,
                       reinterpret_cast<unsigned long long*>(acc), hits, T);
    SN2_RETURN_LAUNCH();
}

extern "C" int sn2_points_finalize(const long long* acc, const int* hits, long T, float* scores, float* weight, void* stream) {
    if (!acc || !hits || !scores || !weight || T <= 0) return SN2_EINVAL;
    if (T >= (1L << 31)) return SN2_ELIMIT;
    hipLaunchKernelGGL(points_finalize_kernel, dim3(sn2_cdiv(T, 256)), dim3(256), 0, (hipStream_t)stream, acc, hits, T, scores, weight);
    SN2_RETURN_LAUNCH();
}
