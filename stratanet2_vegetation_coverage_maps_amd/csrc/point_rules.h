// point_rules.h -- the rule of the per-point scores of a parcel cloud, stated once (the text: include/strata_hip.h, "Per-point
// scores"): which samples of a batch contribute, to which parcel column, with which weight, in which fixed-point unit, where a
// point's nine sums lie, and how they become scores.  csrc/points.hip calls these functions and nothing else decides a byte.
#pragma once
#include "common.h"

constexpr int PT_WORDS = SN2_POINTS_ACC_WORDS;   // int64 sums of a point: [0] the weights, [1..4] coverages, [5..8] probabilities
constexpr int PT_LANES = 16;                      // lanes that share one sample: lane k < 9 adds word k, lane 9 the hit
constexpr double PT_ONE = 4294967296.0;           // 2^32: the unit of the sums

// Where word k of point col lies.  Point-major (a point's nine words side by side: the nine adds of a contribution fall into 72
// contiguous bytes, two cache lines at most) unless the library is built with -DSN2_POINTS_CHANNEL_MAJOR (a timing variant:
// nine planes of T words, every add of a wave instruction in a row of its own).  The bytes of the scores do not depend on it.
__device__ __forceinline__ size_t pt_word(long col, int k, long T) {
#ifdef SN2_POINTS_CHANNEL_MAJOR
    return (size_t)k * (size_t)T + (size_t)col;
#else
    (void)T;
    return (size_t)col * PT_WORDS + (size_t)k;
#endif
}

// The parcel column of sample j of plot b, or -1 when the sample is no contribution: a repeat (j >= n_live[b]), a fake ground
// point or an index outside the plot (c not in [0, n_b)), a plot whose offsets do not lie inside point_index, a column outside
// [0, T).
__device__ __forceinline__ long pt_column(int b, int j, const int* __restrict__ idx, long N, const int* __restrict__ n_live,
                                          const int* __restrict__ offsets, const int* __restrict__ point_index, long sum_n,
                                          const int* __restrict__ col_base, long T) {
    if (j >= n_live[b]) return -1;
    const long o0 = offsets[b], o1 = offsets[b + 1];
    if (o0 < 0 || o1 < o0 || o1 > sum_n) return -1;
    const long c = idx[(size_t)b * N + j];
    if (c < 0 || c >= o1 - o0) return -1;
    const long col = (col_base ? (long)col_base[b] : 0L) + (long)point_index[o0 + c];
    return (col < 0 || col >= T) ? -1 : col;
}

// w = 1.5 - sqrt(dx^2 + dy^2) / diam_meters in fp64: the products of two fp32 values are exact in fp64 and their sum is rounded
// once with or without contraction; the root and the quotient are IEEE-rounded (the build has no fast-math flag).
__device__ __forceinline__ double pt_weight(float dx, float dy, double diam_meters) {
    const double r2 = (double)dx * (double)dx + (double)dy * (double)dy;
    return 1.5 - sqrt(r2) / diam_meters;
}

// the fixed-point terms: round-to-nearest-even of w 2^32 and of w v 2^32
__device__ __forceinline__ long long pt_fix_weight(double w) { return llrint(w * PT_ONE); }
__device__ __forceinline__ long long pt_fix_value(double w, float v) { return llrint(w * (double)v * PT_ONE); }

// finalisation of one point
__device__ __forceinline__ float pt_score(long long num, long long den) { return (float)((double)num / (double)den); }
__device__ __forceinline__ float pt_total_weight(long long den) { return (float)((double)den / PT_ONE); }
