// indicators.hip -- the cross-validation report (include/strata_hip.h: sn2_cv_indicators): the per-plot performance indicators of
// learning/accuracy.py (calculate_performance_indicators_V1/V2/V3), the class indices of its confusion matrices
// (compute_confusion_matrix, adjust_predictions_based_on_margin) and their sums, from the (P,4) plot-wise predictions and ground
// truths that a validation pass leaves on the device.
//   launch 1  one workgroup per slice of CV_SLICE plots, one thread per plot: the plot's row and classes (they depend on that plot
//             alone), then the slice's column sums (NaN entries left out and counted out), a fixed butterfly inside a wave, the
//             sixteen waves added in wave order by one thread per column; the slice's confusion counts in integer LDS atomics.
//             Everything a slice found goes to ITS block of the workspace: no global atomics, nothing to clear.
//   launch 2  one workgroup, one thread per entry of `stats`: the sum of that entry over the slices in ascending order.
// All arithmetic is fp64, every expression one operation (no product feeds a sum: nothing to contract; the pragma says so too).
#include "common.h"

namespace {
constexpr int CV_SLICE = SN2_CV_SLICE_PLOTS;
constexpr int CV_COLS = SN2_CV_COLUMNS;
constexpr int CV_CM = 2 * 3 * 8 * 8;
// a slice's block of the workspace, in 32-bit words: CV_COLS fp64 sums, CV_COLS counts + the continuous-row count + a pad, the counts
constexpr int CV_WS_SUMS = 0, CV_WS_COUNTS = 2 * CV_COLS, CV_WS_CM = CV_WS_COUNTS + CV_COLS + 2, CV_WS_SLICE = CV_WS_CM + CV_CM;
static_assert(CV_WS_SLICE == SN2_CV_WS_SLICE_WORDS && CV_WS_SLICE % 2 == 0, "workspace layout");
static_assert(SN2_CV_STATS_DOUBLES == 2 * CV_COLS + CV_CM + 1, "stats layout");
static_assert(CV_SLICE == 1024, "one thread per plot of a slice");

// learning/accuracy.py:13-42: the class centres and the borders [lo, hi] of each class, the doubles nearest these literals
__device__ const double CV_C[8] = {0.0, 0.10, 0.25, 0.33, 0.50, 0.75, 0.90, 1.0};
__device__ const double CV_LO[8] = {0.0, 0.05, 0.18, 0.29, 0.42, 0.63, 0.83, 0.95};
__device__ const double CV_HI[8] = {0.05, 0.18, 0.29, 0.42, 0.63, 0.83, 0.95, 1.05};
constexpr double CV_MARGIN = 0.1;

// get_closest_class_center_index: the FIRST k that minimises |c[k] - y| (an exact tie: the lower class; all NaN: 0)
__device__ __forceinline__ int cv_closest(double y) {
#pragma clang fp contract(off)
    double best = fabs(CV_C[0] - y);
    int k = 0;
#pragma unroll
    for (int j = 1; j < 8; ++j) {
        const double d = fabs(CV_C[j] - y);
        if (d < best) best = d, k = j;
    }
    return k;
}

// 0 inside [lo, hi], else the distance to the nearer border (compute_mae2 / compute_mae3)
__device__ __forceinline__ double cv_outside(double lo, double hi, double p, bool inside) {
#pragma clang fp contract(off)
    return inside ? 0.0 : fmin(fabs(lo - p), fabs(hi - p));
}

__device__ __forceinline__ double cv_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int cv_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(CV_SLICE) void cv_rows_kernel(const float4* __restrict__ pred, const double* __restrict__ gt, int P,
                                                           int relabel, double* __restrict__ rows, int* __restrict__ cls,
                                                           int* __restrict__ ws) {
#pragma clang fp contract(off)
    __shared__ double s_sum[CV_SLICE / 64][CV_COLS];
    __shared__ int s_cnt[CV_SLICE / 64][CV_COLS + 1];
    __shared__ int s_cm[CV_CM];
    const int t = threadIdx.x, w = t >> 6;
    const int p_id = blockIdx.x * CV_SLICE + t;
    const bool live = p_id < P;
    for (int i = t; i < CV_CM; i += CV_SLICE) s_cm[i] = 0;
    __syncthreads();

    double v[CV_COLS] = {};
    int bad = 0;
    if (live) {
        const float4 pf = pred[p_id];
        const double pr[3] = {(double)pf.x, (double)pf.z, (double)pf.w};                     // strata = columns 0, 2, 3
        const double gr[3] = {gt[4 * (size_t)p_id], gt[4 * (size_t)p_id + 2], gt[4 * (size_t)p_id + 3]};
        double err[3], err2[3], err3[3], acc[3], acc2[3], acc3[3];
        int c_true[3], c_pred[3], c_adj[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const double p = pr[s];
            double g = gr[s];
            if (relabel) g = CV_C[cv_closest(g)];                                             // main.py:102-109
            const double g1000 = g * 1000.0;
            g = rint(g1000) / 1000.0;                                                         // .round(3)
            int k = -1;                                                                       // kt
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (g == CV_C[j]) k = j;
            if (k < 0) bad = 1;
            const int kk = k < 0 ? 0 : k;                                                     // (a continuous row is overwritten below)
            const double lo = CV_LO[kk], hi = CV_HI[kk];
            const double lo2 = lo - CV_MARGIN, hi2 = hi + CV_MARGIN;
            const double L = CV_LO[kk > 0 ? kk - 1 : 0], H = CV_HI[kk < 7 ? kk + 1 : 7];
            const bool a1 = lo <= p && p <= hi, a2 = lo2 <= p && p <= hi2, a3 = L <= p && p <= H;
            err[s] = fabs(p - g);
            acc[s] = a1 ? 1.0 : 0.0;
            err2[s] = cv_outside(lo, hi, p, a1);
            acc2[s] = a2 ? 1.0 : 0.0;
            err3[s] = cv_outside(L, H, p, a3);
            acc3[s] = a3 ? 1.0 : 0.0;
            c_true[s] = cv_closest(g);
            c_pred[s] = cv_closest(p);
        }
#pragma unroll
        for (int s = 0; s < 3; ++s)                                                           // adjust_predictions_based_on_margin
            c_adj[s] = (!bad && acc2[s] == 1.0) ? c_true[s] : c_pred[s];
        // V1 | V2 | V3, each: the three strata, b_and_moy, all -- errors, then accuracies
        v[0] = err[0], v[1] = err[1], v[2] = err[2];
        v[3] = (err[0] + err[1]) / 2.0;
        v[4] = ((err[0] + err[1]) + err[2]) / 3.0;
        v[5] = acc[0], v[6] = acc[1], v[7] = acc[2];
        v[8] = (acc[0] + acc[1]) / 2.0;
        v[9] = (acc[0] + acc[1]) / 2.0;                                                       // accuracy.py:169: acc_all over TWO strata
        v[10] = err2[0], v[11] = err2[1], v[12] = err2[2];
        v[13] = (err2[0] + err2[1]) / 2.0;
        v[14] = ((err2[0] + err2[1]) + err2[2]) / 3.0;
        v[15] = acc2[0], v[16] = acc2[1], v[17] = acc2[2];
        v[18] = (acc2[0] + acc2[1]) / 2.0;
        v[19] = ((acc2[0] + acc2[1]) + acc2[2]) / 3.0;
        v[20] = err3[0], v[21] = err3[1], v[22] = err3[2];
        v[23] = (err3[0] + err3[1]) / 2.0;
        v[24] = ((err3[0] + err2[1]) + err3[2]) / 3.0;                                        // accuracy.py:242: error2_veg_moy
        v[25] = acc3[0], v[26] = acc3[1], v[27] = acc3[2];
        v[28] = (acc3[0] + acc3[1]) / 2.0;
        v[29] = ((acc3[0] + acc3[1]) + acc3[2]) / 3.0;
        if (bad) {                                                                            // the reference raises KeyError here
            const double nan = __longlong_as_double(0x7FF8000000000000LL);
#pragma unroll
            for (int c = 5; c < CV_COLS; ++c) v[c] = nan;
        }
        double2* r2 = reinterpret_cast<double2*>(rows + (size_t)p_id * CV_COLS);              // 240-byte rows: 16-byte aligned
#pragma unroll
        for (int c = 0; c < CV_COLS / 2; ++c) r2[c] = make_double2(v[2 * c], v[2 * c + 1]);
        int* cp = cls + (size_t)p_id * 9;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            cp[s] = c_true[s], cp[3 + s] = c_pred[s], cp[6 + s] = c_adj[s];
            atomicAdd(&s_cm[(s * 8 + c_true[s]) * 8 + c_pred[s]], 1);
            atomicAdd(&s_cm[((3 + s) * 8 + c_true[s]) * 8 + c_adj[s]], 1);
        }
    }
    // the slice's sums: a NaN entry (and a thread past P) adds 0 to the sum and 0 to the count
#pragma unroll
    for (int c = 0; c < CV_COLS; ++c) {
        const bool in = live && v[c] == v[c];
        const double sum = cv_wave_sum(in ? v[c] : 0.0);
        const int cnt = cv_wave_sum(in ? 1 : 0);
        if ((t & 63) == 0) s_sum[w][c] = sum, s_cnt[w][c] = cnt;
    }
    {
        const int nb = cv_wave_sum(live ? bad : 0);
        if ((t & 63) == 0) s_cnt[w][CV_COLS] = nb;
    }
    __syncthreads();
    int* my = ws + (size_t)blockIdx.x * CV_WS_SLICE;
    if (t < CV_COLS) {
        double a = 0.0;
        for (int k = 0; k < CV_SLICE / 64; ++k) a += s_sum[k][t];
        reinterpret_cast<double*>(my + CV_WS_SUMS)[t] = a;
    }
    if (t <= CV_COLS + 1) {                                                                   // the counts, the continuous rows, the pad
        int n = 0;
        if (t <= CV_COLS)
            for (int k = 0; k < CV_SLICE / 64; ++k) n += s_cnt[k][t];
        my[CV_WS_COUNTS + t] = n;
    }
    for (int i = t; i < CV_CM; i += CV_SLICE) my[CV_WS_CM + i] = s_cm[i];
}

// stats: sum[CV_COLS], count[CV_COLS], the confusion counts (2,3,8,8), the continuous rows -- one thread per entry adds the slices'
// entries in ascending slice order (integers as integers: exact).  CV_STATS_AHEAD loads are issued before their adds: the order of
// the additions is the ascending one, only the latency of a chain of dependent global loads is gone (a million plots: 977 slices).
constexpr int CV_STATS_AHEAD = 16;

template <typename T, typename A>
__device__ __forceinline__ A cv_sum_slices(const T* __restrict__ src, int slices, size_t stride) {
#pragma clang fp contract(off)
    A a = 0;
    int s = 0;
    for (; s + CV_STATS_AHEAD <= slices; s += CV_STATS_AHEAD) {
        T v[CV_STATS_AHEAD];
#pragma unroll
        for (int j = 0; j < CV_STATS_AHEAD; ++j) v[j] = src[(size_t)(s + j) * stride];
#pragma unroll
        for (int j = 0; j < CV_STATS_AHEAD; ++j) a += v[j];
    }
    for (; s < slices; ++s) a += src[(size_t)s * stride];
    return a;
}

__global__ __launch_bounds__(512) void cv_stats_kernel(const int* __restrict__ ws, int slices, double* __restrict__ stats) {
    static_assert(SN2_CV_STATS_DOUBLES <= 512, "one thread per entry");
    const int e = threadIdx.x;
    if (e >= SN2_CV_STATS_DOUBLES) return;
    if (e < CV_COLS) {
        stats[e] = cv_sum_slices<double, double>(reinterpret_cast<const double*>(ws + CV_WS_SUMS) + e, slices, CV_WS_SLICE / 2);
    } else {
        // count c -> word CV_WS_COUNTS + c; confusion i -> CV_WS_CM + i; the continuous rows -> CV_WS_COUNTS + CV_COLS
        const int word = e < 2 * CV_COLS ? CV_WS_COUNTS + (e - CV_COLS)
                         : e < 2 * CV_COLS + CV_CM ? CV_WS_CM + (e - 2 * CV_COLS) : CV_WS_COUNTS + CV_COLS;
        stats[e] = (double)cv_sum_slices<int, long long>(ws + word, slices, CV_WS_SLICE);
    }
}
}  // namespace

extern "C" int sn2_cv_indicators_ws_words(int P, size_t* words) {
    if (!words) return SN2_EINVAL;
    *words = 0;
    if (P < 1) return SN2_EINVAL;
    if (P > SN2_CV_MAX_PLOTS) return SN2_ELIMIT;
    *words = SN2_CV_WS_WORDS(P);
    return 0;
}

extern "C" int sn2_cv_indicators(const float* pred, const double* gt, int P, int relabel, double* rows, int* cls, double* stats,
                                 void* ws, void* stream) {
    if (!pred || !gt || !rows || !cls || !stats || !ws || P < 1) return SN2_EINVAL;
    if ((((uintptr_t)pred | (uintptr_t)rows) & 15) != 0 || (((uintptr_t)ws | (uintptr_t)gt | (uintptr_t)stats) & 7) != 0) return SN2_EINVAL;
    if (P > SN2_CV_MAX_PLOTS) return SN2_ELIMIT;
    hipStream_t st = (hipStream_t)stream;
    const int slices = (int)SN2_CV_SLICES(P);
    hipLaunchKernelGGL(cv_rows_kernel, dim3(slices), dim3(CV_SLICE), 0, st, reinterpret_cast<const float4*>(pred), gt, P,
                       relabel ? 1 : 0, rows, cls, (int*)ws);
    hipLaunchKernelGGL(cv_stats_kernel, dim3(1), dim3(512), 0, st, (const int*)ws, slices, stats);
    SN2_RETURN_LAUNCH();
}
