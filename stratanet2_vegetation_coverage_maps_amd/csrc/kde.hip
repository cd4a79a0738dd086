// kde.hip -- fitting the KDE mixture of the NLL loss: KdeMixture.fit + evaluate_kdes (learning/kde_mixture.py:50-100), three
// weighted Gaussian KDEs over the symmetrised heights {-z} u {z}, evaluated on one equidistant grid and divided by their common
// maximum.  The reference fits with KDEpy's FFTKDE = linear binning + a convolution with the sampled kernel; the estimator is
// written out in include/strata_hip.h (sn2_kde_fit) and restated in numpy in tests/test_kde_fit_host.py.
//
// Four or five launches on the caller's stream, nothing read back in between:
//   1 kde_absmax_kernel  per-workgroup maxima of |z| (a maximum does not depend on the order it is taken in);
//   2 kde_bin_kernel     the grid X, the Gaussian taps and the linear binning.  A workgroup OWNS BIN_ROWS consecutive bins and
//                        scans ALL heights: thread t takes heights t, t + 256, ... in that order and adds the ones that touch an
//                        owned bin onto accumulators of its own (LDS, one column per thread: no atomics), and the 256 columns are
//                        added in a fixed tree.  So a bin's sum is a fixed expression of the input: the same bytes every call,
//                        whatever the scheduling -- and no float atomic meets the ~45 bins that hold 40 % of real heights.
//                        The price is that every workgroup reads every height (2 MB out of L2 at n = 5e5, 625 times at K = 5000);
//                        a height is tested against the workgroup's z range before anything is computed for it.
//                        Heights pile up (55 % of the synthetic mixture lands in ~24 bins, i.e. in three workgroups, which then
//                        run ~100 times longer than the rest), so the heights are cut into up to SN2_KDE_FIT_SLICES slices --
//                        blockIdx.y, a function of n alone -- each with a bin table of its own, and kde_slices_kernel adds the
//                        slices' tables in ascending order.
//                        Both signs of a height are binned as they stand: t(-z) is NOT the mirror image of t(z) in floating
//                        point, and the tables are held to the restated estimator term by term.
//   3 kde_conv_kernel    "same"-sized convolution with the taps, zero outside the grid, and per-workgroup maxima;
//   4 kde_norm_kernel    division by the maximum over the three tables.
// Every fp64 operation that decides a bin index or a fraction is done unfused, in the order the header writes it.
#include "common.h"

#include <math.h>

namespace {

constexpr int BIN_ROWS = 8;                        // bins a workgroup of kde_bin_kernel owns: 8 * 3 * 256 doubles = 48 KB of LDS
constexpr int SCAN = 8;                            // heights a thread of kde_bin_kernel fetches before it tests them
constexpr int ABS_SLOTS = SN2_KDE_FIT_ABS_SLOTS;   // workgroups of kde_absmax_kernel at most = threads of its consumers

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// max over a block of 256 threads, the same value in every thread
__device__ __forceinline__ double block_max_f64(double v, double* s4) {
    v = wave_max_f64(v);
    __syncthreads();                               // s4 may still be read from an earlier call
    if (lane_id() == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(s4[0], s4[1]), fmax(s4[2], s4[3]));
}

__global__ __launch_bounds__(256) void kde_absmax_kernel(const float* __restrict__ z, long n, float* __restrict__ part) {
    __shared__ double s4[4];
    float m = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) m = fmaxf(m, fabsf(z[i]));
    const double bm = block_max_f64((double)m, s4);
    if (threadIdx.x == 0) part[blockIdx.x] = (float)bm;
}

struct kde_grid {
    double A, dx;                                  // X = linspace(-A, A, K), dx = 2A / (K-1)
    int L;                                         // the kernel is sampled at -L*dx .. L*dx
};

// every workgroup derives the grid from the partial maxima itself: the same operations, so the same bits, everywhere
__device__ __forceinline__ kde_grid kde_make_grid(const float* __restrict__ part, int nparts, double bw, int K, double* s4) {
#pragma clang fp contract(off)
    const double zm = block_max_f64((int)threadIdx.x < nparts ? (double)part[threadIdx.x] : 0.0, s4);
    kde_grid g;
    const double margin = (0.05 * 2.0) * zm, reach = 5.0 * bw;
    g.A = zm + (margin > reach ? margin : reach);
    g.dx = (2.0 * g.A) / (double)(K - 1);
    const double l = floor(reach / g.dx);          // A >= 5 bw, so l <= (K-1)/2
    g.L = l < (double)(K - 1) ? (int)l : K - 1;
    return g;
}

__global__ __launch_bounds__(256) void kde_bin_kernel(const float* __restrict__ z, long n_all, long slice, const float* __restrict__ part,
                                                      int nparts, double bw, double gnorm, int K, double* __restrict__ X,
                                                      double* __restrict__ bins, double* __restrict__ taps) {
#pragma clang fp contract(off)
    __shared__ double acc[BIN_ROWS * 3][256];      // [owned bin * 3 + table][thread]: a thread touches its own column only
    __shared__ double s4[4];
    const int tid = threadIdx.x;
    const kde_grid G = kde_make_grid(part, nparts, bw, K, s4);
    const double X0 = -G.A, dx = G.dx;
    const int j0 = blockIdx.x * BIN_ROWS;
    z += (long)blockIdx.y * slice;                 // this workgroup's slice of the heights, and its bin table
    bins += (size_t)blockIdx.y * 3 * K;
    const long n = n_all - (long)blockIdx.y * slice < slice ? n_all - (long)blockIdx.y * slice : slice;
    if (blockIdx.y == 0 && tid < BIN_ROWS && j0 + tid < K) {          // this slice of the grid and of the taps (tap j is read for j <= L only)
        const int j = j0 + tid;
        X[j] = j == K - 1 ? G.A : (double)j * dx + X0;
        const double u = (double)j * dx;
        taps[j] = exp(-(u * u) / (2.0 * (bw * bw))) / gnorm;
    }
#pragma unroll
    for (int s = 0; s < BIN_ROWS * 3; ++s) acc[s][tid] = 0.0;
    // a sample point s touches an owned bin iff floor(t) is in [j0-1, j0+BIN_ROWS-1].  The test in z is one grid step wider on each
    // side than that (t is off from (s - X0)/dx by rounding only) and rounded outwards to fp32, which a height converts to exactly;
    // the owned-bin test below is exact.  SCAN heights are fetched ahead of their tests: the loop is bound by the latency of its
    // loads, not by their number.  A slot past the end holds NaN, which passes no test.
    const float lo = __double2float_rd((double)(j0 - 2) * dx + X0), hi = __double2float_ru((double)(j0 + BIN_ROWS + 1) * dx + X0);
    for (long base = 0; base < n; base += 256 * SCAN) {
        float zs[SCAN];
#pragma unroll
        for (int u = 0; u < SCAN; ++u) {
            const long i = base + u * 256 + tid;
            zs[u] = i < n ? z[i] : __int_as_float(0x7fc00000);
        }
#pragma unroll
        for (int u = 0; u < SCAN; ++u) {
            const float zf = zs[u];
            if (!((zf >= lo && zf <= hi) || (-zf >= lo && -zf <= hi))) continue;
            const double zi = (double)zf, a = fabs(zi);
            const double w1 = a < 0.5 ? 1.0 : 0.05;
            const double w2 = (0.5 < a && a < 1.5) ? 1.0 : 0.05;
            const double w3 = 1.5 < a ? 1.0 : (0.5 < a ? 0.5 : 0.05);
            for (int sg = 0; sg < 2; ++sg) {       // +z, then -z
                const double s = sg ? -zi : zi;
                const double t = (s - X0) / dx;
                const double ft = floor(t);
                const int j = ft < (double)(K - 2) ? (int)ft : K - 2;
                const double f = t - (double)j;
                const double g = 1.0 - f;
                const unsigned r0 = (unsigned)(j - j0), r1 = (unsigned)(j + 1 - j0);
                if (r0 < (unsigned)BIN_ROWS) {
                    acc[r0 * 3 + 0][tid] += w1 * g;
                    acc[r0 * 3 + 1][tid] += w2 * g;
                    acc[r0 * 3 + 2][tid] += w3 * g;
                }
                if (r1 < (unsigned)BIN_ROWS) {
                    acc[r1 * 3 + 0][tid] += w1 * f;
                    acc[r1 * 3 + 1][tid] += w2 * f;
                    acc[r1 * 3 + 2][tid] += w3 * f;
                }
            }
        }
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int s = wave; s < BIN_ROWS * 3; s += 4) {
        double v = (acc[s][lane] + acc[s][lane + 64]) + (acc[s][lane + 128] + acc[s][lane + 192]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        const int j = j0 + s / 3;
        if (lane == 0 && j < K) bins[(size_t)(s % 3) * K + j] = v;
    }
}

// bins (3K) = the slices' tables added in ascending order
__global__ __launch_bounds__(256) void kde_slices_kernel(const double* __restrict__ sliced, int slices, int total,
                                                         double* __restrict__ bins) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    double v = sliced[i];
    for (int s = 1; s < slices; ++s) v += sliced[(size_t)s * total + i];
    bins[i] = v;
}

// blockIdx.y = table.  Y[k][i] = sum_{d = -L..L, 0 <= i+d < K} bins[k][i+d] * taps[|d|], d ascending; pmax: one slot per workgroup
__global__ __launch_bounds__(256) void kde_conv_kernel(const float* __restrict__ part, int nparts, double bw, int K,
                                                       const double* __restrict__ bins, const double* __restrict__ taps,
                                                       double* __restrict__ Y, double* __restrict__ pmax) {
#pragma clang fp contract(off)
    __shared__ double s4[4];
    const kde_grid G = kde_make_grid(part, nparts, bw, K, s4);
    const int i = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    double v = 0.0;
    if (i < K) {
        const double* __restrict__ b = bins + (size_t)k * K;
        const int d0 = G.L < i ? -G.L : -i, d1 = G.L < K - 1 - i ? G.L : K - 1 - i;
        for (int d = d0; d <= d1; ++d) v += b[i + d] * taps[d < 0 ? -d : d];
        Y[(size_t)k * K + i] = v;
    }
    const double m = block_max_f64(v, s4);
    if (threadIdx.x == 0) pmax[blockIdx.y * gridDim.x + blockIdx.x] = m;
}

__global__ __launch_bounds__(256) void kde_norm_kernel(double* __restrict__ Y, int total, const double* __restrict__ pmax, int np) {
    __shared__ double s4[4];
    double m = 0.0;
    for (int p = threadIdx.x; p < np; p += 256) m = fmax(m, pmax[p]);
    m = block_max_f64(m, s4);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < total) Y[i] = Y[i] / m;
}

}  // namespace

extern "C" size_t sn2_kde_fit_ws_words(int K) { return SN2_KDE_FIT_WS_WORDS(K); }

extern "C" int sn2_kde_fit(const float* z, long n, double bw, int K, void* ws, double* X, double* Y, void* stream) {
    if (!z || !ws || !X || !Y || n <= 0 || K < 2 || !(bw > 0.0) || !(bw <= 1.7e308) || ((uintptr_t)ws & 7)) return SN2_EINVAL;
    if (n > 0x7fffffffL || K > SN2_KDE_FIT_MAX_K) return SN2_ELIMIT;
    hipStream_t st = (hipStream_t)stream;
    const int conv_blocks = sn2_cdiv(K, 256);
    double* bins = (double*)ws;                    // (3,K)
    double* taps = bins + 3 * (size_t)K;           // (K)
    double* pmax = taps + K;                       // (3 * conv_blocks)
    double* sliced = pmax + 3 * conv_blocks;       // (SN2_KDE_FIT_SLICES,3,K)
    float* part = (float*)(sliced + (size_t)SN2_KDE_FIT_SLICES * 3 * K);  // (ABS_SLOTS)
    int nparts = sn2_cdiv(n, 2048);
    nparts = nparts < 1 ? 1 : (nparts > ABS_SLOTS ? ABS_SLOTS : nparts);
    // slices of the heights: a function of n alone (the tables' bytes depend on it), whole SCAN rounds of a workgroup each
    int slices = sn2_cdiv(n, 16 * 256 * SCAN);
    slices = slices < 1 ? 1 : (slices > SN2_KDE_FIT_SLICES ? SN2_KDE_FIT_SLICES : slices);
    const long slice = (long)sn2_cdiv(sn2_cdiv(n, slices), 256 * SCAN) * (256 * SCAN);
    slices = sn2_cdiv(n, slice);
    const double gnorm = bw * sqrt(2.0 * M_PI);
    hipLaunchKernelGGL(kde_absmax_kernel, dim3(nparts), dim3(256), 0, st, z, n, part);
    hipLaunchKernelGGL(kde_bin_kernel, dim3(sn2_cdiv(K, BIN_ROWS), slices), dim3(256), 0, st, z, n, slice, part, nparts, bw, gnorm,
                       K, X, slices > 1 ? sliced : bins, taps);
    if (slices > 1)
        hipLaunchKernelGGL(kde_slices_kernel, dim3(sn2_cdiv(3L * K, 256)), dim3(256), 0, st, sliced, slices, 3 * K, bins);
    hipLaunchKernelGGL(kde_conv_kernel, dim3(conv_blocks, 3), dim3(256), 0, st, part, nparts, bw, K, bins, taps, Y, pmax);
    hipLaunchKernelGGL(kde_norm_kernel, dim3(sn2_cdiv(3L * K, 256)), dim3(256), 0, st, Y, 3 * K, pmax, 3 * conv_blocks);
    SN2_RETURN_LAUNCH();
}
