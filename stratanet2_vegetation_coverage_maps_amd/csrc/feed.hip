// feed.hip -- a training batch written straight into the caller's buffers from a plot set that lives on the device: the
// reference's `load_cloud(train=True)` (data_loader/loader.py:73-87: centre, fake ground points, rotate, flip, clipped gaussian
// noise, rescale, subsample) for B plots picked by a device-side id table, with every random draw made on the device from the
// counter-based generator of sn2_subsample.  Host side: hip_ops.train_batch, train_data.ResidentPlots.fill, train_data.EpochFeeder.
//
// Contract and generator layout: include/strata_hip.h, sn2_train_batch.  A plot's rows depend on (seed, epoch, plot id, N) alone.
//   launch 1  train_plots_kernel: one thread per plot -- its key, rotation, flips, FPS starts and ground truth row;
//   [2 .. 5   the subsample of sample.hip with the id table, only when some plot of the SET can have more than N candidates;]
//   last      train_points_kernel: one thread per output point.  A plot with n_b <= N candidates (real plots at N = 32 768 mostly)
//             takes its source index from the cheap branch of the subsample inline: no index row is read.
// The per-point kernel gathers 10 floats and stores 13 per output point in 256-byte wave rows (one dword per lane, coalesced on
// both sides where the source index is the identity): it is bound by memory, the draws (two generator calls and three fp64
// Box-Muller pairs per point) ride beside the loads.
#include "common.h"
#include "philox.h"

namespace {

constexpr double TWO_PI = 6.283185307179586;          // the fp64 nearest 2 pi (numpy's 2 * np.pi)
constexpr double NOISE_SIGMA = 0.1;                   // loader.py:180,202: sigma of x, y AND of the colours
constexpr double NOISE_CLIP_XY = 0.3, NOISE_CLIP_COLOUR = 0.03 * 65536;

// workspace, in 32-bit words: [B] keys (int64) | [B][2] rotation (fp64) | [B][2] flips | [B][N] subsample rows | sn2_subsample's own
__host__ __device__ __forceinline__ size_t head_words(int B) { return 8 * (size_t)B; }
inline size_t idx_words(int B, int n_max, int N) { return n_max > N ? (((size_t)B * N + 3) & ~(size_t)3) : 0; }

__global__ __launch_bounds__(64) void train_plots_kernel(const int* __restrict__ ids, int B, int P,
                                                         const double* __restrict__ coverages, unsigned long long seed,
                                                         long long epoch, int N, int M1, int train,
                                                         const double* __restrict__ cos_sin, int* __restrict__ ws,
                                                         double* __restrict__ gt, int* __restrict__ fps_start,
                                                         const int* __restrict__ offs, int n_fake, int* __restrict__ n_live) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int p = ids[b];
    if (n_live) {                                                 // the distinct rows at the front of the plot (sn2_fps_live)
        const long nc = (long)(offs[p + 1] - offs[p]) + n_fake;
        n_live[b] = nc < N ? (int)nc : N;
    }
    const long long key = epoch * (long long)P + p;
    reinterpret_cast<long long*>(ws)[b] = key;
    double* rot = reinterpret_cast<double*>(ws + 2 * (size_t)B);
    int* flips = ws + 6 * (size_t)B;
#pragma unroll
    for (int k = 0; k < 4; ++k) gt[4 * (size_t)b + k] = coverages[4 * (size_t)p + k];
    unsigned w[4];
    sn2_philox4(seed, key, 1u, 1u, w);
    fps_start[b] = (int)(((unsigned long long)w[0] * (unsigned)N) >> 32);
    fps_start[B + b] = (int)(((unsigned long long)w[1] * (unsigned)M1) >> 32);
    double cs = 1.0, sn = 0.0;
    int fx = 0, fy = 0;
    if (train) {
        sn2_philox4(seed, key, 0u, 1u, w);
        fx = (int)(w[0] >> 31);
        fy = (int)(w[1] >> 31);
        const int angle = (int)(((unsigned long long)w[2] * 360u) >> 32);
        cs = cos_sin[2 * angle];
        sn = cos_sin[2 * angle + 1];
    }
    rot[2 * b] = cs;
    rot[2 * b + 1] = sn;
    flips[2 * b] = fx;
    flips[2 * b + 1] = fy;
}

// one Box-Muller pair from two words: u1 = (wa + 1) 2^-32 in (0, 1], u2 = wb 2^-32
__device__ __forceinline__ void box_muller(unsigned wa, unsigned wb, double& g0, double& g1) {
#pragma clang fp contract(off)
    const double u1 = ((double)wa + 1.0) * 0x1p-32, u2 = (double)wb * 0x1p-32;
    const double r = sqrt(-2.0 * log(u1)), t = TWO_PI * u2;
    g0 = r * cos(t);
    g1 = r * sin(t);
}
__device__ __forceinline__ float noise_term(double g, double clip) {
#pragma clang fp contract(off)
    const double v = NOISE_SIGMA * g;
    return (float)(v < -clip ? -clip : (v > clip ? clip : v));
}

// The arithmetic of prepare_plots_kernel (misc.hip), statement for statement: fp32 throughout, the rotation an fp64 product cast
// back, no contraction.  blockIdx.y = the plot's place in the batch, so everything per plot is a uniform (scalar) load.
__global__ __launch_bounds__(256) void train_points_kernel(const float* __restrict__ raw, long T, const int* __restrict__ offs,
                                                           const float* __restrict__ centers, const int* __restrict__ ids,
                                                           const float* __restrict__ fake_xy, int n_fake, int n_max,
                                                           const int* __restrict__ idx, int N, int train, int noise,
                                                           unsigned long long seed, const int* __restrict__ ws, int B, float z_max,
                                                           float* __restrict__ cloud, float* __restrict__ xyz) {
#pragma clang fp contract(off)
    const int b = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const int p = ids[b];
    const int lo = offs[p], n_raw = offs[p + 1] - lo;
    const long nc = (long)n_raw + n_fake;
    const int n_b = nc > n_max ? n_max : (int)nc;                 // as sample.hip counts a plot's candidates
    const long long key = reinterpret_cast<const long long*>(ws)[b];
    int src;
    if (n_b <= N)                                                 // the cheap branch of sn2_subsample, inline
        src = n < n_b ? n : (n_b > 0 ? (int)__umul64hi(sn2_philox_u(seed, key, (unsigned)n), (unsigned long long)n_b) : 0);
    else
        src = idx[(size_t)b * N + n];
    float v[10];
    if (src < n_raw) {
#pragma unroll
        for (int c = 0; c < 10; ++c) v[c] = raw[(size_t)c * T + lo + src];
        v[0] = v[0] - centers[2 * p];
        v[1] = v[1] - centers[2 * p + 1];
    } else {
        const int k = src - n_raw;
        v[0] = k < n_fake ? fake_xy[2 * k] : 0.f;
        v[1] = k < n_fake ? fake_xy[2 * k + 1] : 0.f;
#pragma unroll
        for (int c = 2; c < 10; ++c) v[c] = 0.f;
    }
    float px = v[0], py = v[1];
    const float pz = v[2];
    if (train) {
        const double* rot = reinterpret_cast<const double*>(ws + 2 * (size_t)B);
        const int* flips = ws + 6 * (size_t)B;
        const double cs = rot[2 * b], sn = rot[2 * b + 1];
        const double rx = (double)v[0] * cs + (double)v[1] * sn, ry = (double)v[0] * (-sn) + (double)v[1] * cs;
        v[0] = px = (float)rx;
        v[1] = py = (float)ry;
        if (flips[2 * b]) { v[0] = -v[0]; px = -px; }
        if (flips[2 * b + 1]) { v[1] = -v[1]; py = -py; }
        if (noise) {                                              // keyed by the SOURCE index: duplicates share their noise
            unsigned w[4];
            double g0, g1, g2, g3;
            sn2_philox4(seed, key, (unsigned)src, 2u, w);
            box_muller(w[0], w[1], g0, g1);
            box_muller(w[2], w[3], g2, g3);
            v[0] += noise_term(g0, NOISE_CLIP_XY);
            v[1] += noise_term(g1, NOISE_CLIP_XY);
            v[3] += noise_term(g2, NOISE_CLIP_COLOUR);
            v[4] += noise_term(g3, NOISE_CLIP_COLOUR);
            sn2_philox4(seed, key, (unsigned)src, 3u, w);
            box_muller(w[0], w[1], g0, g1);
            v[5] += noise_term(g0, NOISE_CLIP_COLOUR);
            v[6] += noise_term(g1, NOISE_CLIP_COLOUR);
        }
    }
    v[0] = v[0] / 10.f;
    v[1] = v[1] / 10.f;
    v[2] = v[2] / z_max;
#pragma unroll
    for (int c = 3; c < 7; ++c) v[c] = v[c] / 65536.f;
    v[7] = v[7] / 32768.f;
    v[8] = (v[8] - 1.f) / 6.f;
    v[9] = (v[9] - 1.f) / 6.f;
#pragma unroll
    for (int c = 0; c < 10; ++c) cloud[((size_t)b * 10 + c) * N + n] = v[c];
    xyz[((size_t)b * 3 + 0) * N + n] = px;
    xyz[((size_t)b * 3 + 1) * N + n] = py;
    xyz[((size_t)b * 3 + 2) * N + n] = pz;
}

}  // namespace

extern "C" int sn2_train_batch_ws_words(int B, int n_max, int N, size_t* words) {
    if (!words || B <= 0 || n_max <= 0 || N <= 0) return SN2_EINVAL;
    *words = head_words(B) + idx_words(B, n_max, N) + (n_max > N ? sn2_subsample_ws_words(B, n_max, N, 0) : 0);
    return 0;
}

extern "C" int sn2_train_batch(const float* raw, long T, const int* offsets, const float* centers, const double* coverages, int P,
                               const int* plot_ids, int B, const float* fake_xy, int n_fake, int n_max, int N, int M1, float z_max,
                               unsigned long long seed, long long epoch, const double* cos_sin, int train, int noise, int* ws,
                               size_t ws_words, float* cloud, float* xyz, double* gt, int* fps_start, void* stream) {
    return sn2_train_batch_live(raw, T, offsets, centers, coverages, P, plot_ids, B, fake_xy, n_fake, n_max, N, M1, z_max, seed, epoch,
                                cos_sin, train, noise, ws, ws_words, cloud, xyz, gt, fps_start, nullptr, stream);
}

extern "C" int sn2_train_batch_live(const float* raw, long T, const int* offsets, const float* centers, const double* coverages, int P,
                                    const int* plot_ids, int B, const float* fake_xy, int n_fake, int n_max, int N, int M1,
                                    float z_max, unsigned long long seed, long long epoch, const double* cos_sin, int train,
                                    int noise, int* ws, size_t ws_words, float* cloud, float* xyz, double* gt, int* fps_start,
                                    int* n_live, void* stream) {
    if (!raw || !offsets || !centers || !coverages || !plot_ids || !cloud || !xyz || !gt || !fps_start) return SN2_EINVAL;
    if (B <= 0 || N <= 0 || P <= 0 || T <= 0 || M1 <= 0 || n_fake < 0 || n_max <= 0 || epoch < 0 || !(z_max > 0.f)) return SN2_EINVAL;
    if (n_fake > 0 && !fake_xy) return SN2_EINVAL;
    if (train && !cos_sin) return SN2_EINVAL;
    if (T >= (1L << 31) || B > 65535) return SN2_ELIMIT;
    size_t need = 0;
    SN2_TRY(sn2_train_batch_ws_words(B, n_max, N, &need));
    if (!ws || ((uintptr_t)ws & 15) || ws_words < need) return SN2_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(train_plots_kernel, dim3(sn2_cdiv(B, 64)), dim3(64), 0, st, plot_ids, B, P, coverages, seed, epoch, N, M1,
                       train, cos_sin, ws, gt, fps_start, offsets, n_fake, n_live);
    int* idx = nullptr;
    if (n_max > N) {
        idx = ws + head_words(B);
        int* sub_ws = idx + idx_words(B, n_max, N);
        const size_t sub_words = sn2_subsample_ws_words(B, n_max, N, 0);
        SN2_TRY(sn2_subsample_ids(offsets, plot_ids, n_fake, n_max, B, N, seed, reinterpret_cast<const long long*>(ws), 0,
                                  sub_words ? sub_ws : nullptr, sub_words, idx, st));
    }
    hipLaunchKernelGGL(train_points_kernel, dim3(sn2_cdiv(N, 256), B), dim3(256), 0, st, raw, T, offsets, centers, plot_ids, fake_xy,
                       n_fake, n_max, idx, N, train, train && noise, seed, ws, B, z_max, cloud, xyz);
    SN2_RETURN_LAUNCH();
}
