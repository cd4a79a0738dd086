// project.hip -- scatter-max projections of pointwise coverages onto 2D rasters.
// Replaces /root/reference/model/project_to_2d.py: project_to_plotwise_coverages (:7-55, torch.unique + torch_scatter
// scatter_max/scatter_mean with per-plot device<->CPU bounces) and project_to_2d_rasters (:58-113, a python loop over
// pixels).  Both become: pixel id per point (index arithmetic operation-for-operation in fp32 -- the ids must be
// bit-exact), a 64-bit max per (pixel, channel) over the key (ordered(value) << 32 | ~point), i.e. largest value, FIRST
// point on ties as torch_scatter's CPU loop -- LDS atomics per workgroup slice, then one global atomic per touched
// pixel -- and a tiny per-plot finalisation.  HBM-bound: 8 B (xy) + 16 B (coverages) read per point.
#include "common.h"
#include "loss_rules.h"
#include "mosaic_rules.h"
#include "projection_rules.h"

namespace {

constexpr int MAX_CELLS = PL_MAX_CELLS;  // diam_pix <= 45: the D*D*3 keys of a workgroup fit the default 48 KiB dynamic LDS

// (the pixel of a point, the key, the scatter of a slice and the finalisation of a plot: projection_rules.h)

// also clears the plot's (pixel, channel) key table for the scatter kernel that follows (see sn2_fill_words in common.h
// for why this is not a hipMemsetAsync)
__global__ __launch_bounds__(1024) void plot_minmax_kernel(const float* __restrict__ xy, long plot_stride, int N,
                                                           float* __restrict__ mm, unsigned long long* __restrict__ keys,
                                                           int ncell3) {
    __shared__ float s[4][16];
    const int b = blockIdx.x;
    for (int i = threadIdx.x; i < ncell3; i += 1024) keys[(size_t)b * ncell3 + i] = 0ull;
    const float* x = xy + (size_t)b * plot_stride;
    const float* y = x + N;
    float xmn = INFINITY, xmx = -INFINITY, ymn = INFINITY, ymx = -INFINITY;
    int i = threadIdx.x;
    for (; i + 7 * 1024 < N; i += 8 * 1024) {        // sixteen independent loads in flight
        float a[8], c[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] = x[i + u * 1024], c[u] = y[i + u * 1024];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            xmn = fminf(xmn, a[u]);
            xmx = fmaxf(xmx, a[u]);
            ymn = fminf(ymn, c[u]);
            ymx = fmaxf(ymx, c[u]);
        }
    }
    for (; i < N; i += 1024) {
        const float a = x[i], c = y[i];
        xmn = fminf(xmn, a);
        xmx = fmaxf(xmx, a);
        ymn = fminf(ymn, c);
        ymx = fmaxf(ymx, c);
    }
    xmn = wave_min(xmn);
    xmx = wave_max(xmx);
    ymn = wave_min(ymn);
    ymx = wave_max(ymx);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s[0][w] = xmn;
        s[1][w] = xmx;
        s[2][w] = ymn;
        s[3][w] = ymx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 16; ++k) {
            xmn = fminf(xmn, s[0][k]);
            xmx = fmaxf(xmx, s[1][k]);
            ymn = fminf(ymn, s[2][k]);
            ymx = fmaxf(ymx, s[3][k]);
        }
        mm[b * 4 + 0] = xmn;
        mm[b * 4 + 1] = xmx;
        mm[b * 4 + 2] = ymn;
        mm[b * 4 + 3] = ymx;
    }
}

// MODE 0: P2 grid (bbox-normalised, cell = x_pix*D + y_pix).  MODE 1: P1 grid (fixed, cell = y_pix*D + x_pix).
template <int MODE>
__global__ __launch_bounds__(1024) void scatter_max_kernel(const float* __restrict__ vals, const float* __restrict__ xy,
                                                           long plot_stride, int N, int D, const float* __restrict__ mm,
                                                           float sf, float off, unsigned long long* __restrict__ keys,
                                                           int* __restrict__ pix) {
    extern __shared__ unsigned long long s_keys[];  // D*D*3
    const int b = blockIdx.y;
    const int ncell3 = D * D * 3;
    pj_clear(s_keys, ncell3);
    __syncthreads();
    const float* x = xy + (size_t)b * plot_stride;
    const float* y = x + N;
    float xmn = 0.f, xmx = 0.f, ymn = 0.f, ymx = 0.f;
    if (MODE == 0) {
        xmn = mm[b * 4 + 0];
        xmx = mm[b * 4 + 1];
        ymn = mm[b * 4 + 2];
        ymx = mm[b * 4 + 3];
    }
    int lo, hi;
    pj_slice(N, gridDim.x, blockIdx.x, lo, hi);
    for (int n = lo + threadIdx.x; n < hi; n += 1024) {
        int cell;
        if (MODE == 0) {
            cell = p2_pix(x[n], xmn, xmx, D) * D + p2_pix(y[n], ymn, ymx, D);
        } else {
            cell = p1_pix(y[n], sf, off, D) * D + p1_pix(x[n], sf, off, D);
        }
        pix[(size_t)b * N + n] = cell;
        pj_push(s_keys, cell, reinterpret_cast<const float4*>(vals)[(size_t)b * N + n], n);
    }
    __syncthreads();
    pj_copy_out<true>(s_keys, ncell3, keys + (size_t)b * ncell3);
}

// The pixel id of every point depends on the plot's x, y only (project_to_2d.py:16-22): a training loop that runs its
// position-only kernels ahead of the feature pass computes them there (sn2_plot_pixels) and the feature pass keeps two
// launches: this scatter from the stored ids and the finalisation.  No key table to clear and no global atomics: the
// `gridDim.x` slices of a plot each write their own table, the finalisation takes the maximum over the slices (same keys,
// same winner: the maximum of maxima).
__global__ __launch_bounds__(1024) void plot_pixels_kernel(const float* __restrict__ xy, long plot_stride, int N, int D,
                                                           const float* __restrict__ mm, int* __restrict__ pix) {
    const int b = blockIdx.y;
    const float* x = xy + (size_t)b * plot_stride;
    const float* y = x + N;
    const float xmn = mm[b * 4 + 0], xmx = mm[b * 4 + 1], ymn = mm[b * 4 + 2], ymx = mm[b * 4 + 3];
    int lo, hi;
    pj_slice(N, gridDim.x, blockIdx.x, lo, hi);
    for (int n = lo + threadIdx.x; n < hi; n += 1024) pix[(size_t)b * N + n] = p2_pix(x[n], xmn, xmx, D) * D + p2_pix(y[n], ymn, ymx, D);
}

__global__ __launch_bounds__(1024) void scatter_max_pix_kernel(const float* __restrict__ vals, const int* __restrict__ pix, int N,
                                                               int D, unsigned long long* __restrict__ keys_part) {
    extern __shared__ unsigned long long s_keys[];  // D*D*3
    pj_scatter_slice(s_keys, vals, pix, N, D, blockIdx.y, gridDim.x, blockIdx.x, keys_part);
}

// P2: pred[b] = mean over occupied pixels of [low, 1-low, med, high]   (project_to_2d.py:41-53)
// parts: key tables per plot (1 = the table the global atomics of scatter_max_kernel<0> filled; more: the slices of
// scatter_max_pix_kernel, of which the maximum is taken here)
__global__ __launch_bounds__(256) void p2_finalize_kernel(const unsigned long long* __restrict__ keys, int D, int parts,
                                                          int* __restrict__ arg, int* __restrict__ nocc,
                                                          float* __restrict__ pred) {
    __shared__ float s[5][4];
    const int b = blockIdx.x;
    float t[5];
    pj_finalize_plot<true>(keys, b, D, parts, arg, s, t);
    if (threadIdx.x == 0) {
        const float n = fmaxf(t[4], 1.f);
        for (int q = 0; q < 4; ++q) pred[b * 4 + q] = t[q] / n;
        nocc[b] = (int)t[4];
    }
}

__global__ void p2_backward_kernel(const float* __restrict__ dpred, const int* __restrict__ arg,
                                   const int* __restrict__ nocc, const int* __restrict__ pix, int B, int N, int D,
                                   float4* __restrict__ dpw) {
    // gather form: a point receives a pixel's gradient iff it is that pixel's arg-max, so every row of dpointwise is
    // written exactly once (no zero fill in front, no scatter): one launch
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * N) return;
    const int b = (int)(i / N), n = (int)(i - (size_t)b * N);
    const int* a = arg + ((size_t)b * D * D + pix[i]) * 3;
    const float inv = 1.0f / fmaxf((float)nocc[b], 1.f);
    const float4 g = reinterpret_cast<const float4*>(dpred)[b];
    float4 o;
    o.x = a[0] == n ? (g.x - g.y) * inv : 0.f;   // low vegetation also feeds bare soil = 1 - low
    o.y = 0.f;
    o.z = a[1] == n ? g.z * inv : 0.f;
    o.w = a[2] == n ? g.w * inv : 0.f;
    dpw[i] = o;
}

// P1: rasters (B,3,D,D) [low,med,high], image[y][x], NaN where empty, rows flipped (project_to_2d.py:80-113)
__global__ void p1_finalize_kernel(const unsigned long long* __restrict__ keys, int B, int D, float* __restrict__ rasters) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int ncell = D * D;
    if (i >= B * ncell * 3) return;
    const int b = i / (ncell * 3), rem = i - b * ncell * 3;
    const int cell = rem / 3, slot = rem - cell * 3;
    const int y = cell / D, x = cell - y * D;
    const unsigned long long k = keys[i];
    const float v = k ? pj_key_value(k) : __uint_as_float(0x7FC00000u);
    rasters[(((size_t)b * 3 + slot) * D + (D - 1 - y)) * D + x] = v;
}

}  // namespace

extern "C" int sn2_plot_project_forward(const float* pred_pointwise, const float* cloud_xy, long plot_stride, int B, int N,
                                        int D, unsigned long long* keys, int* pix, int* arg, int* nocc, float* pred,
                                        void* stream) {
    if (!pred_pointwise || !cloud_xy || !keys || !pix || !arg || !nocc || !pred || B <= 0 || N <= 0 || D <= 0)
        return SN2_EINVAL;
    if (D * D > MAX_CELLS || plot_stride < 2L * N) return SN2_ELIMIT;
    hipStream_t st = (hipStream_t)stream;
    // the first 4*B floats of `pred` double as the per-plot (xmin,xmax,ymin,ymax) scratch until the finalisation
    float* mm = pred;
    hipLaunchKernelGGL(plot_minmax_kernel, dim3(B), dim3(1024), 0, st, cloud_xy, plot_stride, N, mm, keys, D * D * 3);
    hipLaunchKernelGGL((scatter_max_kernel<0>), dim3(grid_slices(N), B), dim3(1024), (size_t)D * D * 3 * 8, st,
                       pred_pointwise, cloud_xy, plot_stride, N, D, (const float*)mm, 0.f, 0.f, keys, pix);
    hipLaunchKernelGGL(p2_finalize_kernel, dim3(B), dim3(256), 0, st, (const unsigned long long*)keys, D, 1, arg, nocc, pred);
    SN2_RETURN_LAUNCH();
}

extern "C" size_t sn2_p2_key_parts(int N) { return (size_t)SN2_P2_KEY_PARTS(N); }

extern "C" int sn2_plot_pixels(const float* cloud_xy, long plot_stride, int B, int N, int D, float* mm, int* pix, void* stream) {
    if (!cloud_xy || !mm || !pix || B <= 0 || N <= 0 || D <= 0) return SN2_EINVAL;
    if (D * D > MAX_CELLS || plot_stride < 2L * N) return SN2_ELIMIT;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(plot_minmax_kernel, dim3(B), dim3(1024), 0, st, cloud_xy, plot_stride, N, mm,
                       (unsigned long long*)nullptr, 0);
    hipLaunchKernelGGL(plot_pixels_kernel, dim3(grid_slices(N), B), dim3(1024), 0, st, cloud_xy, plot_stride, N, D,
                       (const float*)mm, pix);
    SN2_RETURN_LAUNCH();
}

extern "C" int sn2_plot_project_forward_pix(const float* pred_pointwise, const int* pix, int B, int N, int D,
                                            unsigned long long* keys, int* arg, int* nocc, float* pred, void* stream) {
    if (!pred_pointwise || !pix || !keys || !arg || !nocc || !pred || B <= 0 || N <= 0 || D <= 0) return SN2_EINVAL;
    if (D * D > MAX_CELLS) return SN2_ELIMIT;
    hipStream_t st = (hipStream_t)stream;
    const int parts = grid_slices(N);
    hipLaunchKernelGGL(scatter_max_pix_kernel, dim3(parts, B), dim3(1024), (size_t)D * D * 3 * 8, st, pred_pointwise, pix, N, D,
                       keys);
    hipLaunchKernelGGL(p2_finalize_kernel, dim3(B), dim3(256), 0, st, (const unsigned long long*)keys, D, parts, arg, nocc, pred);
    SN2_RETURN_LAUNCH();
}

// ------------------------------------------------------------------------------------------------------------
// Projection + loss of the training step in THREE launches instead of seven (round 5): learning/train.py:54-62,
//   pred = project_to_plotwise_coverages(coverages_pointwise, clouds, args)                       model/project_to_2d.py:7-55
//   loss = get_absolute_loss(pred, gt) + m get_NLL_loss(proba, pdf) + e get_entropy_loss(proba)   learning/loss_functions.py:9-57
// and their gradients.  The chip's floor for ANY launch is ~4.5 us (an empty kernel), the seven kernels were 4-7 us each:
//   launch 1  two independent jobs side by side: workgroups [0, parts B) scatter the coverages into per-slice key tables
//             (pj_scatter_slice, as scatter_max_pix_kernel), the rest sum the pointwise loss terms (pl_row_terms, as
//             loss_point_kernel);
//   launch 2  per plot: maximum over the slices, arg-max points, mean over occupied pixels (pj_finalize_plot, as
//             p2_finalize_kernel) -- and the workgroup that leaves last adds the loss up (pl_abs_term, pl_block_sum3 and
//             pl_outputs, as loss_final_kernel); the B x 5 words it needs from its peers travel as agent-scope atomics,
//             complete before their ticket;
//   backward  one pass over the points: d loss / d proba (pl_row_dproba, as loss_bwd_kernel) and d loss / d coverages (as
//             p2_backward_kernel, with the B x 3 values of d loss / d pred it needs recomputed from pred and gt by every thread).
// The same device functions per element as the separate kernels: the same pred, arg, dcov, dproba bits; the loss sums are
// grouped by 1024 instead of 256 rows per workgroup (fp64: 1e-16).
// ------------------------------------------------------------------------------------------------------------
namespace {
constexpr int PL_LOSS_BLOCKS = 512;

template <bool NLL, bool ENT>
__global__ __launch_bounds__(1024) void projected_loss_scatter_kernel(const float* __restrict__ vals, const int* __restrict__ pix,
                                                                     int B, int N, int D, int parts,
                                                                     unsigned long long* __restrict__ keys_part,
                                                                     const float4* __restrict__ proba, const double* __restrict__ pdf,
                                                                     int R, double* __restrict__ partials, int n_loss_blocks,
                                                                     unsigned* __restrict__ ticket) {
    extern __shared__ unsigned long long s_keys[];  // D*D*3 (the scatter workgroups)
    const int n_scatter = parts * B;
    if ((int)blockIdx.x < n_scatter) {
        const int b = blockIdx.x / parts;
        pj_scatter_slice(s_keys, vals, pix, N, D, b, parts, blockIdx.x - b * parts, keys_part);
        return;
    }
    // ---- the pointwise loss terms: one row per lane, 16 B of probabilities + 24 B of densities
    const int lb = blockIdx.x - n_scatter;
    if (lb == 0 && threadIdx.x == 0) *ticket = 0u;                  // the finalisation's arrival counter (next launch)
    __shared__ double s_part[2][16];
    double nll = 0.0, ent = 0.0;
    for (int i = lb * 1024 + threadIdx.x; i < R; i += n_loss_blocks * 1024) pl_row_terms<NLL, ENT>(proba[i], pdf, (size_t)i, nll, ent);
    pl_wave_partials(s_part, nll, ent);
    __syncthreads();
    if (threadIdx.x == 0) pl_store_partials16(s_part, partials + 2 * lb);
}

__global__ __launch_bounds__(256) void projected_loss_finalize_kernel(const unsigned long long* __restrict__ keys, int B, int D,
                                                                      int parts, int* __restrict__ arg, int* __restrict__ nocc,
                                                                      float* __restrict__ pred, const double* __restrict__ gt,
                                                                      const double* __restrict__ partials, int n_loss_blocks, int R,
                                                                      double m, double e, unsigned* __restrict__ ticket,
                                                                      double* __restrict__ out) {
    __shared__ float s[5][4];
    __shared__ int s_last;
    __shared__ double s3[3][256];
    const int b = blockIdx.x;
    float t[5];
    pj_finalize_plot<true>(keys, b, D, parts, arg, s, t);
    if (threadIdx.x == 0) {
        const float n = fmaxf(t[4], 1.f);
        // (agent-scope stores: the workgroup that adds the loss up reads them from another CU, maybe another XCD)
        for (int q = 0; q < 4; ++q)
            __hip_atomic_store(reinterpret_cast<unsigned*>(pred) + b * 4 + q, __float_as_uint(t[q] / n), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(nocc + b, (int)t[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // acq_rel at agent scope: the release orders this workgroup's pred / nocc stores before its ticket, the acquire makes
        // every earlier workgroup's stores visible to the last one (a relaxed add orders neither)
        s_last = (__hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)B - 1u) ? 1 : 0;
    }
    __syncthreads();
    if (!s_last) return;
    // ---- the last workgroup out: the loss value (as loss_final_kernel)
    double nll = 0.0, ent = 0.0, ab = 0.0;
    for (int i = threadIdx.x; i < n_loss_blocks; i += 256) nll += partials[2 * i], ent += partials[2 * i + 1];
    for (int i = threadIdx.x; i < 3 * B; i += 256) {
        const int bb = i / 3, col = pl_stratum_col(i - 3 * bb);
        const float pv = __uint_as_float(__hip_atomic_load(reinterpret_cast<unsigned*>(pred) + 4 * bb + col, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        ab += pl_abs_term(pv, gt[4 * bb + col]);
    }
    pl_block_sum3(s3, nll, ent, ab);
    if (threadIdx.x == 0) pl_outputs(s3[2][0] / (3.0 * B), s3[0][0], s3[1][0], n_loss_blocks > 0, R, m, e, out);
}

template <bool NLL, bool ENT>
__global__ __launch_bounds__(256) void projected_loss_bwd_kernel(const float* __restrict__ pred, const double* __restrict__ gt, int B,
                                                                 const float4* __restrict__ proba, const double* __restrict__ pdf,
                                                                 int N, int D, double m, double e, const double* __restrict__ gout,
                                                                 const int* __restrict__ arg, const int* __restrict__ nocc,
                                                                 const int* __restrict__ pix, float4* __restrict__ dcov,
                                                                 float4* __restrict__ dproba) {
    // (the arithmetic lives in loss_rules.h: the head backward's fused route evaluates the same two functions)
    const size_t R = (size_t)B * N;
    const double g = gout[0];
    double cn, ce;
    pl_row_coeffs(g, m, e, R, cn, ce);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < R; i += (size_t)gridDim.x * 256) {
        const float4 p = proba[i];
        double f0 = 0.0, f1 = 0.0, f2 = 0.0;
        if constexpr (NLL) f0 = pdf[3 * i], f1 = pdf[3 * i + 1], f2 = pdf[3 * i + 2];
        // d loss / d pred of the row's plot is recomputed here by every thread
        const int b = (int)(i / N), n = (int)(i - (size_t)b * N);
        const float4 pg = pl_plot_grad(pred, gt, nocc, b, B, g);
        const int* a = arg + ((size_t)b * D * D + pix[i]) * 3;
        float4 d, o;
        pl_row_grad(NLL, ENT, p, f0, f1, f2, cn, ce, pg, a[0], a[1], a[2], n, d, o);
        dproba[i] = d;
        dcov[i] = o;
    }
}
}  // namespace

extern "C" int sn2_projected_loss_forward(const float* coverages, const int* pix, const float* proba, const double* pdf,
                                          const double* gt, int B, int N, int D, double m, double e, unsigned long long* keys,
                                          int* arg, int* nocc, float* pred, double* partials, double* out, void* stream) {
    if (!coverages || !pix || !proba || !gt || !keys || !arg || !nocc || !pred || !partials || !out || B <= 0 || N <= 0 || D <= 0)
        return SN2_EINVAL;
    if (D * D > MAX_CELLS || (long)B * N >= (1L << 31)) return SN2_ELIMIT;
    const bool nll = m != 0.0, ent = e != 0.0;
    if (nll && !pdf) return SN2_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int parts = grid_slices(N), R = B * N;
    int nlb = (nll || ent) ? sn2_cdiv(R, 1024) : 0;
    if (nlb > PL_LOSS_BLOCKS) nlb = PL_LOSS_BLOCKS;
    unsigned* ticket = reinterpret_cast<unsigned*>(partials + 2 * PL_LOSS_BLOCKS);
    const int grid = parts * B + (nlb > 0 ? nlb : 1);              // (at least one loss workgroup: it clears the ticket)
    const size_t lds = (size_t)D * D * 3 * 8;
    const float4* p4 = reinterpret_cast<const float4*>(proba);
    pl_for_terms(nll, ent, [&](auto NLL, auto ENT) {        // (neither term: nlb = 0, no row is read)
        hipLaunchKernelGGL((projected_loss_scatter_kernel<NLL(), ENT()>), dim3(grid), dim3(1024), lds, st, coverages, pix, B, N, D, parts,
                           keys, p4, pdf, nlb > 0 ? R : 0, partials, nlb > 0 ? nlb : 1, ticket);
    });
    hipLaunchKernelGGL(projected_loss_finalize_kernel, dim3(B), dim3(256), 0, st, (const unsigned long long*)keys, B, D, parts, arg, nocc,
                       pred, gt, (const double*)partials, nlb, R, m, e, ticket, out);
    SN2_RETURN_LAUNCH();
}

extern "C" int sn2_projected_loss_backward(const float* pred, const double* gt, int B, const float* proba, const double* pdf, int N,
                                           int D, double m, double e, const double* grad_total, const int* arg, const int* nocc,
                                           const int* pix, float* dcoverages, float* dproba, void* stream) {
    if (!pred || !gt || !proba || !grad_total || !arg || !nocc || !pix || !dcoverages || !dproba || B <= 0 || N <= 0 || D <= 0)
        return SN2_EINVAL;
    const bool nll = m != 0.0, ent = e != 0.0;
    if (nll && !pdf) return SN2_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int grid = sn2_cdiv((long)B * N, 256);
    if (grid > 2048) grid = 2048;
    const float4* p4 = reinterpret_cast<const float4*>(proba);
    float4 *dc = reinterpret_cast<float4*>(dcoverages), *dp = reinterpret_cast<float4*>(dproba);
    pl_for_terms(nll, ent, [&](auto NLL, auto ENT) {
        hipLaunchKernelGGL((projected_loss_bwd_kernel<NLL(), ENT()>), dim3(grid), dim3(256), 0, st, pred, gt, B, p4, pdf, N, D, m, e,
                           grad_total, arg, nocc, pix, dc, dp);
    });
    SN2_RETURN_LAUNCH();
}

// ------------------------------------------------------------------------------------------------------------
// Validation pass: the losses of EVERY PLOT of a batch on its own (learning/test.py:52-79 evaluates with batch_size = 1, so its
// loss_abs / loss_log / loss_e / get_absolute_loss_by_strata are per-plot numbers that an AverageValueMeter then averages).
//   launch 1  one workgroup per (plot, slice of PL_SLICE_ROWS rows): scatters its rows' coverages into its own key table
//             (pj_push, as scatter_max_pix_kernel) AND sums the pointwise loss terms of the same rows (pl_row_terms, as
//             loss_point_kernel) -- the number of slices depends on N alone, so the pointwise pass of a single plot already is
//             cdiv(N, 2048) workgroups;
//   launch 2  one workgroup per plot: maximum over the slices and mean over occupied pixels (pj_finalize_plot, as
//             p2_finalize_kernel: the same pred bits), the plot's partial sums added slice 0, 1, 2, ... by one thread, the seven
//             outputs.
// Nothing crosses a plot's boundary and every sum has one fixed order that depends on N and D only: a plot's row is the same
// bytes at any position of any batch, run after run, and a NaN stays in its plot.  No atomics outside LDS (integer maxima).
// ------------------------------------------------------------------------------------------------------------
namespace {
constexpr int PL_SLICE_ROWS = SN2_PLOT_LOSSES_SLICE_ROWS;

inline int plot_losses_slices(int N) { return SN2_PLOT_LOSSES_SLICES(N); }

template <bool NLL, bool ENT>
__global__ __launch_bounds__(1024) void plot_losses_scatter_kernel(const float4* __restrict__ vals, const int* __restrict__ pix,
                                                                  const float4* __restrict__ proba, const double* __restrict__ pdf,
                                                                  int N, int D, int parts, unsigned long long* __restrict__ keys_part,
                                                                  double* __restrict__ partials) {
    extern __shared__ unsigned long long s_keys[];  // D*D*3
    __shared__ double s_part[2][16];
    const int b = blockIdx.x / parts, part = blockIdx.x - b * parts;
    const int ncell3 = D * D * 3;
    pj_clear(s_keys, ncell3);
    __syncthreads();
    int lo, hi;
    pj_slice(N, parts, part, lo, hi);
    double nll = 0.0, ent = 0.0;
    for (int n = lo + threadIdx.x; n < hi; n += 1024) {
        const size_t i = (size_t)b * N + n;
        pj_push(s_keys, pix[i], vals[i], n);
        if constexpr (NLL || ENT) pl_row_terms<NLL, ENT>(proba[i], pdf, i, nll, ent);
    }
    if constexpr (NLL || ENT) pl_wave_partials(s_part, nll, ent);
    __syncthreads();
    pj_copy_out<false>(s_keys, ncell3, keys_part + (size_t)blockIdx.x * ncell3);
    if constexpr (NLL || ENT) {
        if (threadIdx.x == 0) pl_store_partials16(s_part, partials + 2 * (size_t)blockIdx.x);
    }
}

// out row: total, absolute, NLL, entropy, abs_low, abs_med, abs_high
__global__ __launch_bounds__(256) void plot_losses_finalize_kernel(const unsigned long long* __restrict__ keys, int N, int D, int parts,
                                                                   const double* __restrict__ gt, const double* __restrict__ partials,
                                                                   int pointwise, double m, double e, float* __restrict__ pred,
                                                                   double* __restrict__ out) {
    __shared__ float s[5][4];
    const int b = blockIdx.x;
    float t[5];
    pj_finalize_plot<false>(keys, b, D, parts, nullptr, s, t);
    if (threadIdx.x != 0) return;
    const float n = fmaxf(t[4], 1.f);
    float pv[4];
    for (int q = 0; q < 4; ++q) pred[b * 4 + q] = pv[q] = t[q] / n;
    double* o = out + 7 * (size_t)b;
    double ab[3];
    for (int c = 0; c < 3; ++c) o[4 + c] = ab[c] = pl_abs_term(pv[pl_stratum_col(c)], gt[4 * b + pl_stratum_col(c)]);
    double nll = 0.0, ent = 0.0;
    if (pointwise) {
        const double* pp = partials + 2 * (size_t)b * parts;
        for (int q = 0; q < parts; ++q) nll += pp[2 * q], ent += pp[2 * q + 1];
    }
    pl_outputs(((ab[0] + ab[1]) + ab[2]) / 3.0, nll, ent, pointwise != 0, N, m, e, o);
}
}  // namespace

extern "C" size_t sn2_plot_losses_ws_words(int B, int N, int D) {
    if (B <= 0 || N <= 0 || D <= 0 || D > 45 || D * D > MAX_CELLS || (long)B * N >= (1L << 31)) return 0;
    const size_t slices = (size_t)B * plot_losses_slices(N);
    return 2 * (slices * (size_t)D * D * 3 + slices * 2);          // u64 key tables, then two fp64 partial sums per slice
}

extern "C" int sn2_plot_losses(const float* coverages, const int* pix, const float* proba, const double* pdf, const double* gt,
                               int B, int N, int D, double m, double e, void* ws, float* pred, double* out, void* stream) {
    if (!coverages || !pix || !gt || !ws || !pred || !out || B <= 0 || N <= 0 || D <= 0) return SN2_EINVAL;
    const bool nll = m != 0.0, ent = e != 0.0;
    if ((nll || ent) && !proba) return SN2_EINVAL;
    if (nll && !pdf) return SN2_EINVAL;
    if (((uintptr_t)ws & 7) != 0) return SN2_EINVAL;
    if (D > 45 || D * D > MAX_CELLS || (long)B * N >= (1L << 31)) return SN2_ELIMIT;
    hipStream_t st = (hipStream_t)stream;
    const int parts = plot_losses_slices(N);
    const size_t slices = (size_t)B * parts;
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws);
    double* partials = reinterpret_cast<double*>(keys + slices * (size_t)D * D * 3);
    const size_t lds = (size_t)D * D * 3 * 8;
    const float4* c4 = reinterpret_cast<const float4*>(coverages);
    const float4* p4 = reinterpret_cast<const float4*>(proba);
    const dim3 grid((unsigned)slices);
    pl_for_terms(nll, ent, [&](auto NLL, auto ENT) {
        hipLaunchKernelGGL((plot_losses_scatter_kernel<NLL(), ENT()>), grid, dim3(1024), lds, st, c4, pix, p4, pdf, N, D, parts, keys, partials);
    });
    hipLaunchKernelGGL(plot_losses_finalize_kernel, dim3(B), dim3(256), 0, st, (const unsigned long long*)keys, N, D, parts, gt,
                       (const double*)partials, (nll || ent) ? 1 : 0, m, e, pred, out);
    SN2_RETURN_LAUNCH();
}

extern "C" int sn2_plot_project_backward(const float* dpred, const int* arg, const int* nocc, const int* pix, int B, int N,
                                         int D, float* dpointwise, void* stream) {
    if (!dpred || !arg || !nocc || !pix || !dpointwise || B <= 0 || N <= 0 || D <= 0) return SN2_EINVAL;
    hipLaunchKernelGGL(p2_backward_kernel, dim3(sn2_cdiv((long)B * N, 256)), dim3(256), 0, (hipStream_t)stream, dpred, arg,
                       nocc, pix, B, N, D, reinterpret_cast<float4*>(dpointwise));
    SN2_RETURN_LAUNCH();
}

extern "C" int sn2_raster_project(const float* coverages, const float* cloud_xy, long plot_stride, int B, int N, int D,
                                  int diam_meters, unsigned long long* keys, int* pix, float* rasters, void* stream) {
    if (!coverages || !cloud_xy || !keys || !pix || !rasters || B <= 0 || N <= 0 || D <= 0 || diam_meters <= 0)
        return SN2_EINVAL;
    if (D * D > MAX_CELLS || plot_stride < 2L * N) return SN2_ELIMIT;
    hipStream_t st = (hipStream_t)stream;
    const float sf = (float)(10.0 * ((double)D / (double)diam_meters));  // python: 10 * (diam_pix / diam_meters)
    const float off = (float)(diam_meters / 2);                           // diam_meters // 2
    sn2_fill_words(keys, 0u, (size_t)B * D * D * 3 * 2, st);
    hipLaunchKernelGGL((scatter_max_kernel<1>), dim3(grid_slices(N), B), dim3(1024), (size_t)D * D * 3 * 8, st, coverages,
                       cloud_xy, plot_stride, N, D, (const float*)nullptr, sf, off, keys, pix);
    hipLaunchKernelGGL(p1_finalize_kernel, dim3(sn2_cdiv((long)B * D * D * 3, 256)), dim3(256), 0, st,
                       (const unsigned long long*)keys, B, D, rasters);
    SN2_RETURN_LAUNCH();
}

// ------------------------------------------------------------------------------------------------------------
// Parcel mosaic: fold the plots of a batch, in order, into the running (mean, weight-sum) rasters with the rule of the
// rasterio.merge callback (inference/geotiff_raster.py:294-347).  One thread per (band, parcel pixel) of the window; the
// plot offsets are wave-uniform (scalar loads), the raster reads are contiguous along x.
// ------------------------------------------------------------------------------------------------------------
namespace {
__global__ void mosaic_merge_kernel(const float* __restrict__ rasters, const float* __restrict__ weights,
                                    const int* __restrict__ offsets, int B, int D, int H, int W,
                                    float* __restrict__ mean, float* __restrict__ wsum, int y0, int x0, int wh, int ww) {
    // (the fold itself: mosaic_rules.h, shared with the atlas kernels)
    const int wx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int wy = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int band = blockIdx.z;
    if (wx >= ww || wy >= wh) return;
    const int gy = y0 + wy, gx = x0 + wx;
    if (gy < 0 || gy >= H || gx < 0 || gx >= W) return;
    mosaic_fold_pixel(rasters, weights, offsets, 2, 0, B, D, band, H, W, gy, gx, mean, wsum);
}
}  // namespace

extern "C" int sn2_mosaic_merge(const float* rasters, const float* weights, const int* offsets, int B, int D, int H, int W,
                                float* mean, float* wsum, int win_y0, int win_x0, int win_h, int win_w, void* stream) {
    if (!rasters || !weights || !offsets || !mean || !wsum || B <= 0 || D <= 0 || H <= 0 || W <= 0) return SN2_EINVAL;
    if (win_h <= 0 || win_w <= 0) return 0;
    hipLaunchKernelGGL(mosaic_merge_kernel, dim3(sn2_cdiv(win_w, 64), sn2_cdiv(win_h, 4), 3), dim3(256), 0,
                       (hipStream_t)stream, rasters, weights, offsets, B, D, H, W, mean, wsum, win_y0, win_x0, win_h, win_w);
    SN2_RETURN_LAUNCH();
}

// ------------------------------------------------------------------------------------------------------------
// Mosaic finalisation: finalize_merged_raster without the GIS step (inference/geotiff_raster.py:262-285 + :119-144).
// The reference finds the hard medium-vegetation threshold by evaluating 10 001 thresholds, each over the whole image
// (O(10^4 x pixels) in numpy).  Here every valid pixel is binned once by the number k(v) of thresholds below its value;
// the number of pixels above threshold i is then a suffix sum of that histogram, the 10 001 deltas come from it, and the
// first minimum is taken as numpy's argmin does.  Thresholds lin[i] = i * (1/10000) in fp64, lin[10000] = 1 (np.linspace);
// the comparison v > lin[i] is made in fp64.
// ------------------------------------------------------------------------------------------------------------
namespace {
// (HARD_STEPS, hard_lin, the bin rule, the threshold search and the NaN rule: mosaic_rules.h, shared with the atlas kernels)
// ws: [0..HARD_STEPS] histogram of k, [HARD_STEPS+1] number of valid pixels; sum_ws: fp64 sum of the valid values
__global__ __launch_bounds__(256) void hard_hist_kernel(const float* __restrict__ med, long P, int* __restrict__ ws,
                                                        double* __restrict__ sum_ws) {
    double sum;
    int cnt;
    hard_hist_block(med, P, (long)blockIdx.x * 256, (long)gridDim.x * 256, ws, sum, cnt);
    if (threadIdx.x == 0) {
        atomicAdd(sum_ws, sum);
        atomicAdd(&ws[HARD_STEPS + 1], cnt);
    }
}

// one workgroup: suffix sums, deltas, first minimum -> thr_out[0] = threshold (fp64 value as float), thr_out[1] = index
__global__ __launch_bounds__(1024) void hard_threshold_kernel(const int* __restrict__ ws, const double* __restrict__ sum_ws,
                                                              float* __restrict__ thr_out) {
    hard_threshold_search(ws, ws[HARD_STEPS + 1], sum_ws[0], thr_out);
}

// out (5,H,W) = [Vb, Vm_soft, Vh, Vm_hard, weights] with the reference's NaN rule: NaN -> 0 wherever at least one of the
// three scores is a number, all bands NaN elsewhere
__global__ __launch_bounds__(256) void mosaic_finalize_kernel(const float* __restrict__ mean, const float* __restrict__ wsum,
                                                              long P, const float* __restrict__ thr, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    mosaic_finalize_pixel(mean, wsum, P, i, hard_lin((int)thr[1]), out);
}
}  // namespace

extern "C" int sn2_mosaic_finalize(const float* mean, const float* wsum, int H, int W, int* hist_ws, double* sum_ws,
                                   float* thr_out, float* out, void* stream) {
    if (!mean || !wsum || !hist_ws || !sum_ws || !thr_out || !out || H <= 0 || W <= 0) return SN2_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const long P = (long)H * W;
    sn2_fill_words(hist_ws, 0u, (size_t)SN2_MOSAIC_HIST_WORDS, st);
    sn2_fill_words(sum_ws, 0u, 2, st);
    int grid = sn2_cdiv(P, 256);
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(hard_hist_kernel, dim3(grid), dim3(256), 0, st, mean + P, P, hist_ws, sum_ws);
    hipLaunchKernelGGL(hard_threshold_kernel, dim3(1), dim3(1024), 0, st, (const int*)hist_ws, (const double*)sum_ws, thr_out);
    hipLaunchKernelGGL(mosaic_finalize_kernel, dim3(sn2_cdiv(P, 256)), dim3(256), 0, st, mean, wsum, P, (const float*)thr_out, out);
    SN2_RETURN_LAUNCH();
}

// ------------------------------------------------------------------------------------------------------------
// Parcel crop and band means of the mosaic: crop_merged_raster (inference/geotiff_raster.py:238-253) + the band-wise nanmean of
// get_parcel_predicted_values (inference/predict_utils.py:124-146).  The rule is written out in include/strata_hip.h.
// A workgroup owns row segments of 256 pixels, one pixel per thread; the walk over the edges and the summation trees are
// mosaic_crop_block / mosaic_crop_fold of mosaic_rules.h, which the atlas kernels (atlas.hip) execute as well.
// ------------------------------------------------------------------------------------------------------------
namespace {
// psum, pcnt: (gridDim.x, C) partial sums and counts, every entry written
template <bool CROP>
__global__ __launch_bounds__(CROP_T) void mosaic_crop_kernel(float* __restrict__ bands, int C, int H, int W, double x_min,
                                                             double y_max, double pix, const double* __restrict__ edges, int E,
                                                             double* __restrict__ psum, long long* __restrict__ pcnt) {
    __shared__ CropLds s;
    mosaic_crop_block<CROP>(s, bands, C, H, W, x_min, y_max, pix, edges, E, (int)blockIdx.x, (int)gridDim.x,
                            psum + (size_t)blockIdx.x * C, pcnt + (size_t)blockIdx.x * C);
}

// one workgroup: thread t adds the partials of workgroups t, t + 256, ... in order, the threads in a fixed tree
__global__ __launch_bounds__(CROP_T) void mosaic_crop_fold_kernel(const double* __restrict__ psum, const long long* __restrict__ pcnt,
                                                                  int C, int nblk, double* __restrict__ mean,
                                                                  long long* __restrict__ count) {
    mosaic_crop_fold(psum, pcnt, C, nblk, mean, count);
}
}  // namespace

extern "C" size_t sn2_mosaic_crop_ws_words(int C, int H, int W) {
    if (C < 1 || H < 1 || W < 1) return 0;
    return SN2_MOSAIC_CROP_WS_WORDS(C, H, W);
}

extern "C" int sn2_mosaic_crop_stats(float* bands, int C, int H, int W, double x_min, double y_max, double pix, const double* edges,
                                     int E, void* ws, double* mean, long long* count, void* stream) {
    if (!bands || !ws || !mean || !count || C < 1 || H < 1 || W < 1 || E < 0) return SN2_EINVAL;
    if ((E == 0) != (edges == nullptr) || (E > 0 && E < 3)) return SN2_EINVAL;        // a ring has three edges or more
    if (!(pix > 0.0) || !std::isfinite(pix) || !std::isfinite(x_min) || !std::isfinite(y_max)) return SN2_EINVAL;
    if (((uintptr_t)ws & 7) != 0) return SN2_EINVAL;
    if (C > SN2_MOSAIC_CROP_MAX_BANDS || (long)H * W >= (1L << 31) || E > SN2_MOSAIC_CROP_MAX_EDGES) return SN2_ELIMIT;
    hipStream_t st = (hipStream_t)stream;
    const int nblk = (int)SN2_MOSAIC_CROP_BLOCKS(H, W);
    double* psum = (double*)ws;
    long long* pcnt = (long long*)(psum + (size_t)nblk * C);
    if (E > 0)
        hipLaunchKernelGGL(mosaic_crop_kernel<true>, dim3(nblk), dim3(CROP_T), 0, st, bands, C, H, W, x_min, y_max, pix, edges, E, psum,
                           pcnt);
    else
        hipLaunchKernelGGL(mosaic_crop_kernel<false>, dim3(nblk), dim3(CROP_T), 0, st, bands, C, H, W, x_min, y_max, pix, edges, E, psum,
                           pcnt);
    hipLaunchKernelGGL(mosaic_crop_fold_kernel, dim3(1), dim3(CROP_T), 0, st, (const double*)psum, (const long long*)pcnt, C, nblk, mean,
                       count);
    SN2_RETURN_LAUNCH();
}
