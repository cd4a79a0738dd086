// loss_rules.h -- the three loss terms (absolute, NLL, entropy: learning/loss_functions.py:9-57) and their gradients, stated once
// as device functions: what ONE ROW adds to the pointwise sums and receives from them, what ONE PLOT adds to the absolute term
// and receives from it, and how the sums become the four outputs.  The kernels of loss.hip, the one-node and per-plot routes
// of project.hip and head_bwd_mfma_kernel (head.hip: the fused route, sn2_head.loss) call them, so every path evaluates the
// same expression tree: the same bits whether a gradient travels through memory or not.  What the kernels keep to themselves is
// the ORDER in which they add their partial sums (it is part of their output bits); a reduction stands here only where two
// kernels share it.
#pragma once
#include <type_traits>

#include "common.h"

constexpr int PL_MAX_CELLS = 2025;  // diam_pix <= 45: the D*D*3 keys of a workgroup fit the default 48 KiB dynamic LDS
constexpr int PL_HEAD_MAX_PLOTS = SN2_HEAD_LOSS_MAX_PLOTS;   // the fused route's per-plot table in head_bwd_mfma_kernel's LDS (2 KB)
constexpr float PL_EPS_F = 0.0001f;
constexpr double PL_EPS_D = 0.0001;

// one call of f(NLL, ENT) with the two switches as compile-time constants (std::true_type / std::false_type): the launch of a
// kernel template <bool NLL, bool ENT> for a runtime pair is  pl_for_terms(nll, ent, [&](auto NLL, auto ENT) { ...<NLL(), ENT()>... })
template <class F>
inline void pl_for_terms(bool nll, bool ent, F&& f) {
    if (nll && ent) f(std::true_type{}, std::true_type{});
    else if (nll) f(std::true_type{}, std::false_type{});
    else if (ent) f(std::false_type{}, std::true_type{});
    else f(std::false_type{}, std::false_type{});
}

#ifdef __HIPCC__
__device__ __forceinline__ double pl_wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- forward, one row: p = its probabilities, pdf[3 i ..] = its densities (not read when !NLL).  A term whose weight is zero
// is SKIPPED, not multiplied by zero: a caller that asks for the entropy of rows that are no probability vectors -- the
// reference's docstring says "coverage raster" -- must not get 0 * log(<= 0) = NaN from a likelihood nobody asked for, and the
// densities need not exist.  Types as torch's promotion gives the reference: the likelihood in fp64, the entropy terms in fp32.
template <bool NLL, bool ENT>
__device__ __forceinline__ void pl_row_terms(float4 p, const double* __restrict__ pdf, size_t i, double& nll, double& ent) {
    if constexpr (NLL) {
        const double f0 = pdf[3 * i], f1 = pdf[3 * i + 1], f2 = pdf[3 * i + 2];
        const float pg = p.x + p.y;                               // pred[:, :2].sum(1) in fp32 (:44)
        const double lik = ((double)pg * f0 + (double)p.z * f1) + (double)p.w * f2;
        nll -= log(lik);
    }
    if constexpr (ENT) {
        const float e2 = p.z * logf(p.z + PL_EPS_F) + (1.f - p.z) * logf(1.f - p.z + PL_EPS_F);
        const float e3 = p.w * logf(p.w + PL_EPS_F) + (1.f - p.w) * logf(1.f - p.w + PL_EPS_F);
        ent -= (double)e2 + (double)e3;
    }
}

// the lanes of each of a workgroup's W waves by butterfly, one partial per wave into LDS (the kernel's barrier follows) ...
template <int W>
__device__ __forceinline__ void pl_wave_partials(double (&s)[2][W], double nll, double ent) {
    nll = pl_wave_sum_f64(nll);
    ent = pl_wave_sum_f64(ent);
    if ((threadIdx.x & 63) == 0) s[0][threadIdx.x >> 6] = nll, s[1][threadIdx.x >> 6] = ent;
}
// ... and, for the two 1024-thread kernels, the sixteen waves added 0..15 onto 0.0 by one thread
__device__ __forceinline__ void pl_store_partials16(const double (&s)[2][16], double* __restrict__ out2) {
    double a = 0.0, c = 0.0;
    for (int k = 0; k < 16; ++k) a += s[0][k], c += s[1][k];
    out2[0] = a;
    out2[1] = c;
}

// ---- the absolute term of one (plot, stratum): strata low, medium, high = columns 0, 2, 3 of pred / gt (:12; column 1, bare
// soil, has no target)
__device__ __forceinline__ int pl_stratum_col(int c) { return c == 0 ? 0 : c + 1; }
__device__ __forceinline__ double pl_abs_term(float pred, double gt) {
    const double d = (double)pred - gt;
    return sqrt(d * d + PL_EPS_D);
}

// the 256-thread halving tree over three running sums: the totals end in s[.][0], for thread 0
__device__ __forceinline__ void pl_block_sum3(double (&s)[3][256], double a, double b, double c) {
    s[0][threadIdx.x] = a, s[1][threadIdx.x] = b, s[2][threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            s[0][threadIdx.x] += s[0][threadIdx.x + o];
            s[1][threadIdx.x] += s[1][threadIdx.x + o];
            s[2][threadIdx.x] += s[2][threadIdx.x + o];
        }
        __syncthreads();
    }
}

// out[0..3] = total, absolute, NLL, entropy from the absolute term's mean and the two pointwise sums over `rows` rows
// (pointwise false: no row was summed, both terms are 0.0).  The reference's entropy is an fp32 tensor.
__device__ __forceinline__ void pl_outputs(double l_abs, double nll, double ent, bool pointwise, int rows, double m, double e,
                                           double* __restrict__ out) {
    const double l_nll = pointwise ? nll / rows : 0.0;
    const double l_ent = pointwise ? (double)(float)(ent / (2.0 * rows)) : 0.0;
    out[0] = l_abs + m * l_nll + e * l_ent;
    out[1] = l_abs;
    out[2] = l_nll;
    out[3] = l_ent;
}

// ---- backward.  cn, ce: what the NLL and the entropy term's derivative of a row are scaled by (g = d objective / d total)
__device__ __forceinline__ void pl_row_coeffs(double g, double m, double e, size_t R, double& cn, double& ce) {
    cn = g * m / (double)R;
    ce = g * e / (2.0 * (double)R);
}

// d loss / d pred of one element of columns 0, 2, 3
__device__ __forceinline__ float pl_pred_grad(float pred, double gt, int B, double g) {
    const double d = (double)pred - gt;
    return (float)(g * d / sqrt(d * d + PL_EPS_D) / (3.0 * B));
}

// plot b -> (gx, gz, gw, inv): d loss / d pred of columns 0, 2, 3 and 1 / max(occupied pixels, 1)
__device__ __forceinline__ float4 pl_plot_grad(const float* __restrict__ pred, const double* __restrict__ gt,
                                               const int* __restrict__ nocc, int b, int B, double g) {
    const float4 pr = reinterpret_cast<const float4*>(pred)[b];
    float4 o;
    o.x = pl_pred_grad(pr.x, gt[4 * b + 0], B, g);
    o.y = pl_pred_grad(pr.z, gt[4 * b + 2], B, g);
    o.z = pl_pred_grad(pr.w, gt[4 * b + 3], B, g);
    o.w = 1.0f / fmaxf((float)nocc[b], 1.f);
    return o;
}

// d loss / d proba of one row: p = the STORED probabilities, f0..f2 = its densities (not read when !nll)
__device__ __forceinline__ float4 pl_row_dproba(bool nll, bool ent, float4 p, double f0, double f1, double f2, double cn, double ce) {
    double d0 = 0.0, d2 = 0.0, d3 = 0.0;
    if (nll) {
        const float pgr = p.x + p.y;
        const double lik = ((double)pgr * f0 + (double)p.z * f1) + (double)p.w * f2;
        const double il = -cn / lik;
        d0 = il * f0, d2 = il * f1, d3 = il * f2;
    }
    if (ent) {
        const float h2 = -(logf(p.z + PL_EPS_F) + p.z / (p.z + PL_EPS_F) - logf(1.f - p.z + PL_EPS_F) - (1.f - p.z) / (1.f - p.z + PL_EPS_F));
        const float h3 = -(logf(p.w + PL_EPS_F) + p.w / (p.w + PL_EPS_F) - logf(1.f - p.w + PL_EPS_F) - (1.f - p.w) / (1.f - p.w + PL_EPS_F));
        d2 += ce * (double)h2, d3 += ce * (double)h3;
    }
    float4 d;
    d.x = d.y = (float)d0;
    d.z = (float)d2;
    d.w = (float)d3;
    return d;
}

// row n of its plot: pl_row_dproba, and d loss / d coverages: the point receives its pixel's gradient iff it is the pixel's
// arg-max (p2_backward_kernel).  pg = pl_plot_grad of its plot, a0..a2 = the arg-max points of its pixel (-1: empty)
__device__ __forceinline__ void pl_row_grad(bool nll, bool ent, float4 p, double f0, double f1, double f2, double cn, double ce,
                                            float4 pg, int a0, int a1, int a2, int n, float4& dproba, float4& dcov) {
    dproba = pl_row_dproba(nll, ent, p, f0, f1, f2, cn, ce);
    const float gx = pg.x, gz = pg.y, gw = pg.z, inv = pg.w;
    dcov.x = a0 == n ? (gx - 0.f) * inv : 0.f;      // (g.x - g.y) with g.y = 0: bare soil carries no gradient of its own
    dcov.y = 0.f;
    dcov.z = a1 == n ? gz * inv : 0.f;
    dcov.w = a2 == n ? gw * inv : 0.f;
}
#endif
