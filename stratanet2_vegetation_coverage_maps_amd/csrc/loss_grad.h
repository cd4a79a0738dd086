// loss_grad.h -- the gradient of projection + loss (sn2_projected_loss_backward) as two device functions: what ONE PLOT
// contributes (d loss / d pred of its three strata and 1 / occupied pixels) and what ONE ROW receives (d loss / d proba from
// the NLL and entropy terms, d loss / d coverages where the row is its pixel's arg-max).  projected_loss_bwd_kernel
// (project.hip) and head_bwd_mfma_kernel (head.hip: the fused route, sn2_head.loss) both call them, so the two paths
// evaluate the same expression tree: the same dproba / dcoverages bits whether they travel through memory or not.
#pragma once
#include "common.h"

constexpr int PL_MAX_CELLS = 2025;  // diam_pix <= 45: the D*D*3 keys of a workgroup fit the default 48 KiB dynamic LDS
constexpr int PL_HEAD_MAX_PLOTS = SN2_HEAD_LOSS_MAX_PLOTS;   // the fused route's per-plot table in head_bwd_mfma_kernel's LDS (2 KB)
constexpr float PL_EPS_F = 0.0001f;
constexpr double PL_EPS_D = 0.0001;

#ifdef __HIPCC__
// cn, ce: what the NLL and the entropy term's derivative of a row are scaled by (g = d objective / d total)
__device__ __forceinline__ void pl_row_coeffs(double g, double m, double e, size_t R, double& cn, double& ce) {
    cn = g * m / (double)R;
    ce = g * e / (2.0 * (double)R);
}

// plot b -> (gx, gz, gw, inv): d loss / d pred of columns 0, 2, 3 (loss_bwd_kernel's formula: column 1, bare soil, has no
// target) and 1 / max(occupied pixels, 1)
__device__ __forceinline__ float4 pl_plot_grad(const float* __restrict__ pred, const double* __restrict__ gt,
                                               const int* __restrict__ nocc, int b, int B, double g) {
    const float4 pr = reinterpret_cast<const float4*>(pred)[b];
    const double e0 = (double)pr.x - gt[4 * b + 0], e2 = (double)pr.z - gt[4 * b + 2], e3 = (double)pr.w - gt[4 * b + 3];
    float4 o;
    o.x = (float)(g * e0 / sqrt(e0 * e0 + PL_EPS_D) / (3.0 * B));
    o.y = (float)(g * e2 / sqrt(e2 * e2 + PL_EPS_D) / (3.0 * B));
    o.z = (float)(g * e3 / sqrt(e3 * e3 + PL_EPS_D) / (3.0 * B));
    o.w = 1.0f / fmaxf((float)nocc[b], 1.f);
    return o;
}

// row n of its plot: p = the STORED probabilities, f0..f2 = its densities (not read when !nll), pg = pl_plot_grad of its
// plot, a0..a2 = the arg-max points of its pixel (-1: empty)
__device__ __forceinline__ void pl_row_grad(bool nll, bool ent, float4 p, double f0, double f1, double f2, double cn, double ce,
                                            float4 pg, int a0, int a1, int a2, int n, float4& dproba, float4& dcov) {
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
    dproba.x = dproba.y = (float)d0;
    dproba.z = (float)d2;
    dproba.w = (float)d3;
    // d loss / d coverages: the point receives its pixel's gradient iff it is the pixel's arg-max (p2_backward_kernel)
    const float gx = pg.x, gz = pg.y, gw = pg.z, inv = pg.w;
    dcov.x = a0 == n ? (gx - 0.f) * inv : 0.f;      // (g.x - g.y) with g.y = 0: bare soil carries no gradient of its own
    dcov.y = 0.f;
    dcov.z = a1 == n ? gz * inv : 0.f;
    dcov.w = a2 == n ? gw * inv : 0.f;
}
#endif
