// loss.hip -- the loss block of the training step as three kernels (gfx950).
//
// Replaces the ~75 elementwise / reduction launches torch needs for
//   loss = get_absolute_loss(pred, gt) + m * get_NLL_loss(proba, pdf_all) + e * get_entropy_loss(proba)
// (/root/reference/learning/loss_functions.py:9-57 as combined by learning/train.py:58-62) and for its backward.
// Arithmetic types follow what torch's type promotion gives the reference: the absolute loss and the NLL in fp64
// (gt and the KDE densities are fp64 numpy arrays), the entropy terms in fp32.  Sums are per-workgroup partials added in
// a fixed order: deterministic.
#include "common.h"
#include "loss_rules.h"

namespace {

constexpr int LOSS_BLOCKS = SN2_LOSS_BLOCKS;

// one row per lane: 16 B of probabilities + 24 B of densities, both contiguous across the wave.  NLL / ENT: which of the two
// pointwise terms are wanted (pl_row_terms)
template <bool NLL, bool ENT>
__global__ __launch_bounds__(256) void loss_point_kernel(const float4* __restrict__ proba, const double* __restrict__ pdf,
                                                         int R, double* __restrict__ partials) {
    __shared__ double s_part[2][4];
    double nll = 0.0, ent = 0.0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < R; i += gridDim.x * 256) pl_row_terms<NLL, ENT>(proba[i], pdf, (size_t)i, nll, ent);
    pl_wave_partials(s_part, nll, ent);
    __syncthreads();
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = (s_part[0][0] + s_part[0][1]) + (s_part[0][2] + s_part[0][3]);
        partials[2 * blockIdx.x + 1] = (s_part[1][0] + s_part[1][1]) + (s_part[1][2] + s_part[1][3]);
    }
}

// out[0..3] = total, absolute, NLL, entropy
__global__ __launch_bounds__(256) void loss_final_kernel(const float* __restrict__ pred, const double* __restrict__ gt, int B,
                                                         const double* __restrict__ partials, int nblocks, int R, double m,
                                                         double e, double* __restrict__ out) {
    __shared__ double s[3][256];
    double nll = 0.0, ent = 0.0, ab = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) { nll += partials[2 * i]; ent += partials[2 * i + 1]; }
    for (int i = threadIdx.x; i < 3 * B; i += 256) {
        const int b = i / 3, col = pl_stratum_col(i - 3 * b);
        ab += pl_abs_term(pred[4 * b + col], gt[4 * b + col]);
    }
    pl_block_sum3(s, nll, ent, ab);
    if (threadIdx.x == 0) pl_outputs(B > 0 ? s[2][0] / (3.0 * B) : 0.0, s[0][0], s[1][0], nblocks > 0, R, m, e, out);
}

// d loss / d proba, d loss / d pred for the upstream gradient g of the TOTAL loss (device scalar)
template <bool NLL, bool ENT>
__global__ __launch_bounds__(256) void loss_bwd_kernel(const float* __restrict__ pred, const double* __restrict__ gt, int B,
                                                       const float4* __restrict__ proba, const double* __restrict__ pdf, int R,
                                                       double m, double e, const double* __restrict__ gout,
                                                       float* __restrict__ dpred, float4* __restrict__ dproba) {
    const double g = gout[0];
    double cn = 0.0, ce = 0.0;
    if (R > 0) pl_row_coeffs(g, m, e, (size_t)R, cn, ce);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < R; i += gridDim.x * 256) {
        double f0 = 0.0, f1 = 0.0, f2 = 0.0;
        if constexpr (NLL) f0 = pdf[3 * (size_t)i], f1 = pdf[3 * (size_t)i + 1], f2 = pdf[3 * (size_t)i + 2];
        dproba[i] = pl_row_dproba(NLL, ENT, proba[i], f0, f1, f2, cn, ce);
    }
    if (blockIdx.x == 0 && dpred) {
        for (int i = threadIdx.x; i < 4 * B; i += 256) dpred[i] = (i & 3) != 1 ? pl_pred_grad(pred[i], gt[i], B, g) : 0.f;
    }
}

// KDE-mixture densities at the points' heights: KdeMixture.predict (learning/kde_mixture.py:65-70) = three scipy
// interp1d(kind="linear") over one knot vector, evaluated by get_NLL_loss on the CPU for all B*N points every step
// (learning/loss_functions.py:30-42).  Same arithmetic as scipy's _call_linear, in fp64 without contraction:
//   i = clip(searchsorted(X, z, side="left"), 1, K-1);  slope = (y[i] - y[i-1]) / (X[i] - X[i-1]);  y = slope*(z - X[i-1]) + y[i-1]
// z = fp64( fp32(cloud[b][zc][n]) * fp32(z_max) ) as the reference forms it (a float32 tensor times a python float).
// Heights outside [X[0], X[K-1]] (scipy raises ValueError there) give NaN.
__global__ __launch_bounds__(256) void kde_lookup_kernel(const float* __restrict__ cloud, int C, int N, int zc, float z_max,
                                                         const double* __restrict__ X, const double* __restrict__ Y, int K,
                                                         long R, double* __restrict__ pdf) {
#pragma clang fp contract(off)
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const long b = r / N, n = r - b * N;
    const double z = (double)(cloud[(b * C + zc) * N + n] * z_max);
    int lo = 0, hi = K;                         // first index with X[i] >= z
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (X[mid] < z) lo = mid + 1;
        else hi = mid;
    }
    const bool inside = z >= X[0] && z <= X[K - 1];
    int i = lo < 1 ? 1 : (lo > K - 1 ? K - 1 : lo);
    const double x_lo = X[i - 1], x_hi = X[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double y_lo = Y[(size_t)k * K + i - 1], y_hi = Y[(size_t)k * K + i];
        const double slope = (y_hi - y_lo) / (x_hi - x_lo);
        const double v = slope * (z - x_lo) + y_lo;
        pdf[3 * r + k] = inside ? v : __longlong_as_double(0x7ff8000000000000LL);
    }
}

inline int loss_grid(int R) {
    const int n = sn2_cdiv(R, 256);
    return n < LOSS_BLOCKS ? n : LOSS_BLOCKS;
}

}  // namespace

extern "C" int sn2_loss_forward(const float* pred, const double* gt, int B, const float* proba, const double* pdf, int R,
                                double m, double e, double* partials, double* out, void* stream) {
    // a term that is switched off is skipped and its inputs may be absent: B = 0 (no absolute term: pred, gt unused),
    // m == 0 (no NLL: pdf unused), e == 0 (no entropy); m == e == 0 or R == 0: no pass over the points at all
    if (!out || B < 0 || R < 0 || (B > 0 && (!pred || !gt))) return SN2_EINVAL;
    const bool nll = m != 0.0 && R > 0, ent = e != 0.0 && R > 0;
    if ((nll || ent) && (!proba || !partials)) return SN2_EINVAL;
    if (nll && !pdf) return SN2_EINVAL;
    const int nb = (nll || ent) ? loss_grid(R) : 0;
    hipStream_t st = (hipStream_t)stream;
    const float4* p4 = reinterpret_cast<const float4*>(proba);
    pl_for_terms(nll, ent, [&](auto NLL, auto ENT) {
        if constexpr (NLL() || ENT()) hipLaunchKernelGGL((loss_point_kernel<NLL(), ENT()>), dim3(nb), dim3(256), 0, st, p4, pdf, R, partials);
    });
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, st, pred, gt, B, (const double*)partials, nb, R > 0 ? R : 1, m, e, out);
    SN2_RETURN_LAUNCH();
}

extern "C" int sn2_loss_backward(const float* pred, const double* gt, int B, const float* proba, const double* pdf, int R,
                                 double m, double e, const double* grad_total, float* dpred, float* dproba, void* stream) {
    if (!grad_total || B < 0 || R < 0 || (B > 0 && (!pred || !gt || !dpred)) || (R > 0 && (!proba || !dproba))) return SN2_EINVAL;
    const bool nll = m != 0.0 && R > 0, ent = e != 0.0 && R > 0;
    if (nll && !pdf) return SN2_EINVAL;
    if (B == 0 && R == 0) return 0;
    const int grid = R > 0 ? loss_grid(R) : 1;
    hipStream_t st = (hipStream_t)stream;
    const float4* p4 = reinterpret_cast<const float4*>(proba);
    float4* d4 = reinterpret_cast<float4*>(dproba);
    float* dp = B > 0 ? dpred : nullptr;
    pl_for_terms(nll, ent, [&](auto NLL, auto ENT) {
        hipLaunchKernelGGL((loss_bwd_kernel<NLL(), ENT()>), dim3(grid), dim3(256), 0, st, pred, gt, B, p4, pdf, R, m, e, grad_total, dp, d4);
    });
    SN2_RETURN_LAUNCH();
}

extern "C" int sn2_kde_lookup(const float* cloud, int B, int C, int N, int z_channel, float z_max, const double* X,
                              const double* Y, int K, double* pdf, void* stream) {
    if (!cloud || !X || !Y || !pdf || B <= 0 || C <= 0 || N <= 0 || z_channel < 0 || z_channel >= C || K < 2) return SN2_EINVAL;
    const long R = (long)B * N;
    hipLaunchKernelGGL(kde_lookup_kernel, dim3(sn2_cdiv(R, 256)), dim3(256), 0, (hipStream_t)stream, cloud, C, N, z_channel,
                       z_max, X, Y, K, R, pdf);
    SN2_RETURN_LAUNCH();
}
