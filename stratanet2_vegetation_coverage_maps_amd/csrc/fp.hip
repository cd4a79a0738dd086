// fp.hip -- dense-row (Linear->ReLU->BN) blocks with interpolated + skip inputs, forward and backward, in three forms
// (row per lane, the 64-row matrix-core "split" kernels of the small layers, the source-side form of the per-point layer)
// and their dispatch.  Replaces FPModule.forward (knn_interpolate's differentiable half + cat + MLP) and GlobalSAModule's MLP:
// model/point_net2.py:37-42, 62-67 of the reference.  The pointwise head is head.hip, the one-launch global level
// global_level.hip, the inverted interpolation index interp_index.hip; what they share with this file is fp_rows.h.
//
// One row per lane.  A row's input u = [ interp (ca) | skip (cb) ] is rebuilt in registers from the 1 or 3 source rows
// (16-byte gathers out of an L2-resident table), the Linear layer runs against wave-uniform weights (SGPR operands),
// the pre-BN activation h is stored once (row stride padded to 16 B) and its batch statistics are reduced per wave and
// added as fp64 atomics.  Consumers apply the BN affine (a, c) when they read h, so no BN-apply pass exists.
// Backward: (1) dgamma/dbeta reduction over rows, (2) main pass: dpre, dW|db through the MFMA outer-product accumulator
// (rows = MFMA K), input gradient du; (3) the interpolation's transpose as a gather through an inverted index (no
// floating-point atomics: see "backward (3)" in interp_index.hip).
#include "fp_rows.h"

// the two form switches declared in fp_rows.h (sn2_fp_head_eval in head.hip reads the first, launch_src_table the second)
int g_fp_rows_form = 1;
int g_fp_table_form = 1;

namespace {

template <int CA, int CB, bool KNN>
__device__ __forceinline__ void build_input(const float* __restrict__ src, int src_stride, cfp src_a, cfp src_c,
                                            const int* __restrict__ knn_idx,
                                            const float* __restrict__ knn_w, const float* __restrict__ skip,
                                            int skip_stride, size_t r, size_t src_plot_base, float (&u)[CA + CB + 1]) {
    constexpr int Q = (CA + 3) / 4;
    if constexpr (KNN) {
        const int i0 = knn_idx[r * 3 + 0], i1 = knn_idx[r * 3 + 1], i2 = knn_idx[r * 3 + 2];
        const float w0 = knn_w[r * 3 + 0], w1 = knn_w[r * 3 + 1], w2 = knn_w[r * 3 + 2];
        const float inv = 1.0f / ((w0 + w1) + w2);
        const float4* s0 = reinterpret_cast<const float4*>(src + (src_plot_base + i0) * src_stride);
        const float4* s1 = reinterpret_cast<const float4*>(src + (src_plot_base + i1) * src_stride);
        const float4* s2 = reinterpret_cast<const float4*>(src + (src_plot_base + i2) * src_stride);
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float4 a = s0[q], b = s1[q], c = s2[q];
            const float v[4] = {(a.x * w0 + b.x * w1) + c.x * w2, (a.y * w0 + b.y * w1) + c.y * w2,
                                (a.z * w0 + b.z * w1) + c.z * w2, (a.w * w0 + b.w * w1) + c.w * w2};
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (4 * q + t < CA) u[4 * q + t] = v[t] * inv;
        }
    } else {
        const float4* s0 = reinterpret_cast<const float4*>(src + r * src_stride);
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float4 a = s0[q];
            const float v[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (4 * q + t < CA) u[4 * q + t] = v[t];
        }
    }
    if (src_a) {
#pragma unroll
        for (int k = 0; k < CA; ++k) u[k] = fmaf(src_a[k], u[k], src_c[k]);
    }
    if constexpr (CB > 0) {
        const float* sk = skip + r * skip_stride;
        if constexpr (CB % 4 == 0) {
#pragma unroll
            for (int q = 0; q < CB / 4; ++q) {
                const float4 a = reinterpret_cast<const float4*>(sk)[q];
                u[CA + 4 * q + 0] = a.x;
                u[CA + 4 * q + 1] = a.y;
                u[CA + 4 * q + 2] = a.z;
                u[CA + 4 * q + 3] = a.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < CB; ++k) u[CA + k] = sk[k];
        }
    }
    u[CA + CB] = 1.0f;  // the bias column of the outer-product accumulator
}

// ---------------------------------------------------------------------------------------------- forward
template <int CA, int CB, int CO, bool KNN>
__global__ __launch_bounds__(256) void fp_fwd_kernel(int R, int R_per_plot, int S_per_plot, int src_stride, int skip_stride,
                                                     int h_stride, const float* __restrict__ src,
                                                     const float* __restrict__ src_a, const float* __restrict__ src_c,
                                                     const int* __restrict__ knn_idx, const float* __restrict__ knn_w,
                                                     const float* __restrict__ skip, const float* __restrict__ Wg,
                                                     const float* __restrict__ biasg, float* __restrict__ h,
                                                     float* __restrict__ slots) {
    constexpr int CI = CA + CB;
    __shared__ float s_red[4 * 2 * CO];
    float ssum[CO], ssq[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) ssum[o] = ssq[o] = 0.f;
    for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < R; r += (long)gridDim.x * 256) {
        const cfp W = opaque(as_const(Wg)), bias = opaque(as_const(biasg));   // stream the weights inside the loop
        float u[CI + 1];
        const size_t plot = (size_t)(r / R_per_plot);
        build_input<CA, CB, KNN>(src, src_stride, opaque(as_const(src_a)), opaque(as_const(src_c)), knn_idx, knn_w, skip,
                                 skip_stride, (size_t)r, plot * S_per_plot, u);
        float* hr = h + (size_t)r * h_stride;
#pragma unroll
        for (int o4 = 0; o4 < CO; o4 += 4) {
            float v[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int o = o4 + t;
                float acc = 0.f;
                if (o < CO) {
                    acc = bias[o];
#pragma unroll
                    for (int k = 0; k < CI; ++k) acc = fmaf(W[o * CI + k], u[k], acc);
                    acc = fmaxf(acc, 0.f);
                    ssum[o] += acc;
                    ssq[o] = fmaf(acc, acc, ssq[o]);
                }
                v[t] = acc;
            }
            *reinterpret_cast<float4*>(hr + o4) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
    if (slots) stats_to_slot<CO>(ssum, ssq, s_red, slots);
}

// ---------------------------------------------------------------------------------------------- backward (1)
// dbeta[o] = sum_r dy[r][o];  dgamma[o] = sum_r dy[r][o] * (h[r][o] - mean[o]) * invstd[o]
template <int CO>
__global__ __launch_bounds__(256) void fp_bwd_bn_kernel(int R, int h_stride, const float* __restrict__ h,
                                                        const float* __restrict__ dy, const float* __restrict__ mean,
                                                        const float* __restrict__ invstd, float* __restrict__ dgamma,
                                                        float* __restrict__ dbeta, const int* __restrict__ done) {
    if (done && *done == 1) return;                   // the sums already came from the consumer's gradients
    float sb[CO], sg[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) sb[o] = sg[o] = 0.f;
    for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < R; r += (long)gridDim.x * 256) {
        const float4* hr = reinterpret_cast<const float4*>(h + (size_t)r * h_stride);
        const float4* dr = reinterpret_cast<const float4*>(dy + (size_t)r * h_stride);
#pragma unroll
        for (int q = 0; q < (CO + 3) / 4; ++q) {
            const float4 hv = hr[q], dv = dr[q];
            const float hh[4] = {hv.x, hv.y, hv.z, hv.w}, dd[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int o = 4 * q + t;
                if (o < CO) {
                    sb[o] += dd[t];
                    sg[o] = fmaf(dd[t], (hh[t] - mean[o]) * invstd[o], sg[o]);
                }
            }
        }
    }
    __shared__ float s_red[2 * CO];
    for (int i = threadIdx.x; i < 2 * CO; i += 256) s_red[i] = 0.f;
    __syncthreads();
    sums_to_lds<CO>(sb, s_red);
    sums_to_lds<CO>(sg, s_red + CO);
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * CO; i += 256) {
        const float v = s_red[i];
        if (v != 0.f) atomicAdd(i < CO ? &dbeta[i] : &dgamma[i - CO], v);
    }
}

// the same sums for the small layers (4k-16k rows): lane = channel, wave = row subgroup, 64 rows per workgroup -- coalesced
// row reads, no cross-lane reduction (the row-per-lane form spent ~20 us per launch on 128 wave reductions for 1 MB)
template <int CO>
__global__ __launch_bounds__(256) void fp_bwd_bn_small_kernel(int R, int h_stride, const float* __restrict__ h,
                                                              const float* __restrict__ dy, const float* __restrict__ mean,
                                                              const float* __restrict__ invstd, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta, const int* __restrict__ done) {
    static_assert(CO <= 64, "one lane per channel");
    if (done && *done == 1) return;
    __shared__ float s_part[2][4][64];
    const int o = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool on = o < CO;
    const float mu = on ? mean[o] : 0.f, is = on ? invstd[o] : 0.f;
    float sb = 0.f, sg = 0.f;
    const long r0 = (long)blockIdx.x * 64;
    float hv[16], dv[16];                               // all 32 loads in flight (four at a time: 10.7 us for 4096 rows)
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const long r = r0 + w + 4 * u;
        const bool ok = r < R && on;
        hv[u] = ok ? h[(size_t)r * h_stride + o] : mu;
        dv[u] = ok ? dy[(size_t)r * h_stride + o] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        sb += dv[u];
        sg = fmaf(dv[u], (hv[u] - mu) * is, sg);
    }
    s_part[0][w][o] = sb;
    s_part[1][w][o] = sg;
    __syncthreads();
    if (threadIdx.x < 128) {
        const int which = threadIdx.x >> 6;
        if (on) {
            const float v = (s_part[which][0][o] + s_part[which][1][o]) + (s_part[which][2][o] + s_part[which][3][o]);
            if (v != 0.f) atomicAdd(which == 0 ? &dbeta[o] : &dgamma[o], v);
        }
    }
}

// ---------------------------------------------------------------------------------------------- backward (2)
template <int CA, int CB, int CO, bool KNN, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void fp_bwd_main_kernel(
    int R, int R_per_plot, int S_per_plot, int src_stride, int skip_stride, int h_stride, int dskip_stride,
    int du_stride, float invR,
    const float* __restrict__ src, const float* __restrict__ src_a, const float* __restrict__ src_c,
    const int* __restrict__ knn_idx, const float* __restrict__ knn_w, const float* __restrict__ skip,
    const float* __restrict__ Wg, const float* __restrict__ gammag, const float* __restrict__ meang,
    const float* __restrict__ invstdg, const float* __restrict__ dgammag, const float* __restrict__ dbetag,
    const float* __restrict__ h, const float* __restrict__ dy, float* __restrict__ dW, float* __restrict__ db,
    float* __restrict__ du_out /* KNN: (R,CA) scratch; else ACCUMULATED rows (R,du_stride) */,
    float* __restrict__ dskip, int rep_k, int rep_stride) {
    constexpr int CI = CA + CB;
    using Acc = OuterAcc<CO, CI + 1, 32>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* lds = smem + (threadIdx.x >> 6) * Acc::LDS_FLOATS;
    Acc acc;
    acc.init(lds);
    // W as the B operand of the input-gradient product: lane (qq, cc) keeps W[o = 4 kb + qq][col = 16 jt + cc]
    constexpr int KBO = (CO + 3) / 4, TJ = (CI + 15) / 16;
    const int qq = (threadIdx.x & 63) >> 4, cc = threadIdx.x & 15;
    float Wb[KBO][TJ];
#pragma unroll
    for (int kb = 0; kb < KBO; ++kb)
#pragma unroll
        for (int jt = 0; jt < TJ; ++jt) {
            const int o = 4 * kb + qq, col = 16 * jt + cc;
            Wb[kb][jt] = (o < CO && col < CI) ? Wg[o * CI + col] : 0.f;
        }
    const long nthreads = (long)gridDim.x * WAVES * 64;
    const long rounds = (R + nthreads - 1) / nthreads;  // every lane of a wave runs the same number of rounds
    for (long it = 0; it < rounds; ++it) {
        const long r = it * nthreads + (long)blockIdx.x * WAVES * 64 + threadIdx.x;
        const bool valid = r < R;
        const size_t rr = valid ? (size_t)r : 0;
        const cfp W = opaque(as_const(Wg)), gamma = opaque(as_const(gammag)), mean = opaque(as_const(meang)),
                  invstd = opaque(as_const(invstdg)), dgamma = opaque(as_const(dgammag)), dbeta = opaque(as_const(dbetag));
        float u[CI + 1];
        build_input<CA, CB, KNN>(src, src_stride, opaque(as_const(src_a)), opaque(as_const(src_c)), knn_idx, knn_w, skip,
                                 skip_stride, rr, (rr / R_per_plot) * S_per_plot, u);
        float dp[CO];
        const float4* hr = reinterpret_cast<const float4*>(h + rr * h_stride);
        const float4* dr = reinterpret_cast<const float4*>(dy + rr * h_stride);
#pragma unroll
        for (int q = 0; q < (CO + 3) / 4; ++q) {
            const float4 hv = hr[q], dv = dr[q];
            const float hh[4] = {hv.x, hv.y, hv.z, hv.w}, dd[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int o = 4 * q + t;
                if (o < CO) {
                    const float is = invstd[o];
                    const float xh = (hh[t] - mean[o]) * is;
                    const float dh = gamma[o] * is * (dd[t] - dbeta[o] * invR - xh * dgamma[o] * invR);
                    dp[o] = (valid && hh[t] > 0.f) ? dh : 0.f;
                }
            }
        }
        // weight gradient: dW += dp^T [u | 1] over the wave's rows.  Input gradient: d[u] = dp W over the same staged dp
        // rows, also on the matrix cores -- A[row][o] read back from the staging region, B[o][col] = W in registers for the
        // whole kernel (as per-lane FMA chains this product was ~1400 FMAs per row fed by ~300 scalar loads of 16 dwords,
        // and the waves spent most of their time waiting for those loads).
        const long wave_row0 = it * nthreads + (long)blockIdx.x * WAVES * 64 + (threadIdx.x & ~63);
        acc.add_then(lds, dp, u, [&](int hph) __attribute__((always_inline)) {
            if (!du_out && !(CB > 0 && dskip)) return;
#pragma unroll
            for (int t = 0; t < Acc::STAGED_ROWS / 16; ++t) {
                f32x4 D[TJ];
#pragma unroll
                for (int jt = 0; jt < TJ; ++jt) D[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kb = 0; kb < KBO; ++kb) {
                    const float av = lds[(16 * t + cc) * Acc::PS + 4 * kb + qq];
#pragma unroll
                    for (int jt = 0; jt < TJ; ++jt) D[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Wb[kb][jt], D[jt], 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long row = wave_row0 + hph * Acc::STAGED_ROWS + 16 * t + 4 * qq + r;
                    if (row >= R) continue;
#pragma unroll
                    for (int jt = 0; jt < TJ; ++jt) {
                        const int col = 16 * jt + cc;
                        if (col < CA) {
                            if (du_out) {
                                float* dst = du_out + (size_t)row * du_stride + col;
                                if constexpr (KNN) *dst = D[jt][r];
                                else *dst += D[jt][r];
                            }
                        } else if (col < CI) {
                            if constexpr (CB > 0) {
                                if (dskip) dskip[(size_t)row * dskip_stride + (col - CA)] += D[jt][r];
                            }
                        }
                    }
                }
            }
        });
    }
    // workgroup-level reduction of the [dW | db] image (every wave's slab in its own staging region, added in wave order;
    // LDS float atomics where a slab does not fit the region), then one global atomic per element and workgroup
    constexpr bool SLAB = CO * (CI + 1) <= Acc::LDS_FLOATS;
    float* red = smem;
    if constexpr (SLAB) {
        acc.store_slab(lds);
        __syncthreads();
    } else {
        __syncthreads();
        for (int i = threadIdx.x; i < CO * (CI + 1); i += WAVES * 64) red[i] = 0.f;
        __syncthreads();
        acc.flush_lds(red);
        __syncthreads();
    }
    for (int i = threadIdx.x; i < CO * (CI + 1); i += WAVES * 64) {
        float v = 0.f;
        if constexpr (SLAB) {
#pragma unroll
            for (int w = 0; w < WAVES; ++w) v += smem[w * Acc::LDS_FLOATS + i];
        } else {
            v = red[i];
        }
        if (v == 0.f) continue;
        const int o = i / (CI + 1), k = i - o * (CI + 1), img = sn2_grad_image(rep_k, rep_stride);
        if (k < CI) SN2_FLUSH_ADD(&dW[img + o * CI + k], v);
        else SN2_FLUSH_ADD(&db[img + o], v);
    }
}

// ---------------------------------------------------------------------------------------------- backward (3)
// Step D of the interpolation's transpose (steps A-C, the inverted index, and the reasons: interp_index.hip): one wave per
// source row, lane = channel: coalesced du rows, accumulation in registers, one plain store.
template <int CA>
__global__ __launch_bounds__(256) void interp_gather_kernel(int n_src, int R_per_plot, int S, int dsrc_stride,
                                                            const int* __restrict__ off, const int* __restrict__ cnt,
                                                            const int* __restrict__ inv_row, const float* __restrict__ inv_w,
                                                            const float* __restrict__ du, float* __restrict__ dsrc) {
    const int lane = threadIdx.x & 63;
    const int s = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (s >= n_src) return;
    const int b = s / S;
    const int n = cnt[s], st = off[s];
    const float* dub = du + (size_t)b * R_per_plot * CA;
    const bool on = lane < CA;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f;
    // The list is ~96 entries long and every entry is one 136-byte row somewhere in a 70 MB array: pure latency.  64 list
    // entries are fetched with one coalesced load (lane j keeps entry j, broadcast by v_readlane), then eight independent
    // row loads are in flight at a time (four gave 1.7 TB/s).
    for (int base = 0; base < n; base += 64) {
        const int m = (n - base) < 64 ? (n - base) : 64;
        const int rj = lane < m ? inv_row[st + base + lane] : 0;          // entries past the end: row 0 with weight 0
        const float wj = lane < m ? inv_w[st + base + lane] : 0.f;
        for (int i = 0; i < m; i += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int r = __builtin_amdgcn_readlane(rj, i + u);
                v[u] = on ? dub[(size_t)r * CA + lane] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; u += 4) {
                g0 = fmaf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(wj), i + u)), v[u], g0);
                g1 = fmaf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(wj), i + u + 1)), v[u + 1], g1);
                g2 = fmaf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(wj), i + u + 2)), v[u + 2], g2);
                g3 = fmaf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(wj), i + u + 3)), v[u + 3], g3);
            }
        }
    }
    if (on) dsrc[(size_t)s * dsrc_stride + lane] += (g0 + g1) + (g2 + g3);
}

// The same for LONG lists (the global level: one source per plot, every target row on its list): one workgroup of WAVES
// waves per source, wave w takes the entries w, w + WAVES, ... in blocks of 64, the partial sums are added in wave order
// (one wave walking 256 entries, eight in flight, took 15 us).
template <int CA, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void interp_gather_long_kernel(int n_src, int R_per_plot, int S, int dsrc_stride,
                                                                        const int* __restrict__ off, const int* __restrict__ cnt,
                                                                        const int* __restrict__ inv_row,
                                                                        const float* __restrict__ inv_w,
                                                                        const float* __restrict__ du, float* __restrict__ dsrc) {
    __shared__ float s_part[WAVES][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int s = blockIdx.x;
    const int b = s / S;
    const int n = cnt[s], st = off[s];
    const float* dub = du + (size_t)b * R_per_plot * CA;
    const bool on = lane < CA;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f;
    for (int base = wave * 8; base < n; base += WAVES * 8) {           // eight entries per wave and turn, all in flight
        const int m = (n - base) < 8 ? (n - base) : 8;
        const int rj = lane < m ? inv_row[st + base + lane] : 0;        // entries past the end: row 0 with weight 0
        const float wj = lane < m ? inv_w[st + base + lane] : 0.f;
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int r = __builtin_amdgcn_readlane(rj, u);
            v[u] = on ? dub[(size_t)r * CA + lane] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; u += 4) {
            g0 = fmaf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(wj), u)), v[u], g0);
            g1 = fmaf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(wj), u + 1)), v[u + 1], g1);
            g2 = fmaf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(wj), u + 2)), v[u + 2], g2);
            g3 = fmaf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(wj), u + 3)), v[u + 3], g3);
        }
    }
    s_part[wave][lane] = (g0 + g1) + (g2 + g3);
    __syncthreads();
    if (wave == 0 && on) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) t += s_part[w][lane];
        dsrc[(size_t)s * dsrc_stride + lane] += t;
    }
}

// ---------------------------------------------------------------------------------------------- source-side form
// The per-point layer (FP1: 524 288 rows interpolating 16 384 source rows) spent most of its time on work that is linear
// in the interpolation and can be done once per SOURCE row instead of once per target row:
//   W_A u_r = W_A (a o sum_j w_rj src[i_rj] + c) = sum_j w_rj T[i_rj],   T[s] = W_A (a o src[s] + c)      (sum_j w_rj = 1)
//   dsrc[s] = sum_{r,j: i_rj = s} w_rj dp_r W_A = G[s] W_A,              G[s] = sum_{r,j: i_rj = s} w_rj dp_r
//   dW_A    = sum_r dp_r^T u_r = sum_s G[s]^T (a o src[s] + c)
// so the row side keeps only the skip columns (CB = 8 of 42 inputs: 5x fewer multiply-adds) and becomes a streaming pass:
//   forward : T (n_src x CO, one small kernel), then per row 3 gathers of T rows + W_B skip + b -> relu -> h, statistics
//   backward: rows: dp = BN/ReLU backward of dy (stored once), dW_B | db;  sources: G (gather of dp rows through the
//             inverted index), dsrc += G W_A;  dW_A += G^T (a o src + c) on the matrix cores over the n_src rows.
// The row kernels use QH = ceil(CO/4) consecutive lanes per row, one float4 quad each: a load or store instruction covers
// 64/QH whole rows = ~1 KB of consecutive bytes, and nothing but the lane's own quad constants lives in registers.
// Results differ from the row-per-lane form by fp32 re-association only.
// (the rows' accessors, the source table, the input stream and the (row, quad) arithmetic of the row passes: fp_rows.h)

// batch statistics of a row pass (256 lanes, QH lanes per row, lane (g, q) holding the sums of channels 4 q .. 4 q + 3 over its
// rows): per-lane partials -> LDS -> one slot per workgroup ([sum(C) | sumsq(C)], as stats_to_slot)
template <int CO>
__device__ __forceinline__ void row_quads_stats_to_slot(float (&s_part)[8][256], bool on, const float (&ssum)[4], const float (&ssq)[4],
                                                        float* __restrict__ slots) {
    constexpr int QH = (CO + 3) / 4, G = 64 / QH;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        s_part[t][threadIdx.x] = on ? ssum[t] : 0.f;
        s_part[4 + t][threadIdx.x] = on ? ssq[t] : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * CO; e += 256) {
        const int which = e / CO, c = e - which * CO, cq = c >> 2, ct = c & 3;
        float acc = 0.f;
        for (int w = 0; w < 4; ++w)
            for (int gg = 0; gg < G; ++gg) acc += s_part[which * 4 + ct][w * 64 + cq + QH * gg];
        slots[(size_t)blockIdx.x * 2 * CO + e] = acc;
    }
}

template <int CA, int CB, int CO, bool BF>
__global__ __launch_bounds__(256) void fp_fwd_rows_kernel(int R, int R_per_plot, int S_per_plot, int skip_stride,
                                                          const float* __restrict__ T, const int* __restrict__ knn_idx,
                                                          const float* __restrict__ knn_w, const float* __restrict__ skip,
                                                          const float* __restrict__ Wg, const float* __restrict__ biasg,
                                                          float* __restrict__ h, float* __restrict__ slots) {
    constexpr int QH = (CO + 3) / 4, HS = 4 * QH, G = 64 / QH, QB = CB / 4, U = 2;
    static_assert(CB > 0 && CB % 4 == 0, "skip quads");
    __shared__ float s_part[8][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane % QH, g = lane / QH;
    const bool on = lane < G * QH;
    const FpQuadW<CB> fw = fp_quad_w<CA, CB, CO>(Wg, biasg, q);
    float ssum[4] = {0.f, 0.f, 0.f, 0.f}, ssq[4] = {0.f, 0.f, 0.f, 0.f};
    // (a wave's turn = U groups of G rows = one "iteration" of row_iters)
    const RowIters ri = row_iters((int)(((long)R + G * U - 1) / (G * U)), wave);
    const long n_grp_all = ((long)R + G - 1) / G;
    const long n_grp = n_grp_all < (long)ri.it_hi * U ? n_grp_all : (long)ri.it_hi * U;
    const long n_waves = ri.stride;
    long grp0 = (long)ri.it0 * U;
    // the 3-NN entries and skip columns run one iteration ahead of the gathers that depend on them
    FpRowIn<QB> nx[U];
#pragma unroll
    for (int u = 0; u < U; ++u) nx[u] = fp_row_in<QB>((grp0 + u) * G + g, on && grp0 < n_grp, R, knn_idx, knn_w, skip, skip_stride);
    for (; grp0 < n_grp; grp0 += n_waves * U) {
        FpRowIn<QB> in[U];
        float4 ta[U][3];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            in[u] = nx[u];
            fp_table_rows<HS>(T, (in[u].rr / (unsigned)R_per_plot) * (unsigned)S_per_plot, in[u].i0, in[u].i1, in[u].i2, q, ta[u]);
        }
        const long grp1 = grp0 + n_waves * U;
#pragma unroll
        for (int u = 0; u < U; ++u) nx[u] = fp_row_in<QB>((grp1 + u) * G + g, on && grp1 < n_grp, R, knn_idx, knn_w, skip, skip_stride);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float v[4];
            fp_row_quad<CB, CO>(fw, ta[u], in[u].w0, in[u].w1, in[u].w2, in[u].sk, in[u].valid, q, v);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if constexpr (BF) v[t] = bf16_round(v[t]);   // the batch statistics describe the rows as they are stored
                ssum[t] += v[t];
                ssq[t] = fmaf(v[t], v[t], ssq[t]);
            }
#if defined(SN2_FR_DIAG) && (SN2_FR_DIAG & 1)
            if (in[u].valid && v[0] == 12345.678f) row_quad_st<BF>(h, in[u].rr, HS, q, v[0], v[1], v[2], v[3]);   // (diagnostic: no stores)
#else
            if (in[u].valid) row_quad_st<BF>(h, in[u].rr, HS, q, v[0], v[1], v[2], v[3]);
#endif
        }
    }
    if (slots) row_quads_stats_to_slot<CO>(s_part, on, ssum, ssq, slots);
}

// The same row pass with its INPUT STREAM decoupled from the lanes that consume it (round 5).  fp_fwd_rows_kernel's nine lanes of a
// row each load the row's 3-NN entry and skip columns themselves, one iteration ahead: 16 registers per row and stage, so one
// stage is all that fits, and a wave's iteration (14 rows, ~0.3 us of arithmetic) then waits out a memory round trip (~1 us):
// with every load and store but these switched off the kernel still took 18 us for 29 MB (scripts/time_fp1.py; 2048 waves x
// 784 B in flight = 1.6 MB: Little's law).  Here a wave fetches an iteration's 42 indices, 42 weights and 14 x QB skip quads
// with ONE element per lane (three load instructions, six registers per stage), FP_ROWS_PD iterations ahead, hands them to the
// (row, quad) lanes through a wave-private LDS region, and asks for the NEXT iteration's table rows before it computes the
// current one.  Same rows per wave, same lane mapping, same arithmetic in the same order as fp_fwd_rows_kernel: same bits,
// statistics slots included.
#ifndef SN2_FR_PD
#define SN2_FR_PD 2       // (2 / 4 / 6 stages: FP1's forward entry 41.1 / 42.3 / 44.5 us at config 2 -- more in flight is not faster here)
#endif
#ifndef SN2_FR_OCC
#define SN2_FR_OCC 2
#endif
constexpr int FP_ROWS_PD = SN2_FR_PD;
template <class F, int... I>
__device__ __forceinline__ void for_each_stage(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int CA, int CB, int CO, bool BF>
__global__ __launch_bounds__(256, SN2_FR_OCC) void fp_fwd_rows2_kernel(int R, int R_per_plot, int S_per_plot, int skip_stride,
                                                              const float* __restrict__ T, const int* __restrict__ knn_idx,
                                                              const float* __restrict__ knn_w, const float* __restrict__ skip,
                                                              const float* __restrict__ Wg, const float* __restrict__ biasg,
                                                              float* __restrict__ h, float* __restrict__ slots) {
    constexpr int CI = CA + CB, QH = (CO + 3) / 4, HS = 4 * QH, G = 64 / QH, QB = CB / 4, U = 2, RPI = G * U, PD = FP_ROWS_PD;
    static_assert(CB > 0 && CB % 4 == 0, "skip quads");
    static_assert(3 * RPI <= 64 && RPI * QB <= 64, "an iteration's inputs are one element per lane");
    static_assert(PD % 2 == 0, "the two exchange regions alternate over the stages");
    constexpr int LW = 3 * RPI + 3 * RPI + 4 * RPI * QB;                  // words of an exchange region: idx | w | skip quads
    constexpr int LWP = (LW + 3) / 4 * 4;
    static_assert((6 * RPI) % 4 == 0, "the skip quads start 16-byte aligned");
    __shared__ float s_part[8][256];
    __shared__ __attribute__((aligned(16))) float s_x[4][2][LWP];         // per wave: two regions (this iteration's, the next one's)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane % QH, g = lane / QH;
    const bool on = lane < G * QH;
    // channel PAIRS (4 q + 2 pr, + 1): the skip weights, the bias and the statistics, for the packed fp32 instructions
    f32x2 wB[2][CB], b4[2];
#pragma unroll
    for (int pr = 0; pr < 2; ++pr)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int o = 4 * q + 2 * pr + e;
            b4[pr][e] = o < CO ? biasg[o] : 0.f;
#pragma unroll
            for (int k = 0; k < CB; ++k) wB[pr][k][e] = o < CO ? Wg[o * CI + CA + k] : 0.f;
        }
    f32x2 ssum[2] = {{0.f, 0.f}, {0.f, 0.f}}, ssq[2] = {{0.f, 0.f}, {0.f, 0.f}};
    const int n_it_all = (R + RPI - 1) / RPI;                              // iterations: RPI consecutive rows each (3 R < 2^31)
    const RowIters ri = row_iters(n_it_all, wave);
    const int n_it = ri.it_hi, n_waves = ri.stride, it0 = ri.it0;          // this wave's iterations: it0 + k n_waves < n_it
    // ---- the input stream: one element per lane and stage
    typedef float f32x4 __attribute__((ext_vector_type(4)));              // (an array of HIP's float4 STRUCT stayed in scratch memory)
    int p_idx[PD];
    float p_w[PD];
    f32x4 p_sk[PD];
    // (every load of the steady state is UNCONDITIONAL, its address clamped into the arrays: a branch around a load makes the
    // compiler's count of outstanding memory operations unknown and it answers with s_waitcnt vmcnt(0) -- the first version of this
    // kernel drained its whole pipeline 24 times per unrolled body and ran 2 us faster than the kernel it replaces, not 10)
    const int last_e = 3 * R - 1, last_it = n_it - 1;
    const int lane_e = lane < 3 * RPI ? lane : 3 * RPI - 1, lane_s = lane < RPI * QB ? lane : RPI * QB - 1;
    auto fetch = [&](auto S, int it) {
        constexpr int s = decltype(S)::value;            // (a run-time stage index left the stage registers in scratch memory)
        const int itc = it < last_it ? it : last_it;
        const int e0 = itc * (3 * RPI) + lane_e, e = e0 < last_e ? e0 : last_e;
        p_idx[s] = knn_idx[e];
        p_w[s] = knn_w[e];
        const int rs0 = itc * RPI + lane_s / QB, rs = rs0 < R ? rs0 : R - 1;
        p_sk[s] = reinterpret_cast<const f32x4*>(skip + (size_t)rs * skip_stride)[lane_s % QB];
    };
    // stage s -> exchange region `buf`; the (row, quad) lanes read their rows' indices back and ask for the table rows
    auto hand_over = [&](auto S, int buf, int it, float4 (&ta)[U][3]) {
        constexpr int s = decltype(S)::value;
        float* xw = s_x[wave][buf];
        xw[lane_e] = __int_as_float(p_idx[s]);                             // (the surplus lanes hold a copy of the last element)
        xw[3 * RPI + lane_e] = p_w[s];
        reinterpret_cast<f32x4*>(xw + 6 * RPI)[lane_s] = p_sk[s];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int rl = on ? G * u + g : 0;                              // row of the iteration
            const int row = it * RPI + rl;
            const bool valid = on && row < R && it < n_it;
            const unsigned rr = valid ? (unsigned)row : 0u;
            const int i0 = valid ? __float_as_int(xw[3 * rl + 0]) : 0, i1 = valid ? __float_as_int(xw[3 * rl + 1]) : 0,
                      i2 = valid ? __float_as_int(xw[3 * rl + 2]) : 0;
            fp_table_rows<HS>(T, (rr / (unsigned)R_per_plot) * (unsigned)S_per_plot, i0, i1, i2, q, ta[u]);
        }
    };
    auto compute = [&](int buf, int it, const float4 (&ta)[U][3]) {
        const float* xw = s_x[wave][buf];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int rl = on ? G * u + g : 0;
            const int row = it * RPI + rl;
            const bool valid = on && row < R && it < n_it;
            const float w0 = xw[3 * RPI + 3 * rl + 0], w1 = xw[3 * RPI + 3 * rl + 1], w2 = xw[3 * RPI + 3 * rl + 2];
            float4 sk[QB];
#pragma unroll
            for (int b = 0; b < QB; ++b) sk[b] = reinterpret_cast<const float4*>(xw + 6 * RPI)[rl * QB + b];
            const float inv = 1.0f / ((w0 + w1) + w2);
            const float4 a = ta[u][0], b = ta[u][1], c = ta[u][2];
            const f32x2 a2[2] = {{a.x, a.y}, {a.z, a.w}}, b2[2] = {{b.x, b.y}, {b.z, b.w}}, c2[2] = {{c.x, c.y}, {c.z, c.w}};
            float v[4];
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) {
                f32x2 acc = interp_bias2(a2[pr], b2[pr], c2[pr], w0, w1, w2, inv, b4[pr]);
#if defined(SN2_FR_DIAG) && (SN2_FR_DIAG & 4)
                acc += (f32x2){sk[0].x + sk[QB - 1].w, sk[0].x};             // (diagnostic: no skip contraction)
#else
#pragma unroll
                for (int k4 = 0; k4 < QB; ++k4) {
                    acc = __builtin_elementwise_fma(wB[pr][4 * k4 + 0], (f32x2){sk[k4].x, sk[k4].x}, acc);
                    acc = __builtin_elementwise_fma(wB[pr][4 * k4 + 1], (f32x2){sk[k4].y, sk[k4].y}, acc);
                    acc = __builtin_elementwise_fma(wB[pr][4 * k4 + 2], (f32x2){sk[k4].z, sk[k4].z}, acc);
                    acc = __builtin_elementwise_fma(wB[pr][4 * k4 + 3], (f32x2){sk[k4].w, sk[k4].w}, acc);
                }
#endif
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    float x = (valid && 4 * q + 2 * pr + e < CO) ? fmaxf(acc[e], 0.f) : 0.f;
                    if constexpr (BF) x = bf16_round(x);     // the batch statistics describe the rows as they are stored
                    acc[e] = x;
                    v[2 * pr + e] = x;
                }
                ssum[pr] += acc;
                ssq[pr] = __builtin_elementwise_fma(acc, acc, ssq[pr]);
            }
#if defined(SN2_FR_DIAG) && (SN2_FR_DIAG & 1)
            if (valid && v[0] == 12345.678f) row_quad_st<BF>(h, (size_t)row, HS, q, v[0], v[1], v[2], v[3]);   // (diagnostic: no stores)
#else
            if (valid) row_quad_st<BF>(h, (size_t)row, HS, q, v[0], v[1], v[2], v[3]);
#endif
        }
    };
    // this wave's iterations, rounded up to whole blocks of PD: the surplus ones have no valid row (nothing stored, zeros added to
    // the statistics) and keep the loop body free of branches
    const int n_mine = it0 < n_it ? (n_it - it0 + n_waves - 1) / n_waves : 0;
    const int n_blocks = (n_mine + PD - 1) / PD;
    if (n_blocks > 0) {
        using S0 = std::integral_constant<int, 0>;
        using Stages = std::make_integer_sequence<int, PD>;
        for_each_stage([&](auto S) { fetch(S, it0 + decltype(S)::value * n_waves); }, Stages{});
        float4 ta_a[U][3], ta_b[U][3];
        hand_over(S0{}, 0, it0, ta_a);
        fetch(S0{}, it0 + PD * n_waves);
        // the stage of an iteration is its count modulo PD; exchange region and table-row set = its parity.  One step: hand over the
        // NEXT iteration's inputs (its table rows are then on their way), refill that stage, compute THIS iteration
        auto step = [&](auto S, int kb) {
            constexpr int st = decltype(S)::value;
            using SN = std::integral_constant<int, (st + 1) % PD>;
            const int it = it0 + (kb * PD + st) * n_waves, itn = it + n_waves;
            if constexpr (st % 2 == 0) {
                hand_over(SN{}, 1, itn, ta_b);
                fetch(SN{}, itn + PD * n_waves);
                compute(0, it, ta_a);
            } else {
                hand_over(SN{}, 0, itn, ta_a);
                fetch(SN{}, itn + PD * n_waves);
                compute(1, it, ta_b);
            }
            // (this iteration's reads of its region lie in front of the hand-over that refills it, two iterations on)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        };
        for (int kb = 0; kb < n_blocks; ++kb) for_each_stage([&](auto S) { step(S, kb); }, Stages{});
    }
    if (!slots) return;
    const float s1[4] = {ssum[0][0], ssum[0][1], ssum[1][0], ssum[1][1]}, s2[4] = {ssq[0][0], ssq[0][1], ssq[1][0], ssq[1][1]};
    row_quads_stats_to_slot<CO>(s_part, on, s1, s2, slots);
}

// Where the d pre-activation rows of the source-side backward live (du_scratch).  With 33 or 34 channels a 36-float row
// straddles two 128-byte lines nearly always, and the source pass -- which gathers single rows from all over a 75 MB array --
// fetched both: 135 MB over the fabric for 75 MB of rows (PMC, round 3).  SPLIT layout for those widths: channels 0..31 of
// row r as ONE aligned line at main[r * 32] (bfloat16: 64 bytes), channels 32, 33 as a pair at side[r * 2] behind the
// R main rows (4.2 MB for the metric's batch: it stays in L2).  Other widths: plain rows of HS.
template <int CO>
constexpr bool dp_split() { return CO > 32 && CO <= 34; }
template <bool BF>
__device__ __forceinline__ void dp_side_st(float* __restrict__ dp, size_t R, size_t row, float a, float b) {
    if constexpr (BF) {
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        bf16x2 v;
        v[0] = (__bf16)a; v[1] = (__bf16)b;
        reinterpret_cast<unsigned*>(reinterpret_cast<unsigned short*>(dp) + R * 32)[row] = __builtin_bit_cast(unsigned, v);
    } else {
        reinterpret_cast<float2*>(dp + R * 32)[row] = make_float2(a, b);
    }
}
template <bool BF>
__device__ __forceinline__ float2 dp_side_ld(const float* __restrict__ dp, size_t R, size_t row) {
    if constexpr (BF) {
        const unsigned u = reinterpret_cast<const unsigned*>(reinterpret_cast<const unsigned short*>(dp) + R * 32)[row];
        return make_float2(__uint_as_float(u << 16), __uint_as_float(u & 0xFFFF0000u));
    } else {
        return reinterpret_cast<const float2*>(dp + R * 32)[row];
    }
}

// rows: dp = relu'/BN backward of dy (stored, row stride HS, pad channels 0), dW_B | db
template <int CA, int CB, int CO, int NT, bool BF>
__global__ __launch_bounds__(NT) void fp_bwd_rows_kernel(int R, int skip_stride, float invR, const float* __restrict__ skip,
                                                          const float* __restrict__ gammag, const float* __restrict__ meang,
                                                          const float* __restrict__ invstdg, const float* __restrict__ dgammag,
                                                          const float* __restrict__ dbetag, const float* __restrict__ h,
                                                          const float* __restrict__ dy, float* __restrict__ dp_out,
                                                          float* __restrict__ dW, float* __restrict__ db, int rep_k,
                                                          int rep_stride, const int* __restrict__ row_perm, int R_per_plot) {
    constexpr int CI = CA + CB, QH = (CO + 3) / 4, HS = 4 * QH, G = 64 / QH, QB = CB / 4, U = 2, NV = 4 * (CB + 1);
    static_assert(CB > 0 && CB % 4 == 0, "skip quads");
    extern __shared__ __attribute__((aligned(16))) float smem[];   // [NT / 64][HS][CB + 1]: the waves' sums
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane % QH, g = lane / QH;
    const bool on = lane < G * QH;
    float c_is[4], c_mu[4], c_gis[4], c_dbR[4], c_dg[4];
    bool ch[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int o = 4 * q + t;
        ch[t] = o < CO;
        const int oo = ch[t] ? o : 0;
        c_is[t] = invstdg[oo];
        c_mu[t] = meang[oo];
        c_gis[t] = gammag[oo] * c_is[t];
        c_dbR[t] = dbetag[oo] * invR;
        c_dg[t] = dgammag[oo];
    }
    float aW[4][CB], ab[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        ab[t] = 0.f;
#pragma unroll
        for (int k = 0; k < CB; ++k) aW[t][k] = 0.f;
    }
    // (round 5: dealing these rows XCD-aware as in the forward row pass -- XCD x then writes the d pre-activation rows of the plots whose
    // sources fp_bwd_src_chunk_kernel gathers from XCD x -- made the source pass 2 us faster (some of the rows are still in that L2)
    // and this pass 1.7 us slower: nothing in sum, scripts/time_fp1_bwd.py)
    const long n_grp = ((long)R + G - 1) / G;
    const long n_waves = (long)gridDim.x * (NT / 64);
    for (long grp0 = ((long)blockIdx.x * (NT / 64) + wave) * U; grp0 < n_grp; grp0 += n_waves * U) {
        float4 hv[U], dv[U], sk[U][QB];
        bool valid[U];
        unsigned rr[U], ro[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long row = (grp0 + u) * G + g;
            valid[u] = on && row < R;
            rr[u] = valid[u] ? (unsigned)row : 0u;
            // where the row's d pre-activation goes: its own place, or its plot's row_perm[] place (the source pass gathers
            // rows that are neighbours in space: along a space-filling curve they are neighbours in memory too)
            ro[u] = row_perm ? (rr[u] / (unsigned)R_per_plot) * (unsigned)R_per_plot + (unsigned)row_perm[rr[u]] : rr[u];
            hv[u] = row_quad_ld<BF>(h, rr[u], HS, q);
            dv[u] = row_quad_ld<BF>(dy, rr[u], HS, q);
#pragma unroll
            for (int b = 0; b < QB; ++b)
                sk[u][b] = reinterpret_cast<const float4*>(skip + (size_t)rr[u] * skip_stride)[b];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float hh[4] = {hv[u].x, hv[u].y, hv[u].z, hv[u].w}, dd[4] = {dv[u].x, dv[u].y, dv[u].z, dv[u].w};
            float d4[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float xh = (hh[t] - c_mu[t]) * c_is[t];
                const float dh = c_gis[t] * (dd[t] - c_dbR[t] - xh * c_dg[t] * invR);
                d4[t] = (valid[u] && ch[t] && hh[t] > 0.f) ? dh : 0.f;
                ab[t] += d4[t];
#pragma unroll
                for (int b = 0; b < QB; ++b) {
                    aW[t][4 * b + 0] = fmaf(d4[t], sk[u][b].x, aW[t][4 * b + 0]);
                    aW[t][4 * b + 1] = fmaf(d4[t], sk[u][b].y, aW[t][4 * b + 1]);
                    aW[t][4 * b + 2] = fmaf(d4[t], sk[u][b].z, aW[t][4 * b + 2]);
                    aW[t][4 * b + 3] = fmaf(d4[t], sk[u][b].w, aW[t][4 * b + 3]);
                }
            }
            if constexpr (dp_split<CO>()) {
                if (valid[u] && q < 8) row_quad_st<BF>(dp_out, ro[u], 32, q, d4[0], d4[1], d4[2], d4[3]);
                if (valid[u] && q == 8) dp_side_st<BF>(dp_out, (size_t)R, ro[u], d4[0], d4[1]);
            } else {
                if (valid[u]) row_quad_st<BF>(dp_out, ro[u], HS, q, d4[0], d4[1], d4[2], d4[3]);
            }
        }
    }
    // per-lane partials -> the wave's sums over its G row groups by lane shuffles (lanes q, q + QH, q + 2 QH, ... hold the same
    // channel quad) -> a [wave][channel][CB + 1] image in LDS (10 KB; all lanes' partials side by side were 74 KB per
    // workgroup: one workgroup per CU wherever an FPS workgroup holds its share of the LDS) -> one sum per element and
    // workgroup -> global atomics
    constexpr int NWV = NT / 64;
    static_assert(G <= 8, "three shuffle steps add up to eight row groups");
    float* red = smem;                                   // [NWV][HS][CB + 1]
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int k = 0; k <= CB; ++k) {
            float v = on ? (k < CB ? aW[t][k] : ab[t]) : 0.f;
#pragma unroll
            for (int step = 4; step > 0; step >>= 1) {
                const float o2 = __shfl(v, (lane + QH * step) & 63);
                if (g < step && g + step < G) v += o2;
            }
            if (g == 0 && on) red[(wave * HS + 4 * q + t) * (CB + 1) + k] = v;
        }
    __syncthreads();
    for (int e = threadIdx.x; e < CO * (CB + 1); e += NT) {
        const int o = e / (CB + 1), k = e - o * (CB + 1);
        float acc = 0.f;
#pragma unroll
        for (int w = 0; w < NWV; ++w) acc += red[(w * HS + o) * (CB + 1) + k];
        const int img = sn2_grad_image(rep_k, rep_stride);
        if (acc != 0.f) SN2_FLUSH_ADD(k < CB ? &dW[img + o * CI + CA + k] : &db[img + o], acc);
    }
    (void)NV;
}

// Source pass of the source-side backward: G[s] = sum over the inverted list of s of w * d pre-activation row.
// The unit of work is a CHUNK of a list (inv_order_kernel's chunk table: at most INV_CHUNK entries = one load of row numbers,
// one of weights, STEPS row gathers in flight per lane), and a wave owns L CONSECUTIVE slots of the chunk table, wave w the
// slots [w L, (w + 1) L): it loads their headers with one instruction, and the row numbers of the next chunk travel together
// with the gathers of this one -- one memory round trip per chunk instead of three, the same short chain for
// every wave whatever the lists look like (a wave per SOURCE waited for the few sources whose lists are 13 chunks long:
// C2's lists have a median of 25 entries and a tenth of them 500-800).  Sums run on across the chunks of one source and are
// written out as a partial row Gpart[slot] at the source's last chunk and at the wave's last slot;
// fp_bwd_src_merge_dw_kernel adds a source's partial rows in slot order (and applies G to dsrc and dW_A).
template <int CA, int CB, int CO, bool BF>
__global__ __launch_bounds__(256) void fp_bwd_src_chunk_kernel(int n_chunks, int L, int R_total, int R_per_plot, int S,
                                                               const int4* __restrict__ chunks, const int* __restrict__ inv_row,
                                                               const float* __restrict__ inv_w, const float* __restrict__ dp,
                                                               float* __restrict__ Gpart) {
    constexpr bool SPLIT = dp_split<CO>();
    constexpr int QH = (CO + 3) / 4, HS = 4 * QH, QM = SPLIT ? 8 : QH, RS = SPLIT ? 32 : HS, G = 64 / QM, STEPS = 64 / G;
    constexpr unsigned EB = BF ? 2u : 4u, ROWB = RS * EB;                   // bytes per element / per row
    static_assert(G * STEPS >= INV_CHUNK, "a chunk is one round of gathers");
    static_assert(STEPS % 2 == 0, "two halves");
    __shared__ __attribute__((aligned(16))) float s_part[SPLIT ? 1 : 4][G][HS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (uniform: SGPRs)
    const int q = lane % QM, g = lane / QM;
    const bool on = lane < G * QM;
    const unsigned qoff = (unsigned)q * 4u * EB;
    // workgroups go to the XCDs round-robin; the waves of one XCD own consecutive stretches of the table (plots one after the
    // other, each along its sources' Morton order): neighbouring sources share target rows, and so an L2 (gridDim.x % 8 == 0)
    const int xcd = blockIdx.x & 7, wg_x = blockIdx.x >> 3, n_wg_x = gridDim.x >> 3;
    const long r0 = ((long)(xcd * n_wg_x + wg_x) * 4 + wave) * L;
    if (r0 >= n_chunks) return;                              // (no workgroup barriers in this kernel)
    const int nk = (n_chunks - r0) < L ? (int)(n_chunks - r0) : L;
    const int4 it = lane < nk ? chunks[r0 + lane] : make_int4(0, 0, 0, 0);       // L <= 64
    // (the headers are awaited HERE, once: left to the loop, the wait at its top also sits out every partial row's store)
    // padding only: NO slot of the wave holds a chunk (first and last slot empty is not enough: with plots of fewer than 64
    // chunks a wave's range may start in one plot's padding, cover the next plot's chunks and end in that plot's padding)
    if (__ballot(lane < nk && it.z != 0) == 0ull) return;
    int id = 0, pb = 0, m = 0, rj = 0;                               // round k = -1 only fetches the entries of chunk 0
    float wj = 0.f;
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, sa0 = 0.f, sa1 = 0.f;
    // one round of gathers: NS steps of G entries (entries past the chunk's end: row 0 with weight 0)
    auto gather = [&](auto ns, const char* __restrict__ base) {
        constexpr int NS = decltype(ns)::value;
        float4 v[NS];
        float wv[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int e = G * j + g;
            const unsigned r = (unsigned)__shfl(rj, e);
            wv[j] = __shfl(wj, e);
            if constexpr (!SPLIT) wv[j] = on ? wv[j] : 0.f;
            const unsigned off = r * ROWB + qoff;
            if constexpr (BF) {
                const uint2 u = *reinterpret_cast<const uint2*>(base + off);
                v[j] = make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xFFFF0000u), __uint_as_float(u.y << 16),
                                   __uint_as_float(u.y & 0xFFFF0000u));
            } else {
                v[j] = *reinterpret_cast<const float4*>(base + off);
            }
        }
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            acc[0] = fmaf(wv[j], v[j].x, acc[0]);
            acc[1] = fmaf(wv[j], v[j].y, acc[1]);
            acc[2] = fmaf(wv[j], v[j].z, acc[2]);
            acc[3] = fmaf(wv[j], v[j].w, acc[3]);
        }
    };
    for (int k = -1; k < nk; ++k) {
        int id_n = 0, st_n = 0, m_n = 0, pb_n = 0;
        if (k + 1 < nk) {
            id_n = __builtin_amdgcn_readlane(it.x, k + 1);
            pb_n = __builtin_amdgcn_readlane(it.w, k + 1);
            st_n = __builtin_amdgcn_readlane(it.y, k + 1);
            m_n = __builtin_amdgcn_readlane(it.z, k + 1);
        }
        // the next chunk's entries first: in flight together with this chunk's gathers (loads return in order)
        const int rj_n = lane < m_n ? inv_row[st_n + lane] : 0;          // entries past the end: row 0 with weight 0
        const float wj_n = lane < m_n ? inv_w[st_n + lane] : 0.f;
        if (m > 0) {
            const size_t row0 = (size_t)pb * R_per_plot;
            const char* base = reinterpret_cast<const char*>(dp) + row0 * ROWB;
            float2 sv = make_float2(0.f, 0.f);
            if constexpr (SPLIT) sv = dp_side_ld<BF>(dp, (size_t)R_total, row0 + rj);   // this lane's own entry
            if (m > G * STEPS / 2) gather(std::integral_constant<int, STEPS>{}, base);
            else gather(std::integral_constant<int, STEPS / 2>{}, base);
            sa0 = fmaf(wj, sv.x, sa0);
            sa1 = fmaf(wj, sv.y, sa1);
            if (m_n == 0 || id_n != id) {                    // the source's last chunk, or this wave's last: a partial row
                float* out = Gpart + (size_t)(r0 + k) * HS;
                if constexpr (SPLIT) {
                    // eight lanes per entry: the entries of a step differ in lane bits 3..5
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        acc[t] += __int_as_float(SN2_DPP(__float_as_int(acc[t]), 0x128, 0xF));     // row_ror:8 = lane ^ 8
                        acc[t] += __shfl_xor(acc[t], 16);
                        acc[t] += __shfl_xor(acc[t], 32);
                    }
                    const float s0 = wave_sum(sa0), s1 = wave_sum(sa1);
                    if (lane < 8) reinterpret_cast<float4*>(out)[lane] = make_float4(acc[0], acc[1], acc[2], acc[3]);
                    if (lane == 8) reinterpret_cast<float4*>(out)[8] = make_float4(s0, s1, 0.f, 0.f);
                } else {
                    if (on) *reinterpret_cast<float4*>(&s_part[wave][g][4 * q]) = make_float4(acc[0], acc[1], acc[2], acc[3]);
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    if (lane < HS) {
                        float gk = 0.f;
#pragma unroll
                        for (int gg = 0; gg < G; ++gg) gk += s_part[wave][gg][lane];
                        out[lane] = gk;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
                acc[0] = acc[1] = acc[2] = acc[3] = 0.f;
                sa0 = sa1 = 0.f;
            }
        }
        rj = rj_n, wj = wj_n, id = id_n, pb = pb_n, m = m_n;
    }
}

// What G[s] is for, 64 sources per workgroup in the order of the item table, one per lane of EVERY wave: the four
// waves add up the sources' partial rows (in slot order, a quarter of the channels each) and then each does a quarter of the
// rest: dsrc[s][k] += sum_o G[s][o] W_A[o][k] for its quarter of the channels k (the weights through scalar loads), and
// dW_A[:, 16 w .. 16 w + 15] += sum_s G[s]^T (a o src[s] + c) for its 16 columns (rows = MFMA K).  (One wave doing all of it
// for its 64 sources was one long chain per CU: 18 us.)
template <int CA, int CB, int CO>
__global__ __launch_bounds__(256) void fp_bwd_src_merge_dw_kernel(int n_src, int S, int CM, int src_stride, int dsrc_stride,
                                                                  const int4* __restrict__ items, const float* __restrict__ src,
                                                                  const float* __restrict__ src_a, const float* __restrict__ src_c,
                                                                  const float* __restrict__ Gpart, const float* __restrict__ Wg,
                                                                  float* __restrict__ dsrc, float* __restrict__ dW, int rep_k,
                                                                  int rep_stride, int L) {
    constexpr int CI = CA + CB, QH = (CO + 3) / 4, HS = 4 * QH, TK = (CA + 15) / 16, KQ = (CA + 3) / 4;
    static_assert(TK <= 4, "a wave per 16 columns of dW_A");
    static_assert(KQ <= CA, "a window of KQ columns fits a row");
    using Acc = OuterAcc<CO, 16, 32>;
    static_assert(CO * 16 <= Acc::LDS_FLOATS, "a wave's image fits its staging region");
    __shared__ __attribute__((aligned(16))) float smem[4 * Acc::LDS_FLOATS];
    __shared__ float s_p[HS * 64];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float* lds = smem + w * Acc::LDS_FLOATS;
    const int pp = blockIdx.x * 64 + lane;
    const bool valid = pp < n_src;
    const int4 item = valid ? items[pp] : make_int4(0, 0, 0, 0);
    const size_t ss = (size_t)item.x;
    // what comes from memory at the END of the chain is asked for now: the old values of this wave's quarter of dsrc[s] ..
    float* dr = dsrc + ss * dsrc_stride;
    float d_old[KQ];
    const int k0 = w * KQ + KQ <= CA ? w * KQ : CA - KQ;     // (the last wave's window of KQ columns is pulled back inside the row)
#pragma unroll
    for (int i = 0; i < KQ; ++i) d_old[i] = valid ? dr[k0 + i] : 0.f;
    // .. and this wave's columns of (a o src + c)
    float x[16];
    if (w < TK) {
        const float4* sr = reinterpret_cast<const float4*>(src + ss * src_stride);
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            if (4 * (4 * w + q4) < CA) a = sr[4 * w + q4];
            x[4 * q4] = a.x, x[4 * q4 + 1] = a.y, x[4 * q4 + 2] = a.z, x[4 * q4 + 3] = a.w;
        }
    }
    // the source's chunks are the slots [f, f + nch) of the chunk table; its partial rows: at its last slot and at every
    // slot that is the last of a wave of fp_bwd_src_chunk_kernel (slot % L == L - 1).  Wave w adds up the quads w, w + 4, ..
    // of the rows, four rows in flight, and the waves swap their sums through LDS.
    const int nch = (item.z + INV_CHUNK - 1) / INV_CHUNK;
    const int f = (item.x / S) * CM + item.w, last = f + nch - 1;        // (slots: B * CM < 2^31, checked by the host)
    constexpr int NQ = (QH + 3) / 4;
    float4 pq[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) pq[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r = f; __builtin_amdgcn_ballot_w64(r <= last) != 0;) {
        float4 a[4][NQ];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool more = r <= last;
            const int e = more ? min(last, (int)((unsigned)r / (unsigned)L) * L + L - 1) : 0;
            const float4* gr = reinterpret_cast<const float4*>(Gpart + (size_t)e * HS);
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                a[j][i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (more && w + 4 * i < QH) a[j][i] = gr[w + 4 * i];
            }
            if (more) r = e + 1;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < NQ; ++i)
                pq[i].x += a[j][i].x, pq[i].y += a[j][i].y, pq[i].z += a[j][i].z, pq[i].w += a[j][i].w;
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i)
        if (w + 4 * i < QH) {
            const int o = 4 * (w + 4 * i);
            s_p[(o + 0) * 64 + lane] = pq[i].x, s_p[(o + 1) * 64 + lane] = pq[i].y;
            s_p[(o + 2) * 64 + lane] = pq[i].z, s_p[(o + 3) * 64 + lane] = pq[i].w;
        }
    __syncthreads();
    float p[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) p[o] = s_p[o * 64 + lane];
    if (w < TK) {
        const cfp sa = opaque(as_const(src_a)), sc = opaque(as_const(src_c));
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int k = 16 * w + i;
            if (k >= CA || !valid) x[i] = 0.f;
            else if (src_a) x[i] = fmaf(sa[k], x[i], sc[k]);
        }
        if (!valid) {
#pragma unroll
            for (int o = 0; o < CO; ++o) p[o] = 0.f;
        }
        Acc acc;
        acc.init(lds);
        acc.add(lds, p, x);
        acc.store_slab(lds);                                 // slab[o * 16 + i]
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int img = sn2_grad_image(rep_k, rep_stride);
        for (int i = lane; i < CO * 16; i += 64) {
            const int o = i >> 4, k = 16 * w + (i & 15);
            const float v = lds[i];
            if (k < CA && v != 0.f) SN2_FLUSH_ADD(&dW[img + o * CI + k], v);
        }
    }
    // dsrc last: its arithmetic runs while the float atomics above are on their way
    if (valid) {
        // (KQ consecutive weights per o: wide scalar loads; the last wave's window is pulled back inside the row, its
        // first columns computed twice and not stored)
        const cfp W = opaque(as_const(Wg)) + k0;
        float d[KQ];
#pragma unroll
        for (int i = 0; i < KQ; ++i) d[i] = 0.f;
#pragma unroll 2
        for (int o = 0; o < CO; ++o) {                       // (not unrolled in full: 306 weights do not fit the SGPRs)
            const float po = s_p[o * 64 + lane];
#pragma unroll
            for (int i = 0; i < KQ; ++i) d[i] = fmaf(po, W[o * CI + i], d[i]);
        }
        const int sh = w * KQ - k0;                          // columns of the window that belong to the wave before
#pragma unroll
        for (int i = 0; i < KQ; ++i)
            if (i >= sh) dr[k0 + i] = d_old[i] + d[i];
    }
}

// ---------------------------------------------------------------------------------------------- small layers
// Layers with few rows (SA3, FP3, FP2: 4k-16k rows, up to 96 -> 64 channels) gain nothing from one long FMA stream per
// lane: 4096 rows are only 64 waves on a 1024-SIMD chip and each wave would issue >6000 dependent FMAs (the first
// version ran 0.3-0.7 ms per kernel at ~1 % of the chip).  Here one workgroup = 64 rows x 4 waves and wave g owns the
// output channels [g*COG, (g+1)*COG): 4x the waves, 4x shorter streams, the same weights-in-SGPR inner loops.
template <int CA, int CB, int CO, bool KNN, bool BF16>
__global__ __launch_bounds__(256) void fp_fwd_split_kernel(int R, int R_per_plot, int S_per_plot, int src_stride,
                                                           int skip_stride, int h_stride, const float* __restrict__ src,
                                                           const float* __restrict__ src_a, const float* __restrict__ src_c,
                                                           const int* __restrict__ knn_idx, const float* __restrict__ knn_w,
                                                           const float* __restrict__ skip, const float* __restrict__ W,
                                                           const float* __restrict__ bias, float* __restrict__ h,
                                                           float* __restrict__ slots) {
    // 64 rows per workgroup.  The four waves first build the rows' inputs [u | 1] together in LDS (wave g: the channel
    // quads q = g mod 4 of the interpolated part and of the skip part), then wave g computes the 16 output channels
    // [16 g, 16 g + 16) of all 64 rows on the matrix cores: A[row][k] from the staged inputs, B[k][o] = W^T | bias in
    // registers ((CI + 1)/4 values per lane).  As per-lane FMA chains with scalar-loaded weights (16 x 96 per lane for FP3,
    // every wave rebuilding the whole input) these layers took 15-30 us each for 4-16k rows.
    constexpr int CI = CA + CB, CK = CI + 1, KB = (CK + 3) / 4, QA = (CA + 3) / 4, NG = (CO + 15) / 16;
    constexpr int QS = OuterAcc<16, CK>::QS;
    static_assert(NG <= 4 && 4 * KB <= QS, "fp_fwd_split_kernel shapes");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_q = smem;                       // [64][QS]
    float* s_red = smem + 64 * QS;           // [2 * 16 * NG]
    const int lane = threadIdx.x & 63;
    const int g = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long r = (long)blockIdx.x * 64 + lane;
    const bool valid = r < R;
    const size_t rr = valid ? (size_t)r : (size_t)(R - 1);
    stage_inputs<CA, CB, KNN>(s_q, QS, g, lane, (long)blockIdx.x * 64, R, R_per_plot, S_per_plot, src, src_stride, src_a, src_c,
                              knn_idx, knn_w, skip, skip_stride);
    if (g == 2) {                            // K padding of the contraction: finite (0 x garbage would be NaN)
#pragma unroll
        for (int k = CK; k < 4 * KB; ++k) s_q[lane * QS + k] = 0.f;
    }
    // B operand: lane (qq, cc) keeps [W | bias][o = 16 g + cc][k = 4 kb + qq]
    const int qq = lane >> 4, cc = lane & 15;
    const int o = 16 * g + cc;
    float Wb[KB];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
        const int k = 4 * kb + qq;
        // bf16 operands: the bias stays out of the contraction (it would be rounded) and starts the accumulator instead
        Wb[kb] = (g < NG && o < CO) ? (k < CI ? W[o * CI + k] : ((k == CI && !BF16) ? bias[o] : 0.f)) : 0.f;
    }
    const float bias_o = (BF16 && g < NG && o < CO) ? bias[o] : 0.f;
    __syncthreads();
    float ssum = 0.f, ssq = 0.f;
    if (g < NG) {
        f32x4 D[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) D[t] = f32x4{bias_o, bias_o, bias_o, bias_o};
        if constexpr (!BF16) {
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    D[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_q[(16 * t + cc) * QS + 4 * kb + qq], Wb[kb], D[t], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                D[t] = contract<true, KB>(D[t], [&](int kb) { return s_q[(16 * t + cc) * QS + 4 * kb + qq]; },
                                          [&](int kb) { return Wb[kb]; });
        }
        // D[t][j]: row 16 t + 4 qq + j, channel o
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long row = (long)blockIdx.x * 64 + 16 * t + 4 * qq + j;
                const float v = (row < R && o < CO) ? fmaxf(D[t][j], 0.f) : 0.f;
                ssum += v;
                ssq = fmaf(v, v, ssq);
                if (row < R && o < h_stride) h[(size_t)row * h_stride + o] = v;      // pad channels: 0
            }
        // the four row groups (qq) of a channel
        ssum += __shfl_xor(ssum, 16);
        ssq += __shfl_xor(ssq, 16);
        ssum += __shfl_xor(ssum, 32);
        ssq += __shfl_xor(ssq, 32);
        if (qq == 0) {
            s_red[o] = ssum;
            s_red[16 * NG + o] = ssq;
        }
    }
    if (slots) {
        __syncthreads();
        for (int i = threadIdx.x; i < 2 * CO; i += 256)
            slots[(size_t)blockIdx.x * 2 * CO + i] = i < CO ? s_red[i] : s_red[16 * NG + (i - CO)];
    }
}

#ifdef SN2_SPLIT_STAMPS
// diagnostic build only (never shipped): phase stamps of thread 0 of one workgroup of fp_bwd_split_kernel<64, 32, 64>
__device__ unsigned long long g_split_dbg[16];
extern "C" int sn2_debug_split_stamps(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_split_dbg), sizeof(g_split_dbg));
}
#define FSTAMP(i)                                                                                   \
    if (CA == 64 && CB == 32 && blockIdx.x == 7 && threadIdx.x == 0) {                              \
        unsigned long long t_;                                                                      \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                   \
        g_split_dbg[i] = t_;                                                                        \
    }
#else
#define FSTAMP(i)
#endif

// LDS of fp_bwd_split_kernel: inputs [64][QS] + per-wave dp [4][64][16] + the input-gradient slab(s) [1 or 4][64][CI|1]
// + the BatchNorm vectors [5][64]
template <int CI>
constexpr size_t fp_split_lds_bytes(int slabs) {
    return (size_t)(64 * OuterAcc<16, CI + 1>::QS + 4 * 64 * 16 + slabs * 64 * (CI | 1) + 5 * 64) * 4;
}
template <int CI>
constexpr bool fp_split_du_seq() { return fp_split_lds_bytes<CI>(4) > 150 * 1024; }   // one slab, the waves take turns

template <int CA, int CB, int CO, bool KNN, bool BF16>
__global__ __launch_bounds__(256) void fp_bwd_split_kernel(
    int R, int R_per_plot, int S_per_plot, int src_stride, int skip_stride, int h_stride, int dskip_stride, int du_stride,
    float invR, const float* __restrict__ src, const float* __restrict__ src_a, const float* __restrict__ src_c,
    const int* __restrict__ knn_idx, const float* __restrict__ knn_w, const float* __restrict__ skip,
    const float* __restrict__ W, const float* __restrict__ gamma, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ dgamma, const float* __restrict__ dbeta,
    const float* __restrict__ h, const float* __restrict__ dy, float* __restrict__ dW, float* __restrict__ db,
    float* __restrict__ du_out, float* __restrict__ dskip, int rep_k, int rep_stride) {
    constexpr int CI = CA + CB, COG = (CO + 3) / 4;
    using Acc = OuterAcc<16, CI + 1>;
    constexpr int QS = Acc::QS, TK = Acc::TK, CIP = CI | 1;
    constexpr bool DU_SEQ = fp_split_du_seq<CI>();
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_q = smem;                       // [64][QS]  the rows' inputs | 1, shared by the four waves
    float* s_p = s_q + 64 * QS;              // [4][64][16] per-wave d pre-activation of its channel group
    float* s_du = s_p + 4 * 64 * 16;         // [4][64][CIP] per-wave partial input gradient (summed at write-out: LDS
                                             // float atomics are slow on this chip, plain stores + 4 reads are not)
    const int lane = threadIdx.x & 63;
    const int g = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long r = (long)blockIdx.x * 64 + lane;
    const bool valid = r < R;
    const size_t rr = valid ? (size_t)r : (size_t)(R - 1);
    FSTAMP(0);
    // no clearing pass over the staging regions (it cost 4000 clocks + a barrier): the input columns past CI only feed
    // output columns nobody reads, the channel pads of s_p are written below
    FSTAMP(1);
    stage_inputs<CA, CB, KNN>(s_q, QS, g, lane, (long)blockIdx.x * 64, R, R_per_plot, S_per_plot, src, src_stride, src_a, src_c,
                              knn_idx, knn_w, skip, skip_stride);
    // d pre-activation: the block's 64 x CO tile of h and dy read thread-linearly as float4 quads (whole rows per load
    // instruction, as above), the five per-channel vectors of the BatchNorm backward staged in LDS
    constexpr int HS4 = (CO + 3) / 4, NU = (64 * HS4 + 255) / 256;
    float* s_par = s_du + (DU_SEQ ? 1 : 4) * 64 * CIP;       // [5][64]: mean, invstd, gamma, dbeta, dgamma
    if (threadIdx.x < CO) {
        const int o = threadIdx.x;
        s_par[0 * 64 + o] = mean[o], s_par[1 * 64 + o] = invstd[o], s_par[2 * 64 + o] = gamma[o];
        s_par[3 * 64 + o] = dbeta[o], s_par[4 * 64 + o] = dgamma[o];
    }
    float4 hv[NU], dv[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int i4 = threadIdx.x + 256 * u, row = i4 / HS4, qd = i4 - row * HS4;
        const long rw = (long)blockIdx.x * 64 + row;
        const size_t ra = (i4 < 64 * HS4 && rw < R) ? (size_t)rw : (size_t)(R - 1);
        hv[u] = reinterpret_cast<const float4*>(h + ra * h_stride)[i4 < 64 * HS4 ? qd : 0];
        dv[u] = reinterpret_cast<const float4*>(dy + ra * h_stride)[i4 < 64 * HS4 ? qd : 0];
    }
#pragma unroll
    for (int t = 0; t < 16; ++t)
        if (t >= COG || g * COG + t >= CO) s_p[(g * 64 + lane) * 16 + t] = 0.f;   // K padding of dp . W: finite
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int i4 = threadIdx.x + 256 * u, row = i4 / HS4, qd = i4 - row * HS4;
        const bool live = i4 < 64 * HS4 && (long)blockIdx.x * 64 + row < R;
        const float hq[4] = {hv[u].x, hv[u].y, hv[u].z, hv[u].w}, dq[4] = {dv[u].x, dv[u].y, dv[u].z, dv[u].w};
        if (i4 < 64 * HS4) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int o = 4 * qd + t;
                if (o < CO) {
                    const float hh = hq[t], dd = dq[t];
                    const float is = s_par[1 * 64 + o];
                    const float xh = (hh - s_par[0 * 64 + o]) * is;
                    const float dh = s_par[2 * 64 + o] * is * (dd - s_par[3 * 64 + o] * invR - xh * s_par[4 * 64 + o] * invR);
                    s_p[((o / COG) * 64 + row) * 16 + (o % COG)] = (live && hh > 0.f) ? dh : 0.f;
                }
            }
        }
    }
    FSTAMP(2);
    __syncthreads();
    FSTAMP(3);
    // dW|db rows of this channel group: rows of the block are the MFMA K dimension
    f32x4 acc[TK];
#pragma unroll
    for (int c = 0; c < TK; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    {
        const int r4 = lane >> 4, c16 = lane & 15;
        const float* rp = s_p + (g * 64 + r4) * 16 + c16;
        const float* rq = s_q + r4 * QS + c16;
        if constexpr (!BF16) {
#pragma unroll 4
            for (int st = 0; st < 16; ++st) {
                const float av = rp[st * 4 * 16];
#pragma unroll
                for (int c = 0; c < TK; ++c)
                    acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, rq[st * 4 * QS + c * 16], acc[c], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int s8 = 0; s8 < 2; ++s8) {          // the block's 64 rows = the K of two v_mfma_f32_16x16x32_bf16
                float av[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) av[u] = rp[(8 * s8 + u) * 4 * 16];
#pragma unroll
                for (int c = 0; c < TK; ++c)
                    acc[c] = contract<true, 8>(acc[c], [&](int u) { return av[u]; },
                                               [&](int u) { return rq[(8 * s8 + u) * 4 * QS + c * 16]; });
            }
        }
    }
    FSTAMP(4);
    // partial input gradient of this channel group, dp_g (64 x 16) . W_g (16 x CI), on the matrix cores: A[row][o] read
    // back from this wave's staged dp rows, B[o][col] = the group's weight rows in registers (as per-lane FMA chains with
    // scalar-loaded weights this was the longest part of the kernel: 16 x 96 FMAs per lane for FP3)
    {
        constexpr int TJ = (CI + 15) / 16;
        const int qq = lane >> 4, cc = lane & 15;
        float Wb[4][TJ];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int jt = 0; jt < TJ; ++jt) {
                const int t = 4 * kb + qq, o = g * COG + t, col = 16 * jt + cc;
                Wb[kb][jt] = (t < COG && o < CO && col < CI) ? W[o * CI + col] : 0.f;
            }
        // DU_SEQ (wide inputs: CI = 128): one slab for the workgroup, the four waves add their partial products in turn
        // (four slabs would not fit LDS); otherwise one slab per wave, summed at write-out
        for (int turn = 0; turn < (DU_SEQ ? 4 : 1); ++turn) {
            if (!DU_SEQ || g == turn) {
#pragma unroll
                for (int tile = 0; tile < 4; ++tile) {
                    f32x4 D[TJ];
#pragma unroll
                    for (int jt = 0; jt < TJ; ++jt) D[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if constexpr (!BF16) {
#pragma unroll
                        for (int kb = 0; kb < 4; ++kb) {
                            const float av = s_p[(g * 64 + 16 * tile + cc) * 16 + 4 * kb + qq];
#pragma unroll
                            for (int jt = 0; jt < TJ; ++jt)
                                D[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Wb[kb][jt], D[jt], 0, 0, 0);
                        }
                    } else {
#pragma unroll
                        for (int jt = 0; jt < TJ; ++jt)
                            D[jt] = contract<true, 4>(D[jt], [&](int kb) { return s_p[(g * 64 + 16 * tile + cc) * 16 + 4 * kb + qq]; },
                                                      [&](int kb) { return Wb[kb][jt]; });
                    }
#pragma unroll
                    for (int jt = 0; jt < TJ; ++jt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int col = 16 * jt + cc;
                            if (col < CI) {
                                float* dst = &s_du[((DU_SEQ ? 0 : g) * 64 + 16 * tile + 4 * qq + r) * CIP + col];
                                *dst = (DU_SEQ && turn > 0) ? *dst + D[jt][r] : D[jt][r];
                            }
                        }
                }
            }
            if (DU_SEQ) __syncthreads();
        }
    }
    FSTAMP(5);
    __syncthreads();
    FSTAMP(6);
    auto du_sum = [&](int row, int k) {
        if (DU_SEQ) return s_du[row * CIP + k];
        return (s_du[(0 * 64 + row) * CIP + k] + s_du[(1 * 64 + row) * CIP + k]) +
               (s_du[(2 * 64 + row) * CIP + k] + s_du[(3 * 64 + row) * CIP + k]);
    };
    const long r0 = (long)blockIdx.x * 64;
    // accumulated outputs: all the old values are loaded before the first is used (one dependent load per loop turn made
    // this write-out 12 000 clocks, a quarter of the kernel)
    if (du_out) {
        constexpr int NI = (64 * CA + 255) / 256;
        float old[NI];
#pragma unroll
        for (int u = 0; u < NI; ++u) {
            const int i = threadIdx.x + 256 * u, row = i / CA, k = i - row * CA;
            old[u] = (!KNN && i < 64 * CA && r0 + row < R) ? du_out[(size_t)(r0 + row) * du_stride + k] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < NI; ++u) {
            const int i = threadIdx.x + 256 * u, row = i / CA, k = i - row * CA;
            if (i < 64 * CA && r0 + row < R) {
                float* dst = du_out + (size_t)(r0 + row) * du_stride + k;
                if (KNN) *dst = du_sum(row, k);
                else *dst = old[u] + du_sum(row, k);
            }
        }
    }
    if (CB > 0 && dskip) {
        constexpr int NI = (64 * CB + 255) / 256;
        float old[NI > 0 ? NI : 1];
#pragma unroll
        for (int u = 0; u < NI; ++u) {
            const int i = threadIdx.x + 256 * u, row = i / (CB > 0 ? CB : 1), k = i - row * CB;
            old[u] = (i < 64 * CB && r0 + row < R) ? dskip[(size_t)(r0 + row) * dskip_stride + k] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < NI; ++u) {
            const int i = threadIdx.x + 256 * u, row = i / (CB > 0 ? CB : 1), k = i - row * CB;
            if (i < 64 * CB && r0 + row < R) dskip[(size_t)(r0 + row) * dskip_stride + k] = old[u] + du_sum(row, CA + k);
        }
    }
    FSTAMP(7);
    {
        const int r4 = lane >> 4, c16 = lane & 15, img = sn2_grad_image(rep_k, rep_stride);
#pragma unroll
        for (int c = 0; c < TK; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int t = r4 * 4 + q, o = g * COG + t, k = c * 16 + c16;
                if (t < COG && o < CO) {
                    if (k < CI) SN2_FLUSH_ADD(&dW[img + o * CI + k], acc[c][q]);
                    else if (k == CI) SN2_FLUSH_ADD(&db[img + o], acc[c][q]);
                }
            }
    }
    FSTAMP(8);
}

// ---- the dispatch: one plan per direction says which of the three kernel forms a descriptor takes, or refuses it, in host
// arithmetic alone; one launcher per form launches it.  sn2_fp_form (include/strata_hip.h, "Routes") is the plans, exported.
enum class FpForm { Split = SN2_FP_FORM_SPLIT, SourceSide = SN2_FP_FORM_SOURCE_SIDE, Dense = SN2_FP_FORM_DENSE };

// the blocks whose source-side kernels are instantiated: the same test as sn2_fp_source_side's, at compile time
template <int CB, bool KNN>
constexpr bool FP_SRC_SIDE_CB = KNN && CB > 0 && CB % 4 == 0 && CB <= 16;

// The forward's rule.  Split: the matrix-core kernel (64 rows x 4 channel groups per workgroup): its per-workgroup statistic
// slots bound the rows of a TRAINING pass.  SourceSide: more rows than that on a block with the workspace (the per-point layer
// keeps this form in every mode).  What is left: Dense -- but an eval pass (mode 0) writes no statistics, so any row count takes
// Split (parcel inference: FP3 on 80 000 rows ran the dense kernel at 0.31 ms, 15 x what the contraction needs).
// mode == SN2_BN_FROZEN_KEEP: the form a TRAINING pass of this shape takes (the backward pass that follows must find the rows
// of that form), without statistic sums; BatchNorm finalised from the running statistics, nothing updated.
template <int CA, int CB, int CO, bool KNN>
int fp_forward_plan(const sn2_fp* p, int mode, FpForm* form) {
    if (mode < 0 || mode > SN2_BN_FROZEN_KEEP) return SN2_EINVAL;
    const long R = (long)p->B * p->R_per_plot;
    const bool src_side = FP_SRC_SIDE_CB<CB, KNN> && sn2_fp_source_side(R, CB, 0) && fp_source_side_ok<CA, CO>(p);
    *form = sn2_fp_rows_small(R) ? FpForm::Split : src_side ? FpForm::SourceSide : mode == 0 ? FpForm::Split : FpForm::Dense;
    // bfloat16 rows: the source-side form of the per-point layer only; bfloat16 operands: the matrix-core kernel only
    if ((p->act_bf16 && *form != FpForm::SourceSide) || (p->blk.mma_bf16 && *form != FpForm::Split)) return SN2_ELIMIT;
    return 0;
}

// Split and Dense hand the rows' input gradients to the transpose of the interpolation (bwd_gather) unless the caller does
// that itself (scatter_ready < 0)
template <bool KNN>
bool fp_backward_gathers(const sn2_fp* p) { return KNN && p->dsrc && p->scatter_ready >= 0; }

// The backward's rule: the forward's in a training pass, with two differences.  There is no eval case; and the source-side
// form also needs the backward's own buffers -- dsrc, du_scratch and the inverted index in scatter_ws, and no dskip (its
// kernels write none) -- so a block that ran SourceSide forward falls back to Dense when they are not all there.
template <int CA, int CB, int CO, bool KNN>
int fp_backward_plan(const sn2_fp* p, FpForm* form) {
    if (!p->dy || !p->blk.dW || !p->blk.db || !p->blk.dgamma || !p->blk.dbeta) return SN2_EINVAL;
    const long R = (long)p->B * p->R_per_plot;
    const bool src_side = FP_SRC_SIDE_CB<CB, KNN> && sn2_fp_source_side(R, CB, 0) && fp_source_side_ok<CA, CO>(p) && p->dsrc &&
                          !p->dskip && p->du_scratch && p->scatter_ws;
    *form = sn2_fp_rows_small(R) ? FpForm::Split : src_side ? FpForm::SourceSide : FpForm::Dense;
    // bfloat16 rows: the source-side form only, and its BatchNorm sums come from the consumer (no row pass reads bfloat16 dy)
    if (p->act_bf16 && !(*form == FpForm::SourceSide && p->bn_sums_done)) return SN2_ELIMIT;
    if (KNN && p->dsrc && !p->du_scratch) return SN2_EINVAL;
    // bfloat16 operands: the matrix-core kernel only; permuted du rows: the source-side kernels only
    if ((p->blk.mma_bf16 && *form != FpForm::Split) || (p->row_perm && *form != FpForm::SourceSide)) return SN2_ELIMIT;
    if (*form == FpForm::SourceSide || fp_backward_gathers<KNN>(p)) {       // what reads the inverted index
        if (!p->scatter_ws) return SN2_EINVAL;
        if (p->S_per_plot > 8192) return SN2_ELIMIT;
    }
    // the chunk table of the source-side form: B * CM slots within what its kernels index
    if (*form == FpForm::SourceSide && (long)p->B * inv_chunks_per_plot(p->R_per_plot, p->S_per_plot) >= (1L << 31) / 64)
        return SN2_ELIMIT;
    return 0;
}

// ---- forward launchers: each ends in its sn2_bn_finalize
// (fp_fwd_split_kernel and fp_fwd_kernel take the same arguments)
template <class K>
int launch_fwd_rows(K kern, int grid, size_t lds, const sn2_fp* p, int training, hipStream_t st) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, p->B * p->R_per_plot, p->R_per_plot,
                       p->S_per_plot, p->src_stride, p->skip_stride, p->h_stride, p->src, p->src_a, p->src_c, p->knn_idx,
                       p->knn_w, p->skip, p->blk.W, p->blk.b, p->h, training ? p->blk.stat_slots : (float*)nullptr);
    SN2_RETURN_LAUNCH();
}

template <int CA, int CB, int CO, bool KNN>
int fwd_split(const sn2_fp* p, int training, hipStream_t st) {
    const int R = p->B * p->R_per_plot, grid = sn2_cdiv(R, 64);
    constexpr size_t lf = (size_t)(64 * OuterAcc<16, CA + CB + 1>::QS + 2 * 16 * ((CO + 15) / 16)) * sizeof(float);
    static_assert(lf <= 48 * 1024, "fp_fwd_split_kernel staging");
    auto kf = p->blk.mma_bf16 ? &fp_fwd_split_kernel<CA, CB, CO, KNN, true> : &fp_fwd_split_kernel<CA, CB, CO, KNN, false>;
    SN2_TRY(launch_fwd_rows(kf, grid, lf, p, training, st));
    return sn2_bn_finalize(&p->blk, training ? grid : 0, nullptr, R, training, st);
}

template <int CA, int CB, int CO>
int fwd_source_side(const sn2_fp* p, int training, hipStream_t st) {
    const int R = p->B * p->R_per_plot, n_src = p->B * p->S_per_plot;
    SN2_TRY((launch_src_table<CA, CB, CO>(n_src, p->src_stride, p->src, p->src_a, p->src_c, p->blk.W, p->src_ws, st)));
    const long n_grp = sn2_cdiv(R, 64 / ((CO + 3) / 4));
    int grid = sn2_cdiv(n_grp, 8);
    // two workgroups per CU: at 143 VGPRs three waves fit a SIMD, so 1024 workgroups ran as one full round and a
    // third of a second one (0.057 ms; 768: 0.056; 512: 0.052; 384: 0.058)
    const int cap_fwd_rows = 2 * sn2_cu_count() < SN2_STAT_SLOTS ? 2 * sn2_cu_count() : SN2_STAT_SLOTS;
    if (grid > cap_fwd_rows) grid = cap_fwd_rows;
    // (round 4: a variant with the plot's whole table in LDS -- 144 KB, one 16-wave workgroup per CU, the 226 MB of L2
    // gathers replaced by ds_read_b128 -- ran in 38.1 us against this kernel's 36.5: the gathers are not its bound; at
    // ~14 instructions per row and wave-instruction it is instruction issue, like the head kernels; the skip part's FMA
    // chains as v_pk_fma_f32 pairs -- 32 instructions fewer per two rows -- ran in 38.0 us as well)
    // (round 5: the row pass with its input stream fetched one element per lane, four iterations ahead;
    // sn2_debug_fp_rows_form(0): the first form, kept for cross-checks -- same bits)
    const bool rows2 = g_fp_rows_form != 0;
    auto kr = rows2 ? (p->act_bf16 ? &fp_fwd_rows2_kernel<CA, CB, CO, true> : &fp_fwd_rows2_kernel<CA, CB, CO, false>)
                    : (p->act_bf16 ? &fp_fwd_rows_kernel<CA, CB, CO, true> : &fp_fwd_rows_kernel<CA, CB, CO, false>);
    hipLaunchKernelGGL(kr, dim3(grid), dim3(256), 0, st, R, p->R_per_plot, p->S_per_plot,
                       p->skip_stride, (const float*)p->src_ws, p->knn_idx, p->knn_w, p->skip, p->blk.W, p->blk.b, p->h,
                       training ? p->blk.stat_slots : (float*)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    return sn2_bn_finalize(&p->blk, grid, nullptr, R, training, st);
}

template <int CA, int CB, int CO, bool KNN>
int fwd_dense(const sn2_fp* p, int training, hipStream_t st) {
    const int R = p->B * p->R_per_plot;
    int grid = pick_grid(R, 256, 4);
    if (grid > SN2_STAT_SLOTS) grid = SN2_STAT_SLOTS;
    SN2_TRY(launch_fwd_rows(&fp_fwd_kernel<CA, CB, CO, KNN>, grid, 0, p, training, st));
    return sn2_bn_finalize(&p->blk, grid, nullptr, R, training, st);
}

template <int CA, int CB, int CO, bool KNN>
int fp_forward_t(const sn2_fp* p, int mode, hipStream_t st) {
    FpForm form;
    SN2_TRY((fp_forward_plan<CA, CB, CO, KNN>(p, mode, &form)));
    const int training = mode == 1;
    switch (form) {
    case FpForm::Split: return fwd_split<CA, CB, CO, KNN>(p, training, st);
    case FpForm::Dense: return fwd_dense<CA, CB, CO, KNN>(p, training, st);
    case FpForm::SourceSide:
        if constexpr (FP_SRC_SIDE_CB<CB, KNN>) return fwd_source_side<CA, CB, CO>(p, training, st);
    }
    return SN2_EINVAL;
}

extern "C" int sn2_debug_fp_table_form(int form) {
    g_fp_table_form = form ? 1 : 0;
    return 0;
}
extern "C" int sn2_debug_fp_rows_form(int form) {
    g_fp_rows_form = form ? 1 : 0;
    return 0;
}
// diagnostic (bench.py): which of the three kernels of the per-point layer's source-side backward run -- bit 0 the row pass, 1 the
// source pass over the chunk table, 2 the merge (7 = all, the only setting that computes the gradients)
static int g_fp1_bwd_parts = 7;
extern "C" int sn2_debug_fp1_backward_parts(int mask) {
    g_fp1_bwd_parts = mask & 7 ? mask & 7 : 7;
    return 0;
}

// ---- backward launchers
// 1 / (rows of the batch statistics); frozen_stats: the forward's statistics were constants (running statistics) -- the
// batch-mean and batch-variance terms of the BatchNorm backward vanish
inline float fp_inv_rows(const sn2_fp* p) { return p->blk.frozen_stats ? 0.f : 1.0f / (float)(p->B * p->R_per_plot); }
// fp_bwd_split_kernel and fp_bwd_main_kernel take the same arguments; du: where they leave the rows' input gradients
template <int CA, bool KNN, class K>
int launch_bwd_rows(K kern, int grid, int threads, size_t lds, const sn2_fp* p, hipStream_t st) {
    float* du = !KNN ? p->dsrc : p->dsrc ? p->du_scratch : nullptr;
    if (lds > 48 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, st, p->B * p->R_per_plot, p->R_per_plot, p->S_per_plot, p->src_stride,
                       p->skip_stride, p->h_stride, p->dskip_stride, KNN ? CA : p->dsrc_stride, fp_inv_rows(p), p->src,
                       p->src_a, p->src_c, p->knn_idx, p->knn_w, p->skip, p->blk.W, p->blk.gamma,
                       (const float*)p->blk.mean, (const float*)p->blk.invstd, (const float*)p->blk.dgamma,
                       (const float*)p->blk.dbeta, (const float*)p->h, p->dy, p->blk.dW, p->blk.db, du, p->dskip,
                       p->blk.grad_replicas, p->blk.grad_replica_stride);
    SN2_RETURN_LAUNCH();
}

// dgamma / dbeta of the block's BatchNorm from a pass over the rows.  bn_sums_done (non-NULL): sn2_head_bn_sums /
// sn2_fp_bn_sums already completed them (by the identity or by their own pass over the rows)
template <int CO>
int bwd_bn_sums(const sn2_fp* p, hipStream_t st) {
    if (p->bn_sums_done) return 0;
    const int R = p->B * p->R_per_plot;
    if (R <= (1 << 16)) {
        hipLaunchKernelGGL((fp_bwd_bn_small_kernel<CO>), dim3(sn2_cdiv(R, 64)), dim3(256), 0, st, R, p->h_stride, p->h, p->dy,
                           p->blk.mean, p->blk.invstd, p->blk.dgamma, p->blk.dbeta, p->bn_sums_done);
    } else {
        int g1 = pick_grid(R, 256, R >= (1 << 18) ? 8 : 1);
        if (g1 > 256) g1 = 256;
        hipLaunchKernelGGL((fp_bwd_bn_kernel<CO>), dim3(g1), dim3(256), 0, st, R, p->h_stride, p->h, p->dy,
                           p->blk.mean, p->blk.invstd, p->blk.dgamma, p->blk.dbeta, p->bn_sums_done);
    }
    SN2_RETURN_LAUNCH();
}

// the 64-row x 4-channel-group kernel for small layers
template <int CA, int CB, int CO, bool KNN>
int bwd_split(const sn2_fp* p, hipStream_t st) {
    constexpr int CI = CA + CB;
    constexpr size_t lb = fp_split_lds_bytes<CI>(fp_split_du_seq<CI>() ? 1 : 4);
    static_assert(lb <= 150 * 1024, "fp_bwd_split_kernel staging must fit LDS");
    auto ks = p->blk.mma_bf16 ? &fp_bwd_split_kernel<CA, CB, CO, KNN, true> : &fp_bwd_split_kernel<CA, CB, CO, KNN, false>;
    return launch_bwd_rows<CA, KNN>(ks, sn2_cdiv(p->B * p->R_per_plot, 64), 256, lb, p, st);
}

template <int CA, int CB, int CO>
int bwd_source_side(const sn2_fp* p, hipStream_t st) {
    const int S = p->S_per_plot, Rp = p->R_per_plot, B = p->B, R = B * Rp, n_src = B * S;
    constexpr int NT = 512;                       // 2 workgroups x 8 waves per CU
    constexpr size_t lb1 = (size_t)(NT / 64) * (4 * ((CO + 3) / 4)) * (CB + 1) * sizeof(float);
    auto k1 = p->act_bf16 ? &fp_bwd_rows_kernel<CA, CB, CO, NT, true> : &fp_bwd_rows_kernel<CA, CB, CO, NT, false>;
    if (lb1 > 48 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k1), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lb1);
    const int parts = g_fp1_bwd_parts;
    if (parts & 1)
        hipLaunchKernelGGL(k1, dim3(2 * sn2_cu_count()), dim3(NT), lb1, st, R, p->skip_stride, fp_inv_rows(p), p->skip,
                           p->blk.gamma, (const float*)p->blk.mean, (const float*)p->blk.invstd,
                           (const float*)p->blk.dgamma, (const float*)p->blk.dbeta, (const float*)p->h, p->dy,
                           p->du_scratch, p->blk.dW, p->blk.db, p->blk.grad_replicas, p->blk.grad_replica_stride,
                           p->row_perm, Rp);
    if (!p->scatter_ready) SN2_TRY(build_interp_index(p->knn_idx, p->knn_w, nullptr, B, Rp, S, p->scatter_ws, st, p->row_perm));
    const InterpIndex x = carve_interp_index(p->scatter_ws, B, Rp, S);
    // waves over the chunk table (as many as the chip holds at once, L <= 64 slots each), then a lane per source for
    // what G[s] is for
    const int n_chunks = B * x.CM;
    const int waves_resident = sn2_cu_count() * 32;
    int L = sn2_cdiv(n_chunks, waves_resident);
    if (L < 4) L = 4;
    if (L > 64) L = 64;
    const int gc = (sn2_cdiv(sn2_cdiv(n_chunks, L), 4) + 7) & ~7;
    auto kc = p->act_bf16 ? &fp_bwd_src_chunk_kernel<CA, CB, CO, true> : &fp_bwd_src_chunk_kernel<CA, CB, CO, false>;
    if (parts & 2)
        hipLaunchKernelGGL(kc, dim3(gc), dim3(256), 0, st, n_chunks, L, R, Rp, S, (const int4*)x.chunks, (const int*)x.inv_row,
                           (const float*)x.inv_w, (const float*)p->du_scratch, p->src_ws);
    if (parts & 4)
        hipLaunchKernelGGL((fp_bwd_src_merge_dw_kernel<CA, CB, CO>), dim3(sn2_cdiv(n_src, 64)), dim3(256), 0, st, n_src, S, x.CM,
                           p->src_stride, p->dsrc_stride, (const int4*)x.items, p->src, p->src_a, p->src_c,
                           (const float*)p->src_ws, p->blk.W, p->dsrc,
                           p->blk.dW, p->blk.grad_replicas, p->blk.grad_replica_stride, L);
    SN2_RETURN_LAUNCH();
}

template <int CA, int CB, int CO, bool KNN>
int bwd_dense(const sn2_fp* p, hipStream_t st) {
    using Acc = OuterAcc<CO, CA + CB + 1, 32>;
    // waves per workgroup (one workgroup per CU): as many as the staging regions and 256 VGPRs per lane allow
    constexpr int WAVES = (Acc::LDS_FLOATS * 4 * 8 <= 150 * 1024) ? 8 : ((Acc::LDS_FLOATS * 4 * 4 <= 150 * 1024) ? 4 : 2);
    constexpr size_t lds_bytes = (size_t)Acc::LDS_FLOATS * 4 * WAVES;
    int grid = pick_grid(p->B * p->R_per_plot, WAVES * 64, 4);
    if (grid > 256) grid = 256;
    return launch_bwd_rows<CA, KNN>(&fp_bwd_main_kernel<CA, CB, CO, KNN, WAVES>, grid, WAVES * 64, lds_bytes, p, st);
}

// the transpose of the interpolation for Split and Dense: dsrc += the rows of du_scratch, gathered through the inverted index
template <int CA>
int bwd_gather(const sn2_fp* p, hipStream_t st) {
    const int S = p->S_per_plot, Rp = p->R_per_plot, B = p->B, n_src = B * S;
    if (!p->scatter_ready) SN2_TRY(build_interp_index(p->knn_idx, p->knn_w, nullptr, B, Rp, S, p->scatter_ws, st));
    const InterpIndex x = carve_interp_index(p->scatter_ws, B, Rp, S);
    if ((long)Rp >= 128L * S && CA <= 64)     // >= 128 entries per list on average: a workgroup per source
        hipLaunchKernelGGL((interp_gather_long_kernel<CA, 16>), dim3(n_src), dim3(1024), 0, st, n_src, Rp, S,
                           p->dsrc_stride, (const int*)x.off, (const int*)x.cnt, (const int*)x.inv_row, (const float*)x.inv_w,
                           (const float*)p->du_scratch, p->dsrc);
    else
        hipLaunchKernelGGL((interp_gather_kernel<CA>), dim3(sn2_cdiv(n_src, 4)), dim3(256), 0, st, n_src, Rp, S,
                           p->dsrc_stride, (const int*)x.off, (const int*)x.cnt, (const int*)x.inv_row, (const float*)x.inv_w,
                           (const float*)p->du_scratch, p->dsrc);
    SN2_RETURN_LAUNCH();
}

template <int CA, int CB, int CO, bool KNN>
int fp_backward_t(const sn2_fp* p, hipStream_t st) {
    FpForm form;
    SN2_TRY((fp_backward_plan<CA, CB, CO, KNN>(p, &form)));
    SN2_TRY(bwd_bn_sums<CO>(p, st));
    switch (form) {
    case FpForm::Split: SN2_TRY((bwd_split<CA, CB, CO, KNN>(p, st))); break;
    case FpForm::Dense: SN2_TRY((bwd_dense<CA, CB, CO, KNN>(p, st))); break;
    case FpForm::SourceSide:
        if constexpr (FP_SRC_SIDE_CB<CB, KNN>) return bwd_source_side<CA, CB, CO>(p, st);
        return SN2_EINVAL;
    }
    return fp_backward_gathers<KNN>(p) ? bwd_gather<CA>(p, st) : 0;
}

// sn2_fp_form: pass 0 / 1 / 2 = the forward in that mode, 3 = the backward
template <int CA, int CB, int CO, bool KNN>
int fp_form_t(const sn2_fp* p, int pass) {
    FpForm form;
    if (pass == 3) SN2_TRY((fp_backward_plan<CA, CB, CO, KNN>(p, &form)));
    else SN2_TRY((fp_forward_plan<CA, CB, CO, KNN>(p, pass, &form)));
    return (int)form;
}

// the four dense-row blocks of the reference architecture (model/point_net2.py:83,88-93)
#define FP_DISPATCH(FN, ...)                                                                                      \
    do {                                                                                                          \
        const bool knn = p->knn_idx != nullptr;                                                                   \
        if (!knn && p->ca == 32 && p->cb == 3 && p->blk.cout == 64) return FN<32, 3, 64, false>(__VA_ARGS__);     \
        if (knn && p->ca == 64 && p->cb == 32 && p->blk.cout == 64) return FN<64, 32, 64, true>(__VA_ARGS__);     \
        if (knn && p->ca == 64 && p->cb == 16 && p->blk.cout == 34) return FN<64, 16, 34, true>(__VA_ARGS__);     \
        if (knn && p->ca == 34 && p->cb == 8 && p->blk.cout == 34) return FN<34, 8, 34, true>(__VA_ARGS__);       \
        /* FP1 over four point features (n_input_feats = 6): one skip quad per row instead of two */              \
        if (knn && p->ca == 34 && p->cb == 4 && p->blk.cout == 34) return FN<34, 4, 34, true>(__VA_ARGS__);       \
        /* the two extra blocks of the 3sa-arch variant: global SA on [x3 | pos3], FP4 on [global | x3] */       \
        if (!knn && p->ca == 64 && p->cb == 3 && p->blk.cout == 64) return FN<64, 3, 64, false>(__VA_ARGS__);     \
        if (knn && p->ca == 64 && p->cb == 64 && p->blk.cout == 64) return FN<64, 64, 64, true>(__VA_ARGS__);     \
        return SN2_ELIMIT;                                                                                        \
    } while (0)

}  // namespace

// Routes (include/strata_hip.h).  The templates above instantiate the source-side kernels for the blocks whose cb passes the
// same test at compile time (FP_SRC_SIDE_CB).
extern "C" int sn2_fp_rows_small(long R) { return sn2_cdiv(R, 64) <= SN2_STAT_SLOTS; }
extern "C" int sn2_fp_source_side(long R, int cb, int force) {
    return cb > 0 && cb <= 16 && cb % 4 == 0 && (!sn2_fp_rows_small(R) || force);
}
extern "C" size_t sn2_fp_src_ws_words(int B, int R_per_plot, int S_per_plot, int cout) {
    return SN2_FP_SRC_WS_WORDS(B, R_per_plot, S_per_plot, cout);
}
extern "C" int sn2_fp_form(const sn2_fp* p, int pass) {
    SN2_TRY(check_fp(p));
    if (pass < 0 || pass > 3) return SN2_EINVAL;
    FP_DISPATCH(fp_form_t, p, pass);
}

extern "C" int sn2_fp_forward(const sn2_fp* p, int training, void* stream) {
    SN2_TRY(check_fp(p));
    FP_DISPATCH(fp_forward_t, p, training, (hipStream_t)stream);
}

extern "C" int sn2_fp_backward(const sn2_fp* p, void* stream) {
    SN2_TRY(check_fp(p));
    FP_DISPATCH(fp_backward_t, p, (hipStream_t)stream);
}
