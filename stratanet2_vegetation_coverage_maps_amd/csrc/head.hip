// head.hip -- the pointwise head (lin1 -> ReLU -> dropout -> lin2 -> softmax x sigmoid) forward and backward on the matrix
// cores, the eval kernels that fuse the per-point layer FP1 (source-side form) with the head, and the BatchNorm gradient sums
// taken from the consumer's weight gradients.  Entry points: sn2_head_forward, sn2_fp_head_eval, sn2_head_bn_sums,
// sn2_fp_bn_sums, sn2_head_backward.  Replaces the head of PointNet2.forward.  The three forward kernels (head_fwd_mfma_kernel,
// fp_head_eval_kernel, fp_head_eval2_kernel) fill a wave's LDS tile in their own way and share ONE head turn on it (HeadLaneW,
// head_fwd_turn).  The rows' accessors, WAVE_LDS_SYNC, the row side's input stream and arithmetic (fp_row_quad, fp_table_rows)
// and the source table come from fp_rows.h.
#include "fp_rows.h"
#include "loss_rules.h"

namespace {

// a wave re-reads LDS words other lanes of the SAME wave wrote: the LDS executes a wave's instructions in order, the compiler
// must not move the accesses across this point (the regions are reused under different element types)
// (WAVE_LDS_SYNC: defined with fp_src_table_mfma_kernel in fp_rows.h)
constexpr int HEAD_T_QUADS = 64 * 9;   // a wave's 64 consecutive rows of 36 floats: 9216 contiguous bytes, nine quads per lane

// The head forward on the matrix cores (rows of exactly 36 floats).  Per wave and turn 64 consecutive rows:
//   global -> LDS (nine fully coalesced float4 loads; one row per lane, 144-byte stride, touched 64 lines per load) -> lin1: A[row][k] = fa_k f + fc_k read back from LDS
//   in the MFMA operand layout (stride 36: conflict-free), B = W1^T in nine registers per lane, bias = accumulator start
//   -> ReLU (+ dropout) in the result layout -> z1 to LDS [64][20] -> lin2 the same way (four k-steps, five live outputs)
//   -> scores to LDS [64][8] -> one row per lane: softmax, sigmoid, two coalesced float4 stores.
// 52 MFMAs per 64 rows instead of 624 FMA instructions per row-lane fed by scalar weight loads.  It is NOT faster than that
// form (24-28 us for 92 MB either way: the kernel streams at 3.3-3.8 TB/s and fp32 MFMA has the packed-VALU rate, 2 x the
// scalar-operand FMA rate); it frees the VALU and scalar cache for whatever runs beside it.  The backward
// (head_bwd_mfma_kernel, round 4) is built the same way.
// The three forward kernels differ in how the tile is filled -- head_fwd_mfma_kernel loads 64 stored rows, the eval kernels compute
// 63 rows of FP1 into it --; what follows the WAVE_LDS_SYNC that publishes the tile is head_fwd_turn, stated once.

// the head's weights of lane (n, kq) in the MFMA operand layout, in registers for the whole kernel: column n of W1^T and of W2^T
// and the rows' affine (fa, fc) at the k indices 4 ks + kq of the lane's k-steps; the biases the accumulators start from
struct HeadLaneW {
    float w1[9], ak[9], ck[9], w2[4], bias1, bias2;
};
__device__ __forceinline__ HeadLaneW head_lane_w(const float* __restrict__ fa, const float* __restrict__ fc,
                                                 const float* __restrict__ W1, const float* __restrict__ b1,
                                                 const float* __restrict__ W2, const float* __restrict__ b2, int n, int kq) {
    HeadLaneW hw;
#pragma unroll
    for (int ks = 0; ks < 9; ++ks) {
        const int k = 4 * ks + kq;
        hw.w1[ks] = k < 34 ? W1[n * 34 + k] : 0.f;
        hw.ak[ks] = k < 34 ? fa[k] : 0.f;
        hw.ck[ks] = k < 34 ? fc[k] : 0.f;
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) hw.w2[ks] = n < 5 ? W2[n * 16 + 4 * ks + kq] : 0.f;
    hw.bias1 = b1[n], hw.bias2 = n < 5 ? b2[n] : 0.f;
    return hw;
}

// The head's turn on a wave's filled tile st [64][36] (rows r0 .. r0 + ROWS - 1 of R; the caller has published the tile with
// WAVE_LDS_SYNC): lin1 -> ReLU (+ dropout) -> zt -> lin2 -> sc -> softmax, sigmoid, two float4 stores of the rows < ROWS.
// drop_mask / drop_scale: F.dropout(relu(lin1), p) of model/point_net2.py:142 -- bit j of the row's word set = channel j kept and
// scaled by 1/(1-p); a caller that passes nullptr (the eval kernels) compiles no dropout.
template <int ROWS>
__device__ __forceinline__ void head_fwd_turn(const HeadLaneW& hw, float* __restrict__ st, long r0, int R, float* __restrict__ cov,
                                              float* __restrict__ proba, const int* __restrict__ drop_mask, float drop_scale) {
    static_assert(ROWS > 0 && ROWS <= 64, "at most the tile's 64 rows");
    const int lane = threadIdx.x & 63, n = lane & 15, kq = lane >> 4;
    float* zt = st;                    // [64][20] after lin1 has read the rows
    float* sc = st + 64 * 20;          // [64][8]
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        acc[t] = f32x4{hw.bias1, hw.bias1, hw.bias1, hw.bias1};
#pragma unroll
        for (int ks = 0; ks < 9; ++ks) {
            const float v = st[(16 * t + n) * 36 + 4 * ks + kq];
            const float a = (4 * ks + kq < 34) ? fmaf(hw.ak[ks], v, hw.ck[ks]) : 0.f;
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, hw.w1[ks], acc[t], 0, 0, 0);
        }
    }
    WAVE_LDS_SYNC();
    // acc[t][j]: row 16 t + 4 kq + j, hidden channel n
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = 16 * t + 4 * kq + j;
            float z = fmaxf(acc[t][j], 0.f);
            if (drop_mask) {
                const long r = r0 + row;
                const int keep = drop_mask[r < R ? r : R - 1];
                z = ((keep >> n) & 1) ? z * drop_scale : 0.f;
            }
            zt[row * 20 + n] = z;
        }
    WAVE_LDS_SYNC();
    f32x4 s2[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        s2[t] = f32x4{hw.bias2, hw.bias2, hw.bias2, hw.bias2};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
            s2[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(zt[(16 * t + n) * 20 + 4 * ks + kq], hw.w2[ks], s2[t], 0, 0, 0);
    }
    if (n < 8) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) sc[(16 * t + 4 * kq + j) * 8 + n] = s2[t][j];
    }
    WAVE_LDS_SYNC();
    const long r = r0 + lane;
    const float4 s03 = *reinterpret_cast<const float4*>(&sc[lane * 8]);
    const float s4 = sc[lane * 8 + 4];
    WAVE_LDS_SYNC();
    const float sv[4] = {s03.x, s03.y, s03.z, s03.w};
    const float m = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
    float e[4], den = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        e[i] = expf(sv[i] - m);
        den += e[i];
    }
    float pr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) pr[i] = e[i] / den;
    const float dens = 1.0f / (1.0f + expf(-s4));
    if ((ROWS == 64 || lane < ROWS) && r < R) {
        reinterpret_cast<float4*>(proba)[r] = make_float4(pr[0], pr[1], pr[2], pr[3]);
        reinterpret_cast<float4*>(cov)[r] = make_float4(pr[0] * dens, pr[1] * dens, pr[2] * dens, pr[3] * dens);
    }
}

// workgroups per CU head_fwd_mfma_kernel is compiled for = its register budget.  At 4 (128 VGPRs, one spilled) the compiler issued the nine
// row loads of a turn ONE BY ONE, each behind an s_waitcnt vmcnt(0) of its own (every load into the same four registers): 23.4 us
// at config 2; at 3 / 2 the loads are in flight together: 22.3 / 22.1 us (scripts/time_head_fwd.py)
#ifndef SN2_HF_OCC
#define SN2_HF_OCC 3
#endif
template <bool BF>
__global__ __launch_bounds__(256, SN2_HF_OCC) void head_fwd_mfma_kernel(int R, const float* __restrict__ f, const float* __restrict__ fa,
                                                            const float* __restrict__ fc, const float* __restrict__ W1,
                                                            const float* __restrict__ b1, const float* __restrict__ W2,
                                                            const float* __restrict__ b2, float* __restrict__ cov,
                                                            float* __restrict__ proba, const int* __restrict__ drop_mask,
                                                            float drop_scale, float4* __restrict__ zero4, long nzero4) {
    __shared__ float4 s_t[4 * HEAD_T_QUADS];
    // sn2_head.zero_fill: the backward pass's accumulate-into arena, cleared here -- 5 MB of stores beside 92 MB of rows --
    // instead of by a launch of its own in front of the backward pass (4.9 us: the floor of any launch on this chip)
    if (zero4)
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nzero4; i += (long)gridDim.x * 256) zero4[i] = float4{0.f, 0.f, 0.f, 0.f};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float4* st4 = s_t + wave * HEAD_T_QUADS;
    const HeadLaneW hw = head_lane_w(fa, fc, W1, b1, W2, b2, lane & 15, lane >> 4);
    for (long r0 = ((long)blockIdx.x * 4 + wave) * 64; r0 < R; r0 += (long)gridDim.x * 256) {
        {
            const long lim = (R - r0) * 9;
            float4 t[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int e = lane + 64 * k;
                // quad e of the wave's 64 consecutive rows: 16 bytes of fp32 or 8 bytes of bfloat16, contiguous either way
                // (unconditional loads from a clamped address: a load under a divergent branch is waited for at the join)
                const float4 v = row_quad_ld<BF>(f, (size_t)r0, 36, e < lim ? e : 0);
                t[k] = e < lim ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) st4[lane + 64 * k] = t[k];
        }
        WAVE_LDS_SYNC();
        head_fwd_turn<64>(hw, reinterpret_cast<float*>(st4), r0, R, cov, proba, drop_mask, drop_scale);
    }
}

// EVAL: the per-point layer FP1 (source-side form: fp_fwd_rows_kernel's row side) and the head in ONE kernel.  An eval pass keeps
// nothing for a backward, so the 144-byte rows of h1 need not exist: a wave computes 63 consecutive rows (nine groups of seven,
// nine lanes per row as in fp_fwd_rows_kernel) straight into the LDS tile head_fwd_mfma_kernel reads its rows from, and runs
// that kernel's turn on it (row 63 of the tile is padding).  The row side (fp_table_rows, fp_row_quad) and the turn (head_fwd_turn)
// are the device functions the two kernels call -- the same operations in the same order: the same bits.  Saves the write and the read of h1 (parcel inference: 740 MB per launch of 256 plots) and a launch.
template <int CA, int CB, int CO>
__global__ __launch_bounds__(256, 2) void fp_head_eval_kernel(int R, int R_per_plot, int S_per_plot, int skip_stride,
                                                              const float* __restrict__ T, const int* __restrict__ knn_idx,
                                                              const float* __restrict__ knn_w, const float* __restrict__ skip,
                                                              const float* __restrict__ Wg, const float* __restrict__ biasg,
                                                              const float* __restrict__ fa, const float* __restrict__ fc,
                                                              const float* __restrict__ W1, const float* __restrict__ b1,
                                                              const float* __restrict__ W2, const float* __restrict__ b2,
                                                              float* __restrict__ cov, float* __restrict__ proba) {
    constexpr int QH = (CO + 3) / 4, HS = 4 * QH, G = 64 / QH, QB = CB / 4, U = 3, ROWS = G * 9;
    static_assert(CO == 34 && HS == 36 && G == 7 && ROWS == 63, "the head reads rows of 36 floats, 63 per turn");
    static_assert(CB > 0 && CB % 4 == 0, "skip quads");
    __shared__ float4 s_t[4 * HEAD_T_QUADS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float4* st4 = s_t + wave * HEAD_T_QUADS;
    const int q = lane % QH, g = lane / QH;
    const bool on = lane < G * QH;
    // the row side's weights (fp_fwd_rows_kernel) and the head's (head_fwd_mfma_kernel), in registers for the whole kernel
    const FpQuadW<CB> fw = fp_quad_w<CA, CB, CO>(Wg, biasg, q);
    const HeadLaneW hw = head_lane_w(fa, fc, W1, b1, W2, b2, lane & 15, lane >> 4);
    const long n_turns = ((long)R + ROWS - 1) / ROWS;
    for (long turn = (long)blockIdx.x * 4 + wave; turn < n_turns; turn += (long)gridDim.x * 4) {
        const long r0 = turn * ROWS;
        // ---- FP1, rows r0 .. r0 + 62 -> the tile (a group of seven rows per step, U groups' loads in flight)
#pragma unroll 1
        for (int g0 = 0; g0 < 9; g0 += U) {
            FpRowIn<QB> in[U];
            float4 ta[U][3];
#pragma unroll
            for (int u = 0; u < U; ++u) in[u] = fp_row_in<QB>(r0 + (long)(g0 + u) * G + g, on, R, knn_idx, knn_w, skip, skip_stride);
#pragma unroll
            for (int u = 0; u < U; ++u)
                fp_table_rows<HS>(T, (in[u].rr / (unsigned)R_per_plot) * (unsigned)S_per_plot, in[u].i0, in[u].i1, in[u].i2, q, ta[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float v[4];
                fp_row_quad<CB, CO>(fw, ta[u], in[u].w0, in[u].w1, in[u].w2, in[u].sk, in[u].valid, q, v);
                if (on) st4[((g0 + u) * G + g) * QH + q] = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
        if (lane < QH) st4[ROWS * QH + lane] = make_float4(0.f, 0.f, 0.f, 0.f);      // row 63: padding
        WAVE_LDS_SYNC();
        // ---- the head on the tile
        head_fwd_turn<ROWS>(hw, reinterpret_cast<float*>(st4), r0, R, cov, proba, nullptr, 1.f);
    }
}

// The same kernel with the row side's INPUT STREAM decoupled from the lanes that consume it, as fp_fwd_rows2_kernel (round 5).  The
// first form's nine lanes of a row load the row's 3-NN entry and skip columns themselves, then gather, then compute, three groups
// of seven rows at a time: six memory round trips per 63-row turn, one after the other, in front of the head's arithmetic.  Here
// a wave fetches a whole turn's 189 indices, 189 weights and 63 x QB skip quads with one element per lane and load (3 + 3 + NSK loads: eight
// with two skip quads per row, seven with one),
// ONE TURN AHEAD (the loads are issued in front of the head phase of the turn before), hands them to the (row, quad) lanes
// through LDS, and asks for a batch's table rows before it computes the batch before: one round trip per turn is left in the
// open.  Turns dealt XCD-aware (row_iters: an XCD's L2 holds its own plots' table rows).  Same operations in the same order:
// the same bits as the first form (sn2_debug_fp_rows_form(0)) and as the two separate kernels.
template <int CA, int CB, int CO>
__global__ __launch_bounds__(256, 2) void fp_head_eval2_kernel(int R, int R_per_plot, int S_per_plot, int skip_stride,
                                                               const float* __restrict__ T, const int* __restrict__ knn_idx,
                                                               const float* __restrict__ knn_w, const float* __restrict__ skip,
                                                               const float* __restrict__ Wg, const float* __restrict__ biasg,
                                                               const float* __restrict__ fa, const float* __restrict__ fc,
                                                               const float* __restrict__ W1, const float* __restrict__ b1,
                                                               const float* __restrict__ W2, const float* __restrict__ b2,
                                                               float* __restrict__ cov, float* __restrict__ proba) {
    constexpr int QH = (CO + 3) / 4, HS = 4 * QH, G = 64 / QH, QB = CB / 4, U = 3, ROWS = G * 9;
    static_assert(CO == 34 && HS == 36 && G == 7 && ROWS == 63, "the head reads rows of 36 floats, 63 per turn");
    static_assert(CB > 0 && CB % 4 == 0, "skip quads");
    constexpr int NSK = (ROWS * QB + 63) / 64;                                 // skip quads per lane and turn (QB = 2: 126 quads = two per lane; QB = 1: one)
    constexpr int XW = 3 * ROWS + 3 * ROWS + 4 * ROWS * QB + 2;                // idx | w | skip quads (16-byte aligned: 378 % 4 = 2 -> +2)
    constexpr int XO_W = 3 * ROWS, XO_S = 6 * ROWS + 2;
    static_assert(XO_S % 4 == 0, "the skip quads start 16-byte aligned");
    typedef float f32x4v __attribute__((ext_vector_type(4)));
    __shared__ float4 s_t[4 * HEAD_T_QUADS];
    __shared__ __attribute__((aligned(16))) float s_x[4][(XW + 3) / 4 * 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float4* st4 = s_t + wave * HEAD_T_QUADS;
    float* xw = s_x[wave];
    const int q = lane % QH, g = lane / QH;
    const bool on = lane < G * QH;
    const FpQuadW<CB> fw = fp_quad_w<CA, CB, CO>(Wg, biasg, q);
    const HeadLaneW hw = head_lane_w(fa, fc, W1, b1, W2, b2, lane & 15, lane >> 4);
    const int n_turns = (R + ROWS - 1) / ROWS;
    const RowIters ri = row_iters(n_turns, wave);
    // ---- a turn's inputs, one element per lane and load, unconditional from clamped addresses
    int p_idx[3];
    float p_w[3];
    f32x4v p_sk[NSK];
    const int last_e = 3 * R - 1;
    auto fetch = [&](int turn) {
        const int tc = turn < ri.it_hi ? turn : ri.it_hi - 1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int el = lane + 64 * k < 3 * ROWS ? lane + 64 * k : 3 * ROWS - 1;
            const int e0 = tc * (3 * ROWS) + el, e = e0 < last_e ? e0 : last_e;
            p_idx[k] = knn_idx[e];
            p_w[k] = knn_w[e];
        }
#pragma unroll
        for (int k = 0; k < NSK; ++k) {
            const int el = lane + 64 * k < ROWS * QB ? lane + 64 * k : ROWS * QB - 1;
            const int r0 = tc * ROWS + el / QB, r = r0 < R ? r0 : R - 1;
            p_sk[k] = reinterpret_cast<const f32x4v*>(skip + (size_t)r * skip_stride)[el % QB];
        }
    };
    auto hand_over = [&]() {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int el = lane + 64 * k < 3 * ROWS ? lane + 64 * k : 3 * ROWS - 1;     // (the surplus lanes rewrite the last element)
            xw[el] = __int_as_float(p_idx[k]);
            xw[XO_W + el] = p_w[k];
        }
#pragma unroll
        for (int k = 0; k < NSK; ++k) {
            const int el = lane + 64 * k < ROWS * QB ? lane + 64 * k : ROWS * QB - 1;
            reinterpret_cast<f32x4v*>(xw + XO_S)[el] = p_sk[k];
        }
        WAVE_LDS_SYNC();
    };
    // the table rows of batch `bt` (groups 3 bt .. 3 bt + 2) of the turn
    auto gathers = [&](int turn, int bt, float4 (&ta)[U][3]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int rl = on ? (3 * bt + u) * G + g : 0;                     // row of the turn
            const int row = turn * ROWS + rl;
            const bool valid = on && row < R;
            const unsigned rr = valid ? (unsigned)row : 0u;
            const int i0 = valid ? __float_as_int(xw[3 * rl + 0]) : 0, i1 = valid ? __float_as_int(xw[3 * rl + 1]) : 0,
                      i2 = valid ? __float_as_int(xw[3 * rl + 2]) : 0;
            fp_table_rows<HS>(T, (rr / (unsigned)R_per_plot) * (unsigned)S_per_plot, i0, i1, i2, q, ta[u]);
        }
    };
    auto rows_of = [&](int turn, int bt, const float4 (&ta)[U][3]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int rl = on ? (3 * bt + u) * G + g : 0;
            const int row = turn * ROWS + rl;
            const bool valid = on && row < R;
            float4 sk[QB];
#pragma unroll
            for (int b = 0; b < QB; ++b) sk[b] = reinterpret_cast<const float4*>(xw + XO_S)[rl * QB + b];
            float v[4];
            fp_row_quad<CB, CO>(fw, ta[u], xw[XO_W + 3 * rl + 0], xw[XO_W + 3 * rl + 1], xw[XO_W + 3 * rl + 2], sk, valid, q, v);
            if (on) st4[((3 * bt + u) * G + g) * QH + q] = make_float4(v[0], v[1], v[2], v[3]);
        }
    };
    if (ri.it0 < ri.it_hi) fetch(ri.it0);
    for (int turn = ri.it0; turn < ri.it_hi; turn += ri.stride) {
        const long r0 = (long)turn * ROWS;
        // ---- FP1, rows r0 .. r0 + 62 -> the tile
        hand_over();
        float4 ta_a[U][3], ta_b[U][3];
        gathers(turn, 0, ta_a);
        gathers(turn, 1, ta_b);
        rows_of(turn, 0, ta_a);
        gathers(turn, 2, ta_a);
        rows_of(turn, 1, ta_b);
        rows_of(turn, 2, ta_a);
        if (lane < QH) st4[ROWS * QH + lane] = make_float4(0.f, 0.f, 0.f, 0.f);      // row 63: padding
        WAVE_LDS_SYNC();
        fetch(turn + ri.stride);                              // the NEXT turn's inputs travel while the head runs (clamped past the end)
        // ---- the head on the tile
        head_fwd_turn<ROWS>(hw, reinterpret_cast<float*>(st4), r0, R, cov, proba, nullptr, 1.f);
    }
}

// The head backward on the matrix cores (round 4; rows of exactly 36 floats).  Its predecessor gave every lane one row: ~1900
// FMA instructions per row, a third of them on the two weight-gradient outer products through an LDS transposition, behind
// 144-byte strided row loads and stores (64 lines per instruction): 57 us for 168 MB.  Here a wave takes 64 consecutive rows
// per turn, as head_fwd_mfma_kernel does, and every contraction is a chain of 16x16x4 tiles fed from three LDS regions:
//   st [64][36]  y = fa f + fc (applied once, on the way in from the coalesced float4 loads; column 34 := 1 -- the bias
//                column of [y | 1] --, column 35 := 0); at the end of the turn the d rows, stored coalesced the same way
//   zt [64][20]  z1 = dropout(relu(lin1)) for lin2 and dW2, then d pre-activation of lin1 for dW1 and the d rows
//   sc [64][12]  the five scores, then their gradients (softmax / sigmoid backward with one row per lane), columns 5..7 zero
//   lin1 36 + lin2 16 + dW2 16 + d pre 8 + dW1 48 + d rows 48 = 172 tiles per 64 rows; dW1 | db1 and dW2 stay in
//   accumulators for the whole kernel, db2 is a per-lane sum; the next turn's rows and gradients are requested before the
//   current turn's arithmetic.
// LDS traffic, not the matrix cores, is what the layout is about (ds_read_b32 / ds_write_b32: 32 banks, lanes 0..31 and
// 32..63 apart; ds_read_b64: 64 banks):
//   * a tile's k index is free as long as both operands agree.  Where a lane's operand runs along a ROW (lin1, lin2, d pre,
//     d rows: lane (n, kq) = row n of the tile) steps 2p and 2p+1 take columns 8p + 2kq and 8p + 2kq + 1: ONE ds_read_b64
//     per two tiles, conflict-free at the even strides 36 / 20 / 12 (the plain 4 ks + kq columns are 2-way, 4-way at 12);
//   * where it runs along a COLUMN (dW2, dW1: lane (n, kq) = column n) step s takes rows 16 (s / 4) + s % 4 + 4 kq: lanes
//     kq and kq + 1 are four rows = 16 banks apart at every stride.
//   * the per-lane weight operands (30 floats) live in a table of float4 per (quad, lane), read phase by phase: held in
//     registers for the whole loop they left no room beside the prefetched rows (spills, and a spill's reload waits for the
//     prefetch with it).
// Operands are read in batches in front of their tiles (sched_barrier: left alone the scheduler puts every read right in front
// of its tile and pays the LDS latency 170 times per turn).
// Same sums as the row-per-lane form up to fp32 re-association.
#ifdef SN2_HB_STAMPS
// diagnostic build only (never shipped): phase stamps of wave 0 of one workgroup of head_bwd_mfma_kernel, second turn
__device__ unsigned long long g_hb_dbg[16];
extern "C" int sn2_debug_hb_stamps(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_hb_dbg), sizeof(g_hb_dbg));
}
#define HSTAMP(i)                                                                                   \
    if (blockIdx.x == 37 && threadIdx.x == 0 && turn_no == 1) {                                     \
        unsigned long long t_;                                                                      \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                   \
        g_hb_dbg[i] = t_;                                                                           \
    }
#else
#define HSTAMP(i)
#endif
// one ds_read_b64 (left to the compiler two of them at nearby offsets become a ds_read2_b64: banked like ds_read_b32, 4 x the
// cycles).  The compiler does not count this read: the caller waits (HB_WAIT_B64) before the first use.
typedef float hb_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ hb_f32x2 lds_read_b64(const float* p) {
    hb_f32x2 v;
    const unsigned a = (unsigned)(size_t)(const __attribute__((address_space(3))) float*)p;
    asm volatile("ds_read_b64 %0, %1" : "=v"(v) : "v"(a) : "memory");
    return v;
}
typedef unsigned hb_u32x4 __attribute__((ext_vector_type(4)));
typedef hb_u32x4 hb_u32x4_a8 __attribute__((aligned(8)));       // a 16-byte load from an 8-byte aligned address (a row's fp64 densities)
constexpr int HB_ST = 64 * 36, HB_ZT = 64 * 20, HB_SC = 64 * 12;
constexpr int HB_WAVE_FLOATS = HB_ST + HB_ZT + HB_SC + 64;      // + the rows' dropout words
#ifndef SN2_HB_DIAG
#define SN2_HB_DIAG 0      /* timing experiments (scripts/time_head_bwd.py): 1 = no d-row stores, 2 = no arithmetic (rows in, rows out) */
#endif
constexpr int HB_DIAG = SN2_HB_DIAG;
constexpr int HB_CQ = 8;                                        // float4 quads of per-lane weight operands (one table per workgroup)
constexpr int HB_TAB_FLOATS = HB_CQ * 64 * 4 + 18 * 4;          // + fa, fc as nine quads each
constexpr int HB_RED = 16 * 35 + 5 * 16 + 5;                    // a wave's weight-gradient image: dW1 | db1, dW2, db2
template <bool BF>
__global__ __launch_bounds__(256, 2) void head_bwd_mfma_kernel(int R, const float* __restrict__ f, const float* __restrict__ fa,
                                                            const float* __restrict__ fc, const float* __restrict__ W1,
                                                            const float* __restrict__ b1, const float* __restrict__ W2,
                                                            const float* __restrict__ b2, const float* __restrict__ dcov,
                                                            const float* __restrict__ dproba, float* __restrict__ dy,
                                                            float* __restrict__ dW1, float* __restrict__ db1,
                                                            float* __restrict__ dW2, float* __restrict__ db2, int rep_k,
                                                            int rep_stride, const int* __restrict__ drop_mask, float drop_scale,
                                                            const sn2_loss_grad lg) {
    typedef hb_f32x2 f32x2;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the fused route (sn2_head.loss; wave-uniform, as dcov / dproba / drop_mask are): the incoming gradients of a row are
    // computed in its one-row-per-lane phase from the loss's own inputs (loss_rules.h) instead of being read
    const bool loss = lg.proba != nullptr;
    float* st = smem + wave * HB_WAVE_FLOATS;
    float4* st4 = reinterpret_cast<float4*>(st);
    float* zt = st + HB_ST;
    float* sc = zt + HB_ZT;
    int* mk = reinterpret_cast<int*>(sc + HB_SC);
    const int n = lane & 15, kq = lane >> 4;
    float* tab = smem + 4 * HB_WAVE_FLOATS;
    float4* ptab = reinterpret_cast<float4*>(tab + HB_TAB_FLOATS);          // fused route: (gx, gz, gw, 1 / nocc) per plot ...
    double* pco = reinterpret_cast<double*>(ptab + PL_HEAD_MAX_PLOTS);      // ... and the two row coefficients (cn, ce)
    if (loss && wave >= 2) {
        // the fp64 square roots and divisions of d loss / d pred: once per plot and workgroup (waves 2, 3; wave 0 fills the
        // weight table below) instead of once per point
        const int pb = (int)threadIdx.x - 128;
        const double g = lg.grad_total[0];
        if (pb < lg.B) ptab[pb] = pl_plot_grad(lg.pred, lg.gt, lg.nocc, pb, lg.B, g);
        if (pb == 0) pl_row_coeffs(g, lg.m, lg.e, (size_t)R, pco[0], pco[1]);
    }
    // ---- the weight operands of lane (n, kq) -> the table
    if (wave == 0) {
        float c[4 * HB_CQ];
#pragma unroll
        for (int pp = 0; pp < 4; ++pp) {                        // lin1: B[k][n] = W1[n][k], k = 8 pp + 2 kq (+ 1)
            c[2 * pp] = W1[n * 34 + 8 * pp + 2 * kq];
            c[2 * pp + 1] = W1[n * 34 + 8 * pp + 2 * kq + 1];
        }
        c[8] = kq < 2 ? W1[n * 34 + 32 + kq] : 0.f;             // ... and the ninth step: k = 32 + kq
        c[9] = b1[n];
        c[10] = n < 5 ? b2[n] : 0.f;
        c[11] = 0.f;
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {                        // lin2: B[k][n] = W2[n][k]
            c[12 + 2 * pp] = n < 5 ? W2[n * 16 + 8 * pp + 2 * kq] : 0.f;
            c[13 + 2 * pp] = n < 5 ? W2[n * 16 + 8 * pp + 2 * kq + 1] : 0.f;
        }
        c[16] = 2 * kq < 5 ? W2[(2 * kq) * 16 + n] : 0.f;       // d pre: B[i][j] = W2[i][j], i = 2 kq (+ 1)
        c[17] = 2 * kq + 1 < 5 ? W2[(2 * kq + 1) * 16 + n] : 0.f;
        c[18] = c[19] = 0.f;
#pragma unroll
        for (int ct = 0; ct < 3; ++ct)                          // d rows: B[j][col] = W1[j][col], j = 8 pp + 2 kq (+ 1)
#pragma unroll
            for (int pp = 0; pp < 2; ++pp) {
                const int col = 16 * ct + n;
                c[20 + 4 * ct + 2 * pp] = col < 34 ? W1[(8 * pp + 2 * kq) * 34 + col] : 0.f;
                c[21 + 4 * ct + 2 * pp] = col < 34 ? W1[(8 * pp + 2 * kq + 1) * 34 + col] : 0.f;
            }
        float4* ct4 = reinterpret_cast<float4*>(tab);
#pragma unroll
        for (int q = 0; q < HB_CQ; ++q) ct4[q * 64 + lane] = make_float4(c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]);
        if (lane < 36) {                                        // [y | 1 | 0]: fa = 0 and fc = 1 in column 34, both 0 in column 35
            tab[HB_CQ * 256 + lane] = lane < 34 ? fa[lane] : 0.f;
            tab[HB_CQ * 256 + 36 + lane] = lane < 34 ? fc[lane] : (lane == 34 ? 1.f : 0.f);
        }
    }
    __syncthreads();
    const float4* ctab = reinterpret_cast<const float4*>(tab) + lane;
    const float4* fa4 = reinterpret_cast<const float4*>(tab + HB_CQ * 256);
    const float4* fc4 = fa4 + 9;
    const int lane9 = lane % 9;
    const int nn = n < 8 ? n : 5;                               // lanes n >= 8 of dW2's A operand read a zero column
    f32x4 dw1acc[3], dw2acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ct = 0; ct < 3; ++ct) dw1acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    float dsum[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    const long stride = (long)gridDim.x * 256;
    long r0 = ((long)blockIdx.x * 4 + wave) * 64;
    float4 t[9], ga = make_float4(0.f, 0.f, 0.f, 0.f);
    hb_u32x4 gb01 = {0u, 0u, 0u, 0u};           // (ONE 16-byte value, as gc / gp were: two 8-byte ones that the compiler merges into
    uint2 gb2 = make_uint2(0u, 0u);             // one load afterwards are copied apart behind it, and the copy waits for the prefetch)
    int keep = 0xFFFF, pixv = 0;
    // (a gradient or mask that is absent is loaded from the rows instead -- 16 valid bytes per row -- and dropped at its use:
    // a load under a branch, even a uniform one, is waited for where the branch joins, which would end the prefetch; for the
    // same reason the rows past the end are loaded from a clamped address: finite values whose d scores are zero)
    // The same registers serve both routes, by address selection alone: `ga` = the row's dcoverages, or its stored probabilities;
    // `gb01`, `gb2` = the 16 bytes of its dproba (and its first 8 again), or its three fp64 densities (24 B per row, 8-byte
    // aligned; none when m = 0: the dummy again); `pixv` = its pixel id.
    const float4* gap = reinterpret_cast<const float4*>(loss ? lg.proba : (dcov ? dcov : f));
    const char* gbp = loss ? reinterpret_cast<const char*>(lg.pdf ? reinterpret_cast<const float*>(lg.pdf) : f)
                           : reinterpret_cast<const char*>(dproba ? dproba : f);
    const int gb_stride = loss ? 24 : 16, gb_third = loss ? 16 : 0;
    const int* kp = drop_mask ? drop_mask : reinterpret_cast<const int*>(f);
    const int* pxp = loss ? lg.pix : reinterpret_cast<const int*>(f);
    const int* argp = loss ? lg.arg : reinterpret_cast<const int*>(f);
    const unsigned rows_per_plot = loss ? (unsigned)lg.N : 1u, ncell = loss ? (unsigned)(lg.D * lg.D) : 0u;
    auto request = [&](long q0) {               // the rows of a turn, one row's incoming gradients and dropout word per lane
        const long lim = (R - q0) * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int e = lane + 64 * k;
            t[k] = row_quad_ld<BF>(f, (size_t)q0, 36, e < lim ? e : 0);
        }
        const long r = q0 + lane;
        const size_t rr = r < R ? (size_t)r : 0;
        ga = gap[rr];
        const char* pb = gbp + rr * (size_t)gb_stride;
        gb01 = *reinterpret_cast<const hb_u32x4_a8*>(pb);
        gb2 = *reinterpret_cast<const uint2*>(pb + gb_third);
        keep = kp[rr];
        pixv = pxp[rr];
    };
    if (r0 < R) request(r0);
    int turn_no = -1;
    for (; r0 < R; r0 += stride) {
        ++turn_no;
        HSTAMP(0)
        // ---- quad e = lane + 64 k of the tile is quad (lane + k) % 9 of its row
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int q9 = lane9 + k < 9 ? lane9 + k : lane9 + k - 9;
            const float4 a4 = fa4[q9], c4 = fc4[q9], v = t[k];
            float4 y = make_float4(fmaf(a4.x, v.x, c4.x), fmaf(a4.y, v.y, c4.y), fmaf(a4.z, v.z, c4.z), fmaf(a4.w, v.w, c4.w));
            if (q9 == 8) y.z = 1.f, y.w = 0.f;                  // (whatever the rows' padding holds)
            st4[lane + 64 * k] = y;
        }
        if (drop_mask) mk[lane] = keep;
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        const bool valid = r0 + lane < R;
        // fused route: the row's plot (per LANE: a turn straddles two plots whenever N is no multiple of 64) and the arg-max
        // points of its pixel -- a second round trip that depends on the prefetched pixel id, issued here and consumed in the
        // d-scores phase, behind lin1 and lin2.  Without a descriptor: three words of the rows, dropped at their use.
        const unsigned rowi = valid ? (unsigned)(r0 + lane) : 0u;
        const unsigned plot = rowi / rows_per_plot;
        const int row_in_plot = (int)(rowi - plot * rows_per_plot);
        const int* ap = argp + (loss ? ((size_t)plot * ncell + (size_t)pixv) * 3 : (size_t)0);
        const int a0 = ap[0], a1 = ap[1], a2 = ap[2];
        WAVE_LDS_SYNC();
        HSTAMP(1)
        if (!(HB_DIAG & 2)) {
        // ---- lin1, ReLU, dropout (z[tt][j]: row 16 tt + 4 kq + j, hidden channel n)
#pragma unroll
        for (int tp = 0; tp < 4; tp += 2) {
            f32x2 av[2][4];
            float as[2];
            f32x4 z[2];
            const float4 q0 = ctab[0], q1 = ctab[64], q2 = ctab[128];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
                for (int pp = 0; pp < 4; ++pp)
                    av[tt][pp] = lds_read_b64(&st[(16 * (tp + tt) + n) * 36 + 8 * pp + 2 * kq]);
                as[tt] = st[(16 * (tp + tt) + n) * 36 + 32 + kq];
            }
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(av[0][0]), "+v"(av[0][1]), "+v"(av[0][2]), "+v"(av[0][3]), "+v"(av[1][0]), "+v"(av[1][1]), "+v"(av[1][2]), "+v"(av[1][3]) :: "memory");
            __builtin_amdgcn_sched_barrier(0);
            const float w1p[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) z[tt] = f32x4{q2.y, q2.y, q2.y, q2.y};
#pragma unroll
            for (int pp = 0; pp < 4; ++pp)
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int tt = 0; tt < 2; ++tt)
                        z[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[tt][pp][h], w1p[2 * pp + h], z[tt], 0, 0, 0);
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) z[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(as[tt], q2.x, z[tt], 0, 0, 0);
            int kw[2][4];
            if (drop_mask) {
#pragma unroll
                for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                    for (int j = 0; j < 4; ++j) kw[tt][j] = mk[16 * (tp + tt) + 4 * kq + j];
            }
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float zz = fmaxf(z[tt][j], 0.f);
                    if (drop_mask) zz = ((kw[tt][j] >> n) & 1) ? zz * drop_scale : 0.f;
                    zt[(16 * (tp + tt) + 4 * kq + j) * 20 + n] = zz;
                }
        }
        WAVE_LDS_SYNC();
        HSTAMP(2)
        // ---- lin2 -> scores
        {
            f32x2 zv[4][2];
            f32x4 s2[4];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int pp = 0; pp < 2; ++pp) zv[tt][pp] = lds_read_b64(&zt[(16 * tt + n) * 20 + 8 * pp + 2 * kq]);
            const float4 w2q = ctab[3 * 64];
            const float bias2 = ctab[2 * 64].z;
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(zv[0][0]), "+v"(zv[0][1]), "+v"(zv[1][0]), "+v"(zv[1][1]), "+v"(zv[2][0]), "+v"(zv[2][1]), "+v"(zv[3][0]), "+v"(zv[3][1]) :: "memory");
            __builtin_amdgcn_sched_barrier(0);
            const float w2p[4] = {w2q.x, w2q.y, w2q.z, w2q.w};
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) s2[tt] = f32x4{bias2, bias2, bias2, bias2};
#pragma unroll
            for (int pp = 0; pp < 2; ++pp)
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt)
                        s2[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(zv[tt][pp][h], w2p[2 * pp + h], s2[tt], 0, 0, 0);
            if (n < 8) {
#pragma unroll
                for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                    for (int j = 0; j < 4; ++j) sc[(16 * tt + 4 * kq + j) * 12 + n] = s2[tt][j];
            }
        }
        WAVE_LDS_SYNC();
        HSTAMP(3)
        // ---- one row per lane: softmax, sigmoid and their backward -> d scores
        {
            const float4 s03 = *reinterpret_cast<const float4*>(&sc[lane * 12]);
            const float s4 = sc[lane * 12 + 4];
            const float sv[4] = {s03.x, s03.y, s03.z, s03.w};
            const float m = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
            float e[4], den = 0.f, pr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                e[i] = expf(sv[i] - m);
                den += e[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) pr[i] = e[i] / den;
            const float dens = 1.0f / (1.0f + expf(-s4));
            // the incoming gradients: from the STORED probabilities on the fused route (the bits of sn2_projected_loss_backward's
            // dproba; the softmax backward below keeps the recomputed ones, as before), else what was loaded
            float4 gcv, gpv;
            if (loss) {
                const float4 pg = ptab[plot];
                pl_row_grad(lg.m != 0.0, lg.e != 0.0, ga, __hiloint2double((int)gb01.y, (int)gb01.x), __hiloint2double((int)gb01.w, (int)gb01.z),
                            __hiloint2double((int)gb2.y, (int)gb2.x), pco[0], pco[1], pg, a0, a1, a2, row_in_plot, gpv, gcv);
            } else {
                gcv = dcov ? ga : zero4;
                gpv = dproba ? make_float4(__uint_as_float(gb01.x), __uint_as_float(gb01.y), __uint_as_float(gb01.z), __uint_as_float(gb01.w)) : zero4;
            }
            const float gcs[4] = {gcv.x, gcv.y, gcv.z, gcv.w}, gps[4] = {gpv.x, gpv.y, gpv.z, gpv.w};
            float dp[4], dot = 0.f, ddens = 0.f, ds[5];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                dp[i] = fmaf(gcs[i], dens, gps[i]);
                ddens = fmaf(gcs[i], pr[i], ddens);
                dot = fmaf(dp[i], pr[i], dot);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) ds[i] = valid ? pr[i] * (dp[i] - dot) : 0.f;
            ds[4] = valid ? ddens * dens * (1.f - dens) : 0.f;
#pragma unroll
            for (int i = 0; i < 5; ++i) dsum[i] += ds[i];
            WAVE_LDS_SYNC();
            *reinterpret_cast<float4*>(&sc[lane * 12]) = make_float4(ds[0], ds[1], ds[2], ds[3]);
            *reinterpret_cast<float4*>(&sc[lane * 12 + 4]) = make_float4(ds[4], 0.f, 0.f, 0.f);
        }
        WAVE_LDS_SYNC();
        HSTAMP(4)
        // ---- dW2[i][j] += sum_rows d score[row][i] z1[row][j]   (step s: rows 16 (s / 4) + s % 4 + 4 kq)
        f32x4 dpre[4];
        {
            f32x4 odd = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                float da[8], zb[8];
#pragma unroll
                for (int s8 = 0; s8 < 8; ++s8) {
                    const int sidx = 8 * half + s8, row0 = 16 * (sidx >> 2) + (sidx & 3);
                    da[s8] = sc[(row0 + 4 * kq) * 12 + nn];
                    zb[s8] = zt[(row0 + 4 * kq) * 20 + n];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int s8 = 0; s8 < 8; s8 += 2) {
                    dw2acc = __builtin_amdgcn_mfma_f32_16x16x4f32(da[s8], zb[s8], dw2acc, 0, 0, 0);
                    odd = __builtin_amdgcn_mfma_f32_16x16x4f32(da[s8 + 1], zb[s8 + 1], odd, 0, 0, 0);
                }
            }
            HSTAMP(5)
            // ---- d pre-activation of lin1 = (d scores W2) through the dropout and the ReLU (z1 > 0: kept AND active)
            f32x2 dv[4];
            float zm[4][4];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                dv[tt] = lds_read_b64(&sc[(16 * tt + n) * 12 + 2 * kq]);
#pragma unroll
                for (int j = 0; j < 4; ++j) zm[tt][j] = zt[(16 * tt + 4 * kq + j) * 20 + n];
            }
            const float4 c4 = ctab[4 * 64];
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(dv[0]), "+v"(dv[1]), "+v"(dv[2]), "+v"(dv[3]) :: "memory");
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) dpre[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) dpre[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[tt][h], h ? c4.y : c4.x, dpre[tt], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) dw2acc[j] += odd[j];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int j = 0; j < 4; ++j) dpre[tt][j] = zm[tt][j] > 0.f ? dpre[tt][j] * drop_scale : 0.f;
        }
        WAVE_LDS_SYNC();                        // dW2 has read z1: its region takes d pre
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int j = 0; j < 4; ++j) zt[(16 * tt + 4 * kq + j) * 20 + n] = dpre[tt][j];
        WAVE_LDS_SYNC();
        HSTAMP(6)
        // (the next turn's rows are requested here, in front of the two longest tile chains, not at the top of the turn: a dozen
        // vector-memory instructions in front of lin1's LDS reads held those back -- 50.4 -> 48.8 us)
        if (r0 + stride < R) request(r0 + stride);
        // ---- dW1 | db1 += d pre^T [y | 1]   (the tile's columns 35.. feed accumulator columns nobody reads)
#pragma unroll
        for (int quarter = 0; quarter < 4; ++quarter) {
            float pa[4], yv[4][3];
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                const int row = 16 * quarter + s4 + 4 * kq;
                pa[s4] = zt[row * 20 + n];
#pragma unroll
                for (int ct = 0; ct < 3; ++ct) yv[s4][ct] = st[row * 36 + 16 * ct + n];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                for (int ct = 0; ct < 3; ++ct) dw1acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[s4], yv[s4][ct], dw1acc[ct], 0, 0, 0);
        }
        WAVE_LDS_SYNC();                        // dW1 has read the rows: their region takes the d rows
        HSTAMP(7)
        // ---- d rows = d pre W1
        {
            f32x2 pv[4][2];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int pp = 0; pp < 2; ++pp) pv[tt][pp] = lds_read_b64(&zt[(16 * tt + n) * 20 + 8 * pp + 2 * kq]);
            float w1b[3][4];
#pragma unroll
            for (int ct = 0; ct < 3; ++ct) {
                const float4 v = ctab[(5 + ct) * 64];
                w1b[ct][0] = v.x, w1b[ct][1] = v.y, w1b[ct][2] = v.z, w1b[ct][3] = v.w;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(pv[0][0]), "+v"(pv[0][1]), "+v"(pv[1][0]), "+v"(pv[1][1]), "+v"(pv[2][0]), "+v"(pv[2][1]), "+v"(pv[3][0]), "+v"(pv[3][1]) :: "memory");
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                f32x4 o[3];
#pragma unroll
                for (int ct = 0; ct < 3; ++ct) o[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int pp = 0; pp < 2; ++pp)
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int ct = 0; ct < 3; ++ct)
                            o[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv[tt][pp][h], w1b[ct][2 * pp + h], o[ct], 0, 0, 0);
#pragma unroll
                for (int ct = 0; ct < 3; ++ct) {
                    if (16 * ct + n < 36) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) st[(16 * tt + 4 * kq + j) * 36 + 16 * ct + n] = o[ct][j];
                    }
                }
            }
        }
        }
        WAVE_LDS_SYNC();
        HSTAMP(8)
        if (!(HB_DIAG & 1)) {
            const long lim = (R - r0) * 9;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int e = lane + 64 * k;
                const float4 v = st4[e];
                if (e < lim) row_quad_st<BF>(dy, (size_t)r0, 36, e, v.x, v.y, v.z, v.w);
            }
        }
        WAVE_LDS_SYNC();
        HSTAMP(9)
    }
    // ---- the wave's weight-gradient image -> LDS, summed over the workgroup's waves, one atomic per element and workgroup
    __syncthreads();
    float* img_w = smem + wave * HB_WAVE_FLOATS;
#pragma unroll
    for (int ct = 0; ct < 3; ++ct) {
        const int col = 16 * ct + n;
        if (col < 35) {
#pragma unroll
            for (int j = 0; j < 4; ++j) img_w[(4 * kq + j) * 35 + col] = dw1acc[ct][j];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (4 * kq + j < 5) img_w[16 * 35 + (4 * kq + j) * 16 + n] = dw2acc[j];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        float v = dsum[i];
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
        if (lane == 0) img_w[16 * 35 + 5 * 16 + i] = v;
    }
    __syncthreads();
    const int img = sn2_grad_image(rep_k, rep_stride);
    for (int i = threadIdx.x; i < HB_RED; i += 256) {
        const float v = (smem[i] + smem[HB_WAVE_FLOATS + i]) + (smem[2 * HB_WAVE_FLOATS + i] + smem[3 * HB_WAVE_FLOATS + i]);
        if (v == 0.f) continue;
        if (i < 16 * 35) {
            const int oo = i / 35, k = i - oo * 35;
            SN2_FLUSH_ADD(k < 34 ? &dW1[img + oo * 34 + k] : &db1[img + oo], v);
        } else if (i < 16 * 35 + 5 * 16) {
            SN2_FLUSH_ADD(&dW2[img + (i - 16 * 35)], v);
        } else {
            SN2_FLUSH_ADD(&db2[img + (i - 16 * 35 - 5 * 16)], v);
        }
    }
}

// dgamma / dbeta of a BatchNorm from the gradients of the Linear layer that consumes its output.  Let y = gamma*xhat +
// beta be the BatchNorm's output rows and let the consumer see u[r] = sum_k w_rk * y[idx_rk] with sum_k w_rk = 1 (the head:
// u = y; an FP block: the inverse-distance interpolation of knn_interpolate) in columns col0.. of its input.  With
// dy = (transposed interpolation of) W^T dpre:
//   dbeta[o]  = sum_rows dy[.][o]          = sum_j W[j][col0+o] * db[j]
//   dgamma[o] = sum_rows dy[.][o]*xhat[.][o] = sum_j W[j][col0+o] * G[j][o],  G[j][o] = sum_r dpre[r][j] * sum_k w_rk xhat[idx_rk][o]
// and dW[j][col0+o] = sum_r dpre[r][j]*u[r][o] = gamma[o]*G[j][o] + beta[o]*db[j], so G = (dW - beta*db) / gamma.
// C dot products of length cout instead of a pass over all rows (FP1's BatchNorm: 0.03 ms and 150 MB at C2).  Needs
// |gamma| > 1e-4 AND |beta| <= 64 |gamma| on every channel (bn_identity_ok); accumulated in fp64.  The subtraction
// dW - beta db cancels, and the quotient magnifies by |beta / gamma| what dW, db and the rows' fp32 affine c = beta - mean a
// carry: measured against the fp64 row pass (tests/test_gpu_bn_sums_consumer.py) dgamma is off by up to
// 1.1 x 2^-24 x |beta / gamma| of the tensor's largest element, whatever |gamma| is -- inside the 1e-5 of the gradient rule
// at |beta / gamma| = 100, 1.3e-5 ... 1.8e-5 at 800, 4.9e-3 at 8e4, and with beta = 0 within 4e-6 even at |gamma| = 1e-4.
// 64 keeps it below half of 1e-5.  When some channel fails the test the same
// workgroups make the ordinary pass themselves, one channel each over all rows (h = the BatchNorm's input rows, dyv = the
// gradient of its output that the consumer's backward left: slow -- a strided column per workgroup -- and rare), so the
// sums are complete either way and sn2_fp_backward launches no kernel of its own for them (three launches per step that
// did nothing but read a flag).  ok (device int): 1 = the identity was used, 0 = the pass over the rows.
__device__ __forceinline__ bool bn_identity_ok(float gamma, float beta) {
    return fabsf(gamma) > 1e-4f && fabsf(beta) <= 64.f * fabsf(gamma);      // (false for NaN)
}
__global__ __launch_bounds__(256) void bn_sums_from_consumer_kernel(
    int C, int cout, int cin, int col0, const float* __restrict__ W, const float* __restrict__ dW,
    const float* __restrict__ db, const float* __restrict__ gamma, const float* __restrict__ beta,
    float* __restrict__ dgamma, float* __restrict__ dbeta, int* __restrict__ ok, int rep_k, int rep_stride,
    const float* __restrict__ h, int h_stride, const float* __restrict__ dyv, int dy_stride, long R,
    const float* __restrict__ mean, const float* __restrict__ invstd, int rows_bf16) {
    // one workgroup per channel o of the BatchNorm; its threads share the (consumer row j, gradient image r) pairs
    __shared__ int s_ok;
    __shared__ double s_red[2][4];
    const int o = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_ok = 1;
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256)
        if (!bn_identity_ok(gamma[c], beta[c])) s_ok = 0;
    __syncthreads();
    if (o == 0 && threadIdx.x == 0) *ok = s_ok;
    if (!s_ok) {
        const float mu = mean[o], is = invstd[o];
        double sb = 0.0, sg = 0.0;
        for (long r = threadIdx.x; r < R; r += 256) {
            float dd, hh;
            if (rows_bf16) {
                dd = __uint_as_float((unsigned)reinterpret_cast<const unsigned short*>(dyv)[(size_t)r * dy_stride + o] << 16);
                hh = __uint_as_float((unsigned)reinterpret_cast<const unsigned short*>(h)[(size_t)r * h_stride + o] << 16);
            } else {
                dd = dyv[(size_t)r * dy_stride + o], hh = h[(size_t)r * h_stride + o];
            }
            sb += (double)dd;
            sg += (double)(dd * ((hh - mu) * is));
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            sb += __shfl_xor(sb, m);
            sg += __shfl_xor(sg, m);
        }
        if (lane == 0) s_red[0][wave] = sb, s_red[1][wave] = sg;
        __syncthreads();
        if (threadIdx.x == 0) {
            dbeta[o] += (float)((s_red[0][0] + s_red[0][1]) + (s_red[0][2] + s_red[0][3]));
            dgamma[o] += (float)((s_red[1][0] + s_red[1][1]) + (s_red[1][2] + s_red[1][3]));
        }
        return;
    }
    const int images = rep_k > 1 ? rep_k : 1;                   // the consumer's (dW, db) images are summed on the fly
    const double g = (double)gamma[o], b = (double)beta[o];
    double sb = 0.0, sg = 0.0;
    for (int idx = threadIdx.x; idx < cout * images; idx += 256) {
        const int r = idx / cout, j = idx - r * cout;
        const double w = (double)W[j * cin + col0 + o];
        const double dbj = (double)db[(size_t)r * rep_stride + j];
        const double dwj = (double)dW[(size_t)r * rep_stride + j * cin + col0 + o];
        sb += w * dbj;
        sg += w * (dwj - b * dbj);
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        sb += __shfl_xor(sb, m);
        sg += __shfl_xor(sg, m);
    }
    if (lane == 0) s_red[0][wave] = sb, s_red[1][wave] = sg;
    __syncthreads();
    if (threadIdx.x == 0) {
        sb = (s_red[0][0] + s_red[0][1]) + (s_red[0][2] + s_red[0][3]);
        sg = (s_red[1][0] + s_red[1][1]) + (s_red[1][2] + s_red[1][3]);
        dbeta[o] += (float)sb;
        dgamma[o] += (float)(sg / g);
    }
}

int check_head(const sn2_head* p) {
    if (!p || p->R <= 0 || p->cin != 34 || p->f_stride != 36) return p && p->R > 0 ? SN2_ELIMIT : SN2_EINVAL;
    if (!p->f || !p->fa || !p->fc || !p->W1 || !p->b1 || !p->W2 || !p->b2) return SN2_EINVAL;
    return 0;
}

}  // namespace

extern "C" int sn2_head_forward(const sn2_head* p, void* stream) {
    SN2_TRY(check_head(p));
    if (!p->coverages || !p->proba) return SN2_EINVAL;
    if (p->zero_fill && ((p->zero_fill_words & 3) || p->zero_fill_words <= 0 || ((uintptr_t)p->zero_fill & 15))) return SN2_EINVAL;
    // check_head: rows of exactly 36 floats (34 channels)
    auto kf = p->act_bf16 ? &head_fwd_mfma_kernel<true> : &head_fwd_mfma_kernel<false>;
    // no more workgroups than are resident together (SN2_HF_OCC per CU; each wave loops over its turns): with 1024 workgroups at
    // three per CU a quarter of them ran as a second round at a third of the occupancy (round 5)
    int hf_grid = pick_grid(p->R, 256, 2);
    if (hf_grid > SN2_HF_OCC * sn2_cu_count()) hf_grid = SN2_HF_OCC * sn2_cu_count();
    hipLaunchKernelGGL(kf, dim3(hf_grid), dim3(256), 0, (hipStream_t)stream, p->R, p->f, p->fa,
                       p->fc, p->W1, p->b1, p->W2, p->b2, p->coverages, p->proba, p->drop_mask,
                       p->drop_mask ? p->drop_scale : 1.f, reinterpret_cast<float4*>(p->zero_fill),
                       p->zero_fill ? p->zero_fill_words / 4 : 0L);
    SN2_RETURN_LAUNCH();
}

// the launches of sn2_fp_head_eval, over the layer's skip width (checked by the caller)
template <int CB>
static int fp_head_eval_t(const sn2_fp* p, const sn2_head* hd, hipStream_t st) {
    const int R = hd->R, n_src = p->B * p->S_per_plot;
    // the layer's BatchNorm on its running statistics -> (a, c) = what the head applies to the rows (hd->fa, hd->fc name the
    // same two vectors: p->blk.a, p->blk.c)
    SN2_TRY(sn2_bn_finalize(&p->blk, 0, nullptr, R, 0, st));
    SN2_TRY((launch_src_table<34, CB, 34>(n_src, p->src_stride, p->src, p->src_a, p->src_c, p->blk.W, p->src_ws, st)));
    const long turns = ((long)R + 62) / 63;
    int grid = sn2_cdiv(turns, 4);
    if (g_fp_rows_form != 0 && grid >= 2 * sn2_cu_count()) {
        // (round 5) the pipelined form: as many workgroups as are resident together (two per CU by its registers), each wave
        // several turns with the next turn's inputs in flight
        grid = 2 * sn2_cu_count();
        hipLaunchKernelGGL((fp_head_eval2_kernel<34, CB, 34>), dim3(grid), dim3(256), 0, st, R, p->R_per_plot, p->S_per_plot,
                           p->skip_stride, (const float*)p->src_ws, p->knn_idx, p->knn_w, p->skip, p->blk.W, p->blk.b, hd->fa, hd->fc,
                           hd->W1, hd->b1, hd->W2, hd->b2, hd->coverages, hd->proba);
        SN2_RETURN_LAUNCH();
    }
    const int cap = 4 * sn2_cu_count();
    if (grid > cap) grid = cap;
    hipLaunchKernelGGL((fp_head_eval_kernel<34, CB, 34>), dim3(grid), dim3(256), 0, st, R, p->R_per_plot, p->S_per_plot,
                       p->skip_stride, (const float*)p->src_ws, p->knn_idx, p->knn_w, p->skip, p->blk.W, p->blk.b, hd->fa, hd->fc,
                       hd->W1, hd->b1, hd->W2, hd->b2, hd->coverages, hd->proba);
    SN2_RETURN_LAUNCH();
}

extern "C" int sn2_fp_head_eval(const sn2_fp* p, const sn2_head* hd, void* stream) {
    // (neither p->h nor hd->f is read: the rows stay in LDS)
    if (!p || !hd || p->B <= 0 || p->R_per_plot <= 0 || p->S_per_plot <= 0 || !p->src || !p->blk.W || !p->blk.b || !p->skip ||
        !p->blk.a || !p->blk.c || (p->src_stride & 3) || p->src_stride < p->ca || p->blk.cin != p->ca + p->cb)
        return SN2_EINVAL;
    if (hd->R <= 0 || hd->cin != 34 || !hd->fa || !hd->fc || !hd->W1 || !hd->b1 || !hd->W2 || !hd->b2) return SN2_EINVAL;
    if (!hd->coverages || !hd->proba || hd->drop_mask || hd->act_bf16 || p->act_bf16) return SN2_EINVAL;
    if (!(p->knn_idx && p->ca == 34 && (p->cb == 8 || p->cb == 4) && p->blk.cout == 34 && hd->R == p->B * p->R_per_plot)) return SN2_ELIMIT;
    if (!fp_source_side_ok<34, 34>(p, /*with_h=*/false)) return SN2_ELIMIT;       // (hd->R == B * R_per_plot: the line above)
    // (eight point features, or four: one skip quad per row)
    return p->cb == 4 ? fp_head_eval_t<4>(p, hd, (hipStream_t)stream) : fp_head_eval_t<8>(p, hd, (hipStream_t)stream);
}

extern "C" int sn2_head_bn_sums(const sn2_head* p, const float* gamma, const float* beta, const float* mean,
                                const float* invstd, float* dgamma, float* dbeta, int* ok, void* stream) {
    SN2_TRY(check_head(p));
    if (!p->dW1 || !p->db1 || !p->dy || !gamma || !beta || !mean || !invstd || !dgamma || !dbeta || !ok) return SN2_EINVAL;
    hipLaunchKernelGGL(bn_sums_from_consumer_kernel, dim3(p->cin), dim3(256), 0, (hipStream_t)stream, p->cin, 16, p->cin, 0, p->W1,
                       (const float*)p->dW1, (const float*)p->db1, gamma, beta, dgamma, dbeta, ok, p->grad_replicas,
                       p->grad_replica_stride, p->f, p->f_stride, (const float*)p->dy, p->f_stride, (long)p->R, mean, invstd,
                       p->act_bf16);
    SN2_RETURN_LAUNCH();
}

extern "C" int sn2_fp_bn_sums(const sn2_fp* p, const float* gamma, const float* beta, const float* mean, const float* invstd,
                              float* dgamma, float* dbeta, int* ok, void* stream) {
    SN2_TRY(check_fp(p));
    if (!p->knn_idx || !p->blk.dW || !p->blk.db || !p->dsrc || !gamma || !beta || !mean || !invstd || !dgamma || !dbeta || !ok ||
        p->ca > 64)
        return SN2_EINVAL;
    hipLaunchKernelGGL(bn_sums_from_consumer_kernel, dim3(p->ca), dim3(256), 0, (hipStream_t)stream, p->ca, p->blk.cout, p->blk.cin, 0,
                       (const float*)p->blk.W, (const float*)p->blk.dW, (const float*)p->blk.db, gamma, beta, dgamma, dbeta, ok,
                       p->blk.grad_replicas, p->blk.grad_replica_stride, p->src, p->src_stride, (const float*)p->dsrc,
                       p->dsrc_stride, (long)p->B * p->S_per_plot, mean, invstd, 0);
    SN2_RETURN_LAUNCH();
}

// 79 136 bytes, and with a descriptor 2 064 more (the per-plot table and two coefficients).  Two workgroups per CU either way,
// ASSUMING the hardware hands LDS out in blocks of at most 512 bytes: 81 200 rounds up to 81 408, twice that is 162 816 of
// 163 840.  A coarser granularity (1 KB would still do: 81 920 x 2 = 163 840, no slack at all) or one more kilobyte of LDS ends
// that: sn2_debug_head_backward_occupancy asks the runtime, and tests/test_gpu_head_loss_backward.py holds it to 2.
constexpr size_t HB_LDS_TAB = ((size_t)HB_WAVE_FLOATS * 4 + HB_TAB_FLOATS) * 4, HB_LDS_LOSS = PL_HEAD_MAX_PLOTS * 16 + 16;
constexpr size_t hb_lds_round(size_t b) { return (b + 511) / 512 * 512; }
static_assert(2 * hb_lds_round(HB_LDS_TAB + HB_LDS_LOSS) <= 160 * 1024, "head backward: two workgroups per CU");

extern "C" int sn2_debug_head_backward_occupancy(int bf16, int with_loss) {
    auto km = bf16 ? &head_bwd_mfma_kernel<true> : &head_bwd_mfma_kernel<false>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(km), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(HB_LDS_TAB + HB_LDS_LOSS));
    int n = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, km, 256, HB_LDS_TAB + (with_loss ? HB_LDS_LOSS : 0));
    return e == hipSuccess ? n : -(int)e;
}

extern "C" int sn2_head_backward(const sn2_head* p, void* stream) {
    SN2_TRY(check_head(p));
    if (!p->dy || !p->dW1 || !p->db1 || !p->dW2 || !p->db2) return SN2_EINVAL;
    sn2_loss_grad lg = {};
    if (p->loss) {
        lg = *p->loss;
        if (p->dcoverages || p->dproba || !sn2_head_loss_route(lg.B, lg.N, lg.D) || (long)lg.B * lg.N != (long)p->R) return SN2_EINVAL;
        if (!lg.pred || !lg.gt || !lg.proba || !lg.grad_total || !lg.arg || !lg.nocc || !lg.pix || (lg.m != 0.0 && !lg.pdf)) return SN2_EINVAL;
        if (lg.m == 0.0) lg.pdf = nullptr;
    }
    const size_t lds_m = HB_LDS_TAB + (p->loss ? HB_LDS_LOSS : 0);
    auto km = p->act_bf16 ? &head_bwd_mfma_kernel<true> : &head_bwd_mfma_kernel<false>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(km), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(HB_LDS_TAB + HB_LDS_LOSS));
    int gm = sn2_cdiv(sn2_cdiv(p->R, 64), 4);
    const int cap = 2 * sn2_cu_count();
    if (gm > cap) gm = cap;
    hipLaunchKernelGGL(km, dim3(gm), dim3(256), lds_m, (hipStream_t)stream, p->R, p->f, p->fa, p->fc, p->W1, p->b1, p->W2,
                       p->b2, p->dcoverages, p->dproba, p->dy, p->dW1, p->db1, p->dW2, p->db2, p->grad_replicas,
                       p->grad_replica_stride, p->drop_mask, p->drop_mask ? p->drop_scale : 1.f, lg);
    SN2_RETURN_LAUNCH();
}

extern "C" int sn2_head_loss_route(int B, int N, int D) {
    return B > 0 && N > 0 && D > 0 && B <= PL_HEAD_MAX_PLOTS && D <= 45 && D * D <= PL_MAX_CELLS && (long)B * N < (1L << 31);
}
