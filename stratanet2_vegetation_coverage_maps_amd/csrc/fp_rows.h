// fp_rows.h -- what the dense-row units share (fp.hip, head.hip, global_level.hip, global_level_bwd.hip, interp_index.hip): the accessors of a row of
// per-point activations in either storage precision, the spelled-out interpolation arithmetic, the input stream and the
// (row, quad) arithmetic of the source-side row passes (fp_table_rows, fp_row_quad), the two source-table kernels with their launcher, the staging of a 64-row block's inputs, the host
// view of the inverted interpolation index, and the small host helpers of the dispatch code.  Templates are instantiated
// where they are used.
#pragma once
#include "mlp.h"

// which row pass the source-side forward launches: 1 (default) fp_fwd_rows2_kernel / fp_head_eval2_kernel, 0 fp_fwd_rows_kernel /
// fp_head_eval_kernel (same bits; test hook: sn2_debug_fp_rows_form).  Defined in fp.hip.
extern int g_fp_rows_form;
// which kernel builds the source table: 1 (default) fp_src_table_mfma_kernel, 0 fp_src_table_kernel (test hook:
// sn2_debug_fp_table_form).  Defined in fp.hip.
extern int g_fp_table_form;

// the inverted index of a 3-NN table (interp_index.hip): G batches of B plots each in one set of launches (G = 1: one batch);
// batch h's workspace at ws + h * ws_stride words.  row_order (G*B*Rp, per plot a permutation of 0..Rp-1) or nullptr: the order
// the rows are walked in; idx_sorted / w_sorted (with row_order, both or neither): the table's rows in that order
int build_interp_index(const int* knn_idx, const float* knn_w, const float* src_pos, int B, int Rp, int S, float* ws,
                       hipStream_t st, const int* row_perm = nullptr, int G = 1, size_t ws_stride = 0, const int* row_order = nullptr,
                       const int* idx_sorted = nullptr, const float* w_sorted = nullptr);

namespace {

// ---- rows of per-point activations in either storage precision (sn2_fp.act_bf16 / sn2_head.act_bf16).  A row has `stride`
// ELEMENTS either way; quad q = elements 4q .. 4q+3: one 16-byte (fp32) or one 8-byte (bfloat16) access.  bfloat16 rows are
// written with v_cvt_pk_bf16_f32 (round to nearest even) and read back exactly (a bfloat16 IS the upper half of an fp32).
template <bool BF>
__device__ __forceinline__ float4 row_quad_ld(const float* __restrict__ base, size_t row, int stride, int q) {
    if constexpr (BF) {
        const uint2 u = reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(base) + row * stride)[q];
        return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xFFFF0000u), __uint_as_float(u.y << 16),
                           __uint_as_float(u.y & 0xFFFF0000u));
    } else {
        return reinterpret_cast<const float4*>(base + row * stride)[q];
    }
}
__device__ __forceinline__ uint2 pack_bf16x4(float a, float b, float c, float d) {
    bf16x4 v;
    v[0] = (__bf16)a; v[1] = (__bf16)b; v[2] = (__bf16)c; v[3] = (__bf16)d;
    return __builtin_bit_cast(uint2, v);
}
template <bool BF>
__device__ __forceinline__ void row_quad_st(float* __restrict__ base, size_t row, int stride, int q, float a, float b, float c, float d) {
    if constexpr (BF) reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(base) + row * stride)[q] = pack_bf16x4(a, b, c, d);
    else reinterpret_cast<float4*>(base + row * stride)[q] = make_float4(a, b, c, d);
}
// the value a bfloat16 store keeps (for sums that must describe the STORED rows)
__device__ __forceinline__ float bf16_round(float x) { return (float)(__bf16)x; }

template <int CA, int CB, int CO>
__global__ __launch_bounds__(256) void fp_src_table_kernel(int n_src, int src_stride, const float* __restrict__ src,
                                                           const float* __restrict__ src_a, const float* __restrict__ src_c,
                                                           const float* __restrict__ Wg, float* __restrict__ T) {
    // 64 source rows per workgroup, wave g = output channels [g*QH, (g+1)*QH): 4x the waves, 4x shorter FMA chains
    constexpr int CI = CA + CB, QH = (CO + 3) / 4, HS = 4 * QH;
    const int s = blockIdx.x * 64 + (threadIdx.x & 63), grp = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t ss = s < n_src ? (size_t)s : 0;
    const cfp W = opaque(as_const(Wg));
    float x[CA];
    const float4* sr = reinterpret_cast<const float4*>(src + ss * src_stride);
#pragma unroll
    for (int q4 = 0; q4 < (CA + 3) / 4; ++q4) {
        const float4 a = sr[q4];
        const float v[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (4 * q4 + t < CA) x[4 * q4 + t] = v[t];
    }
    if (src_a) {
        const cfp sa = opaque(as_const(src_a)), sc = opaque(as_const(src_c));
#pragma unroll
        for (int k = 0; k < CA; ++k) x[k] = fmaf(sa[k], x[k], sc[k]);
    }
    float* out = T + ss * HS + grp * QH;
#pragma unroll
    for (int j = 0; j < QH; ++j) {
        const int o = grp * QH + j;                     // wave-uniform
        float acc = 0.f;
        if (o < CO) {
#pragma unroll
            for (int k = 0; k < CA; ++k) acc = fmaf(W[o * CI + k], x[k], acc);
        }
        if (s < n_src) out[j] = acc;
    }
}

// a wave re-reads LDS words other lanes of the SAME wave wrote: the LDS executes a wave's instructions in order, the compiler
// must not move the accesses across this point
#define WAVE_LDS_SYNC() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
// The same table on the matrix cores (round 5): a wave takes 64 consecutive source rows -- fetched with coalesced float4 loads into
// an LDS tile, the BatchNorm affine of the layer in front applied on the way out of it --, contracts them with W_A held in
// registers (`v_mfma_f32_16x16x4_f32`, k ascending: the exact fp32 products and the accumulation order of the scalar kernel's
// fmaf chain), and writes the 64 table rows back through the tile as coalesced float4.  fp_src_table_kernel gives every lane a
// row and takes its weights through scalar loads, ~1200 FMA instructions per row-lane behind 144-byte strided loads: 243 us for
// the parcel loop's 1.28 M sources (1.5 TB/s); this form streams.
template <int CA, int CB, int CO>
__global__ __launch_bounds__(256) void fp_src_table_mfma_kernel(int n_src, int src_stride, const float* __restrict__ src,
                                                                const float* __restrict__ src_a, const float* __restrict__ src_c,
                                                                const float* __restrict__ Wg, float* __restrict__ T) {
    constexpr int CI = CA + CB, QH = (CO + 3) / 4, HS = 4 * QH, KS = (CA + 3) / 4, TJ = (HS + 15) / 16;
    // tile row stride: the source row, padded so that the sixteen rows of an A-operand read sit in different banks
    constexpr int LS = (4 * KS) % 32 == 0 ? 4 * KS + 4 : 4 * KS;
    static_assert(HS <= LS, "the table rows go back through the tile");
    extern __shared__ __attribute__((aligned(16))) float s_tile[];            // [4 waves][64][LS]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* st = s_tile + (size_t)wave * 64 * LS;
    const int n = lane & 15, kq = lane >> 4;
    float wb[TJ][KS], ak[KS], ck[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int k = 4 * ks + kq;
        ak[ks] = k < CA ? (src_a ? src_a[k] : 1.f) : 0.f;
        ck[ks] = (k < CA && src_a) ? src_c[k] : 0.f;
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
            const int o = 16 * j + n;
            wb[j][ks] = (o < CO && k < CA) ? Wg[o * CI + k] : 0.f;
        }
    }
    const long n_turns = ((long)n_src + 63) / 64;
    for (long turn = (long)blockIdx.x * 4 + wave; turn < n_turns; turn += (long)gridDim.x * 4) {
        const long s0 = turn * 64;
        // ---- 64 rows x KS quads, coalesced; rows past the end: the last row (never written back)
        const int rows_here = n_src - s0 < 64 ? (int)(n_src - s0) : 64;
        const float* base = src + (size_t)s0 * src_stride;
        const int QR = src_stride / 4;                                      // quads of a source row in memory
#pragma unroll
        for (int i = 0; i < KS; ++i) {
            const int e = lane + 64 * i;                                     // quad e of the 64 x KS quads this wave wants
            const int r = e / KS, qk = e - r * KS;
            const int rc = r < rows_here ? r : rows_here - 1;
            const float4 v = reinterpret_cast<const float4*>(base + (size_t)rc * src_stride)[qk < QR ? qk : QR - 1];
            *reinterpret_cast<float4*>(&st[r * LS + 4 * qk]) = v;
        }
        WAVE_LDS_SYNC();
        f32x4 acc[4][TJ];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int j = 0; j < TJ; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const float x = st[(16 * t + n) * LS + 4 * ks + kq];
                const float a = (4 * ks + kq < CA) ? (src_a ? fmaf(ak[ks], x, ck[ks]) : x) : 0.f;
#pragma unroll
                for (int j = 0; j < TJ; ++j) acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[j][ks], a, acc[t][j], 0, 0, 0);
            }
        WAVE_LDS_SYNC();
        // acc[t][j][r]: output channel 16 j + 4 kq + r of source row 16 t + n  (A = weights: rows of D are channels)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int j = 0; j < TJ; ++j) {
                const int o = 16 * j + 4 * kq;
                if (o < HS) *reinterpret_cast<float4*>(&st[(16 * t + n) * LS + o]) = make_float4(acc[t][j][0], acc[t][j][1], acc[t][j][2], acc[t][j][3]);
            }
        WAVE_LDS_SYNC();
        float* out = T + (size_t)s0 * HS;
#pragma unroll
        for (int i = 0; i < QH; ++i) {
            const int e = lane + 64 * i;
            const int r = e / QH, qo = e - r * QH;
            if (r < rows_here) reinterpret_cast<float4*>(out + (size_t)r * HS)[qo] = *reinterpret_cast<const float4*>(&st[r * LS + 4 * qo]);
        }
        WAVE_LDS_SYNC();
    }
}
template <int CA, int CB, int CO>
int launch_src_table(int n_src, int src_stride, const float* src, const float* src_a, const float* src_c, const float* W, float* T,
                     hipStream_t st) {
    // where it pays: many sources of the 34-channel layer (the parcel loop's 1.28 M: 243 -> 122 us).  Not the 64-channel layer
    // (68-word tile rows, two workgroups per CU: 85 -> 99 us) and not a training batch's 16 384 sources (64 workgroups, each one
    // long chain: 6.9 -> 9.1 us).  Both kernels give the same bits (tests), so the choice is free.
    if (g_fp_table_form != 0 && CA <= 36 && n_src >= 65536 && src_stride >= 4 * ((CA + 3) / 4)) {
        constexpr int KS = (CA + 3) / 4, LS = (4 * KS) % 32 == 0 ? 4 * KS + 4 : 4 * KS;
        const size_t lds = (size_t)4 * 64 * LS * sizeof(float);
        auto k = &fp_src_table_mfma_kernel<CA, CB, CO>;
        if (lds > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        long grid = ((long)n_src + 255) / 256;
        const long cap = 4L * sn2_cu_count();
        if (grid > cap) grid = cap;
        hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(256), lds, st, n_src, src_stride, src, src_a, src_c, W, T);
    } else {
        hipLaunchKernelGGL((fp_src_table_kernel<CA, CB, CO>), dim3(sn2_cdiv(n_src, 64)), dim3(256), 0, st, n_src, src_stride, src, src_a,
                           src_c, W, T);
    }
    SN2_RETURN_LAUNCH();
}

// The interpolated part of a pre-activation, in ONE spelled-out order of operations -- fma(fma(fma(c, w2, fma(b, w1, a w0)) ...:
//   s = a w0;  s = fma(b, w1, s);  s = fma(c, w2, s);  acc = fma(s, 1 / sum w, bias)
// Left to the compiler's contraction, the two row passes of fp.hip (same source text) fused different products and differed in the
// last bit of every fourth column.  fp_fwd_rows2_kernel issues the same operations two channels at a time (v_pk_mul_f32 /
// v_pk_fma_f32: IEEE per component, the same bits).
__device__ __forceinline__ float interp_bias(float a, float b, float c, float w0, float w1, float w2, float inv, float bias) {
    float s2;
    {
#pragma clang fp contract(off)
        s2 = a * w0;
    }
    s2 = fmaf(b, w1, s2);
    s2 = fmaf(c, w2, s2);
    return fmaf(s2, inv, bias);
}
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 interp_bias2(f32x2 a, f32x2 b, f32x2 c, float w0, float w1, float w2, float inv, f32x2 bias) {
    f32x2 s2;
    {
#pragma clang fp contract(off)
        s2 = a * (f32x2){w0, w0};
    }
    s2 = __builtin_elementwise_fma(b, (f32x2){w1, w1}, s2);
    s2 = __builtin_elementwise_fma(c, (f32x2){w2, w2}, s2);
    return __builtin_elementwise_fma(s2, (f32x2){inv, inv}, bias);
}
// Which iterations (FP_ROWS_PER_IT consecutive rows each) a wave of the row kernels works on: it0, it0 + stride, ... < it_hi.
// Workgroups go to the XCDs round-robin (blockIdx % 8), and the iterations are dealt the same way when they go wave after wave --
// every XCD's L2 then holds the table rows of ALL plots (2.4 MB of a 4 MB L2 at config 2) beside the rows streaming through it.
// With the grid a multiple of 8, XCD x takes the x-th EIGHTH of the rows instead (whole plots where the batch is a multiple of
// eight plots): its L2 holds an eighth of the table.
struct RowIters {
    int it0, stride, it_hi;
};
__device__ __forceinline__ RowIters row_iters(int n_it, int wave, int wpw = 4) {           // wpw: waves per workgroup
    RowIters r;
    if ((gridDim.x & 7) == 0) {
        const int xcd = blockIdx.x & 7, wg_x = blockIdx.x >> 3, n_wg_x = gridDim.x >> 3;
        const int lo = (int)((long)n_it * xcd / 8);
        r.it_hi = (int)((long)n_it * (xcd + 1) / 8);
        r.stride = n_wg_x * wpw;
        r.it0 = lo + wg_x * wpw + wave;
    } else {
        r.it_hi = n_it, r.stride = (int)gridDim.x * wpw, r.it0 = (int)blockIdx.x * wpw + wave;
    }
    return r;
}
// what a (row, quad) lane of the row kernels reads ahead of its gathers: the row's 3-NN entry and skip columns
template <int QB>
struct FpRowIn {
    unsigned rr;
    bool valid;
    int i0, i1, i2;
    float w0, w1, w2;
    float4 sk[QB];
};
template <int QB>
__device__ __forceinline__ FpRowIn<QB> fp_row_in(long row, bool on, int R, const int* __restrict__ knn_idx,
                                                 const float* __restrict__ knn_w, const float* __restrict__ skip,
                                                 int skip_stride) {
    FpRowIn<QB> in;
    in.valid = on && row < R;
    in.rr = in.valid ? (unsigned)row : 0u;
    in.i0 = knn_idx[in.rr * 3 + 0], in.i1 = knn_idx[in.rr * 3 + 1], in.i2 = knn_idx[in.rr * 3 + 2];
    in.w0 = knn_w[in.rr * 3 + 0], in.w1 = knn_w[in.rr * 3 + 1], in.w2 = knn_w[in.rr * 3 + 2];
#pragma unroll
    for (int b = 0; b < QB; ++b) in.sk[b] = reinterpret_cast<const float4*>(skip + (size_t)in.rr * skip_stride)[b];
    return in;
}
// quad q of the three table rows a row interpolates (rows of HS floats; base = the first source row of the row's plot)
// (SN2_FR_DIAG: timing builds of the row passes, scripts/time_fp1.py -- 1 no stores, 2 no table gathers, 4 no skip contraction)
template <int HS>
__device__ __forceinline__ void fp_table_rows(const float* __restrict__ T, unsigned base, int i0, int i1, int i2, int q, float4 (&ta)[3]) {
#if defined(SN2_FR_DIAG) && (SN2_FR_DIAG & 2)
    ta[0] = make_float4((float)(base + i0), 1.f, 2.f, 3.f);      // (diagnostic: values made from the indices)
    ta[1] = make_float4((float)i1, 1.f, 2.f, 3.f);
    ta[2] = make_float4((float)i2, 1.f, 2.f, 3.f);
#else
    ta[0] = reinterpret_cast<const float4*>(T + (size_t)(base + i0) * HS)[q];
    ta[1] = reinterpret_cast<const float4*>(T + (size_t)(base + i1) * HS)[q];
    ta[2] = reinterpret_cast<const float4*>(T + (size_t)(base + i2) * HS)[q];
#endif
}
// The row side of the source-side form for one (row, quad) lane, stated once for fp_fwd_rows_kernel and the two eval kernels of
// head.hip (same operations in the same order: the same bits): the lane's skip weights W_B and bias, output channels 4 q .. 4 q + 3
// (zero past CO), in registers for the whole kernel --
template <int CB>
struct FpQuadW {
    float wB[4][CB], b4[4];
};
template <int CA, int CB, int CO>
__device__ __forceinline__ FpQuadW<CB> fp_quad_w(const float* __restrict__ Wg, const float* __restrict__ biasg, int q) {
    FpQuadW<CB> w;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int o = 4 * q + t;
        w.b4[t] = o < CO ? biasg[o] : 0.f;
#pragma unroll
        for (int k = 0; k < CB; ++k) w.wB[t][k] = o < CO ? Wg[o * (CA + CB) + CA + k] : 0.f;
    }
    return w;
}
// -- and the quad itself: v = relu(interp_bias(table rows, 3-NN weights) + W_B skip), zero where the row is not valid or the
// channel lies past CO
template <int CB, int CO>
__device__ __forceinline__ void fp_row_quad(const FpQuadW<CB>& w, const float4 (&ta)[3], float w0, float w1, float w2,
                                            const float4 (&sk)[CB / 4], bool valid, int q, float (&v)[4]) {
    const float inv = 1.0f / ((w0 + w1) + w2);
    const float4 a = ta[0], b = ta[1], c = ta[2];
    v[0] = interp_bias(a.x, b.x, c.x, w0, w1, w2, inv, w.b4[0]), v[1] = interp_bias(a.y, b.y, c.y, w0, w1, w2, inv, w.b4[1]);
    v[2] = interp_bias(a.z, b.z, c.z, w0, w1, w2, inv, w.b4[2]), v[3] = interp_bias(a.w, b.w, c.w, w0, w1, w2, inv, w.b4[3]);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float acc = v[t];
#if defined(SN2_FR_DIAG) && (SN2_FR_DIAG & 4)
        acc += sk[0].x + sk[CB / 4 - 1].w;          // (diagnostic: no skip contraction)
#else
#pragma unroll
        for (int b2 = 0; b2 < CB / 4; ++b2) {
            acc = fmaf(w.wB[t][4 * b2 + 0], sk[b2].x, acc);
            acc = fmaf(w.wB[t][4 * b2 + 1], sk[b2].y, acc);
            acc = fmaf(w.wB[t][4 * b2 + 2], sk[b2].z, acc);
            acc = fmaf(w.wB[t][4 * b2 + 3], sk[b2].w, acc);
        }
#endif
        v[t] = (valid && 4 * q + t < CO) ? fmaxf(acc, 0.f) : 0.f;
    }
}

// The four waves of a 64-row workgroup build the rows' inputs [u | 1] together in LDS, s_q[64][QS]; wave g builds the rows
// 16 g .. 16 g + 15.  A row's interpolated part is CA / 4 float4 quads: that many consecutive lanes share a row, so one load
// instruction covers 64 / (CA / 4) whole source rows -- with one row per lane every instruction touched 64 different cache
// lines and the four waves queued behind the CU's one address unit (17 000 clocks of a 46 000-clock kernel).  The same
// arithmetic, element by element, as build_input (fp.hip).  Columns past CA + CB are left alone.
template <int CA, int CB, bool KNN>
__device__ __forceinline__ void stage_inputs(float* __restrict__ s_q, int QS, int g, int lane, long r0, int R, int R_per_plot,
                                             int S_per_plot, const float* __restrict__ src, int src_stride,
                                             const float* __restrict__ src_a, const float* __restrict__ src_c,
                                             const int* __restrict__ knn_idx, const float* __restrict__ knn_w,
                                             const float* __restrict__ skip, int skip_stride) {
    constexpr int CI = CA + CB, QA = (CA + 3) / 4;
    constexpr int LPR = QA <= 8 ? 8 : (QA <= 16 ? 16 : (QA <= 32 ? 32 : 64));     // lanes per row (a power of two >= QA)
    static_assert(QA <= 64, "at most 256 interpolated channels");
    constexpr int RPI = 64 / LPR;                     // rows per load instruction
    const int q = lane & (LPR - 1);
    const bool qon = q < QA;
    const int qc = qon ? q : 0;
    // the skip columns of the few-channel form (CB no multiple of four: the positions of the global SA block) are asked for HERE,
    // together with the rows of the interpolated part: behind them they were a memory round trip of their own
    constexpr bool SKIP_SCALAR = CB > 0 && !(CB % 4 == 0 && ((CB / 4) & (CB / 4 - 1)) == 0 && CB <= 64);
    float skr[SKIP_SCALAR ? CB : 1];
    if constexpr (SKIP_SCALAR) {
        const long r = r0 + 16 * g + (lane & 15);
        const size_t rr = r < R ? (size_t)r : (size_t)(R - 1);
#pragma unroll
        for (int k = 0; k < CB; ++k) skr[k] = skip[rr * skip_stride + k];
    }
    float a4[4] = {1.f, 1.f, 1.f, 1.f}, c4[4] = {0.f, 0.f, 0.f, 0.f};
    if (src_a) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (4 * qc + t < CA) a4[t] = src_a[4 * qc + t], c4[t] = src_c[4 * qc + t];
    }
#pragma unroll
    for (int st = 0; st < 16 / RPI; ++st) {
        const int row = 16 * g + st * RPI + lane / LPR;
        const long r = r0 + row;
        const size_t rr = r < R ? (size_t)r : (size_t)(R - 1);
        float v[4];
        if constexpr (KNN) {
            const size_t base = (rr / R_per_plot) * S_per_plot;
            const int i0 = knn_idx[rr * 3 + 0], i1 = knn_idx[rr * 3 + 1], i2 = knn_idx[rr * 3 + 2];
            const float w0 = knn_w[rr * 3 + 0], w1 = knn_w[rr * 3 + 1], w2 = knn_w[rr * 3 + 2];
            const float inv = 1.0f / ((w0 + w1) + w2);
            const float4 a = reinterpret_cast<const float4*>(src + (base + i0) * src_stride)[qc];
            const float4 b = reinterpret_cast<const float4*>(src + (base + i1) * src_stride)[qc];
            const float4 c = reinterpret_cast<const float4*>(src + (base + i2) * src_stride)[qc];
            v[0] = ((a.x * w0 + b.x * w1) + c.x * w2) * inv, v[1] = ((a.y * w0 + b.y * w1) + c.y * w2) * inv;
            v[2] = ((a.z * w0 + b.z * w1) + c.z * w2) * inv, v[3] = ((a.w * w0 + b.w * w1) + c.w * w2) * inv;
        } else {
            const float4 a = reinterpret_cast<const float4*>(src + rr * src_stride)[qc];
            v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
        }
        if (src_a) {
#pragma unroll
            for (int t = 0; t < 4; ++t) v[t] = fmaf(a4[t], v[t], c4[t]);
        }
        if (qon) {
            if (CA % 4 == 0 || q < QA - 1) {
                *reinterpret_cast<float4*>(&s_q[row * QS + 4 * q]) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (4 * q + t < CA) s_q[row * QS + 4 * q + t] = v[t];
            }
        }
    }
    if constexpr (CB > 0 && CB % 4 == 0 && ((CB / 4) & (CB / 4 - 1)) == 0 && CB <= 64) {
        constexpr int QB = CB / 4, RPB = 64 / QB;     // the skip part the same way
#pragma unroll
        for (int st = 0; st < (16 + RPB - 1) / RPB; ++st) {
            const int rl = st * RPB + lane / QB;      // 0..15 within the wave's rows
            const int row = 16 * g + rl;
            const long r = r0 + row;
            const size_t rr = r < R ? (size_t)r : (size_t)(R - 1);
            if (rl < 16) {
                const float4 a = reinterpret_cast<const float4*>(skip + rr * skip_stride)[lane & (QB - 1)];
                float* d = &s_q[row * QS + CA + 4 * (lane & (QB - 1))];
                d[0] = a.x, d[1] = a.y, d[2] = a.z, d[3] = a.w;
            }
        }
    } else if constexpr (CB > 0) {
        if (lane < 16) {
            const int row = 16 * g + lane;
#pragma unroll
            for (int k = 0; k < CB; ++k) s_q[row * QS + CA + k] = skr[k];
        }
    }
    if (lane < 16) s_q[(16 * g + lane) * QS + CI] = 1.0f;       // the bias column
}

// ---- the inverted interpolation index (built by interp_index.hip, read by the backward kernels of fp.hip)
// rows of a slice of the histogram and fill passes; entries of a chunk of a source's list; chunk slots of a plot
constexpr int INV_SLICE_ROWS = 2048;
constexpr int INV_CHUNK = 63;
__host__ __device__ constexpr int inv_chunks_per_plot(int Rp, int S) { return (3 * Rp + INV_CHUNK - 1) / INV_CHUNK + S; }
// the inverted index of a 3-NN table (kernels A-C, E of interp_index.hip); workspace carve (32-bit words):
// H [B*SL*S] | off [B*S] | cnt [B*S] | inv_row [3*B*Rp] | inv_w [3*B*Rp] | (16-byte aligned) items [B*S] int4 |
// chunks [B*CM] int4
struct InterpIndex {
    int *H, *off, *cnt, *inv_row;
    int4 *items, *chunks;
    float* inv_w;
    int CM;
};
inline InterpIndex carve_interp_index(float* ws, int B, int Rp, int S) {
    const int SL = sn2_cdiv(Rp, INV_SLICE_ROWS);
    InterpIndex x;
    x.H = reinterpret_cast<int*>(ws);
    x.off = x.H + (size_t)B * SL * S;
    x.cnt = x.off + (size_t)B * S;
    x.inv_row = x.cnt + (size_t)B * S;
    x.inv_w = reinterpret_cast<float*>(x.inv_row + (size_t)3 * B * Rp);
    x.items = reinterpret_cast<int4*>((reinterpret_cast<uintptr_t>(x.inv_w + (size_t)3 * B * Rp) + 15) & ~(uintptr_t)15);
    x.chunks = x.items + (size_t)B * S;
    x.CM = inv_chunks_per_plot(Rp, S);
    return x;
}

// ---- host helpers of the dispatch code: the grid of a grid-stride row kernel (at most 2048 workgroups); the argument checks
// every sn2_fp entry point starts with
inline int pick_grid(long R, int threads, int rows_per_lane) {
    long g = (R + (long)threads * rows_per_lane - 1) / ((long)threads * rows_per_lane);
    if (g < 1) g = 1;
    if (g > 2048) g = 2048;
    return (int)g;
}

inline int check_fp(const sn2_fp* p) {
    if (!p || p->B <= 0 || p->R_per_plot <= 0 || p->S_per_plot <= 0 || !p->src || !p->h || !p->blk.W || !p->blk.b)
        return SN2_EINVAL;
    if ((p->src_stride & 3) || p->src_stride < p->ca || (p->h_stride & 3) || p->h_stride < p->blk.cout) return SN2_EINVAL;
    if (p->cb > 0 && (!p->skip || p->skip_stride < p->cb)) return SN2_EINVAL;
    if (p->cb % 4 == 0 && p->cb > 0 && (p->skip_stride & 3)) return SN2_EINVAL;
    if ((p->knn_idx == nullptr) != (p->knn_w == nullptr)) return SN2_EINVAL;
    if (p->dsrc && p->dsrc_stride < p->ca) return SN2_EINVAL;
    if (p->blk.cin != p->ca + p->cb) return SN2_EINVAL;
    return 0;
}

// the source-side form applies: workspace given, quads aligned, 32-bit row offsets; with_h: the rows of h are written
// (sn2_fp_head_eval keeps them in LDS and reads no h_stride)
template <int CA, int CO>
bool fp_source_side_ok(const sn2_fp* p, bool with_h = true) {
    const long R = (long)p->B * p->R_per_plot;
    return p->src_ws && p->knn_idx && (p->skip_stride & 3) == 0 && p->src_stride >= 4 * ((CA + 3) / 4) &&
           (!with_h || p->h_stride == 4 * ((CO + 3) / 4)) && R * 3 < (1L << 31);
}

}  // namespace
