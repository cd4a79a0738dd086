// global_level_bwd.hip -- the backward of the global level in ONE launch, training mode: FP3's BatchNorm sums -> FP3 backward ->
// the plot pool's backward -> SA3's BatchNorm sums -> SA3 backward (global_level_bwd_kernel, entry point
// sn2_global_level_backward).  Replaces sn2_fp_bn_sums (FP3's), sn2_fp_backward (FP3), sn2_global_pool_backward and
// sn2_fp_backward (SA3): four dependent launches for 4096 rows.  The exchange between the plots' workgroups is the forward's
// (global_level.h).
#include <type_traits>
#include "global_level.h"

namespace {

// ------------------------------------------------------------------------------------------------ the global level, backward
// One workgroup of 16 waves owns a PLOT, four groups of four waves take its 64-row blocks side by side (as the forward).
// What the arithmetic of the separate launches does not need:
//   * FP3 interpolates with k = 1 from the plot's ONE source with weight 1, so its interpolated inputs are x3[b] for every row:
//     d x3[b] = sum_rows (dp W[:, 0:64]) = (sum_rows dp) W[:, 0:64], one 64 x 64 matrix-vector product per plot instead of a
//     64 x 64 tile product per row, a (B M2, 64) array written and read back, and a row sum; and
//     dW[:, 0:64] = (sum_rows dp) (x) x3[b], an outer product per plot;
//   * the gradient of SA3's output has B x 64 non-zeros (the rows that attained the maximum): it is formed in registers from
//     d x3 and arg3, never stored;
//   * both layers read the same rows x2: their weight gradients are ONE contraction over the rows,
//     [dp_fp3 | dp_sa3]^T (128 x rows) . [x2 | pos2 | 1] (rows x 36), and d x2 is ONE contraction over the 128 channels,
//     [dp_fp3 | dp_sa3] . [W_fp3[:, 64:96] ; W_sa3[:, 0:32]], added to memory once.
// Per plot b:
//   1  sums of dy3 and dy3 xhat3 over the plot's rows (the BatchNorm sums of FP3, taken directly) -> 128 granules per plot;
//   2  every workgroup collects all B x 128 and adds them in fp64 in plot order: d beta, d gamma of FP3;
//   3  dp of FP3 (the split kernel's BatchNorm / ReLU backward formula) into LDS, its column sums, d x3[b]; the plot's pool
//      terms (g, g xhat_sa3 at the arg row) per channel -> 128 granules per plot;
//   4  collect, fp64, plot order: d beta, d gamma of SA3;
//   5  the two contractions, first with dp of FP3 in the staging tile, then with dp of SA3 (sparse dy + the two mean terms);
//   6  COMMIT: d x2 +=, d x3[b] =, dW | db of both layers += into gradient image b (plain read-add-write: the plot owns image
//      b in this launch, B <= 28 < 32 images), and -- plot 0 -- the four BatchNorm vectors += into image 0.
// Every store to a result lies behind the LAST wait.  So a workgroup whose wait runs out (HIP does not promise that the B
// workgroups are resident together) has committed nothing: it publishes POISON for the phase it will not reach, flags its
// plot (ctl[8 + b]), counts itself (ctl[1]) and leaves; the workgroup that leaves the launch last (ticket, ctl[4]) runs the
// flagged plots alone -- first up to their pool granules, then, all granules being present, to the end -- with the same tiles
// and the same fixed-order sums: the bits of an undisturbed launch, each result committed exactly once.  It reads nothing a
// peer stored in this launch except granules (agent-scope atomics issued in front of the peer's barrier and ticket).
// The last workgroup out also advances the launch epoch (ctl[0]): every workgroup of a launch has read it by then.
#ifdef SN2_GB_STAMPS
// diagnostic build only (never shipped; scripts/gb_stamps.py): phase stamps of thread 0 of workgroup 0
__device__ unsigned long long g_gb_dbg[16];
extern "C" int sn2_debug_gb_stamps(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gb_dbg), sizeof(g_gb_dbg));
}
#define BSTAMP(i)                                                                                   \
    if (blockIdx.x == 0 && threadIdx.x == 0) {                                                      \
        unsigned long long t_;                                                                      \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                   \
        g_gb_dbg[i] = t_;                                                                           \
    }
#else
#define BSTAMP(i)
#endif
constexpr int GB_QS = OuterAcc<16, 36>::QS;      // the staged rows [x2 (32) | pos2 (3) | 1]
constexpr int GB_LD = 68;                        // row stride of a group's dp tile [64 rows][64 channels]
constexpr int GB_WC = 33;                        // row stride of [W_fp3[:, 64:96] ; W_sa3[:, 0:32]] (128 x 32)
constexpr int GB_TILES = GL_GROUPS * 64 * (GB_QS + GB_LD);
constexpr int GB_FIXED_FLOATS = GB_TILES + 128 * GB_WC + 8 * 64 + 16 * 128 + 2 * 128 + 4 * 64;
static_assert(GB_QS >= 48, "three 16-column tiles of staged inputs");
static_assert(GL_GROUPS * 128 * 37 <= GB_TILES, "the groups' dW | db partials go through the staging tiles");
static_assert((GB_FIXED_FLOATS + GL_MAX_PLOTS * 128) * 4 <= 160 * 1024, "LDS");

struct GbLayer {
    const float *W, *gamma, *mean, *invstd, *h;
    float *dW, *db, *dgamma, *dbeta;
};
struct GbArgs {
    int B, M2;
    const float* x2;        // (B*M2, 32)
    const float* pos2;      // (B*M2, 4)
    const float* x3;        // (B, 64)
    const int* arg3;        // (B, 64)
    const float* dy3;       // (B*M2, 64) gradient of FP3's BatchNorm output
    float* dx2;             // (B*M2, 32) +=
    float* dx3;             // (B, 64)    +=
    GbLayer sa3, fp3;
    int img_stride;         // floats between two images of (dW, db)
    gl_u64* xchg;           // [2 phases][GL_MAX_PLOTS][128]
    unsigned* ctl;          // [0] epoch of the last finished launch, [1] workgroups that gave up (sticky), [2] ... that a repair has
                            // handled, [4] exit tickets, [8 + b] plot b was left unfinished in this launch
    unsigned spin_limit;
};

// the sixteen waves' partial sums s_red[wave][128] (column sums of the rows each wave holds) from per-thread partials of
// channels 4 qd .. 4 qd + 3: the four row quarters of a wave by shuffles
__device__ __forceinline__ void gb_wave_sums(float (&s)[4], float* s_red, int wv, int lane, int off) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        s[t] += __shfl_xor(s[t], 16);
        s[t] += __shfl_xor(s[t], 32);
    }
    if (lane < 16) {
#pragma unroll
        for (int t = 0; t < 4; ++t) s_red[wv * 128 + off + 4 * lane + t] = s[t];
    }
}

// one plot.  repair: run by the last workgroup out for a flagged plot (nothing is published as POISON).
// publish_only: stop behind the pool granules (the first pass of a repair).  -> false: a wait ran out, nothing was committed.
// ONE_TRIP: M2 <= 256, every group has at most one block -- the rows of h and dy stay in registers from phase 1 to phase 3 and
// dp of FP3 stays in its tile from phase 3 to phase 5 (92 VGPRs; with the trip count left open the kernel spills).
template <bool ONE_TRIP>
__device__ __forceinline__ bool gb_plot(const GbArgs& A, float* smem, int b, unsigned epoch, bool publish_only, bool repair) {
    const int tid = threadIdx.x, lane = tid & 63, t256 = tid & 255;
    const int grp = __builtin_amdgcn_readfirstlane(tid >> 8), g = __builtin_amdgcn_readfirstlane((tid >> 6) & 3);
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* s_q = smem + grp * 64 * GB_QS;                        // the group's staged rows
    float* s_p = smem + GL_GROUPS * 64 * GB_QS + grp * 64 * GB_LD;     // the group's dp tile
    float* s_wc = smem + GB_TILES;                               // [128][GB_WC]
    float* s_par = s_wc + 128 * GB_WC;                           // FP3: mean | invstd | gamma, SA3: mean | invstd | gamma
    float* s_cf = s_par + 6 * 64;                                // FP3: d beta / R | d gamma / R
    float* s_red = s_cf + 2 * 64;                                // [16][128]
    float* s_bnf = s_red + 16 * 128;                             // FP3: d beta (64) | d gamma (64)
    float* s_bn3 = s_bnf + 128;                                  // SA3: the same
    float* s_sdp = s_bn3 + 128;                                  // column sums of FP3's dp over the plot
    float* s_g = s_sdp + 64;                                     // d x3[b]
    float* s_x3 = s_g + 64;
    int* s_arg = reinterpret_cast<int*>(s_x3 + 64);
    float* s_x = s_x3 + 128;                                     // [B][128] the collected granules of an exchange
    __shared__ int s_fail;
    const int B = A.B, M2 = A.M2;
    const long row_lo = (long)b * M2, R_lim = row_lo + M2;
    const int nblk = (M2 + 63) >> 6, trips = ONE_TRIP ? 1 : (nblk + GL_GROUPS - 1) / GL_GROUPS;
    const float invR = 1.0f / (float)(B * M2);
    const int qd = t256 & 15, rw = t256 >> 4;                    // this thread's quad of channels and its rows rw + 16 u of a block
    const int r4 = lane >> 4, c16 = lane & 15;
    const int n_gran = B * 128;
    gl_u64* xa = A.xchg;
    gl_u64* xb = A.xchg + GL_MAX_PLOTS * 128;
    const unsigned tag_a = epoch * 2u, tag_b = epoch * 2u + 1u;
    __syncthreads();                                             // (a repair runs plot after plot through the same LDS)
    BSTAMP(0)
    // ---- 0: what does not depend on the exchange, asked for in front of it
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = tid + 1024 * j, k = i >> 5, c = i & 31;
        s_wc[k * GB_WC + c] = k < 64 ? A.fp3.W[k * 96 + 64 + c] : A.sa3.W[(k - 64) * 35 + c];
    }
    float wa[4];                                                 // W_fp3[4 part + j][c]: the matrix-vector product of d x3
#pragma unroll
    for (int j = 0; j < 4; ++j) wa[j] = A.fp3.W[(4 * (tid >> 6) + j) * 96 + (tid & 63)];
    float dx3_old = 0.f, xh_arg = 0.f;
    bool arg_ok = false;
    if (tid < 64) {
        s_par[0 * 64 + tid] = A.fp3.mean[tid], s_par[1 * 64 + tid] = A.fp3.invstd[tid], s_par[2 * 64 + tid] = A.fp3.gamma[tid];
        const float m3 = A.sa3.mean[tid], is3 = A.sa3.invstd[tid];
        s_par[3 * 64 + tid] = m3, s_par[4 * 64 + tid] = is3, s_par[5 * 64 + tid] = A.sa3.gamma[tid];
        s_x3[tid] = A.x3[(size_t)b * 64 + tid];
        const int ra = A.arg3[(size_t)b * 64 + tid];
        arg_ok = ra >= 0 && ra < M2;
        s_arg[tid] = arg_ok ? ra : -1;
        if (arg_ok) xh_arg = (A.sa3.h[(size_t)(row_lo + ra) * 64 + tid] - m3) * is3;
        dx3_old = A.dx3[(size_t)b * 64 + tid];
    }
    if (tid == 0) s_fail = 0;
    if constexpr (ONE_TRIP) {
        if (grp < nblk)
            stage_inputs<32, 3, false>(s_q, GB_QS, g, lane, row_lo + (long)grp * 64, (int)R_lim, M2, M2, A.x2, 32, nullptr, nullptr, nullptr,
                                       nullptr, A.pos2, 4);
    }
    float4 hv[4], dv[4];
    auto load_rows = [&](const float* __restrict__ p, long r0, float4 (&v)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long r = r0 + rw + 16 * u;
            v[u] = reinterpret_cast<const float4*>(p + (size_t)(r < R_lim ? r : R_lim - 1) * 64)[qd];
        }
    };
    __syncthreads();
    BSTAMP(1)
    // the per-channel constants of this thread's quad stay in LDS (one 16-byte read each where they are used)
    auto quad = [&](const float* p, float (&v)[4]) {
        const float4 q = *reinterpret_cast<const float4*>(p + 4 * qd);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    };
    // ================================================================ 1: FP3's BatchNorm sums over the plot's rows
    {
        float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f}, mean_f[4], is_f[4];
        quad(s_par, mean_f), quad(s_par + 64, is_f);
        for (int it = 0; it < trips; ++it) {
            const int blk = it * GL_GROUPS + grp;
            const long r0 = row_lo + (long)blk * 64;
            if (blk < nblk) {
                load_rows(A.fp3.h, r0, hv);
                load_rows(A.dy3, r0, dv);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool live = r0 + rw + 16 * u < R_lim;
                    const float hq[4] = {hv[u].x, hv[u].y, hv[u].z, hv[u].w}, dq[4] = {dv[u].x, dv[u].y, dv[u].z, dv[u].w};
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const float dd = live ? dq[t] : 0.f;
                        s1[t] += dd;
                        s2[t] = fmaf(dd, (hq[t] - mean_f[t]) * is_f[t], s2[t]);
                    }
                }
            }
        }
        gb_wave_sums(s1, s_red, wv, lane, 0);
        gb_wave_sums(s2, s_red, wv, lane, 64);
        __syncthreads();
        if (tid < 128) {
            float v = 0.f;
#pragma unroll
            for (int w = 0; w < 16; ++w) v += s_red[w * 128 + tid];
            __hip_atomic_store(xa + (size_t)b * 128 + tid, ((gl_u64)tag_a << 32) | (gl_u64)__float_as_uint(v), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    BSTAMP(2)
    // ================================================================ 2: everybody's, fp64, plot order
    if (!gl_collect(xa, n_gran, tag_a, s_x, A.spin_limit)) s_fail = 1;
    __syncthreads();
    BSTAMP(3)
    if (s_fail) {
        if (!repair && tid < 128)
            __hip_atomic_store(xb + (size_t)b * 128 + tid, (gl_u64)(tag_b ^ GL_POISON) << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return false;
    }
    if (tid < 128) {
        double acc = 0.0;
        for (int w = 0; w < B; ++w) acc += (double)s_x[w * 128 + tid];
        s_bnf[tid] = (float)acc;
        s_cf[tid] = (float)acc * invR;
    }
    __syncthreads();
    // ================================================================ 3: dp of FP3, its column sums, d x3[b], the pool's terms
    // d pre-activation of a (Linear -> ReLU -> BatchNorm) block from the gradient of its output, fp_bwd_split_kernel's formula
    // (dbeta_r, dgamma_r: the BatchNorm sums over the batch's rows)
    auto dp_of = [&](float hh, float dd, float mean, float is, float gam, float dbeta_r, float dgamma_r, bool live) {
        const float xh = (hh - mean) * is;
        const float dh = gam * is * (dd - dbeta_r - xh * dgamma_r);
        return (live && hh > 0.f) ? dh : 0.f;
    };
    // the block's dp of FP3 -> the group's tile; adds its column sums to sd
    auto stage_dp_fp3 = [&](long r0, float (&sd)[4]) {
        float mean_f[4], is_f[4], gam_f[4], dbt_f[4], dgm_f[4];
        quad(s_par, mean_f), quad(s_par + 64, is_f), quad(s_par + 128, gam_f), quad(s_cf, dbt_f), quad(s_cf + 64, dgm_f);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool live = r0 + rw + 16 * u < R_lim;
            const float hq[4] = {hv[u].x, hv[u].y, hv[u].z, hv[u].w}, dq[4] = {dv[u].x, dv[u].y, dv[u].z, dv[u].w};
            float p[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                p[t] = dp_of(hq[t], dq[t], mean_f[t], is_f[t], gam_f[t], dbt_f[t], dgm_f[t], live);
                sd[t] += p[t];
            }
            *reinterpret_cast<float4*>(&s_p[(rw + 16 * u) * GB_LD + 4 * qd]) = make_float4(p[0], p[1], p[2], p[3]);
        }
    };
    {
        float sd[4] = {0.f, 0.f, 0.f, 0.f};
        for (int it = 0; it < trips; ++it) {
            const int blk = it * GL_GROUPS + grp;
            const long r0 = row_lo + (long)blk * 64;
            if (blk < nblk) {
                if constexpr (!ONE_TRIP) {           // (one trip: the rows are still in registers)
                    load_rows(A.fp3.h, r0, hv);
                    load_rows(A.dy3, r0, dv);
                }
                stage_dp_fp3(r0, sd);
            }
        }
        gb_wave_sums(sd, s_red, wv, lane, 0);
        __syncthreads();
        if (tid < 64) {
            float v = 0.f;
#pragma unroll
            for (int w = 0; w < 16; ++w) v += s_red[w * 128 + tid];
            s_sdp[tid] = v;
        }
        __syncthreads();
        {
            const int part = tid >> 6;
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = fmaf(s_sdp[4 * part + j], wa[j], acc);
            s_red[part * 128 + 64 + (tid & 63)] = acc;
        }
        __syncthreads();
        if (tid < 64) {
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) v += s_red[k * 128 + 64 + tid];
            const float gg = dx3_old + v;
            s_g[tid] = gg;
            const float g1 = arg_ok ? gg : 0.f;
            __hip_atomic_store(xb + (size_t)b * 128 + tid, ((gl_u64)tag_b << 32) | (gl_u64)__float_as_uint(g1), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(xb + (size_t)b * 128 + 64 + tid, ((gl_u64)tag_b << 32) | (gl_u64)__float_as_uint(g1 * xh_arg),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    BSTAMP(4)
    if (publish_only) return true;
    // ================================================================ 5: the two contractions, block by block
    // (FP3's dW has no third column tile: the position columns are not its inputs and its db is the column sum of dp above)
    f32x4 acc_f[2], acc_3[3];                    // dW rows 16 g .. 16 g + 15 of FP3 (skip columns) and dW | db of SA3
    f32x4 D[2];                                  // d x2 rows 16 g .. 16 g + 15 of the block
    acc_f[0] = acc_f[1] = acc_3[0] = acc_3[1] = acc_3[2] = D[0] = D[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 hs[4];
    float dx2_old[2][4];                         // asked for ahead, added behind the contractions: one round trip, not eight
    auto ask_block = [&](long r0) {
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = r0 + 16 * g + 4 * r4 + r;
                dx2_old[jt][r] = A.dx2[(size_t)(row < R_lim ? row : R_lim - 1) * 32 + 16 * jt + c16];
            }
        load_rows(A.sa3.h, r0, hs);
    };
    // the tile's dp (64 rows x 64 channels of one layer) against the staged inputs (rows are K: NT column tiles of dW) and
    // against the layer's rows k0 .. k0 + 63 of the stacked weights (channels are K: d x2)
    auto contract_tile = [&](auto& acc, auto nt, int k0) {
        constexpr int NT = decltype(nt)::value;
#pragma unroll 4
        for (int st = 0; st < 16; ++st) {
            const float av = s_p[(4 * st + r4) * GB_LD + 16 * g + c16];
#pragma unroll
            for (int c = 0; c < NT; ++c)
                acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, s_q[(4 * st + r4) * GB_QS + 16 * c + c16], acc[c], 0, 0, 0);
        }
#pragma unroll 4
        for (int kb = 0; kb < 16; ++kb) {
            const float av = s_p[(16 * g + c16) * GB_LD + 4 * kb + r4];
#pragma unroll
            for (int jt = 0; jt < 2; ++jt)
                D[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, s_wc[(k0 + 4 * kb + r4) * GB_WC + 16 * jt + c16], D[jt], 0, 0, 0);
        }
    };
    if constexpr (ONE_TRIP) {
        // dp of FP3 is in the tiles and the inputs were staged in phase 0: the first contraction does not need the pool's sums
        // and runs while the peers' granules arrive
        if (grp < nblk) {
            ask_block(row_lo + (long)grp * 64);
            contract_tile(acc_f, std::integral_constant<int, 2>{}, 0);
        }
    }
    // ---- 4: SA3's BatchNorm sums: B terms per channel
    if (!gl_collect(xb, n_gran, tag_b, s_x, A.spin_limit)) s_fail = 1;
    __syncthreads();
    BSTAMP(5)
    if (s_fail) return false;
    if (tid < 128) {
        double acc = 0.0;
        for (int w = 0; w < B; ++w) acc += (double)s_x[w * 128 + tid];
        s_bn3[tid] = (float)acc;
    }
    __syncthreads();
    for (int it = 0; it < trips; ++it) {
        const int blk = it * GL_GROUPS + grp;
        const long r0 = row_lo + (long)blk * 64;
        const bool act = blk < nblk;
        if constexpr (!ONE_TRIP) {
            if (act) {
                ask_block(r0);
                stage_inputs<32, 3, false>(s_q, GB_QS, g, lane, r0, (int)R_lim, M2, M2, A.x2, 32, nullptr, nullptr, nullptr, nullptr,
                                           A.pos2, 4);
                float sd[4] = {0.f, 0.f, 0.f, 0.f};
                load_rows(A.fp3.h, r0, hv);
                load_rows(A.dy3, r0, dv);
                stage_dp_fp3(r0, sd);
            }
            __syncthreads();
            D[0] = D[1] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (act) contract_tile(acc_f, std::integral_constant<int, 2>{}, 0);
            __syncthreads();
        }
        if (act) {
            // dp of SA3: the gradient of its output is d x3[b][c] at row arg3[b][c] and zero elsewhere
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int rp = blk * 64 + rw + 16 * u;            // row of the plot
                const bool live = rp < M2;
                const float hq[4] = {hs[u].x, hs[u].y, hs[u].z, hs[u].w};
                float p[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int c = 4 * qd + t;
                    const float dd = s_arg[c] == rp ? s_g[c] : 0.f;
                    p[t] = dp_of(hq[t], dd, s_par[3 * 64 + c], s_par[4 * 64 + c], s_par[5 * 64 + c], s_bn3[c] * invR, s_bn3[64 + c] * invR, live);
                }
                *reinterpret_cast<float4*>(&s_p[(rw + 16 * u) * GB_LD + 4 * qd]) = make_float4(p[0], p[1], p[2], p[3]);
            }
        }
        __syncthreads();
        if (act) {
            contract_tile(acc_3, std::integral_constant<int, 3>{}, 64);
#pragma unroll
            for (int jt = 0; jt < 2; ++jt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long row = r0 + 16 * g + 4 * r4 + r;
                    if (row < R_lim) A.dx2[(size_t)row * 32 + 16 * jt + c16] = dx2_old[jt][r] + D[jt][r];
                }
        }
        __syncthreads();
    }
    BSTAMP(6)
    // ================================================================ 6: commit the plot's dW | db, d x3, the BatchNorm vectors
    // (the old values of every word are asked for together, in front of the groups' exchange: as read-add-write one after the
    // other the adds were a chain of dependent memory round trips)
    {
        float* s_acc = smem;                     // [4 groups][128 channels][37] through the staging tiles
        const int img = b * A.img_stride;
        float* dst[5];
        float old[5], old_o[4], old_bn[2] = {0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int i = tid + 1024 * j, o = i / 36, k = i - o * 36;
            dst[j] = nullptr;
            if (i < 128 * 36) {
                if (o < 64) {
                    if (k < 32) dst[j] = A.fp3.dW + img + o * 96 + 64 + k;
                    else if (k == 35) dst[j] = A.fp3.db + img + o;        // (the position columns are not FP3's)
                } else {
                    dst[j] = k < 35 ? A.sa3.dW + img + (o - 64) * 35 + k : A.sa3.db + img + (o - 64);
                }
            }
            old[j] = dst[j] ? *dst[j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {            // FP3's interpolated columns
            const int i = tid + 1024 * j;
            old_o[j] = A.fp3.dW[img + (i >> 6) * 96 + (i & 63)];
        }
        float* bn_dst[2] = {nullptr, nullptr};
        if (b == 0 && tid < 128) {
            bn_dst[0] = tid < 64 ? A.fp3.dbeta + tid : A.fp3.dgamma + (tid - 64);
            bn_dst[1] = tid < 64 ? A.sa3.dbeta + tid : A.sa3.dgamma + (tid - 64);
            old_bn[0] = *bn_dst[0], old_bn[1] = *bn_dst[1];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int o = 16 * g + 4 * r4 + q, k = 16 * c + c16;
                if (k < 36) {
                    if (c < 2) s_acc[(grp * 128 + o) * 37 + k] = acc_f[c][q];
                    s_acc[(grp * 128 + 64 + o) * 37 + k] = acc_3[c][q];
                }
            }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int i = tid + 1024 * j, o = i / 36, k = i - o * 36;
            if (dst[j]) {
                const float v = (o < 64 && k == 35) ? s_sdp[o]          // FP3's db: the column sums of its dp
                                                    : (s_acc[(0 * 128 + o) * 37 + k] + s_acc[(1 * 128 + o) * 37 + k]) +
                                                          (s_acc[(2 * 128 + o) * 37 + k] + s_acc[(3 * 128 + o) * 37 + k]);
                *dst[j] = old[j] + v;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {            // (sum_rows dp) (x) x3[b]
            const int i = tid + 1024 * j, o = i >> 6, k = i & 63;
            A.fp3.dW[img + o * 96 + k] = old_o[j] + s_sdp[o] * s_x3[k];
        }
        if (tid < 64) A.dx3[(size_t)b * 64 + tid] = s_g[tid];
        if (bn_dst[0]) {
            *bn_dst[0] = old_bn[0] + s_bnf[tid];
            *bn_dst[1] = old_bn[1] + s_bn3[tid];
        }
    }
    BSTAMP(7)
    return true;
}

// The last workgroup out finishes the flagged plots alone: first every one of them up to its pool granules (they replace the
// POISON), then -- every granule of both phases is present now -- each to its end.  (A function of its own, not inlined: the
// registers of the launch proper are allocated without it.)
template <bool ONE_TRIP>
__device__ __noinline__ void gb_repair(GbArgs A, float* smem, unsigned epoch) {
    for (int pass = 0; pass < 2; ++pass)
        for (int b = 0; b < A.B; ++b)
            if (__hip_atomic_load(&A.ctl[8 + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) gb_plot<ONE_TRIP>(A, smem, b, epoch, pass == 0, true);
    __syncthreads();
    if (threadIdx.x == 0) {                      // the give-ups are handled
        for (int b = 0; b < A.B; ++b) __hip_atomic_store(&A.ctl[8 + b], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&A.ctl[2], __hip_atomic_load(&A.ctl[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <bool ONE_TRIP>
__global__ __launch_bounds__(1024) void global_level_bwd_kernel(GbArgs A) {
    extern __shared__ __attribute__((aligned(16))) float gb_smem[];
    __shared__ unsigned s_epoch;
    __shared__ int s_last;
    const int tid = threadIdx.x;
    if (tid == 0) s_epoch = __hip_atomic_load(&A.ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
    __syncthreads();
    const unsigned epoch = s_epoch;
    const bool ok = gb_plot<ONE_TRIP>(A, gb_smem, (int)blockIdx.x, epoch, false, false);
    if (!ok && tid == 0) {
        __hip_atomic_store(&A.ctl[8 + blockIdx.x], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        atomicAdd(&A.ctl[1], 1u);
    }
    __syncthreads();                             // (every wave's atomics of the body are complete)
    if (tid == 0) {
        const unsigned t = atomicAdd(&A.ctl[4], 1u);
        int last = 0;
        if (t == gridDim.x - 1) {                // every other workgroup of the launch has left its body
            __hip_atomic_store(&A.ctl[4], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            last = __hip_atomic_load(&A.ctl[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) !=
                           __hip_atomic_load(&A.ctl[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                       ? 2
                       : 1;
        }
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    if (s_last == 2) gb_repair<ONE_TRIP>(A, gb_smem, epoch);
    if (tid == 0) __hip_atomic_store(&A.ctl[0], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

// Routes (include/strata_hip.h).  gl_bwd_covers: what the launch takes besides the architecture's shapes (any number of rows per
// plot); the route of the network's backward is narrower ON PURPOSE: one 64-row block per group of the workgroup is the instance
// that has been measured against the four separate launches.
static bool gl_bwd_covers(int B, int frozen, int bf16) { return B <= GL_MAX_PLOTS && !frozen && !bf16; }
extern "C" int sn2_global_level_backward_route(int B, int M2, int frozen, int bf16) {
    return gl_bwd_covers(B, frozen, bf16) && M2 <= GL_BWD_MAX_ROWS;
}

extern "C" int sn2_global_level_backward(const sn2_fp* sa3, const sn2_fp* fp3, const int* arg3, unsigned long long* xchg,
                                         unsigned* ctl, void* stream) {
    if (!sa3 || !fp3 || !arg3 || !xchg || !ctl) return SN2_EINVAL;
    const int B = sa3->B, M2 = sa3->R_per_plot;
    if (!(B > 0 && M2 > 0 && fp3->B == B && fp3->R_per_plot == M2 && sa3->S_per_plot == M2 && fp3->S_per_plot == 1)) return SN2_EINVAL;
    if (!(sa3->ca == 32 && sa3->cb == 3 && sa3->blk.cin == 35 && sa3->blk.cout == 64 && fp3->ca == 64 && fp3->cb == 32 &&
          fp3->blk.cin == 96 && fp3->blk.cout == 64))
        return SN2_ELIMIT;
    if (!gl_bwd_covers(B, sa3->blk.frozen_stats || fp3->blk.frozen_stats, sa3->blk.mma_bf16 || fp3->blk.mma_bf16) || sa3->act_bf16 ||
        fp3->act_bf16)
        return SN2_ELIMIT;
    if (sa3->knn_idx || sa3->src_a || !fp3->knn_idx || fp3->src_a) return SN2_EINVAL;
    if (!sa3->src || sa3->src_stride != 32 || !sa3->skip || sa3->skip_stride != 4 || !sa3->h || sa3->h_stride != 64) return SN2_EINVAL;
    if (!fp3->src || fp3->src_stride != 64 || fp3->skip != sa3->src || fp3->skip_stride != 32 || !fp3->h || fp3->h_stride != 64)
        return SN2_EINVAL;
    // FP3: dy = the gradient of its output, dsrc = d x3 (B, 64), dskip = d x2 (B*M2, 32); SA3: dsrc = the same d x2
    if (!fp3->dy || !fp3->dsrc || fp3->dsrc_stride != 64 || !fp3->dskip || fp3->dskip_stride != 32 || sa3->dsrc != fp3->dskip ||
        sa3->dsrc_stride != 32)
        return SN2_EINVAL;
    for (const sn2_block* k : {&sa3->blk, &fp3->blk})
        if (!k->W || !k->gamma || !k->mean || !k->invstd || !k->dW || !k->db || !k->dgamma || !k->dbeta) return SN2_EINVAL;
    // a plot adds its dW | db into an image of its own
    if ((long)B * M2 >= (1L << 31) / 64) return SN2_ELIMIT;
    if (sa3->blk.grad_replicas < B || fp3->blk.grad_replicas < B || sa3->blk.grad_replica_stride != fp3->blk.grad_replica_stride)
        return SN2_ELIMIT;
    GbArgs A;
    A.B = B, A.M2 = M2;
    A.x2 = sa3->src, A.pos2 = sa3->skip, A.x3 = fp3->src, A.arg3 = arg3, A.dy3 = fp3->dy, A.dx2 = fp3->dskip, A.dx3 = fp3->dsrc;
    auto layer = [](const sn2_fp* p) {
        GbLayer l;
        l.W = p->blk.W, l.gamma = p->blk.gamma, l.mean = p->blk.mean, l.invstd = p->blk.invstd, l.h = p->h;
        l.dW = p->blk.dW, l.db = p->blk.db, l.dgamma = p->blk.dgamma, l.dbeta = p->blk.dbeta;
        return l;
    };
    A.sa3 = layer(sa3), A.fp3 = layer(fp3);
    A.img_stride = sa3->blk.grad_replica_stride;
    A.xchg = xchg, A.ctl = ctl;
    A.spin_limit = g_gl_spin_limit;
    const size_t lds = ((size_t)GB_FIXED_FLOATS + (size_t)B * 128) * 4;
    auto kern = M2 <= GL_GROUPS * 64 ? &global_level_bwd_kernel<true> : &global_level_bwd_kernel<false>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3(B), dim3(1024), lds, (hipStream_t)stream, A);
    SN2_RETURN_LAUNCH();
}
