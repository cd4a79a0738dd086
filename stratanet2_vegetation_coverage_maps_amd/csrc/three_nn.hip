// three_nn.hip -- the three nearest sources of every target: the brute-force scan and the exact grid search with its grid
// build and target sort.  Entry points sn2_three_nn, sn2_three_nn_xy, sn2_three_nn_xy_copy and their size helpers.
// All discrete decisions use the canonical fp32 squared distance sn2_d2 (common.h) so that the index structures
// are bit-identical to the oracle's.
#include "common.h"
#include "plot_sort.h"
#include <stdlib.h>

// ------------------------------------------------------------------------------------------------------------
// three_nn: one lane per target point, the plot's source positions staged through LDS in tiles of 1024 (AoS4, every
// lane reads the same address -> broadcast), ascending source index with strict '<' insertion so ties keep the
// lowest index (oracle: stable sort).  Writes idx (B*T,3), w (B*T,3) = 1/max(d2,1e-16); unused slots w = 0.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void three_nn_kernel(const float* __restrict__ src, int S, const float* __restrict__ dst,
                                                       int T, int k, int* __restrict__ idx, float* __restrict__ w) {
    __shared__ float4 s_src[1024];
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const bool valid = t < T;
    const float* sx = src + (size_t)b * 3 * S;
    const float* dx = dst + (size_t)b * 3 * T;
    const float qx = valid ? dx[t] : 0.f, qy = valid ? dx[(size_t)T + t] : 0.f, qz = valid ? dx[2 * (size_t)T + t] : 0.f;
    float d0 = INFINITY, d1 = INFINITY, d2 = INFINITY;
    int i0 = -1, i1 = -1, i2 = -1;
    for (int s0 = 0; s0 < S; s0 += 1024) {
        const int tn = (S - s0) < 1024 ? (S - s0) : 1024;
        __syncthreads();
        for (int i = threadIdx.x; i < tn; i += 256)
            s_src[i] = make_float4(sx[s0 + i], sx[(size_t)S + s0 + i], sx[2 * (size_t)S + s0 + i], 0.f);
        __syncthreads();
        for (int i = 0; i < tn; ++i) {
            const float4 p = s_src[i];
            const float dd = sn2_d2(p.x, p.y, p.z, qx, qy, qz);
            if (dd < d2) {
                if (dd < d1) {
                    d2 = d1;
                    i2 = i1;
                    if (dd < d0) {
                        d1 = d0;
                        i1 = i0;
                        d0 = dd;
                        i0 = s0 + i;
                    } else {
                        d1 = dd;
                        i1 = s0 + i;
                    }
                } else {
                    d2 = dd;
                    i2 = s0 + i;
                }
            }
        }
    }
    if (!valid) return;
    const size_t o = ((size_t)b * T + t) * 3;
    const bool u1 = (k >= 2) && (i1 >= 0), u2 = (k >= 3) && (i2 >= 0);
    idx[o + 0] = i0;
    idx[o + 1] = u1 ? i1 : i0;
    idx[o + 2] = u2 ? i2 : i0;
    w[o + 0] = 1.0f / fmaxf(d0, 1e-16f);
    w[o + 1] = u1 ? 1.0f / fmaxf(d1, 1e-16f) : 0.f;
    w[o + 2] = u2 ? 1.0f / fmaxf(d2, 1e-16f) : 0.f;
}

// ------------------------------------------------------------------------------------------------------------
// Grid 3-NN (exact), for targets that FPS already put into Morton order (FP1: the targets are the plot's points).
// The plot's S sources are binned once into a G x G grid over their x,y bounding box (nn_grid_build_kernel: LDS counting
// sort -> a table of (x, y, z, source index) in cell order + the cell starts).  One wave takes 64 consecutive SORTED
// targets -- neighbours in space -- and treats them as one query box: it visits the cells under the box, then square
// rings of growing radius rho around it, every lane testing every visited source (wave-uniform loops, LDS broadcast
// reads; a per-lane walk of each lane's own cells was tried first and lost to the brute-force scan: a wave runs as long
// as its worst lane at every cell).  It stops when the largest k-th best squared distance of its lanes is below what any
// unvisited source can reach: such a source lies in a cell more than rho columns or rows away from the cells of ALL the
// wave's targets, so its x or y gap -- hence its distance -- to each of them exceeds rho cell widths (taken 0.1 % short
// and minus 1e-4 m, which covers the fp32 rounding of the cell assignment and of sn2_d2).  Candidates arrive in arbitrary
// index order, so the running best three are kept in (d2, index) lexicographic order: exactly the brute-force scan's
// "ascending index, strict <" result, bit for bit.  ~50-150 distance evaluations per target instead of S = 1024.
// ------------------------------------------------------------------------------------------------------------
constexpr int NN_GMAX = 32;
constexpr int NN_HDR = NN_GMAX * NN_GMAX + 1 + 7;   // cell starts (G*G+1), then x0, y0, inv_x, inv_y, min cell width, G (as int), pad

__global__ __launch_bounds__(256) void nn_grid_build_kernel(const float* __restrict__ src, int S, int G,
                                                            float4* __restrict__ tbl, int* __restrict__ hdr) {
    __shared__ int s_hist[NN_GMAX * NN_GMAX + 1];
    __shared__ float s_mm[4][4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* sx = src + (size_t)b * 3 * S;
    const float* sy = sx + S;
    const float* sz = sy + S;
    auto load = [&](int i) { return make_float3(sx[i], sy[i], sz[i]); };
    float lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
    for_plot_points<1, 256>(S, load, [&](int, float3 v) {
        lo[0] = fminf(lo[0], v.x); hi[0] = fmaxf(hi[0], v.x);
        lo[1] = fminf(lo[1], v.y); hi[1] = fmaxf(hi[1], v.y);
    });
    block_minmax<256, 2>(lo, hi, s_mm);
    const float x0 = lo[0], y0 = lo[1];
    const float ex = fmaxf(hi[0] - x0, 1e-6f), ey = fmaxf(hi[1] - y0, 1e-6f);
    const float ix = (float)G / ex, iy = (float)G / ey;
    int* hb = hdr + (size_t)b * NN_HDR;
    if (tid == 0) {
        float* hf = reinterpret_cast<float*>(hb + NN_GMAX * NN_GMAX + 1);
        hf[0] = x0; hf[1] = y0; hf[2] = ix; hf[3] = iy; hf[4] = fminf(ex, ey) / (float)G;
        hb[NN_GMAX * NN_GMAX + 1 + 5] = G;
    }
    float4* tb = tbl + (size_t)b * S;
    plot_counting_sort<1, 256, NN_GMAX * NN_GMAX, true>(
        s_hist, G * G, S, load,
        [&](float3 v) {
            int cx = (int)((v.x - x0) * ix), cy = (int)((v.y - y0) * iy);
            cx = cx < 0 ? 0 : (cx > G - 1 ? G - 1 : cx);
            cy = cy < 0 ? 0 : (cy > G - 1 ? G - 1 : cy);
            return cy * G + cx;
        },
        [&](int cell, int start) { hb[cell] = start; },       // cell starts + end word (= S)
        [&](int i, int p, float3 v) { tb[p] = make_float4(v.x, v.y, v.z, __int_as_float(i)); });
}

#ifdef SN2_NN_STAMPS
// diagnostic build only (never shipped): per wave {cycles, candidates tested, final ring, query box cells}
__device__ unsigned long long g_nn_dbg[4 * 16384];
extern "C" int sn2_debug_nn_stamps(unsigned long long* out, int n) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_nn_dbg), sizeof(unsigned long long) * n);
}
#endif
__global__ __launch_bounds__(256) void three_nn_grid_kernel(const float4* __restrict__ tbl, const int* __restrict__ hdr, int S,
                                                            int T, int k, const int* __restrict__ dst_order,
                                                            const float4* __restrict__ dst_sorted,
                                                            int* __restrict__ idx, float* __restrict__ w, int B, int gx,
                                                            int* __restrict__ idx_sorted, float* __restrict__ w_sorted) {
    extern __shared__ __attribute__((aligned(16))) float4 s_tbl[];      // S entries, then the cell starts
    // XCD-aware placement (as ball_query_grid_kernel): with B = 0 the grid is (gx, plots) as before; with B > 0 it is one-
    // dimensional, workgroup w = (XCD w & 7, turn w >> 3), and plot b is worked on by XCD b % 8 only -- the results go to the
    // targets' ORIGINAL rows, 24 bytes each into lines that ten waves share, and only waves behind the same L2 merge them
    // there before they are written back
    int b = blockIdx.y, bx = blockIdx.x;
    if (B > 0) {
        const int turn = (int)(blockIdx.x >> 3);
        b = (int)(blockIdx.x & 7u) + 8 * (turn / gx);
        bx = turn % gx;
        if (b >= B) return;
    }
    const int lane = threadIdx.x & 63;
    const int* hb = hdr + (size_t)b * NN_HDR;
    const int G = __builtin_amdgcn_readfirstlane(hb[NN_GMAX * NN_GMAX + 1 + 5]);
    int* s_cell = reinterpret_cast<int*>(s_tbl + S);
    for (int i = threadIdx.x; i < S; i += 256) s_tbl[i] = tbl[(size_t)b * S + i];
    for (int i = threadIdx.x; i <= G * G; i += 256) s_cell[i] = hb[i];
    __syncthreads();
    const int p = bx * 256 + threadIdx.x;                                // sorted position
    if (p - lane >= T) return;                                           // whole wave past the end
    const bool valid = p < T;
    const float* hf = reinterpret_cast<const float*>(hb + NN_GMAX * NN_GMAX + 1);
    const float x0 = hf[0], y0 = hf[1], ix = hf[2], iy = hf[3], cw = hf[4];
    const float4 q = dst_sorted[(size_t)b * T + (valid ? p : T - 1)];
    const float qx = q.x, qy = q.y, qz = q.z;
    // the cells under the wave's targets (clamped like the sources' cells; the cell function is monotone)
    auto cell1 = [&](float v, float o, float inv) {
        int c = (int)((v - o) * inv);
        return (v - o < 0.f || c < 0) ? 0 : (c > G - 1 ? G - 1 : c);
    };
    const int bx0 = __builtin_amdgcn_readfirstlane(cell1(wave_min(qx), x0, ix)),
              bx1 = __builtin_amdgcn_readfirstlane(cell1(wave_max(qx), x0, ix));
    const int by0 = __builtin_amdgcn_readfirstlane(cell1(wave_min(qy), y0, iy)),
              by1 = __builtin_amdgcn_readfirstlane(cell1(wave_max(qy), y0, iy));
    constexpr unsigned long long KINF = (0x7F800000ull << 32) | 0x7FFFFFFFull;     // (+inf, no index)
    unsigned long long k0 = KINF, k1 = KINF, k2 = KINF;
    const int kk = k < S ? k : S;          // slots that will be filled
#ifdef SN2_NN_STAMPS
    unsigned long long t_begin;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_begin)::"memory");
    unsigned n_cand = 0;
    int rho_last = 0;
#endif
    for (int rho = 0;; ++rho) {
#ifdef SN2_NN_STAMPS
        rho_last = rho;
#endif
        const int xl = bx0 - rho, xh = bx1 + rho, yl = by0 - rho, yh = by1 + rho;
        const int cxl = xl < 0 ? 0 : xl, cxh = xh > G - 1 ? G - 1 : xh;
        for (int cy = (yl < 0 ? 0 : yl); cy <= (yh > G - 1 ? G - 1 : yh); ++cy) {
            // a new row of the rectangle is one segment of contiguous cells; an old row contributes its two new end cells
            const bool whole = rho == 0 || cy == yl || cy == yh;
            for (int sg = 0; sg < (whole ? 1 : 2); ++sg) {
                int c_lo, c_hi;
                if (whole) {
                    c_lo = cy * G + cxl; c_hi = cy * G + cxh;
                } else if (sg == 0) {
                    if (xl < 0) continue;
                    c_lo = c_hi = cy * G + xl;
                } else {
                    if (xh > G - 1) continue;
                    c_lo = c_hi = cy * G + xh;
                }
                // wave-uniform bounds in SGPRs: scalar loop control and one broadcast LDS read per candidate; the common
                // case (the candidate beats nobody's third best) is 8 VALU ops, one compare and one branch.  (Written
                // inline, not as a lambda: called through a closure the best-three state ended up in scratch memory.)
                const int p_lo = __builtin_amdgcn_readfirstlane(s_cell[c_lo]), p_hi = __builtin_amdgcn_readfirstlane(s_cell[c_hi + 1]);
#ifdef SN2_NN_STAMPS
                n_cand += p_hi - p_lo;
#endif
// the running best three as 64-bit keys (d2 bits << 32 | source index): d2 >= 0, so the unsigned order of the keys IS the
// lexicographic (d2, index) order, and an insertion is three branch-free min/max steps.  (With 64 lanes per query box
// nearly every candidate is a hit for SOME lane, so the nested-if insertion ran, divergent, for most candidates.)
#define NN_INSERT(DD, CW)                                                                                  \
    {                                                                                                      \
        const unsigned long long kn_ = ((unsigned long long)__float_as_uint(DD) << 32) | (unsigned)__float_as_int(CW); \
        k2 = kn_ < k2 ? kn_ : k2;                                                                          \
        const unsigned long long a_ = k1 < k2 ? k1 : k2, b_ = k1 < k2 ? k2 : k1;                           \
        k1 = a_; k2 = b_;                                                                                  \
        const unsigned long long c_ = k0 < k1 ? k0 : k1, e_ = k0 < k1 ? k1 : k0;                           \
        k0 = c_; k1 = e_;                                                                                  \
    }
                int sp = p_lo;
                for (; sp + 4 <= p_hi; sp += 4) {
                    const float4 c0 = s_tbl[sp], c1 = s_tbl[sp + 1], c2 = s_tbl[sp + 2], c3 = s_tbl[sp + 3];
                    const float e0 = sn2_d2(c0.x, c0.y, c0.z, qx, qy, qz), e1 = sn2_d2(c1.x, c1.y, c1.z, qx, qy, qz);
                    const float e2 = sn2_d2(c2.x, c2.y, c2.z, qx, qy, qz), e3 = sn2_d2(c3.x, c3.y, c3.z, qx, qy, qz);
                    if (fminf(fminf(e0, e1), fminf(e2, e3)) <= __uint_as_float((unsigned)(k2 >> 32))) {
                        NN_INSERT(e0, c0.w)
                        NN_INSERT(e1, c1.w)
                        NN_INSERT(e2, c2.w)
                        NN_INSERT(e3, c3.w)
                    }
                }
                for (; sp < p_hi; ++sp) {
                    const float4 c = s_tbl[sp];
                    const float dd = sn2_d2(c.x, c.y, c.z, qx, qy, qz);
                    NN_INSERT(dd, c.w)
                }
#undef NN_INSERT
            }
        }
        if (xl <= 0 && yl <= 0 && xh >= G - 1 && yh >= G - 1) break;     // the whole grid has been visited
        const float reach = (float)rho * cw * 0.999f - 1e-4f;           // nothing unvisited is closer than this
        const float dk = __uint_as_float((unsigned)((kk >= 3 ? k2 : (kk == 2 ? k1 : k0)) >> 32));
        const float worst = wave_max(valid ? dk : 0.f);
        if (reach > 0.f && worst < reach * reach) break;
    }
    const float d0 = __uint_as_float((unsigned)(k0 >> 32)), d1 = __uint_as_float((unsigned)(k1 >> 32)),
                d2 = __uint_as_float((unsigned)(k2 >> 32));
    const int i0 = (int)(unsigned)k0, i1 = (int)(unsigned)k1, i2 = (int)(unsigned)k2;
#ifdef SN2_NN_STAMPS
    {
        unsigned long long t_end;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_end)::"memory");
        const int wid = (b * gx + bx) * 4 + (threadIdx.x >> 6);
        if (lane == 0 && wid < 16384) {
            g_nn_dbg[4 * wid + 0] = t_end - t_begin;
            g_nn_dbg[4 * wid + 1] = n_cand;
            g_nn_dbg[4 * wid + 2] = rho_last;
            g_nn_dbg[4 * wid + 3] = (unsigned long long)((bx1 - bx0 + 1) * (by1 - by0 + 1));
        }
    }
#endif
    if (!valid) return;
    const int t = dst_order[(size_t)b * T + p];
    const size_t o = ((size_t)b * T + t) * 3;
    const bool u1 = (k >= 2) && (i1 != 0x7FFFFFFF), u2 = (k >= 3) && (i2 != 0x7FFFFFFF);
    const int j1 = u1 ? i1 : i0, j2 = u2 ? i2 : i0;
    const float w0 = 1.0f / fmaxf(d0, 1e-16f), w1 = u1 ? 1.0f / fmaxf(d1, 1e-16f) : 0.f, w2 = u2 ? 1.0f / fmaxf(d2, 1e-16f) : 0.f;
    idx[o + 0] = i0;
    idx[o + 1] = j1;
    idx[o + 2] = j2;
    w[o + 0] = w0;
    w[o + 1] = w1;
    w[o + 2] = w2;
    // the same row once more at its SORTED position (sn2_three_nn_xy_copy): 24 bytes per lane, contiguous across the wave --
    // the table in the order the inverted index is built in (interp_index.hip)
    if (idx_sorted) {
        const size_t q = ((size_t)b * T + p) * 3;
        idx_sorted[q + 0] = i0;
        idx_sorted[q + 1] = j1;
        idx_sorted[q + 2] = j2;
        w_sorted[q + 0] = w0;
        w_sorted[q + 1] = w1;
        w_sorted[q + 2] = w2;
    }
}

// The targets of a plot in the order of the SOURCE grid's cells (rows of cells walked in a snake, so that consecutive cells
// are always neighbours): counting sort in LDS, one workgroup per plot.  A wave of three_nn_grid_kernel then holds 64
// targets of one or two adjacent cells -- a 1-2 cell query box for every wave.  (In the order sn2_fps leaves, a 3-D
// Morton order of a 16^3 grid, the boxes averaged 7 cells and reached 72: 162 candidates per wave on average, 726 in
// the slowest, and the slowest wave is the kernel.)  The order inside a cell is whatever the cursor atomics give: the
// search is exact, so its results do not depend on it.
// U loads per coordinate in flight (a loop of one point per thread and trip spends a trip of dependent loads per point and
// pass: 54 us at T = 32 768).  A target below the sources' box on an axis (vx < 0) goes to the first cell of that axis.
template <int U, int NT>
__global__ __launch_bounds__(NT) void nn_target_sort_chunk_kernel(const float* __restrict__ dst, int T, const int* __restrict__ hdr,
                                                                    int* __restrict__ order, float4* __restrict__ sorted) {
    __shared__ int s_hist[NN_GMAX * NN_GMAX];
    __shared__ int s_wsum[NT / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* dx = dst + (size_t)b * 3 * T;
    const float* dy = dx + T;
    const float* dz = dy + T;
    const int* hb = hdr + (size_t)b * NN_HDR;
    const int G = hb[NN_GMAX * NN_GMAX + 1 + 5];
    const float* hf = reinterpret_cast<const float*>(hb + NN_GMAX * NN_GMAX + 1);
    const float x0 = hf[0], y0 = hf[1], ix = hf[2], iy = hf[3];
    auto key_of = [&](float px_, float py_) {
        const float vx = px_ - x0, vy = py_ - y0;
        int cx = (int)(vx * ix), cy = (int)(vy * iy);
        cx = (vx < 0.f || cx < 0) ? 0 : (cx > G - 1 ? G - 1 : cx);
        cy = (vy < 0.f || cy < 0) ? 0 : (cy > G - 1 ? G - 1 : cy);
        return cy * G + ((cy & 1) ? G - 1 - cx : cx);
    };
    for (int i = tid; i < G * G; i += NT) s_hist[i] = 0;
    __syncthreads();
    // (plot_sort.h's loader written out: through it the 256-thread form measured 3 % slower, profiles/plot_sort)
    for (int i0 = 0; i0 < T; i0 += NT * U) {
        float vx[U], vy[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * NT + tid, ii = i < T ? i : T - 1;
            vx[u] = dx[ii]; vy[u] = dy[ii];
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (i0 + u * NT + tid < T) atomicAdd(&s_hist[key_of(vx[u], vy[u])], 1);
    }
    __syncthreads();
    block_scan_cells<NT, NN_GMAX * NN_GMAX, false>(s_hist, G * G, s_wsum, [](int, int) {});
    int* ob = order + (size_t)b * T;
    float4* sb = sorted + (size_t)b * T;
    for (int i0 = 0; i0 < T; i0 += NT * U) {
        float vx[U], vy[U], vz[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * NT + tid, ii = i < T ? i : T - 1;
            vx[u] = dx[ii]; vy[u] = dy[ii]; vz[u] = dz[ii];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * NT + tid;
            if (i < T) {
                const int p = atomicAdd(&s_hist[key_of(vx[u], vy[u])], 1);
                ob[p] = i;
                sb[p] = make_float4(vx[u], vy[u], vz[u], 0.f);
            }
        }
    }
}

static bool nn_grid_sources(int S) { return S >= 128 && S <= 8192; }      // what the per-plot x,y grid of three_nn_grid_kernel holds in LDS
extern "C" int sn2_three_nn_uses_grid(int S, int T) { return nn_grid_sources(S) && T > 2048; }
extern "C" size_t sn2_three_nn_ws_words(int B, int S) { return SN2_THREE_NN_WS_WORDS(B, S); }
extern "C" size_t sn2_three_nn_xy_ws_words(int B, int S, int T) { return SN2_THREE_NN_XY_WS_WORDS(B, S, T); }

// the workspace of sn2_three_nn_xy, in 32-bit words:  tbl [4 B S] | sorted [4 B T] | hdr [B NN_HDR] | order [B T] |
// idx_sorted [3 B T] | w_sorted [3 B T]
static_assert(NN_HDR == 1032, "SN2_THREE_NN_XY_WS_WORDS counts 1032 header words per plot");
extern "C" int sn2_three_nn_xy_order_offset(int B, int S, int T, size_t* order_words, size_t* copy_words) {
    if (B <= 0 || S <= 0 || T <= 0 || !order_words) return SN2_EINVAL;
    *order_words = (size_t)B * (4 * (size_t)S + 4 * (size_t)T + NN_HDR);
    if (copy_words) *copy_words = *order_words + (size_t)B * T;
    return 0;
}

extern "C" int sn2_three_nn_xy_copy(const float* src_soa, int B, int S, const float* dst_soa, int T, int k, int* idx, float* w,
                                    void* ws, int sorted_copy, void* stream) {
    if (!src_soa || !dst_soa || !idx || !w || !ws || B <= 0 || S <= 0 || T <= 0 || k < 1 || k > 3) return SN2_EINVAL;
    if (!nn_grid_sources(S) || (((size_t)ws) % 16) != 0) return SN2_ELIMIT;
    hipStream_t st = (hipStream_t)stream;
    int G = (int)sqrtf((float)S / 4.f);   // about 4 sources per cell
    G = G < 2 ? 2 : (G > NN_GMAX ? NN_GMAX : G);
    float4* tbl = reinterpret_cast<float4*>(ws);
    float4* sorted = tbl + (size_t)B * S;
    int* hdr = reinterpret_cast<int*>(sorted + (size_t)B * T);
    int* order = hdr + (size_t)B * NN_HDR;
    int* idx_sorted = sorted_copy ? order + (size_t)B * T : nullptr;
    float* w_sorted = sorted_copy ? reinterpret_cast<float*>(idx_sorted + (size_t)3 * B * T) : nullptr;
    hipLaunchKernelGGL(nn_grid_build_kernel, dim3(B), dim3(256), 0, st, src_soa, S, G, tbl, hdr);
    if (sn2_small_sort_wg(B) && T <= 16 * 1024)        // many plots: 256 threads per plot (common.h)
        hipLaunchKernelGGL((nn_target_sort_chunk_kernel<16, 256>), dim3(B), dim3(256), 0, st, dst_soa, T, (const int*)hdr, order, sorted);
    else if (T <= 8 * 1024)
        hipLaunchKernelGGL((nn_target_sort_chunk_kernel<8, 1024>), dim3(B), dim3(1024), 0, st, dst_soa, T, (const int*)hdr, order, sorted);
    else
        hipLaunchKernelGGL((nn_target_sort_chunk_kernel<16, 1024>), dim3(B), dim3(1024), 0, st, dst_soa, T, (const int*)hdr, order, sorted);
    const size_t lds = (size_t)S * 16 + (size_t)(G * G + 1) * 4;
    if (lds > 48 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&three_nn_grid_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    {
        const int gx = sn2_cdiv(T, 256);
        static const bool no_xcd = getenv("SN2_NN_NO_XCD") != nullptr;      // (diagnostic switch)
        if (!no_xcd && (B % 8 == 0 || B >= 64))      // plots balance over the XCDs: XCD-aware placement
            hipLaunchKernelGGL(three_nn_grid_kernel, dim3(8 * sn2_cdiv(B, 8) * gx), dim3(256), lds, st, (const float4*)tbl,
                               (const int*)hdr, S, T, k, (const int*)order, (const float4*)sorted, idx, w, B, gx, idx_sorted,
                               w_sorted);
        else
            hipLaunchKernelGGL(three_nn_grid_kernel, dim3(gx, B), dim3(256), lds, st, (const float4*)tbl,
                               (const int*)hdr, S, T, k, (const int*)order, (const float4*)sorted, idx, w, 0, gx, idx_sorted,
                               w_sorted);
    }
    SN2_RETURN_LAUNCH();
}

extern "C" int sn2_three_nn_xy(const float* src_soa, int B, int S, const float* dst_soa, int T, int k, int* idx, float* w,
                               void* ws, void* stream) {
    return sn2_three_nn_xy_copy(src_soa, B, S, dst_soa, T, k, idx, w, ws, 0, stream);
}

extern "C" int sn2_three_nn(const float* src_soa, int B, int S, const float* dst_soa, int T, int k, int* idx, float* w,
                            void* ws, const int* dst_fps_ws, void* stream) {
    if (!src_soa || !dst_soa || !idx || !w || B <= 0 || S <= 0 || T <= 0 || k < 1 || k > 3) return SN2_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    // grid search: needs the targets in the spatial order sn2_fps built for them (workspace laid out as there)
    if (ws && dst_fps_ws && sn2_three_nn_uses_grid(S, T) && (((size_t)B * T) % 4 == 0) && (((size_t)ws) % 16 == 0)) {
        int G = (int)sqrtf((float)S / 4.f);   // about 4 sources per cell (2, 3, 8 and 12 per cell measured slower)
        G = G < 2 ? 2 : (G > NN_GMAX ? NN_GMAX : G);
        float4* tbl = reinterpret_cast<float4*>(ws);
        int* hdr = reinterpret_cast<int*>(tbl + (size_t)B * S);
        hipLaunchKernelGGL(nn_grid_build_kernel, dim3(B), dim3(256), 0, st, src_soa, S, G, tbl, hdr);
        const size_t lds = (size_t)S * 16 + (size_t)(G * G + 1) * 4;
        if (lds > 48 * 1024)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&three_nn_grid_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(three_nn_grid_kernel, dim3(sn2_cdiv(T, 256), B), dim3(256), lds, st, (const float4*)tbl,
                           (const int*)hdr, S, T, k, dst_fps_ws, reinterpret_cast<const float4*>(dst_fps_ws + (size_t)B * T),
                           idx, w, 0, sn2_cdiv(T, 256), (int*)nullptr, (float*)nullptr);
        SN2_RETURN_LAUNCH();
    }
    dim3 grid(sn2_cdiv(T, 256), B);
    hipLaunchKernelGGL(three_nn_kernel, grid, dim3(256), 0, st, src_soa, S, dst_soa, T, k, idx, w);
    SN2_RETURN_LAUNCH();
}
