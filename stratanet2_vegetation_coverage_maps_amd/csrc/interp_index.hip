// interp_index.hip -- the inverted interpolation index: from a 3-NN table (target row -> three sources and weights) to the
// lists source -> (target row, normalised weight), which the backward kernels of fp.hip walk.  Kernels inv_hist / inv_scan /
// inv_fill / inv_order, their launcher build_interp_index and the entry points sn2_interp_index, sn2_interp_index_perm,
// sn2_interp_index_group, sn2_interp_index_ordered.  The host view of the workspace (InterpIndex / carve_interp_index) and the slice and chunk sizes
// are in fp_rows.h.
//
// ---------------------------------------------------------------------------------------------- backward (3) of fp.hip
// Transpose of the interpolation:  dsrc[s][k] += sum over (target r, slot j) with idx_j(r) = s of (w_j / sum w) * du[r][k].
// Done as a GATHER through an inverted index (source -> list of (row, weight)), built per call from the saved 3-NN table:
//   A  per (plot, row slice): histogram of the slice's source ids in LDS (integer atomics on 4 KB) -> H[plot][slice][s]
//   B  per plot: exclusive prefix over the slices of every source and over the sources -> list offsets
//   C  per (plot, row slice): LDS cursors -> (row, normalised weight) entries at their final positions
//   D  one wave per source row, lane = channel: coalesced du rows, accumulation in registers, one plain store
//      (interp_gather_kernel and the source pass of the source-side form, both in fp.hip).
// No floating-point atomics anywhere (LDS float atomics ran at ~0.4 lane-ops/clk/CU here: 275 us for FP1; global float
// atomics onto random rows are worse), and dsrc is written exactly once per row.
#include "fp_rows.h"
#include "plot_sort.h"

namespace {

// The workspace of ONE batch's inverted index (SN2_INTERP_WS_WORDS(B, Rp, S) 32-bit words), carved the same way on the host
// (carve_interp_index, fp_rows.h) and inside the kernels that build it:
//   H [B*SL*S] | off [B*S] | cnt [B*S] | inv_row [3*B*Rp] | inv_w [3*B*Rp] | (16-byte aligned) items [B*S] int4 | chunks [B*CM] int4
// GROUPED builds (round 5: sn2_interp_index_group): one launch covers G consecutive batches of B plots each -- plot bg of the
// launch is plot bg % B of batch bg / B, whose workspace starts ws_stride words behind the previous batch's -- so that the
// position-only pass of a pipelined loop, which samples eight batches in one FPS launch, builds their inverted indices in 12
// launches instead of 96.  Every batch's workspace is an ordinary B-plot workspace: its consumers do not change.
struct InvWs {
    int *H, *off, *cnt, *inv_row;
    float* inv_w;
    int4 *items, *chunks;
};
__host__ __device__ __forceinline__ InvWs inv_ws_of(float* ws, int B, int Rp, int S) {
    const int SL = (Rp + INV_SLICE_ROWS - 1) / INV_SLICE_ROWS;
    InvWs x;
    x.H = reinterpret_cast<int*>(ws);
    x.off = x.H + (size_t)B * SL * S;
    x.cnt = x.off + (size_t)B * S;
    x.inv_row = x.cnt + (size_t)B * S;
    x.inv_w = reinterpret_cast<float*>(x.inv_row + (size_t)3 * B * Rp);
    x.items = reinterpret_cast<int4*>((reinterpret_cast<uintptr_t>(x.inv_w + (size_t)3 * B * Rp) + 15) & ~(uintptr_t)15);
    x.chunks = x.items + (size_t)B * S;
    return x;
}

// Where a workgroup of inv_hist / inv_fill works.  GB = 0: the grid is (SL, plots).  GB > 0 (plots that balance over the XCDs,
// the rule of three_nn_grid_kernel): the grid is one-dimensional, workgroup w = (XCD w & 7, turn w >> 3), and all SL slices
// of plot bg run on XCD bg % 8 -- the slices of a plot write into ONE list area (3 R entries of 4 + 4 bytes), and only
// workgroups behind the same L2 fill its lines there before they are written back.  false: nothing to do.
__device__ __forceinline__ bool inv_place(int SL, int GB, int& bg, int& sl) {
    if (GB == 0) {
        bg = blockIdx.y, sl = blockIdx.x;
        return true;
    }
    const int turn = (int)(blockIdx.x >> 3);
    bg = (int)(blockIdx.x & 7u) + 8 * (turn / SL);
    sl = turn % SL;
    return bg < GB;
}

// THE ORDER OF THE WALK.  Slice sl covers positions [INV_SLICE_ROWS sl, INV_SLICE_ROWS (sl + 1)) of the plot; position p is
// row row_order[p] (row_order == nullptr: row p).  With the order the 3-NN search sorted its targets in (sn2_three_nn_xy:
// by the cells of the source grid) a slice names about a hundred sources instead of all of them, a list receives its
// entries from the two or three slices around its source, and every slice writes ONE contiguous run of it: whole lines
// from one workgroup.  In the targets' own order every entry is a 4-byte store to a place of its own.
// The table row of position p is read at p (by_row == 0: knn_idx / knn_w are the search's sorted copy, or there is no
// order) or at row_order[p] (by_row != 0: a gather from the table in row order).
__global__ __launch_bounds__(1024) void inv_hist_kernel(int R_per_plot, int S, const int* __restrict__ knn_idx,
                                                        const float* __restrict__ knn_w, float* __restrict__ ws, int Bb,
                                                        size_t ws_stride, int SL, int GB, const int* __restrict__ row_order) {
    extern __shared__ int s_hist[];
    int bg, sl;
    if (!inv_place(SL, GB, bg, sl)) return;
    const int hb = bg / Bb, b = bg - hb * Bb;                    // batch of the group, plot of the batch
    int* H = inv_ws_of(ws + (size_t)hb * ws_stride, Bb, R_per_plot, S).H;
    for (int i = threadIdx.x; i < S; i += 1024) s_hist[i] = 0;
    __syncthreads();
    const int r_lo = sl * INV_SLICE_ROWS, r_hi = min(R_per_plot, r_lo + INV_SLICE_ROWS);
    for (int rl = r_lo + threadIdx.x; rl < r_hi; rl += 1024) {
        const size_t r = (size_t)bg * R_per_plot + (row_order ? row_order[(size_t)bg * R_per_plot + rl] : rl);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (j == 0 || knn_w[r * 3 + j] != 0.f) atomicAdd(&s_hist[knn_idx[r * 3 + j]], 1);
    }
    __syncthreads();
    int* out = H + ((size_t)b * SL + sl) * S;
    for (int i = threadIdx.x; i < S; i += 1024) out[i] = s_hist[i];
}

// H[plot][slice][s] -> exclusive prefix over slices (in place);  off[plot*S + s] = plot*3*R + exclusive scan of the totals;
// cnt[plot*S + s] = total
__global__ __launch_bounds__(1024) void inv_scan_kernel(int R_per_plot, int S, int SL, float* __restrict__ ws, int Bb,
                                                        size_t ws_stride) {
    __shared__ int s_w[16];
    __shared__ int s_carry;
    const int bg = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int hb = bg / Bb, b = bg - hb * Bb;
    const InvWs x = inv_ws_of(ws + (size_t)hb * ws_stride, Bb, R_per_plot, S);
    int* __restrict__ H = x.H;
    int* __restrict__ off = x.off;
    int* __restrict__ cnt = x.cnt;
    if (threadIdx.x == 0) s_carry = b * 3 * R_per_plot;
    __syncthreads();
    // (block_scan_excl of plot_sort.h written out: through the function this kernel measured 3 % slower, profiles/plot_sort)
    for (int s0 = 0; s0 < S; s0 += 1024) {
        const int s = s0 + threadIdx.x;
        int tot = 0;
        if (s < S) {
            for (int sl = 0; sl < SL; ++sl) {
                int* h = H + ((size_t)b * SL + sl) * S + s;
                const int t = *h;
                *h = tot;
                tot += t;
            }
            cnt[(size_t)b * S + s] = tot;
        }
        const int incl = wave_scan_incl(tot);
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        int base = s_carry;
        for (int k = 0; k < wave; ++k) base += s_w[k];
        if (s < S) off[(size_t)b * S + s] = base + incl - tot;
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = base + incl;
        __syncthreads();
    }
}

__global__ __launch_bounds__(1024) void inv_fill_kernel(int R_per_plot, int S, const int* __restrict__ knn_idx,
                                                        const float* __restrict__ knn_w, float* __restrict__ ws, int Bb,
                                                        size_t ws_stride, const int* __restrict__ row_perm, int SL, int GB,
                                                        const int* __restrict__ row_order, int by_row) {
    extern __shared__ int s_cur[];
    int bg, sl;
    if (!inv_place(SL, GB, bg, sl)) return;
    const int hb = bg / Bb, b = bg - hb * Bb;
    const InvWs x = inv_ws_of(ws + (size_t)hb * ws_stride, Bb, R_per_plot, S);
    const int* __restrict__ H = x.H;
    const int* __restrict__ off = x.off;
    int* __restrict__ inv_row = x.inv_row;
    float* __restrict__ inv_w = x.inv_w;
    const int* hp = H + ((size_t)b * SL + sl) * S;
    for (int i = threadIdx.x; i < S; i += 1024) s_cur[i] = off[(size_t)b * S + i] + hp[i];
    __syncthreads();
    const int r_lo = sl * INV_SLICE_ROWS, r_hi = min(R_per_plot, r_lo + INV_SLICE_ROWS);
    for (int rl = r_lo + threadIdx.x; rl < r_hi; rl += 1024) {
        const size_t r0 = (size_t)bg * R_per_plot;
        const int row = row_order ? row_order[r0 + rl] : rl;
        const size_t r = r0 + (by_row ? row : rl);
        const float w0 = knn_w[r * 3 + 0], w1 = knn_w[r * 3 + 1], w2 = knn_w[r * 3 + 2];
        const float inv = 1.0f / ((w0 + w1) + w2);
        const float w[3] = {w0, w1, w2};
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (j == 0 || w[j] != 0.f) {
                const int p = atomicAdd(&s_cur[knn_idx[r * 3 + j]], 1);
                inv_row[p] = row_perm ? row_perm[r0 + row] : row;  // where the row's d pre-activation is kept (sn2_fp.row_perm)
                inv_w[p] = w[j] * inv;
            }
    }
}

// E  the plot's sources along a Morton curve (identity without positions): items[plot*S + rank] = {source id, list offset,
//    list length, -}: one load tells a wave of the source-side kernel all about its source.  The source-side kernels walk
//    the sources in this order, one contiguous stretch of it per XCD, so that the target rows shared by neighbouring
//    sources (every target row is on the lists of its three nearest sources) are fetched into that XCD's L2 once.
//    Keys: 10 bits per axis inside the plot's bounding box; ranks by comparison counting in LDS (ties by id).
__device__ __forceinline__ unsigned spread10(unsigned v) {
    v &= 1023u;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
//    F  the lists cut into CHUNKS of at most INV_CHUNK (fp_rows.h) entries, in the same order: chunks[plot*CM + j] = {source id, offset of
//    the chunk's first entry, its length, plot}, CM = inv_chunks_per_plot (unused slots: length 0), and items[].w = the plot-local
//    number of the source's first chunk.  The lists are anything but even (C2: median 25 entries, a tenth of the sources
//    500-800: the synthetic stands are clumped like real ones), and a wave per SOURCE left the source pass waiting for a few
//    waves that walk 13 chunks one after the other; a wave per CHUNK has one short chain for everybody.

__global__ __launch_bounds__(1024) void inv_order_kernel(const float4* __restrict__ pos, int S, int CM, int R_per_plot,
                                                         float* __restrict__ ws, int Bb, size_t ws_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned s_key[];   // [S rounded up to 4] keys | [S] source of every rank
    __shared__ float s_mm[6][16];
    __shared__ int s_w[16];
    const int bg = blockIdx.x;
    const int hb = bg / Bb, b = bg - hb * Bb;
    const InvWs x = inv_ws_of(ws + (size_t)hb * ws_stride, Bb, R_per_plot, S);
    const int* __restrict__ off = x.off;
    const int* __restrict__ cnt = x.cnt;
    int4* __restrict__ items = x.items;
    int4* __restrict__ chunks = x.chunks;
    const float4* pb = pos + (size_t)bg * S;
    const int S4 = (S + 3) & ~3;
    int* s_ord = reinterpret_cast<int*>(s_key + S4);
    if (pos) {
        float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
        for (int i = threadIdx.x; i < S; i += 1024) {
            const float4 p = pb[i];
            lo[0] = fminf(lo[0], p.x), lo[1] = fminf(lo[1], p.y), lo[2] = fminf(lo[2], p.z);
            hi[0] = fmaxf(hi[0], p.x), hi[1] = fmaxf(hi[1], p.y), hi[2] = fmaxf(hi[2], p.z);
        }
        block_minmax<1024, 3>(lo, hi, s_mm);
        float sc[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) sc[a] = hi[a] > lo[a] ? 1023.999f / (hi[a] - lo[a]) : 0.f;
        for (int i = threadIdx.x; i < S4; i += 1024) {
            unsigned key = 0xFFFFFFFFu;                                    // padding sorts last
            if (i < S) {
                const float4 p = pb[i];
                const unsigned qx = (unsigned)((p.x - lo[0]) * sc[0]), qy = (unsigned)((p.y - lo[1]) * sc[1]),
                               qz = (unsigned)((p.z - lo[2]) * sc[2]);
                key = spread10(qx) | (spread10(qy) << 1) | (spread10(qz) << 2);
            }
            s_key[i] = key;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < S; i += 1024) {
            const unsigned mine = s_key[i];
            int rank = 0;
            for (int j = 0; j < S4; j += 4) {
                const uint4 o = *reinterpret_cast<const uint4*>(&s_key[j]);
                rank += (o.x < mine || (o.x == mine && j < i)) ? 1 : 0;
                rank += (o.y < mine || (o.y == mine && j + 1 < i)) ? 1 : 0;
                rank += (o.z < mine || (o.z == mine && j + 2 < i)) ? 1 : 0;
                rank += (o.w < mine || (o.w == mine && j + 3 < i)) ? 1 : 0;
            }
            s_ord[rank] = i;
        }
    } else {                                                           // no positions: identity
        for (int i = threadIdx.x; i < S; i += 1024) s_ord[i] = i;
    }
    __syncthreads();
    int carry = 0;                                                     // chunks so far
    for (int k0 = 0; k0 < S; k0 += 1024) {
        const int k = k0 + threadIdx.x;
        int id = 0, o = 0, n = 0, nch = 0;
        if (k < S) {
            id = b * S + s_ord[k];
            o = off[id], n = cnt[id];
            nch = (n + INV_CHUNK - 1) / INV_CHUNK;
        }
        int next;
        const int first = block_scan_excl<1024>(nch, s_w, carry, next);
        if (k < S) {
            items[(size_t)b * S + k] = make_int4(id, o, n, first);
            for (int c = 0; c < nch; ++c)
                chunks[(size_t)b * CM + first + c] = make_int4(id, o + c * INV_CHUNK, min(INV_CHUNK, n - c * INV_CHUNK), b);
        }
        carry = next;
    }
    for (int j = carry + threadIdx.x; j < CM; j += 1024) chunks[(size_t)b * CM + j] = make_int4(0, 0, 0, 0);
}

}  // namespace

int build_interp_index(const int* knn_idx, const float* knn_w, const float* src_pos, int B, int Rp, int S, float* ws,
                       hipStream_t st, const int* row_perm, int G, size_t ws_stride, const int* row_order, const int* idx_sorted,
                       const float* w_sorted) {
    if (S > 8192) return SN2_ELIMIT;
    if (G < 1 || (G > 1 && (ws_stride & 3))) return SN2_EINVAL;           // (every batch's workspace 16-byte aligned)
    const int SL = sn2_cdiv(Rp, INV_SLICE_ROWS);
    const int CM = inv_chunks_per_plot(Rp, S);
    if ((long)G * B >= 65535) return SN2_ELIMIT;                           // grid.y
    // (diagnostic switches, so that the parts can be timed apart: SN2_INV_NO_XCD keeps the two-dimensional grid, SN2_INV_NO_ORDER
    // walks the rows in their own order whatever the caller hands in, SN2_INV_GATHER reads the table in row order through
    // row_order although the search left its sorted copy)
    static const bool no_xcd = getenv("SN2_INV_NO_XCD") != nullptr, gather = getenv("SN2_INV_GATHER") != nullptr;
    static const bool no_order = getenv("SN2_INV_NO_ORDER") != nullptr;
    if (no_order) row_order = nullptr;
    const int GB = G * B;
    // plots balance over the XCDs: the rule of sn2_three_nn_xy (one slice per plot: the two grids place alike, the plain one stays)
    const bool xcd = !no_xcd && SL > 1 && (GB % 8 == 0 || GB >= 64);
    const dim3 grid = xcd ? dim3(8 * sn2_cdiv(GB, 8) * SL) : dim3(SL, GB);
    const bool copy = row_order && idx_sorted && w_sorted && !gather;
    const int* t_idx = copy ? idx_sorted : knn_idx;
    const float* t_w = copy ? w_sorted : knn_w;
    hipLaunchKernelGGL(inv_hist_kernel, grid, dim3(1024), (size_t)S * 4, st, Rp, S, t_idx, t_w, ws, B, ws_stride, SL, xcd ? GB : 0,
                       copy ? nullptr : row_order);              // (a slice of the copy needs no row numbers to be counted)
    hipLaunchKernelGGL(inv_scan_kernel, dim3(G * B), dim3(1024), 0, st, Rp, S, SL, ws, B, ws_stride);
    hipLaunchKernelGGL(inv_fill_kernel, grid, dim3(1024), (size_t)S * 4, st, Rp, S, t_idx, t_w, ws, B, ws_stride, row_perm, SL,
                       xcd ? GB : 0, row_order, (row_order && !copy) ? 1 : 0);
    // keys + the source of every rank: 64 KB of dynamic LDS at the S = 8192 limit (+ ~450 B static): above the 48 KB a kernel
    // gets without asking
    const size_t order_lds = (size_t)(((S + 3) & ~3) + S) * 4;
    if (order_lds > 48 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&inv_order_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)order_lds);
    hipLaunchKernelGGL(inv_order_kernel, dim3(G * B), dim3(1024), order_lds, st, reinterpret_cast<const float4*>(src_pos), S, CM, Rp,
                       ws, B, ws_stride);
    SN2_RETURN_LAUNCH();
}

extern "C" size_t sn2_interp_chunks(int R_per_plot, int S_per_plot) { return SN2_INTERP_CHUNKS(R_per_plot, S_per_plot); }
extern "C" size_t sn2_interp_ws_words(int B, int R_per_plot, int S_per_plot) { return SN2_INTERP_WS_WORDS(B, R_per_plot, S_per_plot); }

extern "C" int sn2_interp_index(const int* knn_idx, const float* knn_w, const float* src_pos, int B, int R_per_plot,
                                int S_per_plot, float* ws, void* stream) {
    if (!knn_idx || !knn_w || !ws || B <= 0 || R_per_plot <= 0 || S_per_plot <= 0) return SN2_EINVAL;
    return build_interp_index(knn_idx, knn_w, src_pos, B, R_per_plot, S_per_plot, ws, (hipStream_t)stream);
}

extern "C" int sn2_interp_index_perm(const int* knn_idx, const float* knn_w, const float* src_pos, const int* row_perm, int B,
                                     int R_per_plot, int S_per_plot, float* ws, void* stream) {
    if (!knn_idx || !knn_w || !ws || B <= 0 || R_per_plot <= 0 || S_per_plot <= 0) return SN2_EINVAL;
    return build_interp_index(knn_idx, knn_w, src_pos, B, R_per_plot, S_per_plot, ws, (hipStream_t)stream, row_perm);
}

extern "C" int sn2_interp_index_group(const int* knn_idx, const float* knn_w, const float* src_pos, const int* row_perm, int G, int B,
                                      int R_per_plot, int S_per_plot, float* ws, size_t ws_stride_words, void* stream) {
    if (!knn_idx || !knn_w || !ws || G <= 0 || B <= 0 || R_per_plot <= 0 || S_per_plot <= 0) return SN2_EINVAL;
    if (G > 1 && ws_stride_words < SN2_INTERP_WS_WORDS(B, R_per_plot, S_per_plot)) return SN2_EINVAL;
    return build_interp_index(knn_idx, knn_w, src_pos, B, R_per_plot, S_per_plot, ws, (hipStream_t)stream, row_perm, G, ws_stride_words);
}

extern "C" int sn2_interp_index_ordered(const int* knn_idx, const float* knn_w, const float* src_pos, const int* row_perm,
                                        const int* row_order, const int* idx_sorted, const float* w_sorted, int G, int B,
                                        int R_per_plot, int S_per_plot, float* ws, size_t ws_stride_words, void* stream) {
    if (!knn_idx || !knn_w || !ws || G <= 0 || B <= 0 || R_per_plot <= 0 || S_per_plot <= 0) return SN2_EINVAL;
    if (G > 1 && ws_stride_words < SN2_INTERP_WS_WORDS(B, R_per_plot, S_per_plot)) return SN2_EINVAL;
    if ((idx_sorted != nullptr) != (w_sorted != nullptr) || (idx_sorted && !row_order)) return SN2_EINVAL;
    return build_interp_index(knn_idx, knn_w, src_pos, B, R_per_plot, S_per_plot, ws, (hipStream_t)stream, row_perm, G, ws_stride_words,
                              row_order, idx_sorted, w_sorted);
}
