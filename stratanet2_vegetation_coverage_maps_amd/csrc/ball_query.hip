// ball_query.hip -- radius ball query: the full scan, the grid form over the tables sn2_fps left (fps_ws.h), and the sum of
// the neighbour counts.  Entry points sn2_ball_query, sn2_count_sum, sn2_count_sum_group.
// All discrete decisions use the canonical fp32 squared distance sn2_d2 (common.h) so that the index structures
// are bit-identical to the oracle's.
#include "common.h"
#include "plot_sort.h"
#include "fps_ws.h"
#include <stdlib.h>

// ------------------------------------------------------------------------------------------------------------
// ball_query: one wave owns TC centroids of one plot (coordinates and running counts wave-uniform -> SGPRs) and
// streams the plot's points 64 at a time (coalesced SoA loads, L2-resident after the first wave); per centroid a
// ballot + prefix popcount compacts the hits, so each list comes out in ascending source index and the stores of
// one wave-instruction are contiguous.  Algorithmic HBM bytes: 12*(N+M) read + 4*E + 4*M written per plot.
// ------------------------------------------------------------------------------------------------------------
template <int TC>
__global__ __launch_bounds__(256) void ball_query_kernel(const float* __restrict__ src, int B, int N,
                                                         const float* __restrict__ cpos, int M, float r2, int cap,
                                                         int* __restrict__ nbr, int* __restrict__ cnt,
                                                         unsigned long long* __restrict__ total, int tiles_per_plot) {
    const int lane = threadIdx.x & 63;
    const int wg = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * 256 + threadIdx.x) >> 6));
    const int b = wg / tiles_per_plot;
    if (b >= B) return;
    const int c0 = (wg - b * tiles_per_plot) * TC;
    const float* px = src + (size_t)b * 3 * N;
    const float* py = px + N;
    const float* pz = py + N;
    float cx[TC], cy[TC], cz[TC];
    int n[TC];
#pragma unroll
    for (int t = 0; t < TC; ++t) {
        const int ci = (c0 + t < M) ? c0 + t : M - 1;
        cx[t] = cpos[((size_t)b * 3 + 0) * M + ci];
        cy[t] = cpos[((size_t)b * 3 + 1) * M + ci];
        cz[t] = cpos[((size_t)b * 3 + 2) * M + ci];
        n[t] = 0;
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int j0 = 0; j0 < N; j0 += 64) {
        const int j = j0 + lane;
        const bool valid = j < N;
        const float x = valid ? px[j] : 0.f, y = valid ? py[j] : 0.f, z = valid ? pz[j] : 0.f;
#pragma unroll
        for (int t = 0; t < TC; ++t) {
            const bool hit = valid && (sn2_d2(x, y, z, cx[t], cy[t], cz[t]) < r2);
            const unsigned long long mask = __ballot(hit);
            if (mask) {
                const int p = n[t] + __popcll(mask & below);
                if (hit && p < cap && c0 + t < M) nbr[((size_t)b * M + c0 + t) * cap + p] = j;
                n[t] += __popcll(mask);
            }
        }
    }
    unsigned long long sum = 0;
#pragma unroll
    for (int t = 0; t < TC; ++t) {
        const int c = n[t] < cap ? n[t] : cap;
        if (c0 + t < M) {
            if (lane == 0) cnt[(size_t)b * M + c0 + t] = c;
            sum += (unsigned long long)c;
        }
    }
    (void)sum;
    (void)total;
}

// ------------------------------------------------------------------------------------------------------------
// Grid ball query (exact): the sources were already sorted into 16^3 Morton cells by spatial_order_chunk_kernel (FPS level 1
// runs on the same points).  One wave per centroid walks only the cells that can intersect the ball -- the cell range of
// [c - r, c + r] per axis under the same monotone fp32 cell function, so no point with d2 < r2 is missed --, tests the
// cells' points with the canonical sn2_d2, compacts the hits into a wave-private LDS list, rank-sorts them by ORIGINAL
// index (the contract: ascending source index, first `cap` kept) and writes the list.  ~200 candidates per centroid
// instead of 32 768.  A ball with more hits than the LDS list (GQ_LIST) falls back to the full scan for that centroid.
// ------------------------------------------------------------------------------------------------------------
constexpr int GQ_LIST = 512;
#ifndef SN2_GQ_DENSE
#define SN2_GQ_DENSE 512
#endif
constexpr int GQ_DENSE = SN2_GQ_DENSE;   // hits beyond which the bitmap path takes over from the rank sort (measured: switching at 192
                                         // instead of 512 made the query slower at both sizes, 0.30 vs 0.26 ms at 8 x 131 072, 0.075 vs 0.054 at 16 x 32 768)
static_assert(GQ_DENSE <= GQ_LIST, "the list holds the sparse balls");
#ifndef SN2_GQ_BM_CAND
#define SN2_GQ_BM_CAND 160
#endif
constexpr int GQ_BM_WORDS = 512, GQ_BM_CAND = SN2_GQ_BM_CAND;   // bitmap first: plots of <= 16 384 points, more candidates than this

__global__ __launch_bounds__(256) void ball_query_grid_kernel(const float* __restrict__ src, int B, int N,
                                                              const float* __restrict__ cpos, int M, float r, float r2,
                                                              int cap, const int* __restrict__ order,
                                                              const float4* __restrict__ sorted, const int* __restrict__ grid,
                                                              int* __restrict__ nbr, int* __restrict__ cnt,
                                                              unsigned long long* __restrict__ total, int xcd_aware) {
    __shared__ int s_list[4][GQ_LIST];
    extern __shared__ unsigned gq_bits[];              // [4][(N + 31) / 32]: one bit per source point, per wave (dense balls)
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    // XCD-aware placement (round 4): workgroups go to the eight XCDs round-robin, and every XCD has its own L2 -- with the
    // centroids dealt out in index order all eight L2s fetched every plot's sorted table (PMC: 5.2 x the compulsory bytes at
    // 16 x 32 768).  Plot b is worked on by the workgroups of XCD b % 8 only: workgroup w = (XCD w & 7, turn w >> 3), the turns
    // of an XCD walk its plots one after the other, (M + 3) / 4 workgroups of four centroids per plot.
    // (xcd_aware = 0: fewer plots than that balances -- a single plot would run on one XCD --: workgroup w takes plot w / bpp)
    const int bpp = (M + 3) >> 2;
    const int turn = xcd_aware ? (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    const int pb = xcd_aware ? (int)(blockIdx.x & 7u) + 8 * (turn / bpp) : turn / bpp;
    const int pm = (turn % bpp) * 4 + wib;
    if (pb >= B || pm >= M) return;
    const int ci = __builtin_amdgcn_readfirstlane(pb * M + pm);
    const int nwords = (N + 31) >> 5;
    unsigned* bits = gq_bits + (size_t)wib * nwords;
    // (Round 4 tried working the centroids in the order of their Morton cells instead of FPS order -- consecutive waves then
    // walk the same cells while those are in L1 / L2 --: no gain at 16 x 32 768 (step 0.7661 against 0.7656 ms) and a small loss
    // in the parcel loop (51.2 against 52.2 k plots/s): the kernel is bound by its instructions per candidate, not by where the
    // candidates come from.)
    const int b = ci / M, m = ci - b * M;
    const float cx = cpos[((size_t)b * 3 + 0) * M + m], cy = cpos[((size_t)b * 3 + 1) * M + m],
                cz = cpos[((size_t)b * 3 + 2) * M + m];
    const int* gb = grid + (size_t)b * GRID_WORDS;
    const float* gf = reinterpret_cast<const float*>(gb + ORDER_CELLS + 1);
    const int* ord = order + (size_t)b * N;
    const float4* pts = sorted + (size_t)b * N;
    int* list = s_list[wib];
    // conservative cell range: slightly enlarged radius, same cell function as the sort (monotone in the coordinate)
    const float rr = r * 1.0001f + 1e-6f;
    int lo3[3], hi3[3];
    {
        const float cc[3] = {cx, cy, cz};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int G = a < 2 ? ORDER_GX : ORDER_GZ;
            int l = (int)(((cc[a] - rr) - gf[a]) * gf[3 + a]), h = (int)(((cc[a] + rr) - gf[a]) * gf[3 + a]);
            // (int) truncates toward zero: a negative argument must still map to cell 0 -> clamp covers it
            lo3[a] = l < 0 ? 0 : (l > G - 1 ? G - 1 : l);
            hi3[a] = h < 0 ? 0 : (h > G - 1 ? G - 1 : h);
            if ((cc[a] - rr) - gf[a] < 0.f) lo3[a] = 0;
        }
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    int h = 0;
    // one lane per candidate cell: all cell bounds arrive with ONE round trip, then the candidates of all cells form one
    // flat sequence that the wave walks 64 at a time (a cell-by-cell walk serialised ~50 dependent loads per centroid)
    const int ncx = hi3[0] - lo3[0] + 1, ncy = hi3[1] - lo3[1] + 1, ncz = hi3[2] - lo3[2] + 1;
    const int ncell = ncx * ncy * ncz;
    bool overflow = ncell > 64;
    bool dense = false;                                // more hits than the list holds: the bitmap path below
    if (!overflow) {
        __shared__ int s_pre[4][65], s_p0[4][64];
        int p0 = 0, len = 0;
        if (lane < ncell) {
            const int ix = lo3[0] + lane % ncx, iy = lo3[1] + (lane / ncx) % ncy, iz = lo3[2] + lane / (ncx * ncy);
            const unsigned cell = morton_cell((unsigned)ix, (unsigned)iy, (unsigned)iz);
            p0 = gb[cell];
            len = gb[cell + 1] - p0;
        }
        const int incl = wave_scan_incl(len);
        const int T = __shfl(incl, 63);
        s_pre[wib][lane + 1] = incl;   // exclusive prefix of cell i = s_pre[i]
        if (lane == 0) s_pre[wib][0] = 0;
        s_p0[wib][lane] = p0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // four blocks of 64 candidates per turn, their positions AND original indices all requested before the first test:
        // one round trip per 256 candidates (block by block, with the index fetched for the hits only, a centroid with 250
        // candidates waited for eight dependent loads: 54 us per launch at 16 x 32 768)
#ifndef SN2_GQ_INFLIGHT
#define SN2_GQ_INFLIGHT 4
#endif
        constexpr int GQ_INFLIGHT = SN2_GQ_INFLIGHT;
        // (a ball with few candidates -- the parcel loop's 10 000-point plots put ~70 into the 27 cells -- takes the same turn
        // with one or two blocks: the cell search and the tests of empty blocks were a fifth of the kernel's instructions)
        auto turn = [&](auto nb, int t0) {
            constexpr int NB = decltype(nb)::value;
            float4 qv[NB];
            int oi[NB];
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                const int t = t0 + 64 * c + lane;
                // the cell of candidate t: largest i with s_pre[i] <= t (binary search over <= 64 entries)
                int lo_i = 0;
#pragma unroll
                for (int step = 32; step > 0; step >>= 1) {
                    const int mid = lo_i + step;
                    if (mid < ncell && s_pre[wib][mid] <= t) lo_i = mid;
                }
                const int p = t < T ? s_p0[wib][lo_i] + (t - s_pre[wib][lo_i]) : 0;
                qv[c] = pts[p];
                oi[c] = ord[p];
            }
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                const bool in = t0 + 64 * c + lane < T;
                const bool hit = in && (sn2_d2(qv[c].x, qv[c].y, qv[c].z, cx, cy, cz) < r2);
                const unsigned long long mask = __ballot(hit);
                if (mask && !dense) {
                    const int nh = __popcll(mask);
                    if (h + nh > GQ_DENSE) {
                        dense = true;
                    } else {
                        if (hit) list[h + __popcll(mask & below)] = oi[c];
                        h += nh;
                    }
                }
            }
        };
        // Small plots with many candidates (the parcel loop: 10 000 points, r = sqrt 2: ~500 candidates and ~150 hits per centroid)
        // go to the bitmap at once: it is N / 32 words (5 trips of the wave to clear, 5 to read) whatever the count, while
        // rank-sorting h hits is h^2 / 64 steps -- 1.3 ms of the 5.5 ms a launch of 256 plots takes went into those sorts --, and
        // deciding it before the first walk saves the second one.  Same lists: ascending original index either way.
        if (nwords <= GQ_BM_WORDS && T > GQ_BM_CAND) dense = true;
        else if (T <= 64) turn(std::integral_constant<int, 1>{}, 0);
        else if (T <= 128) turn(std::integral_constant<int, 2>{}, 0);
        else
            for (int t0 = 0; t0 < T && !dense; t0 += 64 * GQ_INFLIGHT) turn(std::integral_constant<int, GQ_INFLIGHT>{}, t0);
        if (dense) {
            // A dense ball (the ground layer of a 131 072-point plot puts ~700 points into a 1 m ball): rank-sorting h hits
            // costs h^2 / 64 steps and the old fallback re-scanned the whole plot (2048 steps per centroid: 0.78 ms at
            // BASELINE config 5).  Instead: one bit per source point in LDS, the candidates walked once more to set the
            // hits' bits, then the bitmap read in order -- ascending original index by construction, no sort, any count.
            for (int i = lane; i < nwords; i += 64) bits[i] = 0u;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int t0 = 0; t0 < T; t0 += 64 * GQ_INFLIGHT) {
                float4 qv[GQ_INFLIGHT];
                int oi[GQ_INFLIGHT];
#pragma unroll
                for (int c = 0; c < GQ_INFLIGHT; ++c) {
                    const int t = t0 + 64 * c + lane;
                    int lo_i = 0;
#pragma unroll
                    for (int step = 32; step > 0; step >>= 1) {
                        const int mid = lo_i + step;
                        if (mid < ncell && s_pre[wib][mid] <= t) lo_i = mid;
                    }
                    const int p = t < T ? s_p0[wib][lo_i] + (t - s_pre[wib][lo_i]) : 0;
                    qv[c] = pts[p];
                    oi[c] = ord[p];
                }
#pragma unroll
                for (int c = 0; c < GQ_INFLIGHT; ++c)
                    if (t0 + 64 * c + lane < T && (sn2_d2(qv[c].x, qv[c].y, qv[c].z, cx, cy, cz) < r2))
                        atomicOr(&bits[oi[c] >> 5], 1u << (oi[c] & 31));
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            int* outd = nbr + (size_t)ci * cap;
            int n = 0;
            for (int w0 = 0; w0 < nwords; w0 += 64) {
                unsigned word = (w0 + lane < nwords) ? bits[w0 + lane] : 0u;
                const int c = __popc(word);
                if (__ballot(c != 0) == 0ull) continue;
                const int incl = wave_scan_incl(c);
                int pos = n + incl - c;
                while (word) {
                    const int bit = __ffs(word) - 1;
                    word &= word - 1;
                    if (pos < cap) outd[pos] = (w0 + lane) * 32 + bit;
                    ++pos;
                }
                n += __shfl(incl, 63);
            }
            if (lane == 0) cnt[ci] = n < cap ? n : cap;
            return;
        }
    }
    int* out = nbr + (size_t)ci * cap;
    if (!overflow) {
        // rank sort by original index (indices are distinct), keep the first `cap`
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int i0 = 0; i0 < h; i0 += 64) {
            const int i = i0 + lane;
            const int mine = i < h ? list[i] : 0x7FFFFFFF;
            int rank = 0;
            for (int j = 0; j < h; ++j) rank += list[j] < mine ? 1 : 0;
            if (i < h && rank < cap) out[rank] = mine;
        }
        const int c = h < cap ? h : cap;
        if (lane == 0) cnt[ci] = c;
    } else {
        // dense ball: full scan of the plot in index order (identical to ball_query_kernel for one centroid)
        const float* px = src + (size_t)b * 3 * N;
        const float* py = px + N;
        const float* pz = py + N;
        int n = 0;
        for (int j0 = 0; j0 < N; j0 += 64) {
            const int j = j0 + lane;
            const bool valid = j < N;
            const float x = valid ? px[j] : 0.f, y = valid ? py[j] : 0.f, z = valid ? pz[j] : 0.f;
            const bool hit = valid && (sn2_d2(x, y, z, cx, cy, cz) < r2);
            const unsigned long long mask = __ballot(hit);
            if (mask) {
                const int p = n + __popcll(mask & below);
                if (hit && p < cap) out[p] = j;
                n += __popcll(mask);
            }
        }
        const int c = n < cap ? n : cap;
        if (lane == 0) cnt[ci] = c;
    }
}

// *total = sum of cnt (one workgroup; thousands of same-address atomics from the query waves cost 0.2 ms)
// (grouped: workgroup h sums the n counts of batch h into total[h * tstride] -- sn2_count_sum_group)
__global__ __launch_bounds__(1024) void count_sum_kernel(const int* __restrict__ cnt_all, int n, unsigned long long* __restrict__ total_all,
                                                         size_t tstride = 0) {
    __shared__ unsigned long long s_tot;
    const int* __restrict__ cnt = cnt_all + (size_t)blockIdx.x * n;
    unsigned long long* __restrict__ total = total_all + (size_t)blockIdx.x * tstride;
    unsigned long long acc = 0;
    // sixteen counts per lane in flight (one dependent load per trip: 0.19 ms for the parcel loop's 640 000 counts)
    const int n16 = (reinterpret_cast<uintptr_t>(cnt) & 15) == 0 ? n / 16 : 0;
    const int4* c4 = reinterpret_cast<const int4*>(cnt);
    for (int i = threadIdx.x; i < n16; i += 1024) {
        int4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = c4[(size_t)i * 4 + u];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc += (unsigned long long)((long)v[u].x + v[u].y + v[u].z + v[u].w);
    }
    for (int i = n16 * 16 + threadIdx.x; i < n; i += 1024) acc += (unsigned long long)cnt[i];
    if (threadIdx.x == 0) s_tot = 0ull;
    __syncthreads();
    atomicAdd(&s_tot, acc);
    __syncthreads();
    if (threadIdx.x == 0) *total = s_tot;
}

extern "C" int sn2_ball_query(const float* src_soa, int B, int N, const float* cpos_soa, int M, float r2, int cap,
                              int* nbr, int* cnt, unsigned long long* total, const int* fps_ws, void* stream) {
    if (!src_soa || !cpos_soa || !nbr || !cnt || B <= 0 || N <= 0 || M <= 0 || cap <= 0 || !(r2 > 0.f)) return SN2_EINVAL;
    const float r = sqrtf(r2);   // only used (enlarged) to bound the cell range; the hit test is d2 < r2
    if (fps_ws && N > 2048 && (((size_t)B * N) % 4 == 0)) {
        // the sources are the point set FPS just sorted: walk its cell lists instead of the whole plot
        const fps_ws_tables w = fps_ws_carve(fps_ws, B, N);
        const int* order = w.order;
        const float4* sorted = w.sorted;
        const int* grid = w.grid;
        const size_t lds = (size_t)4 * ((N + 31) / 32) * sizeof(unsigned);       // the dense-ball bitmaps: 64 KB at N = 131 072
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ball_query_grid_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds);
        // grid: eight XCDs x the plots of the fullest XCD x the workgroups of a plot (ball_query_grid_kernel: placement)
        // (plots per XCD must balance: a multiple of 8 plots, or so many that the remainder does not matter)
        static const bool gq_no_xcd = getenv("SN2_GQ_NO_XCD") != nullptr;        // (diagnostic switch)
        const int xcd_aware = (!gq_no_xcd && (B % 8 == 0 || B >= 64)) ? 1 : 0;
        const long gq_blocks = xcd_aware ? 8L * sn2_cdiv(B, 8) * sn2_cdiv(M, 4) : (long)B * sn2_cdiv(M, 4);
        if (gq_blocks >= (1L << 31)) return SN2_ELIMIT;
        hipLaunchKernelGGL(ball_query_grid_kernel, dim3((unsigned)gq_blocks), dim3(256), lds, (hipStream_t)stream, src_soa,
                           B, N, cpos_soa, M, r, r2, cap, order, sorted, grid, nbr, cnt, total, xcd_aware);
        if (total) hipLaunchKernelGGL(count_sum_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const int*)cnt, B * M, total);
        SN2_RETURN_LAUNCH();
    }
    constexpr int TC = 8;
    const int tiles = sn2_cdiv(M, TC);
    const long waves = (long)B * tiles;
    hipLaunchKernelGGL((ball_query_kernel<TC>), dim3(sn2_cdiv(waves, 4)), dim3(256), 0, (hipStream_t)stream, src_soa, B,
                       N, cpos_soa, M, r2, cap, nbr, cnt, total, tiles);
    if (total) hipLaunchKernelGGL(count_sum_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const int*)cnt, B * M, total);
    SN2_RETURN_LAUNCH();
}

extern "C" int sn2_count_sum_group(const int* cnt, int G, int n, unsigned long long* total, size_t total_stride, void* stream) {
    if (!cnt || !total || G <= 0 || n <= 0 || (G > 1 && total_stride < 1)) return SN2_EINVAL;
    hipLaunchKernelGGL(count_sum_kernel, dim3(G), dim3(1024), 0, (hipStream_t)stream, cnt, n, total, total_stride);
    SN2_RETURN_LAUNCH();
}

extern "C" int sn2_count_sum(const int* cnt, int n, unsigned long long* total, void* stream) {
    if (!cnt || !total || n <= 0) return SN2_EINVAL;
    hipLaunchKernelGGL(count_sum_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, cnt, n, total);
    SN2_RETURN_LAUNCH();
}
