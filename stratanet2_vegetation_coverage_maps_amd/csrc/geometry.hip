// geometry.hip -- position-only kernels: row packing and farthest point sampling (the radius ball query, the 3-NN searches and
// the z-normalisation that stood here have units of their own: ball_query.hip, three_nn.hip, znorm.hip).
// All discrete decisions use the canonical fp32 squared distance sn2_d2 (common.h) so that the index structures
// are bit-identical to the oracle's.
#include "common.h"
#include "plot_sort.h"
#include <stdlib.h>

// ------------------------------------------------------------------------------------------------------------
// pack_rows: (cloud (B,C,N), xyz (B,3,N)) -> rows0 (B*N,12) = [cloud rows 2..9 | x y z 0]
// HBM-bound: reads 44 B/point coalesced (11 channel rows), writes 48 B/point as 3 x 16 B per lane.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_rows_kernel(const float* __restrict__ cloud, const float* __restrict__ xyz,
                                                        int C, int N, float* __restrict__ rows0) {
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float* cl = cloud + (size_t)b * C * N + n;
    const float* xp = xyz + (size_t)b * 3 * N + n;
    float4 v0 = make_float4(cl[2 * (size_t)N], cl[3 * (size_t)N], cl[4 * (size_t)N], cl[5 * (size_t)N]);
    float4 v1 = make_float4(cl[6 * (size_t)N], cl[7 * (size_t)N], cl[8 * (size_t)N], cl[9 * (size_t)N]);
    float4 v2 = make_float4(xp[0], xp[(size_t)N], xp[2 * (size_t)N], 0.f);
    float4* o = reinterpret_cast<float4*>(rows0 + ((size_t)b * N + n) * 12);
    o[0] = v0;
    o[1] = v1;
    o[2] = v2;
}

extern "C" int sn2_pack_rows(const float* cloud, const float* xyz, int B, int C, int N, float* rows0, void* stream) {
    if (!cloud || !xyz || !rows0 || B <= 0 || N <= 0) return SN2_EINVAL;
    if (C != 10) return SN2_ELIMIT;
    dim3 grid(sn2_cdiv(N, 256), B);
    hipLaunchKernelGGL(pack_rows_kernel, grid, dim3(256), 0, (hipStream_t)stream, cloud, xyz, C, N, rows0);
    SN2_RETURN_LAUNCH();
}

// pack_rows_feat: the same rows for a model that reads F = 4 point features -- rows0 (B*N,8) = [4 features | x y z 0].
// SIX = false: a ten-row cloud in the reference's layout, the features are its rows 2, 7, 8, 9 (z, intensity, return_num,
// num_returns: the colour rows 3..6 are never read);  SIX = true: a six-row cloud, its rows 2..5.
// Reads 28 B/point coalesced (7 channel rows), writes 32 B/point as 2 x 16 B per lane.
template <bool SIX>
__global__ __launch_bounds__(256) void pack_rows4_kernel(const float* __restrict__ cloud, const float* __restrict__ xyz,
                                                         int N, float* __restrict__ rows0) {
    constexpr int C = SIX ? 6 : 10, R1 = SIX ? 3 : 7;            // cloud rows of features 1..3: R1, R1 + 1, R1 + 2
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float* cl = cloud + (size_t)b * C * N + n;
    const float* xp = xyz + (size_t)b * 3 * N + n;
    float4 v0 = make_float4(cl[2 * (size_t)N], cl[R1 * (size_t)N], cl[(R1 + 1) * (size_t)N], cl[(R1 + 2) * (size_t)N]);
    float4 v1 = make_float4(xp[0], xp[(size_t)N], xp[2 * (size_t)N], 0.f);
    float4* o = reinterpret_cast<float4*>(rows0 + ((size_t)b * N + n) * 8);
    o[0] = v0;
    o[1] = v1;
}

extern "C" int sn2_pack_rows_feat(const float* cloud, const float* xyz, int B, int C, int N, int F, float* rows0, void* stream) {
    if (!cloud || !xyz || !rows0 || B <= 0 || C <= 0 || N <= 0 || F <= 0) return SN2_EINVAL;
    if (C == 10 && F == 8) return sn2_pack_rows(cloud, xyz, B, C, N, rows0, stream);
    if (F != 4 || (C != 6 && C != 10)) return SN2_ELIMIT;
    dim3 grid(sn2_cdiv(N, 256), B);
    if (C == 6) hipLaunchKernelGGL(pack_rows4_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, cloud, xyz, N, rows0);
    else hipLaunchKernelGGL(pack_rows4_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, cloud, xyz, N, rows0);
    SN2_RETURN_LAUNCH();
}

// ------------------------------------------------------------------------------------------------------------
// fps: one workgroup per plot; the plot's points and their running min-distance stay in VGPRs (PPT per lane);
// per round: PPT canonical distance updates per lane, a per-lane running (max, slot), a 64-bit wave max over
// (dist_bits << 32 | ~index) -- max distance, lowest index on ties, as torch.argmax -- one LDS exchange between the
// waves and ONE barrier (LDS slots double-buffered by round parity).
// Latency/VALU-bound by construction: M strictly sequential rounds; HBM traffic is 12 B/point once.
// ------------------------------------------------------------------------------------------------------------
// The live prefix of a plot (sn2_fps_live in include/strata_hip.h): n_live[b] clamped to [1, N] on the device, N without the array.
// Points at and behind it are DEAD in every FPS kernel below: their running distance is +0.0f from the first round on (fminf keeps
// it there), so none of them is ever a strict maximum, and a kernel that finds the plot's maximum at 0 ends through fps_fill_zero.
__device__ __forceinline__ int fps_live_count(const int* __restrict__ n_live, int b, int N) {
    int n = n_live ? n_live[b] : N;
    n = n < 1 ? 1 : (n > N ? N : n);
    return __builtin_amdgcn_readfirstlane(n);
}
// A plot's output rows: idx (B, M), cpos_soa (B, 3, M), cpos_aos (B * M, 4).  THE statement of how a sample leaves: the bucketed
// kernels and fps_fill_zero all write through `emit`.  A sample's `code` is its original index, or -1 - its sorted position where
// a kernel defers the load of ord[] (`translate` at its end: in the sampling loop it would sit on the selecting wave's critical path).
struct fps_rows {
    int* idx_out;
    float *cpos_soa, *cpos_aos;
    int b, M;
    // (the stores go through __restrict__ parameters: written on the members, which carry no such promise, they cost
    // fps_bucket_kernel eight VGPRs -- <128, 16> a wave per SIMD -- and changed the registers of every fps_kernel)
    static __device__ __forceinline__ void emit_to(int* __restrict__ idx_out, float* __restrict__ cpos_soa, float* __restrict__ cpos_aos,
                                                   int b, int M, int at, float x, float y, float z, int code) {
        idx_out[(size_t)b * M + at] = code;
        cpos_soa[((size_t)b * 3 + 0) * M + at] = x;
        cpos_soa[((size_t)b * 3 + 1) * M + at] = y;
        cpos_soa[((size_t)b * 3 + 2) * M + at] = z;
        reinterpret_cast<float4*>(cpos_aos)[(size_t)b * M + at] = make_float4(x, y, z, 0.f);
    }
    __device__ __forceinline__ void emit(int at, float x, float y, float z, int code) const {
        emit_to(idx_out, cpos_soa, cpos_aos, b, M, at, x, y, z, code);
    }
    // by all `nt` threads of the workgroup, behind a barrier.  log = nullptr: the samples are out, their codes become indices;
    // log = the M samples (x, y, z, code) that fps_cluster_kernel kept in LDS: they leave here
    __device__ __forceinline__ void translate(const int* __restrict__ ord, int tid, int nt, const float4* log) const {
        for (int i = tid; i < M; i += nt) {
            if (log) {
                const float4 e = log[i];
                const int code = __float_as_int(e.w);
                emit(i, e.x, e.y, e.z, code < 0 ? ord[-1 - code] : code);
            } else {
                const int v = idx_out[(size_t)b * M + i];
                if (v < 0) idx_out[(size_t)b * M + i] = ord[-1 - v];
            }
        }
    }
};
// The plot's maximum reached 0 with `from` samples out: every point is at distance 0, the arg-max of an all-zero row is index 0,
// and so is every later sample.  Called by all `nt` threads of the workgroup that writes the plot's samples.
__device__ __forceinline__ void fps_fill_zero(const float* __restrict__ px, int N, int M, int b, int from, int tid, int nt,
                                              int* __restrict__ idx_out, float* __restrict__ cpos_soa,
                                              float* __restrict__ cpos_aos, int* __restrict__ n_live_out) {
    const float x0 = px[0], y0 = px[N], z0 = px[2 * (size_t)N];
    const fps_rows out = {idx_out, cpos_soa, cpos_aos, b, M};
    for (int i = from + tid; i < M; i += nt) out.emit(i, x0, y0, z0, 0);
    if (tid == 0 && n_live_out) n_live_out[b] = from;
}
template <int PPT, int T, bool ZLDS>
__global__ __launch_bounds__(T) void fps_kernel(const float* __restrict__ pos, int N, int M,
                                                const int* __restrict__ start, int* __restrict__ idx_out,
                                                float* __restrict__ cpos_soa, float* __restrict__ cpos_aos,
                                                const int* __restrict__ n_live, int* __restrict__ n_live_out) {
    constexpr int NW = T / 64;
    // PLDS: a copy of the positions in LDS (16 B per point) where it is small: the winner's coordinates are then one LDS read
    // per round instead of three dependent global loads (~500 clocks of the ~1250 a round of the 1024 -> 256 level took)
    constexpr bool PLDS = !ZLDS && PPT * T * 16 <= 32 * 1024;
    __shared__ float4 s_pos[PLDS ? PPT * T : 1];
    __shared__ unsigned long long s_key[2][NW];
    // ZLDS (PPT = 32): x, y and the running distance fill the 128-VGPR budget of a 1024-lane workgroup, so the z
    // row lives in LDS (128 KiB, each lane re-reads only its own slots: conflict-free ds_read_b32).
    __shared__ float s_z[ZLDS ? PPT * T : 1];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* px = pos + (size_t)b * 3 * N;
    const float* py = px + N;
    const float* pz = py + N;
    float x[PPT], y[PPT], z[ZLDS ? 1 : PPT], d[PPT];
    const int nlive = fps_live_count(n_live, b, N);
    if (tid == 0 && n_live_out) n_live_out[b] = M;    // unless the maximum reaches 0 first (fps_fill_zero)
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int j = k * T + tid;
        const bool v = j < N;
        x[k] = v ? px[j] : 0.f;
        y[k] = v ? py[j] : 0.f;
        if constexpr (ZLDS) s_z[j] = v ? pz[j] : 0.f; else z[k] = v ? pz[j] : 0.f;
        if constexpr (PLDS) s_pos[j] = make_float4(x[k], y[k], z[k], 0.f);
        d[k] = j < nlive ? INFINITY : 0.f;  // dead points and padding lanes: distance 0 -> never a strict maximum
    }
    int cur = start ? start[b] : 0;
    cur = cur < 0 ? 0 : (cur >= N ? N - 1 : cur);
    if constexpr (PLDS) __syncthreads();
    for (int i = 0; i < M; ++i) {
        cur = __builtin_amdgcn_readfirstlane(cur);
        float lx, ly, lz;
        if constexpr (PLDS) {
            const float4 c = s_pos[cur];
            lx = c.x; ly = c.y; lz = c.z;
        } else {
            lx = px[cur]; ly = py[cur]; lz = pz[cur];
        }
        if (tid == 0) {
            idx_out[(size_t)b * M + i] = cur;
            cpos_soa[((size_t)b * 3 + 0) * M + i] = lx;
            cpos_soa[((size_t)b * 3 + 1) * M + i] = ly;
            cpos_soa[((size_t)b * 3 + 2) * M + i] = lz;
            reinterpret_cast<float4*>(cpos_aos)[(size_t)b * M + i] = make_float4(lx, ly, lz, 0.f);
        }
        if (i == M - 1) break;
        float best = -1.f;
        int bk = 0;
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            float zk;
            if constexpr (ZLDS) zk = s_z[k * T + tid]; else zk = z[k];
            const float dd = sn2_d2(x[k], y[k], zk, lx, ly, lz);
            const float nd = fminf(d[k], dd);
            d[k] = nd;
            if (nd > best) {  // strict: the lowest slot (= lowest index of this lane) wins ties
                best = nd;
                bk = k;
            }
            // keep the scheduler from hoisting all 32 LDS reads at once (that spills at the 128-VGPR budget)
            if constexpr (ZLDS) { if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0); }
        }
        // wave level: maximal distance by DPP, then the lowest index among the lanes attaining it (two 6-step DPP
        // reductions instead of a 64-bit ds_bpermute butterfly)
        const float wm = wave_max_dpp(best);
        const unsigned wi = wave_min_u32_dpp(best == wm ? (unsigned)(bk * T + tid) : 0xFFFFFFFFu);
        if (lane == 0) s_key[i & 1][wave] = ((unsigned long long)__float_as_uint(wm) << 32) | (unsigned long long)wi;
        __syncthreads();
        const unsigned long long k2 = s_key[i & 1][lane % NW];
        const float gv = wave_max_dpp(__uint_as_float((unsigned)(k2 >> 32)));
        const unsigned gi = wave_min_u32_dpp(__uint_as_float((unsigned)(k2 >> 32)) == gv ? (unsigned)(k2 & 0xFFFFFFFFull) : 0xFFFFFFFFu);
        cur = (int)gi;
        if (gv == 0.f) {
            fps_fill_zero(px, N, M, b, i + 1, tid, T, idx_out, cpos_soa, cpos_aos, n_live_out);
            break;
        }
    }
}

// the arguments of sn2_fps_live (include/strata_hip.h), as every launcher below takes them
struct fps_call {
    const float* pos;
    int B, N, M;
    const int *start, *nl;
    int* idx;
    float *cs, *ca;
    int *ws, *nlo;
    unsigned* status;
    hipStream_t st;
};

template <int PPT, int T, bool ZLDS = false>
static int launch_fps(const fps_call& a) {
    hipLaunchKernelGGL((fps_kernel<PPT, T, ZLDS>), dim3(a.B), dim3(T), 0, a.st, a.pos, a.N, a.M, a.start, a.idx, a.cs, a.ca, a.nl, a.nlo);
    SN2_RETURN_LAUNCH();
}

// ------------------------------------------------------------------------------------------------------------
// Bucketed FPS (exact).  The brute-force kernel above touches all N points in each of the M sequential rounds
// (4.1 ms for 16 x 32768 -> 1024 on MI355X: 40 % of a training step).  But a new sample s only lowers the running
// distance of points closer to s than their current distance, i.e. points near s.  So:
//   * spatial_order_chunk_kernel sorts a plot's points by the Morton code of a 16x16x16 cell grid (LDS counting sort);
//   * consecutive runs of 64 sorted points form a BUCKET = one VGPR slot of one wave (bucket b -> wave b % 16, slot
//     b / 16, so spatially adjacent buckets sit in different waves and a round's work spreads over the 16 waves);
//   * per bucket LDS keeps the bounding box and the maximum running distance; per round each wave tests its <= 32
//     buckets (one lane each): a bucket can only change if  boxdist2(s) < bucket_max.  The test is EXACT, not a
//     heuristic: boxdist2 is evaluated with the same canonical fp32 operations as sn2_d2, and fp32 rounding is
//     monotone, so boxdist2(s) <= d2(p, s) for every point p of the box, bit for bit; if boxdist2(s) >= bucket_max
//     then min(dist_p, d2(p,s)) == dist_p for all its points and skipping the bucket changes nothing.
//   * dirty buckets are updated by their wave (x, y, z in VGPRs, running distance in LDS) and get a new maximum;
//   * the next sample is the point of maximal running distance; exact ties are resolved towards the lowest ORIGINAL
//     index, as torch.argmax does on the unsorted array (candidates = lanes whose distance equals the global maximum).
// Result: bit-identical indices to the brute-force kernel, with ~20x fewer distance evaluations after the first rounds.
// ------------------------------------------------------------------------------------------------------------
#include "fps_ws.h"

// One workgroup per plot walks the points three times (bounding box, histogram, scatter: the counting sort of plot_sort.h); a
// trip fetches U points per thread before it touches the first (two trips per pass at N = 32 768 with U = 16 and 1024 threads:
// one DEPENDENT load per trip took 71 us, all 32 points of a thread in registers at once spill).  What is left (61 us) are the
// LDS atomics: 55 % of a plot's points are ground points in a few cell layers, and a wave's adds onto one counter serialise.
// rank (or NULL): rank[plot * N + i] = sorted position of point i -- the inverse of `order` (sn2_fp.row_perm)
template <int U, int NT>
__global__ __launch_bounds__(NT) void spatial_order_chunk_kernel(const float* __restrict__ pos, int N, int* __restrict__ order,
                                                                 float4* __restrict__ sorted, int* __restrict__ grid,
                                                                 unsigned* __restrict__ xchg, unsigned* __restrict__ ctl,
                                                                 int* __restrict__ rank, const int* __restrict__ n_live) {
    __shared__ int s_hist[ORDER_CELLS];
    __shared__ float s_mm[6][NT / 64];
    __shared__ int s_wsum[NT / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* px = pos + (size_t)b * 3 * N;
    const float* py = px + N;
    const float* pz = py + N;
    // fn(i, x, y, z) for every point i of the plot, U points per thread and trip (plot_sort.h's loader, box and cell scan written
    // out: built from its functions this kernel measured 0.5 - 2.4 % slower, profiles/plot_sort)
    auto for_points = [&](auto fn) {
        for (int i0 = 0; i0 < N; i0 += NT * U) {
            float vx[U], vy[U], vz[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = i0 + u * NT + tid;
                const int ii = i < N ? i : N - 1;
                vx[u] = px[ii]; vy[u] = py[ii]; vz[u] = pz[ii];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = i0 + u * NT + tid;
                if (i < N) fn(i, vx[u], vy[u], vz[u]);
            }
        }
    };
    if (xchg) {
        for (int i = tid; i < FPS_XCHG_WORDS; i += NT) xchg[(size_t)b * FPS_XCHG_WORDS + i] = 0u;
        if (b == 0 && tid < FPS_CTL_WORDS) ctl[tid] = 0u;
    }
    for (int i = tid; i < ORDER_CELLS; i += NT) s_hist[i] = 0;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for_points([&](int, float vx, float vy, float vz) {
        mn[0] = fminf(mn[0], vx); mx[0] = fmaxf(mx[0], vx);
        mn[1] = fminf(mn[1], vy); mx[1] = fmaxf(mx[1], vy);
        mn[2] = fminf(mn[2], vz); mx[2] = fmaxf(mx[2], vz);
    });
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        mn[a] = wave_min(mn[a]);
        mx[a] = wave_max(mx[a]);
        if (lane == 0) {
            s_mm[a][wave] = mn[a];
            s_mm[3 + a][wave] = mx[a];
        }
    }
    __syncthreads();
    float lo[3], sc[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float l = s_mm[a][0], h = s_mm[3 + a][0];
        for (int k = 1; k < NT / 64; ++k) {
            l = fminf(l, s_mm[a][k]);
            h = fmaxf(h, s_mm[3 + a][k]);
        }
        lo[a] = l;
        const float ext = fmaxf(h - l, 1e-6f);
        sc[a] = (a < 2 ? (float)ORDER_GX : (float)ORDER_GZ) / ext;
    }
    for_points([&](int, float vx, float vy, float vz) { atomicAdd(&s_hist[order_cell(lo, sc, vx, vy, vz)], 1); });
    __syncthreads();
    // exclusive scan over the cells: PER consecutive cells per thread, wave scan, 16 wave totals
    constexpr int PER = ORDER_CELLS / NT;
    int loc[PER], sum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        loc[k] = s_hist[tid * PER + k];
        sum += loc[k];
    }
    const int incl = wave_scan_incl(sum);
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    int base = 0;
    for (int k = 0; k < wave; ++k) base += s_wsum[k];
    int run = base + incl - sum;
    int* gb = grid + (size_t)b * GRID_WORDS;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        s_hist[tid * PER + k] = run;
        gb[tid * PER + k] = run;                        // cell -> first sorted position (the ball query walks these cell lists)
        run += loc[k];
    }
    if (tid == 0) {
        gb[ORDER_CELLS] = N;
        float* gf = reinterpret_cast<float*>(gb + ORDER_CELLS + 1);
        gf[0] = lo[0]; gf[1] = lo[1]; gf[2] = lo[2]; gf[3] = sc[0]; gf[4] = sc[1]; gf[5] = sc[2];
        gb[GRID_WORDS - 1] = 0;
    }
    __syncthreads();
    int* ob = order + (size_t)b * N;
    float4* sb = sorted + (size_t)b * N;
    const int nlive = fps_live_count(n_live, b, N);
    for_points([&](int i, float vx, float vy, float vz) {
        const int p = atomicAdd(&s_hist[order_cell(lo, sc, vx, vy, vz)], 1);
        ob[p] = i;
        sb[p] = make_float4(vx, vy, vz, i < nlive ? INFINITY : 0.f);      // .w = running FPS distance (dead points: 0 throughout)
        if (rank) rank[(size_t)b * N + i] = p;
    });
}

// the plot's Morton order, sorted table and cell starts (+ the zeroed exchange area)
static void launch_spatial_order(const float* pos, int B, int N, int* order, float4* sorted, int* grid, unsigned* xchg,
                                 unsigned* ctl, int* rank, const int* nl, hipStream_t st) {
    if (sn2_small_sort_wg(B) && N <= 16 * 1024)          // many plots: 256 threads per plot (common.h)
        hipLaunchKernelGGL((spatial_order_chunk_kernel<16, 256>), dim3(B), dim3(256), 0, st, pos, N, order, sorted, grid, xchg, ctl, rank, nl);
    else if (N <= 8 * 1024)
        hipLaunchKernelGGL((spatial_order_chunk_kernel<8, 1024>), dim3(B), dim3(1024), 0, st, pos, N, order, sorted, grid, xchg, ctl, rank, nl);
    else
        hipLaunchKernelGGL((spatial_order_chunk_kernel<16, 1024>), dim3(B), dim3(1024), 0, st, pos, N, order, sorted, grid, xchg, ctl, rank, nl);
}

// canonical, monotone lower bound of sn2_d2(p, c) over all p inside the box [lo, hi]
__device__ __forceinline__ float sn2_box_d2(float lx, float ly, float lz, float hx, float hy, float hz, float cx, float cy,
                                            float cz) {
#pragma clang fp contract(off)
    const float dx = fmaxf(fmaxf(lx - cx, cx - hx), 0.f);
    const float dy = fmaxf(fmaxf(ly - cy, cy - hy), 0.f);
    const float dz = fmaxf(fmaxf(lz - cz, cz - hz), 0.f);
    const float xx = dx * dx;
    const float yy = dy * dy;
    const float zz = dz * dz;
    const float s = xx + yy;
    return s + zz;
}

// SPW = bucket slots per wave (bucket b lives in wave b % 16, slot b / 16); 16 waves.  The sorted points stay in
// global memory (an L2-resident 16 B x N table, one dwordx4 per lane fetches a whole bucket) and the table's .w lane is
// the point's RUNNING DISTANCE: it arrives with the coordinates in the same dwordx4 and is written back when it shrinks.
// Plain loads and stores are enough: a bucket is only ever touched by its own wave, and a CU's vector L1 is write-through
// and coherent with that CU's own stores (agent-scope `sc1` accesses were tried first: they bypass the XCD's L2 too and
// made the kernel 27 % slower).
// LDS holds only the bucket boxes and the per-wave exchange records (13 KB): with the distances in LDS (128 KB at
// N = 32768) a workgroup needed a CU with no other LDS user, and next to the feature kernels of the pipelined training
// step such a CU only turned up when another FPS workgroup retired -- two FPS passes in flight ran back to back.
// Registers hold no per-point state, so the round loop is a short body executed only for the buckets that can change
// (no 32-way unrolled branch chain: that version was instruction-fetch bound).
__device__ __forceinline__ void fps_st_dist(float4* t, int p, float v) { reinterpret_cast<float*>(t + p)[3] = v; }
#ifdef SN2_FPS_STAMPS
// diagnostic build only (never shipped): per-phase cycle totals of wave 0 of workgroup 0
__device__ unsigned long long g_fps_dbg[8];
__device__ unsigned long long g_fps_dbg2[32];
extern "C" int sn2_debug_fps_stamps2(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fps_dbg2), sizeof(g_fps_dbg2));
}
#define STAMP(var) unsigned long long var; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var)::"memory")
extern "C" int sn2_debug_fps_stamps(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fps_dbg), sizeof(g_fps_dbg));
}
#else
#define STAMP(var)
#endif

// wave64 max with the DPP modifier fused into v_max_f32 (the update_dpp builtin of wave_max_dpp costs a v_mov, a v_mov_dpp, an
// s_nop and the v_max per step: 24 instructions per reduction; this is 12).  All 64 lanes must be active.
__device__ __forceinline__ float wave_max_fused(float v) {
    asm("s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "s_nop 1"
        : "+v"(v));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// ------------------------------------------------------------------------------------------------------------
// The bucket phases, stated ONCE for the three bucketed kernels below (fps_bucket_kernel = route ROUND, fps_spec_kernel = SPEC
// and the repair launch, fps_cluster_kernel = CLUSTER).  The kernels must agree bit for bit, so what they share is one text:
// the plot's pointers and first sample, the rows a sample is written to, the bucket boxes, phase A's queue push, phase B's
// entry update and the exact-tie search.  Where the callers differ they differ in a compile-time BUCKET VIEW (fps_buckets).
// ------------------------------------------------------------------------------------------------------------
// a plot's inputs: its SoA rows in the original order, the Morton order and the sorted table of spatial_order_chunk_kernel
struct fps_plot {
    const float *px, *py, *pz;
    const int* ord;                                    // sorted position -> original index
    float4* pts;                                       // sorted: (x, y, z, running distance = +inf from the sort; dead points: 0)
    __device__ __forceinline__ fps_plot(const float* pos, const int* order, float4* sorted, int b, int N)
        : px(pos + (size_t)b * 3 * N), py(px + N), pz(py + N), ord(order + (size_t)b * N), pts(sorted + (size_t)b * N) {}
};
// the first sample: start[b] clamped into the plot (0 without the array), wave-uniform
__device__ __forceinline__ int fps_first(const int* __restrict__ start, int b, int N) {
    int cur = start ? start[b] : 0;
    cur = cur < 0 ? 0 : (cur >= N ? N - 1 : cur);
    return __builtin_amdgcn_readfirstlane(cur);
}
// BUCKET VIEW: where the buckets of a workgroup of NW waves lie.  Its local bucket lb = slot * NW + wave is bucket lb * P + part
// of the plot (P = 1: the workgroup owns the whole plot), and the bucket's 64 points are the sorted positions 64 * bucket + lane:
// quads of the L2-resident table `pts`, or -- LP -- of the workgroup's own copy in LDS (s_pts, filled by `keep` while the boxes
// are built: the updates of phase B then never leave the CU).
template <int NW_, int P_ = 1, bool LP_ = false>
struct fps_buckets {
    static constexpr int NW = NW_, P = P_;
    float4* pts;
    int N, part;
    float4* s_pts;
    __device__ __forceinline__ int pos(int lb, int lane) const { return (lb * P + (P > 1 ? part : 0)) * 64 + lane; }
    // the point of `lane` in local bucket lb; p = pos(lb, lane), which the caller has at hand
    __device__ __forceinline__ float4 quad(int lb, int lane, int p) const {     // (a padding lane of the last bucket: any quad)
        if constexpr (LP_) return s_pts[lb * 64 + lane]; else return pts[p < N ? p : 0];
    }
    __device__ __forceinline__ float dist(int lb, int lane, int p) const {      // of a real point
        if constexpr (LP_) return s_pts[lb * 64 + lane].w; else return pts[p].w;
    }
    __device__ __forceinline__ void set_dist(int lb, int lane, int p, float v) const {
        if constexpr (LP_) reinterpret_cast<float*>(s_pts + lb * 64 + lane)[3] = v; else fps_st_dist(pts, p, v);
    }
    __device__ __forceinline__ void keep(int lb, int lane, const float4& q) const {
        if constexpr (LP_) s_pts[lb * 64 + lane] = q;
    }
};

// the boxes of this wave's SPW buckets -> s_box, SoA rows [component][wave][slot]: lane j reads word j of its wave's row =>
// conflict-free (an AoS box layout cost 32-way conflicts).  Returns the wave's row (+ component * SPW * NW + slot).
template <int SPW, class View>
__device__ __forceinline__ float* fps_bucket_boxes(const View& vw, float* s_box, int wave, int lane) {
    constexpr int NBK = SPW * View::NW;
    float* my_box = s_box + wave * SPW;
    for (int k = 0; k < SPW; ++k) {
        const int lb = k * View::NW + wave, p = vw.pos(lb, lane);
        const bool v = p < vw.N;
        const float4 q = v ? vw.pts[p] : make_float4(0.f, 0.f, 0.f, 0.f);
        vw.keep(lb, lane, q);
        const float lx = -wave_max_fused(v ? -q.x : -INFINITY), ly = -wave_max_fused(v ? -q.y : -INFINITY),
                    lz = -wave_max_fused(v ? -q.z : -INFINITY);
        const float hx = wave_max_fused(v ? q.x : -INFINITY), hy = wave_max_fused(v ? q.y : -INFINITY),
                    hz = wave_max_fused(v ? q.z : -INFINITY);
        if (lane == 0) {
            my_box[0 * NBK + k] = lx; my_box[1 * NBK + k] = ly; my_box[2 * NBK + k] = lz;
            my_box[3 * NBK + k] = hx; my_box[4 * NBK + k] = hy; my_box[5 * NBK + k] = hz;
        }
    }
    return my_box;
}

// phase A's push, by a whole wave: the lanes with a sample mask `sm` != 0 append (local bucket | sm << 11) to the workgroup's
// queue -- one ballot, one atomicAdd per wave, the lane's slot from mbcnt
__device__ __forceinline__ void fps_queue_push(unsigned* s_q, int* s_qn, unsigned sm, int lb, int lane) {
    const unsigned long long bal = __ballot(sm != 0u);
    if (bal) {
        int base = 0;
        if (lane == 0) base = atomicAdd(s_qn, __popcll(bal));
        base = __builtin_amdgcn_readfirstlane(base);
        if (sm != 0u) s_q[base + __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u))] =
            (unsigned)lb | (sm << 11);
    }
}

// phase B: the qn queue entries dealt out to the waves, four per wave in flight (8 measured no faster: the phase is VALU-bound):
// new distances from the samples of the entry's mask (lanes 0.. of ax, ay, az); if the bucket's maximum (or its holder) moved,
// the new (max, second max, arg-max point) go to LDS.  `stamp` (SN2_FPS_STAMPS builds): this wave counts its entries.
// HOLD: an entry's sorted position stays in a register from its load to its update (as every kernel's own loop had it) instead of
// being computed twice.  Four of them across the loads cost the kernels at 6 or 7 waves per SIMD one of those waves, so only
// the rungs whose occupancy other registers set hold them: there the second computation was measured (profiles/fps_phases).
template <bool HOLD, class View>
__device__ __forceinline__ void fps_update_queue(const View& vw, int qn, int wave, int lane, float ax, float ay, float az,
                                                 const unsigned* s_q, float* s_val, float* s_max2, float4* s_pt,
                                                 [[maybe_unused]] bool stamp) {
    constexpr int QD = 4;
    for (int i0 = wave; i0 < qn; i0 += QD * View::NW) {
        unsigned ent[QD];
        [[maybe_unused]] int held[QD];
        bool on[QD];
        float4 q[QD];
        float U[QD];
#pragma unroll
        for (int u = 0; u < QD; ++u) {
            const int i = i0 + u * View::NW;
            on[u] = i < qn;
            ent[u] = s_q[on[u] ? i : 0];
            const int lb = (int)(ent[u] & 2047u);
            const int p = vw.pos(lb, lane);
            if constexpr (HOLD) held[u] = p;
            q[u] = vw.quad(lb, lane, p);
            U[u] = s_val[lb];
        }
#pragma unroll
        for (int u = 0; u < QD; ++u) {
            if (!on[u]) continue;
            const int lb = (int)(ent[u] & 2047u);
            unsigned sm = ent[u] >> 11;
            const float d0 = q[u].w;
            float nd = d0;
            while (sm) {
                const int k = __ffs(sm) - 1;
                sm &= sm - 1;
                const float sx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ax), k));
                const float sy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ay), k));
                const float sz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(az), k));
                nd = fminf(nd, sn2_d2(q[u].x, q[u].y, q[u].z, sx, sy, sz));
            }
            int p;
            if constexpr (HOLD) p = held[u]; else p = vw.pos(lb, lane);
            const bool real = p < vw.N;
            const bool changed = real && nd < d0;
            if (changed) vw.set_dist(lb, lane, p, nd);
#ifdef SN2_FPS_STAMPS
            if (stamp && lane == 0) {
                g_fps_dbg2[25] += 1;                                                     // entries
                g_fps_dbg2[26] += __ballot(changed) != 0ull ? 1 : 0;                     // ... with a changed point
                g_fps_dbg2[27] += (__ballot(changed && d0 == U[u]) == 0ull && U[u] != INFINITY) ? 0 : 1;   // ... slow path
                g_fps_dbg2[28] += __popc(ent[u] >> 11);                                  // samples per entry
                g_fps_dbg2[29] += __popcll(__ballot(changed));                           // changed points
            }
#endif
            // five of six queue entries change no point at all (the box test is necessary, not sufficient: fps_stamps.py);
            // a bucket's FIRST visit always takes its maximum (a bucket of dead points only changes nothing and holds 0)
            if (__ballot(changed) == 0ull && U[u] != INFINITY) continue;
            // nothing of the bucket's maximum moved (no changed point held it): its (max, point) stand, and its
            // second-max entry stays an UPPER bound of the true one, which is all the acceptance tests need
            if (__ballot(changed && d0 == U[u]) == 0ull && U[u] != INFINITY) continue;
            if (!real) nd = -1.f;                               // padding lanes of the last bucket never win
            const float m1 = wave_max_fused(nd);
            const unsigned long long bal = __ballot(nd == m1);
            const int first = __ffsll((long long)bal) - 1;
            float m2 = m1;
            if (__popcll(bal) == 1) m2 = wave_max_fused(nd == m1 ? -1.f : nd);
            const float fx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q[u].x), first));
            const float fy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q[u].y), first));
            const float fz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q[u].z), first));
            if (lane == 0) {
                s_val[lb] = m1;
                s_max2[lb] = m2;
                s_pt[lb] = make_float4(fx, fy, fz, __int_as_float(vw.pos(lb, first)));
            }
        }
    }
}

// exact tie of the maximal distance V (duplicated points, ...): the lowest ORIGINAL index among this wave's points at V -> s_win
// (atomicMin; the caller set it to 0xFFFFFFFF and puts a barrier behind).  at_max(h): slot 64 h + lane of this wave holds V.
template <int SL, class View, class AtMax>
__device__ __forceinline__ void fps_tie_search(const View& vw, const int* __restrict__ ord, int wave, int lane, float V,
                                               unsigned* s_win, AtMax at_max) {
#pragma unroll
    for (int h = 0; h < SL; ++h) {
        unsigned long long cand = __ballot(at_max(h));
        while (cand) {
            const int lb = (64 * h + __ffsll((long long)cand) - 1) * View::NW + wave;
            cand &= cand - 1;
            const int pp = vw.pos(lb, lane);
            const float d = pp < vw.N ? vw.dist(lb, lane, pp) : -1.f;
            unsigned oi = 0xFFFFFFFFu;
            if (d == V) oi = (unsigned)ord[pp];
            oi = wave_min_u32_dpp(oi);
            if (lane == 0) atomicMin(s_win, oi);
        }
    }
}

// fps_bucket_kernel (route ROUND: waves = 1, instantiated for 16 waves only): one sample per arg-max round, as the comment above
// the shared statements describes it.  Set-up, boxes, tie search and emission are those statements (view: P = 1, points in the
// L2 table); the per-wave dirty test, the in-register bucket state and the one-barrier exchange of a round are its own.
template <int SPW, int NW>
__global__ __launch_bounds__(NW * 64) void fps_bucket_kernel(const float* __restrict__ pos, int N, int M,
                                                          const int* __restrict__ start, const int* __restrict__ order,
                                                          float4* sorted, int* __restrict__ idx_out,
                                                          float* __restrict__ cpos_soa, float* __restrict__ cpos_aos,
                                                          int* __restrict__ n_live_out) {
    constexpr int NBK = SPW * NW;
    constexpr int SL = (SPW + 63) / 64;                // bucket slots per lane: slot s = 64 h + lane, h < SL
    static_assert(SPW <= 128 && NW <= 16, "at most two bucket slots per lane");
    __shared__ float s_box[6 * NBK];                   // bucket boxes (fps_bucket_boxes)
    __shared__ float4 s_xchg[2][2][NW];                // per wave: (max distance, tie flag, -, -) and (x, y, z, sorted position)
    __shared__ unsigned s_win;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const fps_plot plot(pos, order, sorted, b, N);
    const float *px = plot.px, *py = plot.py, *pz = plot.pz;
    const int* ord = plot.ord;
    float4* pts = plot.pts;
    const fps_rows out = {idx_out, cpos_soa, cpos_aos, b, M};
    const fps_buckets<NW> view = {pts, N, 0, nullptr};
    if (tid == 0 && n_live_out) n_live_out[b] = M;     // unless the maximum reaches 0 first (fps_fill_zero)
    const float* my_box = fps_bucket_boxes<SPW>(view, s_box, wave, lane);
    // lane j < SPW keeps the state of bucket slot j of this wave in registers: its maximal running distance, the point
    // attaining it (lowest lane on ties) and whether several points share the maximum (then the lowest ORIGINAL index must
    // be found the slow way)
    float mine[SL], bx[SL], by[SL], bz[SL];
    int bpos[SL];
    bool tiej[SL];
#pragma unroll
    for (int h = 0; h < SL; ++h) {
        const int sl = 64 * h + lane;
        mine[h] = (sl < SPW && (sl * NW + wave) * 64 < N) ? INFINITY : -1.f;
        bx[h] = by[h] = bz[h] = 0.f;
        bpos[h] = 0;
        tiej[h] = false;
    }
    int cur = fps_first(start, b, N);
    float cx = px[cur], cy = py[cur], cz = pz[cur];
    int cur_pos = -1;                                   // >= 0: the sample is sorted point cur_pos (index = ord[cur_pos])
    __syncthreads();

    // one dirty bucket: new distances, bucket maximum, its point -> the registers of lane k
    auto update = [&](int k, int p, const float4& q) {
        const float d = q.w;
        const float dd = sn2_d2(q.x, q.y, q.z, cx, cy, cz);
        const float nd = p < N ? fminf(d, dd) : -1.f;   // padding lanes of the last bucket never win
        if (p < N && nd < d) fps_st_dist(pts, p, nd);
        const float m = wave_max_dpp(nd);
        const unsigned long long bal = __ballot(nd == m);
        const int first = __ffsll((long long)bal) - 1;
        const float fx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q.x), first));
        const float fy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q.y), first));
        const float fz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q.z), first));
#pragma unroll
        for (int h = 0; h < SL; ++h)
            if (k == 64 * h + lane) {
                mine[h] = m;
                tiej[h] = __popcll(bal) > 1;
                bx[h] = fx;
                by[h] = fy;
                bz[h] = fz;
                bpos[h] = p - lane + first;
            }
    };

    for (int i = 0; i < M; ++i) {
        if (tid == 0) out.emit(i, cx, cy, cz, cur_pos >= 0 ? ord[cur_pos] : cur);
        if (i == M - 1) break;
        STAMP(t0);
        // (a) which of this wave's buckets can change?  lane j tests slots j, j + 64, ...
        unsigned long long masks[SL];
#pragma unroll
        for (int h = 0; h < SL; ++h) {
            const int sl = 64 * h + lane;
            bool dirty = false;
            if (sl < SPW) {
                dirty = sn2_box_d2(my_box[0 * NBK + sl], my_box[1 * NBK + sl], my_box[2 * NBK + sl], my_box[3 * NBK + sl],
                                   my_box[4 * NBK + sl], my_box[5 * NBK + sl], cx, cy, cz) < mine[h];
            }
            masks[h] = __ballot(dirty);
        }
        STAMP(t1);
#ifdef SN2_FPS_STAMPS
        int ndirty = 0;
#pragma unroll
        for (int h = 0; h < SL; ++h) ndirty += __popcll(masks[h]);
#endif
        // (b) update the dirty buckets, four at a time so that their L2 loads overlap
#pragma unroll
        for (int h = 0; h < SL; ++h) {
            unsigned long long mask = masks[h];
            while (mask) {
                int k[4], p[4];
                bool on[4];
                float4 q[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    on[u] = mask != 0;
                    k[u] = 64 * h + (on[u] ? __ffsll((long long)mask) - 1 : 0);
                    mask &= mask - 1;   // no-op when mask == 0
                    p[u] = (k[u] * NW + wave) * 64 + lane;
                    q[u] = pts[p[u] < N ? p[u] : 0];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (on[u]) update(k[u], p[u], q[u]);   // the round loop is VALU-issue bound: no duplicated work
            }
        }
        STAMP(t2);
        // (c) this wave's best bucket, then ONE barrier and the best of the 16 waves
        float lm = -1.f;
#pragma unroll
        for (int h = 0; h < SL; ++h) lm = fmaxf(lm, mine[h]);               // invalid slots hold -1
        const float wm = wave_max_dpp(lm);
        int nbest = 0;
        bool published = false;
#pragma unroll
        for (int h = 0; h < SL; ++h) {
            const unsigned long long balw = __ballot(mine[h] == wm);
            nbest += __popcll(balw);
        }
#pragma unroll
        for (int h = 0; h < SL; ++h) {
            const unsigned long long balw = __ballot(mine[h] == wm);
            if (balw && !published) {                                        // wave-uniform: the first slot group that has it
                const int slot = __ffsll((long long)balw) - 1;
                if (lane == slot) {
                    const int wtie = (nbest > 1) || tiej[h];
                    s_xchg[i & 1][0][wave] = make_float4(wm, __int_as_float(wtie), 0.f, 0.f);
                    s_xchg[i & 1][1][wave] = make_float4(bx[h], by[h], bz[h], __int_as_float(bpos[h]));
                }
                published = true;
            }
        }
        STAMP(t3);
        __syncthreads();
        STAMP(t4);
        const float4 e = s_xchg[i & 1][0][lane & (NW - 1)];
        const float4 r = s_xchg[i & 1][1][lane & (NW - 1)];
        const float V = wave_max_dpp(e.x);
        const unsigned balv = (unsigned)__ballot(e.x == V) & ((1u << NW) - 1u);
        const int ww = __ffs(balv) - 1;
        const bool gtie = (__popc(balv) > 1) || (__builtin_amdgcn_readlane(__float_as_int(e.y), ww) != 0);
        if (V == 0.f) {                                 // workgroup-uniform: every wave read the same records
            fps_fill_zero(px, N, M, b, i + 1, tid, NW * 64, idx_out, cpos_soa, cpos_aos, n_live_out);
            break;
        }
        if (!gtie) {
            cx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r.x), ww));
            cy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r.y), ww));
            cz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r.z), ww));
            cur_pos = __builtin_amdgcn_readlane(__float_as_int(r.w), ww);
        } else {
            // rare exact tie of the maximal distance (duplicated points): lowest ORIGINAL index among all candidates
            if (tid == 0) s_win = 0xFFFFFFFFu;
            __syncthreads();
            fps_tie_search<SL>(view, ord, wave, lane, V, &s_win, [&](int h) { return mine[h] == V; });
            __syncthreads();
            cur = __builtin_amdgcn_readfirstlane((int)s_win);
            cur_pos = -1;
            cx = px[cur];
            cy = py[cur];
            cz = pz[cur];
        }
#ifdef SN2_FPS_STAMPS
        STAMP(t5);
        if (b == 0 && tid == 0) {
            g_fps_dbg[0] += t1 - t0;
            g_fps_dbg[1] += t2 - t1;
            g_fps_dbg[2] += t3 - t2;
            g_fps_dbg[3] += t4 - t3;
            g_fps_dbg[4] += t5 - t4;
            g_fps_dbg[5] += (unsigned long long)ndirty;
            g_fps_dbg[6] += 1;
            g_fps_dbg[7] += gtie ? 1 : 0;
        }
#endif
    }
}


// ------------------------------------------------------------------------------------------------------------
// Speculative bucketed FPS (exact; round 2).  fps_bucket_kernel above pays, for EVERY sample, a sequential chain of
// test -> L2 load -> update -> wave reduction -> LDS exchange -> barrier -> arg-max (1.75 us per round at N = 32768, of
// which the 16-wave barrier + exchange + selection are more than half).  But consecutive FPS samples are far apart:
// sample t only lowers distances inside the ball of radius sqrt(D_t(max)) around it, and the next maxima sit in other
// holes of the sampling.  So one SUPER-ROUND accepts up to K samples from one arg-max pass:
//   let m_0 > m_1 > ... be the bucket maxima in strictly decreasing order, c_e the point attaining m_e.  c_0 is the next
//   sample.  c_e (e >= 1) is the sample after c_0..c_{e-1}  iff  (1) m_e is strictly larger than every other bucket
//   maximum left (m_e > m_{e+1}) and than the second-largest distance of its own bucket and of the buckets of
//   c_0..c_{e-1} (their other points only ever get smaller), and (2) c_e itself is untouched by c_0..c_{e-1}:
//   sn2_d2(c_e, c_j) >= m_e for all j < e (then fminf(D(c_e), d2) == D(c_e) bit for bit).  Under (1)+(2) c_e is the
//   unique arg-max of the running distances after the first e samples were applied -- without applying them.
//   The accepted prefix c_0..c_{j-1} is then applied to the dirty buckets in ONE pass (a bucket is loaded once and
//   min-ed with the samples whose box test it fails), and the barriers, the exchange and the arg-max are paid once per
//   super-round instead of once per sample.  Exact ties anywhere (equal maxima, duplicated points) end the prefix; a tie
//   for m_0 takes the lowest-ORIGINAL-index search of the old kernel.  Indices are bit-identical to the brute-force
//   kernel and to the oracle (tests/test_gpu_geometry.py), whatever K is.
// Per super-round: all waves test + update their dirty buckets and refresh (max, second max, arg-max point) of those
// buckets in LDS; barrier; wave 0 alone extracts the K+1 largest maxima (three sorted heads per lane, DPP wave max),
// runs the acceptance tests (lane e = candidate e), emits the samples; barrier.
// Set-up, phases (A)'s push and (B), the tie search and the samples' way out are the shared statements above (view: P = 1,
// the points in the L2-resident table); the box tests of (A) and phases (C) and (D) are this kernel's own.
// ------------------------------------------------------------------------------------------------------------
template <int SPW, int NW, int K>
__global__ __launch_bounds__(NW * 64) void fps_spec_kernel(const float* __restrict__ pos, int N, int M,
                                                        const int* __restrict__ start, const int* __restrict__ order,
                                                        float4* sorted, int* __restrict__ idx_out,
                                                        float* __restrict__ cpos_soa, float* __restrict__ cpos_aos,
                                                        const unsigned* gate, unsigned* status,
                                                        const int* __restrict__ n_live, int* __restrict__ n_live_out) {
    constexpr int NBK = SPW * NW;
    constexpr int SL = (SPW + 63) / 64;                // bucket slots per lane of the owning wave
    constexpr int T = 4;                               // maxima every wave hands to the final selection
    static_assert(SPW <= 128 && NW <= 16 && K >= 2 && K <= 16 && NW * T <= 64 && SPW >= T, "limits");
    extern __shared__ __attribute__((aligned(16))) unsigned char fps_smem[];
    float4* s_pt = reinterpret_cast<float4*>(fps_smem);            // [NBK] arg-max point of the bucket: x, y, z, sorted position
    float4* s_acc = s_pt + NBK;                                    // [K] accepted samples of this super-round
    float* s_box = reinterpret_cast<float*>(s_acc + K);            // [6][NBK] bucket boxes, [component][wave][slot]
    float* s_val = s_box + 6 * NBK;                                // [NBK] largest running distance of the bucket (-1: empty)
    float* s_max2 = s_val + NBK;                                   // [NBK] >= the second largest (== s_val: treated as a tie)
    unsigned* s_q = reinterpret_cast<unsigned*>(s_max2 + NBK);     // [NBK] work queue of a super-round: bucket | samples << 11
    float2* s_top = reinterpret_cast<float2*>(s_q + NBK);          // [NW*T] per-wave maxima: (value, bucket | place << 16)
    float2* s_cand = s_top + NW * T;                               // [K + 2] the selection's candidates in order (+ the next one)
    int* s_keys = reinterpret_cast<int*>(s_cand + K + 2);          // [64] the selection's integer keys
    int* s_ctl = s_keys + 64;           // [0] accepted (0: tie search), [1] done (2: the maximum is 0), [2] tie value, [3] queue length
    unsigned* s_win = reinterpret_cast<unsigned*>(s_ctl + 4);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const fps_plot plot(pos, order, sorted, b, N);
    const float *px = plot.px, *py = plot.py, *pz = plot.pz;
    const int* ord = plot.ord;
    float4* pts = plot.pts;
    const fps_rows out = {idx_out, cpos_soa, cpos_aos, b, M};
    const fps_buckets<NW> view = {pts, N, 0, nullptr};
    if (gate) {
        // REPAIR launch behind fps_cluster_kernel (gate = that launch's control words): nothing to do unless one of its waits
        // gave up (gate[1] = the count); then every plot is sampled again by this kernel, which waits for nobody.  The running
        // distances the abandoned pass left in the sorted table go back to +inf (dead points: 0) first.
        const unsigned gave_up = __builtin_amdgcn_readfirstlane(gate[1]);
        if (gave_up == 0u) return;
        const int nlive = fps_live_count(n_live, b, N);
        for (int p = tid; p < N; p += NW * 64) fps_st_dist(pts, p, ord[p] < nlive ? INFINITY : 0.f);
        if (b == 0 && tid == 0 && status) atomicAdd(status, gave_up);      // sticky: the host reads it where it synchronises anyway
        __threadfence_block();
        __syncthreads();
    }
    const float* my_box = fps_bucket_boxes<SPW>(view, s_box, wave, lane);     // bucket of (wave, slot) = slot * NW + wave
    for (int g = tid; g < NBK; g += NW * 64) {
        s_val[g] = g * 64 < N ? INFINITY : -1.f;       // every real bucket is dirty for the first sample
        s_max2[g] = -1.f;
    }
    int cur = fps_first(start, b, N);
    // the accepted samples of the current super-round live in lanes 0..j-1 of (ax, ay, az) in EVERY wave
    float ax = px[cur], ay = py[cur], az = pz[cur];
    int j = 1, cnt = 1;
    if (tid == 0) {
        out.emit(0, ax, ay, az, cur);
        s_ctl[3] = 0;
        if (n_live_out) n_live_out[b] = M;              // unless the maximum reaches 0 first (fps_fill_zero)
    }
    if (M <= 1) return;
    __syncthreads();

    while (true) {
        STAMP(t0);
        // (A) which of this wave's buckets can change, and through which of the j samples?  lane = bucket slot.  Dirty
        // buckets go into ONE queue of the workgroup, so that (B) can deal them out evenly: with the buckets tied to their
        // waves the slowest wave had twice the average load and the others waited for it.
#pragma unroll
        for (int h = 0; h < SL; ++h) {
            const int sl = 64 * h + lane;
            unsigned sm = 0u;
            if (sl < SPW) {
                const float b0 = my_box[0 * NBK + sl], b1 = my_box[1 * NBK + sl], b2 = my_box[2 * NBK + sl];
                const float b3 = my_box[3 * NBK + sl], b4 = my_box[4 * NBK + sl], b5 = my_box[5 * NBK + sl];
                const float mx = s_val[sl * NW + wave];
                for (int k = 0; k < j; ++k) {
                    const float sx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ax), k));
                    const float sy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ay), k));
                    const float sz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(az), k));
                    if (sn2_box_d2(b0, b1, b2, b3, b4, b5, sx, sy, sz) < mx) sm |= 1u << k;
                }
            }
            fps_queue_push(s_q, &s_ctl[3], sm, sl * NW + wave, lane);
        }
        STAMP(t1);
        __syncthreads();
        // (B) the queue: new distances and, where a bucket's maximum moved, its new (max, second max, arg-max point)
        const int qn = s_ctl[3];
        fps_update_queue<false>(view, qn, wave, lane, ax, ay, az, s_q, s_val, s_max2, s_pt, b == 0 && wave == 0);
        STAMP(t2);
        __syncthreads();
        STAMP(t3);
        // (C) every wave: the T largest maxima of its own buckets, in order -> s_top
        {
            float v[SL];
            int gid[SL];
#pragma unroll
            for (int h = 0; h < SL; ++h) {
                const int sl = 64 * h + lane;
                gid[h] = sl * NW + wave;
                v[h] = sl < SPW ? s_val[gid[h]] : -2.f;
            }
#pragma unroll
            for (int t = 0; t < T; ++t) {
                float lm = v[0];
#pragma unroll
                for (int h = 1; h < SL; ++h) lm = fmaxf(lm, v[h]);
                const float m = wave_max_fused(lm);
                const int owner = __ffsll((long long)__ballot(lm == m)) - 1;
                int hh = SL - 1;
#pragma unroll
                for (int h = SL - 2; h >= 0; --h) hh = v[h] == m ? h : hh;
                const int gsel = __builtin_amdgcn_readlane(gid[0] + hh * 64 * NW, owner);
                if (lane == owner) {
#pragma unroll
                    for (int h = 0; h < SL; ++h) if (h == hh) v[h] = -3.f;
                }
                if (lane == 0) s_top[wave * T + t] = make_float2(m, __int_as_float(gsel | (t << 16)));
            }
        }
        STAMP(t3b);
        __syncthreads();
        STAMP(t4);
        // (D) wave 0: the K+1 largest of the NW*T values in order, acceptance tests, emission -- written for latency: this
        // wave runs alone while the other fifteen wait (reduction chains, one per candidate, took 5300 clocks here).
        //   ranks: every entry counts the entries above it (integer keys = value bits with the low 6 bits replaced by the
        //   entry's place, so all keys differ; 16 broadcast LDS reads + 64 compare-and-adds, no chains) and drops itself
        //   into s_cand[rank];   tests: lane 8 e + j looks at the pair (candidate e, earlier candidate j);
        //   prefix length: scalar bit arithmetic on two ballots.
        if (wave == 0) {
            static_assert(K == 8, "the acceptance tests use an 8 x 8 lane grid");
            const float2 tp = s_top[lane < NW * T ? lane : 0];
            const float val = lane < NW * T ? tp.x : -3.f;
            const int key = (__float_as_int(val) & ~63) | (63 - lane);
            s_keys[lane] = key;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            int rank = 0;
#pragma unroll
            for (int q4 = 0; q4 < 16; ++q4) {
                const int4 k4 = reinterpret_cast<const int4*>(s_keys)[q4];
                rank += (k4.x > key ? 1 : 0) + (k4.y > key ? 1 : 0) + (k4.z > key ? 1 : 0) + (k4.w > key ? 1 : 0);
            }
            if (rank <= K) s_cand[rank] = make_float2(val, tp.y);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const int e = lane >> 3, jj = lane & 7;
            const float2 ce = s_cand[e], cj = s_cand[jj], cn = s_cand[e + 1];
            const float me = ce.x;
            const int ie = __float_as_int(ce.y), ij = __float_as_int(cj.y);
            const float4 pte = s_pt[ie & 0xFFFF], ptj = s_pt[ij & 0xFFFF];
            const float m2e = s_max2[ie & 0xFFFF], m2j = s_max2[ij & 0xFFFF];
            // strictly above the next maximum even at the keys' 64-ulp resolution (then above every other entry too), own
            // bucket's second maximum below it, and its wave still has a known next value (a wave's fifth largest is unknown)
            const bool self_ok = (ie >> 16) < T - 1 && me > 0.f && (__float_as_int(me) >> 6) > (__float_as_int(cn.x) >> 6) && m2e < me;
            const bool pair_bad = jj < e && (sn2_d2(pte.x, pte.y, pte.z, ptj.x, ptj.y, ptj.z) < me || m2j >= me);
            const unsigned long long okm = __ballot(self_ok), badm = __ballot(pair_bad);
            int nj = 0;
#pragma unroll
            for (int c = 0; c < K; ++c) {
                const bool okc = ((okm >> (8 * c)) & 1ull) != 0 && ((badm >> (8 * c)) & 0xFFull) == 0;
                if (okc && nj == c) nj = c + 1;
            }
#ifdef SN2_FPS_STAMPS
            if (b == 0 && lane == 0) g_fps_dbg2[nj] += 1;
#endif
            const int rem = M - cnt;
            nj = nj > rem ? rem : nj;
            if (jj == 0 && e < nj) {
                s_acc[e] = make_float4(pte.x, pte.y, pte.z, 0.f);
                // (phase D keeps its own stores, the text of fps_rows::emit: through `out` wave 0's critical path was longer,
                // 16 x 32768 -> 1024 with 8 waves 1.3750 against 1.3703 ms, with these lines 1.3704: profiles/fps_phases)
                int* out_idx = idx_out + (size_t)b * M;
                out_idx[cnt + e] = -1 - __float_as_int(pte.w);
                cpos_soa[((size_t)b * 3 + 0) * M + cnt + e] = pte.x;
                cpos_soa[((size_t)b * 3 + 1) * M + cnt + e] = pte.y;
                cpos_soa[((size_t)b * 3 + 2) * M + cnt + e] = pte.z;
                reinterpret_cast<float4*>(cpos_aos)[(size_t)b * M + cnt + e] = make_float4(pte.x, pte.y, pte.z, 0.f);
            }
            // no candidate accepted = the maximum is not unique at the keys' resolution: the tie search needs the TRUE maximum
            // (candidate 0 is only the first of the entries that share the top key)
            float vtop = 0.f;
            if (nj == 0) vtop = wave_max_fused(val);
            const bool zero = nj == 0 && vtop <= 0.f;   // the plot's maximum is 0: no tie search, the rest is index 0
            if (lane == 0) {
                s_ctl[0] = nj;
                s_ctl[1] = zero ? 2 : ((cnt + (nj > 0 ? nj : 1) >= M) ? 1 : 0);
                s_ctl[2] = __float_as_int(vtop);
                s_ctl[3] = 0;
                *s_win = 0xFFFFFFFFu;
            }
        }
        STAMP(t5);
        __syncthreads();
        j = s_ctl[0];
        const int done = s_ctl[1];
        if (done == 2) {
            fps_fill_zero(px, N, M, b, cnt, tid, NW * 64, idx_out, cpos_soa, cpos_aos, n_live_out);
            break;
        }
#ifdef SN2_FPS_STAMPS
        STAMP(t6);
        if (b == 0 && tid == 0) {
            g_fps_dbg[0] += t1 - t0;
            g_fps_dbg[1] += t2 - t1;
            g_fps_dbg[2] += t5 - t4;
            g_fps_dbg[3] += (t3 - t2) + (t6 - t5) + (t4 - t3b);
            g_fps_dbg2[24] += t3b - t3;
            g_fps_dbg[4] += (unsigned long long)(j > 0 ? j : 1);
            g_fps_dbg[5] += (unsigned long long)qn;
            g_fps_dbg[6] += 1;
            g_fps_dbg[7] += j == 0 ? 1 : 0;
        }
#endif
        if (j > 0) {
            const float4 a = s_acc[lane < j ? lane : 0];
            ax = a.x; ay = a.y; az = a.z;
        } else {
            // exact tie of the maximal distance (duplicated points, ...): lowest ORIGINAL index among all points attaining it
            const float V = __int_as_float(s_ctl[2]);
            fps_tie_search<SL>(view, ord, wave, lane, V, s_win, [&](int h) {
                const int sl = 64 * h + lane;
                return sl < SPW && s_val[sl * NW + wave] == V;
            });
            __syncthreads();
            cur = __builtin_amdgcn_readfirstlane((int)*s_win);
            ax = px[cur]; ay = py[cur]; az = pz[cur];
            if (tid == 0) out.emit(cnt, ax, ay, az, cur);
            j = 1;
        }
        cnt += j;
        if (done) break;
    }
    __syncthreads();
    out.translate(ord, tid, NW * 64, nullptr);
}

template <int SPW, int NW, int K>
static size_t fps_spec_lds_bytes() {
    return (size_t)(SPW * NW) * 16 + (size_t)K * 16 + (size_t)(SPW * NW) * 4 * 9 + (size_t)NW * 4 * 8 + (size_t)(K + 2) * 8 + 64 * 4 + 32;
}

#ifndef SN2_FPS_K
#define SN2_FPS_K 8       // samples a super-round may accept (measured at 16 x 32768 -> 1024: 4.9 accepted on average with 8, 5.5
                          // with 12, 5.6 with 16 -- the prefix mostly ends at a candidate touched by an earlier one -- while
                          // the selection's cost grows with K)
#endif
static void launch_spatial_order(const fps_call& a, const fps_ws_parts& w) {
    launch_spatial_order(a.pos, a.B, a.N, w.order, w.sorted, w.grid, w.xchg, w.ctl, w.rank, a.nl, a.st);
}

// SPEC.  repair = this launch follows fps_cluster_kernel on the same workspace: the tables are there, and the kernel returns at
// once unless the control words say that the multi-workgroup pass gave up (the count then goes to the status word)
template <int SPW, int NW = 16>
static int launch_fps_spec(const fps_call& a, bool repair = false) {
    const fps_ws_parts w = fps_ws_carve(a.ws, a.B, a.N);
    const unsigned* gate = repair ? w.ctl : nullptr;
    unsigned* status = repair ? a.status : nullptr;
    if (!repair) launch_spatial_order(a, w);
    constexpr int K = SN2_FPS_K;
    const size_t lds = fps_spec_lds_bytes<SPW, NW, K>();
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fps_spec_kernel<SPW, NW, K>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    // (Round 4 tried the FPS waves at the highest wave priority, `s_setprio 3`: beside the feature kernels a super-round takes
    // three times as long as alone, and what the pass costs the step follows the time it is resident -- no effect, 0.7652
    // against 0.762 ms per step; round 3 had tried the opposite, the feature kernels raised: none either.)
    hipLaunchKernelGGL((fps_spec_kernel<SPW, NW, K>), dim3(a.B), dim3(NW * 64), lds, a.st, a.pos, a.N, a.M, a.start,
                       (const int*)w.order, w.sorted, a.idx, a.cs, a.ca, gate, status, a.nl, a.nlo);
    SN2_RETURN_LAUNCH();
}
// ROUND: 16 waves (sn2_fps_route), so this is the only place that names fps_bucket_kernel
template <int SPW>
static int launch_fps_round(const fps_call& a) {
    const fps_ws_parts w = fps_ws_carve(a.ws, a.B, a.N);
    launch_spatial_order(a, w);
    hipLaunchKernelGGL((fps_bucket_kernel<SPW, 16>), dim3(a.B), dim3(16 * 64), 0, a.st, a.pos, a.N, a.M, a.start,
                       (const int*)w.order, w.sorted, a.idx, a.cs, a.ca, a.nlo);
    SN2_RETURN_LAUNCH();
}

// ------------------------------------------------------------------------------------------------------------
// Multi-workgroup speculative FPS (exact; round 3).  fps_spec_kernel keeps a whole plot in ONE workgroup: 16 plots use 16
// of 256 CUs, and two thirds of a super-round are work that only scales with the buckets a workgroup owns -- the box tests
// (A) and the dirty-bucket updates (B: VALU-issue bound on one CU's four SIMDs).  Here P workgroups share a plot:
//   * bucket g (64 consecutive points of the Morton order) belongs to workgroup g % P -- interleaved, so the ~17 buckets a
//     new sample dirties spread evenly over the P workgroups; each workgroup keeps (max, second max, arg-max point) of
//     its NBL = ceil(buckets / P) buckets in LDS and runs phases (A) and (B) on them: the push and phase (B) are the statements
//     fps_spec_kernel uses (fps_queue_push, fps_update_queue), under the view <NW, P, LP>; (A)'s box tests are its own;
//   * per super-round ONE exchange through L2: wave 0 of every workgroup publishes its TP = 8 largest bucket maxima (value,
//     second max, point) and a bound on everything it did not publish as 8-byte {tag = super-round, value} granules
//     (agent-scope relaxed stores = `global_store_dwordx2 sc1`, the data is its own flag: cdna_hip_programming.md
//     Guideline 16, form R2), sweeps the granules of all P workgroups until every tag matches, and then runs the SAME
//     selection on the SAME 8 P records as its peers: every workgroup derives the same accepted samples, no broadcast;
//   * the local top-8 come from a THRESHOLD, not from reduction chains: tau = the value of the (accepted + 16)-th merged
//     candidate of the previous super-round (running distances only ever shrink, so at most that many buckets of the whole
//     plot can still reach tau); the buckets >= tau are compacted with two ballots and ranked among themselves (a dozen
//     integer compares per lane).  Whatever tau is, the result is exact: a workgroup states `bound` = tau (all its other
//     buckets are below) or its 8-th value (when more than 8 reach tau), a candidate is accepted only above every
//     workgroup's bound, and a super-round that finds nothing above the bounds lowers tau and tries again (more than 64
//     survivors: eight wave-max rounds instead of the ranking);
//   * acceptance tests, exact-tie search (lowest ORIGINAL index at the plot's TRUE maximum: two more granules per workgroup, its
//     winner and the maximum of its own buckets -- the published records are its top by 64-ulp keys only) and emitted samples are
//     those of fps_spec_kernel, bit for bit (tests/test_gpu_geometry.py holds all kernels to each other and to the oracle): the
//     search inside a workgroup is fps_tie_search, a sample leaves through fps_rows (here by way of the LDS log);
// Residency: a workgroup waits only for the P-1 peers of its plot.  Plots are handed out by a ticket counter in arrival
// order (not by blockIdx), so the peers of every resident workgroup are resident too or are the very next workgroups to
// start -- no dispatch-order assumption; every spin is bounded (`spin_limit` sweeps, then the kernel gives up, counts the
// timeout in control word 1 and exits WITHOUT writing its samples: never a hang).  Nothing guarantees that the B * P workgroups
// are resident together (another stream's or another process's kernels may hold the CUs a peer needs), so every launch of
// this kernel is followed, on the same stream, by the single-workgroup kernel as a REPAIR launch (fps_spec_kernel with
// `gate`): it returns at once when control word 1 is zero and samples every plot again when it is not -- the results are
// right either way, and the count reaches the host through `status` (sn2_fps_status).
// ------------------------------------------------------------------------------------------------------------
typedef unsigned long long fc_u64;
constexpr int FC_TP = 8;                     // records a workgroup publishes per super-round
constexpr int FC_PARITY_U64 = 512;           // granules per parity (6 * 8P record fields + P bounds + 2P tie words <= 408)
constexpr unsigned FC_SPIN_LIMIT = 1u << 18; // sweeps (~1 us each) before a wait gives up (a resident peer answers within a few)
#ifndef SN2_FC_FLAG_SLEEP
#define SN2_FC_FLAG_SLEEP 3
#endif
#ifndef SN2_FC_TAU_KEEP
#define SN2_FC_TAU_KEEP 15                   // candidates beyond the accepted ones that stay above the next threshold
#endif
static_assert(2 * 2 * FC_PARITY_U64 * 2 == FPS_XCHG_WORDS, "exchange area: two copies x two parities");
constexpr int FC_COPY_U64 = 2 * FC_PARITY_U64;      // copy 0: plain stores (same-XCD peers see them in their L2), copy 1: write-through

#ifndef SN2_FC_DUAL
#define SN2_FC_DUAL 0
#endif
constexpr bool FC_DUAL = SN2_FC_DUAL != 0;
// (FC_DUAL, measured and switched off: see below) one granule goes out TWICE: a plain store into copy 0 (it stays in this XCD's L2, where a peer on the SAME XCD finds it with an
// L1-bypassing load a few hundred clocks later) and a write-through `sc1` store into copy 1 (what a peer on ANOTHER XCD sees,
// ~1000 clocks later).  A reader takes whichever copy carries the tag first: which one it is depends on placement, the value
// does not -- both hold the same 8 bytes, each written by one store.
__device__ __forceinline__ void fc_store(fc_u64* g, unsigned epoch, unsigned v) {
    const fc_u64 x = ((fc_u64)epoch << 32) | (fc_u64)v;
    if (FC_DUAL) __hip_atomic_store(g, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_store(g + FC_COPY_U64, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// both copies of a granule -> the one that carries `epoch` (or one that does not: the caller checks the tag)
__device__ __forceinline__ fc_u64 fc_pick(fc_u64 a, fc_u64 b, unsigned epoch) { return (FC_DUAL && (unsigned)(a >> 32) == epoch) ? a : b; }
__device__ __forceinline__ fc_u64 fc_load(const fc_u64* g) {
    return __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// max over lanes 0..7 (three DPP steps inside the first row), broadcast to the wave
__device__ __forceinline__ float max_of_first8(float v) {
    asm("s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1"
        : "+v"(v));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
}

template <int SPW, int NW, int P, bool LP>
__global__ __launch_bounds__(NW * 64) void fps_cluster_kernel(const float* __restrict__ pos, int B, int N, int M,
                                                           const int* __restrict__ start, const int* __restrict__ order,
                                                           float4* sorted, int* __restrict__ idx_out,
                                                           float* __restrict__ cpos_soa, float* __restrict__ cpos_aos,
                                                           fc_u64* xchg_all, unsigned* ctl, int log_cap, int tau_keep,
                                                           unsigned spin_limit, int* __restrict__ n_live_out) {
    constexpr int NBL = SPW * NW;                      // buckets of this workgroup: local bucket lb = slot * NW + wave
    constexpr int SL = (SPW + 63) / 64;                // bucket slots per lane of the owning wave
    constexpr int VL = (NBL + 63) / 64;                // bucket values per lane of wave 0 in the selection
    constexpr int K = 8, TP = FC_TP, NE = TP * P;      // accepted per super-round, records per workgroup, merged records
    constexpr int SPWP = SPW < 64 ? SPW : 64;          // phase A: lane = (slot, sample): SPWP slots x KPL samples per pass
    constexpr int KPL = 64 / SPWP < 8 ? 64 / SPWP : 8;
    static_assert(NE <= 64 && P <= 8 && SPW <= 128 && NBL <= 2048 && NW <= 16 && 6 * NE + 3 * P <= FC_PARITY_U64, "limits");
    static_assert((SPWP & (SPWP - 1)) == 0 && TP <= 15, "slots per wave: a power of two; the record count rides in 4 bits");
    extern __shared__ __attribute__((aligned(16))) unsigned char fc_smem[];
    float4* s_pt = reinterpret_cast<float4*>(fc_smem);             // [NBL] arg-max point of the bucket: x, y, z, sorted position
    float4* s_acc = s_pt + NBL;                                    // [K] accepted samples of this super-round
    float4* s_crA = s_acc + K;                                     // [NE + 16] merged records in order: (value, second max, position, -)
    float4* s_crB = s_crA + NE + 16;                               // [NE + 16] ... (x, y, z, -)
    float4* s_ownA = s_crB + NE + 16;                              // [TP] this workgroup's published records (not re-read from memory)
    float4* s_ownB = s_ownA + TP;                                  // [TP]
    float* s_box = reinterpret_cast<float*>(s_ownB + TP);          // [6][NBL] bucket boxes, [component][wave][slot]
    float* s_val = s_box + 6 * NBL;                                // [NBL] largest running distance of the bucket (-1: empty)
    float* s_max2 = s_val + NBL;                                   // [NBL] >= the second largest (== s_val: treated as a tie)
    unsigned* s_q = reinterpret_cast<unsigned*>(s_max2 + NBL);     // [NBL] work queue: local bucket | samples << 11
    int* s_keys = reinterpret_cast<int*>(s_q + NBL);               // [64 + 8] integer keys of a ranking (+ the pad of its last quad)
    int* s_ctl = s_keys + 72;                                      // [0] accepted, [1] done, [2] tie value, [3] queue length,
                                                                   // [4] mode (0 accept, 1 tie search, 2 lower tau, 3 gave up,
                                                                   //     4 the plot's maximum is 0),
                                                                   // [5] tie winner, [7] ticket
    unsigned* s_win = reinterpret_cast<unsigned*>(s_ctl + 8);
    float4* s_log = reinterpret_cast<float4*>(s_win + 4);          // [log_cap] every sample of the plot (x, y, z, -1 - position | index):
                                                                   // written out once at the end (log_cap = 0: emitted as they come)
    float4* s_pts = s_log + log_cap;                               // LP: [NBL * 64] this workgroup's points (x, y, z, running distance):
                                                                   // the updates of phase B never leave the CU
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // which plot, which part: by XCD.  Plot c belongs to XCD c % 8; a workgroup takes the next free part of its XCD's plots (a
    // per-XCD arrival counter), so the P workgroups of a plot share an L2 and exchange through it.  HIP promises nothing about
    // placement: a workgroup whose XCD is full waits until all B * P have registered and takes the first hole left on another
    // XCD (its exchange then runs through the write-through copy: slower, same result).  ctl: [0] overflow tickets,
    // [1] timeouts, [16 + x] arrivals on XCD x.
    if (tid == 0) {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        xcc &= 7u;
        const unsigned t = atomicAdd(&ctl[16 + xcc], 1u);
        const unsigned mine = xcc < (unsigned)B ? ((unsigned)B - 1u - xcc) / 8u + 1u : 0u;     // plots of this XCD
        int slot = -1;
        if (t < mine * P) {
            slot = (int)((xcc + 8u * (t / P)) * P + t % P);
        } else {
            unsigned o = atomicAdd(&ctl[0], 1u);
            unsigned n[8];
            for (unsigned spins = 0; spins < spin_limit; ++spins) {
                unsigned sum = 0;
                for (int x = 0; x < 8; ++x) {
                    n[x] = __hip_atomic_load(&ctl[16 + x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    sum += n[x];
                }
                if (sum == (unsigned)(B * P)) {
                    for (int c = 0; c < B && slot < 0; ++c) {
                        const unsigned before = (unsigned)(c / 8) * P, nx = n[c & 7];
                        const unsigned have = nx <= before ? 0u : (nx - before < (unsigned)P ? nx - before : (unsigned)P);
                        if (o < (unsigned)P - have) slot = c * P + (int)(have + o);
                        else o -= (unsigned)P - have;
                    }
                    break;
                }
                __builtin_amdgcn_s_sleep(8);
            }
            if (slot < 0) atomicAdd(&ctl[1], 1u);
        }
        s_ctl[7] = slot;
    }
    __syncthreads();
    const int ticket = s_ctl[7];
    if (ticket < 0) return;
    const int b = ticket / P, part = ticket - b * P;
    const bool use_log = log_cap >= M;
    const fps_plot plot(pos, order, sorted, b, N);
    const float *px = plot.px, *py = plot.py, *pz = plot.pz;
    const int* ord = plot.ord;
    const fps_rows out = {idx_out, cpos_soa, cpos_aos, b, M};
    const fps_buckets<NW, P, LP> view = {plot.pts, N, part, s_pts};
    fc_u64* xchg = xchg_all + (size_t)b * (2 * FC_COPY_U64);
    const float* my_box = fps_bucket_boxes<SPW>(view, s_box, wave, lane);     // (LP: and the workgroup's points -> s_pts)
    for (int lb = tid; lb < NBL; lb += NW * 64) {
        s_val[lb] = view.pos(lb, 0) < N ? INFINITY : -1.f;          // every real bucket is dirty for the first sample
        s_max2[lb] = -1.f;
    }
    int cur = fps_first(start, b, N);
    // the accepted samples of the current super-round: s_acc[0..j-1], and lanes 0..j-1 of (ax, ay, az) in EVERY wave
    float ax = px[cur], ay = py[cur], az = pz[cur];
    int j = 1, cnt = 1;
    unsigned epoch = 0;
    float tau = -1.f;                                  // wave 0's threshold for the next selection
    bool gave_up = false;                              // a wait ran out: leave without writing (the repair launch samples the plot)
    // one sample of the plot: into the LDS log where the plot's samples fit (they leave together at the end), else out at once
    auto emit = [&](int at, float x, float y, float z, int code) {
        if (use_log) s_log[at] = make_float4(x, y, z, __int_as_float(code));
        else out.emit(at, x, y, z, code);
    };
    if (tid == 0) {
        if (part == 0) emit(0, ax, ay, az, cur);
        if (part == 0 && n_live_out) n_live_out[b] = M;            // unless the maximum reaches 0 first (mode 4)
        s_acc[0] = make_float4(ax, ay, az, 0.f);
        s_ctl[3] = 0;
    }
    if (M <= 1 && !use_log) return;
    __syncthreads();
    // phase A: lane = (slot asl, sample group akk), slot-major so that the hits of one slot are contiguous ballot bits
    const int asl = lane / KPL, akk = lane & (KPL - 1);

#ifdef SN2_FC_STAMPS
    unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned n_rounds = 0, n_acc = 0, n_fb = 0, n_m1 = 0, n_m2 = 0, n_surv = 0, n_spins = 0;
#define FCSTAMP(var) unsigned long long var; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var)::"memory")
#else
#define FCSTAMP(var)
#endif
    while (M > 1) {
        ++epoch;
        fc_u64* xg = xchg + (epoch & 1u) * FC_PARITY_U64;
        FCSTAMP(t0);
        // (A) which of this wave's buckets can change, and through which of the j samples?  lane = (slot, sample): every lane
        // runs ONE box test per pass of KPL samples (a lane per slot ran j of them in sequence: 1100 clocks whatever SPW was)
#pragma unroll
        for (int h = 0; h < SL; ++h) {
            const int sl = 64 * h + asl;
            const bool slot_ok = asl < SPWP && sl < SPW;
            float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f, b4 = 0.f, b5 = 0.f, mx = -1.f;
            if (slot_ok) {
                b0 = my_box[0 * NBL + sl]; b1 = my_box[1 * NBL + sl]; b2 = my_box[2 * NBL + sl];
                b3 = my_box[3 * NBL + sl]; b4 = my_box[4 * NBL + sl]; b5 = my_box[5 * NBL + sl];
                mx = s_val[sl * NW + wave];
            }
            unsigned sm = 0u;
            for (int k0 = 0; k0 < j; k0 += KPL) {
                const int k = k0 + akk;
                bool hit = false;
                if (slot_ok && k < j) {
                    const float4 sp = s_acc[k];
                    hit = sn2_box_d2(b0, b1, b2, b3, b4, b5, sp.x, sp.y, sp.z) < mx;
                }
                const unsigned long long hb = __ballot(hit);
                sm |= ((unsigned)(hb >> ((asl * KPL) & 63)) & ((1u << KPL) - 1u)) << k0;     // the KPL hits of this lane's slot
            }
            if (akk != 0 || !slot_ok) sm = 0u;           // one lane per slot pushes
            fps_queue_push(s_q, &s_ctl[3], sm, sl * NW + wave, lane);
        }
        FCSTAMP(t1);
        __syncthreads();
        FCSTAMP(t2);
        // (B) the queue: new distances and, where a bucket's maximum moved, its new (max, second max, arg-max point)
        const int qn = s_ctl[3];
        // (256 and more buckets per workgroup: the points are never in LDS, and the selection's registers set the occupancy)
        fps_update_queue<(NBL >= 256)>(view, qn, wave, lane, ax, ay, az, s_q, s_val, s_max2, s_pt, false);
        FCSTAMP(t3);
        __syncthreads();
        FCSTAMP(t4);
        // (C + D) wave 0: this workgroup's records, the exchange, the selection (identical in all P workgroups).  ONE wave issues
        // an instruction every 4-5 clocks whatever its kind: this block is written for instruction count.
        if (wave == 0) {
            // one record leaves the workgroup: as granules for the peers and into LDS for ourselves
            auto publish = [&](int r, float val, float m2, const float4& pt) {
                fc_u64* rg = xg + part * TP + r;       // record (part, r), field f at xg[f * NE + part * TP + r]
                fc_store(rg + 0 * NE, epoch, __float_as_uint(val));
                fc_store(rg + 1 * NE, epoch, __float_as_uint(m2));
                fc_store(rg + 2 * NE, epoch, __float_as_uint(pt.w));
                fc_store(rg + 3 * NE, epoch, __float_as_uint(pt.x));
                fc_store(rg + 4 * NE, epoch, __float_as_uint(pt.y));
                fc_store(rg + 5 * NE, epoch, __float_as_uint(pt.z));
                s_ownA[r] = make_float4(val, m2, pt.w, 0.f);
                s_ownB[r] = make_float4(pt.x, pt.y, pt.z, 0.f);
            };
            float v[VL], m2v[VL];
            float4 ptv[VL];
            bool surv[VL];
            unsigned long long bal[VL];
            int n = 0;
#pragma unroll
            for (int h = 0; h < VL; ++h) {
                const int lb = 64 * h + lane;
                v[h] = lb < NBL ? s_val[lb] : -1.f;
            }
#pragma unroll
            for (int h = 0; h < VL; ++h) {
                surv[h] = v[h] >= tau && v[h] >= 0.f;
                bal[h] = __ballot(surv[h]);
                n += __popcll(bal[h]);
                m2v[h] = -1.f;
                ptv[h] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (surv[h] && n <= 64) {              // what a published record carries (read now: off the ranking's path)
                    m2v[h] = s_max2[64 * h + lane];
                    ptv[h] = s_pt[64 * h + lane];
                }
            }
            float bound = tau;                         // every bucket of this workgroup that is not published is below `bound`
            int npub = n < TP ? n : TP;                // records this workgroup publishes (the peers ignore the rest of its area)
            if (n <= 64) {
                // the survivors ranked among themselves: integer keys = value bits with the low 6 bits replaced by the
                // survivor's place (all keys differ), every survivor counts the keys above its own
                int key[VL], rank[VL];
                if (n > TP && lane < 4) s_keys[n + lane] = INT_MIN;
                int base = 0;
#pragma unroll
                for (int h = 0; h < VL; ++h) {
                    key[h] = INT_MAX;
                    rank[h] = 0;
                    if (surv[h]) {
                        const int si = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal[h] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal[h], 0u));
                        key[h] = (__float_as_int(v[h]) & ~63) | (63 - si);
                        rank[h] = si;                  // n <= TP: every survivor is published, in any order (the merge ranks them)
                        if (n > TP) s_keys[si] = key[h];
                    }
                    base += __popcll(bal[h]);
                }
                if (n > TP) {
#pragma unroll
                    for (int h = 0; h < VL; ++h) rank[h] = 0;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
#pragma unroll 1
                    for (int q4 = 0; q4 < (n + 3) / 4; ++q4) {
                        const int4 k4 = reinterpret_cast<const int4*>(s_keys)[q4];
#pragma unroll
                        for (int h = 0; h < VL; ++h)
                            rank[h] += (k4.x > key[h] ? 1 : 0) + (k4.y > key[h] ? 1 : 0) + (k4.z > key[h] ? 1 : 0) + (k4.w > key[h] ? 1 : 0);
                    }
                }
                float b7 = -1.f;
#pragma unroll
                for (int h = 0; h < VL; ++h) {
                    if (surv[h] && rank[h] < TP) publish(rank[h], v[h], m2v[h], ptv[h]);
                    if (surv[h] && rank[h] == TP - 1) b7 = v[h];
                }
                if (n > TP) {                          // the unpublished survivors are <= the TP-th value
                    const int l7 = __ffsll((long long)__ballot(b7 >= 0.f)) - 1;
                    bound = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b7), l7));
                }
            } else {
                // more than 64 buckets reach tau (the first super-rounds, or after tau was lowered): TP wave-max rounds
                float pval = -1.f;
                int plb = 0;
                npub = 0;
#pragma unroll 1
                for (int t = 0; t < TP; ++t) {
                    float lm = v[0];
#pragma unroll
                    for (int h = 1; h < VL; ++h) lm = fmaxf(lm, v[h]);
                    const float m = wave_max_fused(lm);
                    const int owner = __ffsll((long long)__ballot(lm == m)) - 1;
                    int hh = VL - 1;
#pragma unroll
                    for (int h = VL - 2; h >= 0; --h) hh = v[h] == m ? h : hh;
                    const int lbsel = __builtin_amdgcn_readlane(64 * hh + lane, owner);
                    if (lane == owner) {
#pragma unroll
                        for (int h = 0; h < VL; ++h) if (h == hh) v[h] = -3.f;
                    }
                    if (lane == t) {
                        pval = m;
                        plb = lbsel;
                    }
                    if (m >= 0.f) {
                        npub = t + 1;
                        bound = m;
                    }
                }
                if (lane < npub) publish(lane, pval, s_max2[plb], s_pt[plb]);
            }
            // the header: the bound (its low 4 bits give way to the record count: only bits 6 and up are ever compared)
            if (lane == 0) fc_store(xg + 6 * NE + part, epoch, (__float_as_uint(bound) & ~15u) | (unsigned)npub);
            // sweep: lane l < NE takes record l of the merged set and its workgroup's header, lane l < P also header l (for the
            // bounds); our own records come from LDS.  A record counts once its header and -- if the header lists it -- its
            // six fields carry this super-round's tag.
            fc_u64 x[6] = {0, 0, 0, 0, 0, 0}, hw = 0, hb = 0;
            const int rw = lane / TP, rr = lane - rw * TP;
            const bool peer_rec = lane < NE && rw != part, peer_bnd = lane < P && lane != part;
            bool failed = false;
            FCSTAMP(t5);
#ifdef SN2_FC_STAMPS
            n_surv += n; n_fb += n > 64 ? 1 : 0;
#endif
            unsigned spins = 0;
            for (;;) {
                bool ok = true;
                if (peer_rec) {
                    const fc_u64 h0 = FC_DUAL ? fc_load(xg + 6 * NE + rw) : 0ull, h1 = fc_load(xg + FC_COPY_U64 + 6 * NE + rw);
                    fc_u64 y[6];
#pragma unroll
                    for (int f = 0; f < 6; ++f) {
                        x[f] = FC_DUAL ? fc_load(xg + f * NE + lane) : 0ull;
                        y[f] = fc_load(xg + FC_COPY_U64 + f * NE + lane);
                    }
                    hw = fc_pick(h0, h1, epoch);
#pragma unroll
                    for (int f = 0; f < 6; ++f) x[f] = fc_pick(x[f], y[f], epoch);
                    ok = (unsigned)(hw >> 32) == epoch;
                    if (rr < (int)((unsigned)hw & 15u)) {
#pragma unroll
                        for (int f = 0; f < 6; ++f) ok &= (unsigned)(x[f] >> 32) == epoch;
                    }
                }
                if (peer_bnd) {
                    hb = fc_pick(FC_DUAL ? fc_load(xg + 6 * NE + lane) : 0ull, fc_load(xg + FC_COPY_U64 + 6 * NE + lane), epoch);
                    ok &= (unsigned)(hb >> 32) == epoch;
                }
                if (__ballot(!ok) == 0ull) break;
                if (++spins > spin_limit) {
                    failed = true;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            FCSTAMP(t6);
#ifdef SN2_FC_STAMPS
            n_spins += spins;
#endif
            float4 rA = make_float4(__uint_as_float((unsigned)x[0]), __uint_as_float((unsigned)x[1]), __uint_as_float((unsigned)x[2]), 0.f);
            float4 rB = make_float4(__uint_as_float((unsigned)x[3]), __uint_as_float((unsigned)x[4]), __uint_as_float((unsigned)x[5]), 0.f);
            bool valid = peer_rec && rr < (int)((unsigned)hw & 15u);
            if (lane < NE && !peer_rec && rr < npub) {
                rA = s_ownA[rr];
                rB = s_ownB[rr];
                valid = true;
            }
            const float val = rA.x;
            const unsigned long long vb = __ballot(valid);
            const int nvalid = __popcll(vb);
            // the valid records ranked by value (keys as above): rank = place in the merged order
            const int key = (__float_as_int(val) & ~63) | (63 - lane);
            if (lane < 4) s_keys[nvalid + lane] = INT_MIN;
            if (valid) s_keys[__builtin_amdgcn_mbcnt_hi((unsigned)(vb >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)vb, 0u))] = key;
            if (lane < 9) s_crA[nvalid + lane] = make_float4(-1.f, -1.f, 0.f, 0.f);       // sentinels behind the valid records
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            const float Ub = max_of_first8(lane < P ? __uint_as_float((lane == part ? __float_as_uint(bound) : (unsigned)hb) & ~15u) : -1.f);
            __builtin_amdgcn_wave_barrier();
            int rank = 0;
#pragma unroll 2
            for (int q4 = 0; q4 < (nvalid + 3) / 4; ++q4) {
                const int4 k4 = reinterpret_cast<const int4*>(s_keys)[q4];
                rank += (k4.x > key ? 1 : 0) + (k4.y > key ? 1 : 0) + (k4.z > key ? 1 : 0) + (k4.w > key ? 1 : 0);
            }
            if (valid) {
                s_crA[rank] = rA;
                s_crB[rank] = rB;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // acceptance tests: lane 8 e + jj looks at the pair (candidate e, earlier candidate jj)
            const int e = lane >> 3, jj = lane & 7;
            const float4 Ae = s_crA[e], Be = s_crB[e], Aj = s_crA[jj], Bj = s_crB[jj], An = s_crA[e + 1];
            const float me = Ae.x;
            const float nxt = fmaxf(An.x, Ub);          // the next known maximum, or what an unpublished bucket may still hold
            const bool self_ok = me > 0.f && (__float_as_int(me) >> 6) > (__float_as_int(nxt) >> 6) && Ae.y < me;
            const bool pair_bad = jj < e && (sn2_d2(Be.x, Be.y, Be.z, Bj.x, Bj.y, Bj.z) < me || Aj.y >= me);
            // candidate c stands iff bit 8c of okm is set and byte c of badm is empty; accepted = the leading run of those
            const unsigned long long okm = __ballot(self_ok);
            unsigned long long badm = __ballot(pair_bad);
            badm |= badm >> 4;
            badm |= badm >> 2;
            badm |= badm >> 1;
            const unsigned long long stand = okm & ~badm & 0x0101010101010101ull;
            const unsigned long long fell = ~stand & 0x0101010101010101ull;
            int nj = fell ? __builtin_ctzll(fell) >> 3 : K;
            const int rem = M - cnt;
            nj = nj > rem ? rem : nj;
            if (jj == 0 && e < nj) {
                s_acc[e] = make_float4(Be.x, Be.y, Be.z, 0.f);
                if (part == 0) emit(cnt + e, Be.x, Be.y, Be.z, -1 - __float_as_int(Ae.z));
            }
            int mode = 0;
            float vtop = 0.f;
            if (nj == 0) {
                // nothing accepted: either the maximum is not unique at the keys' resolution (exact-tie search for the TRUE
                // maximum) or nothing reached the bounds (lower the threshold and select again)
                if (nvalid > 0) {
                    vtop = wave_max_fused(valid ? val : -1.f);
                    // the largest record at 0 = the plot's maximum is 0, the rest is index 0.  (A record of 0 is only published
                    // with tau <= 0, i.e. every workgroup's top eight by key: a larger value left out of them would lie in the
                    // 64-ulp key class of 0 -- a positive squared distance below 64 denormal ulps, which no coordinates give.)
                    mode = vtop <= 0.f ? 4 : 1;
                } else {
                    mode = 2;
                }
            }
            // the next threshold: the candidate SN2_FC_TAU_KEEP places behind the accepted ones stays above it.  Only buckets
            // that reached THIS threshold are known, so a list that is too short is extended downwards by its own average
            // spacing (any value is exact -- see the header comment --, a good one keeps a dozen survivors per super-round:
            // few enough to rank in a few compares, enough that a super-round never runs out of candidates)
            tau = -1.f;
            if (mode != 2 && nvalid >= 2) {
                const int want = nj + tau_keep;
                if (want <= nvalid - 1) {
                    tau = s_crA[want].x;
                } else {
                    const float v0 = s_crA[0].x, vl = s_crA[nvalid - 1].x;
                    tau = vl - (v0 - vl) / (float)(nvalid - 1) * (float)(want - (nvalid - 1));
                }
            }
            if (failed) mode = 3;
            if (lane == 0) {
                if (failed) atomicAdd(&ctl[1], 1u);
                s_ctl[0] = nj;
                s_ctl[1] = (mode >= 3 || cnt + (mode == 0 ? nj : (mode == 1 ? 1 : 0)) >= M) ? 1 : 0;
                s_ctl[2] = __float_as_int(vtop);
                s_ctl[3] = 0;
                s_ctl[4] = mode;
                s_win[0] = 0xFFFFFFFFu;                 // the tie search's winner (atomicMin) and this workgroup's maximum (atomicMax)
                s_win[1] = 0u;
            }
#ifdef SN2_FC_STAMPS
            FCSTAMP(t7);
            acc[0] += t1 - t0; acc[1] += t2 - t1; acc[2] += t3 - t2; acc[3] += t4 - t3; acc[4] += t5 - t4; acc[5] += t6 - t5;
            acc[6] += t7 - t6;
            n_rounds += 1; n_acc += nj; n_m1 += mode == 1; n_m2 += mode == 2;
#endif
        }
        FCSTAMP(t8);
        __syncthreads();
#ifdef SN2_FC_STAMPS
        { FCSTAMP(t9); acc[7] += t9 - t8; }
#endif
        j = s_ctl[0];
        int done = s_ctl[1];
        const int mode = s_ctl[4];
        if (mode == 3) {
            gave_up = true;
            break;
        }
        if (mode == 4) {
            // every workgroup of the plot derived this from the same records: all leave, part 0 writes the rest (fps_fill_zero)
            if (part == 0) {
                const float x0 = px[0], y0 = py[0], z0 = pz[0];
                for (int i = cnt + tid; i < M; i += NW * 64) emit(i, x0, y0, z0, 0);
                if (tid == 0 && n_live_out) n_live_out[b] = cnt;
            }
            break;
        }
        if (mode == 0) {
            const float4 a = s_acc[lane < j ? lane : 0];
            ax = a.x; ay = a.y; az = a.z;
        } else if (mode == 1) {
            // exact tie of the maximal distance: lowest ORIGINAL index among all points of the plot attaining it.  The maximum is
            // NOT the largest published record: a workgroup publishes its top records by their 64-ulp keys, so a bucket it left out
            // may hold a value above all of them inside the top key's class (distinct points at nearly equal distances: a rotated
            // lattice of ground points gives hundreds).  Every workgroup therefore searches at its OWN true maximum and states it
            // beside its winner; the plot's maximum is the largest of those.
            float lmx = 0.f;
#pragma unroll
            for (int h = 0; h < SL; ++h) {
                const int sl = 64 * h + lane;
                if (sl < SPW) lmx = fmaxf(lmx, s_val[sl * NW + wave]);          // (empty buckets hold -1)
            }
            lmx = wave_max_fused(lmx);
            if (lane == 0) atomicMax(s_win + 1, __float_as_uint(lmx));           // non-negative floats order as their bits
            __syncthreads();
            const float V = __uint_as_float(s_win[1]);
            fps_tie_search<SL>(view, ord, wave, lane, V, s_win, [&](int h) {
                const int sl = 64 * h + lane;
                return sl < SPW && s_val[sl * NW + wave] == V;
            });
            __syncthreads();
            if (wave == 0) {
                fc_u64* tg = xg + 6 * NE + P;           // two tie words per workgroup: its winner, its maximum
                if (lane == 0) {
                    fc_store(tg + part, epoch, s_win[0]);
                    fc_store(tg + P + part, epoch, s_win[1]);
                }
                fc_u64 tw = 0, tv = 0;
                bool failed = false;
                for (unsigned spins = 0;;) {
                    bool ok = true;
                    if (lane < P) {
                        tw = fc_pick(FC_DUAL ? fc_load(tg + lane) : 0ull, fc_load(tg + FC_COPY_U64 + lane), epoch);
                        tv = fc_pick(FC_DUAL ? fc_load(tg + P + lane) : 0ull, fc_load(tg + FC_COPY_U64 + P + lane), epoch);
                        ok = (unsigned)(tw >> 32) == epoch && (unsigned)(tv >> 32) == epoch;
                    }
                    if (__ballot(!ok) == 0ull) break;
                    if (++spins > spin_limit) {
                        failed = true;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
                // the plot's maximum = the largest of the workgroups' (as bits), the winner = the lowest index among those that hold it
                const unsigned gmax = ~wave_min_u32_dpp(lane < P ? ~(unsigned)tv : 0xFFFFFFFFu);
                const unsigned w = wave_min_u32_dpp(lane < P && (unsigned)tv == gmax ? (unsigned)tw : 0xFFFFFFFFu);
                if (lane == 0) {
                    s_ctl[5] = (int)w;
                    if (failed || w == 0xFFFFFFFFu) {
                        atomicAdd(&ctl[1], 1u);
                        s_ctl[4] = 3;
                    } else {
                        s_acc[0] = make_float4(px[w], py[w], pz[w], 0.f);
                    }
                }
            }
            __syncthreads();
            if (s_ctl[4] == 3) {
                gave_up = true;
                break;
            }
            cur = __builtin_amdgcn_readfirstlane(s_ctl[5]);
            ax = px[cur]; ay = py[cur]; az = pz[cur];
            if (tid == 0 && part == 0) emit(cnt, ax, ay, az, cur);
            j = 1;
        } else {
            j = 0;                                      // mode 2: no sample this super-round, the threshold was lowered
        }
        cnt += j;
        if (done) break;
    }
#ifdef SN2_FC_STAMPS
    if (ticket == 0 && tid == 0) {
        for (int i = 0; i < 8; ++i) ctl[2 + i] = (unsigned)(acc[i] >> 4);       // 16-clock units
        ctl[10] = n_rounds; ctl[11] = n_acc; ctl[12] = n_fb; ctl[13] = n_m1 | (n_m2 << 16); ctl[14] = n_surv; ctl[15] = n_spins;
    }
#endif
    // the samples leave: sorted positions -> original indices (kept out of the loop: the loads would sit on wave 0's critical path)
    // (after a give-up the log holds `cnt` samples and uninitialised LDS behind them: nothing is translated, nothing written)
    if (part != 0 || gave_up) return;
    __syncthreads();
    out.translate(ord, tid, NW * 64, use_log ? s_log : nullptr);
}

static bool fps_cluster_lds_points = getenv("SN2_FC_NO_LDS_POINTS") == nullptr;     // (diagnostic switches)
static int fps_cluster_tau_keep = getenv("SN2_FC_TAU_KEEP") ? atoi(getenv("SN2_FC_TAU_KEEP")) : SN2_FC_TAU_KEEP;
static unsigned fps_cluster_spin_limit = getenv("SN2_FC_SPIN_LIMIT") ? (unsigned)strtoul(getenv("SN2_FC_SPIN_LIMIT"), nullptr, 0) : FC_SPIN_LIMIT;
// tests only: how many sweeps a wait of fps_cluster_kernel makes before it gives up (0 = back to the default); a tiny limit
// makes every exchange give up, which is how tests/test_gpu_geometry.py exercises the repair launch
extern "C" int sn2_debug_fps_spin_limit(unsigned sweeps) {
    fps_cluster_spin_limit = sweeps ? sweeps : FC_SPIN_LIMIT;
    return 0;
}
// dynamic LDS of fps_cluster_kernel: its tables and records, the plot's samples until the end when they fit (16 B each), and
// -- `points` -- the workgroup's own points (64 KB at 8 x 8 x 8) when they fit beside the rest: phase B then never waits for L2
static int fps_cluster_log_cap(int M) { return M <= 4096 ? M : 0; }
static constexpr bool fps_cluster_points_fit(int nbl) { return (size_t)nbl * 64 * 16 <= 96 * 1024; }
static size_t fps_cluster_lds(int nbl, int P, int log_cap, bool points) {
    return (size_t)nbl * 16 + 8 * 16 + 2 * (size_t)(FC_TP * P + 16) * 16 + 2 * FC_TP * 16 + (size_t)nbl * 4 * 9 + 72 * 4 + 8 * 4 + 16 +
           (size_t)log_cap * 16 + (points ? (size_t)nbl * 64 * 16 : 0);
}

// Routes (include/strata_hip.h).  Many small plots (the parcel loop's level 2: 256 .. 512 plots of 2 500 points -> 625): the
// bucketed kernel has 40 buckets to prune among and takes 2 us per sample with 16 waves per plot (1.1 ms at half of every CU's
// wave slots); the brute-force kernel with the plot's points in the registers of FOUR waves takes the whole plot per round and
// is shorter.  N <= 131 072: 128 bucket slots per wave, the largest single-workgroup kernel -- larger plots are SN2_ELIMIT with
// or without a workspace: the brute-force kernels end at 32 768 points.
static bool fps_many_small(int B, int N) { return N <= 4096 && B > 32; }
extern "C" int sn2_fps_fills_ws(int B, int N, int M) {
    return N > 2048 && !fps_many_small(B, N) && M > 16 && ((long)B * N) % 4 == 0 && N <= 131072;
}
// the template rung: the smallest `lo` * 2^k slots (points) per wave at which nw waves hold the plot's 64-point buckets
static int fps_rung(int buckets, int nw, int lo) {
    while (lo * nw < buckets) lo *= 2;
    return lo;
}

// THE route of sn2_fps_live, decided before any launch (include/strata_hip.h, sn2_fps_route, states the rule): host arithmetic
extern "C" int sn2_fps_route(int B, int N, int M, int waves, int have_ws, int cus, sn2_fps_route_t* out) {
    if (!out || B <= 0 || N <= 0 || M <= 0 || M > N) return SN2_EINVAL;
    sn2_fps_route_t r = {SN2_FPS_FORM_SPEC, 16, 1};         // the request: one workgroup of nw waves per plot, or p workgroups
    switch (waves) {
    case 0: case 16: break;
    case 1: r.form = SN2_FPS_FORM_ROUND; break;             // round 1's kernel; cross-checks and timing comparisons
    case 8: case 4: r.nw = waves; break;
    case 34: case 36: case 40: r.p = waves - 32; break;
    case 66: case 68: case 72: r.nw = 8, r.p = waves - 64; break;
    default: return SN2_EINVAL;
    }
    const int buckets = sn2_cdiv(N, 64);
    r.fills_ws = have_ws && sn2_fps_fills_ws(B, N, M);
    if (!r.fills_ws) {                  // the plot in the registers of one workgroup: rung = points per thread, 256 or 1024 threads
        const bool small = N <= 1024, many = N > 2048 && fps_many_small(B, N);
        r = {SN2_FPS_FORM_BRUTE, small || many ? 4 : 16, 1, many ? 16 : fps_rung(buckets, small ? 4 : 16, small ? 1 : 2)};
        if (r.rung > 32) return SN2_ELIMIT;
        *out = r;
        return 0;
    }
    // bucketed (exact, see above): up to 128 bucket slots per wave = 131 072 points per plot.
    // p workgroups per plot: all B * p resident at once, at least two buckets per wave; else the single-workgroup kernel, 16 waves
    auto fits = [&](int p, int nw) { return (long)B * p <= cus && buckets >= 2 * p * nw && buckets <= 512 * p; };
    // 0 = the shortest pass: several workgroups per plot wherever that fits (measured at 16 x 32 768 -> 1024: 8 workgroups of 8
    // waves 0.87 ms, 4 of 8 0.99, the single workgroup 1.24; scripts/time_fps_cluster.py)
    for (int p = 8; waves == 0 && p >= 2 && r.p == 1; p >>= 1)
        if (fits(p, 8)) r.nw = 8, r.p = p;
    if (r.p > 1 && !fits(r.p, r.nw)) r.nw = 16, r.p = 1;
    if (r.p > 1) {
        r.form = SN2_FPS_FORM_CLUSTER;
        r.rung = fps_rung(sn2_cdiv(buckets, r.p), r.nw, 2);
        // (64 slots x 16 waves = 16 bucket values per lane of the selecting wave: spills at 128 VGPRs)
        if (r.rung > (r.nw <= 8 ? 64 : 32)) return SN2_ELIMIT;
        r.lds_points = fps_cluster_points_fit(r.rung * r.nw) && fps_cluster_lds_points &&
                       fps_cluster_lds(r.rung * r.nw, r.p, fps_cluster_log_cap(M), true) <= 150 * 1024;
        // the repair launch: B workgroups of the 16-wave kernel that read control word 1 and leave -- unless a wait of the pass
        // gave up (its workgroups are not guaranteed to be resident together), in which case they sample every plot again
        r.repair = fps_rung(buckets, 16, 4);
    } else {
        // waves = 8: half the waves per plot.  Alone the pass is 9 % slower (1.37 vs 1.26 ms at 32 x 32 768: fewer loads in
        // flight), but it leaves half of its CU's wave slots to whatever else runs: beside the feature pass of a pipelined
        // training loop the STEP is 2.4 % shorter (0.918 vs 0.940 ms; 4 waves: 2.07 ms alone, 0.922 ms per step).
        // waves = 4 (plots of at most 16 384 points): half the wave slots again, for passes that share the chip with MANY other
        // workgroups (the parcel loop: 512 plots per launch = two FPS workgroups per CU); larger plots take the 8-wave kernel
        // (four waves at 32 768 points -- launch_fps_spec<128, 4> -- were measured in the training loop: 0.773 against 0.769 ms
        // per step with eight; not instantiated), and above 32 768 points there are 16 waves or none
        if (r.nw == 4 && N > 16384) r.nw = 8;
        if (r.nw == 8 && N > 32768) r.nw = 16;
        r.rung = fps_rung(buckets, r.nw, r.nw == 16 ? 4 : r.nw == 8 ? 8 : 32);
    }
    *out = r;
    return 0;
}

// One launcher per form: the route's integers -> the template instantiation, and nothing else
static int launch_fps_brute(const fps_call& a, const sn2_fps_route_t& r) {
    switch (r.nw * 100 + r.rung) {
    case 401: return launch_fps<1, 256>(a);
    case 402: return launch_fps<2, 256>(a);
    case 404: return launch_fps<4, 256>(a);
    case 416: return launch_fps<16, 256>(a);
    case 1602: return launch_fps<2, 1024>(a);
    case 1604: return launch_fps<4, 1024>(a);
    case 1608: return launch_fps<8, 1024>(a);
    case 1616: return launch_fps<16, 1024>(a);
    case 1632: return launch_fps<32, 1024, true>(a);
    default: return SN2_ELIMIT;
    }
}
// SPEC, ROUND (16 waves only) and the repair launch behind CLUSTER (SPEC, 16 waves, gated by the workspace's control words)
template <int SPW>
static int launch_fps_16(const fps_call& a, bool spec, bool repair) {
    return spec ? launch_fps_spec<SPW>(a, repair) : launch_fps_round<SPW>(a);
}
static int launch_fps_single(const fps_call& a, int nw, int spw, bool spec, bool repair) {
    switch (nw * 1000 + spw) {
    case 4032: return launch_fps_spec<32, 4>(a);
    case 4064: return launch_fps_spec<64, 4>(a);
    case 8008: return launch_fps_spec<8, 8>(a);
    case 8016: return launch_fps_spec<16, 8>(a);
    case 8032: return launch_fps_spec<32, 8>(a);
    case 8064: return launch_fps_spec<64, 8>(a);
    case 16004: return launch_fps_16<4>(a, spec, repair);
    case 16008: return launch_fps_16<8>(a, spec, repair);
    case 16016: return launch_fps_16<16>(a, spec, repair);
    case 16032: return launch_fps_16<32>(a, spec, repair);
    case 16064: return launch_fps_16<64>(a, spec, repair);
    case 16128: return launch_fps_16<128>(a, spec, repair);
    default: return SN2_ELIMIT;
    }
}
template <int SPW, int NW, int P>
static int launch_fps_cluster(const fps_call& a, const sn2_fps_route_t& r) {
    const fps_ws_parts w = fps_ws_carve(a.ws, a.B, a.N);
    launch_spatial_order(a, w);
    const int log_cap = fps_cluster_log_cap(a.M);
    auto launch = [&](auto lp) {
        constexpr bool LP = decltype(lp)::value;
        const size_t lds = fps_cluster_lds(SPW * NW, P, log_cap, LP);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fps_cluster_kernel<SPW, NW, P, LP>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((fps_cluster_kernel<SPW, NW, P, LP>), dim3(a.B * P), dim3(NW * 64), lds, a.st, a.pos, a.B, a.N, a.M, a.start,
                           (const int*)w.order, w.sorted, a.idx, a.cs, a.ca, reinterpret_cast<fc_u64*>(w.xchg), w.ctl, log_cap,
                           fps_cluster_tau_keep, fps_cluster_spin_limit, a.nlo);
        SN2_RETURN_LAUNCH();
    };
    if constexpr (fps_cluster_points_fit(SPW * NW)) {
        if (r.lds_points) return launch(std::true_type{});
    }
    return launch(std::false_type{});
}
template <int NW, int P>
static int launch_fps_cluster_slots(const fps_call& a, const sn2_fps_route_t& r) {
    switch (r.rung) {
    case 2: return launch_fps_cluster<2, NW, P>(a, r);
    case 4: return launch_fps_cluster<4, NW, P>(a, r);
    case 8: return launch_fps_cluster<8, NW, P>(a, r);
    case 16: return launch_fps_cluster<16, NW, P>(a, r);
    case 32: return launch_fps_cluster<32, NW, P>(a, r);
    case 64:
        if constexpr (NW <= 8) return launch_fps_cluster<64, NW, P>(a, r);
    }
    return SN2_ELIMIT;
}
static int launch_fps_cluster_form(const fps_call& a, const sn2_fps_route_t& r) {
    switch (r.nw * 100 + r.p) {
    case 1602: return launch_fps_cluster_slots<16, 2>(a, r);
    case 1604: return launch_fps_cluster_slots<16, 4>(a, r);
    case 1608: return launch_fps_cluster_slots<16, 8>(a, r);
    case 802: return launch_fps_cluster_slots<8, 2>(a, r);
    case 804: return launch_fps_cluster_slots<8, 4>(a, r);
    case 808: return launch_fps_cluster_slots<8, 8>(a, r);
    default: return SN2_ELIMIT;
    }
}

extern "C" size_t sn2_fps_ws_words(int B, int N) { return (size_t)SN2_FPS_WS_WORDS(B, N); }
extern "C" size_t sn2_fps_ws_grid_offset(int B, int N) { return (size_t)SN2_FPS_WS_GRID_OFFSET(B, N); }
extern "C" size_t sn2_fps_ws_ctl_offset(int B, int N) { return (size_t)SN2_FPS_WS_CTL_OFFSET(B, N); }
extern "C" size_t sn2_fps_ws_rank_offset(int B, int N) { return (size_t)SN2_FPS_WS_RANK_OFFSET(B, N); }

extern "C" int sn2_fps_waves(const float* pos_soa, int B, int N, int M, const int* start, int* idx, float* cpos_soa,
                             float* cpos_aos, int* order_ws, int waves, void* stream) {
    return sn2_fps_live(pos_soa, B, N, M, start, nullptr, idx, cpos_soa, cpos_aos, order_ws, waves, nullptr, nullptr, stream);
}

extern "C" int sn2_fps_status(const float* pos_soa, int B, int N, int M, const int* start, int* idx, float* cpos_soa,
                              float* cpos_aos, int* order_ws, int waves, unsigned* status, void* stream) {
    return sn2_fps_live(pos_soa, B, N, M, start, nullptr, idx, cpos_soa, cpos_aos, order_ws, waves, nullptr, status, stream);
}

// nl = n_live, nlo = n_live_out (include/strata_hip.h): every kernel form honours both
extern "C" int sn2_fps_live(const float* pos_soa, int B, int N, int M, const int* start, const int* nl, int* idx, float* cpos_soa,
                            float* cpos_aos, int* order_ws, int waves, int* nlo, unsigned* status, void* stream) {
    if (!pos_soa || !idx || !cpos_soa || !cpos_aos || B <= 0 || N <= 0 || M <= 0 || M > N) return SN2_EINVAL;
    sn2_fps_route_t r;
    int rc = sn2_fps_route(B, N, M, waves, order_ws && ((size_t)order_ws) % 16 == 0, sn2_cu_count(), &r);
    if (rc != 0) return rc;
    const fps_call a = {pos_soa, B, N, M, start, nl, idx, cpos_soa, cpos_aos, order_ws, nlo, status, (hipStream_t)stream};
    switch (r.form) {
    case SN2_FPS_FORM_BRUTE: return launch_fps_brute(a, r);
    case SN2_FPS_FORM_CLUSTER: rc = launch_fps_cluster_form(a, r); return rc != 0 ? rc : launch_fps_single(a, 16, r.repair, true, true);
    default: return launch_fps_single(a, r.nw, r.rung, r.form == SN2_FPS_FORM_SPEC, false);
    }
}

extern "C" int sn2_fps(const float* pos_soa, int B, int N, int M, const int* start, int* idx, float* cpos_soa,
                       float* cpos_aos, int* order_ws, void* stream) {
    return sn2_fps_waves(pos_soa, B, N, M, start, idx, cpos_soa, cpos_aos, order_ws, 0, stream);
}
