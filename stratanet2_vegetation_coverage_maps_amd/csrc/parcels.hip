// parcels.hip -- the preparation of parcel.hip for K parcels at once: their clouds in one arena, their plots counted, filled and
// z-normalised by the launches one parcel takes.  Host side: parcel.py (ParcelClouds, prepare_parcels).
//
// Contract (include/strata_hip.h, sn2_parcels_*):
//   - a prepared plot is what sn2_parcel_count / _fill / _znorm make of it: every rule is a function of parcel_rules.h, called here
//     with the parcel's own columns, centres, centre grid, (plot, row) entries and z-norm cells, so a parcel's points never see
//     another parcel's centres or points, wherever the parcels lie;
//   - every wave and thread finds its parcel by a binary search on the parcel table; the entry points check the table's host copy
//     against the builder before they launch, so no index derived from it leaves the parcel's ranges;
//   - the output bytes do not depend on arrival order: integer counts and cursors, min / max over floats through order-preserving
//     integers, no floating-point add atomics.
#include "parcel_rules.h"

#include <math.h>
#include <string.h>

#include <vector>

namespace {

constexpr int COLS = SN2_PARCELS_COLS;
constexpr int CHUNK = SN2_PARCELS_BBOX_CHUNK;
// columns of a parcel's row; row K: [C_T0] T_all [C_T] L [C_ROW0] rows [C_C0] P_all [C_P] K [C_E0] entries [C_G0] centre cells + K'
// [C_Z0] z cells [C_LO] radius | z radius << 32
enum { C_T0, C_T, C_ROW0, C_C0, C_P, C_E0, C_G0, C_GX, C_GY, C_X0, C_Y0, C_INV, C_Z0, C_LO, C_HI, C_ZG };

inline long long bits_of(double v) { long long b; memcpy(&b, &v, 8); return b; }
inline double double_of(long long b) { double v; memcpy(&v, &b, 8); return v; }
inline long long pack2(float a, float b) {
    unsigned ua, ub;
    memcpy(&ua, &a, 4);
    memcpy(&ub, &b, 4);
    return (long long)(((unsigned long long)ub << 32) | ua);
}
inline float lo_of(long long v) { const unsigned u = (unsigned)((unsigned long long)v & 0xffffffffu); float f; memcpy(&f, &u, 4); return f; }
inline float hi_of(long long v) { const unsigned u = (unsigned)((unsigned long long)v >> 32); float f; memcpy(&f, &u, 4); return f; }

// the table of K parcels (host arithmetic).  grid (K,3) = gx0, gy0, cell_inv; boxes (K,4) = x_min, y_min, x_max, y_max
int parcels_build(int K, const long long* T, const int* P, const int* GX, const int* GY, const double* grid, const float* boxes,
                  float radius, float zradius, long long* t) {
    if (!T || !P || !GX || !GY || !grid || !boxes || !t || K <= 0 || !(radius > 0.f) || !(zradius > 0.f) || !isfinite(radius) ||
        !isfinite(zradius))
        return SN2_EINVAL;
    long long T_all = 0, P_all = 0, G = 0;
    unsigned __int128 work = 0;                                   // sum of T_k P_k: what decides the row length
    for (int k = 0; k < K; ++k) {
        if (T[k] <= 0 || P[k] < 0) return SN2_EINVAL;
        const float* b = boxes + 4 * k;
        if (!isfinite(b[0]) || !isfinite(b[1]) || !isfinite(b[2]) || !isfinite(b[3]) || !(b[2] >= b[0]) || !(b[3] >= b[1]))
            return SN2_EINVAL;
        if (P[k] > 0) {
            const double inv = grid[3 * k + 2];
            if (GX[k] <= 0 || GY[k] <= 0 || !isfinite(grid[3 * k]) || !isfinite(grid[3 * k + 1]) || !isfinite(inv) || !(inv > 0.0))
                return SN2_EINVAL;
            if (1.0 / inv < (double)radius) return SN2_EINVAL;    // cells narrower than the disc
            G += (long long)GX[k] * GY[k] + 1;
        }
        T_all += T[k];
        P_all += P[k];
        work += (unsigned __int128)T[k] * (unsigned)P[k];
        if (T_all >= (1LL << 31) || P_all >= (1LL << 31) || G > PARCEL_MAX_TABLE) return SN2_ELIMIT;
    }
    // one row length for the set, grown as parcel.prepare_parcel grows it: about 2^26 (plot, row) entries at the most
    const unsigned __int128 per = (work + ((1u << 26) - 1)) >> 26;
    if (per >= (1LL << 31)) return SN2_ELIMIT;
    long long L = ((long long)per + 63) / 64 * 64;
    L = L < 2048 ? 2048 : L;
    long long t0 = 0, row0 = 0, c0 = 0, e0 = 0, g0 = 0, z0 = 0;
    for (int k = 0; k < K; ++k) {
        long long* r = t + (size_t)k * COLS;
        const float* b = boxes + 4 * k;
        const long long rows = P[k] > 0 ? (T[k] + L - 1) / L : 0;
        ZGrid z{0, 0, 0.f};
        if (P[k] > 0) {
            z = zgrid_of(zradius, b[0], b[1], b[2], b[3]);
            if (z.GX == 0) return SN2_ELIMIT;
        }
        r[C_T0] = t0, r[C_T] = T[k], r[C_ROW0] = row0, r[C_C0] = c0, r[C_P] = P[k], r[C_E0] = e0, r[C_G0] = g0;
        r[C_GX] = P[k] > 0 ? GX[k] : 0, r[C_GY] = P[k] > 0 ? GY[k] : 0;
        for (int j = 0; j < 3; ++j) r[C_X0 + j] = P[k] > 0 ? bits_of(grid[3 * k + j]) : 0;
        r[C_Z0] = z0, r[C_LO] = pack2(b[0], b[1]), r[C_HI] = pack2(b[2], b[3]);
        r[C_ZG] = (long long)(((unsigned long long)(unsigned)z.GY << 32) | (unsigned)z.GX);
        t0 += T[k], row0 += rows, c0 += P[k], e0 += rows * P[k], z0 += (long long)z.GX * z.GY;
        if (P[k] > 0) g0 += (long long)GX[k] * GY[k] + 1;
        if (e0 >= PARCEL_MAX_TABLE || z0 > PARCEL_MAX_ZCELLS || row0 >= (1LL << 31)) return SN2_ELIMIT;
    }
    long long* r = t + (size_t)K * COLS;
    for (int j = 0; j < COLS; ++j) r[j] = 0;
    r[C_T0] = t0, r[C_T] = L, r[C_ROW0] = row0, r[C_C0] = c0, r[C_P] = K, r[C_E0] = e0, r[C_G0] = g0, r[C_Z0] = z0;
    r[C_LO] = pack2(radius, zradius);
    return 0;
}

struct Totals { long T_all, rows, P_all, E, G, ZC; int L; float radius, zradius; };

// a table is taken iff the builder makes the same words of its own T, P, grids and boxes
int check_table(int K, const long long* t, Totals* tot) {
    if (!t || K <= 0) return SN2_EINVAL;
    const long long* last = t + (size_t)K * COLS;
    if (last[C_P] != K) return SN2_EINVAL;
    std::vector<long long> T(K), again((size_t)(K + 1) * COLS);
    std::vector<int> P(K), GX(K), GY(K);
    std::vector<double> grid(3 * (size_t)K);
    std::vector<float> boxes(4 * (size_t)K);
    for (int k = 0; k < K; ++k) {
        const long long* r = t + (size_t)k * COLS;
        if (r[C_P] < 0 || r[C_P] >= (1LL << 31) || r[C_GX] < 0 || r[C_GX] >= (1LL << 31) || r[C_GY] < 0 || r[C_GY] >= (1LL << 31))
            return SN2_EINVAL;
        T[k] = r[C_T], P[k] = (int)r[C_P], GX[k] = (int)r[C_GX], GY[k] = (int)r[C_GY];
        for (int j = 0; j < 3; ++j) grid[3 * k + j] = double_of(r[C_X0 + j]);
        boxes[4 * k] = lo_of(r[C_LO]), boxes[4 * k + 1] = hi_of(r[C_LO]), boxes[4 * k + 2] = lo_of(r[C_HI]), boxes[4 * k + 3] = hi_of(r[C_HI]);
    }
    SN2_TRY(parcels_build(K, T.data(), P.data(), GX.data(), GY.data(), grid.data(), boxes.data(), lo_of(last[C_LO]), hi_of(last[C_LO]),
                          again.data()));
    if (memcmp(again.data(), t, again.size() * sizeof(long long)) != 0) return SN2_EINVAL;
    *tot = Totals{(long)last[C_T0], (long)last[C_ROW0], (long)last[C_C0], (long)last[C_E0], (long)last[C_G0], (long)last[C_Z0],
                  (int)last[C_T], lo_of(last[C_LO]), hi_of(last[C_LO])};
    return 0;
}

size_t count_words(long E) { return pscan_words(E) + (size_t)E; }

// the last row k of `tab` with tab[k][col] <= v (rows that own nothing repeat their successor's base and are passed over)
__device__ __forceinline__ int parcel_of(const long long* __restrict__ tab, int K, int col, long long v) {
    int lo = 0, hi = K;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab[(size_t)mid * COLS + col] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- bounding boxes: workgroup b folds CHUNK points of ONE parcel into state[4k..] = ord(x_min), ord(y_min), ord(x_max), ord(y_max)
__global__ __launch_bounds__(256) void parcels_bbox_kernel(const float* __restrict__ arena, size_t T_all, const long long* __restrict__ starts,
                                                           int K, unsigned* __restrict__ state) {
    __shared__ float red[4][4];
    const long long* wg = starts + (K + 1);
    int lo = 0, hi = K;                                   // the parcel of this workgroup: wg[k] <= b < wg[k+1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (wg[mid] <= (long long)blockIdx.x) lo = mid; else hi = mid;
    }
    const long i0 = (long)starts[lo] + ((long)blockIdx.x - (long)wg[lo]) * CHUNK;
    const long end = (long)starts[lo + 1], i1 = i0 + CHUNK < end ? i0 + CHUNK : end;
    float x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
    for (long i = i0 + threadIdx.x; i < i1; i += 256) {
        const float x = arena[i], y = arena[T_all + i];
        x0 = fminf(x0, x), x1 = fmaxf(x1, x), y0 = fminf(y0, y), y1 = fmaxf(y1, y);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        x0 = fminf(x0, __shfl_xor(x0, o)), y0 = fminf(y0, __shfl_xor(y0, o));
        x1 = fmaxf(x1, __shfl_xor(x1, o)), y1 = fmaxf(y1, __shfl_xor(y1, o));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[wave][0] = x0, red[wave][1] = y0, red[wave][2] = x1, red[wave][3] = y1;
    __syncthreads();
    if (threadIdx.x < 4) {
        const int j = threadIdx.x;
        float v = red[0][j];
        for (int w = 1; w < 4; ++w) v = j < 2 ? fminf(v, red[w][j]) : fmaxf(v, red[w][j]);
        if (j < 2) atomicMin(&state[4 * lo + j], f2ord(v)); else atomicMax(&state[4 * lo + j], f2ord(v));
    }
}

// ---- count / fill: global row -> parcel (wave-uniform), then the wave step against that parcel alone
template <bool FILL>
__global__ __launch_bounds__(256) void parcels_pass_kernel(const float* __restrict__ arena, size_t T_all, int L, int rows_all,
                                                           const long long* __restrict__ tab, int K, const float* __restrict__ centers,
                                                           const int* __restrict__ cell_start, const int* __restrict__ cell_items,
                                                           double r2, int* __restrict__ table, const int* __restrict__ plot_base,
                                                           long sum_n, float* __restrict__ raw, int* __restrict__ pidx) {
    const int row = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * PC_WAVES + (threadIdx.x >> 6)));
    if (row >= rows_all) return;                               // uniform per wave
    const long long* t = tab + (size_t)parcel_of(tab, K, C_ROW0, row) * COLS;
    const long T = (long)t[C_T], c0 = (long)t[C_C0];
    const int P = (int)t[C_P], local = row - (int)t[C_ROW0];
    const int rows = (int)((T + L - 1) / L);
    const CenterGrid g{centers + 2 * c0, cell_start + t[C_G0], cell_items, (int)t[C_GX], (int)t[C_GY], __longlong_as_double(t[C_X0]),
                       __longlong_as_double(t[C_Y0]), __longlong_as_double(t[C_INV]), r2};
    if (P <= 0 || local >= rows) return;                       // (not reached with a checked table)
    const long i0 = (long)local * L, i1 = i0 + L < T ? i0 + L : T;
    parcel_wave_step<FILL>(arena + t[C_T0], T_all, i0, i1, g, table + t[C_E0], rows, local, FILL ? plot_base + c0 : plot_base, sum_n,
                           raw, pidx);
}

// plot_start[p] = the first entry of plot p in the scanned table, plot_start[P_all] = all hits
__global__ __launch_bounds__(256) void parcels_plot_start_kernel(const int* __restrict__ prefix, const long long* __restrict__ total,
                                                                 const long long* __restrict__ tab, int K, int L, long P_all,
                                                                 long long* __restrict__ plot_start) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p > P_all) return;
    if (p == P_all) {
        plot_start[p] = total[0];
        return;
    }
    const long long* t = tab + (size_t)parcel_of(tab, K, C_C0, p) * COLS;
    const long rows = (t[C_T] + L - 1) / L;
    plot_start[p] = prefix[t[C_E0] + (p - t[C_C0]) * rows];
}

// ---- z-norm: every point binned into ITS parcel's cells (the fp32 arithmetic of the single-parcel call, the parcel's own origin)
__global__ __launch_bounds__(256) void parcels_cell_kernel(const float* __restrict__ arena, long T_all, const long long* __restrict__ tab,
                                                           int K, float inv, int* __restrict__ cell, int* __restrict__ hist) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= T_all) return;
    const long long* t = tab + (size_t)parcel_of(tab, K, C_T0, i) * COLS;
    const int GX = (int)(t[C_ZG] & 0xffffffffLL), GY = (int)(t[C_ZG] >> 32);
    if (GX <= 0) {                                             // a parcel without centres has no cells
        cell[i] = -1;
        return;
    }
    const int c = (int)t[C_Z0] + pz_cell_of(arena[i], arena[T_all + i], __uint_as_float((unsigned)(t[C_LO] & 0xffffffffLL)),
                                            __uint_as_float((unsigned)((unsigned long long)t[C_LO] >> 32)), inv, GX, GY);
    cell[i] = c;
    atomicAdd(&hist[c], 1);
}

// the order inside a cell is arrival order: it only changes the order of a min over floats, not its value
__global__ __launch_bounds__(256) void parcels_scatter_kernel(const float* __restrict__ arena, long T_all, const int* __restrict__ cell,
                                                              int* __restrict__ cursor, float4* __restrict__ sorted) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= T_all) return;
    const int c = cell[i];
    if (c < 0) return;
    const int p = atomicAdd(&cursor[c], 1);
    sorted[p] = make_float4(arena[i], arena[T_all + i], arena[2 * T_all + i], 0.f);
}

__global__ __launch_bounds__(256) void parcels_query_kernel(const float* __restrict__ arena, long T_all, const long long* __restrict__ tab,
                                                            int K, const int* __restrict__ offs, int P, const float* __restrict__ cen,
                                                            const int* __restrict__ plot_parcel, const int* __restrict__ pidx, long sum_n,
                                                            const int* __restrict__ cell, const int* __restrict__ start,
                                                            const float4* __restrict__ sorted, double zr2, double r2,
                                                            float* __restrict__ raw) {
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s >= sum_n) return;
    int lo = 0, hi = P;                                   // the plot p of slot s: offs[p] <= s < offs[p+1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offs[mid] <= s) lo = mid; else hi = mid;
    }
    int k = plot_parcel[lo];
    k = k < 0 ? 0 : (k > K - 1 ? K - 1 : k);
    const long long* t = tab + (size_t)k * COLS;
    const int GX = (int)(t[C_ZG] & 0xffffffffLL), GY = (int)(t[C_ZG] >> 32);
    const long il = pidx[s];
    if (GX <= 0 || il < 0 || il >= t[C_T]) return;
    const long i = (long)t[C_T0] + il;
    const int z0 = (int)t[C_Z0];
    raw[2 * (size_t)sum_n + s] = pz_query_point((double)arena[i], (double)arena[T_all + i], arena[2 * T_all + i], cell[i] - z0,
                                                cen[2 * lo], cen[2 * lo + 1], start + z0, sorted, GX, GY, zr2, r2);
}

// the (2, K+1) starts of sn2_parcels_bbox: point_start and the prefix of ceil(T_k / CHUNK)
int check_starts(int K, const long long* s, long T_all, long* wgs) {
    if (!s || K <= 0 || T_all <= 0) return SN2_EINVAL;
    if (T_all >= (1L << 31)) return SN2_ELIMIT;
    const long long* wg = s + (K + 1);
    if (s[0] != 0 || wg[0] != 0 || s[K] != T_all) return SN2_EINVAL;
    for (int k = 0; k < K; ++k) {
        const long long T = s[k + 1] - s[k];
        if (T <= 0 || s[k + 1] > T_all || wg[k + 1] - wg[k] != (T + CHUNK - 1) / CHUNK) return SN2_EINVAL;
    }
    *wgs = (long)wg[K];
    return 0;
}
}  // namespace

extern "C" int sn2_parcels_table(int K, const long long* T, const int* P, const int* GX, const int* GY, const double* grid,
                                 const float* boxes, float radius, float zradius, long long* table, int* L, size_t* count_ws_words,
                                 size_t* znorm_ws_words) {
    if (!L || !count_ws_words || !znorm_ws_words) return SN2_EINVAL;
    SN2_TRY(parcels_build(K, T, P, GX, GY, grid, boxes, radius, zradius, table));
    const long long* last = table + (size_t)K * COLS;
    *L = (int)last[C_T];
    *count_ws_words = count_words((long)last[C_E0]);
    *znorm_ws_words = pz_ws_words((long)last[C_T0], (long)last[C_Z0]);
    return 0;
}

extern "C" int sn2_parcels_bbox(const float* arena, long T_all, int K, const long long* starts_host, const long long* starts_dev,
                                unsigned* state, void* stream) {
    if (!arena || !starts_dev || !state) return SN2_EINVAL;
    long wgs = 0;
    SN2_TRY(check_starts(K, starts_host, T_all, &wgs));
    hipLaunchKernelGGL(parcels_bbox_kernel, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, arena, (size_t)T_all, starts_dev, K,
                       state);
    SN2_RETURN_LAUNCH();
}

extern "C" int sn2_parcels_count(const float* arena, int K, const long long* table_host, const long long* table_dev,
                                 const float* centers, const int* cell_start, const int* cell_items, float radius, int* ws,
                                 size_t ws_words, int* prefix, long long* total, long long* plot_start, void* stream) {
    if (!arena || !table_dev || !centers || !cell_start || !cell_items || !ws || !prefix || !total || !plot_start) return SN2_EINVAL;
    Totals n;
    SN2_TRY(check_table(K, table_host, &n));
    if (n.P_all <= 0 || radius != n.radius) return SN2_EINVAL;                  // no centre at all: nothing to count
    if (ws_words < count_words(n.E) || ((size_t)ws % 8) != 0) return SN2_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    long long* bsum = reinterpret_cast<long long*>(ws);                          // pscan_words(E)
    int* table = ws + pscan_words(n.E);                                           // E counts: parcel by parcel, plot-major
    sn2_fill_words(table, 0u, (size_t)n.E, st);
    hipLaunchKernelGGL(parcels_pass_kernel<false>, dim3(sn2_cdiv(n.rows, PC_WAVES)), dim3(256), 0, st, arena, (size_t)n.T_all, n.L,
                       (int)n.rows, table_dev, K, centers, cell_start, cell_items, (double)radius * (double)radius, table,
                       (const int*)nullptr, 0L, (float*)nullptr, (int*)nullptr);
    SN2_TRY(pscan(table, n.E, prefix, bsum, total, st));
    hipLaunchKernelGGL(parcels_plot_start_kernel, dim3(sn2_cdiv(n.P_all + 1, 256)), dim3(256), 0, st, (const int*)prefix,
                       (const long long*)total, table_dev, K, n.L, n.P_all, plot_start);
    SN2_RETURN_LAUNCH();
}

extern "C" int sn2_parcels_fill(const float* arena, int K, const long long* table_host, const long long* table_dev,
                                const float* centers, const int* cell_start, const int* cell_items, float radius, int* prefix,
                                const int* plot_base, long sum_n, float* raw, int* point_index, void* stream) {
    if (!arena || !table_dev || !centers || !cell_start || !cell_items || !prefix || !plot_base || !raw || !point_index || sum_n <= 0)
        return SN2_EINVAL;
    if (sum_n >= (1L << 31)) return SN2_ELIMIT;
    Totals n;
    SN2_TRY(check_table(K, table_host, &n));
    if (n.P_all <= 0 || radius != n.radius) return SN2_EINVAL;
    hipLaunchKernelGGL(parcels_pass_kernel<true>, dim3(sn2_cdiv(n.rows, PC_WAVES)), dim3(256), 0, (hipStream_t)stream, arena,
                       (size_t)n.T_all, n.L, (int)n.rows, table_dev, K, centers, cell_start, cell_items, (double)radius * (double)radius,
                       prefix, plot_base, sum_n, raw, point_index);
    SN2_RETURN_LAUNCH();
}

extern "C" int sn2_parcels_znorm(const float* arena, int K, const long long* table_host, const long long* table_dev, float radius,
                                 float disc_radius, const int* offsets, const float* centers, const int* plot_parcel, int P,
                                 const int* point_index, long sum_n, int* ws, size_t ws_words, float* raw, void* stream) {
    if (!arena || !table_dev || !offsets || !centers || !plot_parcel || !point_index || !ws || !raw || P <= 0 || sum_n <= 0)
        return SN2_EINVAL;
    if (sum_n >= (1L << 31)) return SN2_ELIMIT;
    Totals n;
    SN2_TRY(check_table(K, table_host, &n));
    if (n.ZC <= 0 || radius != n.zradius || disc_radius != n.radius) return SN2_EINVAL;
    if (ws_words < pz_ws_words(n.T_all, n.ZC) || ((size_t)ws % 16) != 0) return SN2_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const long T = n.T_all, nc = n.ZC;
    const size_t sw = (pscan_words(nc) + 3) & ~(size_t)3;
    long long* bsum = reinterpret_cast<long long*>(ws);          // block sums of the cell scan, then its total
    long long* total = bsum + sn2_cdiv(nc, SCAN_BLOCK);
    float4* sorted = reinterpret_cast<float4*>(ws + sw);         // T, 16-byte aligned
    int* cell = ws + sw + 4 * (size_t)T;                         // T
    int* hist = cell + T;                                        // nc
    int* start = hist + nc;                                      // nc + 1
    int* cursor = start + nc + 1;                                // nc
    sn2_fill_words(hist, 0u, (size_t)nc, st);
    const int blocks = sn2_cdiv(T, 256);
    hipLaunchKernelGGL(parcels_cell_kernel, dim3(blocks), dim3(256), 0, st, arena, T, table_dev, K, zgrid_of(radius, 0.f, 0.f, 0.f, 0.f).inv,
                       cell, hist);
    SN2_TRY(pscan(hist, nc, start, bsum, total, st));
    const int cb = sn2_cdiv(nc, 256 * 4);
    hipLaunchKernelGGL(pz_copy_kernel, dim3(cb < 2048 ? cb : 2048), dim3(256), 0, st, (const int*)start, cursor, (size_t)nc);
    hipLaunchKernelGGL(parcels_scatter_kernel, dim3(blocks), dim3(256), 0, st, arena, T, (const int*)cell, cursor, sorted);
    hipLaunchKernelGGL(parcels_query_kernel, dim3(sn2_cdiv(sum_n, 256)), dim3(256), 0, st, arena, T, table_dev, K, offsets, P, centers,
                       plot_parcel, point_index, sum_n, (const int*)cell, (const int*)start, (const float4*)sorted,
                       (double)radius * (double)radius, (double)disc_radius * (double)disc_radius, raw);
    SN2_RETURN_LAUNCH();
}
