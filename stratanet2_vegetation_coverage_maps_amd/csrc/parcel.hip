// parcel.hip -- preparation of a parcel's plots on the device: the discs of `extract_cloud` (inference/prepare_utils.py:47-53,
// a scipy cKDTree radius query per plot centre) and the per-plot z-normalisation of `pre_transform` (utils/load_data.py:
// 228-249), for every plot centre of a parcel at once.  Host side: parcel.py.
//
// Contract (include/strata_hip.h, sn2_parcel_*):
//   - membership of point i in the disc of centre p is scipy's test in fp64 without contraction:
//     dx*dx + dy*dy <= r*r with dx = (double)x_i - (double)cx_p.  With fp32 inputs of similar magnitude every step is exact;
//   - the points of a plot are in ascending parcel index.  A point's slot is fixed by integer counts alone: one wave owns
//     a contiguous range of L points (a "row") and walks it 64 points at a time; per (plot, row) the count pass counts, an
//     exclusive scan turns the counts into starts, and in the fill pass the row's wave takes ranks from its own cursor in
//     index order.  No other wave touches that cursor, so the bytes do not depend on arrival order;
//   - the z of a plot point is z_i - min{ z_j : |xy_i - xy_j| <= zr, j in the SAME disc } (the reference normalises each
//     extracted plot on its own points), with zr the z-norm radius; no float atomics anywhere.
#include "common.h"

#include <limits.h>

namespace {

constexpr int PC_WAVES = 4;              // rows (waves) per workgroup of the count / fill passes
constexpr int SCAN_ITEMS = 16;           // items per thread of the multi-block scan
constexpr int SCAN_BLOCK = 256 * SCAN_ITEMS;
constexpr long PARCEL_MAX_TABLE = 1L << 28;   // (plot, row) cells of the count table
constexpr long PARCEL_MAX_ZCELLS = 1L << 26;  // cells of the z-norm grid

// ---- exclusive scan of n int32 counts -> out (n+1), out[n] = total; block sums and the total in int64 (the caller reads
// the total back and refuses a parcel whose count overflows int32).  Three deterministic passes, no atomics.
__global__ __launch_bounds__(256) void pscan_reduce_kernel(const int* __restrict__ in, long n, long long* __restrict__ bsum) {
    __shared__ long long red[256];
    const long base = (long)blockIdx.x * SCAN_BLOCK;
    long long s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const long j = base + k * 256 + threadIdx.x;
        if (j < n) s += in[j];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = red[0];
}

// one workgroup: exclusive scan of the nb block sums in place; total[0] = their sum, out[n] = (int)total
__global__ __launch_bounds__(1024) void pscan_sums_kernel(long long* __restrict__ bsum, int nb, long long* __restrict__ total,
                                                          int* __restrict__ out, long n) {
    __shared__ long long s_tot[1024];
    const int tid = threadIdx.x;
    const int per = (nb + 1023) / 1024;
    long long sum = 0;
    for (int k = 0; k < per; ++k) {
        const int c = tid * per + k;
        if (c < nb) sum += bsum[c];
    }
    s_tot[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        for (int t = 0; t < 1024; ++t) { const long long v = s_tot[t]; s_tot[t] = run; run += v; }
        total[0] = run;
        out[n] = (int)run;
    }
    __syncthreads();
    long long run = s_tot[tid];
    for (int k = 0; k < per; ++k) {
        const int c = tid * per + k;
        if (c < nb) {
            const long long v = bsum[c];
            bsum[c] = run;
            run += v;
        }
    }
}

__global__ __launch_bounds__(256) void pscan_apply_kernel(const int* __restrict__ in, long n, const long long* __restrict__ boff,
                                                          int* __restrict__ out) {
    __shared__ long long sc[256];
    const int t = threadIdx.x;
    const long base = (long)blockIdx.x * SCAN_BLOCK + (long)t * SCAN_ITEMS;     // SCAN_ITEMS consecutive items per thread
    int v[SCAN_ITEMS];
    long long s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        v[k] = base + k < n ? in[base + k] : 0;
        s += v[k];
    }
    sc[t] = s;
    __syncthreads();
    for (int w = 1; w < 256; w <<= 1) {                   // inclusive Hillis-Steele scan of the thread sums
        const long long a = t >= w ? sc[t - w] : 0;
        __syncthreads();
        sc[t] += a;
        __syncthreads();
    }
    long long run = boff[blockIdx.x] + sc[t] - s;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        if (base + k < n) out[base + k] = (int)run;
        run += v[k];
    }
}

int pscan(const int* in, long n, int* out, long long* bsum, long long* total, hipStream_t st) {
    const int nb = sn2_cdiv(n, SCAN_BLOCK);
    hipLaunchKernelGGL(pscan_reduce_kernel, dim3(nb), dim3(256), 0, st, in, n, bsum);
    hipLaunchKernelGGL(pscan_sums_kernel, dim3(1), dim3(1024), 0, st, bsum, nb, total, out, n);
    hipLaunchKernelGGL(pscan_apply_kernel, dim3(nb), dim3(256), 0, st, in, n, (const long long*)bsum, out);
    SN2_RETURN_LAUNCH();
}

size_t pscan_words(long n) { return 2 * ((size_t)sn2_cdiv(n, SCAN_BLOCK) + 2); }

// ---- the disc test and the candidate centres of a point -------------------------------------------------------------
struct CenterGrid {
    const float* cen;        // (P,2) plot centres
    const int* start;        // (GX*GY+1) CSR of the centre cells, rows of cells contiguous
    const int* items;        // centre ids, ascending inside a cell
    int GX, GY;
    double x0, y0, inv;      // cell of a position: floor((v - x0) * inv); cells are wider than the disc radius
    double r2;
};

__device__ __forceinline__ bool in_disc(double px, double py, float cx, float cy, double r2) {
#pragma clang fp contract(off)
    const double dx = px - (double)cx, dy = py - (double)cy;
    return dx * dx + dy * dy <= r2;
}

// the 3 x 3 window of centre cells around a position (empty: x1 < x0)
struct Window { int x0, x1, y0, y1; };

__device__ __forceinline__ Window window_of(const CenterGrid& g, double px, double py) {
    Window w{0, -1, 0, -1};
    const double fx = floor((px - g.x0) * g.inv), fy = floor((py - g.y0) * g.inv);
    if (fx >= -1.0 && fx <= (double)g.GX && fy >= -1.0 && fy <= (double)g.GY) {
        const int ix = (int)fx, iy = (int)fy;
        w.x0 = ix > 0 ? ix - 1 : 0;
        w.x1 = ix + 1 < g.GX ? ix + 1 : g.GX - 1;
        w.y0 = iy > 0 ? iy - 1 : 0;
        w.y1 = iy + 1 < g.GY ? iy + 1 : g.GY - 1;
    }
    return w;
}

// smallest centre id > prev whose disc holds the point, INT_MAX if none
__device__ __forceinline__ int next_hit(const CenterGrid& g, const Window& w, double px, double py, int prev) {
    int best = INT_MAX;
    for (int yy = w.y0; yy <= w.y1; ++yy) {
        const int lo = g.start[yy * g.GX + w.x0], hi = g.start[yy * g.GX + w.x1 + 1];   // a row's cells are contiguous
        for (int k = lo; k < hi; ++k) {
            const int q = g.items[k];
            if (q > prev && q < best && in_disc(px, py, g.cen[2 * q], g.cen[2 * q + 1], g.r2)) best = q;
        }
    }
    return best;
}

// count pass (FILL = false): table[q*rows + row] += points of the row in disc q.
// fill pass (FILL = true): table holds the exclusive starts; every hit of a kept plot q (plot_base[q] != INT_MIN) goes to
// slot plot_base[q] + cursor + rank, where rank orders the wave's points in q by lane (= index) and the cursor, advanced by
// the row's own wave only, orders its 64-point steps.  The wave visits its lanes' plots in ascending id: each lane keeps its
// smallest unvisited hit, the wave takes the minimum over lanes, and every lane whose next hit it is joins that plot.
template <bool FILL>
__global__ __launch_bounds__(256) void parcel_pass_kernel(const float* __restrict__ cloud, long T, int L, int rows, CenterGrid g,
                                                          int* __restrict__ table, const int* __restrict__ plot_base, long sum_n,
                                                          float* __restrict__ raw, int* __restrict__ pidx) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * PC_WAVES + (int)(threadIdx.x >> 6);
    if (row >= rows) return;                                   // uniform per wave
    const long i0 = (long)row * L, i1 = i0 + L < T ? i0 + L : T;
    for (long b = i0; b < i1; b += 64) {
        const long i = b + lane;
        const bool valid = i < i1;
        double px = 0.0, py = 0.0;
        Window w{0, -1, 0, -1};
        if (valid) {
            px = (double)cloud[i];
            py = (double)cloud[T + i];
            w = window_of(g, px, py);
        }
        int q = next_hit(g, w, px, py, -1);
        while (true) {
            int m = q;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const int v = __shfl_xor(m, o);
                m = v < m ? v : m;
            }
            if (m == INT_MAX) break;
            const bool mine = q == m;
            const unsigned long long mask = __ballot(mine);
            const int leader = __ffsll((long long)mask) - 1;
            int* cur = &table[(long)m * rows + row];
            if (!FILL) {
                if (lane == leader) atomicAdd(cur, __popcll(mask));
            } else {
                const int pb = plot_base[m];
                if (pb != INT_MIN) {
                    int c0 = 0;
                    if (lane == leader) c0 = atomicAdd(cur, __popcll(mask));
                    c0 = __shfl(c0, leader);
                    if (mine) {
                        const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32),
                                                                   __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                        const long s = (long)pb + c0 + rank;
                        pidx[s] = (int)i;
#pragma unroll
                        for (int c = 0; c < 10; ++c)
                            if (c != 2) raw[(size_t)c * sum_n + s] = cloud[(size_t)c * T + i];
                    }
                }
            }
            if (mine) q = next_hit(g, w, px, py, m);
        }
    }
}

// ---- z-normalisation of the plots: the parcel binned once into cells of side >= zr (counting sort), then one thread per
// plot point scans the 3 x 3 cells around its own and keeps the neighbours that lie in the point's disc.
__global__ __launch_bounds__(256) void pz_cell_kernel(const float* __restrict__ x, const float* __restrict__ y, int n, float x0,
                                                      float y0, float inv, int GX, int GY, int* __restrict__ cell,
                                                      int* __restrict__ hist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int cx = (int)((x[i] - x0) * inv), cy = (int)((y[i] - y0) * inv);
    cx = cx < 0 ? 0 : (cx > GX - 1 ? GX - 1 : cx);
    cy = cy < 0 ? 0 : (cy > GY - 1 ? GY - 1 : cy);
    const int c = cy * GX + cx;
    cell[i] = c;
    atomicAdd(&hist[c], 1);
}

__global__ __launch_bounds__(256) void pz_copy_kernel(const int* __restrict__ src, int* __restrict__ dst, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

// the order inside a cell is arrival order: it only changes the order of a min over floats, not its value
__global__ __launch_bounds__(256) void pz_scatter_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                         const float* __restrict__ z, int n, const int* __restrict__ cell,
                                                         int* __restrict__ cursor, float4* __restrict__ sorted) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int p = atomicAdd(&cursor[cell[i]], 1);
    sorted[p] = make_float4(x[i], y[i], z[i], 0.f);
}

__global__ __launch_bounds__(256) void pz_query_kernel(const float* __restrict__ cloud, long T, const int* __restrict__ offs,
                                                       int P, const float* __restrict__ cen, const int* __restrict__ pidx,
                                                       long sum_n, const int* __restrict__ cell, const int* __restrict__ start,
                                                       const float4* __restrict__ sorted, int GX, int GY, double zr2, double r2,
                                                       float* __restrict__ raw) {
#pragma clang fp contract(off)
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s >= sum_n) return;
    int lo = 0, hi = P;                                   // the plot p of slot s: offs[p] <= s < offs[p+1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offs[mid] <= s) lo = mid; else hi = mid;
    }
    const float cx = cen[2 * lo], cy = cen[2 * lo + 1];
    const int i = pidx[s];
    const double qx = (double)cloud[i], qy = (double)cloud[T + i];
    const float zi = cloud[2 * T + i];
    const int c = cell[i], gx = c % GX, gy = c / GX;
    float best = zi;                                      // the point is its own neighbour (distance 0) and in its disc
    for (int yy = (gy > 0 ? gy - 1 : 0); yy <= (gy < GY - 1 ? gy + 1 : GY - 1); ++yy) {
        const int c_lo = yy * GX + (gx > 0 ? gx - 1 : 0), c_hi = yy * GX + (gx < GX - 1 ? gx + 1 : GX - 1);
        for (int k = start[c_lo]; k < start[c_hi + 1]; ++k) {
            const float4 v = sorted[k];
            const double dx = qx - (double)v.x, dy = qy - (double)v.y;
            if (dx * dx + dy * dy <= zr2 && v.z < best && in_disc((double)v.x, (double)v.y, cx, cy, r2)) best = v.z;
        }
    }
    raw[2 * (size_t)sum_n + s] = (float)((double)zi - (double)best);   // fp64 difference, then cast (as sn2_znorm)
}

struct ZGrid { int GX, GY; float inv; };

ZGrid zgrid_of(float radius, float x_min, float y_min, float x_max, float y_max) {
    const float inv = 1.0f / (radius * 1.0001f);
    const long gx = (long)((x_max - x_min) * inv) + 1, gy = (long)((y_max - y_min) * inv) + 1;
    if (gx * gy > PARCEL_MAX_ZCELLS) return ZGrid{0, 0, inv};
    return ZGrid{(int)gx, (int)gy, inv};
}

bool grid_ok(const int* cell_start, const int* cell_items, int GX, int GY, double cell_inv) {
    return cell_start && cell_items && GX > 0 && GY > 0 && (long)GX * GY <= PARCEL_MAX_TABLE && cell_inv > 0.0;
}
}  // namespace

extern "C" size_t sn2_parcel_count_ws_words(int P, int rows) {
    const long n = (long)P * rows;
    return pscan_words(n) + (size_t)n;
}

extern "C" size_t sn2_parcel_znorm_ws_words(long T, float radius, float x_min, float y_min, float x_max, float y_max) {
    const ZGrid z = zgrid_of(radius, x_min, y_min, x_max, y_max);
    if (z.GX == 0 || T <= 0) return 0;
    const size_t nc = (size_t)z.GX * z.GY;
    return ((pscan_words((long)nc) + 3) & ~(size_t)3) + 5 * (size_t)T + 3 * nc + 1;
}

extern "C" int sn2_parcel_count(const float* cloud, long T, int L, int rows, const float* centers, int P, const int* cell_start,
                                const int* cell_items, int GX, int GY, double gx0, double gy0, double cell_inv, float radius,
                                int* ws, size_t ws_words, int* prefix, long long* total, void* stream) {
    if (!cloud || !centers || !ws || !prefix || !total || T <= 0 || P <= 0 || L <= 0 || rows <= 0 || !(radius > 0.f) ||
        !grid_ok(cell_start, cell_items, GX, GY, cell_inv))
        return SN2_EINVAL;
    if (T >= (1L << 31) || (long)P * rows >= PARCEL_MAX_TABLE) return SN2_ELIMIT;
    if ((long)L * rows < T || (long)L * (rows - 1) >= T) return SN2_EINVAL;   // rows cover the points, none is empty
    if (ws_words < sn2_parcel_count_ws_words(P, rows) || ((size_t)ws % 8) != 0) return SN2_EINVAL;
    if (1.0 / cell_inv < (double)radius) return SN2_EINVAL;                       // cells narrower than the disc
    hipStream_t st = (hipStream_t)stream;
    const long n = (long)P * rows;
    long long* bsum = reinterpret_cast<long long*>(ws);                          // pscan_words(n)
    int* table = ws + pscan_words(n);                                             // n counts, plot-major
    sn2_fill_words(table, 0u, (size_t)n, st);
    const CenterGrid g{centers, cell_start, cell_items, GX, GY, gx0, gy0, cell_inv, (double)radius * (double)radius};
    hipLaunchKernelGGL(parcel_pass_kernel<false>, dim3(sn2_cdiv(rows, PC_WAVES)), dim3(256), 0, st, cloud, T, L, rows, g, table,
                       (const int*)nullptr, 0L, (float*)nullptr, (int*)nullptr);
    return pscan(table, n, prefix, bsum, total, st);
}

extern "C" int sn2_parcel_fill(const float* cloud, long T, int L, int rows, const float* centers, int P, const int* cell_start,
                               const int* cell_items, int GX, int GY, double gx0, double gy0, double cell_inv, float radius,
                               int* prefix, const int* plot_base, long sum_n, float* raw, int* point_index, void* stream) {
    if (!cloud || !centers || !prefix || !plot_base || !raw || !point_index || T <= 0 || P <= 0 || L <= 0 || rows <= 0 ||
        sum_n <= 0 || !(radius > 0.f) || !grid_ok(cell_start, cell_items, GX, GY, cell_inv))
        return SN2_EINVAL;
    if (T >= (1L << 31) || sum_n >= (1L << 31) || (long)P * rows >= PARCEL_MAX_TABLE) return SN2_ELIMIT;
    if ((long)L * rows < T || (long)L * (rows - 1) >= T || 1.0 / cell_inv < (double)radius) return SN2_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const CenterGrid g{centers, cell_start, cell_items, GX, GY, gx0, gy0, cell_inv, (double)radius * (double)radius};
    hipLaunchKernelGGL(parcel_pass_kernel<true>, dim3(sn2_cdiv(rows, PC_WAVES)), dim3(256), 0, st, cloud, T, L, rows, g, prefix,
                       plot_base, sum_n, raw, point_index);
    SN2_RETURN_LAUNCH();
}

extern "C" int sn2_parcel_znorm(const float* cloud, long T, float x_min, float y_min, float x_max, float y_max, float radius,
                                float disc_radius, const int* offsets, const float* centers, int P, const int* point_index,
                                long sum_n, int* ws, size_t ws_words, float* raw, void* stream) {
    if (!cloud || !offsets || !centers || !point_index || !ws || !raw || T <= 0 || P <= 0 || sum_n <= 0 || !(radius > 0.f) ||
        !(disc_radius > 0.f) || !(x_max >= x_min) || !(y_max >= y_min))
        return SN2_EINVAL;
    if (T >= (1L << 31) || sum_n >= (1L << 31)) return SN2_ELIMIT;
    const ZGrid z = zgrid_of(radius, x_min, y_min, x_max, y_max);
    if (z.GX == 0) return SN2_ELIMIT;
    if (ws_words < sn2_parcel_znorm_ws_words(T, radius, x_min, y_min, x_max, y_max) || ((size_t)ws % 16) != 0) return SN2_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)T;
    const long nc = (long)z.GX * z.GY;
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
    hipLaunchKernelGGL(pz_cell_kernel, dim3(blocks), dim3(256), 0, st, cloud, cloud + T, n, x_min, y_min, z.inv, z.GX, z.GY, cell,
                       hist);
    SN2_TRY(pscan(hist, nc, start, bsum, total, st));
    const int cb = sn2_cdiv(nc, 256 * 4);
    hipLaunchKernelGGL(pz_copy_kernel, dim3(cb < 2048 ? cb : 2048), dim3(256), 0, st, (const int*)start, cursor, (size_t)nc);
    hipLaunchKernelGGL(pz_scatter_kernel, dim3(blocks), dim3(256), 0, st, cloud, cloud + T, cloud + 2 * T, n, (const int*)cell,
                       cursor, sorted);
    hipLaunchKernelGGL(pz_query_kernel, dim3(sn2_cdiv(sum_n, 256)), dim3(256), 0, st, cloud, T, offsets, P, centers, point_index,
                       sum_n, (const int*)cell, (const int*)start, (const float4*)sorted, z.GX, z.GY,
                       (double)radius * (double)radius, (double)disc_radius * (double)disc_radius, raw);
    SN2_RETURN_LAUNCH();
}
