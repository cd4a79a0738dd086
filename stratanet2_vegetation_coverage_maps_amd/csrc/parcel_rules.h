// parcel_rules.h -- the rules of a prepared plot, stated once: the fp64 disc test, the candidate centres of a point, the wave step
// of the count / fill passes (a plot's points in ascending index, slots fixed by integer counts alone), the multi-block scan, the
// z-norm grid and the per-point search of the z-normalisation.  The single-parcel kernels (parcel.hip) and the kernels over a
// cloud arena of K parcels (parcels.hip) call these functions, so a plot gets the same bytes from either.
// Kernels and host helpers here have internal linkage: every unit that includes the header gets its own copy.
#pragma once
#include "common.h"
#include "plot_sort.h"

#include <limits.h>

constexpr int PC_WAVES = 4;              // rows (waves) per workgroup of the count / fill passes
constexpr int SCAN_ITEMS = 16;           // items per thread of the multi-block scan
constexpr int SCAN_BLOCK = 256 * SCAN_ITEMS;
constexpr long PARCEL_MAX_TABLE = 1L << 28;   // (plot, row) cells of the count table
constexpr long PARCEL_MAX_ZCELLS = 1L << 26;  // cells of the z-norm grid

// ---- exclusive scan of n int32 counts -> out (n+1), out[n] = total; block sums and the total in int64 (the caller reads
// the total back and refuses a parcel whose count overflows int32).  Three deterministic passes, no atomics.
static __global__ __launch_bounds__(256) void pscan_reduce_kernel(const int* __restrict__ in, long n, long long* __restrict__ bsum) {
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
static __global__ __launch_bounds__(1024) void pscan_sums_kernel(long long* __restrict__ bsum, int nb, long long* __restrict__ total,
                                                                 int* __restrict__ out, long n) {
    __shared__ long long s_wsum[16];
    const int tid = threadIdx.x;
    const int per = (nb + 1023) / 1024;
    long long sum = 0;
    for (int k = 0; k < per; ++k) {
        const int c = tid * per + k;
        if (c < nb) sum += bsum[c];
    }
    long long all;
    long long run = block_scan_excl<1024>(sum, s_wsum, 0ll, all);
    if (tid == 0) {
        total[0] = all;
        out[n] = (int)all;
    }
    for (int k = 0; k < per; ++k) {
        const int c = tid * per + k;
        if (c < nb) {
            const long long v = bsum[c];
            bsum[c] = run;
            run += v;
        }
    }
}

static __global__ __launch_bounds__(256) void pscan_apply_kernel(const int* __restrict__ in, long n, const long long* __restrict__ boff,
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

static inline int pscan(const int* in, long n, int* out, long long* bsum, long long* total, hipStream_t st) {
    const int nb = sn2_cdiv(n, SCAN_BLOCK);
    hipLaunchKernelGGL(pscan_reduce_kernel, dim3(nb), dim3(256), 0, st, in, n, bsum);
    hipLaunchKernelGGL(pscan_sums_kernel, dim3(1), dim3(1024), 0, st, bsum, nb, total, out, n);
    hipLaunchKernelGGL(pscan_apply_kernel, dim3(nb), dim3(256), 0, st, in, n, (const long long*)bsum, out);
    SN2_RETURN_LAUNCH();
}

static inline size_t pscan_words(long n) { return 2 * ((size_t)sn2_cdiv(n, SCAN_BLOCK) + 2); }

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

// The wave step of the count and fill passes: one wave walks the points [i0, i1) of ONE cloud (a row), 64 at a time.  cloud:
// the cloud's first column, channel c of point i at cloud[c * stride + i]; table: the cloud's (plot, row) entries, plot-major,
// `rows` per plot; plot_base: per plot of the cloud.  All arguments wave-uniform.
// count pass (FILL = false): table[q*rows + row] += points of the row in disc q.
// fill pass (FILL = true): table holds the exclusive starts; every hit of a kept plot q (plot_base[q] != INT_MIN) goes to
// slot plot_base[q] + cursor + rank, where rank orders the wave's points in q by lane (= index) and the cursor, advanced by
// the row's own wave only, orders its 64-point steps.  The wave visits its lanes' plots in ascending id: each lane keeps its
// smallest unvisited hit, the wave takes the minimum over lanes, and every lane whose next hit it is joins that plot.
template <bool FILL>
__device__ __forceinline__ void parcel_wave_step(const float* __restrict__ cloud, size_t stride, long i0, long i1, const CenterGrid& g,
                                                 int* __restrict__ table, int rows, int row, const int* __restrict__ plot_base,
                                                 long sum_n, float* __restrict__ raw, int* __restrict__ pidx) {
    const int lane = threadIdx.x & 63;
    for (long b = i0; b < i1; b += 64) {
        const long i = b + lane;
        const bool valid = i < i1;
        double px = 0.0, py = 0.0;
        Window w{0, -1, 0, -1};
        if (valid) {
            px = (double)cloud[i];
            py = (double)cloud[stride + i];
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
                            if (c != 2) raw[(size_t)c * sum_n + s] = cloud[(size_t)c * stride + i];
                    }
                }
            }
            if (mine) q = next_hit(g, w, px, py, m);
        }
    }
}

// ---- z-normalisation of the plots: the cloud binned once into cells of side >= zr (counting sort), then one thread per
// plot point scans the 3 x 3 cells around its own and keeps the neighbours that lie in the point's disc.
static __global__ __launch_bounds__(256) void pz_copy_kernel(const int* __restrict__ src, int* __restrict__ dst, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

// the point (qx, qy, zi) of the plot centred on (cx, cy), binned into cell c of its cloud's GX x GY grid; start: the grid's CSR
// into `sorted` (x, y, z per binned point) -> its normalised z
__device__ __forceinline__ float pz_query_point(double qx, double qy, float zi, int c, float cx, float cy,
                                                const int* __restrict__ start, const float4* __restrict__ sorted, int GX, int GY,
                                                double zr2, double r2) {
#pragma clang fp contract(off)
    const int gx = c % GX, gy = c / GX;
    float best = zi;                                      // the point is its own neighbour (distance 0) and in its disc
    for (int yy = (gy > 0 ? gy - 1 : 0); yy <= (gy < GY - 1 ? gy + 1 : GY - 1); ++yy) {
        const int c_lo = yy * GX + (gx > 0 ? gx - 1 : 0), c_hi = yy * GX + (gx < GX - 1 ? gx + 1 : GX - 1);
        for (int k = start[c_lo]; k < start[c_hi + 1]; ++k) {
            const float4 v = sorted[k];
            const double dx = qx - (double)v.x, dy = qy - (double)v.y;
            if (dx * dx + dy * dy <= zr2 && v.z < best && in_disc((double)v.x, (double)v.y, cx, cy, r2)) best = v.z;
        }
    }
    return (float)((double)zi - (double)best);            // fp64 difference, then cast (as sn2_znorm)
}

// the cell of a coordinate pair in a z-norm grid of origin (x0, y0): fp32 arithmetic, clamped to the grid
__device__ __forceinline__ int pz_cell_of(float x, float y, float x0, float y0, float inv, int GX, int GY) {
    int cx = (int)((x - x0) * inv), cy = (int)((y - y0) * inv);
    cx = cx < 0 ? 0 : (cx > GX - 1 ? GX - 1 : cx);
    cy = cy < 0 ? 0 : (cy > GY - 1 ? GY - 1 : cy);
    return cy * GX + cx;
}

struct ZGrid { int GX, GY; float inv; };

static inline ZGrid zgrid_of(float radius, float x_min, float y_min, float x_max, float y_max) {
    const float inv = 1.0f / (radius * 1.0001f);
    const long gx = (long)((x_max - x_min) * inv) + 1, gy = (long)((y_max - y_min) * inv) + 1;
    if (gx * gy > PARCEL_MAX_ZCELLS) return ZGrid{0, 0, inv};
    return ZGrid{(int)gx, (int)gy, inv};
}

// words of the z-norm workspace over T points and nc cells: the cell scan's sums, sorted (4 T), cell (T), hist, start, cursor
static inline size_t pz_ws_words(long T, long nc) {
    return ((pscan_words(nc) + 3) & ~(size_t)3) + 5 * (size_t)T + 3 * (size_t)nc + 1;
}
