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
#include "parcel_rules.h"

namespace {

// one wave per row of L points: the wave step of parcel_rules.h over the parcel's cloud and its (plot, row) table
template <bool FILL>
__global__ __launch_bounds__(256) void parcel_pass_kernel(const float* __restrict__ cloud, long T, int L, int rows, CenterGrid g,
                                                          int* __restrict__ table, const int* __restrict__ plot_base, long sum_n,
                                                          float* __restrict__ raw, int* __restrict__ pidx) {
    const int row = blockIdx.x * PC_WAVES + (int)(threadIdx.x >> 6);
    if (row >= rows) return;                                   // uniform per wave
    const long i0 = (long)row * L, i1 = i0 + L < T ? i0 + L : T;
    parcel_wave_step<FILL>(cloud, (size_t)T, i0, i1, g, table, rows, row, plot_base, sum_n, raw, pidx);
}

// ---- z-normalisation of the plots (parcel_rules.h): the parcel binned once, then one thread per plot point
__global__ __launch_bounds__(256) void pz_cell_kernel(const float* __restrict__ x, const float* __restrict__ y, int n, float x0,
                                                      float y0, float inv, int GX, int GY, int* __restrict__ cell,
                                                      int* __restrict__ hist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = pz_cell_of(x[i], y[i], x0, y0, inv, GX, GY);
    cell[i] = c;
    atomicAdd(&hist[c], 1);
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
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s >= sum_n) return;
    int lo = 0, hi = P;                                   // the plot p of slot s: offs[p] <= s < offs[p+1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offs[mid] <= s) lo = mid; else hi = mid;
    }
    const int i = pidx[s];
    raw[2 * (size_t)sum_n + s] = pz_query_point((double)cloud[i], (double)cloud[T + i], cloud[2 * T + i], cell[i], cen[2 * lo],
                                                cen[2 * lo + 1], start, sorted, GX, GY, zr2, r2);
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
    return pz_ws_words(T, (long)nc);
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
