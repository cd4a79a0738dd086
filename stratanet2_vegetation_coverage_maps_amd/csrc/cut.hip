// cut.hip -- the points of a LAS tile cut into K parcel clouds by buffered polygon: count, scan, fill, in the shape of the
// sn2_parcel_count / sn2_parcel_fill pair.  Host side: parcel.py (cut_parcels), las.py (load_parcels), hip_ops.CutTable.
//
// Contract (include/strata_hip.h, "Parcel cut"):
//   - the rule is stated once, in cut_rules.h; both passes call cut_wave_step with the same arguments, so the fill pass meets the
//     hits of the count pass in the same order;
//   - every entry point checks the candidate table's host copy before it launches, so no index derived from it leaves its arrays;
//   - the output bytes do not depend on arrival order: integer counts and cursors, no floating-point atomics.
#include "cut_rules.h"
#include "parcel_rules.h"

#include <math.h>

namespace {

struct Sizes { long T, rows, entries; };

// the checks of the header, on the host copy
int check_table(const sn2_cut_table* t, Sizes* n) {
    if (!t || !t->cell_start || !t->cell_items || !t->edge_start || !t->edges) return SN2_EINVAL;
    if (t->K < 1 || t->T < 1 || t->GX < 1 || t->GY < 1 || t->n_items < 0 || t->n_edges < 0) return SN2_EINVAL;
    if (!isfinite(t->buffer) || !(t->buffer >= 0.0) || !isfinite(t->gx0) || !isfinite(t->gy0) || !isfinite(t->inv) || !(t->inv > 0.0))
        return SN2_EINVAL;
    if (t->L < 64 || t->L % 64 != 0) return SN2_EINVAL;
    if (t->T >= (1LL << 31)) return SN2_ELIMIT;
    const long cells = (long)t->GX * t->GY;
    if (cells > CUT_MAX_CELLS || t->n_items > CUT_MAX_ITEMS || t->n_edges > CUT_MAX_EDGES) return SN2_ELIMIT;
    const long rows = (long)((t->T + t->L - 1) / t->L);
    if (rows * t->K > PARCEL_MAX_TABLE) return SN2_ELIMIT;
    if (t->cell_start[0] != 0 || t->cell_start[cells] != t->n_items || t->edge_start[0] != 0 || t->edge_start[t->K] != t->n_edges)
        return SN2_EINVAL;
    for (long c = 0; c < cells; ++c) {
        const long lo = t->cell_start[c], hi = t->cell_start[c + 1];
        if (hi < lo || hi > t->n_items) return SN2_EINVAL;
        for (long j = lo; j < hi; ++j) {
            const int id = t->cell_items[j];
            if (id < 0 || id >= t->K || (j > lo && id <= t->cell_items[j - 1])) return SN2_EINVAL;
        }
    }
    for (int k = 0; k < t->K; ++k)
        if (t->edge_start[k + 1] < t->edge_start[k] || t->edge_start[k + 1] > t->n_edges) return SN2_EINVAL;
    for (long j = 0; j < 4 * (long)t->n_edges; ++j)
        if (!(fabs(t->edges[j]) <= CUT_MAX_COORD)) return SN2_EINVAL;          // (also refuses NaN)
    *n = Sizes{(long)t->T, rows, rows * t->K};
    return 0;
}

size_t count_words(long entries) { return pscan_words(entries) + (size_t)entries; }

int check_mask(const unsigned char* cls, const unsigned* drop, CutDrop* d) {
    if ((cls == nullptr) != (drop == nullptr)) return SN2_EINVAL;
    for (int j = 0; j < 8; ++j) d->w[j] = drop ? drop[j] : 0u;
    return 0;
}

template <bool FILL>
__global__ __launch_bounds__(256) void cut_pass_kernel(const float* __restrict__ cloud, long T, const unsigned char* __restrict__ cls,
                                                       CutDrop drop, int L, int rows, CutGrid g, const int* __restrict__ edge_start,
                                                       const double* __restrict__ edges, double b2, int* __restrict__ table,
                                                       const int* __restrict__ parcel_base, long sum_n, float* __restrict__ out,
                                                       int* __restrict__ pidx) {
    const int row = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * PC_WAVES + (threadIdx.x >> 6)));
    if (row >= rows) return;                               // uniform per wave
    const long i0 = (long)row * L, i1 = i0 + L < T ? i0 + L : T;
    cut_wave_step<FILL>(cloud, T, cls, drop, i0, i1, g, edge_start, edges, b2, table, rows, row, parcel_base, sum_n, out, pidx);
}

// parcel_start[k] = the first entry of parcel k in the scanned table, parcel_start[K] = all hits
__global__ __launch_bounds__(256) void cut_start_kernel(const int* __restrict__ prefix, const long long* __restrict__ total, int K,
                                                        long rows, long long* __restrict__ parcel_start) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k > K) return;
    parcel_start[k] = k == K ? total[0] : (long long)prefix[(long)k * rows];
}

CutGrid grid_of(const sn2_cut_table* t) {
    return CutGrid{t->cell_start_dev, t->cell_items_dev, t->GX, t->GY, t->gx0, t->gy0, t->inv};
}
}  // namespace

extern "C" int sn2_cut_ws_words(const sn2_cut_table* table, size_t* words) {
    if (!words) return SN2_EINVAL;
    Sizes n;
    SN2_TRY(check_table(table, &n));
    *words = count_words(n.entries);
    return 0;
}

extern "C" int sn2_cut_count(const float* cloud, const unsigned char* classification, const unsigned* drop, const sn2_cut_table* table,
                             int* ws, size_t ws_words, int* prefix, long long* parcel_start, void* stream) {
    if (!cloud || !ws || !prefix || !parcel_start) return SN2_EINVAL;
    Sizes n;
    SN2_TRY(check_table(table, &n));
    if (!table->cell_start_dev || !table->cell_items_dev || !table->edge_start_dev || !table->edges_dev) return SN2_EINVAL;
    CutDrop d;
    SN2_TRY(check_mask(classification, drop, &d));
    if (ws_words < count_words(n.entries) || ((size_t)ws % 8) != 0) return SN2_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    long long* bsum = reinterpret_cast<long long*>(ws);                          // pscan_words(entries)
    int* counts = ws + pscan_words(n.entries);                                   // K rows counts, parcel-major
    long long* total = parcel_start + table->K + 1;
    sn2_fill_words(counts, 0u, (size_t)n.entries, st);
    hipLaunchKernelGGL(cut_pass_kernel<false>, dim3(sn2_cdiv(n.rows, PC_WAVES)), dim3(256), 0, st, cloud, n.T, classification, d, table->L,
                       (int)n.rows, grid_of(table), table->edge_start_dev, table->edges_dev, table->buffer * table->buffer, counts,
                       (const int*)nullptr, 0L, (float*)nullptr, (int*)nullptr);
    SN2_TRY(pscan(counts, n.entries, prefix, bsum, total, st));
    hipLaunchKernelGGL(cut_start_kernel, dim3(sn2_cdiv(table->K + 1, 256)), dim3(256), 0, st, (const int*)prefix, (const long long*)total,
                       table->K, n.rows, parcel_start);
    SN2_RETURN_LAUNCH();
}

extern "C" int sn2_cut_fill(const float* cloud, const unsigned char* classification, const unsigned* drop, const sn2_cut_table* table,
                            int* prefix, const int* parcel_base, long sum_n, float* out, int* point_index, void* stream) {
    if (!cloud || !prefix || !parcel_base || !out || !point_index || sum_n <= 0) return SN2_EINVAL;
    if (sum_n >= (1L << 31)) return SN2_ELIMIT;
    Sizes n;
    SN2_TRY(check_table(table, &n));
    if (!table->cell_start_dev || !table->cell_items_dev || !table->edge_start_dev || !table->edges_dev) return SN2_EINVAL;
    CutDrop d;
    SN2_TRY(check_mask(classification, drop, &d));
    hipLaunchKernelGGL(cut_pass_kernel<true>, dim3(sn2_cdiv(n.rows, PC_WAVES)), dim3(256), 0, (hipStream_t)stream, cloud, n.T,
                       classification, d, table->L, (int)n.rows, grid_of(table), table->edge_start_dev, table->edges_dev,
                       table->buffer * table->buffer, prefix, parcel_base, sum_n, out, point_index);
    SN2_RETURN_LAUNCH();
}
