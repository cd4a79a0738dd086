// atlas_table.h -- the canvas table of a mosaic atlas (include/strata_hip.h, "Mosaic atlas"), stated once: how a row follows from
// the row before it, the check that a host table is sn2_atlas_canvas_table's, and the search by which a workgroup finds its
// canvas.  atlas.hip and admissibility.hip index the arenas by this table.
#pragma once
#include <cmath>
#include <cstring>

#include "common.h"

constexpr int ATLAS_COLS = SN2_ATLAS_CANVAS_COLS;

// the last row r of [0, n) with table[r * stride + col] <= blk (rows are non-decreasing in that column, row 0 holds 0).
// Every argument is uniform over the workgroup: the loads are scalar.
template <typename T>
__device__ __forceinline__ int last_row_at_or_below(const T* __restrict__ table, int stride, int col, int n, long long blk) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((long long)table[(size_t)mid * stride + col] <= blk) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

static inline long long atlas_bits_of(double v) {
    long long b;
    std::memcpy(&b, &v, 8);
    return b;
}
static inline double atlas_double_of(long long b) {
    double v;
    std::memcpy(&v, &b, 8);
    return v;
}

// row k of the table from the row before it; SN2_EINVAL / SN2_ELIMIT as the entry points answer them
static inline int atlas_canvas_row(long long H, long long W, double x_min, double y_max, const long long* prev, long long* row) {
    constexpr int COLS = ATLAS_COLS;
    if (H <= 0 || W <= 0 || H > 0x7fffffffLL || W > 0x7fffffffLL) return SN2_EINVAL;
    if (!std::isfinite(x_min) || !std::isfinite(y_max)) return SN2_EINVAL;
    if (H * W >= (1LL << 31)) return SN2_ELIMIT;
    row[0] = prev[0];
    row[1] = H;
    row[2] = W;
    row[3] = prev[3];
    row[4] = prev[4];
    row[5] = atlas_bits_of(x_min);
    row[6] = atlas_bits_of(y_max);
    row[7] = 0;
    row[COLS + 0] = prev[0] + H * W;
    row[COLS + 3] = prev[3] + (long long)SN2_ATLAS_FINALIZE_BLOCKS(H, W);
    row[COLS + 4] = prev[4] + (long long)SN2_MOSAIC_CROP_BLOCKS(H, W);
    return 0;
}

// a host table is taken only if it is what sn2_atlas_canvas_table writes: the kernels index the arenas by it
static inline int atlas_check_table(int K, const long long* t) {
    constexpr int COLS = ATLAS_COLS;
    if (!t || K <= 0) return SN2_EINVAL;
    if (t[0] != 0 || t[3] != 0 || t[4] != 0) return SN2_EINVAL;
    long long want[2 * COLS];
    for (int k = 0; k < K; ++k) {
        const long long* r = t + (size_t)k * COLS;
        const int rc = atlas_canvas_row(r[1], r[2], atlas_double_of(r[5]), atlas_double_of(r[6]), r, want);
        if (rc) return rc;
        if (r[7] != 0 || r[COLS + 0] != want[COLS + 0] || r[COLS + 3] != want[COLS + 3] || r[COLS + 4] != want[COLS + 4]) return SN2_EINVAL;
        if (r[COLS + 3] > 0x7fffffffLL || r[COLS + 4] > 0x7fffffffLL) return SN2_ELIMIT;     // a grid of at most 2^31 - 1 workgroups
    }
    const long long* last = t + (size_t)K * COLS;
    if (last[1] != 0 || last[2] != 0 || last[5] != 0 || last[6] != 0 || last[7] != 0) return SN2_EINVAL;
    return 0;
}
