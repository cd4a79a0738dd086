// dbf.hip -- the records of a dBase (.dbf) table, as the file holds them, annotated with n numeric fields formatted on the device:
// the PRED_* fields the parcel job appends to its shapefile.  Every byte the source record holds is copied; nothing is re-encoded.
// Host side: shp.py (`write_predictions`).
//
// Contract (include/strata_hip.h, "dBase records, annotated"; the rule's functions: dbf_rules.h):
//   - ONE launch, no synchronisation between workgroups, nothing read back: safe to capture;
//   - no store touches a byte at or beyond K Ld other than the counter's eight, no load a source byte at or beyond K L, a row_of entry
//     beyond K or a value outside values[0, R C);
//   - the overflow count is an integer, reduced per wave and per workgroup first and added with one integer atomic per workgroup
//     that has something to add: the same input gives the same bytes.
//
// ONE form.  L is arbitrary, so neither the source nor the output records are word-aligned; the output is therefore taken as one
// stream of K Ld bytes and cut into tiles of DBF_TILE_BYTES = 16 KiB that start on multiples of 16 KiB.  A workgroup of 256 composes
// its tile in LDS -- the copied bytes first, consecutive lanes on consecutive bytes of the stream (byte loads of one cache line per
// wave), then the fields, a lane per field that has a byte in the tile -- and the tile leaves with 16-byte stores, lane after lane
// (the last tile's odd bytes one by one).  A field that straddles two tiles is formatted by both and counted by the first.
#include <string.h>

#include "common.h"
#include "dbf_rules.h"

static_assert(DBF_EINVAL == SN2_EINVAL && DBF_ELIMIT == SN2_ELIMIT && DBF_TILE_BYTES % 16 == 0, "dbf_rules.h restates the header's constants");

namespace {

constexpr int DBF_WG = 256;
constexpr int DBF_WAVES = DBF_WG / 64;

struct dbf_params {
    dbf_shape s;
    const uint8_t* src;
    const uint64_t* values;            // the doubles' bit patterns: no floating-point operation touches them
    const int* row_of;
    uint8_t* dst;
    unsigned long long* counter;
    uint64_t record_bytes, missing;
    long long R;
    int C;
    int cols[DBF_MAX_FIELDS];
};

struct dbf_lds_sink {
    uint8_t* lds;
    uint64_t o0;
    __device__ __forceinline__ void byte(uint64_t o, uint32_t v) const { lds[o - o0] = (uint8_t)v; }
};
struct dbf_values {
    const dbf_params* P;
    __device__ __forceinline__ uint64_t operator()(uint64_t k, int f) const {
        const int row = P->row_of[k];
        if (row < 0 || (long long)row >= P->R) return P->missing;
        return P->values[(size_t)row * (size_t)P->C + (size_t)P->cols[f]];
    }
};

__global__ __launch_bounds__(DBF_WG) void dbf_annotate_kernel(const dbf_params P) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[DBF_TILE_BYTES];
    __shared__ uint32_t red[DBF_WAVES];
    const uint64_t o0 = (uint64_t)blockIdx.x * DBF_TILE_BYTES;
    const uint64_t o1 = P.record_bytes - o0 < DBF_TILE_BYTES ? P.record_bytes : o0 + DBF_TILE_BYTES;
    const dbf_lds_sink sink{tile, o0};
    dbf_copy_range(P.src, P.s, o0, o1, sink, threadIdx.x, DBF_WG);
    uint32_t overflow = dbf_field_range(dbf_values{&P}, P.s, o0, o1, sink, threadIdx.x, DBF_WG);
    for (int m = 32; m >= 1; m >>= 1) overflow += __shfl_xor(overflow, m, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = overflow;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (int w = 0; w < DBF_WAVES; ++w) total += red[w];
        if (total) atomicAdd(P.counter, (unsigned long long)total);
    }
    const uint32_t bytes = (uint32_t)(o1 - o0), full = bytes >> 4, tail = bytes & 15;
    uint8_t* out = P.dst + o0;                                         // 16-byte aligned
    for (uint32_t c = threadIdx.x; c < full; c += DBF_WG) reinterpret_cast<uint4*>(out)[c] = reinterpret_cast<const uint4*>(tile)[c];
    if (threadIdx.x < tail) out[(size_t)full * 16 + threadIdx.x] = tile[full * 16 + threadIdx.x];
}
}  // namespace

extern "C" int sn2_dbf_annotate(const void* src_records, long K, int L, const double* values, long R, int C, const int* row_of,
                                const int* cols, int n, int size, int decimal, double missing, void* dst, size_t dst_bytes,
                                void* stream) {
    if (!src_records || !values || !row_of || !cols || !dst) return SN2_EINVAL;
    if (R <= 0 || C <= 0) return SN2_EINVAL;
    uint64_t record_bytes = 0, total = 0;
    SN2_TRY(dbf_check_shape(K, L, n, size, decimal, &record_bytes, &total));
    for (int f = 0; f < n; ++f)
        if (cols[f] < 0 || cols[f] >= C) return SN2_EINVAL;
    if ((uintptr_t)dst % 16 != 0 || dst_bytes < total) return SN2_EINVAL;
    const uint64_t tiles = dbf_tiles(record_bytes);
    if (tiles > 0x7FFFFFFFull || (unsigned long)R >= (1ul << 31)) return SN2_ELIMIT;
    dbf_params P = {};
    P.s.K = K;
    P.s.L = L;
    P.s.n = n;
    P.s.size = size;
    P.s.decimal = decimal;
    P.s.Ld = L + n * size;
    P.src = (const uint8_t*)src_records;
    P.values = reinterpret_cast<const uint64_t*>(values);
    P.row_of = row_of;
    P.dst = (uint8_t*)dst;
    P.counter = reinterpret_cast<unsigned long long*>((uint8_t*)dst + (total - DBF_COUNTER_BYTES));
    P.record_bytes = record_bytes;
    memcpy(&P.missing, &missing, sizeof(missing));
    P.R = R;
    P.C = C;
    for (int f = 0; f < n; ++f) P.cols[f] = cols[f];
    hipLaunchKernelGGL(dbf_annotate_kernel, dim3((unsigned)tiles), dim3(DBF_WG), 0, (hipStream_t)stream, P);
    SN2_RETURN_LAUNCH();
}
