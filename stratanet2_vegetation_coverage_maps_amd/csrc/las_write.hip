// las_write.hip -- the inverse of las.hip: the point records of a LAS file, as the file holds them, annotated with the network's
// per-point scores.  Every byte the source record holds is copied; the classification field is decided from the class
// probabilities and the chosen scores are appended as extra bytes.  Host side: las.py (`encode`, `write_scored`, `write_parcels`).
//
// Contract (include/strata_hip.h, "LAS point records, written"; the rule's functions: las_write_rules.h):
//   - one launch, no synchronisation between workgroups, nothing read back: safe to capture;
//   - no store touches a byte at or beyond T_out * L_dst, no load a source byte at or beyond T_src * L_src nor a score column
//     outside [col0, col0 + T_out);
//   - the statistics are integers, reduced per wave and per workgroup first and added with integer atomics: the same input gives
//     the same bytes.
//
// STAGED form (L_dst <= LAS_ENCODE_STAGE_MAX_L): a workgroup of 256 takes tiles of 256 consecutive output records = 256 L_dst
// contiguous bytes that start at a multiple of 256 L_dst, hence 16-byte aligned.  Each lane composes its record in LDS: with an odd
// L_dst no record is aligned and neighbouring lanes' records share dwords, so a lane stores whole aligned words where its record
// owns them and single bytes at its two ends (las_word_stream); the tile then leaves with 16-byte stores, lane after lane (the last
// tile's odd bytes one by one).  Without point_index the tile's source records are staged the same way,
// as the decoder stages them; with point_index each lane fetches its own record with aligned dword loads.
// DIRECT form (longer records): each lane writes its record to memory byte by byte.
// Both forms walk the tiles with a grid of the workgroups that are resident at once, so a launch ends with a few thousand atomics
// however many records it wrote; the staged form loads a tile's source chunks and scores one tile ahead.
#include "common.h"
#include "las_write_rules.h"

namespace {

constexpr int LASW_WG = 256;
constexpr int LASW_WAVES = LASW_WG / 64;
constexpr int LAS_ENCODE_STAGE_MAX_L = 120;      // 256 (L_src + L_dst) <= 60 KiB of LDS: two workgroups and more on a CU's 160 KiB
constexpr int LAS_ENCODE_WG_PER_CU = 8;          // the grid: what is resident at once, no more (each workgroup walks its tiles)
constexpr size_t LASW_CU_LDS = 160 * 1024;
constexpr int LASW_STAT_WORDS = 6 + LAS_STATS_RETURN_BINS + 2;       // min[3], max[3], by_return[15], n_bad, n_scored
constexpr size_t LASW_RED_BYTES = (size_t)LASW_WAVES * LASW_STAT_WORDS * 8;
int g_las_encode_form = 0;                       // sn2_debug_las_encode_form: 0 = by L_dst, 1 = the direct form for every L_dst

struct las_write_params {
    las_write_rule rule;
    las_score_cols cols;
    const uint8_t* src;
    const int* point_index;
    uint8_t* dst;
    uint8_t* stats;
    long T_src, T_out;
    size_t col0;
};

// the statistics of one thread over all its records; the counts are kept per wave (ballots), the extremes per lane
struct las_stats_acc {
    int32_t lo[3], hi[3];
    uint32_t by_return[LAS_STATS_RETURN_BINS], n_bad, n_scored;

    __device__ __forceinline__ void init() {
        for (int a = 0; a < 3; ++a) {
            lo[a] = INT32_MAX;
            hi[a] = INT32_MIN;
        }
        for (int r = 0; r < LAS_STATS_RETURN_BINS; ++r) by_return[r] = 0;
        n_bad = n_scored = 0;
    }
    // every lane of the wave calls this, `live` false for a lane without a record
    __device__ __forceinline__ void add(bool live, const las_written& w) {
        const bool good = live && !w.bad;
        if (good) {
            lo[0] = min(lo[0], w.X); hi[0] = max(hi[0], w.X);
            lo[1] = min(lo[1], w.Y); hi[1] = max(hi[1], w.Y);
            lo[2] = min(lo[2], w.Z); hi[2] = max(hi[2], w.Z);
        }
#pragma unroll
        for (int r = 0; r < LAS_STATS_RETURN_BINS; ++r) by_return[r] += (uint32_t)__popcll(__ballot(good && w.return_num == (uint32_t)(r + 1)));
        n_bad += (uint32_t)__popcll(__ballot(live && w.bad));
        n_scored += (uint32_t)__popcll(__ballot(good && w.scored));
    }
    // wave -> workgroup (`red`: LASW_RED_BYTES of LDS) -> one integer atomic per word that has something to say
    __device__ __forceinline__ void flush(uint8_t* stats, long long* red) {
        for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = min(lo[a], __shfl_xor(lo[a], m, 64));
                hi[a] = max(hi[a], __shfl_xor(hi[a], m, 64));
            }
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
            long long* r = red + wave * LASW_STAT_WORDS;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                r[a] = lo[a];
                r[3 + a] = hi[a];
            }
#pragma unroll
            for (int k = 0; k < LAS_STATS_RETURN_BINS; ++k) r[6 + k] = by_return[k];
            r[6 + LAS_STATS_RETURN_BINS] = n_bad;
            r[7 + LAS_STATS_RETURN_BINS] = n_scored;
        }
        __syncthreads();
        const int j = threadIdx.x;
        if (j >= LASW_STAT_WORDS) return;
        long long v = red[j];
        for (int w = 1; w < LASW_WAVES; ++w) {
            const long long o = red[w * LASW_STAT_WORDS + j];
            v = j < 3 ? (o < v ? o : v) : (j < 6 ? (o > v ? o : v) : v + o);
        }
        if (j < 3) {
            if (v != INT32_MAX) atomicMin(reinterpret_cast<int*>(stats + LAS_STATS_OFF_MIN) + j, (int)v);
        } else if (j < 6) {
            if (v != INT32_MIN) atomicMax(reinterpret_cast<int*>(stats + LAS_STATS_OFF_MAX) + (j - 3), (int)v);
        } else if (v != 0) {
            atomicAdd(reinterpret_cast<unsigned long long*>(stats + LAS_STATS_OFF_BY_RETURN) + (j - 6), (unsigned long long)v);
        }
    }
};
static_assert(LAS_STATS_OFF_N_BAD == LAS_STATS_OFF_BY_RETURN + 8 * LAS_STATS_RETURN_BINS && LAS_STATS_OFF_N_SCORED == LAS_STATS_OFF_N_BAD + 8 &&
                  LAS_STATS_BYTES == LAS_STATS_OFF_N_SCORED + 8,
              "by_return, n_bad and n_scored are consecutive 64-bit words");

__host__ __device__ __forceinline__ size_t lasw_slots(int L) { return ((size_t)LASW_WG * L + 15) / 16 + 1; }   // and one of slack

// what a lane holds of a tile before the tile's turn: its share of the source's 16-byte chunks (identity form), its source index
// (gathered form) and its point's scores.  Loaded one tile ahead, so the loads' latency passes behind the composition and the
// stores of the tile before.
// CH chunks per lane hold 256 L_src bytes for L_src <= 16 CH: 3 for the least lengths of formats 0-3 and 6-8 and some bytes more,
// 8 for every staged length, 1 (unused) with point_index.
constexpr int LASW_MAX_CHUNKS = (LASW_WG * LAS_ENCODE_STAGE_MAX_L / 16 + LASW_WG - 1) / LASW_WG;      // 8
constexpr int LASW_FEW_CHUNKS = 3;
typedef uint32_t lasw_v4 __attribute__((ext_vector_type(4)));       // sixteen bytes in registers (a plain vector: it stays there)
template <int CH>
struct las_tile_regs {
    lasw_v4 chunk[CH];
    las_point_scores scores;
    int s;
};

template <int CH>
__device__ __forceinline__ void lasw_load_tile(const las_write_params& P, long tile, bool gather, las_tile_regs<CH>& R) {
    const long first = tile * LASW_WG;
    const int n = (int)(P.T_out - first < LASW_WG ? P.T_out - first : LASW_WG);           // records of this tile, >= 1
    if (!gather) {                                                     // T_out <= T_src: the tile's source records exist
        const int full = (n * P.rule.L_src) >> 4;
        const lasw_v4* base = reinterpret_cast<const lasw_v4*>(P.src + (size_t)first * (size_t)P.rule.L_src);   // 16-byte aligned: first L_src is a multiple of 256
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int c = (int)threadIdx.x + j * LASW_WG;
            if (c < full) R.chunk[j] = base[c];
        }
    }
    if ((int)threadIdx.x < n) {
        const size_t i = (size_t)first + threadIdx.x;
        if (gather) R.s = P.point_index[i];
        R.scores = las_load_scores(P.cols, P.col0 + i, P.rule);
    }
}

template <int CH>
__global__ __launch_bounds__(LASW_WG) void las_encode_staged_kernel(las_write_params P) {
    extern __shared__ __attribute__((aligned(16))) uint4 lasw_lds[];
    const int L_src = P.rule.L_src, L_dst = L_src + P.rule.E;
    const bool gather = P.point_index != nullptr;
    uint4* dst_lds = lasw_lds;                                         // cdiv(256 L_dst, 16) slots and one of slack
    uint4* src_lds = dst_lds + lasw_slots(L_dst);                      // the same for L_src, or nothing with point_index
    long long* red = reinterpret_cast<long long*>(src_lds + (gather ? 0 : lasw_slots(L_src)));
    const las_word_stream sink{reinterpret_cast<uint8_t*>(dst_lds), 0, 0, 0};
    las_stats_acc acc;
    acc.init();
    const long tiles = (P.T_out + LASW_WG - 1) / LASW_WG;
    las_tile_regs<CH> cur = {}, nxt = {};
    if ((long)blockIdx.x < tiles) lasw_load_tile(P, blockIdx.x, gather, cur);
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long first = tile * LASW_WG;
        const int n = (int)(P.T_out - first < LASW_WG ? P.T_out - first : LASW_WG);
        if (!gather) {
            const int bytes = n * L_src;
            const int full = bytes >> 4, tail = bytes & 15;
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                const int c = (int)threadIdx.x + j * LASW_WG;
                if (c < full) reinterpret_cast<lasw_v4*>(src_lds)[c] = cur.chunk[j];
            }
            if (tail && threadIdx.x < 16) {                            // the last tile only: the block's own bytes, no further
                const uint8_t* base = P.src + (size_t)first * (size_t)L_src;
                uint8_t* l8 = reinterpret_cast<uint8_t*>(src_lds + full);
                l8[threadIdx.x] = (int)threadIdx.x < tail ? base[(size_t)full * 16 + threadIdx.x] : (uint8_t)0;
            }
        }
        __syncthreads();
        if (tile + gridDim.x < tiles) lasw_load_tile(P, tile + gridDim.x, gather, nxt);
        const bool live = (int)threadIdx.x < n;
        las_written w = {};
        if (live) {
            const size_t d0 = (size_t)threadIdx.x * (size_t)L_dst;
            if (gather) {
                const bool have = cur.s >= 0 && (long)cur.s < P.T_src;
                const las_guarded_words src{P.src, (size_t)P.T_src * (size_t)L_src};
                w = las_compose(src, have ? (size_t)cur.s * (size_t)L_src : (size_t)0, have, sink, d0, P.rule, cur.scores);
            } else {
                const las_staged_words src{reinterpret_cast<const uint32_t*>(src_lds)};
                w = las_compose(src, (size_t)threadIdx.x * (size_t)L_src, true, sink, d0, P.rule, cur.scores);
            }
        }
        acc.add(live, w);
        __syncthreads();
        const int bytes = n * L_dst;                                   // <= 30 720
        uint8_t* out = P.dst + (size_t)first * (size_t)L_dst;          // 16-byte aligned
        const int full = bytes >> 4, tail = bytes & 15;
        for (int c = threadIdx.x; c < full; c += LASW_WG) reinterpret_cast<uint4*>(out)[c] = dst_lds[c];
        if ((int)threadIdx.x < tail) out[(size_t)full * 16 + threadIdx.x] = reinterpret_cast<const uint8_t*>(dst_lds + full)[threadIdx.x];
        cur = nxt;
    }
    acc.flush(P.stats, red);
}

__global__ __launch_bounds__(LASW_WG) void las_encode_direct_kernel(las_write_params P) {
    extern __shared__ __attribute__((aligned(16))) uint4 lasw_lds[];
    const int L_src = P.rule.L_src, L_dst = L_src + P.rule.E;
    const las_byte_stream sink{P.dst, 0};
    const las_guarded_words src{P.src, (size_t)P.T_src * (size_t)L_src};
    las_stats_acc acc;
    acc.init();
    const long tiles = (P.T_out + LASW_WG - 1) / LASW_WG;
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long i = tile * LASW_WG + threadIdx.x;
        const bool live = i < P.T_out;
        las_written w = {};
        if (live) {
            const long s = P.point_index ? (long)P.point_index[i] : i;
            const bool have = s >= 0 && s < P.T_src;
            w = las_compose(src, have ? (size_t)s * (size_t)L_src : (size_t)0, have, sink, (size_t)i * (size_t)L_dst, P.rule,
                            las_load_scores(P.cols, P.col0 + (size_t)i, P.rule));
        }
        acc.add(live, w);
    }
    acc.flush(P.stats, reinterpret_cast<long long*>(lasw_lds));
}
}  // namespace

extern "C" int sn2_las_encode_stage_max(void) { return LAS_ENCODE_STAGE_MAX_L; }

extern "C" int sn2_debug_las_encode_form(int form) {
    if (form != 0 && form != 1) return SN2_EINVAL;
    g_las_encode_form = form;
    return 0;
}

extern "C" int sn2_las_encode(const void* src, size_t src_bytes, int format, int L_src, long T_src, const int* point_index, long T_out,
                              const float* scores, const float* weight, const int* hits, long score_stride, long col0, int field_mask,
                              int class_mode, const int* class_codes, int unscored_code, void* dst, size_t dst_bytes, void* stats,
                              void* stream) {
    if (!src || !dst || !stats || T_out <= 0 || T_src <= 0) return SN2_EINVAL;
    if (las_format_is_laz(format) || !las_format_known(format)) return SN2_EINVAL;
    if (L_src < las_min_length(format) || L_src > 65535) return SN2_EINVAL;
    if (field_mask < 0 || ((unsigned)field_mask & ~LAS_FIELD_MASK_ALL) != 0) return SN2_EINVAL;
    if (class_mode != 0 && class_mode != 1) return SN2_EINVAL;
    const int E = las_write_extra_bytes((unsigned)field_mask);
    const int L_dst = L_src + E;
    if (L_dst > 65535) return SN2_EINVAL;
    if (T_out >= (1L << 31) || T_src >= (1L << 31)) return SN2_ELIMIT;
    if (src_bytes / (size_t)L_src < (size_t)T_src) return SN2_EINVAL;              // src_bytes < T_src L_src, without the product
    if (dst_bytes / (size_t)L_dst < (size_t)T_out) return SN2_EINVAL;
    if ((uintptr_t)src % 16 != 0 || (uintptr_t)dst % 16 != 0 || (uintptr_t)stats % 8 != 0) return SN2_EINVAL;
    if (!point_index && T_out > T_src) return SN2_EINVAL;                          // record i is source record i
    if (col0 < 0 || score_stride <= 0 || col0 > score_stride - T_out) return SN2_EINVAL;
    const bool plain = field_mask == 0 && class_mode == 0;
    if (!plain && (!scores || !weight || !hits)) return SN2_EINVAL;
    int codes[4] = {0, 0, 0, 0};
    if (class_mode == 1) {
        if (!class_codes) return SN2_EINVAL;
        const int top = las_write_max_code(format);
        for (int k = 0; k < 4; ++k) {
            codes[k] = class_codes[k];
            if (codes[k] < 0 || codes[k] > top) return SN2_EINVAL;
        }
        if (unscored_code < -1 || unscored_code > top) return SN2_EINVAL;
    }
    las_write_params P = {};
    P.rule.format = format;
    P.rule.L_src = L_src;
    P.rule.E = E;
    P.rule.mask = (unsigned)field_mask;
    P.rule.class_mode = class_mode;
    P.rule.codes = las_write_pack_codes(codes);
    P.rule.unscored = unscored_code;
    P.cols.scores = scores;
    P.cols.weight = weight;
    P.cols.hits = hits;
    P.cols.stride = (size_t)score_stride;
    P.src = (const uint8_t*)src;
    P.point_index = point_index;
    P.dst = (uint8_t*)dst;
    P.stats = (uint8_t*)stats;
    P.T_src = T_src;
    P.T_out = T_out;
    P.col0 = (size_t)col0;
    const long tiles = (T_out + LASW_WG - 1) / LASW_WG;
    if (L_dst <= LAS_ENCODE_STAGE_MAX_L && g_las_encode_form == 0) {
        const size_t lds = 16 * (lasw_slots(L_dst) + (point_index ? 0 : lasw_slots(L_src))) + LASW_RED_BYTES;
        void (*kernel)(las_write_params) = point_index ? las_encode_staged_kernel<1>
                                           : (L_src <= 16 * LASW_FEW_CHUNKS ? las_encode_staged_kernel<LASW_FEW_CHUNKS>
                                                                            : las_encode_staged_kernel<LASW_MAX_CHUNKS>);
        int per_cu = 0;                                                // a host-side query: no launch, no synchronisation
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, LASW_WG, lds) != hipSuccess || per_cu < 1) {
            (void)hipGetLastError();
            per_cu = (int)(LASW_CU_LDS / lds);
        }
        per_cu = per_cu < 1 ? 1 : (per_cu > LAS_ENCODE_WG_PER_CU ? LAS_ENCODE_WG_PER_CU : per_cu);
        const long most = (long)per_cu * sn2_cu_count();
        hipLaunchKernelGGL(kernel, dim3((unsigned)(tiles < most ? tiles : most)), dim3(LASW_WG), lds, (hipStream_t)stream, P);
    } else {
        const long most = (long)LAS_ENCODE_WG_PER_CU * sn2_cu_count();
        hipLaunchKernelGGL(las_encode_direct_kernel, dim3((unsigned)(tiles < most ? tiles : most)), dim3(LASW_WG), LASW_RED_BYTES,
                           (hipStream_t)stream, P);
    }
    SN2_RETURN_LAUNCH();
}
