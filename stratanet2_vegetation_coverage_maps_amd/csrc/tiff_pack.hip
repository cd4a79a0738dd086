// tiff_pack.hip -- the band arena of a mosaic atlas turned into the bytes its GeoTIFF files hold after their headers: the rows of
// an uncompressed little-endian TIFF, band-sequential or pixel-interleaved, under predictor 1 or 3, with the per-band statistics
// the header wants.  Host side: geotiff.py (`pack`, `write_atlas`, `write_parcel`, `write_bands`).
//
// Contract (include/strata_hip.h, "GeoTIFF image data"; the rule's functions: tiff_rules.h):
//   - ONE launch for all K canvases, no synchronisation between workgroups, nothing read back: safe to capture;
//   - no store touches a byte outside [data_base_k, data_base_k + block bytes) of a canvas that gets a file, nor outside the
//     statistics block; the padding between the blocks is never written; no load leaves the canvas's (C,H,W) view;
//   - the statistics are integers, reduced per wave and per workgroup first and added with integer atomics: the same input gives
//     the same bytes.
//
// A workgroup finds its canvas in the place table by the wave-uniform search the atlas kernels use (atlas_table.h).
// STAGED form (rows of at most TIFF_STAGE_BYTES = 16 KiB): the workgroup gathers a few consecutive image rows -- R rows with
// R 4 wc <= 16 KiB -- from the C planes with coalesced loads into LDS in ROW order (the PIXEL layout interleaves here), and every
// lane then composes sixteen output bytes at a time from LDS -- the byte planes and the differences of predictor 3 are functions
// of at most two staged floats -- and stores them as one 16-byte word.  17 KiB (the rows, skewed by one word in sixteen against
// bank conflicts) + the reduction's few words per workgroup: eight workgroups fit a CU's 160 KiB, all its wave slots.
// DIRECT form (longer rows): a workgroup takes 16 KiB of one row and reads the at most two source floats of every byte from
// memory.  The bytes are the same: both forms run tiff_write_range over tiff_row_byte.
#include "atlas_table.h"
#include "common.h"
#include "tiff_rules.h"

static_assert(TIFF_EINVAL == SN2_EINVAL && TIFF_ELIMIT == SN2_ELIMIT && TIFF_MAX_BANDS == SN2_MOSAIC_CROP_MAX_BANDS &&
                  TIFF_CANVAS_COLS == SN2_ATLAS_CANVAS_COLS && TIFF_PLACE_COLS == SN2_TIFF_PLACE_COLS &&
                  TIFF_STATS_BYTES == SN2_TIFF_STATS_BYTES && TIFF_LAYOUT_BAND == SN2_TIFF_LAYOUT_BAND &&
                  TIFF_LAYOUT_PIXEL == SN2_TIFF_LAYOUT_PIXEL,
              "tiff_rules.h restates the header's constants");

namespace {

constexpr int TIFF_WG = 256;
constexpr int TIFF_WAVES = TIFF_WG / 64;
int g_tiff_pack_form = 0;                        // sn2_debug_tiff_pack_form: 0 = by row length, 1 = the direct form for every row

struct tiff_params {
    const uint32_t* bands;
    const long long* canvas;
    const long long* place;
    uint8_t* dst;
    int C, K, layout, predictor, force_direct;
};

// the statistics of one band over a thread's floats
struct tiff_band_acc {
    uint32_t n, lo, hi;
    __device__ __forceinline__ void init() {
        n = 0;
        lo = TIFF_KEY_MIN_INIT;
        hi = TIFF_KEY_MAX_INIT;
    }
    __device__ __forceinline__ void add(uint32_t bits) {
        if (tiff_is_nan(bits)) return;
        const uint32_t k = tiff_key(bits);
        ++n;
        lo = k < lo ? k : lo;
        hi = k > hi ? k : hi;
    }
    // wave -> this wave's slot of band c in LDS (red: TIFF_MAX_BANDS * TIFF_WAVES * 3 words); every lane of the wave calls it
    __device__ __forceinline__ void to_wave_slot(uint32_t* red, int c) {
        for (int m = 32; m >= 1; m >>= 1) {
            n += __shfl_xor(n, m, 64);
            const uint32_t l = __shfl_xor(lo, m, 64), h = __shfl_xor(hi, m, 64);
            lo = l < lo ? l : lo;
            hi = h > hi ? h : hi;
        }
        if ((threadIdx.x & 63) == 0) {
            uint32_t* r = red + (c * TIFF_WAVES + (threadIdx.x >> 6)) * 3;
            r[0] = n;
            r[1] = lo;
            r[2] = hi;
        }
    }
};

// after a barrier: thread c of the bands [c0, c1) adds the workgroup's sums of band c to the canvas's statistics
__device__ __forceinline__ void tiff_flush_stats(const uint32_t* red, uint8_t* stats, int c0, int c1) {
    const int c = c0 + (int)threadIdx.x;
    if (c >= c1) return;
    uint32_t n = 0, lo = TIFF_KEY_MIN_INIT, hi = TIFF_KEY_MAX_INIT;
    for (int w = 0; w < TIFF_WAVES; ++w) {
        const uint32_t* r = red + (c * TIFF_WAVES + w) * 3;
        n += r[0];
        lo = r[1] < lo ? r[1] : lo;
        hi = r[2] > hi ? r[2] : hi;
    }
    if (n == 0) return;
    uint8_t* s = stats + (size_t)c * TIFF_STATS_BYTES;
    atomicAdd(reinterpret_cast<unsigned long long*>(s), (unsigned long long)n);
    atomicMin(reinterpret_cast<unsigned int*>(s + 8), lo);
    atomicMax(reinterpret_cast<unsigned int*>(s + 12), hi);
}

struct tiff_global_sink {
    uint8_t* out;                                // the canvas's block, 16-byte aligned
    __device__ __forceinline__ void byte(uint64_t o, uint32_t v) const { out[o] = (uint8_t)v; }
    __device__ __forceinline__ void chunk(uint64_t o, uint32_t a, uint32_t b, uint32_t c, uint32_t d) const {
        *reinterpret_cast<uint4*>(out + o) = make_uint4(a, b, c, d);
    }
};
// A lane composes sixteen consecutive bytes of a byte plane, i.e. reads sixteen consecutive staged floats, so the lanes of a wave
// read words 16 apart: four banks of the 64.  Word i is therefore kept at i + i / 16 -- lane L then starts at 17 L + const, an odd
// multiple, and the 64 lanes fall on 64 banks.
__device__ __forceinline__ uint32_t tiff_skew(uint32_t i) { return i + (i >> 4); }
constexpr uint32_t TIFF_STAGE_WORDS = TIFF_STAGE_BYTES / 4 + TIFF_STAGE_BYTES / 64;
struct tiff_lds_rows {                           // rows q0, q0 + 1, ... of wc floats each, in row order, skewed
    const uint32_t* lds;
    uint32_t q0, wc;
    __device__ __forceinline__ uint32_t word(uint32_t q, uint32_t f) const { return lds[tiff_skew((q - q0) * wc + f)]; }
};
struct tiff_global_rows {
    const uint32_t* view;                        // the canvas's (C,H,W) view
    tiff_shape s;
    int layout;
    __device__ __forceinline__ uint32_t word(uint32_t q, uint32_t f) const { return view[tiff_source_word(layout, s, q, f)]; }
};

__global__ __launch_bounds__(TIFF_WG) void tiff_pack_kernel(tiff_params P) {
    __shared__ __attribute__((aligned(16))) uint32_t stage[TIFF_STAGE_WORDS];
    __shared__ uint32_t red[TIFF_MAX_BANDS * TIFF_WAVES * 3];
    const int k = last_row_at_or_below(P.place, TIFF_PLACE_COLS, 2, P.K, (long long)blockIdx.x);
    const long long* cv = P.canvas + (size_t)k * ATLAS_COLS;
    const long long* pl = P.place + (size_t)k * TIFF_PLACE_COLS;
    const int C = P.C;
    const tiff_shape s = tiff_shape_of(P.layout, (uint32_t)C, (uint32_t)cv[1], (uint32_t)cv[2]);
    const uint32_t* view = P.bands + (size_t)C * (size_t)cv[0];
    const tiff_global_sink sink{P.dst + pl[0]};
    uint8_t* stats = P.dst + P.place[(size_t)P.K * TIFF_PLACE_COLS] + (size_t)k * C * TIFF_STATS_BYTES;
    const uint32_t unit = blockIdx.x - (uint32_t)pl[2];
    const bool pixel = P.layout == TIFF_LAYOUT_PIXEL;
    const size_t HW = (size_t)s.H * s.W;
    tiff_band_acc acc;
    if (tiff_staged(s, P.force_direct)) {
        const uint32_t R = tiff_group_rows(s);
        const uint32_t groups = (s.H + R - 1) / R;
        const uint32_t g = pixel ? unit : unit % groups;
        const uint32_t r0 = g * R;
        const uint32_t n = s.H - r0 < R ? s.H - r0 : R;                 // image rows of this group, >= 1
        const uint32_t nw = n * s.W;                                     // floats per band: contiguous in the plane
        const int c0 = pixel ? 0 : (int)(unit / groups), c1 = pixel ? C : c0 + 1;
        for (int c = c0; c < c1; ++c) {
            const uint32_t* src = view + (size_t)c * HW + (size_t)r0 * s.W;
            acc.init();
            if (pixel) {
                for (uint32_t i = threadIdx.x; i < nw; i += TIFF_WG) {
                    const uint32_t v = src[i];
                    stage[tiff_skew(i * (uint32_t)C + (uint32_t)c)] = v;
                    acc.add(v);
                }
            } else {
                for (uint32_t i = threadIdx.x; i < nw; i += TIFF_WG) {
                    const uint32_t v = src[i];
                    stage[tiff_skew(i)] = v;
                    acc.add(v);
                }
            }
            acc.to_wave_slot(red, c);
        }
        __syncthreads();
        tiff_flush_stats(red, stats, c0, c1);
        const uint32_t q0 = pixel ? r0 : (uint32_t)c0 * s.H + r0;
        const tiff_lds_rows rows{stage, q0, s.wc};
        tiff_write_range(rows, sink, s, P.predictor, (uint64_t)q0 * s.row_bytes, (uint64_t)(q0 + n) * s.row_bytes, threadIdx.x, TIFF_WG);
    } else {
        const uint32_t pieces = (uint32_t)((s.row_bytes + TIFF_STAGE_BYTES - 1) / TIFF_STAGE_BYTES);
        const uint32_t q = unit / pieces, piece = unit % pieces;
        const uint64_t o0 = (uint64_t)q * s.row_bytes + (uint64_t)piece * TIFF_STAGE_BYTES;
        const uint64_t end = (uint64_t)(q + 1) * s.row_bytes;
        const uint64_t o1 = o0 + TIFF_STAGE_BYTES < end ? o0 + TIFF_STAGE_BYTES : end;
        // the statistics: the piece's share of the row's floats, every float of the row in exactly one piece
        const uint32_t f0 = piece * (TIFF_STAGE_BYTES / 4);
        const uint32_t f1 = s.wc - f0 < TIFF_STAGE_BYTES / 4 ? s.wc : f0 + TIFF_STAGE_BYTES / 4;
        const int c0 = pixel ? 0 : (int)(q / s.H), c1 = pixel ? C : c0 + 1;
        for (int c = c0; c < c1; ++c) {
            acc.init();
            if (pixel) {
                const uint32_t first = f0 + ((uint32_t)c + (uint32_t)C - f0 % (uint32_t)C) % (uint32_t)C;     // the first f >= f0 of band c
                const uint32_t* src = view + (size_t)c * HW + (size_t)q * s.W;
                for (uint64_t f = (uint64_t)first + (uint64_t)threadIdx.x * C; f < f1; f += (uint64_t)TIFF_WG * C) acc.add(src[f / (uint32_t)C]);
            } else {
                const uint32_t* src = view + (size_t)q * s.W;
                for (uint64_t f = (uint64_t)f0 + threadIdx.x; f < f1; f += TIFF_WG) acc.add(src[f]);
            }
            acc.to_wave_slot(red, c);
        }
        __syncthreads();
        tiff_flush_stats(red, stats, c0, c1);
        const tiff_global_rows rows{view, s, P.layout};
        tiff_write_range(rows, sink, s, P.predictor, o0, o1, threadIdx.x, TIFF_WG);
    }
}
}  // namespace

extern "C" int sn2_tiff_pack_stage_max(void) { return (int)TIFF_STAGE_BYTES; }

extern "C" int sn2_debug_tiff_pack_form(int form) {
    if (form != 0 && form != 1) return SN2_EINVAL;
    g_tiff_pack_form = form;
    return 0;
}

extern "C" int sn2_tiff_place_table(int C, int K, const long long* canvas_host, int layout, const unsigned char* skip, long long* place) {
    if (!canvas_host || !place) return SN2_EINVAL;
    SN2_TRY(atlas_check_table(K, canvas_host));
    return tiff_place_table(layout, C, K, canvas_host, skip, g_tiff_pack_form, place);
}

extern "C" int sn2_tiff_pack(const float* bands, int C, int K, const long long* canvas_host, const long long* canvas_dev,
                             const long long* place_host, const long long* place_dev, int layout, int predictor, void* dst,
                             size_t dst_bytes, void* stream) {
    if (!bands || !canvas_host || !canvas_dev || !place_host || !place_dev || !dst) return SN2_EINVAL;
    if (C < 1 || C > SN2_MOSAIC_CROP_MAX_BANDS) return SN2_EINVAL;
    if (layout != SN2_TIFF_LAYOUT_BAND && layout != SN2_TIFF_LAYOUT_PIXEL) return SN2_EINVAL;
    if (predictor != 1 && predictor != 3) return SN2_EINVAL;
    SN2_TRY(atlas_check_table(K, canvas_host));
    SN2_TRY(tiff_check_place(layout, C, K, canvas_host, g_tiff_pack_form, place_host));
    const long long* last = place_host + (size_t)K * TIFF_PLACE_COLS;
    if ((uintptr_t)dst % 16 != 0 || last[0] % 16 != 0) return SN2_EINVAL;
    if (dst_bytes < (size_t)last[3]) return SN2_EINVAL;
    if (last[2] == 0) return 0;                                    // no canvas gets a file
    tiff_params P = {};
    P.bands = reinterpret_cast<const uint32_t*>(bands);
    P.canvas = canvas_dev;
    P.place = place_dev;
    P.dst = (uint8_t*)dst;
    P.C = C;
    P.K = K;
    P.layout = layout;
    P.predictor = predictor;
    P.force_direct = g_tiff_pack_form;
    hipLaunchKernelGGL(tiff_pack_kernel, dim3((unsigned)last[2]), dim3(TIFF_WG), 0, (hipStream_t)stream, P);
    SN2_RETURN_LAUNCH();
}
