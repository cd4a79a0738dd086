// tiff_rules.h -- the rule of the GeoTIFF band packer (include/strata_hip.h, "GeoTIFF image data"), stated once: which source float
// a float of an output row is, which byte of the image data block a byte of a row is under predictor 1 and 3, how the extrema
// of a band are ordered, how a canvas is cut into workgroups and the place table that follows from it.  The kernel of
// tiff_pack.hip, the host-side checks of sn2_tiff_pack / sn2_tiff_place_table and a stand-alone host program
// (scripts/tiff_pack_sanitize.cpp: the rows under a sanitizer) execute these functions.
// Predictor 3 is the floating-point predictor of TIFF Technical Note 3 as libtiff's fpDiff applies it on a little-endian host.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TIFF_FN __host__ __device__ __forceinline__
#else
#define TIFF_FN inline
#endif

constexpr int TIFF_EINVAL = -1, TIFF_ELIMIT = -2;       // SN2_EINVAL, SN2_ELIMIT (this header stands without the library's)
constexpr int TIFF_LAYOUT_BAND = 0, TIFF_LAYOUT_PIXEL = 1;
constexpr int TIFF_MAX_BANDS = 8;                       // SN2_MOSAIC_CROP_MAX_BANDS
constexpr int TIFF_CANVAS_COLS = 8;                     // SN2_ATLAS_CANVAS_COLS
constexpr int TIFF_PLACE_COLS = 4;                      // [0] data_base [1] no file [2] exclusive prefix of workgroups [3] block bytes
constexpr int TIFF_STATS_BYTES = 16;                    // per (canvas, band): uint64 count, uint32 key of the minimum, of the maximum
constexpr uint32_t TIFF_STAGE_BYTES = 16384;            // a workgroup's rows in LDS; also the piece of a longer row a workgroup takes
constexpr uint32_t TIFF_KEY_MIN_INIT = 0xFFFFFFFFu, TIFF_KEY_MAX_INIT = 0u;     // neither is the key of a value that is not NaN

// ---- the order of the extrema: -0 < +0, the infinities are ordinary values.  key and bits map onto each other both ways.
TIFF_FN uint32_t tiff_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
TIFF_FN uint32_t tiff_key_bits(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }
TIFF_FN bool tiff_is_nan(uint32_t bits) { return (bits & 0x7FFFFFFFu) > 0x7F800000u; }

// ---- the rows of one canvas's image data block
struct tiff_shape {
    uint32_t C, H, W;
    uint32_t wc;          // floats per row
    uint32_t rows;        // rows of the block
    uint32_t stride;      // the predictor's distance in bytes = samples per pixel of a row
    uint64_t row_bytes;   // 4 wc
    uint64_t block_bytes; // rows * row_bytes
};
TIFF_FN tiff_shape tiff_shape_of(int layout, uint32_t C, uint32_t H, uint32_t W) {
    tiff_shape s;
    s.C = C;
    s.H = H;
    s.W = W;
    const bool pixel = layout == TIFF_LAYOUT_PIXEL;
    const uint64_t wc = pixel ? (uint64_t)W * C : (uint64_t)W;
    s.wc = (uint32_t)wc;                                    // (callers refuse a block of 2^32 bytes first: wc < 2^30)
    s.rows = pixel ? H : C * H;
    s.stride = pixel ? C : 1u;
    s.row_bytes = 4 * wc;
    s.block_bytes = s.row_bytes * (pixel ? (uint64_t)H : (uint64_t)C * H);
    return s;
}
// float f of row q, as a word index into the canvas's (C,H,W) view
TIFF_FN size_t tiff_source_word(int layout, const tiff_shape& s, uint32_t q, uint32_t f) {
    if (layout == TIFF_LAYOUT_PIXEL) return (size_t)(f % s.C) * s.H * s.W + (size_t)q * s.W + f / s.C;
    return (size_t)q * s.W + f;                             // q = c H + r: the view is band-major as the block is
}
// the band of float f of row q
TIFF_FN uint32_t tiff_source_band(int layout, const tiff_shape& s, uint32_t q, uint32_t f) {
    return layout == TIFF_LAYOUT_PIXEL ? f % s.C : q / s.H;
}

// ---- a byte of a row.  Row: word(f) = the bits of float f of the row, 0 <= f < wc.
// predictor 1: byte j is byte j % 4 of float j / 4, the fp32's own bytes.
// predictor 3: t[j] = byte 3 - j / wc of float j % wc (plane 0 = the sign and exponent bytes); out[j] = t[j] for j < stride, else
// (t[j] - t[j - stride]) mod 256.  Nothing carries from one row to the next.
template <typename Row>
TIFF_FN uint32_t tiff_plane_byte(const Row& row, uint32_t wc, uint32_t j) {
    const uint32_t p = (uint32_t)(j >= wc) + (uint32_t)(j >= 2 * (uint64_t)wc) + (uint32_t)(j >= 3 * (uint64_t)wc);
    return (row.word(j - p * wc) >> (8 * (3 - p))) & 0xFFu;
}
template <typename Row>
TIFF_FN uint32_t tiff_row_byte(const Row& row, uint32_t wc, uint32_t stride, int predictor, uint32_t j) {
    if (predictor == 1) return (row.word(j >> 2) >> (8 * (j & 3u))) & 0xFFu;
    const uint32_t t = tiff_plane_byte(row, wc, j);
    if (j < stride) return t;
    return (t - tiff_plane_byte(row, wc, j - stride)) & 0xFFu;
}

// ---- the cut into workgroups.  STAGED (row_bytes <= TIFF_STAGE_BYTES): a workgroup takes R = tiff_group_rows consecutive image
// rows -- of one band in the BAND layout, of all C bands in the PIXEL layout --, whole output rows that are contiguous in the block,
// as many as fit TIFF_STAGE_BYTES.  (Groups of 4 KiB, four times the workgroups, were measured: sixteen 1 ha canvases in the BAND
// layout under predictor 3 went from 0.017 to 0.013 ms, the PIXEL layout from 0.019 to 0.025 and one 335 x 335 canvas under
// predictor 1 from 0.008 to 0.017 -- every workgroup ends in three atomics on its band's sixteen bytes.  Left at one size.)
// DIRECT: a workgroup takes one piece of TIFF_STAGE_BYTES bytes of one row.
TIFF_FN bool tiff_staged(const tiff_shape& s, int force_direct) { return !force_direct && s.row_bytes <= TIFF_STAGE_BYTES; }
TIFF_FN uint32_t tiff_group_rows(const tiff_shape& s) {
    const uint32_t fit = (uint32_t)(TIFF_STAGE_BYTES / s.row_bytes);                     // >= 1 in the staged form
    return fit < s.H ? fit : s.H;
}
TIFF_FN uint64_t tiff_units(int layout, const tiff_shape& s, int force_direct) {
    if (tiff_staged(s, force_direct)) {
        const uint32_t R = tiff_group_rows(s);
        const uint64_t groups = (s.H + R - 1) / R;
        return layout == TIFF_LAYOUT_PIXEL ? groups : groups * s.C;
    }
    return (uint64_t)s.rows * ((s.row_bytes + TIFF_STAGE_BYTES - 1) / TIFF_STAGE_BYTES);
}

// ---- the place table: (K+1) rows of TIFF_PLACE_COLS int64.  Row k: [0] data_base_k, a multiple of 16: the blocks follow one another
// in canvas order, each rounded up to 16 bytes  [1] 1 = no file: no bytes, no workgroups  [2] the exclusive prefix of tiff_units
// [3] the block's bytes (0 without a file).  Row K: [0] the offset of the statistics block (K C TIFF_STATS_BYTES bytes)
// [1] 0  [2] the workgroups in all  [3] the bytes in all, statistics included.
static inline int tiff_place_row(int layout, int C, const long long* canvas_row, long long skip, int force_direct, const long long* prev,
                                 long long* row) {
    const long long H = canvas_row[1], W = canvas_row[2];
    if (H <= 0 || W <= 0 || H > 0x7fffffffLL || W > 0x7fffffffLL || H * W >= (1LL << 31)) return TIFF_EINVAL;      // not an atlas row
    if (skip != 0 && skip != 1) return TIFF_EINVAL;
    if ((unsigned long long)C * (unsigned long long)H * (unsigned long long)W >= (1ULL << 30)) {
        if (!skip) return TIFF_ELIMIT;                                                    // a block of 2^32 bytes or more
    }
    unsigned long long bytes = 0, units = 0;
    if (!skip) {
        const tiff_shape s = tiff_shape_of(layout, (uint32_t)C, (uint32_t)H, (uint32_t)W);
        bytes = s.block_bytes;
        units = tiff_units(layout, s, force_direct);
    }
    row[0] = prev[0];
    row[1] = skip;
    row[2] = prev[2];
    row[3] = (long long)bytes;
    row[TIFF_PLACE_COLS + 0] = prev[0] + (long long)((bytes + 15) / 16 * 16);
    row[TIFF_PLACE_COLS + 2] = prev[2] + (long long)units;
    if (row[TIFF_PLACE_COLS + 0] >= (1LL << 32)) return TIFF_ELIMIT;
    if (row[TIFF_PLACE_COLS + 2] > 0x7fffffffLL) return TIFF_ELIMIT;
    return 0;
}
// writes the table from the canvas table and the K flags (NULL: every canvas gets a file)
static inline int tiff_place_table(int layout, int C, int K, const long long* canvas, const unsigned char* skip, int force_direct,
                                   long long* place) {
    if (!canvas || !place || K <= 0) return TIFF_EINVAL;
    if (C < 1 || C > TIFF_MAX_BANDS) return TIFF_EINVAL;
    if (layout != TIFF_LAYOUT_BAND && layout != TIFF_LAYOUT_PIXEL) return TIFF_EINVAL;
    long long next[2 * TIFF_PLACE_COLS] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < K; ++k) {
        long long row[2 * TIFF_PLACE_COLS];
        const int rc = tiff_place_row(layout, C, canvas + (size_t)k * TIFF_CANVAS_COLS, skip ? (long long)(skip[k] != 0) : 0, force_direct,
                                      next + TIFF_PLACE_COLS, row);
        if (rc) return rc;
        for (int j = 0; j < TIFF_PLACE_COLS; ++j) place[(size_t)k * TIFF_PLACE_COLS + j] = row[j];
        for (int j = 0; j < 2 * TIFF_PLACE_COLS; ++j) next[j] = row[j];
    }
    long long* last = place + (size_t)K * TIFF_PLACE_COLS;
    last[0] = next[TIFF_PLACE_COLS + 0];
    last[1] = 0;
    last[2] = next[TIFF_PLACE_COLS + 2];
    last[3] = last[0] + (long long)K * C * TIFF_STATS_BYTES;
    if (last[3] >= (1LL << 32)) return TIFF_ELIMIT;
    return 0;
}
// a host table is taken only if it is what tiff_place_table writes for its own flags: the kernel indexes dst by it
static inline int tiff_check_place(int layout, int C, int K, const long long* canvas, int force_direct, const long long* place) {
    if (!canvas || !place || K <= 0) return TIFF_EINVAL;
    long long prev[TIFF_PLACE_COLS] = {0, 0, 0, 0};
    for (int k = 0; k < K; ++k) {
        const long long* r = place + (size_t)k * TIFF_PLACE_COLS;
        long long want[2 * TIFF_PLACE_COLS];
        const int rc = tiff_place_row(layout, C, canvas + (size_t)k * TIFF_CANVAS_COLS, r[1], force_direct, prev, want);
        if (rc) return rc;
        for (int j = 0; j < TIFF_PLACE_COLS; ++j)
            if (r[j] != want[j]) return TIFF_EINVAL;
        prev[0] = want[TIFF_PLACE_COLS + 0];
        prev[2] = want[TIFF_PLACE_COLS + 2];
    }
    const long long* last = place + (size_t)K * TIFF_PLACE_COLS;
    const long long total = prev[0] + (long long)K * C * TIFF_STATS_BYTES;
    if (total >= (1LL << 32)) return TIFF_ELIMIT;
    if (last[0] != prev[0] || last[1] != 0 || last[2] != prev[2] || last[3] != total) return TIFF_EINVAL;
    return 0;
}

// ---- the bytes [o0, o1) of a block, as a workgroup writes them.  Rows: word(q, f) = the bits of float f of row q.  Sink: byte(o, v)
// and, for o a multiple of 16, chunk(o, w0, w1, w2, w3).  The block starts 16-byte aligned, so the pieces before the first and
// after the last multiple of 16 go out byte by byte and nothing outside [o0, o1) is touched.
template <typename Rows>
struct tiff_row_of {
    const Rows& rows;
    uint32_t q;
    TIFF_FN uint32_t word(uint32_t f) const { return rows.word(q, f); }
};
template <typename Rows>
TIFF_FN uint32_t tiff_block_byte(const Rows& rows, const tiff_shape& s, int predictor, uint32_t q, uint32_t j) {
    const tiff_row_of<Rows> row{rows, q};
    return tiff_row_byte(row, s.wc, s.stride, predictor, j);
}
template <typename Rows, typename Sink>
TIFF_FN void tiff_write_range(const Rows& rows, const Sink& sink, const tiff_shape& s, int predictor, uint64_t o0, uint64_t o1,
                              uint32_t lane, uint32_t lanes) {
    const uint32_t rb = (uint32_t)s.row_bytes;
    uint64_t a0 = (o0 + 15) / 16 * 16, a1 = o1 / 16 * 16;
    if (a0 > o1) a0 = o1;
    if (a1 < a0) a1 = a0;
    for (uint64_t o = o0 + lane; o < a0; o += lanes) sink.byte(o, tiff_block_byte(rows, s, predictor, (uint32_t)(o / rb), (uint32_t)(o % rb)));
    for (uint64_t o = a1 + lane; o < o1; o += lanes) sink.byte(o, tiff_block_byte(rows, s, predictor, (uint32_t)(o / rb), (uint32_t)(o % rb)));
    for (uint64_t o = a0 + 16 * (uint64_t)lane; o < a1; o += 16 * (uint64_t)lanes) {
        // tiff_row_byte for sixteen bytes in a row, with running cursors in place of its divisions: (p, f) = the plane and the float
        // of t[j], (pp, pf) those of t[j - stride] -- it rests on byte 0 of the row until j reaches the stride
        uint32_t q = (uint32_t)((uint32_t)o / rb), j = (uint32_t)o - q * rb;
        uint32_t w[4];
        if (predictor == 1) {                                           // o and the rows are multiples of 4: whole floats
            for (int d = 0; d < 4; ++d) {
                w[d] = rows.word(q, j >> 2);
                if ((j += 4) == rb) {
                    j = 0;
                    ++q;
                }
            }
        } else {
            const uint32_t wc = s.wc, stride = s.stride;
            uint32_t p = (uint32_t)(j >= wc) + (uint32_t)(j >= 2 * (uint64_t)wc) + (uint32_t)(j >= 3 * (uint64_t)wc), f = j - p * wc;
            uint32_t pp = 0, pf = 0;
            if (j >= stride) {
                const uint32_t b = j - stride;
                pp = (uint32_t)(b >= wc) + (uint32_t)(b >= 2 * (uint64_t)wc) + (uint32_t)(b >= 3 * (uint64_t)wc);
                pf = b - pp * wc;
            }
            for (int d = 0; d < 4; ++d) {
                uint32_t v = 0;
                for (int b = 0; b < 4; ++b) {
                    uint32_t t = (rows.word(q, f) >> (8 * (3 - p))) & 0xFFu;
                    if (j >= stride) {
                        t = (t - ((rows.word(q, pf) >> (8 * (3 - pp))) & 0xFFu)) & 0xFFu;
                        if (++pf == wc) {
                            pf = 0;
                            ++pp;
                        }
                    }
                    v |= t << (8 * b);
                    if (++f == wc) {
                        f = 0;
                        ++p;
                    }
                    if (++j == rb) {
                        j = 0;
                        ++q;
                        p = f = pp = pf = 0;
                    }
                }
                w[d] = v;
            }
        }
        sink.chunk(o, w[0], w[1], w[2], w[3]);
    }
}
