// las_write_rules.h -- the rule of the LAS encoder (include/strata_hip.h, "LAS point records, written"), stated once: which
// bytes of an output record are the source's, how the classification is decided, which extra bytes are appended, and the layout
// of the statistics.  The kernels of las_write.hip, the host-side checks of sn2_las_encode and a stand-alone host program
// (scripts/las_write_sanitize.cpp: the composition of one record under a sanitizer) execute these functions.
// The record layout is that of las_rules.h, OUR reading of the ASPRS LAS 1.0-1.4 specification; the class codes (low vegetation 3,
// ground 2, medium 4, high 5) are the caller's, the defaults the specification's table of standard classes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "las_rules.h"

#if defined(__HIPCC__)
#define LAS_FN_MEMBER __host__ __device__ __forceinline__
#else
#define LAS_FN_MEMBER inline
#endif
// loops over the eight score rows index registers: they must be unrolled on the device, or the rows go to scratch
#if defined(__clang__)
#define LAS_UNROLL _Pragma("unroll")
#else
#define LAS_UNROLL
#endif

// ---- the statistics block: SN2_LAS_STATS_BYTES of device memory, 8-byte aligned, initialised by the caller
//   byte   0: int32  min[3]        raw X, Y, Z of the records written (initialise to INT32_MAX)
//   byte  12: int32  max[3]                                           (initialise to INT32_MIN)
//   byte  24: uint64 by_return[15] return number r, 1 <= r <= 15, in bin r - 1
//   byte 144: uint64 n_bad         point_index entries outside [0, T_src)
//   byte 152: uint64 n_scored      records with hits > 0
constexpr int LAS_STATS_BYTES = 160;
constexpr int LAS_STATS_OFF_MIN = 0, LAS_STATS_OFF_MAX = 12, LAS_STATS_OFF_BY_RETURN = 24, LAS_STATS_OFF_N_BAD = 144,
              LAS_STATS_OFF_N_SCORED = 152;
constexpr int LAS_STATS_RETURN_BINS = 15;

// ---- the appended extra bytes: bits 0..7 = rows 0..7 of `scores` (fp32), bit 8 = weight (fp32), bit 9 = hits (uint16)
constexpr unsigned LAS_FIELD_MASK_ALL = 0x3FFu;
constexpr int LAS_FIELD_HITS_BIT = 9;
LAS_FN int las_write_extra_bytes(unsigned mask) {
    int n = 0;
    for (int k = 0; k < 9; ++k) n += (int)((mask >> k) & 1u);
    return 4 * n + 2 * (int)((mask >> LAS_FIELD_HITS_BIT) & 1u);
}
LAS_FN uint32_t las_write_hits16(int hits) { return hits < 0 ? 0u : (hits > 65535 ? 65535u : (uint32_t)hits); }

// ---- the classification: the largest of the four class probabilities, strictly -- ties go to the lowest index, a NaN never wins
LAS_FN int las_write_best(float p0, float p1, float p2, float p3) {
    int best = 0;
    float top = p0;
    if (p1 > top) { best = 1; top = p1; }
    if (p2 > top) { best = 2; top = p2; }
    if (p3 > top) { best = 3; top = p3; }
    return best;
}
// four codes of 0..255 in one word, code k in byte k (a kernel argument indexed at run time would go to scratch)
LAS_FN uint32_t las_write_pack_codes(const int* codes) {
    return (uint32_t)codes[0] | ((uint32_t)codes[1] << 8) | ((uint32_t)codes[2] << 16) | ((uint32_t)codes[3] << 24);
}
// the byte that holds the class, patched: formats 6-10 the whole of byte 16; formats 0-5 the low five bits of byte 15, the synthetic,
// key-point and withheld flags in bits 5-7 kept
LAS_FN uint32_t las_write_class_byte(int format, uint32_t old_byte, int code) {
    return las_extended(format) ? (uint32_t)code & 0xFFu : ((old_byte & 0xE0u) | ((uint32_t)code & 0x1Fu));
}
LAS_FN int las_write_max_code(int format) { return las_extended(format) ? 255 : 31; }

// ---- the rule of one launch
struct las_write_rule {
    int format, L_src, E;          // L_dst = L_src + E
    unsigned mask;                 // field_mask
    int class_mode;                // 0: the class field is left alone, 1: decided from rows 4..7 of scores
    uint32_t codes;                // las_write_pack_codes
    int unscored;                  // the code of a point with hits == 0; -1: the source's byte stays
};
struct las_score_cols {            // NULL, all three, exactly when mask == 0 and class_mode == 0
    const float* scores;           // (8, stride)
    const float* weight;
    const int* hits;
    size_t stride;
};
// what a record gave to the statistics
struct las_written {
    int32_t X, Y, Z;
    uint32_t return_num;
    bool bad, scored;
};

// bytes s .. s + 3 of the eight bytes hi:lo (v_alignbyte_b32 on the device)
LAS_FN uint32_t las_write_alignbyte(uint32_t hi, uint32_t lo, uint32_t s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, s);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * s));
#endif
}
// the four bytes of an fp32 as they stand in memory: a NaN keeps its payload
LAS_FN uint32_t las_write_float_bits(const float* p) {
    uint32_t u;
    memcpy(&u, p, 4);
    return u;
}

// one point's score column as the composition needs it: loaded ahead of the record's bytes (the staged kernel loads the next
// tile's while it composes this one).  Only what the rule uses is loaded, and only column c.
struct las_point_scores {
    uint32_t v[8];       // rows 0..7 of scores as bits: those of the mask, and rows 4..7 with class_mode 1
    uint32_t weight;
    int hits;            // 0 without a hits row
};
LAS_FN las_point_scores las_load_scores(const las_score_cols& S, size_t c, const las_write_rule& R) {
    las_point_scores P = {};
    if (S.hits) P.hits = S.hits[c];
    const unsigned rows = (R.mask & 0xFFu) | (R.class_mode == 1 ? 0xF0u : 0u);
    LAS_UNROLL
    for (int k = 0; k < 8; ++k)
        if ((rows >> k) & 1u) P.v[k] = las_write_float_bits(S.scores + (size_t)k * S.stride + c);
    if ((R.mask >> 8) & 1u) P.weight = las_write_float_bits(S.weight + c);
    return P;
}
LAS_FN float las_write_bits_float(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// ---- byte sources: `word(w)` is the aligned 32-bit word w of the source block
// a staged block (LDS on the device): the word after the block's last is a slack word, so every word(w) the composition asks
// for exists
struct las_staged_words {
    const uint32_t* w;
    LAS_FN_MEMBER uint32_t word(size_t i) const { return w[i]; }
};
// a block in memory of `limit` bytes, 4-byte aligned: a word wholly inside is one load, the block's last odd bytes are read one
// by one, and nothing at or beyond `limit` is touched (the bytes there read as zero)
struct las_guarded_words {
    const uint8_t* p;
    size_t limit;
    LAS_FN_MEMBER uint32_t word(size_t i) const {
        const size_t at = 4 * i;
        if (at + 4 <= limit) return *reinterpret_cast<const uint32_t*>(p + at);
        uint32_t v = 0;
        for (int k = 0; k < 3; ++k)
            if (at + k < limit) v |= (uint32_t)p[at + k] << (8 * k);
        return v;
    }
};
// ---- sinks: a record leaves as a stream of its bytes in order, `begin(d0)` at its first byte, then push4 (four bytes), push (n <
// 4 bytes, n the same for every lane), `finish`
// one byte per store: device memory (the direct form) or host memory
struct las_byte_stream {
    uint8_t* p;
    size_t at;
    LAS_FN_MEMBER void begin(size_t d0) { at = d0; }
    LAS_FN_MEMBER void push(uint32_t v, int n) {
        for (int k = 0; k < n; ++k) p[at + k] = (uint8_t)(v >> (8 * k));
        at += (size_t)n;
    }
    LAS_FN_MEMBER void push_first(uint32_t v) { push(v, 4); }
    LAS_FN_MEMBER void push4(uint32_t v) { push(v, 4); }
    LAS_FN_MEMBER void finish() {}
};
// aligned 32-bit stores for every word the record owns alone, single bytes for the word it shares with the record before it and
// the one it shares with the record after it (LDS on the device: with an odd L_dst neighbouring lanes' records share words).  `p` is
// 4-byte aligned.  A record holds 20 bytes or more, so its first push fills the first word.
struct las_word_stream {
    uint8_t* p;
    size_t pos;          // the aligned byte offset of the next word
    uint64_t acc;        // the bytes not yet stored, lowest first
    uint32_t n;          // how many: 0..3 between pushes
    LAS_FN_MEMBER void begin(size_t d0) {
        pos = d0 & ~(size_t)3;
        n = (uint32_t)(d0 & 3);
        acc = 0;
    }
    // the record's first four bytes: the low n bytes of the first word are the neighbour's
    LAS_FN_MEMBER void push_first(uint32_t v) {
        acc = (uint64_t)v << (8 * n);
        const uint32_t w = (uint32_t)acc;
        if (n == 0) {
            *reinterpret_cast<uint32_t*>(p + pos) = w;
        } else {
            for (uint32_t k = 1; k < 4; ++k)
                if (k >= n) p[pos + k] = (uint8_t)(w >> (8 * k));
        }
        acc >>= 32;
        pos += 4;
    }
    LAS_FN_MEMBER void push4(uint32_t v) {
        acc |= (uint64_t)v << (8 * n);
        *reinterpret_cast<uint32_t*>(p + pos) = (uint32_t)acc;
        acc >>= 32;
        pos += 4;
    }
    LAS_FN_MEMBER void push(uint32_t v, int nb) {
        acc |= (uint64_t)(v & ((1u << (8 * nb)) - 1u)) << (8 * n);
        n += (uint32_t)nb;
        if (n >= 4) {
            *reinterpret_cast<uint32_t*>(p + pos) = (uint32_t)acc;
            acc >>= 32;
            pos += 4;
            n -= 4;
        }
    }
    LAS_FN_MEMBER void finish() {
        for (uint32_t k = 0; k < 3; ++k)
            if (k < n) p[pos + k] = (uint8_t)(acc >> (8 * k));
    }
};

// Output record at byte d0 of `dst` from the source record at byte s0 of `src` (have_src false: a bad index, L_dst zero bytes)
// and the point's scores P.  Every byte of [d0, d0 + L_dst) is written and none outside; of the source, words that overlap
// [s0, s0 + L_src) are asked for and none further than one word beyond.
template <class Src, class Sink>
LAS_FN las_written las_compose(const Src& src, size_t s0, bool have_src, Sink dst, size_t d0, const las_write_rule& R,
                               const las_point_scores& P) {
    las_written out = {};
    const int L_dst = R.L_src + R.E;
    dst.begin(d0);
    if (!have_src) {
        dst.push_first(0u);
        int b = 4;
        for (; b + 4 <= L_dst; b += 4) dst.push4(0u);
        if (b < L_dst) dst.push(0u, L_dst - b);
        dst.finish();
        out.bad = true;
        return out;
    }
    const bool ext = las_extended(R.format);
    const int hits = P.hits;
    out.scored = hits > 0;
    // the classification: decided first, set as its word goes by
    int code = -1;
    if (R.class_mode == 1) {
        code = R.unscored;
        if (out.scored) {
            const int best = las_write_best(las_write_bits_float(P.v[4]), las_write_bits_float(P.v[5]), las_write_bits_float(P.v[6]),
                                            las_write_bits_float(P.v[7]));
            code = (int)((R.codes >> (8 * best)) & 0xFFu);
        }
    }
    // the source's bytes, four at a time from the two aligned words around them
    const uint32_t sh = (uint32_t)(s0 & 3);
    size_t wi = s0 >> 2;
    uint32_t lo = src.word(wi), iw = 0;
    int b = 0;
    for (; b + 4 <= R.L_src; b += 4) {
        const uint32_t hi = src.word(++wi);
        uint32_t v = las_write_alignbyte(hi, lo, sh);
        lo = hi;
        if (b == LAS_OFF_X) {
            out.X = (int32_t)v;
            dst.push_first(v);
            continue;
        }
        if (b == LAS_OFF_Y) out.Y = (int32_t)v;
        else if (b == LAS_OFF_Z) out.Z = (int32_t)v;
        else if (b == LAS_OFF_INTENSITY) {                 // intensity, byte 14, byte 15
            iw = v;
            if (!ext && code >= 0) v = (v & 0x00FFFFFFu) | (las_write_class_byte(R.format, v >> 24, code) << 24);
        } else if (b == 16) {                              // bytes 16..19: every format has them (L_src >= 20)
            if (ext && code >= 0) v = (v & 0xFFFFFF00u) | las_write_class_byte(R.format, v & 0xFFu, code);
        }
        dst.push4(v);
    }
    if (b < R.L_src) dst.push(las_write_alignbyte(src.word(wi + 1), lo, sh), R.L_src - b);
    out.return_num = las_return_num((iw >> 16) & 0xFFu, ext);
    // the extra bytes, in ascending bit order: the fp32's own four bytes, no arithmetic
    LAS_UNROLL
    for (int k = 0; k < 8; ++k)
        if ((R.mask >> k) & 1u) dst.push4(P.v[k]);
    if ((R.mask >> 8) & 1u) dst.push4(P.weight);
    if ((R.mask >> LAS_FIELD_HITS_BIT) & 1u) dst.push(las_write_hits16(hits), 2);
    dst.finish();
    return out;
}
