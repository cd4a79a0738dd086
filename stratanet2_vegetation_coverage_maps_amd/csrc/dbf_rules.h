// dbf_rules.h -- the rule of the dBase record annotator (include/strata_hip.h, "dBase records, annotated"), stated once: the decimal
// text of a double at a fixed number of places, the field that text becomes, which byte of the output a byte of a source record
// is, and the cut of the output into tiles.  The kernel of dbf.hip, the host-side checks of sn2_dbf_annotate and a stand-alone
// host program (scripts/dbf_rules_sanitize.cpp: the rule against printf, under a sanitizer) execute these functions.
//
// THE TEXT is that of the EXACT binary value, rounded half-to-even at `decimal` places -- what CPython's format(v, ".10f") and
// glibc's printf("%.10f") print -- made with integer arithmetic only: mantissa and exponent come from the bits, the fraction's
// digits from one 64 x 64 -> 128-bit product and a shift.  No floating-point operation touches the value.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DBF_FN __host__ __device__ __forceinline__
#else
#define DBF_FN inline
#endif

constexpr int DBF_EINVAL = -1, DBF_ELIMIT = -2;         // SN2_EINVAL, SN2_ELIMIT (this header stands without the library's)
constexpr int DBF_MAX_RECORD = 65535;                   // the record length is a uint16 of the file's header
constexpr int DBF_MAX_FIELDS = 255, DBF_MAX_SIZE = 254, DBF_MAX_DECIMAL = 15;
constexpr int DBF_TEXT_MAX = 1 + 16 + 1 + DBF_MAX_DECIMAL;      // sign, the digits of an integer part <= 2^53, point, places
constexpr uint32_t DBF_TILE_BYTES = 16384;              // the output bytes a workgroup composes in LDS
constexpr int DBF_COUNTER_BYTES = 8;                    // the overflow count behind the records

DBF_FN uint64_t dbf_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

DBF_FN uint64_t dbf_pow10(int d) {                      // 0 <= d <= 15
    uint64_t p = 1;
    for (int i = 0; i < d; ++i) p *= 10u;
    return p;
}

// The text of the double with bit pattern `bits` at `decimal` places into text[0 .. DBF_TEXT_MAX) -> its length; -1 for a finite
// |v| >= 2^53 (the field is filled with '*').  0 <= decimal <= DBF_MAX_DECIMAL.
//   v = (-1)^sign M / 2^s with M < 2^53 and 0 <= s <= 1074 (a finite |v| < 2^53 has no positive exponent of two).
//   I = M >> s, F = M - (I << s); G = F 10^decimal < 2^103; r = G >> s < 10^decimal, the remainder G mod 2^s against 2^(s-1): above
//   it, or equal to it with the last kept digit odd, r += 1 (carrying into I).  The sign is '-' whenever the sign bit is set.
DBF_FN int dbf_format(uint64_t bits, int decimal, char* text) {
    const bool neg = (bits >> 63) != 0;
    const uint32_t e = (uint32_t)(bits >> 52) & 0x7FFu;
    const uint64_t frac = bits & 0xFFFFFFFFFFFFFull;
    int len = 0;
    if (e == 0x7FFu) {
        if (frac == 0 && neg) text[len++] = '-';
        const char* w = frac ? "nan" : "inf";
        for (int i = 0; i < 3; ++i) text[len++] = w[i];
        return len;
    }
    if (e >= 1023u + 53u) return -1;
    const uint64_t M = e ? (frac | (1ull << 52)) : frac;
    const uint32_t s = e ? 1075u - e : 1074u;           // 0 .. 1074
    uint64_t I = s < 64 ? M >> s : 0;
    const uint64_t F = s < 64 ? M - (I << s) : M;
    const uint64_t P = dbf_pow10(decimal);
    uint64_t r = 0;
    if (s > 0 && s <= 104) {                            // beyond: G < 2^103 <= 2^(s-1), so r = 0 and nothing rounds up
        const uint64_t lo = F * P, hi = dbf_mulhi(F, P);
        uint64_t rem_hi, rem_lo, half_hi, half_lo;
        if (s < 64) {
            r = (lo >> s) | (hi << (64 - s));
            rem_hi = 0;
            rem_lo = lo & ((1ull << s) - 1);
            half_hi = 0;
            half_lo = 1ull << (s - 1);
        } else if (s == 64) {
            r = hi;
            rem_hi = 0;
            rem_lo = lo;
            half_hi = 0;
            half_lo = 1ull << 63;
        } else {
            r = hi >> (s - 64);
            rem_hi = hi & ((1ull << (s - 64)) - 1);
            rem_lo = lo;
            half_hi = 1ull << (s - 65);
            half_lo = 0;
        }
        const bool above = rem_hi > half_hi || (rem_hi == half_hi && rem_lo > half_lo);
        const bool tie = rem_hi == half_hi && rem_lo == half_lo;
        const bool odd = ((decimal ? r : I) & 1u) != 0;
        if (above || (tie && odd)) {
            if (++r == P) {
                r = 0;
                ++I;
            }
        }
    }
    if (neg) text[len++] = '-';
    char digits[17];
    int nd = 0;
    do {
        digits[nd++] = (char)('0' + (int)(I % 10u));
        I /= 10u;
    } while (I != 0);
    while (nd > 0) text[len++] = digits[--nd];
    if (decimal > 0) {
        text[len++] = '.';
        for (int i = decimal - 1; i >= 0; --i) {
            text[len + i] = (char)('0' + (int)(r % 10u));
            r /= 10u;
        }
        len += decimal;
    }
    return len;
}

// byte c, 0 <= c < size, of the field: the text cut to its first `size` characters and right-justified with spaces
DBF_FN uint8_t dbf_field_byte(const char* text, int len, int size, int c) {
    if (len < 0) return (uint8_t)'*';
    if (len >= size) return (uint8_t)text[c];
    const int pad = size - len;
    return c < pad ? (uint8_t)' ' : (uint8_t)text[c - pad];
}

// ---- the output: K records of Ld = L + n size bytes, record k = the source's L bytes, then the n fields
struct dbf_shape {
    long long K;
    int L, n, size, decimal, Ld;
};

// the argument checks of sn2_dbf_annotate that need no pointer; -> 0 and the bytes of the records and of the whole of dst
DBF_FN int dbf_check_shape(long long K, int L, int n, int size, int decimal, uint64_t* record_bytes, uint64_t* total_bytes) {
    if (K <= 0 || L < 1 || L > DBF_MAX_RECORD || size < 1 || size > DBF_MAX_SIZE) return DBF_EINVAL;
    if (decimal < 0 || decimal > DBF_MAX_DECIMAL || decimal + 2 > size || n < 1 || n > DBF_MAX_FIELDS) return DBF_EINVAL;
    if (L + n * size > DBF_MAX_RECORD) return DBF_EINVAL;
    if ((uint64_t)K > (1ull << 40)) return DBF_ELIMIT;
    *record_bytes = (uint64_t)K * (uint64_t)(L + n * size);
    *total_bytes = (*record_bytes + 7) / 8 * 8 + DBF_COUNTER_BYTES;      // the counter on the next multiple of 8
    return 0;
}

DBF_FN uint64_t dbf_tiles(uint64_t record_bytes) { return (record_bytes + DBF_TILE_BYTES - 1) / DBF_TILE_BYTES; }

// The copied bytes of the output range [o0, o1), o1 - o0 <= DBF_TILE_BYTES, by lane `lane` of `lanes`: consecutive lanes take
// consecutive output bytes.  No load leaves [0, K L) of src, no byte outside [o0, o1) is handed to the sink.
template <typename Sink>
DBF_FN void dbf_copy_range(const uint8_t* src, const dbf_shape& s, uint64_t o0, uint64_t o1, const Sink& sink, uint32_t lane,
                           uint32_t lanes) {
    const uint64_t k0 = o0 / (uint32_t)s.Ld;
    const uint32_t j0 = (uint32_t)(o0 - k0 * (uint32_t)s.Ld);
    const uint32_t span = (uint32_t)(o1 - o0);
    for (uint32_t i = lane; i < span; i += lanes) {
        const uint32_t t = j0 + i, dk = t / (uint32_t)s.Ld, j = t - dk * (uint32_t)s.Ld;
        if (j < (uint32_t)s.L) sink.byte(o0 + i, src[(k0 + dk) * (uint64_t)s.L + j]);
    }
}

// The field bytes of the output range [o0, o1): lane `lane` of `lanes` formats every lanes-th field that has a byte in the range
// and hands the field's bytes inside the range to the sink.  value(k, f) -> the bit pattern of the field's double.  -> the fields
// of this lane that overflowed and whose FIRST byte lies in the range (so every field is counted by exactly one range).
template <typename Value, typename Sink>
DBF_FN uint32_t dbf_field_range(const Value& value, const dbf_shape& s, uint64_t o0, uint64_t o1, const Sink& sink, uint32_t lane,
                                uint32_t lanes) {
    const uint64_t k0 = o0 / (uint32_t)s.Ld, k1 = (o1 - 1) / (uint32_t)s.Ld;
    const uint32_t slots = (uint32_t)(k1 - k0 + 1) * (uint32_t)s.n;          // <= (tile / Ld + 2) n
    uint32_t overflow = 0;
    for (uint32_t i = lane; i < slots; i += lanes) {
        const uint32_t dk = i / (uint32_t)s.n, f = i - dk * (uint32_t)s.n;
        const uint64_t k = k0 + dk;
        const uint64_t a = k * (uint32_t)s.Ld + (uint32_t)s.L + (uint64_t)f * (uint32_t)s.size, b = a + (uint32_t)s.size;
        if (b <= o0 || a >= o1) continue;
        char text[DBF_TEXT_MAX];
        const int len = dbf_format(value(k, (int)f), s.decimal, text);
        overflow += (len < 0 && a >= o0) ? 1u : 0u;
        const int c0 = a < o0 ? (int)(o0 - a) : 0, c1 = b > o1 ? (int)(o1 - a) : s.size;
        for (int c = c0; c < c1; ++c) sink.byte(a + (uint64_t)c, dbf_field_byte(text, len, s.size, c));
    }
    return overflow;
}
