// The rule of the dBase record annotator (csrc/dbf_rules.h: dbf_format, dbf_field_byte, dbf_copy_range and dbf_field_range over the
// tiles -- the functions the kernel of dbf.hip runs) on the CPU, for a run under a sanitizer.  A stand-alone program: nothing of
// the library is loaded.  Every buffer is allocated at its exact size -- the K L source bytes, the R C values, the K row indices, the
// K Ld output bytes, a text of DBF_TEXT_MAX characters -- so a byte read or written outside the rule's bounds is reported.
//   1. dbf_format against snprintf("%.*f") over the planted values (ties, the smallest magnitudes, the neighbours of 1 and of 2^53)
//      at every decimal 0..15, and over 10^6 doubles drawn as random bit patterns with |v| < 2^53 at decimal 10 and at a random one;
//      NaN, the infinities and the overflow against their stated texts.
//   2. Every tile of the cut walked as the kernel walks it, for odd record lengths, records longer than a tile and fields that
//      straddle tiles: the output against a byte-by-byte statement of the rule written here, every byte written exactly once, the
//      overflow count the number of overflowing fields.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I stratanet2_vegetation_coverage_maps_amd/csrc \
//       scripts/dbf_rules_sanitize.cpp -o /tmp/dbf_rules_sanitize && /tmp/dbf_rules_sanitize
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "dbf_rules.h"

template <typename T>
static T* exact(size_t n) {
    void* p = nullptr;
    if (posix_memalign(&p, 16, (n ? n : 1) * sizeof(T)) != 0) abort();
    return (T*)p;
}

static uint64_t bits_of(double v) {
    uint64_t b;
    memcpy(&b, &v, 8);
    return b;
}
static double double_of(uint64_t b) {
    double v;
    memcpy(&v, &b, 8);
    return v;
}

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {                              // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t random_below_2_53() {                // a random bit pattern with a biased exponent below 1023 + 53
    for (;;) {
        const uint64_t b = rnd();
        if (((b >> 52) & 0x7FF) < 1023 + 53) return b;
    }
}

static std::string rule_text(uint64_t bits, int decimal) {
    char* text = exact<char>(DBF_TEXT_MAX);
    const int len = dbf_format(bits, decimal, text);
    std::string s = len < 0 ? std::string("*") : std::string(text, (size_t)len);
    free(text);
    return s;
}

static int against_printf(uint64_t bits, int decimal) {
    char want[400];
    snprintf(want, sizeof want, "%.*f", decimal, double_of(bits));
    const std::string got = rule_text(bits, decimal);
    if (got != want) {
        printf("bits %016llx decimal %d: rule '%s', printf '%s'\n", (unsigned long long)bits, decimal, got.c_str(), want);
        return 1;
    }
    return 0;
}

static const double PLANTED[] = {1.0 / 2048, 3.0 / 2048, 0x1p-34, 0x1p-35, -0x1p-35, -0.0, 0.0, 1.0 - 0x1p-53, 0.99999999995,
                                 9007199254740991.0, 4503599627370495.5, 5e-324, -5e-324, 0.5, 1.5, 2.5, -0.5, 0.125, 0.375,
                                 1e-10, 5e-11, 4.9999999999e-11, 0.00000000005, 999999.99999999995, 9.5, 10.5, 0.95, 0.05,
                                 2.2250738585072014e-308, 1.0, -1.0, 123456789.0123456789, 0x1p52, 0x1p52 + 0.5, 0x1p51 + 0.25};

struct counting_sink {
    uint8_t* out;
    uint8_t* times;
    uint64_t o0, o1;
    void byte(uint64_t o, uint32_t v) const {
        if (o < o0 || o >= o1) abort();                                 // a tile's lanes stay inside their tile
        out[o] = (uint8_t)v;
        ++times[o];
    }
};
struct host_values {
    const uint64_t* values;
    const int* row_of;
    const int* cols;
    long long R;
    int C;
    uint64_t missing;
    uint64_t operator()(uint64_t k, int f) const {
        const int row = row_of[k];
        if (row < 0 || row >= R) return missing;
        return values[(size_t)row * C + cols[f]];
    }
};

static int run_tiles(long long K, int L, int n, int size, int decimal, uint32_t lanes) {
    uint64_t record_bytes = 0, total = 0;
    if (dbf_check_shape(K, L, n, size, decimal, &record_bytes, &total) != 0) return 1;
    const dbf_shape s{K, L, n, size, decimal, L + n * size};
    const long long R = K / 2 + 1;
    const int C = n + 2;
    uint8_t* src = exact<uint8_t>((size_t)K * L);
    for (size_t i = 0; i < (size_t)K * L; ++i) src[i] = (uint8_t)rnd();
    uint64_t* values = exact<uint64_t>((size_t)R * C);
    for (size_t i = 0; i < (size_t)R * C; ++i)
        values[i] = i % 7 == 3 ? bits_of(0x1p53 * (double)(1 + i % 3)) : (i % 11 == 5 ? bits_of(NAN) : random_below_2_53());
    int* row_of = exact<int>((size_t)K);
    for (long long k = 0; k < K; ++k) row_of[k] = k % 3 == 1 ? -1 : (int)((k * 7) % R);
    int* cols = exact<int>((size_t)n);
    for (int f = 0; f < n; ++f) cols[f] = (C - 1 - f * 3 % C + C) % C;
    uint8_t* out = exact<uint8_t>(record_bytes);
    uint8_t* times = exact<uint8_t>(record_bytes);
    memset(out, 0xCD, record_bytes);
    memset(times, 0, record_bytes);
    const host_values value{values, row_of, cols, R, C, bits_of(-1.0)};
    uint64_t overflow = 0;
    for (uint64_t tile = 0; tile < dbf_tiles(record_bytes); ++tile) {
        const uint64_t o0 = tile * DBF_TILE_BYTES, o1 = record_bytes - o0 < DBF_TILE_BYTES ? record_bytes : o0 + DBF_TILE_BYTES;
        const counting_sink sink{out, times, o0, o1};
        for (uint32_t lane = 0; lane < lanes; ++lane) {
            dbf_copy_range(src, s, o0, o1, sink, lane, lanes);
            overflow += dbf_field_range(value, s, o0, o1, sink, lane, lanes);
        }
    }
    // the rule, byte by byte
    int bad = 0;
    uint64_t want_overflow = 0;
    for (long long k = 0; k < K; ++k) {
        const uint8_t* rec = out + (size_t)k * s.Ld;
        bad += memcmp(rec, src + (size_t)k * L, (size_t)L) != 0;
        for (int f = 0; f < n; ++f) {
            const uint64_t b = value((uint64_t)k, f);
            const double v = double_of(b);
            std::string field;
            if (isfinite(v) && fabs(v) >= 0x1p53) {
                field = std::string((size_t)size, '*');
                ++want_overflow;
            } else {
                char text[400];
                if (isnan(v)) snprintf(text, sizeof text, "nan");
                else snprintf(text, sizeof text, "%.*f", decimal, v);
                std::string t(text);
                if ((int)t.size() > size) t.resize((size_t)size);
                field = std::string((size_t)size - t.size(), ' ') + t;
            }
            bad += memcmp(rec + L + (size_t)f * size, field.data(), (size_t)size) != 0;
        }
    }
    for (uint64_t o = 0; o < record_bytes; ++o) bad += times[o] != 1;
    bad += overflow != want_overflow;
    free(src);
    free(values);
    free(row_of);
    free(cols);
    free(out);
    free(times);
    if (bad) printf("tiles K=%lld L=%d n=%d size=%d decimal=%d lanes=%u: %d wrong\n", K, L, n, size, decimal, lanes, bad);
    return bad;
}

int main() {
    int bad = 0;
    long cases = 0;
    for (double v : PLANTED)
        for (int d = 0; d <= DBF_MAX_DECIMAL; ++d, ++cases) bad += against_printf(bits_of(v), d);
    for (int e = 0; e < 1023 + 53; ++e)                                  // every exponent, the least and the greatest mantissa, a tie
        for (uint64_t m : {0ull, 0xFFFFFFFFFFFFFull, 0x8000000000000ull})
            for (int d : {0, 1, 10, 15}) {
                bad += against_printf(((uint64_t)e << 52) | m, d);
                bad += against_printf((1ull << 63) | ((uint64_t)e << 52) | m, d);
                cases += 2;
            }
    for (int i = 0; i < 1000000; ++i, cases += 2) {
        const uint64_t b = random_below_2_53();
        bad += against_printf(b, 10);
        bad += against_printf(b, (int)(rnd() % 16));
    }
    // k / 2^j: the values whose expansions end, ties at every place among them
    for (int i = 0; i < 200000; ++i, ++cases) {
        const double v = (double)(int64_t)(rnd() % 2000001 - 1000000) / (double)(1ull << (rnd() % 40));
        bad += against_printf(bits_of(v), (int)(rnd() % 16));
    }
    bad += rule_text(bits_of(NAN), 10) != "nan";
    bad += rule_text(bits_of(-NAN), 10) != "nan";
    bad += rule_text(bits_of(INFINITY), 10) != "inf";
    bad += rule_text(bits_of(-INFINITY), 10) != "-inf";
    bad += rule_text(bits_of(0x1p53), 10) != "*";
    bad += rule_text(bits_of(-1e300), 10) != "*";
    bad += rule_text(bits_of(-0.0), 10) != "-0.0000000000";
    bad += rule_text(bits_of(-0x1p-35), 10) != "-0.0000000000";
    cases += 8;

    const int Ls[] = {1, 2, 7, 33, 254, 4000, 16383, 16385, 40001};
    for (int L : Ls)
        for (int n : {1, 4})
            for (int sd = 0; sd < 2; ++sd) {
                const int size = sd ? 12 : 50, decimal = sd ? 3 : 10;
                for (long long K : {1ll, 3ll, 65ll, 257ll}) {
                    if ((uint64_t)K * L > (40u << 20)) continue;
                    bad += run_tiles(K, L, n, size, decimal, K % 2 ? 256 : 5);
                    ++cases;
                }
            }
    bad += run_tiles(2000, 9, 255, 2, 0, 64);                            // the most fields, the narrowest
    bad += run_tiles(3, 65535 - 254, 1, 254, 15, 7);                     // the longest record
    bad += run_tiles(40000, 1, 1, 2, 0, 256);                            // the shortest: 5462 records to a tile
    cases += 3;
    printf("%ld cases, %d wrong\n", cases, bad);
    return bad ? 1 : 0;
}
