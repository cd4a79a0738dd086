// The composition of one written LAS record (csrc/las_write_rules.h: las_compose, the function the kernels of las_write.hip run per
// lane) on the CPU, over the odd-length cases, for a run under a sanitizer.  A stand-alone program: nothing of the library is
// loaded.  Every buffer is allocated at its exact size -- the source block T L_src bytes (the staged form: rounded up to 16 and one
// slot of slack, as the kernel's LDS), the destination T L_dst bytes, the score rows T values -- so a byte read or written outside
// the rule's bounds is reported.  The result is compared with a byte-by-byte statement of the rule written here.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I stratanet2_vegetation_coverage_maps_amd/csrc \
//       scripts/las_write_sanitize.cpp -o /tmp/las_write_sanitize && /tmp/las_write_sanitize
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "las_write_rules.h"

static uint8_t* exact(size_t n) {
    void* p = nullptr;
    if (posix_memalign(&p, 16, n ? n : 1) != 0) abort();
    return (uint8_t*)p;
}

static int run_case(int format, int L_src, unsigned mask, int class_mode, int unscored, int T, bool staged, bool gather) {
    const int E = las_write_extra_bytes(mask), L_dst = L_src + E;
    const int codes_host[4] = {3, 2, 4, 5};
    las_write_rule R = {format, L_src, E, mask, class_mode, las_write_pack_codes(codes_host), unscored};
    const size_t src_bytes = (size_t)T * L_src;
    const size_t alloc = staged ? (src_bytes + 15) / 16 * 16 + 16 : src_bytes;
    uint8_t* src = exact(alloc);
    for (size_t i = 0; i < alloc; ++i) src[i] = i < src_bytes ? (uint8_t)(i * 37 + 11) : (uint8_t)0;
    uint8_t* dst = exact((size_t)T * L_dst);
    float* scores = (float*)exact(sizeof(float) * 8 * T);
    float* weight = (float*)exact(sizeof(float) * T);
    int* hits = (int*)exact(sizeof(int) * T);
    const int hit_values[6] = {0, 1, 65535, 65536, 3, -1};
    for (int c = 0; c < T; ++c) {
        for (int k = 0; k < 8; ++k) scores[k * T + c] = (float)((c * 5 + k * 3) % 7) * 0.125f;
        if (c % 4 == 1) scores[5 * T + c] = scores[4 * T + c];           // a tie
        if (c % 4 == 2) scores[6 * T + c] = NAN;
        weight[c] = -0.0f + c;
        hits[c] = hit_values[c % 6];
    }
    las_score_cols S = {scores, weight, hits, (size_t)T};
    int bad = 0;
    // the rule, byte by byte, for the whole block
    std::vector<uint8_t> want((size_t)T * L_dst, 0);
    std::vector<long> source(T);
    for (int i = 0; i < T; ++i) {
        const long s = gather ? (i == 1 ? -1 : (i == 2 ? T : (T - 1 - i))) : i;
        source[i] = s;
        if (s < 0 || s >= T) continue;
        uint8_t* r = &want[(size_t)i * L_dst];
        for (int b = 0; b < L_src; ++b) r[b] = src[(size_t)s * L_src + b];
        if (class_mode == 1) {
            int code = unscored;
            if (hits[i] > 0) {
                int best = 0;
                for (int k = 1; k < 4; ++k)
                    if (scores[(4 + k) * T + i] > scores[(4 + best) * T + i]) best = k;
                code = codes_host[best];
            }
            if (code >= 0) {
                if (format >= 6) r[16] = (uint8_t)code;
                else r[15] = (uint8_t)((r[15] & 0xE0) | code);
            }
        }
        size_t at = L_src;
        for (int k = 0; k < 9; ++k)
            if ((mask >> k) & 1u) {
                memcpy(&r[at], k < 8 ? (const void*)&scores[k * T + i] : (const void*)&weight[i], 4);
                at += 4;
            }
        if ((mask >> 9) & 1u) {
            const int h = hits[i] < 0 ? 0 : (hits[i] > 65535 ? 65535 : hits[i]);
            r[at] = (uint8_t)h;
            r[at + 1] = (uint8_t)(h >> 8);
        }
    }
    // lanes finish in any order: compose the records first to last and last to first, and compare the block when all are done, so
    // a record that writes into its neighbour's bytes shows in one of the two
    for (int order = 0; order < 2; ++order) {
        memset(dst, 0xCD, (size_t)T * L_dst);
        for (int j = 0; j < T; ++j) {
            const int i = order ? T - 1 - j : j;
            const long s = source[i];
            const bool have = s >= 0 && s < T;
            const size_t s0 = have ? (size_t)s * L_src : 0;
            las_written w;
            // the staged form composes through the word stream (as in LDS), the direct form through the byte stream
            if (staged) w = las_compose(las_staged_words{(const uint32_t*)src}, s0, have, las_word_stream{dst, 0, 0, 0}, (size_t)i * L_dst, R, las_load_scores(S, (size_t)i, R));
            else w = las_compose(las_guarded_words{src, src_bytes}, s0, have, las_byte_stream{dst, 0}, (size_t)i * L_dst, R, las_load_scores(S, (size_t)i, R));
            int32_t X = 0;
            if (have) memcpy(&X, &src[s0], 4);
            if (w.bad != !have || (have && (w.X != X || w.scored != (hits[i] > 0)))) ++bad;
        }
        for (int i = 0; i < T; ++i)
            if (memcmp(&want[(size_t)i * L_dst], dst + (size_t)i * L_dst, L_dst) != 0) ++bad;
    }
    free(src);
    free(dst);
    free(scores);
    free(weight);
    free(hits);
    return bad;
}

int main() {
    const int formats[] = {0, 1, 2, 3, 6, 7, 8, 10};
    const unsigned masks[] = {0x000, 0x001, 0x200, 0x2AA, 0x3FF};
    int cases = 0, bad = 0;
    for (int format : formats)
        for (int extra : {0, 1, 3, 5})
            for (unsigned mask : masks)
                for (int mode = 0; mode < 2; ++mode)
                    for (int unscored : {-1, 1})
                        for (int T : {1, 7})
                            for (int form = 0; form < 4; ++form) {
                                bad += run_case(format, las_min_length(format) + extra, mask, mode, unscored, T, (form & 1) != 0, (form & 2) != 0);
                                ++cases;
                            }
    printf("%d cases, %d wrong records\n", cases, bad);
    return bad ? 1 : 0;
}
