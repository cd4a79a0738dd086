// The host-only parcel table builder and the table checks of csrc/parcels.hip under AddressSanitizer and UBSan, over the cases of
// tests/test_parcels_batched_host.py.  Every call either is host arithmetic or fails a check before any launch: no device needed.
//
//   C=stratanet2_vegetation_coverage_maps_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         $C/parcels.hip scripts/micro/parcels_table_asan.cpp -fsanitize=address,undefined -o build/parcels_table_asan && build/parcels_table_asan
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/strata_hip.h"

static int fails = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++fails;                                                  \
        }                                                             \
    } while (0)

struct Set {
    std::vector<long long> T;
    std::vector<int> P, GX, GY;
    std::vector<double> grid;
    std::vector<float> boxes;
    int K() const { return (int)T.size(); }
};

static Set a_set(int K, unsigned empty_mask) {
    Set s;
    for (int k = 0; k < K; ++k) {
        const bool empty = (empty_mask >> k) & 1;
        s.T.push_back(1 + 70001LL * (k + 1));
        s.P.push_back(empty ? 0 : 20 + 7 * k);
        s.GX.push_back(empty ? 0 : 6 + k);
        s.GY.push_back(empty ? 0 : 5 + k);
        const double g[3] = {650000.0 + 1000 * k - 7.0, 6860000.0 - 7.0, empty ? 0.0 : 1.0 / 10.01};
        s.grid.insert(s.grid.end(), g, g + 3);
        const float b[4] = {650000.f + 1000 * k, 6860000.f, 650060.f + 1000 * k + 3 * k, 6860050.f + 5 * k};
        s.boxes.insert(s.boxes.end(), b, b + 4);
    }
    return s;
}

static int build(const Set& s, std::vector<long long>& t, int K = -1, float radius = 10.f, float zr = 1.5f) {
    K = K < 0 ? s.K() : K;
    t.assign((size_t)(K > 0 ? K + 1 : 1) * SN2_PARCELS_COLS, -1);
    int L = 0;
    size_t cw = 0, zw = 0;
    return sn2_parcels_table(K, s.T.data(), s.P.data(), s.GX.data(), s.GY.data(), s.grid.data(), s.boxes.data(), radius, zr, t.data(), &L,
                             &cw, &zw);
}

int main() {
    void* fake = (void*)0x1000;                        // never dereferenced: every call below fails a check first
    std::vector<long long> t;
    for (int K : {1, 4, 5}) {
        for (unsigned mask : {0u, 0x15u, 0x1fu}) {
            Set s = a_set(K, mask);
            EXPECT(build(s, t) == 0);
            const long long* last = t.data() + (size_t)K * SN2_PARCELS_COLS;
            long long T_all = 0, P_all = 0;
            for (int k = 0; k < K; ++k) T_all += s.T[k], P_all += s.P[k];
            EXPECT(last[0] == T_all && last[3] == P_all && last[4] == K && last[1] == 2048);
            // the checked entry points take the table and stop at the next check (no centre: EINVAL; else the short workspace)
            EXPECT(sn2_parcels_count((const float*)fake, K, t.data(), (const long long*)fake, (const float*)fake, (const int*)fake,
                                     (const int*)fake, 10.f, (int*)fake, 0, (int*)fake, (long long*)fake, (long long*)fake, nullptr) ==
                   SN2_EINVAL);
            EXPECT(sn2_parcels_znorm((const float*)fake, K, t.data(), (const long long*)fake, 1.5f, 10.f, (const int*)fake,
                                     (const float*)fake, (const int*)fake, 3, (const int*)fake, 100, (int*)fake, 0, (float*)fake,
                                     nullptr) == SN2_EINVAL);
            for (int r = 0; r <= K; ++r)
                for (int c = 0; c < SN2_PARCELS_COLS; ++c) {                       // a changed layout word: refused, nothing launched
                    if (r < K && ((c >= 9 && c <= 11) || c == 13 || c == 14)) continue;   // (another grid origin or box is another table)
                    std::vector<long long> bad = t;
                    bad[(size_t)r * SN2_PARCELS_COLS + c] += 1;
                    const int rc = sn2_parcels_fill((const float*)fake, K, bad.data(), (const long long*)fake, (const float*)fake,
                                                    (const int*)fake, (const int*)fake, 10.f, (int*)fake, (const int*)fake, 100,
                                                    (float*)fake, (int*)fake, nullptr);
                    EXPECT(rc == SN2_EINVAL || rc == SN2_ELIMIT);
                }
        }
    }
    Set s = a_set(3, 0);
    EXPECT(build(s, t, 0) == SN2_EINVAL && build(s, t, 3, 0.f) == SN2_EINVAL && build(s, t, 3, 10.f, NAN) == SN2_EINVAL);
    { Set b = s; b.T[1] = 0; EXPECT(build(b, t) == SN2_EINVAL); }
    { Set b = s; b.P[1] = -1; EXPECT(build(b, t) == SN2_EINVAL); }
    { Set b = s; b.GX[1] = 0; EXPECT(build(b, t) == SN2_EINVAL); }
    { Set b = s; b.grid[5] = 1.0 / 9.99; EXPECT(build(b, t) == SN2_EINVAL); }
    { Set b = s; b.boxes[10] = INFINITY; EXPECT(build(b, t) == SN2_EINVAL); }
    { Set b = s; b.boxes[10] = b.boxes[8] - 1.f; EXPECT(build(b, t) == SN2_EINVAL); }
    { Set b = s; b.T[0] = b.T[1] = 1LL << 30; EXPECT(build(b, t) == SN2_ELIMIT); }
    { Set b = s; b.P[0] = b.P[1] = 1 << 30; EXPECT(build(b, t) == SN2_ELIMIT); }
    { Set b = s; b.T = {64, 64, 64}; b.P = {1 << 27, 1 << 27, 1 << 27}; EXPECT(build(b, t) == SN2_ELIMIT); }
    { Set b = s; b.T = {1LL << 29, 1LL << 29, 1LL << 29}; b.P = {1 << 28, 1 << 28, 1 << 28}; EXPECT(build(b, t) == SN2_ELIMIT); }
    { Set b = s; b.GX[0] = b.GY[0] = 1 << 14; EXPECT(build(b, t) == SN2_ELIMIT); }
    { Set b = s; b.boxes[2] = b.boxes[0] + 13000.f; b.boxes[3] = b.boxes[1] + 13000.f; EXPECT(build(b, t) == SN2_ELIMIT); }
    {
        Set b = s;
        for (int k = 0; k < 3; ++k) b.boxes[4 * k + 2] = b.boxes[4 * k] + 8000.f, b.boxes[4 * k + 3] = b.boxes[4 * k + 1] + 8000.f;
        EXPECT(build(b, t) == SN2_ELIMIT);
    }
    { Set b = s; b.T = {1LL << 30, 1LL << 29, 5}; b.P = {300, 100, 1}; EXPECT(build(b, t) == 0 && t[3 * SN2_PARCELS_COLS + 1] == 5632); }
    // the bounding boxes' starts
    long long starts[2][5] = {{0, 5, 4101, 8198, 8199}, {0, 1, 2, 4, 5}};
    EXPECT(sn2_parcels_bbox((const float*)fake, 8199, 4, &starts[0][0], nullptr, (unsigned*)fake, nullptr) == SN2_EINVAL);
    starts[0][2] = 5;
    EXPECT(sn2_parcels_bbox((const float*)fake, 8199, 4, &starts[0][0], (const long long*)fake, (unsigned*)fake, nullptr) == SN2_EINVAL);
    starts[0][2] = 4101, starts[1][3] = 3;
    EXPECT(sn2_parcels_bbox((const float*)fake, 8199, 4, &starts[0][0], (const long long*)fake, (unsigned*)fake, nullptr) == SN2_EINVAL);
    printf(fails ? "parcels_table_asan: %d FAILED\n" : "parcels_table_asan: all checks passed\n", fails);
    return fails != 0;
}
