// admissibility.hip -- the admissibility band of the parcel product on the device: sieve of the hard medium-vegetation band
// (connected-component labelling, region sizes, the merge walk), erosion by 1.5 px and the band itself.  The rule is written out
// in include/strata_hip.h ("Admissibility band"); its per-pixel and per-region functions are admissibility_rules.h.
//
// The kernels are written once, over a canvas table (atlas_table.h): a workgroup finds its canvas from the table's prefix of
// SN2_ATLAS_FINALIZE_BLOCKS and takes the pixels 256 j + t, + 256 blocks, ... of that canvas.  The single-canvas entry point
// writes a one-row table into the head of its workspace first.  Seven launches on one stream, each a whole phase: no workgroup waits
// for another, nothing is read back.  Every cross-thread result is an integer minimum, maximum or sum, so the order of arrival
// changes no byte.
#include "admissibility_rules.h"
#include "atlas_table.h"
#include "common.h"
#include "mosaic_rules.h"

namespace {
constexpr int COLS = ATLAS_COLS;
constexpr int ADM_T = 256;
#define ADM_RELAXED __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// the arrays of the workspace behind its head, one entry per pixel of the arena (pixel i of canvas k at base_k + i)
struct AdmWs {
    unsigned long long* key;   // at a region's root: the largest neighbour key (0 = no neighbour)
    int* parent;               // union-find parent as a pixel index of the canvas; after the flatten the region's root = its id; -1 invalid
    int* size;                 // at a root: the region's pixel count
    int* res;                  // at a root: the sieve's output bit S for the region
    int* hp;                   // H', the sieved hard band with the outside set to one
};

AdmWs adm_carve(void* ws, size_t pixels) {
    AdmWs a;
    a.key = (unsigned long long*)((uint32_t*)ws + SN2_ADM_WS_HEAD_WORDS);
    a.parent = (int*)(a.key + pixels);
    a.size = a.parent + pixels;
    a.res = a.size + pixels;
    a.hp = a.res + pixels;
    return a;
}

// this workgroup's canvas and its share of the canvas's pixels
struct AdmCanvas {
    int k, H, W;
    long P, first, step;
    size_t base;
};
__device__ __forceinline__ AdmCanvas adm_canvas(const long long* __restrict__ canvas, int K) {
    AdmCanvas c;
    c.k = last_row_at_or_below(canvas, COLS, 3, K, (long long)blockIdx.x);
    const long long* cv = canvas + (size_t)c.k * COLS;
    c.H = (int)cv[1];
    c.W = (int)cv[2];
    c.P = (long)c.H * (long)c.W;
    c.base = (size_t)cv[0];
    c.first = ((long)blockIdx.x - (long)cv[3]) * ADM_T;
    c.step = (long)(cv[COLS + 3] - cv[3]) * ADM_T;
    return c;
}

// the sum of a per-thread count over the workgroup's waves, added to one int64 word (an integer sum: any order)
__device__ __forceinline__ void adm_count(long long* word, int n) {
    n = rules_wave_sum(n);
    if ((threadIdx.x & 63) == 0 && n != 0) atomicAdd((unsigned long long*)word, (unsigned long long)n);
}

// the one-row table of the single-canvas call: the 2 COLS words the host worked out, stored by one lane
struct AdmTable1 {
    long long v[2 * COLS];
};
__global__ void adm_table_kernel(AdmTable1 t, long long* __restrict__ dst) {
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 2 * COLS; ++c) dst[c] = t.v[c];
    }
}

// ---- 0: every pixel its own region; sizes, keys and the statistics cleared ------------------------------------------------
__global__ __launch_bounds__(ADM_T) void adm_init_kernel(const float* __restrict__ bands5, const long long* __restrict__ canvas, int K,
                                                         AdmWs ws, long long* __restrict__ stats) {
    const AdmCanvas c = adm_canvas(canvas, K);
    const float* hard = bands5 + 5 * c.base + 3 * (size_t)c.P;
    for (long i = c.first + threadIdx.x; i < c.P; i += c.step) {
        const size_t g = c.base + (size_t)i;
        ws.parent[g] = adm_valid(hard[i]) ? (int)i : -1;
        ws.size[g] = 0;
        ws.key[g] = 0ull;                                   // (res is written at every root by phase 4, hp at every pixel by phase 5)
    }
    if (c.first == 0 && threadIdx.x < 4) stats[4 * (size_t)c.k + threadIdx.x] = 0;
}

// ---- 1: labelling.  Union-find in global memory; a root is the smallest pixel index of its tree, and a parent only ever moves
// to a smaller index of the same region, so a stale read is still an ancestor and every loop strictly descends.
__device__ __forceinline__ int adm_find(int* par, int x) {
    int p;
    while ((p = __hip_atomic_load(par + x, ADM_RELAXED)) != x) x = p;
    return x;
}
// atomicMin retries against the value it finds, never against a peer's progress: when the root moved under us (old != a) we
// go on uniting its new parent with b, so the link is made by this thread whatever the others do
__device__ __forceinline__ void adm_unite(int* par, int a, int b) {
    for (;;) {
        a = adm_find(par, a);
        b = adm_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(par + a, b);
        if (old == a) return;
        a = old;
    }
}

__global__ __launch_bounds__(ADM_T) void adm_union_kernel(const float* __restrict__ bands5, const long long* __restrict__ canvas, int K,
                                                          AdmWs ws) {
    const AdmCanvas c = adm_canvas(canvas, K);
    const float* hard = bands5 + 5 * c.base + 3 * (size_t)c.P;
    int* par = ws.parent + c.base;
    for (long i = c.first + threadIdx.x; i < c.P; i += c.step) {
        const float v = hard[i];
        if (!adm_valid(v)) continue;
        const int h = adm_hard_bit(v);
        const int row = (int)(i / c.W), col = (int)(i - (long)row * c.W);
        if (col > 0) {
            const float q = hard[i - 1];
            if (adm_valid(q) && adm_hard_bit(q) == h) adm_unite(par, (int)i, (int)i - 1);
        }
        if (row > 0) {
            const float q = hard[i - c.W];
            if (adm_valid(q) && adm_hard_bit(q) == h) adm_unite(par, (int)i, (int)(i - c.W));
        }
    }
}

// ---- 2: flatten (parent = root = the region's id) and region sizes.  The lanes of a wave that share a root add once.
__global__ __launch_bounds__(ADM_T) void adm_size_kernel(const long long* __restrict__ canvas, int K, AdmWs ws) {
    const AdmCanvas c = adm_canvas(canvas, K);
    int* par = ws.parent + c.base;
    int* size = ws.size + c.base;
    const int lane = threadIdx.x & 63;
    for (long i0 = c.first; i0 < c.P; i0 += c.step) {                  // uniform over the workgroup
        const long i = i0 + threadIdx.x;
        bool todo = i < c.P && __hip_atomic_load(par + (i < c.P ? i : 0), ADM_RELAXED) >= 0;
        int root = -1;
        if (todo) {
            root = adm_find(par, (int)i);
            __hip_atomic_store(par + i, root, ADM_RELAXED);            // a root, hence an ancestor, for whoever reads it meanwhile
        }
        for (;;) {
            const unsigned long long open = __ballot(todo);
            if (open == 0ull) break;
            const int lead = __ffsll((long long)open) - 1;
            const int r0 = __shfl(root, lead);
            const bool mine = todo && root == r0;
            const unsigned long long same = __ballot(mine);
            if (lane == lead) atomicAdd(size + r0, (int)__popcll(same));
            if (mine) todo = false;
        }
    }
}

// ---- 3: big of each small region: the largest neighbour key over all its adjacencies, one 64-bit atomicMax per pixel that has one
__global__ __launch_bounds__(ADM_T) void adm_big_kernel(const float* __restrict__ bands5, const long long* __restrict__ canvas, int K,
                                                        int sieve_size, AdmWs ws) {
    const AdmCanvas c = adm_canvas(canvas, K);
    const float* hard = bands5 + 5 * c.base + 3 * (size_t)c.P;
    const int* par = ws.parent + c.base;
    const int* size = ws.size + c.base;
    unsigned long long* key = ws.key + c.base;
    for (long i = c.first + threadIdx.x; i < c.P; i += c.step) {
        const int rp = par[i];
        if (rp < 0 || !adm_small(size[rp], sieve_size)) continue;
        const int h = adm_hard_bit(hard[i]);
        const int row = (int)(i / c.W), col = (int)(i - (long)row * c.W);
        unsigned long long best = 0ull;
        const long nb[4] = {col > 0 ? i - 1 : -1, col + 1 < c.W ? i + 1 : -1, row > 0 ? i - c.W : -1, row + 1 < c.H ? i + c.W : -1};
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            if (nb[n] < 0) continue;
            const int rq = par[nb[n]];
            if (rq < 0 || adm_hard_bit(hard[nb[n]]) == h) continue;       // invalid: nobody's neighbour; equal bit: the same region
            const unsigned long long k = adm_neighbour_key(size[rq], rq);
            best = k > best ? k : best;
        }
        if (best != 0ull) atomicMax(key + rp, best);
    }
}

// ---- 4: the walk of each small region, one thread per root.  Brent's repeat detection: `mark` is moved to the current region
// after 1, 2, 4, ... steps, and a walk that comes back to it has met a region twice -- it terminates on any table of keys.  (On
// the keys of phase 3 only two-region cycles exist: R is a neighbour of big(R), so the key of big(big(R)) is at least R's, and
// equal only if it is R.)  A walk that stays among small regions for ever and one that meets a region twice are the same walks.
__global__ __launch_bounds__(ADM_T) void adm_walk_kernel(const float* __restrict__ bands5, const long long* __restrict__ canvas, int K,
                                                         int sieve_size, AdmWs ws, long long* __restrict__ stats) {
    const AdmCanvas c = adm_canvas(canvas, K);
    const float* hard = bands5 + 5 * c.base + 3 * (size_t)c.P;
    const int* par = ws.parent + c.base;
    const int* size = ws.size + c.base;
    const unsigned long long* key = ws.key + c.base;
    int* res = ws.res + c.base;
    int regions = 0, small = 0;
    for (long i = c.first + threadIdx.x; i < c.P; i += c.step) {
        if (par[i] != (int)i) continue;                                   // not a root (or invalid)
        ++regions;
        int target = (int)i;
        if (adm_small(size[i], sieve_size)) {
            ++small;
            unsigned cur = (unsigned)i, mark = (unsigned)i, lap = 1, n = 0;
            for (;;) {
                const unsigned long long k = key[cur];
                if (k == 0ull) break;                                     // no neighbour: no big
                const unsigned nxt = adm_key_id(k);
                if ((long)nxt >= c.P) break;                              // (cannot happen on the keys of phase 3)
                if (!adm_small(size[nxt], sieve_size)) { target = (int)nxt; break; }
                if (nxt == mark) break;                                   // a region came up a second time
                if (++n == lap) { mark = nxt; lap <<= 1; n = 0; }
                cur = nxt;
            }
        }
        res[i] = adm_hard_bit(hard[target]);
    }
    adm_count(stats + 4 * (size_t)c.k + 0, regions);
    adm_count(stats + 4 * (size_t)c.k + 1, small);
}

// ---- 5: H' of every pixel
__global__ __launch_bounds__(ADM_T) void adm_sieved_kernel(const float* __restrict__ bands5, const long long* __restrict__ canvas, int K,
                                                           AdmWs ws, long long* __restrict__ stats) {
    const AdmCanvas c = adm_canvas(canvas, K);
    const float* hard = bands5 + 5 * c.base + 3 * (size_t)c.P;
    int changed = 0;
    for (long i = c.first + threadIdx.x; i < c.P; i += c.step) {
        const size_t g = c.base + (size_t)i;
        const int root = ws.parent[g];
        const bool valid = root >= 0;
        int h = 0, S = 0;
        if (valid) {
            h = adm_hard_bit(hard[i]);
            S = ws.res[c.base + (size_t)root];
            changed += S != h;
        }
        ws.hp[g] = adm_sieved_bit(valid, h, S);
    }
    adm_count(stats + 4 * (size_t)c.k + 2, changed);
}

// ---- 6: the offsets test and the six bands
__global__ __launch_bounds__(ADM_T) void adm_band_kernel(const float* __restrict__ bands5, const long long* __restrict__ canvas, int K,
                                                         AdmWs ws, float* __restrict__ bands6, long long* __restrict__ stats) {
    const AdmCanvas c = adm_canvas(canvas, K);
    const size_t P = (size_t)c.P;
    const float* in = bands5 + 5 * c.base;
    float* out = bands6 + 6 * c.base;
    const int* hp = ws.hp + c.base;
    int n_inacc = 0;
    for (long i = c.first + threadIdx.x; i < c.P; i += c.step) {
        const int row = (int)(i / c.W), col = (int)(i - (long)row * c.W);
        bool inacc = true;
#pragma unroll
        for (int dy = -ADM_REACH; dy <= ADM_REACH; ++dy)
#pragma unroll
            for (int dx = -ADM_REACH; dx <= ADM_REACH; ++dx) {
                if (!adm_offset_tested(dx, dy)) continue;
                const int r = row + dy, q = col + dx;
                const int v = (r >= 0 && r < c.H && q >= 0 && q < c.W) ? hp[(long)r * c.W + q] : 0;   // outside the canvas: 0
                inacc = inacc && v == 1;
            }
        const float vb = in[i], vms = in[P + i], vh = in[2 * P + i], hard = in[3 * P + i], wt = in[4 * P + i];
        const bool valid = adm_valid(hard);
        n_inacc += valid && inacc;
        out[i] = vb;
        out[P + i] = vms;
        out[2 * P + i] = vh;
        out[3 * P + i] = hard;
        out[4 * P + i] = adm_band(valid, inacc, vb, vms);
        out[5 * P + i] = wt;
    }
    adm_count(stats + 4 * (size_t)c.k + 3, n_inacc);
}

int adm_run(const float* bands5, int K, const long long* canvas_dev, unsigned grid, size_t pixels, int sieve_size, void* ws_base,
            float* bands6, long long* stats, hipStream_t st) {
    const AdmWs ws = adm_carve(ws_base, pixels);
    const dim3 g(grid), b(ADM_T);
    hipLaunchKernelGGL(adm_init_kernel, g, b, 0, st, bands5, canvas_dev, K, ws, stats);
    hipLaunchKernelGGL(adm_union_kernel, g, b, 0, st, bands5, canvas_dev, K, ws);
    hipLaunchKernelGGL(adm_size_kernel, g, b, 0, st, canvas_dev, K, ws);
    hipLaunchKernelGGL(adm_big_kernel, g, b, 0, st, bands5, canvas_dev, K, sieve_size, ws);
    hipLaunchKernelGGL(adm_walk_kernel, g, b, 0, st, bands5, canvas_dev, K, sieve_size, ws, stats);
    hipLaunchKernelGGL(adm_sieved_kernel, g, b, 0, st, bands5, canvas_dev, K, ws, stats);
    hipLaunchKernelGGL(adm_band_kernel, g, b, 0, st, bands5, canvas_dev, K, ws, bands6, stats);
    SN2_RETURN_LAUNCH();
}
}  // namespace

extern "C" int sn2_admissibility_ws_words(long long pixels, size_t* words) {
    if (!words || pixels <= 0) return SN2_EINVAL;
    *words = SN2_ADM_WS_WORDS(pixels);
    return 0;
}

extern "C" int sn2_mosaic_admissibility(const float* bands5, int H, int W, int sieve_size, void* ws, float* bands6, long long* stats,
                                        void* stream) {
    if (!bands5 || !ws || !bands6 || !stats || H <= 0 || W <= 0 || sieve_size < 0) return SN2_EINVAL;
    if (((uintptr_t)ws & 7) != 0) return SN2_EINVAL;
    AdmTable1 t;
    std::memset(&t, 0, sizeof(t));
    long long row[2 * COLS] = {0};
    SN2_TRY(atlas_canvas_row(H, W, 0.0, 0.0, t.v, row));                    // SN2_ELIMIT on H W >= 2^31
    std::memcpy(t.v, row, sizeof(long long) * COLS);
    t.v[COLS + 0] = row[COLS + 0];
    t.v[COLS + 3] = row[COLS + 3];
    t.v[COLS + 4] = row[COLS + 4];
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(adm_table_kernel, dim3(1), dim3(64), 0, st, t, (long long*)ws);
    return adm_run(bands5, 1, (const long long*)ws, (unsigned)t.v[COLS + 3], (size_t)t.v[COLS + 0], sieve_size, ws, bands6, stats, st);
}

extern "C" int sn2_atlas_admissibility(const float* bands5_arena, int K, const long long* canvas_host, const long long* canvas_dev,
                                       int sieve_size, void* ws, float* bands6_arena, long long* stats, void* stream) {
    if (!bands5_arena || !canvas_host || !canvas_dev || !ws || !bands6_arena || !stats || K <= 0 || sieve_size < 0) return SN2_EINVAL;
    if (((uintptr_t)ws & 7) != 0) return SN2_EINVAL;
    SN2_TRY(atlas_check_table(K, canvas_host));
    const long long* last = canvas_host + (size_t)K * COLS;
    return adm_run(bands5_arena, K, canvas_dev, (unsigned)last[3], (size_t)last[0], sieve_size, ws, bands6_arena, stats,
                   (hipStream_t)stream);
}
