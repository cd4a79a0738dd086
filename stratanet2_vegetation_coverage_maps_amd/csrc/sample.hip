// sample.hip -- the point subsample of every plot of a batch, drawn on the device: the distribution of the reference's
// `sample_cloud` (data_loader/loader.py:233-247: choice(n, N, replace=False) for n > N, else arange(n) followed by N - n draws
// with replacement), from a counter-based generator instead of numpy's sequential Mersenne-Twister stream.  Host side:
// hip_ops.subsample, input_pipeline.prepare_batch(sampler="device"), parcel.ParcelPlots.batches(sampler="device").
//
// Contract (include/strata_hip.h, sn2_subsample): u(seed, key, i) = Philox4x32-10 word pair; a plot with n > N candidates
// keeps the N candidates with the smallest pairs (u, i), listed in ascending order of the pair.  A row depends on
// (seed, key, n, N) alone: integer arithmetic only, and the only atomics are integer counters whose totals -- never their
// arrival order -- reach the output.
//
// How a row with n > N is built (both forms): the keys are uniform, so their leading H bits deal the candidates into
// NB = 2^H buckets of about four.  (1) histogram of the buckets; (2) exclusive scan: a bucket's start is the rank of its
// smallest member, and the bucket t that holds rank N - 1 is the last one that matters; (3) the candidates of buckets <= t
// are scattered into their bucket's slots as 8-byte pairs (the 32 key bits below the bucket bits, index) -- the slot inside
// a bucket comes from an atomic cursor and is arbitrary; (4) one thread per bucket gives every member its rank = bucket
// start + members below it (a handful of compares; equal 32-bit pieces are settled by recomputing both full keys) and
// writes idx[rank] = index for rank < N.  Selection and ordering are the same step, and nothing of it depends on NB.
//   form 1 (LDS):    one workgroup per plot, histogram and pairs in LDS (8 n + 4 NB bytes, n <= SN2_SUBSAMPLE_LDS_MAX);
//                    the generator runs twice per candidate (histogram, scatter) rather than keeping 64-bit keys in LDS.
//   form 2 (global): the same four steps as four launches over a workspace, any n; many workgroups per plot, no waiting
//                    of one workgroup on another.
#include "common.h"
#include "philox.h"
#include "plot_sort.h"

namespace {

constexpr int LDS_MAX_N = SN2_SUBSAMPLE_LDS_MAX;
constexpr int LDS_MAX_BUCKETS = 4096;
constexpr int GLOBAL_MAX_BUCKETS = 1 << 22;
constexpr int ITEMS = 4;                 // form 2 starts one thread per ITEMS candidates (grid-stride loops, at most 256 x B workgroups)

__host__ __device__ __forceinline__ int ceil_log2(long v) {
    int h = 0;
    while ((1L << h) < v) ++h;
    return h;
}
// bucket bits for plots of at most n_max candidates: about four candidates per bucket
inline int bucket_bits(int n_max, int lo, int hi) {
    const int h = ceil_log2(((long)n_max + 3) / 4);
    const int hl = ceil_log2(lo), hh = ceil_log2(hi);
    return h < hl ? hl : (h > hh ? hh : h);
}

// u(seed, key, i): philox.h (counter (i, 0, key.lo, key.hi), key (seed.lo, seed.hi); u = word0 << 32 | word1)
__device__ __forceinline__ unsigned long long philox_u(unsigned long long seed, long long key, unsigned i) {
    return sn2_philox_u(seed, key, i);
}

// first word of the pairs in form 2's workspace (8-byte aligned)
__host__ __device__ __forceinline__ size_t pairs_base(int B, int H) { return ((((size_t)B << H) + (size_t)B) + 3) & ~(size_t)3; }

struct Pair {
    unsigned mid;     // the 32 key bits below the bucket bits (coarsened by mid_mask in the test forms)
    int i;
};

// (u_a, a) < (u_b, b) for two members of one bucket
__device__ __forceinline__ bool pair_less(Pair a, Pair b, unsigned long long seed, long long key) {
    if (a.mid != b.mid) return a.mid < b.mid;
    const unsigned long long ua = philox_u(seed, key, (unsigned)a.i), ub = philox_u(seed, key, (unsigned)b.i);
    return ua != ub ? ua < ub : a.i < b.i;
}

// ids (sn2_train_batch: the plots of a batch gathered from a resident set) or NULL: plot b is entry ids[b] / b of `offs`
__device__ __forceinline__ int plot_candidates(const int* __restrict__ offs, const int* __restrict__ ids, int b, int extra,
                                               int n_max) {
    const int p = ids ? ids[b] : b;
    const long n = (long)offs[p + 1] - offs[p] + extra;
    return n > n_max ? n_max : (n < 0 ? 0 : (int)n);
}

// a row with n <= N candidates: 0 .. n-1, then draws with replacement floor(u(n + j) n / 2^64); n == 0: zeros
__device__ __forceinline__ void small_row(int* __restrict__ row, int n, int N, unsigned long long seed, long long key, int first,
                                          int step) {
    for (int j = first; j < N; j += step)
        row[j] = j < n ? j : (n > 0 ? (int)__umul64hi(philox_u(seed, key, (unsigned)j), (unsigned long long)n) : 0);
}

// the ranks of bucket `bk`'s members (pairs[lo, hi)) -> idx
__device__ __forceinline__ void rank_bucket(const Pair* pairs, int lo, int hi, int N, unsigned long long seed, long long key,
                                            int* __restrict__ row) {
    for (int e = lo; e < hi; ++e) {
        const Pair me = pairs[e];
        int r = lo;
        for (int o = lo; o < hi; ++o)
            if (o != e && pair_less(pairs[o], me, seed, key)) ++r;
        if (r < N) row[r] = me.i;
    }
}

// exclusive scan in place of h[0, nb) by one workgroup (blockDim.x a multiple of 64, at most 1024); *t_out = the bucket that
// holds rank N - 1 (the counts sum to more than N - 1).  s_wave: 16 ints of LDS.
__device__ __forceinline__ void scan_buckets(int* h, int nb, int N, int* s_wave, int* t_out) {
    const int tid = threadIdx.x, nt = blockDim.x, per = (nb + nt - 1) / nt;
    const int c0 = tid * per, c1 = min(nb, c0 + per);
    if (tid == 0) *t_out = nb - 1;                         // never read as such: some bucket below holds rank N - 1
    int sum = 0;
    for (int c = c0; c < c1; ++c) sum += h[c];
    int run = block_scan_excl<1024>(sum, s_wave);
    for (int c = c0; c < c1; ++c) {
        const int v = h[c];
        h[c] = run;
        if (run <= N - 1 && N - 1 < run + v) *t_out = c;
        run += v;
    }
    __syncthreads();
}

// ---- form 1 -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void subsample_lds_kernel(const int* __restrict__ offs, const int* __restrict__ ids, int extra,
                                                             int n_max, int N, unsigned long long seed,
                                                             const long long* __restrict__ keys, int H, unsigned mid_mask,
                                                             int* __restrict__ idx) {
    extern __shared__ __attribute__((aligned(16))) int s_mem[];    // [NB] bucket starts / cursors | [n_max] pairs | scan scratch
    const int NB = 1 << H, b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    int* s_hist = s_mem;
    Pair* s_pairs = (Pair*)(s_mem + NB);
    int* s_wave = s_mem + NB + 2 * n_max;                          // 16 wave totals + the last bucket
    const int n = plot_candidates(offs, ids, b, extra, n_max);
    const long long key = keys[b];
    int* row = idx + (size_t)b * N;
    if (n <= N) {
        small_row(row, n, N, seed, key, tid, nt);
        return;
    }
    for (int c = tid; c < NB; c += nt) s_hist[c] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += nt) atomicAdd(&s_hist[philox_u(seed, key, (unsigned)i) >> (64 - H)], 1);
    __syncthreads();
    scan_buckets(s_hist, NB, N, s_wave, s_wave + 16);
    const int t = s_wave[16];
    for (int i = tid; i < n; i += nt) {
        const unsigned long long u = philox_u(seed, key, (unsigned)i);
        const int bk = (int)(u >> (64 - H));
        if (bk <= t) {
            const int slot = atomicAdd(&s_hist[bk], 1);            // afterwards s_hist[bk] = the END of bucket bk
            s_pairs[slot] = Pair{(unsigned)(u >> (32 - H)) & mid_mask, i};
        }
    }
    __syncthreads();
    for (int bk = tid; bk <= t; bk += nt) rank_bucket(s_pairs, bk ? s_hist[bk - 1] : 0, s_hist[bk], N, seed, key, row);
}

// ---- form 2: workspace = [B][NB] bucket starts / cursors | [B] last bucket of a plot (-1: n <= N) | [B][n_max] pairs ----
__global__ __launch_bounds__(256) void subsample_hist_kernel(const int* __restrict__ offs, const int* __restrict__ ids, int extra,
                                                             int n_max, int N, int B,
                                                             unsigned long long seed, const long long* __restrict__ keys,
                                                             int H, int* __restrict__ ws) {
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const int n = plot_candidates(offs, ids, b, extra, n_max);
        if (n <= N) continue;
        int* hist = ws + ((size_t)b << H);
        const long long key = keys[b];
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
            atomicAdd(&hist[philox_u(seed, key, (unsigned)i) >> (64 - H)], 1);
    }
}

__global__ __launch_bounds__(1024) void subsample_scan_kernel(const int* __restrict__ offs, const int* __restrict__ ids, int extra,
                                                              int n_max, int N, int B,
                                                              int H, int* __restrict__ ws) {
    __shared__ int s_wave[17];
    const int b = blockIdx.x;
    int* last = ws + ((size_t)B << H) + b;
    if (plot_candidates(offs, ids, b, extra, n_max) <= N) {
        if (threadIdx.x == 0) *last = -1;
        return;
    }
    scan_buckets(ws + ((size_t)b << H), 1 << H, N, s_wave, s_wave + 16);
    if (threadIdx.x == 0) *last = s_wave[16];
}

__global__ __launch_bounds__(256) void subsample_scatter_kernel(const int* __restrict__ offs, const int* __restrict__ ids, int extra,
                                                                int n_max, int B,
                                                                unsigned long long seed, const long long* __restrict__ keys,
                                                                int H, unsigned mid_mask, int* __restrict__ ws) {
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const int t = ws[((size_t)B << H) + b];
        if (t < 0) continue;
        const int n = plot_candidates(offs, ids, b, extra, n_max);
        int* hist = ws + ((size_t)b << H);
        Pair* pairs = (Pair*)(ws + pairs_base(B, H)) + (size_t)b * n_max;
        const long long key = keys[b];
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
            const unsigned long long u = philox_u(seed, key, (unsigned)i);
            const int bk = (int)(u >> (64 - H));
            if (bk <= t) {
                const int slot = atomicAdd(&hist[bk], 1);          // slot < the candidates of buckets <= t <= n <= n_max
                pairs[slot] = Pair{(unsigned)(u >> (32 - H)) & mid_mask, (int)i};
            }
        }
    }
}

__global__ __launch_bounds__(256) void subsample_rank_kernel(const int* __restrict__ offs, const int* __restrict__ ids, int extra,
                                                             int n_max, int N, int B,
                                                             unsigned long long seed, const long long* __restrict__ keys,
                                                             int H, const int* __restrict__ ws, int* __restrict__ idx) {
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const int t = ws[((size_t)B << H) + b];
        const long long key = keys[b];
        int* row = idx + (size_t)b * N;
        const int first = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
        if (t < 0) {
            small_row(row, plot_candidates(offs, ids, b, extra, n_max), N, seed, key, first, step);
            continue;
        }
        const int* hist = ws + ((size_t)b << H);
        const Pair* pairs = (const Pair*)(ws + pairs_base(B, H)) + (size_t)b * n_max;
        for (int bk = first; bk <= t; bk += step) rank_bucket(pairs, bk ? hist[bk - 1] : 0, hist[bk], N, seed, key, row);
    }
}

}  // namespace

extern "C" int sn2_subsample_form(int n_max, int N) {
    (void)N;
    return n_max <= LDS_MAX_N ? SN2_SUBSAMPLE_LDS : SN2_SUBSAMPLE_GLOBAL;
}

extern "C" size_t sn2_subsample_ws_words(int B, int n_max, int N, int form) {
    if (B <= 0 || n_max <= 0 || N <= 0) return 0;
    if ((form & 3) == 0) form = sn2_subsample_form(n_max, N);
    if ((form & 3) != SN2_SUBSAMPLE_GLOBAL) return 0;
    return pairs_base(B, bucket_bits(n_max, 1024, GLOBAL_MAX_BUCKETS)) + 2 * (size_t)B * (size_t)n_max;
}

// sn2_subsample with an optional id table on the device (common.h): plot b of the batch is plot ids[b] of `offsets`
int sn2_subsample_ids(const int* offsets, const int* ids, int extra, int n_max, int B, int N, unsigned long long seed,
                      const long long* plot_keys, int form, int* ws, size_t ws_words, int* idx, hipStream_t stream) {
    if (!offsets || !plot_keys || !idx || B <= 0 || N <= 0 || extra < 0 || n_max <= 0) return SN2_EINVAL;
    if (form < 0 || form > 7 || (form & 3) == 3) return SN2_EINVAL;
    const unsigned mid_mask = (form & SN2_SUBSAMPLE_COARSE) ? 0xC0000000u : 0xFFFFFFFFu;
    int f = form & 3;
    if (f == 0) f = sn2_subsample_form(n_max, N);
    hipStream_t st = stream;
    if (f == SN2_SUBSAMPLE_LDS) {
        if (n_max > LDS_MAX_N) return SN2_ELIMIT;
        const int H = bucket_bits(n_max, 256, LDS_MAX_BUCKETS);
        const size_t lds = n_max <= N ? 0 : 4 * (((size_t)1 << H) + 2 * (size_t)n_max + 20);
        if (lds > 48 * 1024)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(subsample_lds_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        // few plots: sixteen waves per plot are the shortest pass; many: workgroups that find room beside other kernels
        const int threads = sn2_small_sort_wg(B) ? 512 : 1024;
        hipLaunchKernelGGL(subsample_lds_kernel, dim3(B), dim3(threads), lds, st, offsets, ids, extra, n_max, N, seed, plot_keys, H,
                           mid_mask, idx);
        SN2_RETURN_LAUNCH();
    }
    if (!ws || ((uintptr_t)ws & 15) || ws_words < sn2_subsample_ws_words(B, n_max, N, SN2_SUBSAMPLE_GLOBAL)) return SN2_EINVAL;
    const int H = bucket_bits(n_max, 1024, GLOBAL_MAX_BUCKETS);
    const int gy = B < 32768 ? B : 32768;
    const int gx = sn2_cdiv(n_max, 256 * ITEMS) < 256 ? sn2_cdiv(n_max, 256 * ITEMS) : 256;
    const long nb = 1L << H;
    const int gr = sn2_cdiv(nb > N ? nb : N, 256 * ITEMS) < 256 ? sn2_cdiv(nb > N ? nb : N, 256 * ITEMS) : 256;
    if (n_max > N) {
        sn2_fill_words(ws, 0u, (size_t)B << H, st);
        hipLaunchKernelGGL(subsample_hist_kernel, dim3(gx, gy), dim3(256), 0, st, offsets, ids, extra, n_max, N, B, seed, plot_keys,
                           H, ws);
    }
    hipLaunchKernelGGL(subsample_scan_kernel, dim3(B), dim3(1024), 0, st, offsets, ids, extra, n_max, N, B, H, ws);
    if (n_max > N)
        hipLaunchKernelGGL(subsample_scatter_kernel, dim3(gx, gy), dim3(256), 0, st, offsets, ids, extra, n_max, B, seed, plot_keys,
                           H, mid_mask, ws);
    hipLaunchKernelGGL(subsample_rank_kernel, dim3(gr, gy), dim3(256), 0, st, offsets, ids, extra, n_max, N, B, seed, plot_keys, H,
                       ws, idx);
    SN2_RETURN_LAUNCH();
}

extern "C" int sn2_subsample(const int* offsets, int extra, int n_max, int B, int N, unsigned long long seed,
                             const long long* plot_keys, int form, int* ws, size_t ws_words, int* idx, void* stream) {
    return sn2_subsample_ids(offsets, nullptr, extra, n_max, B, N, seed, plot_keys, form, ws, ws_words, idx, (hipStream_t)stream);
}
