// mosaic_rules.h -- the per-pixel rules of the parcel mosaic, stated once: the ordered fold of the merge, the threshold bins and
// search and the NaN rule of the finalisation, the row-segment walk and the summation trees of the crop.  The single-canvas
// kernels (project.hip) and the atlas kernels (atlas.hip) call these functions, so a canvas gets the same bits from either.
#pragma once
#include "common.h"

// ---- merge: one step of the rasterio.merge callback's rule (inference/geotiff_raster.py:294-347) on one pixel --------------
// (V, Wt): the running score and weight; (v, w): the next plot's.  Each product, sum and quotient rounded to fp32 on its own, as
// numpy does on the reference's float32 canvas (bit-exact against tests/golden/f_mosaic.npz): no fused multiply-add
__device__ __forceinline__ void mosaic_fold(float& V, float& Wt, float v, float w) {
#pragma clang fp contract(off)
    const float nan = __int_as_float(0x7fc00000);
    const bool on = V != V, nn = v != v, own = Wt != Wt, nwn = w != w;
    if (on && nn) {
        V = nan;
    } else {
        float a_old = V * Wt, a_new = v * w;               // NaN (no data) contributes nothing: np.nansum
        a_old = (on || a_old != a_old) ? 0.f : a_old;
        a_new = (nn || a_new != a_new) ? 0.f : a_new;
        const float w_old = (on || own) ? 0.f : Wt, w_new = (nn || nwn) ? 0.f : w;
        V = (a_old + a_new) / (w_old + w_new);
    }
    Wt = (own && nwn) ? nan : (own ? 0.f : Wt) + (nwn ? 0.f : w);
}

// the fold of plots [b0, b1) in order into pixel (gy, gx) of one band of a (3,H,W) canvas; off: the (row, col) of plot b's
// top-left pixel at off[stride * b], off[stride * b + 1].  b0, b1, off, stride wave-uniform (scalar loads).
__device__ __forceinline__ void mosaic_fold_pixel(const float* __restrict__ rasters, const float* __restrict__ weights,
                                                  const int* __restrict__ off, int stride, int b0, int b1, int D, int band, int H,
                                                  int W, int gy, int gx, float* __restrict__ mean, float* __restrict__ wsum) {
    const size_t o = ((size_t)band * H + gy) * W + gx;
    float V = mean[o], Wt = wsum[o];
    for (int b = b0; b < b1; ++b) {
        const int y = gy - off[(size_t)stride * b], x = gx - off[(size_t)stride * b + 1];
        if (y < 0 || y >= D || x < 0 || x >= D) continue;     // pixel outside this plot's raster: the callback is not
                                                              // called on it
        mosaic_fold(V, Wt, rasters[(((size_t)b * 3 + band) * D + y) * D + x], weights[y * D + x]);
    }
    mean[o] = V;
    wsum[o] = Wt;
}

// ---- finalisation: thresholds lin[i] = i * (1/10000) in fp64, lin[10000] = 1 (np.linspace) -----------------------------------
constexpr int HARD_STEPS = 10001;

__device__ __forceinline__ double hard_lin(int i) { return i >= HARD_STEPS - 1 ? 1.0 : (double)i * (1.0 / 10000.0); }

// k(v) = #{ i : lin[i] < v }, the comparison in fp64
__device__ __forceinline__ int hard_bin(double v) {
    int k = (int)floor(v * 10000.0);
    k = k < 0 ? 0 : (k > HARD_STEPS - 1 ? HARD_STEPS - 1 : k);
    while (k <= HARD_STEPS - 1 && hard_lin(k) < v) ++k;
    while (k > 0 && !(hard_lin(k - 1) < v)) --k;
    return k;
}

__device__ __forceinline__ double rules_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ long long rules_wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int rules_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// A workgroup of 256 bins the valid values of med[i], i = first, first + step, ... < P, into hist (int atomics) and returns --
// in thread 0 -- their number and fp64 sum: a thread adds its values in that order, the lanes of a wave are summed in the
// xor tree, the four waves as (0 + 1) + (2 + 3).
__device__ __forceinline__ void hard_hist_block(const float* __restrict__ med, long P, long first, long step,
                                                int* __restrict__ hist, double& sum_out, int& cnt_out) {
    __shared__ double s_sum[4];
    __shared__ int s_cnt[4];
    double acc = 0.0;
    int nv = 0;
    for (long i = first + threadIdx.x; i < P; i += step) {
        const float vf = med[i];
        if (vf != vf) continue;
        const double v = (double)vf;
        atomicAdd(&hist[hard_bin(v)], 1);
        acc += v;
        ++nv;
    }
    acc = rules_wave_sum(acc);
    nv = rules_wave_sum(nv);
    if ((threadIdx.x & 63) == 0) { s_sum[threadIdx.x >> 6] = acc; s_cnt[threadIdx.x >> 6] = nv; }
    __syncthreads();
    sum_out = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
    cnt_out = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}

// One workgroup of 1024: suffix sums of the histogram ws[0..HARD_STEPS], deltas, first minimum -> thr_out[0] = threshold (fp64
// value as float), thr_out[1] = index.  nvalid: the number of valid pixels, sum: their fp64 sum (both uniform).
__device__ __forceinline__ void hard_threshold_search(const int* __restrict__ ws, int nvalid, double sum, float* __restrict__ thr_out) {
    __shared__ long long s_above[HARD_STEPS + 1];     // s_above[i] = #{pixels with k > i}
    __shared__ double s_best[1024];
    __shared__ int s_idx[1024];
    __shared__ long long s_chunk[1024];
    const int tid = threadIdx.x;
    // chunked suffix sum over k = HARD_STEPS .. 0: 1024 threads x 10 bins
    constexpr int PER = (HARD_STEPS + 1 + 1023) / 1024;
    long long loc = 0;
    const int hi = HARD_STEPS - tid * PER;            // this thread's bins: hi, hi-1, ... (descending)
    for (int j = 0; j < PER; ++j) {
        const int k = hi - j;
        if (k >= 0) loc += ws[k];
    }
    s_chunk[tid] = loc;
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        for (int t = 0; t < 1024; ++t) { const long long c = s_chunk[t]; s_chunk[t] = run; run += c; }
    }
    __syncthreads();
    long long run = s_chunk[tid];                     // pixels with k above this thread's highest bin
    for (int j = 0; j < PER; ++j) {
        const int k = hi - j;
        if (k >= 0) {
            if (k <= HARD_STEPS) s_above[k] = run;    // #{k' > k}
            run += ws[k];
        }
    }
    __syncthreads();
    // np.nanmean of a float32 image is a float32; the hard images are fp64 (1.0 * bool)
    const double target = nvalid > 0 ? (double)(float)(sum / (double)nvalid) : __longlong_as_double(0x7ff8000000000000LL);
    double best = INFINITY;
    int bidx = 0x7FFFFFFF;
    for (int i = tid; i < HARD_STEPS; i += 1024) {
        // pixels with v > lin[i]  <=>  k(v) > i
        const double hard_mean = nvalid > 0 ? (double)s_above[i] / (double)nvalid : __longlong_as_double(0x7ff8000000000000LL);
        const double d = fabs(target - hard_mean);
        if (d < best) { best = d; bidx = i; }         // ascending i per thread: first minimum kept
    }
    s_best[tid] = best;
    s_idx[tid] = bidx;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o) {
            const double ob = s_best[tid + o];
            const int oi = s_idx[tid + o];
            if (ob < s_best[tid] || (ob == s_best[tid] && oi < s_idx[tid])) { s_best[tid] = ob; s_idx[tid] = oi; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int i = s_idx[0] == 0x7FFFFFFF ? 0 : s_idx[0];   // all-NaN deltas: np.argmin returns 0
        thr_out[0] = (float)hard_lin(i);
        thr_out[1] = (float)i;
    }
}

// pixel i of out (5,H,W) = [Vb, Vm_soft, Vh, Vm_hard, weights] with the reference's NaN rule: NaN -> 0 wherever at least one of
// the three scores is a number, all bands NaN elsewhere.  P = H W; t: the threshold, hard_lin(index).
__device__ __forceinline__ void mosaic_finalize_pixel(const float* __restrict__ mean, const float* __restrict__ wsum, long P, long i,
                                                      double t, float* __restrict__ out) {
    const float nanv = __int_as_float(0x7fc00000);
    const float b0 = mean[i], b1 = mean[P + i], b2 = mean[2 * P + i], w = wsum[i];
    const bool none = (b0 != b0) && (b1 != b1) && (b2 != b2);
    float hard = (b1 != b1) ? nanv : (((double)b1 > t) ? 1.f : 0.f);
    auto fix = [&](float v) { return none ? nanv : (v != v ? 0.f : v); };
    out[i] = fix(b0);
    out[P + i] = fix(b1);
    out[2 * P + i] = fix(b2);
    out[3 * P + i] = fix(hard);
    out[4 * P + i] = fix(w);
}

// ---- crop and band statistics (the rule is written out in include/strata_hip.h: sn2_mosaic_crop_stats) ----------------------
// A workgroup owns a row segment of 256 pixels, one per thread.  py is a function of the row, so the workgroup walks the E
// edges once, 256 at a time, and collects the xint of those that cross the row in LDS (wave ballot + prefix); a thread then
// counts the list entries right of its own px.  The list is counted and emptied whenever the next 256 edges might not fit, so
// any E and any number of crossings go through.  The expressions are those of the per-pixel test, so are the bits.
constexpr int CROP_T = 256;                           // threads = pixels of a row segment = edges of a chunk
constexpr int CROP_LIST = 1024;                       // crossings held in LDS between two counting passes
constexpr int CROP_C = SN2_MOSAIC_CROP_MAX_BANDS;

struct CropLds {
    double x[CROP_LIST];
    int wn[CROP_T / 64];
    double sum[CROP_T / 64][CROP_C];
    long long cnt[CROP_T / 64][CROP_C];
};

// Workgroup `blk` of `nblk` takes the row segments blk, blk + nblk, ... of bands (C,H,W); psum, pcnt: its C partial sums and
// counts, every entry written.  blk, nblk and every other argument uniform over the workgroup.
template <bool CROP>
__device__ __forceinline__ void mosaic_crop_block(CropLds& s, float* __restrict__ bands, int C, int H, int W, double x_min,
                                                  double y_max, double pix, const double* __restrict__ edges, int E, int blk,
                                                  int nblk, double* __restrict__ psum, long long* __restrict__ pcnt) {
    // every product, difference, quotient and sum below rounded to fp64 on its own, as numpy does: no fused multiply-add
#pragma clang fp contract(off)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int segs = (W + CROP_T - 1) / CROP_T;
    const long nrs = (long)H * segs;
    const size_t P = (size_t)H * W;
    const float nanv = __int_as_float(0x7fc00000);
    double acc[CROP_C];
    long long cnt[CROP_C];
#pragma unroll
    for (int k = 0; k < CROP_C; ++k) { acc[k] = 0.0; cnt[k] = 0; }

    for (long rs = blk; rs < nrs; rs += nblk) {                      // uniform over the workgroup: the barriers below are safe
        const int r = (int)(rs / segs), c = (int)(rs % segs) * CROP_T + tid;
        bool inside = true;
        if (CROP) {
            const double py = y_max - pix * ((double)r + 0.5);
            const double px = x_min + pix * ((double)c + 0.5);
            int right = 0;                                           // crossing edges with px < xint
            int n = 0;                                               // entries of s.x (uniform)
            for (int e0 = 0; e0 < E; e0 += CROP_T) {
                const int e = e0 + tid;
                bool cr = false;
                double xint = 0.0;
                if (e < E) {
                    const double ax = edges[4 * (size_t)e], ay = edges[4 * (size_t)e + 1];
                    const double bx = edges[4 * (size_t)e + 2], by = edges[4 * (size_t)e + 3];
                    cr = (ay > py) != (by > py);
                    if (cr) xint = ax + ((py - ay) * (bx - ax)) / (by - ay);
                }
                const unsigned long long m = __ballot(cr);
                if (lane == 0) s.wn[wave] = __popcll(m);
                __syncthreads();                                     // (also: the last counting pass over s.x is over)
                int base = n, total = 0;
#pragma unroll
                for (int w = 0; w < CROP_T / 64; ++w) {
                    const int v = s.wn[w];
                    base += w < wave ? v : 0;
                    total += v;
                }
                if (cr) s.x[base + __popcll(m & ((1ull << lane) - 1ull))] = xint;     // n + total <= CROP_LIST: see below
                n += total;
                __syncthreads();
                if (n + CROP_T > CROP_LIST || e0 + CROP_T >= E) {    // the next chunk might not fit, or there is none
                    for (int i = 0; i < n; ++i) right += px < s.x[i] ? 1 : 0;
                    n = 0;
                }
            }
            inside = (right & 1) != 0;
        }
        if (c < W) {
            const size_t o = (size_t)r * W + c;
#pragma unroll
            for (int k = 0; k < CROP_C; ++k) {
                if (k < C) {
                    if (CROP && !inside) {
                        bands[k * P + o] = nanv;
                    } else {
                        const float v = bands[k * P + o];
                        if (v == v) { acc[k] += (double)v; ++cnt[k]; }
                    }
                }
            }
        }
    }
    __syncthreads();                                                 // (a caller may run this twice: s.sum, s.cnt are free again)
#pragma unroll
    for (int k = 0; k < CROP_C; ++k) {
        if (k < C) {
            const double sm = rules_wave_sum(acc[k]);
            const long long q = rules_wave_sum(cnt[k]);
            if (lane == 0) { s.sum[wave][k] = sm; s.cnt[wave][k] = q; }
        }
    }
    __syncthreads();
    if (tid < C) {
        psum[tid] = (s.sum[0][tid] + s.sum[1][tid]) + (s.sum[2][tid] + s.sum[3][tid]);
        pcnt[tid] = (s.cnt[0][tid] + s.cnt[1][tid]) + (s.cnt[2][tid] + s.cnt[3][tid]);
    }
}

// one workgroup: thread t adds the partials of workgroups t, t + 256, ... in order, the threads in a fixed tree
__device__ __forceinline__ void mosaic_crop_fold(const double* __restrict__ psum, const long long* __restrict__ pcnt, int C, int nblk,
                                                 double* __restrict__ mean, long long* __restrict__ count) {
    __shared__ double s_sum[CROP_T / 64];
    __shared__ long long s_cnt[CROP_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = 0; k < C; ++k) {
        double s = 0.0;
        long long q = 0;
        for (int b = tid; b < nblk; b += CROP_T) { s += psum[(size_t)b * C + k]; q += pcnt[(size_t)b * C + k]; }
        s = rules_wave_sum(s);
        q = rules_wave_sum(q);
        if (lane == 0) { s_sum[wave] = s; s_cnt[wave] = q; }
        __syncthreads();
        if (tid == 0) {
            const double t = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
            const long long n = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
            mean[k] = n > 0 ? t / (double)n : __longlong_as_double(0x7ff8000000000000LL);
            count[k] = n;
        }
        __syncthreads();
    }
}
