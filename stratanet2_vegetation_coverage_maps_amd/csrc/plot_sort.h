// plot_sort.h -- the per-plot counting sort (one workgroup bins a plot's points into a cell grid in LDS: histogram, exclusive
// scan of the cells, scatter through cursor atomics) and the workgroup scan, stated once.  Device-only, internal linkage.
// Integer arithmetic on counts and exact min / max: a caller gets the bits a hand-written copy gives.
#pragma once
#include "common.h"

// inclusive prefix sum over the 64 lanes of a wave (int or long long)
template <typename T>
__device__ __forceinline__ T wave_scan_incl(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

// carry + the exclusive prefix sum of every thread's `sum` over the workgroup; total = carry + the sum of all threads, the carry
// of a caller's next round.  NT = the workgroup's size, or an upper bound of it where `total` is not used (the words of waves
// that do not exist are read and dropped).  s_wsum: NT / 64 words of LDS.  Two barriers, reached by every thread: between
// posting and reading the wave totals, and behind the reads -- on return s_wsum is free for the next call.
template <int NT, typename T>
__device__ __forceinline__ T block_scan_excl(T sum, T* s_wsum, T carry, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T incl = wave_scan_incl(sum);
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    T below = carry, all = carry;
#pragma unroll 4
    for (int k = 0; k < NT / 64; ++k) {                // (four reads in flight)
        const T w = s_wsum[k];
        all += w;
        if (k < wave) below += w;
    }
    __syncthreads();
    total = all;
    return below + incl - sum;
}
template <int NT, typename T>
__device__ __forceinline__ T block_scan_excl(T sum, T* s_wsum, T carry = 0) {
    T total;
    return block_scan_excl<NT>(sum, s_wsum, carry, total);
}

// In-place exclusive scan of the LDS counters s_hist[0, ncell), ncell <= MAXCELL, ceil(MAXCELL / NT) consecutive cells per
// thread.  publish(cell, start) is called once per cell; with END the last thread also writes the end word s_hist[ncell] = the
// sum of all counts and publishes it as cell `ncell`.  The counts are complete on entry (a barrier behind the last add); on
// return (a barrier) the starts are in place for everybody and s_wsum is free.
template <int NT, int MAXCELL, bool END, typename Publish>
__device__ __forceinline__ void block_scan_cells(int* s_hist, int ncell, int* s_wsum, Publish publish) {
    constexpr int PER = (MAXCELL + NT - 1) / NT;
    const int c0 = threadIdx.x * PER;
    int loc[PER], sum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        loc[k] = c0 + k < ncell ? s_hist[c0 + k] : 0;
        sum += loc[k];
    }
    int run = block_scan_excl<NT>(sum, s_wsum);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (c0 + k < ncell) {
            s_hist[c0 + k] = run;
            publish(c0 + k, run);
        }
        run += loc[k];
    }
    if (END && threadIdx.x == NT - 1) {     // the last thread ends the scan whatever ncell is (cells past it add 0)
        s_hist[ncell] = run;
        publish(ncell, run);
    }
    __syncthreads();
}

// The workgroup's bounding box on A axes: in, every thread's own min / max; out, the workgroup's.  Two wave reductions: over
// a wave's lanes, then over the waves' results in s_mm (2 A rows).  One barrier; s_mm is read until the workgroup's next one.
template <int NT, int A>
__device__ __forceinline__ void block_minmax(float (&mn)[A], float (&mx)[A], float (*s_mm)[NT / 64]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        mn[a] = wave_min(mn[a]);
        mx[a] = wave_max(mx[a]);
        if (lane == 0) {
            s_mm[a][wave] = mn[a];
            s_mm[A + a][wave] = mx[a];
        }
    }
    __syncthreads();
    const int w = lane < NT / 64 ? lane : 0;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        mn[a] = wave_min(s_mm[a][w]);
        mx[a] = wave_max(s_mm[A + a][w]);
    }
}

// fn(i, load(i)) for every point i < n, thread t taking t, t + NT, ...: a trip issues the loads of U points per thread before it
// touches the first.  The tail loads point n - 1 again and drops it; what fn does not use of a point is not loaded.
template <int U, int NT, typename Load, typename Fn>
__device__ __forceinline__ void for_plot_points(int n, Load load, Fn fn) {
    for (int i0 = threadIdx.x; i0 < n; i0 += NT * U) {
        decltype(load(0)) v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * NT;
            v[u] = load(i < n ? i : n - 1);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * NT;
            if (i < n) fn(i, v[u]);
        }
    }
}

// The counting sort of a plot's n points into ncell <= MAXCELL cells by one workgroup of NT threads: zero s_hist (ncell words,
// + 1 with END), count key_of(point), scan (publish as block_scan_cells), then emit(i, p, point), p = the point's position from
// its cell's cursor: the order inside a cell is whatever the LDS atomics give.  Ends without a barrier.
template <int U, int NT, int MAXCELL, bool END, typename Load, typename Key, typename Publish, typename Emit>
__device__ __forceinline__ void plot_counting_sort(int* s_hist, int ncell, int n, Load load, Key key_of, Publish publish,
                                                   Emit emit) {
    __shared__ int s_wsum[NT / 64];
    for (int i = threadIdx.x; i < ncell + (END ? 1 : 0); i += NT) s_hist[i] = 0;
    __syncthreads();
    for_plot_points<U, NT>(n, load, [&](int, auto v) { atomicAdd(&s_hist[key_of(v)], 1); });
    __syncthreads();
    block_scan_cells<NT, MAXCELL, END>(s_hist, ncell, s_wsum, publish);
    for_plot_points<U, NT>(n, load, [&](int i, auto v) { emit(i, atomicAdd(&s_hist[key_of(v)], 1), v); });
}
