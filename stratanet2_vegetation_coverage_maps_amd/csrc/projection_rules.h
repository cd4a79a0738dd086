// projection_rules.h -- the scatter-max projection of project.hip, stated once: the pixel of a point, the 64-bit key of a
// (value, point) pair, the scatter of a workgroup's slice of a plot into its LDS key table, and the finalisation of one plot
// (maximum over the slices' tables, arg-max points, sums over the occupied pixels).  Every P2 route (sn2_plot_project_forward,
// _forward_pix, sn2_projected_loss_forward, sn2_plot_losses) and the P1 rasters execute these functions, so the routes give each
// other's pred / arg / nocc bits by construction.
#pragma once
#include "common.h"

// project_to_2d.py:16-22   floor((xy - min) / (max - min + 0.0001) * diam_pix).int()
__device__ __forceinline__ int p2_pix(float v, float mn, float mx, int D) {
#pragma clang fp contract(off)
    const float num = v - mn;
    const float den = (mx - mn) + 0.0001f;
    const float q = num / den;
    const float s = q * (float)D;
    int i = (int)floorf(s);
    return i < 0 ? 0 : (i > D - 1 ? D - 1 : i);
}

// project_to_2d.py:68-78   clip(floor((xy + 0.0001) * scaling_factor + diam_meters // 2).int(), 0, diam_pix - 1)
__device__ __forceinline__ int p1_pix(float v, float sf, float off, int D) {
#pragma clang fp contract(off)
    const float t = v + 0.0001f;
    const float m = t * sf;
    const float s = m + off;
    int i = (int)floorf(s);
    return i < 0 ? 0 : (i > D - 1 ? D - 1 : i);
}

// slices of a plot's N points that scatter side by side (SN2_P2_KEY_PARTS)
static inline int grid_slices(int N) {
    int s = sn2_cdiv(N, 4096);
    return s < 1 ? 1 : (s > 64 ? 64 : s);
}

// ---- the key: (ordered(value) << 32) | ~point.  An integer maximum over keys picks the largest value and, among equal values,
// the FIRST point (as torch_scatter's CPU loop); it does not depend on the order of arrival.  0 = nothing arrived (f2ord > 0).
__device__ __forceinline__ unsigned long long pj_key(float v, int n) {
    return ((unsigned long long)f2ord(v) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)n);
}
__device__ __forceinline__ float pj_key_value(unsigned long long k) { return ord2f((uint32_t)(k >> 32)); }
__device__ __forceinline__ int pj_key_point(unsigned long long k) { return (int)(0xFFFFFFFFu - (uint32_t)(k & 0xFFFFFFFFull)); }

// ---- the scatter of one slice by a 1024-thread workgroup; s_keys: its D*D*3 keys in LDS.  The workgroup's barriers stand in
// the kernels: one behind pj_clear, one in front of pj_copy_out.
__device__ __forceinline__ void pj_clear(unsigned long long* s_keys, int ncell3) {
    for (int i = threadIdx.x; i < ncell3; i += 1024) s_keys[i] = 0ull;
}

// rows [lo, hi) of slice `part` of `parts`
__device__ __forceinline__ void pj_slice(int N, int parts, int part, int& lo, int& hi) {
    const int per = (N + parts - 1) / parts;
    lo = part * per;
    hi = min(N, lo + per);
}

// point n of the plot, coverages v = (low, soil, medium, high), falls into `cell`: the three projected channels are x, z, w
__device__ __forceinline__ void pj_push(unsigned long long* s_keys, int cell, float4 v, int n) {
    atomicMax(&s_keys[cell * 3 + 0], pj_key(v.x, n));
    atomicMax(&s_keys[cell * 3 + 1], pj_key(v.z, n));
    atomicMax(&s_keys[cell * 3 + 2], pj_key(v.w, n));
}

// MERGE false: g is the slice's own table, every key stored; true: g is the plot's one table, cleared before the launch, and the
// touched keys are merged into it by global atomics
template <bool MERGE>
__device__ __forceinline__ void pj_copy_out(const unsigned long long* s_keys, int ncell3, unsigned long long* __restrict__ g) {
    for (int i = threadIdx.x; i < ncell3; i += 1024) {
        const unsigned long long k = s_keys[i];
        if (!MERGE) g[i] = k;
        else if (k) atomicMax(&g[i], k);
    }
}

// the whole of it for a workgroup that does nothing else: slice `part` of plot b, from stored pixel ids, into the slice's own
// table of keys_part (B, parts, D*D*3)
__device__ __forceinline__ void pj_scatter_slice(unsigned long long* s_keys, const float* __restrict__ vals,
                                                 const int* __restrict__ pix, int N, int D, int b, int parts, int part,
                                                 unsigned long long* __restrict__ keys_part) {
    const int ncell3 = D * D * 3;
    pj_clear(s_keys, ncell3);
    __syncthreads();
    int lo, hi;
    pj_slice(N, parts, part, lo, hi);
    for (int n = lo + threadIdx.x; n < hi; n += 1024)
        pj_push(s_keys, pix[(size_t)b * N + n], reinterpret_cast<const float4*>(vals)[(size_t)b * N + n], n);
    __syncthreads();
    pj_copy_out<false>(s_keys, ncell3, keys_part + ((size_t)b * parts + part) * ncell3);
}

// ---- the finalisation of plot b by a 256-thread workgroup: per cell the maximum over the plot's `parts` key tables (keys:
// (B, parts, D*D, 3)), ARG: the arg-max points to arg (B, D*D, 3), -1 on an empty cell; then the sums over the occupied cells
// of low, 1 - low, medium, high and their number, lanes by wave_sum, the four waves as (s0 + s1) + (s2 + s3).  -> t[0..4] in
// thread 0 (only there); pred = t[0..3] / max(t[4], 1), nocc = t[4].
template <bool ARG>
__device__ __forceinline__ void pj_finalize_plot(const unsigned long long* __restrict__ keys, int b, int D, int parts,
                                                 int* __restrict__ arg, float (&s)[5][4], float (&t)[5]) {
    const int ncell = D * D;
    float lo = 0.f, so = 0.f, me = 0.f, hi = 0.f, cnt = 0.f;
    for (int c = threadIdx.x; c < ncell; c += 256) {
        const size_t base = ((size_t)b * ncell + c) * 3;
        const unsigned long long* kp = keys + ((size_t)b * parts * ncell + c) * 3;
        unsigned long long k0 = kp[0], k1 = kp[1], k2 = kp[2];
        for (int q = 1; q < parts; ++q) {
            const unsigned long long* kq = kp + (size_t)q * ncell * 3;
            const unsigned long long a0 = kq[0], a1 = kq[1], a2 = kq[2];
            k0 = a0 > k0 ? a0 : k0;
            k1 = a1 > k1 ? a1 : k1;
            k2 = a2 > k2 ? a2 : k2;
        }
        if (k0) {
            const float l = pj_key_value(k0);
            lo += l;
            so += 1.0f - l;
            me += pj_key_value(k1);
            hi += pj_key_value(k2);
            cnt += 1.f;
        }
        if (ARG) {
            arg[base + 0] = k0 ? pj_key_point(k0) : -1;       // (a cell's three channels are occupied together)
            arg[base + 1] = k0 ? pj_key_point(k1) : -1;
            arg[base + 2] = k0 ? pj_key_point(k2) : -1;
        }
    }
    lo = wave_sum(lo);
    so = wave_sum(so);
    me = wave_sum(me);
    hi = wave_sum(hi);
    cnt = wave_sum(cnt);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s[0][w] = lo, s[1][w] = so, s[2][w] = me, s[3][w] = hi, s[4][w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int q = 0; q < 5; ++q) t[q] = (s[q][0] + s[q][1]) + (s[q][2] + s[q][3]);
}
