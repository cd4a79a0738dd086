// global_level.h -- what the two one-launch kernels of the global level share (global_level.hip: the forward,
// global_level_bwd.hip: the backward): the {tag, value} granule of their exchanges, the POISON convention of a workgroup that
// gives up, the bounded collection of a phase's granules and the spin limit of its waits.
#pragma once
#include "fp_rows.h"

// sweeps (~1 us each) before an exchange wait gives up; sn2_debug_global_spin_limit sets it (defined in global_level.hip)
extern unsigned g_gl_spin_limit;

namespace {

typedef unsigned long long gl_u64;
constexpr int GL_GROUPS = 4;                     // groups of four waves in a 16-wave workgroup, one 64-row block each

// all granules of a phase -> s_x (floats), every thread its share, eight loads in flight, swept until every tag matches (or
// the limit runs out, or a publisher says that it gave up: the POISON tag = tag with the top bit flipped)
constexpr unsigned GL_POISON = 0x80000000u;
__device__ __forceinline__ bool gl_collect(const gl_u64* gx, int n, unsigned tag, float* s_x, unsigned spin_limit) {
    bool ok = true;
    for (int i0 = threadIdx.x; i0 < n; i0 += 8 * 1024) {
        gl_u64 v[8];
        unsigned spins = 0;
        bool all, poisoned;
        do {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * 1024;
                v[u] = __hip_atomic_load(gx + (i < n ? i : i0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            all = true, poisoned = false;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                all = all && (unsigned)(v[u] >> 32) == tag;
                poisoned = poisoned || (unsigned)(v[u] >> 32) == (tag ^ GL_POISON);
            }
            if (!all && !poisoned) __builtin_amdgcn_s_sleep(2);
        } while (!all && !poisoned && ++spins < spin_limit);
        if (!all) ok = false;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (i0 + u * 1024 < n) s_x[i0 + u * 1024] = __uint_as_float((unsigned)v[u]);
    }
    return ok;
}

}  // namespace
