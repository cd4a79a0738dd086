// ortho.hip -- rows 3..9 of the (10,T) cloud looked up per point in georeferenced orthoimages: one launch per image set.
// Host side: ortho.py (colorize), hip_ops.ortho_colorize.
//
// Contract (include/strata_hip.h, "Orthoimage colours"):
//   - the rule is stated once, in ortho_rules.h; the kernel only puts a ballot between its steps;
//   - the entry point checks the set's host copy before it launches, so no index derived from it leaves an image or the cloud;
//   - the output bytes do not depend on arrival order: one integer atomic per wave, no floating-point atomics.
#include "common.h"
#include "ortho_rules.h"

namespace {

constexpr int ORTHO_WG = 256;

// One point per lane.  The set is a kernel argument by value: `set.image[s]` with the wave-uniform s is read with scalar loads.
// A wave touches image s only if one of its lanes is still unserved and inside it; a lane on a nodata pixel stays in the walk.
template <class PT, bool PLANAR>
__global__ __launch_bounds__(ORTHO_WG) void ortho_colorize_kernel(float* __restrict__ cloud, size_t row_stride, size_t col0, long T,
                                                                  const sn2_ortho_set set, unsigned char* __restrict__ covered,
                                                                  unsigned long long* __restrict__ missing) {
    const long i = (long)blockIdx.x * ORTHO_WG + threadIdx.x;
    const bool live = i < T;
    double x = 0.0, y = 0.0;
    if (live) {
        x = (double)cloud[col0 + (size_t)i];
        y = (double)cloud[row_stride + col0 + (size_t)i];
    }
    bool open = live;                                      // not served yet
    int served = 0;
    for (int s = 0; s < set.S; ++s) {
        if (__ballot(open) == 0ull) break;
        const sn2_ortho_image& im = set.image[s];
        int col = 0, row = 0;
        const bool in = open && ortho_locate(im, x, y, &col, &row);
        if (__ballot(in) == 0ull) continue;
        if (in) {
            float vals[ORTHO_MAX_MAP];
            if (ortho_sample<PT, PLANAR>(set, im, row, col, vals)) {
#pragma unroll
                for (int k = 0; k < ORTHO_MAX_MAP; ++k)
                    if (k < set.n_map) cloud[(size_t)set.row[k] * row_stride + col0 + (size_t)i] = vals[k];
                served = s + 1;
                open = false;
            }
        }
    }
    if (live && covered) covered[i] = (unsigned char)served;
    const unsigned long long mask = __ballot(open);
    if (mask != 0ull && (threadIdx.x & 63) == 0) atomicAdd(missing, (unsigned long long)__popcll(mask));
}

template <class PT>
void launch(bool planar, float* cloud, long row_stride, long col0, long T, const sn2_ortho_set& set, unsigned char* covered,
            long long* missing, hipStream_t st) {
    const dim3 grid(sn2_cdiv(T, ORTHO_WG)), block(ORTHO_WG);
    if (planar)
        hipLaunchKernelGGL((ortho_colorize_kernel<PT, true>), grid, block, 0, st, cloud, (size_t)row_stride, (size_t)col0, T, set, covered,
                           reinterpret_cast<unsigned long long*>(missing));
    else
        hipLaunchKernelGGL((ortho_colorize_kernel<PT, false>), grid, block, 0, st, cloud, (size_t)row_stride, (size_t)col0, T, set, covered,
                           reinterpret_cast<unsigned long long*>(missing));
}
}  // namespace

extern "C" int sn2_ortho_colorize(float* cloud, long row_stride, long col0, long T, const sn2_ortho_set* set, unsigned char* covered,
                                  long long* missing, void* stream) {
    SN2_TRY(ortho_check_set(set));
    SN2_TRY(ortho_check_launch(cloud, row_stride, col0, T, missing));
    if (T == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const bool planar = set->layout == SN2_ORTHO_PLANAR;
    if (set->dtype == SN2_ORTHO_U8) launch<uint8_t>(planar, cloud, row_stride, col0, T, *set, covered, missing, st);
    else if (set->dtype == SN2_ORTHO_U16) launch<uint16_t>(planar, cloud, row_stride, col0, T, *set, covered, missing, st);
    else launch<float>(planar, cloud, row_stride, col0, T, *set, covered, missing, st);
    SN2_RETURN_LAUNCH();
}
