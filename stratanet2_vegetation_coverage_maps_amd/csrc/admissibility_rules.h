// admissibility_rules.h -- the per-pixel and per-region rules of the admissibility band (include/strata_hip.h, "Admissibility
// band"), stated once.  The kernels of admissibility.hip execute these functions for a single canvas and for every canvas of an
// atlas alike, so both entry points give the same bytes.  The rule is OURS: a reading of insert_admissibility_raster
// (inference/geotiff_raster.py:149-196: rasterio sieve / shapes, a shapely buffer of -1.5, geometry_mask) on the pixel grid; the
// two places where the reading is not pinned -- the sieve size and the 1.5 px tie -- are marked UNPINNED below.
#pragma once
#include "common.h"

// a pixel takes part iff its hard medium-vegetation value is a number (the finalisation makes the five bands NaN together)
__device__ __forceinline__ bool adm_valid(float vm_hard) { return !(vm_hard != vm_hard); }
// the hard bit of a valid pixel
__device__ __forceinline__ int adm_hard_bit(float vm_hard) { return vm_hard > 0.f ? 1 : 0; }

// UNPINNED: the sieve size is the caller's.  A region is small iff size < sieve_size (so 0 and 1 sieve nothing).
__device__ __forceinline__ bool adm_small(int size, int sieve_size) { return size < sieve_size; }

// the neighbour key of a region: the LARGEST key among a small region's neighbours is its `big` -- the largest size, ties to the
// SMALLEST id (id = the region's smallest row-major pixel index).  A 64-bit integer maximum does not depend on the order of
// arrival.  0 = no neighbour (a size is at least 1).
__device__ __forceinline__ unsigned long long adm_neighbour_key(int size, int id) {
    return ((unsigned long long)(unsigned)size << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)id);
}
__device__ __forceinline__ unsigned adm_key_id(unsigned long long key) { return 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull); }

// the sieved hard band H': 1 outside the valid pixels (the reference sets the outside to one "to avoid border effects"), else
// min(h, S): a small patch of ones that the sieve turns to zero disappears, a small hole of zeros stays a hole
__device__ __forceinline__ int adm_sieved_bit(bool valid, int h, int S) { return valid ? (h < S ? h : S) : 1; }

// is the pixel at offset (dx, dy) within 1.5 px of the centre of the pixel at (0, 0)?  The left side is 4 x the squared distance
// from that centre to the pixel square at (dx, dy); 9 = 4 x 1.5^2.
// UNPINNED, THE TIE: the offsets (+-2, 0) and (0, +-2) give exactly 9 -- the centre lies ON the outline of the polygon buffered by
// -1.5.  `<` counts such a centre as inside the buffered polygon (the far pixel is NOT tested); `<=` would count it as outside.
// GDAL's scanline fill, which decides this in the reference, treats the four sides differently and cannot be run here.
constexpr int ADM_REACH = 2;     // offsets beyond +-2 are never within 1.5 px
__device__ __forceinline__ bool adm_offset_tested(int dx, int dy) {
    const int ax = 2 * (dx < 0 ? -dx : dx) - 1, ay = 2 * (dy < 0 ? -dy : dy) - 1;
    const int a = ax > 0 ? ax : 0, b = ay > 0 ? ay : 0;
    return a * a + b * b < 9;
}

// the band: NaN outside the valid pixels, 0 on an inaccessible pixel, else the larger of Vb and Vm_soft (fp32; both are numbers
// on a valid pixel; on a tie, signed zeros included, Vm_soft's bits)
__device__ __forceinline__ float adm_band(bool valid, bool inacc, float vb, float vm_soft) {
    if (!valid) return __int_as_float(0x7fc00000);
    if (inacc) return 0.f;
    return vb > vm_soft ? vb : vm_soft;
}
