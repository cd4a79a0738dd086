// ortho_rules.h -- the rule that colours the points of a cloud from georeferenced orthoimages (include/strata_hip.h, "Orthoimage
// colours"), stated once: the pixel of an image that holds a point, the address of a sample in either layout, the step of the walk
// over the image list for one point and one image, and the checks of the set and of the launch.  The kernel of ortho.hip, the
// host-side checks of sn2_ortho_colorize and a stand-alone host program (scripts/ortho_rules_sanitize.cpp: the rule and the
// validator under a sanitizer) execute these functions; ortho.colorize_ref states the same rule in numpy, and the kernel gives
// its rows, `covered` and `missing` bit for bit.  Every difference and quotient of the rule is rounded to fp64 on its own.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/strata_hip.h"

#if defined(__HIPCC__)
#define ORTHO_FN __host__ __device__ __forceinline__
#else
#define ORTHO_FN inline
#endif
#if defined(__clang__)
#define ORTHO_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define ORTHO_NO_CONTRACT
#endif

constexpr int ORTHO_MAX_IMAGES = SN2_ORTHO_MAX_IMAGES;
constexpr int ORTHO_MAX_MAP = SN2_ORTHO_MAX_MAP;
constexpr long long ORTHO_MAX_SAMPLES = SN2_ORTHO_MAX_SAMPLES;     // W H C of one image
constexpr int ORTHO_ROW_LO = 3, ORTHO_ROW_HI = 9;                  // the rows a launch may write; 0 and 1 are its input

// the pixel whose area holds (x, y): false outside the image.  The comparisons are made in fp64 before any conversion to int, so
// a NaN or infinite coordinate is outside; inside, 0 <= floor(u) < W and 0 <= floor(v) < H fit an int.
ORTHO_FN bool ortho_locate(const sn2_ortho_image& im, double x, double y, int* col, int* row) {
    ORTHO_NO_CONTRACT
    const double u = (x - im.x0) / im.px;
    const double v = (im.y0 - y) / im.py;
    if (u >= 0.0 && u < (double)im.W && v >= 0.0 && v < (double)im.H) {
        *col = (int)floor(u);
        *row = (int)floor(v);
        return true;
    }
    return false;
}

// the sample of `band` at (row, col), in samples from the image's first: chunky (H,W,C) or planar (C,H,W).  64-bit throughout.
template <bool PLANAR>
ORTHO_FN size_t ortho_index(int C, const sn2_ortho_image& im, int row, int col, int band) {
    if (PLANAR) return ((size_t)band * (size_t)im.H + (size_t)row) * (size_t)im.W + (size_t)col;
    return ((size_t)row * (size_t)im.W + (size_t)col) * (size_t)C + (size_t)band;
}

// One step of the walk: the point's pixel (row, col) of image `im`.  vals[k] = (float)sample[band[k]] * scale for k < n_map;
// false = the pixel is nodata (every sampled band equals the set's nodata value) and the point stays in the walk.
template <class PT, bool PLANAR>
ORTHO_FN bool ortho_sample(const sn2_ortho_set& s, const sn2_ortho_image& im, int row, int col, float* vals) {
    const PT* p = (const PT*)im.pixels;
    bool nodata = s.has_nodata != 0;
#pragma unroll
    for (int k = 0; k < ORTHO_MAX_MAP; ++k)
        if (k < s.n_map) {
            const PT q = p[ortho_index<PLANAR>(s.C, im, row, col, s.band[k])];
            nodata = nodata && (double)q == s.nodata;
            vals[k] = (float)q * s.scale;
        }
    return !nodata;
}

// The whole walk for one point, serially: the 1-based index of the first image that covers (x, y) with a pixel that is not nodata
// (vals filled), or 0.  The kernel makes the same steps with a ballot per image in between.
template <class PT, bool PLANAR>
ORTHO_FN int ortho_point(const sn2_ortho_set& s, double x, double y, float* vals) {
    for (int i = 0; i < s.S; ++i) {
        int col, row;
        if (ortho_locate(s.image[i], x, y, &col, &row) && ortho_sample<PT, PLANAR>(s, s.image[i], row, col, vals)) return i + 1;
    }
    return 0;
}

// ---- the checks of the header, on the host copy ------------------------------------------------------------------------------
inline int ortho_sample_bytes(int dtype) { return dtype == SN2_ORTHO_U8 ? 1 : (dtype == SN2_ORTHO_U16 ? 2 : (dtype == SN2_ORTHO_F32 ? 4 : 0)); }

inline int ortho_check_set(const sn2_ortho_set* s) {
    if (!s) return SN2_EINVAL;
    if (s->S < 1 || s->S > ORTHO_MAX_IMAGES || s->C < 1) return SN2_EINVAL;
    if (ortho_sample_bytes(s->dtype) == 0 || (s->layout != SN2_ORTHO_CHUNKY && s->layout != SN2_ORTHO_PLANAR)) return SN2_EINVAL;
    if (s->n_map < 1 || s->n_map > ORTHO_MAX_MAP) return SN2_EINVAL;
    for (int k = 0; k < s->n_map; ++k) {
        if (s->band[k] < 0 || s->band[k] >= s->C) return SN2_EINVAL;
        if (s->row[k] < ORTHO_ROW_LO || s->row[k] > ORTHO_ROW_HI) return SN2_EINVAL;
        for (int j = 0; j < k; ++j)
            if (s->row[j] == s->row[k]) return SN2_EINVAL;
    }
    if (!isfinite(s->scale)) return SN2_EINVAL;
    if (s->has_nodata && s->nodata != s->nodata) return SN2_EINVAL;
    for (int i = 0; i < s->S; ++i) {
        const sn2_ortho_image& im = s->image[i];
        if (!isfinite(im.x0) || !isfinite(im.y0) || !isfinite(im.px) || !isfinite(im.py) || !(im.px > 0.0) || !(im.py > 0.0))
            return SN2_EINVAL;
        if (im.W < 1 || im.H < 1 || !im.pixels) return SN2_EINVAL;
    }
    for (int i = 0; i < s->S; ++i)
        if ((long long)s->image[i].W * s->image[i].H > (ORTHO_MAX_SAMPLES - 1) / s->C) return SN2_ELIMIT;
    return 0;
}

inline int ortho_check_launch(const void* cloud, long row_stride, long col0, long T, const void* missing) {
    if (!cloud || !missing) return SN2_EINVAL;
    if (T < 0 || col0 < 0 || row_stride < 0 || col0 > row_stride || T > row_stride - col0) return SN2_EINVAL;
    if (T >= (1L << 31)) return SN2_ELIMIT;
    return 0;
}
