// las.hip -- the point records of a LAS file, as the file holds them, to the ten fp32 rows of the reference's load_las_file
// (utils/load_data.py:149-184): x, y, z, red, green, blue, nir, intensity, return_num, num_returns.  Host side: las.py.
//
// Contract (include/strata_hip.h, "LAS point records"; the layout and the arithmetic: las_rules.h):
//   - one launch, no atomics, no synchronisation between workgroups, nothing read back: safe to capture;
//   - no load touches a byte at or beyond T * L, so nothing that follows the block can change the output;
//   - every lane writes its own column of its own rows: the same bytes in give the same bytes out.
//
// STAGED form (L <= LAS_STAGE_MAX_L): a workgroup of 256 takes 256 consecutive records = 256 L contiguous bytes that start at a
// multiple of 256 L, hence 16-byte aligned.  It copies them to LDS with 16-byte loads, lane after lane (the last workgroup's odd
// bytes one by one); each lane then assembles its record's fields from the aligned LDS words around them (v_alignbyte: with an
// odd L nothing is aligned) and stores ten coalesced floats.
// DIRECT form (longer records, of which a lane needs 38 bytes at most): a lane reads its fields from global memory byte by byte.
#include "common.h"
#include "las_rules.h"

namespace {

constexpr int LAS_WG = 256;
constexpr int LAS_STAGE_MAX_L = 128;     // 32 KiB of LDS per workgroup at most
int g_las_form = 0;                      // sn2_debug_las_form: 0 = by L, 1 = the direct form for every L

// bytes s .. s + 3 of the eight bytes hi:lo (v_alignbyte_b32 on the device)
__host__ __device__ __forceinline__ uint32_t las_alignbyte(uint32_t hi, uint32_t lo, uint32_t s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, s);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * s));
#endif
}

// four bytes at byte offset `off` of the staged block, from the two aligned words around them
struct lds_bytes {
    const uint32_t* w;
    __host__ __device__ __forceinline__ uint32_t u32(int off) const {
        const uint32_t lo = w[off >> 2], hi = w[(off >> 2) + 1];     // the word after the block's last is the slack word
        return las_alignbyte(hi, lo, (uint32_t)(off & 3));
    }
    __host__ __device__ __forceinline__ uint32_t u16(int off) const { return (w[off >> 2] >> ((off & 3) * 8) | ((off & 3) == 3 ? w[(off >> 2) + 1] << 8 : 0u)) & 0xFFFFu; }
    __host__ __device__ __forceinline__ uint32_t u8(int off) const { return (w[off >> 2] >> ((off & 3) * 8)) & 0xFFu; }
};

// the same reads from global memory, byte by byte: never a byte outside the field
struct global_bytes {
    const uint8_t* p;
    __host__ __device__ __forceinline__ uint32_t u8(size_t off) const { return p[off]; }
    __host__ __device__ __forceinline__ uint32_t u16(size_t off) const { return u8(off) | (u8(off + 1) << 8); }
    __host__ __device__ __forceinline__ uint32_t u32(size_t off) const { return u16(off) | (u16(off + 2) << 16); }
};

// record at byte `r` of `src` -> column `col` of the ten rows (and of classification).  (Host-callable: a stand-alone host program
// can run the field extraction under a sanitizer.)
template <class Bytes, class Off>
__host__ __device__ __forceinline__ void las_emit(const Bytes& src, Off r, int format, const las_xform& xf, float* __restrict__ out,
                                         size_t row_stride, size_t col, uint8_t* __restrict__ classification) {
    const int32_t X = (int32_t)src.u32(r + LAS_OFF_X), Y = (int32_t)src.u32(r + LAS_OFF_Y), Z = (int32_t)src.u32(r + LAS_OFF_Z);
    const uint32_t iw = src.u32(r + LAS_OFF_INTENSITY);               // intensity, byte 14, byte 15
    const bool ext = las_extended(format);
    const uint32_t b14 = (iw >> 16) & 0xFFu;
    const int rgb = las_rgb_offset(format), nir = las_nir_offset(format);
    float red = 0.f, green = 0.f, blue = 0.f, infra = 0.f;
    if (rgb >= 0) {
        const uint32_t rg = src.u32(r + rgb);
        red = (float)(rg & 0xFFFFu);
        green = (float)(rg >> 16);
        blue = (float)src.u16(r + rgb + 4);
    }
    if (nir >= 0) infra = (float)src.u16(r + nir);
    float x, y, z;
    if (xf.mode == SN2_LAS_COORDS_HEADER) {
        x = las_coord_header(X, xf.scale[0], xf.offset[0], xf.origin[0]);
        y = las_coord_header(Y, xf.scale[1], xf.offset[1], xf.origin[1]);
        z = las_coord_header(Z, xf.scale[2], xf.offset[2], xf.origin[2]);
    } else {
        x = las_coord_reference(X, xf.raw0[0]);
        y = las_coord_reference(Y, xf.raw0[1]);
        z = las_coord_reference(Z, xf.raw0[2]);
    }
    float* o = out + col;
    o[0 * row_stride] = x;
    o[1 * row_stride] = y;
    o[2 * row_stride] = z;
    o[3 * row_stride] = red;
    o[4 * row_stride] = green;
    o[5 * row_stride] = blue;
    o[6 * row_stride] = infra;
    o[7 * row_stride] = (float)(iw & 0xFFFFu);
    o[8 * row_stride] = (float)las_return_num(b14, ext);
    o[9 * row_stride] = (float)las_num_returns(b14, ext);
    if (classification) classification[col] = (uint8_t)(ext ? src.u8(r + 16) : (iw >> 24));
}

__global__ __launch_bounds__(LAS_WG) void las_decode_staged_kernel(const uint8_t* __restrict__ records, int format, int L, long T,
                                                                   las_xform xf, float* __restrict__ out, size_t row_stride,
                                                                   size_t col0, uint8_t* __restrict__ classification) {
    extern __shared__ uint4 las_lds[];                                 // cdiv(256 L, 16) slots and one of slack
    const long first = (long)blockIdx.x * LAS_WG;
    const int n = (int)(T - first < LAS_WG ? T - first : LAS_WG);      // records of this workgroup, >= 1
    const int bytes = n * L;                                           // <= 32 768
    const uint8_t* base = records + (size_t)first * (size_t)L;         // 16-byte aligned: first L is a multiple of 256
    const int full = bytes >> 4, tail = bytes & 15;
    for (int c = threadIdx.x; c < full; c += LAS_WG) las_lds[c] = reinterpret_cast<const uint4*>(base)[c];
    if (tail && threadIdx.x < 16) {                                    // the last workgroup only: the block's own bytes, no further
        uint8_t* l8 = reinterpret_cast<uint8_t*>(las_lds + full);
        l8[threadIdx.x] = (int)threadIdx.x < tail ? base[(size_t)full * 16 + threadIdx.x] : (uint8_t)0;
    }
    __syncthreads();
    if ((int)threadIdx.x >= n) return;
    const lds_bytes src{reinterpret_cast<const uint32_t*>(las_lds)};
    las_emit(src, (int)threadIdx.x * L, format, xf, out, row_stride, col0 + (size_t)first + threadIdx.x, classification);
}

__global__ __launch_bounds__(LAS_WG) void las_decode_direct_kernel(const uint8_t* __restrict__ records, int format, int L, long T,
                                                                   las_xform xf, float* __restrict__ out, size_t row_stride,
                                                                   size_t col0, uint8_t* __restrict__ classification) {
    const long i = (long)blockIdx.x * LAS_WG + threadIdx.x;
    if (i >= T) return;
    const global_bytes src{records};
    las_emit(src, (size_t)i * (size_t)L, format, xf, out, row_stride, col0 + (size_t)i, classification);
}
}  // namespace

extern "C" int sn2_las_record_min_length(int format) {
    if (las_format_is_laz(format) || !las_format_known(format)) return SN2_EINVAL;
    return las_min_length(format);
}

extern "C" int sn2_debug_las_form(int form) {
    if (form != 0 && form != 1) return SN2_EINVAL;
    g_las_form = form;
    return 0;
}

extern "C" int sn2_las_decode(const void* records, size_t n_bytes, int format, int L, long T, int mode, const double* xform,
                              const long long* raw0, float* out, long row_stride, long col0, unsigned char* classification,
                              void* stream) {
    if (!records || !out || T <= 0) return SN2_EINVAL;
    if (las_format_is_laz(format) || !las_format_known(format)) return SN2_EINVAL;
    if (L < las_min_length(format) || L > 65535) return SN2_EINVAL;
    if (T >= (1L << 31)) return SN2_ELIMIT;
    if (n_bytes / (size_t)L < (size_t)T) return SN2_EINVAL;            // n_bytes < T L, without the product
    if ((uintptr_t)records % 16 != 0) return SN2_EINVAL;
    if (col0 < 0 || row_stride <= 0 || col0 > row_stride - T) return SN2_EINVAL;
    las_xform xf = {};
    xf.mode = mode;
    if (mode == SN2_LAS_COORDS_REFERENCE) {
        for (int a = 0; a < 3; ++a) {
            xf.raw0[a] = raw0 ? raw0[a] : 0;
            if (xf.raw0[a] > (1LL << 52) || xf.raw0[a] < -(1LL << 52)) return SN2_EINVAL;
        }
    } else if (mode == SN2_LAS_COORDS_HEADER) {
        if (!xform) return SN2_EINVAL;
        for (int a = 0; a < 3; ++a) {
            xf.scale[a] = xform[a];
            xf.offset[a] = xform[3 + a];
            xf.origin[a] = xform[6 + a];
        }
    } else {
        return SN2_EINVAL;
    }
    const int grid = sn2_cdiv(T, LAS_WG);
    if (L <= LAS_STAGE_MAX_L && g_las_form == 0) {
        const size_t lds = ((size_t)LAS_WG * L + 15) / 16 * 16 + 16;
        hipLaunchKernelGGL(las_decode_staged_kernel, dim3(grid), dim3(LAS_WG), lds, (hipStream_t)stream, (const uint8_t*)records,
                           format, L, T, xf, out, (size_t)row_stride, (size_t)col0, classification);
    } else {
        hipLaunchKernelGGL(las_decode_direct_kernel, dim3(grid), dim3(LAS_WG), 0, (hipStream_t)stream, (const uint8_t*)records,
                           format, L, T, xf, out, (size_t)row_stride, (size_t)col0, classification);
    }
    SN2_RETURN_LAUNCH();
}
