// las_rules.h -- the record layout and the arithmetic of the LAS decoder (include/strata_hip.h, "LAS point records"), stated
// once.  The kernels of las.hip and the host-side checks of sn2_las_decode / sn2_las_record_min_length execute these functions.
// The layout is OURS: a reading of the ASPRS LAS 1.0-1.4 specification (the reference reads its files through laspy 1.x, which
// cannot be run beside this library), pinned by records typed out by hand in tests/test_las_host.py.  The coordinate arithmetic
// of the `reference` mode is load_las_file's (utils/load_data.py:149-184).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LAS_FN __host__ __device__ __forceinline__
#else
#define LAS_FN static inline
#endif

constexpr int LAS_MAX_FORMAT = 10;
constexpr int LAS_ROWS = 10;      // x, y, z, red, green, blue, nir, intensity, return_num, num_returns

// bits 7 and 6 of the header's format byte mark a compressed (LAZ) file
LAS_FN bool las_format_is_laz(int format) { return (format & 0xC0) != 0; }
LAS_FN bool las_format_known(int format) { return format >= 0 && format <= LAS_MAX_FORMAT; }

// the least record length of a format; 0 for a format outside 0..10.  The waveform formats 4 / 5 / 9 / 10 lead with the fields
// of 1 / 3 / 6 / 8 and end with 29 bytes of waveform packet.
LAS_FN int las_min_length(int format) {
    switch (format) {
        case 0: return 20;
        case 1: return 28;
        case 2: return 26;
        case 3: return 34;
        case 4: return 57;
        case 5: return 63;
        case 6: return 30;
        case 7: return 36;
        case 8: return 38;
        case 9: return 59;
        case 10: return 67;
        default: return 0;
    }
}

// formats 6-10: the 4-bit return fields, classification at byte 16
LAS_FN bool las_extended(int format) { return format >= 6; }

// fixed fields of every format
constexpr int LAS_OFF_X = 0, LAS_OFF_Y = 4, LAS_OFF_Z = 8, LAS_OFF_INTENSITY = 12, LAS_OFF_RETURNS = 14;
LAS_FN int las_class_offset(int format) { return las_extended(format) ? 16 : 15; }
// byte offset of red (green, blue follow, uint16 each); -1: the format has no colour
LAS_FN int las_rgb_offset(int format) {
    switch (format) {
        case 2: return 20;
        case 3: case 5: return 28;
        case 7: case 8: case 10: return 30;
        default: return -1;
    }
}
// byte offset of the near infrared (uint16); -1: none
LAS_FN int las_nir_offset(int format) { return (format == 8 || format == 10) ? 36 : -1; }

// byte 14: return number and number of returns
LAS_FN unsigned las_return_num(unsigned b14, bool extended) { return extended ? (b14 & 15u) : (b14 & 7u); }
LAS_FN unsigned las_num_returns(unsigned b14, bool extended) { return extended ? ((b14 >> 4) & 15u) : ((b14 >> 3) & 7u); }

// `reference` coordinates: load_las_file's X / 100 on the raw integer (numpy: int32 / int -> a correctly rounded fp64 quotient),
// then the cast to fp32.  raw0 is subtracted as an integer first (0 = the reference).  |X - raw0| < 2^53: the conversion is exact.
LAS_FN float las_coord_reference(int32_t X, long long raw0) {
    const double d = (double)((long long)X - raw0);
    return (float)(d / 100.0);
}

// `header` coordinates: (X * scale + offset) - origin, every operation rounded to fp64 on its own, then the cast to fp32
LAS_FN float las_coord_header(int32_t X, double scale, double offset, double origin) {
#pragma clang fp contract(off)
    const double p = (double)X * scale;
    const double q = p + offset;
    const double r = q - origin;
    return (float)r;
}

// the coordinate transform of one launch, by value in the kernel's arguments
struct las_xform {
    int mode;              // SN2_LAS_COORDS_*
    long long raw0[3];     // reference: X0, Y0, Z0
    double scale[3], offset[3], origin[3];   // header
};
