// cut_rules.h -- the rule that cuts the points of a LAS tile into parcel clouds, stated once: the even-odd crossing of one edge,
// the fp64 distance of a point to one edge, the test of a point against all edges of a parcel, the cell of a position in the
// candidate grid and the wave step of the count / fill passes.  Host side: parcel.polygon_keep states the same rule in numpy, and
// the kernels of cut.hip give its boolean bit for bit (the rule is written out in include/strata_hip.h, "Parcel cut").
// Every product, difference, quotient and sum of the rule is rounded to fp64 on its own, in polygon_keep's association: no fused
// multiply-add.
#pragma once
#include "common.h"

#include <limits.h>

constexpr long CUT_MAX_CELLS = SN2_CUT_MAX_CELLS;      // cells of the candidate grid
constexpr long CUT_MAX_ITEMS = SN2_CUT_MAX_ITEMS;      // entries of all cell lists
constexpr long CUT_MAX_EDGES = 1L << 26;      // edges of all parcels
constexpr double CUT_MAX_COORD = 1e100;       // |edge coordinate|: no product of the rule overflows

// does the edge (ax, ay) -> (bx, by) cross the ray from (px, py) towards +x?  The quotient only where the edge crosses the
// point's row (the expression of mosaic_crop_block)
__device__ __forceinline__ bool cut_crosses_right(double px, double py, double ax, double ay, double bx, double by) {
#pragma clang fp contract(off)
    if ((ay > py) != (by > py)) return px < ax + ((py - ay) * (bx - ax)) / (by - ay);
    return false;
}

// is the point nearer than sqrt(b2) to the edge?  t: the foot's parameter, clamped to the segment; a repeated vertex (l2 == 0) is
// a point
__device__ __forceinline__ bool cut_near(double px, double py, double ax, double ay, double bx, double by, double b2) {
#pragma clang fp contract(off)
    const double dx = bx - ax, dy = by - ay;
    const double l2 = dx * dx + dy * dy;
    double t = l2 > 0.0 ? ((px - ax) * dx + (py - ay) * dy) / l2 : 0.0;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    const double ex = (ax + t * dx) - px, ey = (ay + t * dy) - py;
    return ex * ex + ey * ey < b2;
}

// Does the parcel with the edges [e0, e1) of `edges` (E,4) keep the point?  Called by the whole wave with e0, e1 uniform, so the
// edge addresses are uniform too; `on`: the lanes whose point is asked about.  A lane leaves the loop's work at its first edge
// within the buffer (the answer is an OR), the wave leaves the loop when no lane is left.
__device__ __forceinline__ bool cut_keeps(const double* __restrict__ edges, int e0, int e1, double px, double py, double b2, bool on) {
    bool open = on;                                       // no edge within the buffer yet
    int right = 0;
    for (int e = e0; e < e1; ++e) {
        if (__ballot(open) == 0ull) break;
        const double ax = edges[4 * (size_t)e], ay = edges[4 * (size_t)e + 1];
        const double bx = edges[4 * (size_t)e + 2], by = edges[4 * (size_t)e + 3];
        if (open) {
            right += cut_crosses_right(px, py, ax, ay, bx, by) ? 1 : 0;
            open = !cut_near(px, py, ax, ay, bx, by, b2);
        }
    }
    return on && (!open || (right & 1) != 0);
}

// ---- the candidate grid: CSR over GX x GY square cells, parcel ids ascending inside a cell ------------------------------------
struct CutGrid {
    const int* start;        // (GX*GY+1)
    const int* items;        // parcel ids
    int GX, GY;
    double x0, y0, inv;      // cell of a coordinate: floor((v - x0) * inv), the expression the host lists the parcels with
};

// the cell of a position, -1 outside the grid; a NaN or infinite coordinate fails every comparison and has no cell
__device__ __forceinline__ int cut_cell(const CutGrid& g, double px, double py) {
#pragma clang fp contract(off)
    const double fx = floor((px - g.x0) * g.inv), fy = floor((py - g.y0) * g.inv);
    if (fx >= 0.0 && fx < (double)g.GX && fy >= 0.0 && fy < (double)g.GY) return (int)fy * g.GX + (int)fx;
    return -1;
}

struct CutDrop { unsigned w[8]; };           // the 256 classes: bit c set = a point of class c belongs to no parcel

// The wave step of the count and fill passes (the shape of parcel_wave_step): one wave walks the points [i0, i1) of the cloud
// (a row), 64 at a time.  Each lane holds the candidate list of its point's cell; the wave visits the parcels in ascending id --
// the minimum over the lanes' next candidates -- and the lanes that have parcel m as their candidate run m's edges together.
// cloud: (10,T) channel-major; cls: the points' class bytes or NULL; table: (parcel, row) entries, parcel-major, `rows` per parcel.
// count pass (FILL = false): table[m*rows + row] += points of the row that parcel m keeps.
// fill pass (FILL = true): table holds the exclusive starts; every hit of a parcel with parcel_base[m] != INT_MIN goes to slot
// parcel_base[m] + cursor + rank: rank orders the wave's hits in m by lane (= index), the cursor -- advanced by the row's own wave
// only -- orders its 64-point steps.  So a parcel's points are in ascending tile index.  All arguments wave-uniform.
template <bool FILL>
__device__ __forceinline__ void cut_wave_step(const float* __restrict__ cloud, long T, const unsigned char* __restrict__ cls,
                                              const CutDrop& drop, long i0, long i1, const CutGrid& g,
                                              const int* __restrict__ edge_start, const double* __restrict__ edges, double b2,
                                              int* __restrict__ table, int rows, int row, const int* __restrict__ parcel_base,
                                              long sum_n, float* __restrict__ out, int* __restrict__ pidx) {
    const int lane = threadIdx.x & 63;
    for (long b = i0; b < i1; b += 64) {
        const long i = b + lane;
        double px = 0.0, py = 0.0;
        int pos = 0, end = 0;                             // this lane's candidates: items[pos .. end)
        if (i < i1) {
            bool live = true;
            if (cls) {
                const unsigned c = cls[i];
                live = ((drop.w[c >> 5] >> (c & 31u)) & 1u) == 0u;
            }
            if (live) {
                px = (double)cloud[i];
                py = (double)cloud[T + i];
                const int c = cut_cell(g, px, py);
                if (c >= 0) {
                    pos = g.start[c];
                    end = g.start[c + 1];
                }
            }
        }
        int q = pos < end ? g.items[pos] : INT_MAX;
        while (true) {
            int m = q;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const int v = __shfl_xor(m, o);
                m = v < m ? v : m;
            }
            m = __builtin_amdgcn_readfirstlane(m);
            if (m == INT_MAX) break;
            const bool mine = q == m;
            const bool hit = cut_keeps(edges, edge_start[m], edge_start[m + 1], px, py, b2, mine);
            const unsigned long long mask = __ballot(hit);
            if (mask != 0ull) {
                const int leader = __ffsll((long long)mask) - 1;
                int* cur = &table[(long)m * rows + row];
                if (!FILL) {
                    if (lane == leader) atomicAdd(cur, __popcll(mask));
                } else {
                    const int pb = parcel_base[m];
                    if (pb != INT_MIN) {
                        int c0 = 0;
                        if (lane == leader) c0 = atomicAdd(cur, __popcll(mask));
                        c0 = __shfl(c0, leader);
                        if (hit) {
                            const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32),
                                                                       __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                            const long s = (long)pb + c0 + rank;
                            if (s >= 0 && s < sum_n) {    // (holds whenever the cloud is the one the count pass saw)
                                pidx[s] = (int)i;
#pragma unroll
                                for (int c = 0; c < 10; ++c) out[(size_t)c * sum_n + s] = cloud[(size_t)c * T + i];
                            }
                        }
                    }
                }
            }
            if (mine) {
                ++pos;
                q = pos < end ? g.items[pos] : INT_MAX;
            }
        }
    }
}
