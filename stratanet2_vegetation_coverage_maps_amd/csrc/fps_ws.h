// fps_ws.h -- the workspace that sn2_fps leaves behind (include/strata_hip.h: SN2_FPS_WS_WORDS): the Morton cell grid its points
// are sorted into and the parts the workspace is carved into.  geometry.hip fills it; ball_query.hip reads the sorted tables and
// the grid header through fps_ws_tables -- this header is all that the ball query knows of FPS.
#pragma once
#include "common.h"

// 16 x 16 x 16 cells over the plot's bounding box, full 3-D Morton order.  (Measured on the synthetic plots: 19.6 of 512
// buckets change per FPS round on average, against 27.7 for a 32 x 32 x 8 grid whose two top levels split x,y only.)
constexpr int ORDER_GX = 16, ORDER_GZ = 16, ORDER_CELLS = ORDER_GX * ORDER_GX * ORDER_GZ;

__device__ __forceinline__ unsigned morton_cell(unsigned cx, unsigned cy, unsigned cz) {
    unsigned c = 0;
#pragma unroll
    for (int bit = 3; bit >= 0; --bit) c = (c << 3) | (((cx >> bit) & 1u) << 2) | (((cy >> bit) & 1u) << 1) | ((cz >> bit) & 1u);
    return c;
}

// grid header per plot (32-bit words): [0..4096] first sorted position of every Morton cell (+ end), then lo.xyz, scale.xyz
constexpr int GRID_WORDS = SN2_FPS_WS_GRID_WORDS;
static_assert(GRID_WORDS == ORDER_CELLS + 1 + 6 + 1, "cell starts (+ end), lo.xyz, scale.xyz, padded to an even count");
// exchange area of the multi-workgroup FPS (fps_cluster_kernel): per plot FPS_XCHG_WORDS words of tagged granules, then
// FPS_CTL_WORDS control words per launch (ticket counter, timeout count).  Zeroed HERE, by the kernel in front of every FPS
// launch (a kernel boundary: visible to every workgroup behind it; the tags count super-rounds from 1, so 0 = nothing yet).
constexpr int FPS_XCHG_WORDS = SN2_FPS_WS_XCHG_WORDS, FPS_CTL_WORDS = SN2_FPS_WS_CTL_WORDS;
// the Morton cell of a point (lo, sc: as the grid header keeps them)
__device__ __forceinline__ unsigned order_cell(const float (&lo)[3], const float (&sc)[3], float x, float y, float z) {
    int cx = (int)((x - lo[0]) * sc[0]), cy = (int)((y - lo[1]) * sc[1]), cz = (int)((z - lo[2]) * sc[2]);
    cx = cx < 0 ? 0 : (cx > ORDER_GX - 1 ? ORDER_GX - 1 : cx);
    cy = cy < 0 ? 0 : (cy > ORDER_GX - 1 ? ORDER_GX - 1 : cy);
    cz = cz < 0 ? 0 : (cz > ORDER_GZ - 1 ? ORDER_GZ - 1 : cz);
    return morton_cell((unsigned)cx, (unsigned)cy, (unsigned)cz);
}

// the parts of the workspace (include/strata_hip.h: SN2_FPS_WS_WORDS)
struct fps_ws_parts {
    int* order;          // B*N ints
    float4* sorted;      // B*N float4 (16-byte aligned: B*N*4 bytes offset from a 16-byte aligned base with B*N % 4 == 0)
    int* grid;           // B*GRID_WORDS ints
    unsigned* xchg;      // B*FPS_XCHG_WORDS + FPS_CTL_WORDS
    unsigned* ctl;
    int* rank;           // B*N ints: the inverse of `order` (the last words of the workspace)
};
static fps_ws_parts fps_ws_carve(int* ws, int B, int N) {
    int* grid = ws + SN2_FPS_WS_GRID_OFFSET(B, N);
    return {ws, reinterpret_cast<float4*>(ws + (size_t)B * N), grid, reinterpret_cast<unsigned*>(grid + (size_t)B * GRID_WORDS),
            reinterpret_cast<unsigned*>(ws + SN2_FPS_WS_CTL_OFFSET(B, N)), ws + SN2_FPS_WS_RANK_OFFSET(B, N)};
}
// ... and the tables a reader of a filled workspace takes (sn2_ball_query)
struct fps_ws_tables {
    const int* order;
    const float4* sorted;
    const int* grid;
};
static fps_ws_tables fps_ws_carve(const int* ws, int B, int N) {
    return {ws, reinterpret_cast<const float4*>(ws + (size_t)B * N), ws + SN2_FPS_WS_GRID_OFFSET(B, N)};
}
