// atlas.hip -- the mosaics of K parcels in one arena (a "mosaic atlas"): merge, finalisation and crop + band statistics of many
// canvases per launch.  A shapefile of small parcels gives canvases of a few thousand pixels each; one canvas per launch leaves
// the chip idle and pays the launch floor K times.  Here a workgroup finds its canvas (or its run of plots) from a prefix table
// of workgroups by a wave-uniform binary search -- scalar loads, no divergence -- and then executes the per-pixel rules of
// mosaic_rules.h, the very functions the single-canvas kernels of project.hip execute: canvas k of the atlas gets the bytes the
// single-canvas call leaves on its view.  The layouts and contracts are written out in include/strata_hip.h.
#include <cmath>
#include <cstring>

#include "atlas_table.h"
#include "common.h"
#include "mosaic_rules.h"

namespace {
constexpr int COLS = ATLAS_COLS;
constexpr int SEG = SN2_ATLAS_SEG_COLS;
constexpr int FIN_WORDS = SN2_ATLAS_FINALIZE_CANVAS_WORDS;

// ---- merge: grid (workgroups of all runs, 3 bands); a workgroup owns a 4 x 64 pixel tile of its run's window ----------------
__global__ __launch_bounds__(256) void atlas_merge_kernel(const float* __restrict__ rasters, const float* __restrict__ weights,
                                                          const int* __restrict__ place, int D, const long long* __restrict__ canvas,
                                                          const int* __restrict__ seg, int S, float* __restrict__ mean,
                                                          float* __restrict__ wsum) {
    const int s = last_row_at_or_below(seg, SEG, 7, S, (long long)blockIdx.x);
    const int* g = seg + (size_t)s * SEG;
    const int k = g[0], b0 = g[1], b1 = g[2], y0 = g[3], x0 = g[4], wh = g[5], ww = g[6];
    const int local = (int)blockIdx.x - g[7];
    const int tiles_x = (ww + 63) / 64;
    const int ty = local / tiles_x, tx = local - ty * tiles_x;
    const int wx = tx * 64 + (threadIdx.x & 63), wy = ty * 4 + (threadIdx.x >> 6);
    if (wx >= ww || wy >= wh) return;
    const long long* cv = canvas + (size_t)k * COLS;
    const int H = (int)cv[1], W = (int)cv[2];
    const int gy = y0 + wy, gx = x0 + wx;
    if (gy < 0 || gy >= H || gx < 0 || gx >= W) return;
    const size_t base3 = 3 * (size_t)cv[0];
    // place + 1: (row, col) of plot b at stride 3
    mosaic_fold_pixel(rasters, weights, place + 1, 3, b0, b1, D, (int)blockIdx.y, H, W, gy, gx, mean + base3, wsum + base3);
}

// ---- finalisation ---------------------------------------------------------------------------------------------------------
// ws of canvas k: FIN_WORDS words at ws + k FIN_WORDS = the histogram (SN2_MOSAIC_HIST_WORDS ints, [HARD_STEPS+1] the number of
// valid pixels), then one fp64 partial sum per workgroup of the canvas
__global__ __launch_bounds__(256) void atlas_hist_kernel(const float* __restrict__ mean, const long long* __restrict__ canvas, int K,
                                                         int* __restrict__ ws) {
    const int k = last_row_at_or_below(canvas, COLS, 3, K, (long long)blockIdx.x);
    const long long* cv = canvas + (size_t)k * COLS;
    const long P = (long)cv[1] * (long)cv[2];
    const int j = (int)((long long)blockIdx.x - cv[3]), nblk = (int)(cv[COLS + 3] - cv[3]);
    int* hist = ws + (size_t)k * FIN_WORDS;
    double* partial = reinterpret_cast<double*>(hist + SN2_MOSAIC_HIST_WORDS);
    double sum;
    int cnt;
    hard_hist_block(mean + 3 * (size_t)cv[0] + P, P, (long)j * 256, (long)nblk * 256, hist, sum, cnt);
    if (threadIdx.x == 0) {
        partial[j] = sum;
        atomicAdd(&hist[HARD_STEPS + 1], cnt);
    }
}

// one workgroup per canvas: the partial sums added in workgroup order by one thread, then the search
__global__ __launch_bounds__(1024) void atlas_threshold_kernel(const int* __restrict__ ws, const long long* __restrict__ canvas,
                                                               float* __restrict__ thr) {
    __shared__ double s_total;
    const int k = blockIdx.x;
    const long long* cv = canvas + (size_t)k * COLS;
    const int nblk = (int)(cv[COLS + 3] - cv[3]);
    const int* hist = ws + (size_t)k * FIN_WORDS;
    if (threadIdx.x == 0) {
        const double* partial = reinterpret_cast<const double*>(hist + SN2_MOSAIC_HIST_WORDS);
        double t = 0.0;
        for (int j = 0; j < nblk; ++j) t += partial[j];
        s_total = t;
    }
    __syncthreads();
    hard_threshold_search(hist, hist[HARD_STEPS + 1], s_total, thr + 2 * (size_t)k);
}

__global__ __launch_bounds__(256) void atlas_finalize_kernel(const float* __restrict__ mean, const float* __restrict__ wsum,
                                                             const long long* __restrict__ canvas, int K,
                                                             const float* __restrict__ thr, float* __restrict__ bands) {
    const int k = last_row_at_or_below(canvas, COLS, 3, K, (long long)blockIdx.x);
    const long long* cv = canvas + (size_t)k * COLS;
    const long P = (long)cv[1] * (long)cv[2];
    const int j = (int)((long long)blockIdx.x - cv[3]), nblk = (int)(cv[COLS + 3] - cv[3]);
    const size_t base = (size_t)cv[0];
    const double t = hard_lin((int)thr[2 * (size_t)k + 1]);
    for (long i = (long)j * 256 + threadIdx.x; i < P; i += (long)nblk * 256)
        mosaic_finalize_pixel(mean + 3 * base, wsum + 3 * base, P, i, t, bands + 5 * base);
}

// ---- crop and band statistics ---------------------------------------------------------------------------------------------
// psum (total workgroups, C) fp64, then pcnt (total workgroups, C) int64: canvas k's rows start at its workgroup prefix
__global__ __launch_bounds__(CROP_T) void atlas_crop_kernel(float* __restrict__ bands, int C, const long long* __restrict__ canvas,
                                                            int K, double pix, const double* __restrict__ edges,
                                                            const int* __restrict__ edge_start, double* __restrict__ psum,
                                                            long long* __restrict__ pcnt) {
    __shared__ CropLds s;
    const int k = last_row_at_or_below(canvas, COLS, 4, K, (long long)blockIdx.x);
    const long long* cv = canvas + (size_t)k * COLS;
    const int H = (int)cv[1], W = (int)cv[2];
    const int j = (int)((long long)blockIdx.x - cv[4]), nblk = (int)(cv[COLS + 4] - cv[4]);
    const double x_min = __longlong_as_double(cv[5]), y_max = __longlong_as_double(cv[6]);
    const int e0 = edge_start[k], E = edge_start[k + 1] - e0;
    float* b = bands + (size_t)C * (size_t)cv[0];
    double* ps = psum + (size_t)blockIdx.x * C;
    long long* pc = pcnt + (size_t)blockIdx.x * C;
    if (E > 0) mosaic_crop_block<true>(s, b, C, H, W, x_min, y_max, pix, edges + 4 * (size_t)e0, E, j, nblk, ps, pc);
    else mosaic_crop_block<false>(s, b, C, H, W, x_min, y_max, pix, edges, 0, j, nblk, ps, pc);
}

__global__ __launch_bounds__(CROP_T) void atlas_crop_fold_kernel(const double* __restrict__ psum, const long long* __restrict__ pcnt,
                                                                 int C, const long long* __restrict__ canvas,
                                                                 double* __restrict__ mean, long long* __restrict__ count) {
    const int k = blockIdx.x;
    const long long* cv = canvas + (size_t)k * COLS;
    const size_t first = (size_t)cv[4] * C;
    mosaic_crop_fold(psum + first, pcnt + first, C, (int)(cv[COLS + 4] - cv[4]), mean + (size_t)k * C, count + (size_t)k * C);
}

}  // namespace

extern "C" int sn2_atlas_canvas_table(int K, const int* H, const int* W, const double* x_min, const double* y_max, long long* table) {
    if (!H || !W || !table || K <= 0 || (x_min == nullptr) != (y_max == nullptr)) return SN2_EINVAL;
    std::memset(table, 0, sizeof(long long) * COLS * ((size_t)K + 1));
    for (int k = 0; k < K; ++k) {
        long long* r = table + (size_t)k * COLS;
        long long row[2 * COLS] = {0};
        const int rc = atlas_canvas_row(H[k], W[k], x_min ? x_min[k] : 0.0, y_max ? y_max[k] : 0.0, r, row);
        if (rc) return rc;
        std::memcpy(r, row, sizeof(long long) * COLS);
        r[COLS + 0] = row[COLS + 0];
        r[COLS + 3] = row[COLS + 3];
        r[COLS + 4] = row[COLS + 4];
        if (r[COLS + 3] > 0x7fffffffLL || r[COLS + 4] > 0x7fffffffLL) return SN2_ELIMIT;
    }
    return 0;
}

extern "C" int sn2_atlas_finalize_ws_words(int K, size_t* words) {
    if (!words || K <= 0) return SN2_EINVAL;
    *words = SN2_ATLAS_FINALIZE_WS_WORDS(K);
    return 0;
}

extern "C" int sn2_atlas_merge(const float* rasters, const float* weights, const int* place, int B, int D, int K,
                               const long long* canvas_host, const long long* canvas_dev, const int* seg_host, const int* seg_dev,
                               int S, float* mean, float* wsum, void* stream) {
    if (!rasters || !weights || !place || !canvas_host || !canvas_dev || !seg_host || !seg_dev || !mean || !wsum) return SN2_EINVAL;
    if (B <= 0 || D <= 0 || K <= 0 || S <= 0 || S > B) return SN2_EINVAL;
    const int rc = atlas_check_table(K, canvas_host);
    if (rc) return rc;
    // the runs: canvases ascending, plots [0, B) cut in order, every window inside its canvas, the workgroup prefix as stated
    long long wg = 0;
    int prev_canvas = -1, next_plot = 0;
    for (int s = 0; s < S; ++s) {
        const int* g = seg_host + (size_t)s * SEG;
        if (g[0] <= prev_canvas || g[0] >= K || g[1] != next_plot || g[2] <= g[1] || g[2] > B) return SN2_EINVAL;
        const long long* cv = canvas_host + (size_t)g[0] * COLS;
        if (g[3] < 0 || g[4] < 0 || g[5] < 0 || g[6] < 0 || (long long)g[3] + g[5] > cv[1] || (long long)g[4] + g[6] > cv[2]) return SN2_EINVAL;
        if (g[7] != wg) return SN2_EINVAL;
        wg += (g[5] > 0 && g[6] > 0) ? (long long)sn2_cdiv(g[6], 64) * sn2_cdiv(g[5], 4) : 0;
        if (wg > 0x7fffffffLL) return SN2_ELIMIT;
        prev_canvas = g[0];
        next_plot = g[2];
    }
    if (next_plot != B || seg_host[(size_t)S * SEG + 7] != wg) return SN2_EINVAL;
    if (wg == 0) return 0;                                                      // every window lies outside its canvas
    hipLaunchKernelGGL(atlas_merge_kernel, dim3((unsigned)wg, 3), dim3(256), 0, (hipStream_t)stream, rasters, weights, place, D,
                       canvas_dev, seg_dev, S, mean, wsum);
    SN2_RETURN_LAUNCH();
}

extern "C" int sn2_atlas_finalize(const float* mean, const float* wsum, int K, const long long* canvas_host,
                                  const long long* canvas_dev, void* ws, float* thr, float* bands, void* stream) {
    if (!mean || !wsum || !canvas_host || !canvas_dev || !ws || !thr || !bands || K <= 0) return SN2_EINVAL;
    if (((uintptr_t)ws & 7) != 0) return SN2_EINVAL;
    const int rc = atlas_check_table(K, canvas_host);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)canvas_host[(size_t)K * COLS + 3];
    sn2_fill_words(ws, 0u, SN2_ATLAS_FINALIZE_WS_WORDS(K), st);
    hipLaunchKernelGGL(atlas_hist_kernel, dim3(grid), dim3(256), 0, st, mean, canvas_dev, K, (int*)ws);
    hipLaunchKernelGGL(atlas_threshold_kernel, dim3(K), dim3(1024), 0, st, (const int*)ws, canvas_dev, thr);
    hipLaunchKernelGGL(atlas_finalize_kernel, dim3(grid), dim3(256), 0, st, mean, wsum, canvas_dev, K, (const float*)thr, bands);
    SN2_RETURN_LAUNCH();
}

extern "C" int sn2_atlas_crop_stats(float* bands, int C, int K, const long long* canvas_host, const long long* canvas_dev, double pix,
                                    const double* edges, const int* edge_start_host, const int* edge_start_dev, void* ws,
                                    double* mean, long long* count, void* stream) {
    if (!bands || !canvas_host || !canvas_dev || !edge_start_host || !edge_start_dev || !ws || !mean || !count || C < 1 || K <= 0)
        return SN2_EINVAL;
    if (!(pix > 0.0) || !std::isfinite(pix)) return SN2_EINVAL;
    if (((uintptr_t)ws & 7) != 0) return SN2_EINVAL;
    if (edge_start_host[0] != 0) return SN2_EINVAL;
    bool limit = C > SN2_MOSAIC_CROP_MAX_BANDS;
    for (int k = 0; k < K; ++k) {
        const long long E = (long long)edge_start_host[k + 1] - edge_start_host[k];
        if (E < 0 || (E > 0 && E < 3)) return SN2_EINVAL;                          // a ring has three edges or more
        limit = limit || E > SN2_MOSAIC_CROP_MAX_EDGES;
    }
    if ((edge_start_host[K] == 0) != (edges == nullptr)) return SN2_EINVAL;
    const int rc = atlas_check_table(K, canvas_host);
    if (rc) return rc;
    if (limit) return SN2_ELIMIT;
    hipStream_t st = (hipStream_t)stream;
    const size_t nblk = (size_t)canvas_host[(size_t)K * COLS + 4];
    double* psum = (double*)ws;
    long long* pcnt = (long long*)(psum + nblk * C);
    hipLaunchKernelGGL(atlas_crop_kernel, dim3((unsigned)nblk), dim3(CROP_T), 0, st, bands, C, canvas_dev, K, pix, edges, edge_start_dev,
                       psum, pcnt);
    hipLaunchKernelGGL(atlas_crop_fold_kernel, dim3(K), dim3(CROP_T), 0, st, (const double*)psum, (const long long*)pcnt, C, canvas_dev,
                       mean, count);
    SN2_RETURN_LAUNCH();
}
