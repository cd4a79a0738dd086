/* strata_hip.h -- C ABI of libstrata_hip.so: the MI355X (gfx950) implementation of the PointNet2 hot path of
 * IGNF/StrataNet2-Vegetation-Coverage-Maps.
 *
 * The reference has no FFI: its boundary is the Python API of model/point_net2.py and model/project_to_2d.py,
 * whose arithmetic lives in un-vendored wheels (torch-cluster 1.5.9, torch-geometric 1.7.2, torch-scatter 2.0.7).
 * Each entry point below names the reference call site (file:line under /root/reference) it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (tensor.data_ptr()) unless it points to one of the structs below, which
 *     live in host memory and are only read during the call;
 *   - the caller owns every buffer including workspaces; nothing is allocated, freed or synchronised inside;
 *   - every call is asynchronous on `stream` (a hipStream_t; NULL = default stream);
 *   - fp32 data, int32 indices; indices are LOCAL to their plot (0..N-1) unless stated;
 *   - return value: 0 = ok, >0 = hipError_t of a failed launch, <0 = argument error (SN2_E*), never throws.
 *
 * Layouts
 *   "SoA"   (B,3,N)   x-row, y-row, z-row per plot          (what the reference DataLoader hands over as `xyz`)
 *   "AoS4"  (B*N,4)   x,y,z,0 per point
 *   rows    (R,C)     row-major feature rows
 */
#ifndef STRATA_HIP_H
#define STRATA_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SN2_VERSION 102 /* unchanged by ADDED entry points (sn2_plot_losses): a binding that knows 102 still finds all it asks for */
#define SN2_EINVAL (-1) /* bad size / null pointer             */
#define SN2_ELIMIT (-2) /* size outside what the kernels cover */

#define SN2_MAX_NEIGHBORS 2000 /* model/point_net2.py:24  max_num_neighbors */
#define SN2_STAT_SLOTS 1024    /* workgroups (= partial-sum slots) of a kernel that produces BatchNorm statistics */

int sn2_version(void);
/* diagnostic (tests/test_gpu_bf16.py): D (16,16) = A (16,48) B (48,16) with bfloat16 operands through a K = 32 and a K = 16 MFMA
 * chained on one accumulator -- modes 0..4: csrc/misc.hip, debug_mfma_chain_kernel */
int sn2_debug_mfma_chain(const float *a, const float *b, float *d, int mode, void *stream);
/* diagnostic: `blocks` one-wave workgroups idle for `clocks` shader clocks each (s_sleep loop, bounded); out: NULL or one int */
int sn2_debug_spin(int blocks, long long clocks, int *out, void *stream);

/* measured peaks (bench.py times them with HIP events in the same run as the metric, next to the datasheet figures):
 * sn2_debug_stream_probe: mode 0 = copy dst[i] = src[i] over n_floats floats (2 * 4 * n_floats bytes moved), 1 = read-only sum
 * (4 * n_floats bytes); sink: SN2_PROBE_SINK_WORDS floats of scratch.  sn2_debug_mfma_probe: independent chains of one matrix
 * instruction, 8 workgroups of 4 waves per CU, `iters` rounds -- mode 0 v_mfma_f32_16x16x4_f32, 1 v_mfma_f32_32x32x2_f32,
 * 2 v_mfma_f32_16x16x32_bf16, 3 v_mfma_f32_32x32x16_bf16; *flops (HOST pointer or NULL) = the flops of the launch. */
/* diagnostic (bench.py's roofline record): which kernels of the per-point layer's source-side backward sn2_fp_backward launches --
 * bit 0 the row pass, 1 the source pass, 2 the merge; 7 (default; 0 = back to it) = all, the only setting that yields gradients */
int sn2_debug_fp1_backward_parts(int mask);
/* test hook: which row pass the source-side FORWARD of the per-point layer launches -- 1 (default) the form whose input stream is
 * fetched one element per lane, four iterations ahead (fp_fwd_rows2_kernel, round 5), 0 the first form (every lane of a row loads
 * the row's inputs itself); the two must give the same bits */
int sn2_debug_fp_rows_form(int form);
/* test hook: which kernel builds the source table of the source-side forms -- 1 (default) on the matrix cores (64 rows per wave
 * through an LDS tile, round 5), 0 one row per lane with scalar weights; the fp32 MFMA accumulates k ascending like the fmaf chain */
int sn2_debug_fp_table_form(int form);
#define SN2_PROBE_SINK_WORDS 4096
int sn2_debug_stream_probe(const float *src, float *dst, size_t n_floats, int mode, float *sink, void *stream);
int sn2_debug_mfma_probe(int mode, int iters, float *sink, double *flops, void *stream);

/* ---- one (Linear -> ReLU -> BatchNorm1d) block, model/point_net2.py:45-53 -------------------------------- */
typedef struct sn2_block {
    int cin, cout;
    const float *W, *b;            /* Linear weight (cout,cin) row-major, bias (cout)                            */
    const float *gamma, *beta;     /* BatchNorm affine (cout)                                                   */
    float *running_mean, *running_var; /* (cout) updated in place when training (momentum 0.1, unbiased var)    */
    float *a, *c;                  /* out (cout): the block's output is  a*relu(W u + b) + c                    */
    float *mean, *invstd;          /* out (cout): batch statistics saved for backward (training)                */
    float *stat_slots;             /* workspace, SN2_STAT_SLOTS * 2 * cout floats (per-workgroup batch-statistics
                                      partials; no initialisation needed)                                       */
    float *dW, *db, *dgamma, *dbeta; /* backward outputs, ACCUMULATED; must be ZERO on entry of the backward call
                                        (dgamma/dbeta are read back inside it)                                   */
    int grad_replicas, grad_replica_stride; /* > 1: (dW, db) exist as grad_replicas zeroed images, image r at
                                        + r * grad_replica_stride floats; a workgroup adds into ONE image, so that the
                                        float atomics spread over the memory channels.  The gradient is the sum of the
                                        images (sn2_grad_reduce).  dgamma / dbeta always have one image.  0 or 1: one. */
    int mma_bf16;                  /* != 0: this block's contractions on the matrix cores (forward, input gradient, weight
                                      gradient) take bfloat16 operands (weights and activations rounded to nearest even,
                                      v_mfma_f32_16x16x32_bf16 / 16x16x16, fp32 accumulate); ReLU, BatchNorm, statistics, the
                                      extremum and everything that decides an index stay fp32 (BASELINE.json configs[4]).
                                      0: exact fp32 products (v_mfma_f32_16x16x4_f32), the reference's precision.          */
    long long *num_batches_tracked; /* BatchNorm1d's int64 counter (one element) or NULL: += 1 by the training forward,
                                       inside the statistics finalisation (no launch of its own)                           */
    int frozen_stats;              /* read by the BACKWARD entry points.  != 0: the forward pass ran this BatchNorm on its RUNNING
                                      statistics (a forward with training = SN2_BN_FROZEN_KEEP: model.eval() with gradients
                                      wanted, model/point_net2.py:45-53 under torch's autograd), so mean / invstd are constants of
                                      the backward: d pre-BN = gamma * invstd * dy, without the batch-mean and batch-variance
                                      terms; dgamma / dbeta are the same sums.  0: batch statistics (a training forward).           */
} sn2_block;
/* the `training` argument of sn2_sa_forward / sn2_fp_forward / sn2_net_io.training:
 *   0                   eval: BatchNorm on its running statistics, nothing kept for a backward pass (fewest bytes and launches);
 *   1                   training: batch statistics, running statistics and counters updated, everything kept;
 *   SN2_BN_FROZEN_KEEP  eval WITH a backward to come: running statistics (not updated), and everything a backward pass reads is
 *                       kept exactly as a training forward keeps it (the kernels of a training pass, the finalisation of an eval
 *                       pass); the backward calls must then carry sn2_block.frozen_stats = 1. */
#define SN2_BN_FROZEN_KEEP 2
/* flat[i] += sum_{r=1..replicas-1} flat[r*stride + i], i < n: folds the images of a flat gradient vector into image 0 */
int sn2_grad_reduce(float *flat, int n, int replicas, int stride, void *stream);

/* ---- geometry -------------------------------------------------------------------------------------------- */

/* (cloud (B,C,N), xyz (B,3,N)) -> rows0 (B*N,12) = [cloud rows 2..9 | x y z 0]
 * replaces the long-form/concat glue of PointNet2.forward, model/point_net2.py:107-124 (C must be 10). */
int sn2_pack_rows(const float *cloud, const float *xyz, int B, int C, int N, float *rows0, void *stream);
/* The same for a model that reads F point features (model/point_net2.py:77: n_input_feats = len(args.input_feats) - 2):
 * rows0 (B*N,F+4) = [F features | x y z 0].  (C, F) = (10, 8): cloud rows 2..9, sn2_pack_rows itself;  (6, 4): cloud rows 2..5,
 * the reference's rule for a six-row cloud;  (10, 4): cloud rows 2, 7, 8, 9 -- the reference's ten-row layout with the four
 * colour rows (red, green, blue, nir) never read.  Any other pair: SN2_ELIMIT. */
int sn2_pack_rows_feat(const float *cloud, const float *xyz, int B, int C, int N, int F, float *rows0, void *stream);

/* farthest point sampling -- torch_cluster.fps, model/point_net2.py:22.
 * start (B) local start index per plot or NULL (= 0, i.e. random_start=False).
 * idx (B,M) local indices in selection order; cpos_soa (B,3,M) and cpos_aos (B*M,4) = the selected positions.
 * order_ws: workspace of SN2_FPS_WS_WORDS(B,N) int32 (16-byte aligned, no initialisation: B*N ints of spatial order,
 * B*N float4 of sorted points, B cell-grid headers of 4104 words, B exchange areas of 4096 words for the
 * multi-workgroup kernel, 32 control words, B*N ints = every point's position in the spatial order [the inverse of the
 * first B*N words: what sn2_fp.row_perm takes]) enabling the bucketed kernel (exact same result, several times
 * faster at N = 32768), or NULL for the brute-force kernel.  After the call the workspace describes the sorted point
 * set and can be handed to sn2_ball_query over the same sources. */
#define SN2_FPS_WS_GRID_WORDS 4104 /* cell-grid header of one plot */
#define SN2_FPS_WS_XCHG_WORDS 4096 /* exchange area of one plot     */
#define SN2_FPS_WS_CTL_WORDS 32    /* control words of the workspace: [1] = waits of the LAST pass that gave up */
#define SN2_FPS_WS_GRID_OFFSET(B, N) (5L * (B) * (N))
#define SN2_FPS_WS_CTL_OFFSET(B, N) (SN2_FPS_WS_GRID_OFFSET(B, N) + (long)(SN2_FPS_WS_GRID_WORDS + SN2_FPS_WS_XCHG_WORDS) * (B))
#define SN2_FPS_WS_RANK_OFFSET(B, N) (SN2_FPS_WS_CTL_OFFSET(B, N) + SN2_FPS_WS_CTL_WORDS)
#define SN2_FPS_WS_WORDS(B, N) (SN2_FPS_WS_RANK_OFFSET(B, N) + 1L * (B) * (N))
size_t sn2_fps_ws_words(int B, int N);       /* = the macro of the same name, as every size_t sn2_*_words below: for hosts without a C compiler */
size_t sn2_fps_ws_grid_offset(int B, int N);
size_t sn2_fps_ws_ctl_offset(int B, int N);
size_t sn2_fps_ws_rank_offset(int B, int N);
int sn2_fps(const float *pos_soa, int B, int N, int M, const int *start, int *idx, float *cpos_soa,
            float *cpos_aos, int *order_ws, void *stream);
/* The same with a choice of kernel for the bucketed path.  waves = 0 (what sn2_fps passes): the shortest pass.  16 / 8 / 4: one
 * workgroup of that many waves per plot (8: a 9 % longer pass that leaves half of each occupied CU to concurrent kernels: the
 * setting of a pipelined loop where the pass runs beside another batch's feature kernels; 4: for passes over hundreds of small
 * plots, two or more FPS workgroups per CU: parcel inference).  32 + P / 64 + P, P = 2, 4, 8: P workgroups of 16 / 8 waves per
 * plot (each owns every P-th bucket of the plot's Morton order; one exchange of tagged 8-byte granules through L2 per
 * super-round).  1: one sample per arg-max round (round 1's kernel, kept for cross-checks and timing comparisons).
 * What a request becomes for a given size -- the kernel, and every fall-back -- is sn2_fps_route ("Routes" below).
 * Same indices whichever runs. */
int sn2_fps_waves(const float *pos_soa, int B, int N, int M, const int *start, int *idx, float *cpos_soa,
                  float *cpos_aos, int *order_ws, int waves, void *stream);
/* The same with a STATUS word.  The multi-workgroup kernel's workgroups wait for their peers, and HIP does not promise that
 * the B * P workgroups of a launch are resident together (kernels of other streams or processes may hold the CUs a peer
 * needs): every wait is bounded, a workgroup whose wait runs out leaves without writing, and a REPAIR launch that every
 * multi-workgroup pass is followed by (the single-workgroup kernel, same stream; it reads one control word and returns when
 * no wait gave up) samples all plots again.  The results are the reference's either way; *status (device, one 32-bit
 * word, caller-zeroed once, or NULL) accumulates the number of waits that gave up, so that a host that synchronises anyway
 * can tell that passes are being repeated (torch_cluster.fps has no such failure mode: model/point_net2.py:22). */
int sn2_fps_status(const float *pos_soa, int B, int N, int M, const int *start, int *idx, float *cpos_soa,
                   float *cpos_aos, int *order_ws, int waves, unsigned *status, void *stream);
/* The same over a plot's LIVE points.  n_live (B) int32 on the device, or NULL (= N for every plot); n_live[b] is clamped to
 * [1, N] on the device, no host read.  The live set of plot b is {0 .. n_live[b]-1} together with its start point:
 *   - only live points are ever arg-max candidates (lowest index on ties, as always); the start may lie behind the prefix and is
 *     emitted as itself;
 *   - once the largest running distance over the live points is 0, every remaining sample is index 0 (idx 0, point 0's position);
 *   - n_live_out (B) int32 or NULL: the samples emitted before that happened, M if it never did.
 * Precondition for this to BE farthest point sampling over all N points: every point of [n_live[b], N) is a bit-identical copy
 * of a point of [0, n_live[b]) -- a copy's running distance always equals its original's, so it never wins a lowest-index tie,
 * and a maximum of 0 over the live points is a maximum of 0 over all (torch's argmax of an all-zero row is 0).  That is how
 * sn2_subsample, sn2_train_batch and numpy's sample_cloud lay a plot of fewer than N candidates out.  The prefix itself may hold
 * duplicates.  Then idx / cpos are the bytes of sn2_fps_status, without the all-ties rounds coincident points cost it (a
 * 51-point plot padded to thousands: ~n_live rounds instead of M), and n_live_out is a valid n_live for an FPS over cpos_soa
 * (the next level): positions n_live_out.. are point 0's, which an earlier sample covers.  Without the precondition the answer is
 * the definition above, the same from every kernel form.  The workspace describes all N points afterwards, as after sn2_fps.
 * sn2_fps, sn2_fps_waves and sn2_fps_status are this call with n_live = n_live_out = NULL.  NULL pos_soa / idx / cpos_*, B, N,
 * M <= 0, M > N, an unknown `waves`: SN2_EINVAL before any device work. */
int sn2_fps_live(const float *pos_soa, int B, int N, int M, const int *start, const int *n_live, int *idx, float *cpos_soa,
                 float *cpos_aos, int *order_ws, int waves, int *n_live_out, unsigned *status, void *stream);
/* tests only: sweeps a wait of the multi-workgroup FPS makes before it gives up (0 = the default, 2^18 ~ 0.2 s) */
int sn2_debug_fps_spin_limit(unsigned sweeps);

/* radius ball query -- torch_cluster.radius, model/point_net2.py:23-25.
 * For centroid i of plot b: all source points j of plot b with d2 < r2 (strict, canonical fp32 arithmetic; r2 = the
 * fp32 value of r*r evaluated in double, as torch_cluster compares),
 * ascending j, at most `cap` of them: nbr[(b*M+i)*cap + 0..cnt-1], cnt[b*M+i]. *total = sum of cnt (overwritten).
 * fps_ws: the workspace a bucketed sn2_fps call over the SAME sources left behind (cell lists: ~200 candidates per
 * centroid instead of N), or NULL for the full scan; same result either way. */
int sn2_ball_query(const float *src_soa, int B, int N, const float *cpos_soa, int M, float r2, int cap,
                   int *nbr, int *cnt, unsigned long long *total, const int *fps_ws, void *stream);

/* total = sum of cnt[0..n): the number of messages of a set of neighbour lists (what sn2_ball_query leaves in `total` for
 * the lists of one call; needed again when the lists of one call are handed on in parts). */
int sn2_count_sum(const int *cnt, int n, unsigned long long *total, void *stream);
/* the same for G consecutive lists of n counts each in one launch: total[h * total_stride] = sum of cnt[h*n .. (h+1)*n) */
int sn2_count_sum_group(const int *cnt, int G, int n, unsigned long long *total, size_t total_stride, void *stream);

/* k nearest sources (k = 1..3) + inverse squared distance weights -- the no_grad part of
 * torch_geometric.nn.knn_interpolate, model/point_net2.py:63.
 * idx (B*T,3), w (B*T,3): w = 1/max(d2,1e-16); unused slots (k<3 or S<k) get w = 0 and idx = idx[0].
 * ws + dst_fps_ws (optional, both or neither): ws = 16-byte aligned workspace of SN2_THREE_NN_WS_WORDS(B,S) 32-bit words,
 * dst_fps_ws = the workspace sn2_fps filled for the TARGET points (same B, N = T).  With them, where
 * sn2_three_nn_uses_grid(S, T), a wave takes 64 spatially adjacent targets and searches a per-plot x,y grid of the sources
 * instead of scanning all S (same result, bit for bit); results are still written at the targets' original positions. */
#define SN2_THREE_NN_WS_WORDS(B, S) ((size_t)(B) * (4 * (size_t)(S) + 1032))
size_t sn2_three_nn_ws_words(int B, int S);
int sn2_three_nn(const float *src_soa, int B, int S, const float *dst_soa, int T, int k, int *idx, float *w,
                 void *ws, const int *dst_fps_ws, void *stream);
/* The same search with the targets sorted by the source grid's x,y cells inside the call (a counting sort, one workgroup
 * per plot): every wave then holds 64 targets of one or two adjacent cells, whatever order the targets come in.
 * 128 <= S <= 8192 (the S range of sn2_three_nn_uses_grid; else SN2_ELIMIT); ws = 16-byte aligned workspace of
 * SN2_THREE_NN_XY_WS_WORDS(B,S,T) 32-bit words.  Same results as
 * sn2_three_nn, bit for bit. */
#define SN2_THREE_NN_XY_WS_WORDS(B, S, T) ((size_t)(B) * (4 * (size_t)(S) + 11 * (size_t)(T) + 1032))
size_t sn2_three_nn_xy_ws_words(int B, int S, int T);
int sn2_three_nn_xy(const float *src_soa, int B, int S, const float *dst_soa, int T, int k, int *idx, float *w,
                    void *ws, void *stream);
/* What the call leaves in ws for the inverted index (sn2_interp_index_ordered), as word offsets into ws:
 * *order_words: order (B*T) int32 -- per plot the permutation of 0..T-1 that walks the targets cell by cell of the source grid
 * (rows of cells in a snake), the order the search itself works in;
 * *copy_words (may be NULL): idx_sorted (B*T,3) int32, then w_sorted (B*T,3) at *copy_words + 3*B*T -- the result rows in
 * that order (row p of plot b = row order[b*T + p] of idx / w), written only by sn2_three_nn_xy_copy with sorted_copy != 0
 * (24 bytes per target more; a pass that builds no inverted index leaves it out).
 * Both stay valid until the next call with the same ws.  Returns 0, or SN2_EINVAL. */
int sn2_three_nn_xy_order_offset(int B, int S, int T, size_t *order_words, size_t *copy_words);
int sn2_three_nn_xy_copy(const float *src_soa, int B, int S, const float *dst_soa, int T, int k, int *idx, float *w,
                         void *ws, int sorted_copy, void *stream);

/* Input pipeline of a batch: load_cloud of the reference DataLoader, data_loader/loader.py:73-87 --
 * centre, append the fake ground points, keep xyz, [train: rotate about z, flip, add noise], rescale, gather the subsample --
 * one thread per output point.  raw (10,T): the B plots' raw points side by side (rows x, y, z, red, green, blue,
 * near_infrared, intensity, return_num, num_returns), offsets (B+1), centers (B,2); fake_xy (n_fake,2): the positions that
 * add_fake_empty_ground_points appends to every plot; idx (B,N): the subsample of each plot, values in
 * [0, raw points of the plot + n_fake); rot (B,2) fp64 = cos, sin of the rotation, flips (B,2); noise (6,noise_T) or NULL
 * = the clipped gaussian noise of x, y, red, green, blue, near_infrared for every point of every plot BEFORE subsampling
 * (fake points included), noise_offsets (B).  Outputs cloud (B,10,N), xyz (B,3,N).  All random draws are the caller's. */
int sn2_prepare_plots(const float *raw, long T, const int *offsets, const float *centers, const float *fake_xy, int n_fake,
                      const int *idx, int B, int N, int train, const double *rot, const int *flips, const float *noise,
                      const long *noise_offsets, long noise_T, float z_max, float *cloud, float *xyz, void *stream);

/* ---- the subsample of every plot of a batch, drawn on the device (csrc/sample.hip): the DISTRIBUTION of the reference's
 * sample_cloud (data_loader/loader.py:233-247), not numpy's draws.  idx (B,N) is what sn2_prepare_plots takes.
 * Plot b has n_b = offsets[b+1] - offsets[b] + extra candidates, numbered 0 .. n_b-1 as sn2_prepare_plots numbers them (the
 * plot's raw points, then the `extra` = n_fake appended ones).
 *
 * Generator: u(seed, key, i) is a 64-bit word from Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11), all words 32-bit unsigned:
 *   counter c = (c0, c1, c2, c3) = (i, 0, key & 0xffffffff, key >> 32)          (key: the plot's int64 key as 64 unsigned bits)
 *   key     k = (k0, k1)         = (seed & 0xffffffff, seed >> 32)
 *   ten times:  p0 = 0xD2511F53 * c0, p1 = 0xCD9E8D57 * c2                       (32 x 32 -> 64 bits)
 *               c <- (hi(p1) ^ c1 ^ k0, lo(p1), hi(p0) ^ c3 ^ k1, lo(p0))
 *               and, after each of the ten rounds (the tenth's has no effect), k0 += 0x9E3779B9, k1 += 0xBB67AE85 (mod 2^32)
 *   u = c0 << 32 | c1 of the final counter (the generator's first two output words, the first one on top).
 * Row of plot b with key_b = plot_keys[b]:
 *   n_b >  N: the N candidates i with the smallest pairs (u(seed, key_b, i), i), in ascending order of that pair.  The N smallest
 *             of n independent uniform keys are a uniform N-subset in uniform order, as choice(n, N, replace=False) gives; two
 *             equal keys (probability below n^2 / 2^65 per plot) are ordered by index.
 *   n_b <= N: idx[b, j] = j for j < n_b, and idx[b, j] = floor(u(seed, key_b, j) * n_b / 2^64) for n_b <= j < N (the high 64 bits
 *             of the 64 x 64 bit product; a value's probability is off from 1/n_b by less than 2^-64).
 * So a row depends on (seed, key_b, n_b, N) alone: not on B, the plot's place in the batch or the form that ran; integer
 * arithmetic only, and no atomic whose order could reach the output.
 * n_max: the caller's bound on every n_b (it picks the form and sizes the workspace without a device read).  A plot with more
 * candidates is sampled from its first n_max; a plot WITHOUT candidates (possible only with extra == 0) gets a row of zeros --
 * a caller that knows its counts on the host refuses such a plot before the call.  extra < 0, n_max <= 0, N <= 0: SN2_EINVAL.
 * form: 0 = by sn2_subsample_form(n_max, N); SN2_SUBSAMPLE_LDS = one workgroup per plot with the (key piece, index) pairs in
 * LDS, n_max <= SN2_SUBSAMPLE_LDS_MAX (else SN2_ELIMIT); SN2_SUBSAMPLE_GLOBAL = four launches over the workspace, any n_max.
 * | SN2_SUBSAMPLE_COARSE (tests): the pairs keep 2 key bits instead of 32, so nearly every comparison takes the path that
 * recomputes the full keys.  Every form gives the same bytes.
 * ws: 16-byte aligned, sn2_subsample_ws_words(B, n_max, N, form) 32-bit words (0 for the LDS form: ws may be NULL). */
#define SN2_SUBSAMPLE_LDS 1
#define SN2_SUBSAMPLE_GLOBAL 2
#define SN2_SUBSAMPLE_COARSE 4
#define SN2_SUBSAMPLE_LDS_MAX 16384
int sn2_subsample_form(int n_max, int N); /* SN2_SUBSAMPLE_LDS or SN2_SUBSAMPLE_GLOBAL: what form 0 takes */
size_t sn2_subsample_ws_words(int B, int n_max, int N, int form);
int sn2_subsample(const int *offsets, int extra, int n_max, int B, int N, unsigned long long seed, const long long *plot_keys,
                  int form, int *ws, size_t ws_words, int *idx, void *stream);

/* ---- a training batch from a plot set resident on the device (csrc/feed.hip): load_cloud(train=True) of the reference
 * (data_loader/loader.py:73-87) for B plots picked by an id table ON THE DEVICE, written straight into the caller's buffers in
 * stream order, no host read: centre, fake ground points, rotate, flip, clipped gaussian noise, rescale, subsample gather -- the
 * arithmetic of sn2_prepare_plots, the draws from the generator of sn2_subsample.  No noise tensor exists anywhere.
 * The set: raw (10,T) fp32 (channels as sn2_prepare_plots), offsets (P+1), centers (P,2) fp32, coverages (P,4) fp64; T < 2^31.
 * plot_ids (B) int32 on the device, any order, need not be adjacent; EVERY id must be in [0, P): the caller checks that on the
 * host copy the table was made from (the kernels do not).  n_max: the caller's bound on offsets[p+1] - offsets[p] + n_fake over
 * the set (as sn2_subsample's).  cos_sin (360,2) fp64: cos and sin of 0 .. 359 degrees as the host computes them (numpy:
 * cos(radians(a))), read, not recomputed, so the rotation is the host's bit for bit.  train = 0: no rotation, flip or noise
 * (load_cloud(train=False)); noise = 0: train without the noise.
 * Outputs: cloud (B,10,N), xyz (B,3,N), gt (B,4) fp64 = the plots' coverages rows, fps_start (2,B) int32.
 *
 * Draws: Philox4x32-10 exactly as under sn2_subsample, key (k0,k1) = seed, counter (i, c1, key.lo, key.hi) with the plot's
 * key = epoch * P + plot id: a plot's rows depend on (seed, epoch, plot id, N) alone -- not on B, its place in the batch or the
 * buffers.  c1 separates the domains, w0..w3 are the four output words:
 *   c1 = 0         the subsample: sn2_subsample's row for (seed, key), candidates = the plot's raw points then the fake ones;
 *   c1 = 1, i = 0  flip_x = w0 >> 31, flip_y = w1 >> 31, angle in whole degrees = (w2 * 360) >> 32 (numpy's choice(360));
 *   c1 = 1, i = 1  fps_start[0,b] = (w0 * N) >> 32, fps_start[1,b] = (w1 * M1) >> 32  (drawn with train = 0 too);
 *   c1 = 2, 3, i = the SOURCE index of the point (its candidate number before subsampling, fake points included: duplicates
 *                  of a point share their noise, as in the reference): two Box-Muller pairs per call, all in fp64, from
 *                  (wa, wb) = (w0, w1), then (w2, w3):  u1 = (wa + 1) 2^-32, u2 = wb 2^-32, r = sqrt(-2 ln u1),
 *                  t = 6.283185307179586 u2, pair = (r cos t, r sin t).  c1 = 2 gives the deviates of x, y, red, green in that
 *                  order, c1 = 3 those of blue and near_infrared (its second pair is unused).
 *                  noise term = fp32(clamp(0.1 g, -c, c)), c = 0.3 for x, y and 0.03 * 65536 for the colours (the colours' sigma
 *                  IS the xy sigma: loader.py:180,202), added in fp32 after rotation and flips.
 * ws: 16-byte aligned, *words of sn2_train_batch_ws_words(B, n_max, N, &words) 32-bit words (8 B when n_max <= N: no plot of the
 * set is subsampled without replacement, and no index row is written).  NULL buffers, B, N, P, M1, n_max <= 0, epoch < 0, a small
 * or misaligned workspace: SN2_EINVAL; T >= 2^31 or B > 65535: SN2_ELIMIT -- all before any device work. */
int sn2_train_batch_ws_words(int B, int n_max, int N, size_t *words);
int sn2_train_batch(const float *raw, long T, const int *offsets, const float *centers, const double *coverages, int P,
                    const int *plot_ids, int B, const float *fake_xy, int n_fake, int n_max, int N, int M1, float z_max,
                    unsigned long long seed, long long epoch, const double *cos_sin, int train, int noise, int *ws,
                    size_t ws_words, float *cloud, float *xyz, double *gt, int *fps_start, void *stream);
/* The same with n_live (B) int32 or NULL: n_live[b] = min(offsets[p+1] - offsets[p] + n_fake, N) for the plot p of slot b -- the
 * distinct points at the front of the plot's rows (every later row repeats one of them, noise included: it is keyed by source
 * index), i.e. sn2_fps_live's n_live for this batch.  sn2_train_batch is this call with NULL. */
int sn2_train_batch_live(const float *raw, long T, const int *offsets, const float *centers, const double *coverages, int P,
                         const int *plot_ids, int B, const float *fake_xy, int n_fake, int n_max, int N, int M1, float z_max,
                         unsigned long long seed, long long epoch, const double *cos_sin, int train, int noise, int *ws,
                         size_t ws_words, float *cloud, float *xyz, double *gt, int *fps_start, int *n_live, void *stream);

/* ---- growing such a set on the device (csrc/plotset.hip): K plots of a source plot list -- a parcel's prepared plots
 * (sn2_parcel_fill / sn2_parcel_znorm) with the plot-wise predictions of an eval forward as their coverages, or another set --
 * appended to a destination set that has spare capacity, in stream order, no host read, one launch.
 * Source: src_raw (10,src_T) fp32 with row stride src_T, src_offsets (Ps+1) int32, src_centers (Ps,2) fp32, src_cov (Ps,4) fp32 in
 * the projection's order (low, soil, medium, high).  sel (K) int32 on the device: source plot numbers, any order, need not be
 * adjacent, a plot may be named twice, plots without points are allowed; EVERY entry must be in [0, Ps): the caller checks that on
 * the host copy the table was made from (the kernel does not), as for plot_ids under sn2_train_batch.
 * Destination: dst_raw (10,cap_T) fp32 with row stride cap_T, dst_offsets (cap_P+1) int32, dst_centers (cap_P,2) fp32, dst_cov
 * (cap_P,4) fp64; P0 plots and T0 points are already there.  dst_start (K+1) int32 on the device: the destination column of each
 * appended plot's first point, made by the host from the point counts it knows: dst_start[0] = T0, dst_start[k+1] = dst_start[k]
 * + the points of plot sel[k], dst_start[K] = new_T (the host argument must equal it).
 * Writes, and nothing else:
 *   dst_raw[c, dst_start[k] + i] = src_raw[c, src_offsets[sel[k]] + i]      c = 0..9, i = 0 .. points of sel[k] - 1
 *   dst_offsets[P0 + k] = dst_start[k]                                      k = 0..K   (P0 + K included)
 *   dst_centers[P0 + k] = src_centers[sel[k]],  dst_cov[P0 + k] = (double) src_cov[sel[k]]   k = 0..K-1   (the widening is exact)
 * Columns at or beyond new_T, columns below T0 and table rows outside [P0, P0 + K) (offsets: outside [P0, P0 + K]) keep their
 * bytes.  A plain copy: no atomics, no workspace, every word has one writer -- the bytes do not depend on the order of the waves.
 * NULL buffers, K <= 0, P0 < 0, T0 < 0, P0 + K > cap_P, new_T > cap_T or new_T < T0: SN2_EINVAL; cap_T >= 2^31 or src_T >= 2^31:
 * SN2_ELIMIT -- all before any device work. */
int sn2_plots_append(const float *src_raw, long src_T, const int *src_offsets, const float *src_centers, const float *src_cov,
                     const int *sel, int K, float *dst_raw, long cap_T, int *dst_offsets, float *dst_centers, double *dst_cov,
                     int cap_P, int P0, long T0, const int *dst_start, long new_T, void *stream);

/* z-normalisation of a raw plot (offline preparation): z_i - min{ z_j : |xy_i - xy_j| <= radius } --
 * normalize_z_with_minz_in_a_radius, utils/load_data.py:237-249 (sklearn kd-tree radius query in x,y + a python loop).
 * x, y, z (n) fp32; the test is sklearn's: fp64 reduced distance dx*dx + dy*dy <= radius*radius, inclusive.
 * x_min..y_max: bounding box of the points (the caller has it from loading the plot).  ws: SN2_ZNORM_WS_WORDS(n, cells)
 * 32-bit words with cells = ((x_max-x_min)/radius + 2) * ((y_max-y_min)/radius + 2), 16-byte aligned.
 * zmin (n) and/or z_out (n) = fp32(z - zmin). */
#define SN2_ZNORM_WS_WORDS(n, cells) ((size_t)5 * (n) + 3 * (size_t)(cells) + 8)
size_t sn2_znorm_ws_words(int n, long cells);
int sn2_znorm(const float *x, const float *y, const float *z, int n, float radius, float x_min, float y_min, float x_max,
              float y_max, int *ws, float *zmin, float *z_out, void *stream);

/* ---- a parcel's plots (csrc/parcel.hip; host side parcel.py): the discs of extract_cloud (inference/prepare_utils.py:47-53,
 * scipy cKDTree.query_ball_point) around P plot centres and the per-plot z-normalisation of pre_transform
 * (utils/load_data.py:228-249), for the whole parcel at once.
 * cloud (10,T): the parcel in the reference's channel order and absolute metres.  centers (P,2) fp32.
 * Membership of point i in disc p: fp64 dx*dx + dy*dy <= radius*radius, no contraction (scipy's inclusive test; exact for fp32
 * inputs of similar magnitude).  The points of a plot are in ascending parcel index; the output bytes do not depend on the
 * order in which waves run (integer counts only, no float atomics).  T < 2^31; the hits of all centres < 2^31.
 * Centre grid: cells of side 1/cell_inv >= radius, cell of a position floor((v - g0) * cell_inv) in fp64; cell_start
 * (GX*GY+1) and cell_items (centre ids, ascending inside a cell) are the CSR of the centres over the cells, row-major.
 * Rows: a wave walks `L` consecutive points (one row, rows = ceil(T/L)); P*rows < 2^28.
 *
 * sn2_parcel_count: prefix (P*rows+1) = exclusive scan, plot-major, of the points of row r in disc p; prefix[P*rows] and
 *   total[0] (int64) = all hits.  Plot p holds prefix[(p+1)*rows] - prefix[p*rows] points.  ws: sn2_parcel_count_ws_words.
 * sn2_parcel_fill: writes point i of disc p (p kept: plot_base[p] != INT_MIN) to slot plot_base[p] + prefix[p*rows + r] +
 *   its rank in the row: point_index[slot] = i, raw[c*sum_n + slot] = cloud[c*T + i] for every row c but z (c = 2).  prefix
 *   is consumed (advanced).  sum_n = the slots of the kept plots.
 * sn2_parcel_znorm: raw[2*sum_n + s] = fp32(z_i - min{ z_j : |xy_j - xy_i| <= radius, |xy_j - c_p| <= disc_radius }) for the
 *   point i = point_index[s] of the plot p with offsets[p] <= s < offsets[p+1] (P plots, centres `centers`): the local
 *   minimum of normalize_z_with_minz_in_a_radius over the plot's own points.  x_min..y_max: bounding box of the parcel;
 *   the grid of cells of side radius has at most 2^26 cells.  ws: sn2_parcel_znorm_ws_words (0 = beyond that limit).
 * ws must be 16-byte aligned. */
size_t sn2_parcel_count_ws_words(int P, int rows);
size_t sn2_parcel_znorm_ws_words(long T, float radius, float x_min, float y_min, float x_max, float y_max);
int sn2_parcel_count(const float *cloud, long T, int L, int rows, const float *centers, int P, const int *cell_start,
                     const int *cell_items, int GX, int GY, double gx0, double gy0, double cell_inv, float radius, int *ws,
                     size_t ws_words, int *prefix, long long *total, void *stream);
int sn2_parcel_fill(const float *cloud, long T, int L, int rows, const float *centers, int P, const int *cell_start,
                    const int *cell_items, int GX, int GY, double gx0, double gy0, double cell_inv, float radius, int *prefix,
                    const int *plot_base, long sum_n, float *raw, int *point_index, void *stream);
int sn2_parcel_znorm(const float *cloud, long T, float x_min, float y_min, float x_max, float y_max, float radius,
                     float disc_radius, const int *offsets, const float *centers, int P, const int *point_index, long sum_n,
                     int *ws, size_t ws_words, float *raw, void *stream);

/* ---- the plots of K parcels in one pass (csrc/parcels.hip; host side parcel.py: ParcelClouds, prepare_parcels).  What a
 * prepared plot is does not change: every rule above is stated once (csrc/parcel_rules.h) and executed here with the parcel's own
 * columns, centres, centre grid and z-norm cells, so parcel k's plots are the bytes sn2_parcel_count / _fill / _znorm give for
 * parcel k alone, and a parcel's points never see another parcel's centres or points, even where two parcels overlap in space.
 * The output bytes do not depend on arrival order (the order in which waves run): integer counts and cursors, min / max over
 * floats through order-preserving integers, no floating-point add atomics.
 * CLOUD ARENA.  (10, T_all) fp32, channel-major; parcel k owns the columns [t0_k, t0_k + T_k); every T_k > 0, T_all < 2^31.
 * PARCEL TABLE.  (K+1) rows of SN2_PARCELS_COLS int64, written by sn2_parcels_table (host arithmetic, no device):
 *   [0] t0_k  [1] T_k  [2] first row (a row = L consecutive points of ONE parcel, rows_k = ceil(T_k / L); 0 rows when P_k = 0)
 *   [3] c0_k: first centre  [4] P_k (0 is legal: the parcel owns no rows, no entries and no cells)
 *   [5] first (plot, row) entry; parcel k's entries are plot-major, P_k rows_k of them
 *   [6] first word of its centre-grid CSR in cell_start (GX GY + 1 words; the values index cell_items of ALL parcels, the items are
 *       centre ids relative to c0_k)  [7] GX  [8] GY  [9..11] the fp64 bits of gx0, gy0, cell_inv
 *   [12] first z-norm cell  [13] fp32 bits of x_min | y_min << 32  [14] of x_max | y_max << 32  [15] z-norm GX | GY << 32
 *   row K: [0] T_all  [1] L  [2] rows  [3] centres  [4] K  [5] entries  [6] CSR words  [12] z-norm cells
 *          [13] fp32 bits of radius | z-norm radius << 32; the rest 0.
 *   One L for the set: max(2048, ceil(sum T_k P_k / 2^26) rounded up to 64), as parcel.prepare_parcel grows it.
 * Every entry point but sn2_parcels_bbox takes the table twice, table_host and its copy table_dev, and before it launches checks
 * that the builder makes the same words of the host copy's own sizes, grids and boxes (else SN2_EINVAL: T_k <= 0, bases that are
 * not the prefixes, cells narrower than the radius, a radius that is not the table's; SN2_ELIMIT: T_all >= 2^31, 2^28 entries or
 * CSR words, more than 2^26 z-norm cells).  NULL pointers, K <= 0, a misaligned or short workspace: SN2_EINVAL.
 *
 * sn2_parcels_bbox: ONE launch.  starts (2, K+1) int64, on the host and on the device: point_start, then the exclusive prefix of
 *   ceil(T_k / SN2_PARCELS_BBOX_CHUNK): parcel k is cut into that many workgroups, each found by binary search on the prefix.
 *   state (K,4) uint32, in and out: the order-preserving integers (negative floats: ~bits; others: bits | 2^31) of x_min, y_min,
 *   x_max, y_max, folded in by integer atomic min / max.  The caller initialises it to (~0, ~0, 0, 0) per parcel; a state that
 *   already holds the boxes of the same arena is left as it is.  Decoded, the box is cloud[:2].min(1) / .max(1) of finite values.
 * sn2_parcels_table: host only.  T (K), P (K), GX, GY (K), grid (K,3) = gx0, gy0, cell_inv (read where P_k > 0), boxes (K,4) fp32
 *   -> table, L, and the workspace words of sn2_parcels_count and sn2_parcels_znorm.
 * sn2_parcels_count: clear + ONE pass over all rows (a wave finds its parcel from its global row, wave-uniformly) + one scan
 *   over all entries + a gather: prefix (entries + 1) as sn2_parcel_count's per parcel, total[0] = all hits (int64),
 *   plot_start (P_all + 1) int64 = the first entry's value of every plot, then the total.  centers (P_all,2).  ws 8-byte aligned.
 * sn2_parcels_fill: ONE launch; plot_base (P_all), INT_MIN = dropped; slot = plot_base[p] + the entry's cursor + rank.
 *   point_index[slot] = i - t0_k: the column in the parcel's own cloud.
 * sn2_parcels_znorm: the launches of sn2_parcel_znorm, once.  offsets (P+1), centers (P,2), plot_parcel (P) int32 of the KEPT
 *   plots; radius = the table's z-norm radius, disc_radius = its radius.  ws 16-byte aligned. */
#define SN2_PARCELS_COLS 16
#define SN2_PARCELS_BBOX_CHUNK 4096
int sn2_parcels_table(int K, const long long *T, const int *P, const int *GX, const int *GY, const double *grid,
                      const float *boxes, float radius, float zradius, long long *table, int *L, size_t *count_ws_words,
                      size_t *znorm_ws_words);
int sn2_parcels_bbox(const float *arena, long T_all, int K, const long long *starts_host, const long long *starts_dev,
                     unsigned *state, void *stream);
int sn2_parcels_count(const float *arena, int K, const long long *table_host, const long long *table_dev, const float *centers,
                      const int *cell_start, const int *cell_items, float radius, int *ws, size_t ws_words, int *prefix,
                      long long *total, long long *plot_start, void *stream);
int sn2_parcels_fill(const float *arena, int K, const long long *table_host, const long long *table_dev, const float *centers,
                     const int *cell_start, const int *cell_items, float radius, int *prefix, const int *plot_base, long sum_n,
                     float *raw, int *point_index, void *stream);
int sn2_parcels_znorm(const float *arena, int K, const long long *table_host, const long long *table_dev, float radius,
                      float disc_radius, const int *offsets, const float *centers, const int *plot_parcel, int P,
                      const int *point_index, long sum_n, int *ws, size_t ws_words, float *raw, void *stream);

/* ---- set abstraction: gather + shared MLP + BN + max -- SAModule/PointConv, model/point_net2.py:19,21-29 --- */
typedef struct sn2_sa {
    int B, Nsrc, M, cap;            /* plots, source points per plot, centroids per plot, stride of nbr        */
    int cf;                         /* feature channels of a source row (8 or 16); message = [feat | pos_j-pos_i] */
    int nl;                         /* blocks in local_nn: 1 or 2                                               */
    const float *feat; int feat_stride;  /* source feature rows (B*Nsrc, feat_stride)                           */
    const float *spos; int spos_stride;  /* source positions (x,y,z,.) rows                                      */
    const float *cpos;              /* centroid positions AoS4 (B*M,4)                                          */
    const int *nbr, *cnt;           /* from sn2_ball_query                                                      */
    const unsigned long long *total;/* number of messages E (device)                                            */
    const int *order;               /* from sn2_sa_order, or NULL: quads of consecutive centroids                      */
    sn2_block blk[2];
    float *ext; int *arg;           /* (B*M,cout): signed extremum of the last block's pre-BN activation and the
                                       neighbour slot attaining it (-1: no neighbours).  On a tie the slot is the
                                       LOWEST among those attaining the signed extremum, for either sign of gamma
                                       ("first maximum wins" in ascending source index).  An EVAL forward keeps
                                       nothing for a backward: it leaves both arrays untouched (round 5: its kernel
                                       writes `out` itself)                                                     */
    float *out;                     /* (B*M,cout) = a*ext + c : the module output x                             */
    const float *dout;              /* backward in : d loss / d out (B*M,cout)                                  */
    float *dfeat;                   /* backward out: ACCUMULATED d loss / d feat (B*Nsrc,cf) or NULL            */
    float *bwd_ws;                  /* backward, nl = 2: SN2_SA_BWD_WS_WORDS floats, ZERO on entry (left non-zero), or
                                       NULL.  Given, with dfeat = NULL and fp32 operands, the first block's dW/db come
                                       out of the SAME message pass as the last block's (three sums the BatchNorm
                                       backward is linear in + a one-workgroup combine kernel) instead of a pass of
                                       their own; otherwise it is not touched                                   */
} sn2_sa;
/* sn2_sa.bwd_ws: replicas of the two 16 x 12 images [sum m xhat (x) in | sum m (x) in] of the nl = 2 module (MLP[11,16,16]);
 * with four point features (MLP[7,16,16]) the images are 16 x 8 and use the front of every replica pair */
#define SN2_SA_BWD_WS_REPLICAS 32
#define SN2_SA_BWD_WS_WORDS (SN2_SA_BWD_WS_REPLICAS * 2 * 16 * 12)
/* Work items of the SA passes (position-only: part of the geometry pass).  A wave step is four 16-message tiles; a plot's
 * centroids are ranked by DESCENDING neighbour count (ties by ascending id -- deterministic) and cut into classes:
 *   SOLO (n > SN2_SA_SOLO_MIN: all four tiles, 64 messages per step), QUAD (n > SN2_SA_QUAD_MIN: ranks 4k..4k+3 share the
 *   steps, a tile each), OCT (n > SN2_SA_OCT_MIN: eight ranks, half a tile each, one step), HEX (the rest: sixteen ranks, a
 *   quarter tile each, one step).  (Ball sizes at C2: median 5, mean 25, maximum 261.)
 * Item k of plot b sits at position k*B + b of its table, i.e. heaviest first across plots.  order = SN2_SA_ORDER_WORDS(B,M)
 * ints (-1 = none): 4 B M ints of SOLO / QUAD positions, 4 each (solo: id | SN2_SA_SOLO_FLAG four times; quad: four ids);
 * 16 B SN2_SA_PACKED_ITEMS(M) ints of OCT / HEX positions, 16 each = the centroid of every quarter tile (an OCT's ids twice
 * each, | SN2_SA_OCT_FLAG); a trailer: [0] / [1] = the largest SOLO + QUAD / OCT + HEX item count of any plot. */
#define SN2_SA_SOLO_MIN 64
#define SN2_SA_QUAD_MIN 8
#define SN2_SA_OCT_MIN 4
#define SN2_SA_SOLO_FLAG 0x40000000
#define SN2_SA_OCT_FLAG 0x20000000
#define SN2_SA_PACKED_ITEMS(M) ((M) / 8 + 2)
#define SN2_SA_ORDER_WORDS(B, M) ((size_t)4 * (B) * (M) + (size_t)16 * (B) * SN2_SA_PACKED_ITEMS(M) + 8)
size_t sn2_sa_order_words(int B, int M);
int sn2_sa_order(const int *cnt, int B, int M, int *order, void *stream);
/* G consecutive batches of B plots each in one launch pair: cnt (G*B*M), batch h's work items at order + h * stride_words
 * (stride_words >= SN2_SA_ORDER_WORDS(B,M)): what a geometry pass over several batches of a pipelined loop calls */
int sn2_sa_order_group(const int *cnt, int G, int B, int M, int *order, size_t stride_words, void *stream);
int sn2_sa_forward(const sn2_sa *p, int training, void *stream);
int sn2_sa_backward(const sn2_sa *p, void *stream);

/* ---- dense-row block with interpolated + skip inputs: FPModule / GlobalSAModule, model/point_net2.py:37-42,62-67
 * u_r = [ interp_r (ca) | skip_r (cb) ],  interp_r = sa*( sum_k w_k src[idx_k] / sum_k w_k ) + sc,
 * h = relu(W u + b) (R,cout) stored pre-BN; consumers apply (a,c).  knn_idx = NULL: interp_r = src row r. */
typedef struct sn2_fp {
    int B, R_per_plot, S_per_plot;  /* rows per plot (targets), source rows per plot                            */
    int ca, cb;                     /* interpolated channels, skip channels (cb may be 0)                       */
    const float *src; int src_stride; const float *src_a, *src_c; /* source rows (pre-BN) + their affine or NULL */
    const int *knn_idx; const float *knn_w;                        /* (B*R,3) from sn2_three_nn or NULL          */
    const float *skip; int skip_stride;                            /* (B*R, skip_stride) or NULL                 */
    sn2_block blk;
    float *h; int h_stride;         /* (B*R,h_stride) pre-BN activations; h_stride = cout rounded up to 4        */
    const float *dy;                /* backward in : d loss / d (a*h+c)  (B*R,h_stride)                          */
    float *dsrc; int dsrc_stride;   /* backward out: ACCUMULATED d loss / d (sa*src+sc) (B*S,dsrc_stride) or NULL */
    float *dskip; int dskip_stride; /* backward out: ACCUMULATED (B*R, >=cb) or NULL                             */
    float *du_scratch;              /* backward workspace (B*R, max(ca, h_stride)) when knn_idx and dsrc are given */
    float *scatter_ws;              /* backward workspace when knn_idx and dsrc are given: SN2_INTERP_WS_WORDS(B,R,S)
                                       32-bit words (inverted index of the 3-NN table)                           */
    int scatter_ready;              /* > 0: scatter_ws already holds the index (sn2_interp_index); 0: sn2_fp_backward builds it;
                                       < 0: sn2_fp_backward leaves the per-row input gradients in du_scratch ((B*R, ca) rows)
                                       and does NOT add them onto dsrc: the caller transposes the interpolation itself
                                       (sn2_global_pool_backward does, for the plot's one source)                 */
    const int *bn_sums_done;        /* non-NULL (the `ok` word of sn2_head_bn_sums / sn2_fp_bn_sums): blk.dgamma /
                                       blk.dbeta already hold this BatchNorm's gradients, sn2_fp_backward launches no
                                       pass over the rows for them.  NULL: it does                                  */
    float *src_ws;                  /* workspace SN2_FP_SRC_WS_WORDS(B,R,S,cout) floats or NULL.  Given with knn_idx on a
                                       layer that sn2_fp_source_side(B*R, cb, 0) accepts (the per-point layer),
                                       everything linear in the interpolation is done once per SOURCE row: forward
                                       gathers rows of T = W_A (sa*src+sc) kept here; backward keeps the partial sums of G[s] = sum of
                                       w * d pre-activation over the rows interpolating s here, one row per 63 list
                                       entries (dsrc += G W_A, dW_A += G^T (sa*src+sc)).  NULL: every row rebuilds its interpolated input.     */
    int act_bf16;                   /* non-zero (only with src_ws, i.e. on the per-point layer, and with bn_sums_done): the rows
                                       of h, dy and du_scratch are bfloat16 (same ELEMENT strides: 72-byte rows at cout = 34)
                                       -- BASELINE.json configs[4]: the three per-point activation buffers are what the step
                                       streams; statistics, every sum and the weight gradients stay fp32               */
    const int *row_perm;            /* NULL, or (B*R) ints, a permutation of 0..R-1 per plot (with src_ws only): the backward
                                       pass keeps the d pre-activation row of target row r of plot b at row b*R + row_perm[b*R + r]
                                       of du_scratch, and the inverted index (sn2_interp_index_perm) lists those positions.
                                       With row_perm = the targets' positions along a space-filling curve (the last B*N words
                                       of sn2_fps's workspace) the rows a source gathers lie close together: the gather of the
                                       source-side backward runs out of L2 instead of fetching every row three times          */
} sn2_fp;
/* chunks of at most 63 list entries an inverted 3-NN index of R rows over S sources can have, per plot (+ one slot per
 * source: every list's last chunk may be short) */
#define SN2_INTERP_CHUNKS(R, S) ((3 * (size_t)(R) + 62) / 63 + (size_t)(S))
#define SN2_FP_SRC_WS_WORDS(B, R, S, cout) ((size_t)(B) * SN2_INTERP_CHUNKS(R, S) * ((((cout) + 3) / 4) * 4))
size_t sn2_interp_chunks(int R_per_plot, int S_per_plot);
size_t sn2_fp_src_ws_words(int B, int R_per_plot, int S_per_plot, int cout);
/* The transpose of knn_interpolate (its backward) is done as a gather through an inverted index of the 3-NN table:
 * source -> list of (target row, normalised weight).  The index depends on positions only, so it can be built ahead of
 * the backward pass (in the geometry pass) with sn2_interp_index; otherwise sn2_fp_backward builds it itself. */
#define SN2_INTERP_WS_WORDS(B, R, S) \
    ((size_t)(B) * (S) * (((R) + 2047) / 2048 + 6) + 6 * (size_t)(B) * (R) + 64 + 4 * (size_t)(B) * SN2_INTERP_CHUNKS(R, S))
size_t sn2_interp_ws_words(int B, int R_per_plot, int S_per_plot);
/* src_pos: (B*S,4) x,y,z,- rows of the SOURCE positions or NULL.  Given, the index also holds the sources of every plot
 * in Morton order, and the source-side backward (sn2_fp.src_ws) walks them in that order, one stretch per XCD, so that
 * target rows shared by neighbouring sources stay in that XCD's L2. */
int sn2_interp_index(const int *knn_idx, const float *knn_w, const float *src_pos, int B, int R_per_plot,
                     int S_per_plot, float *ws, void *stream);
/* the same index over PERMUTED target rows: list entries name row_perm[b*R + r] instead of r (sn2_fp.row_perm; NULL = identity) */
int sn2_interp_index_perm(const int *knn_idx, const float *knn_w, const float *src_pos, const int *row_perm, int B,
                          int R_per_plot, int S_per_plot, float *ws, void *stream);
/* the same for G consecutive batches of B plots each in ONE set of launches (round 5): knn_idx / knn_w / src_pos / row_perm are the
 * group's arrays (G*B plots, batch-major), batch h's index is written to ws + h * ws_stride_words (an ordinary B-plot workspace:
 * its consumers do not change; ws_stride_words >= SN2_INTERP_WS_WORDS(B,R,S), a multiple of 4).  The geometry pass of a
 * pipelined loop covers several batches per launch: 12 launches per pass instead of 12 per batch. */
int sn2_interp_index_group(const int *knn_idx, const float *knn_w, const float *src_pos, const int *row_perm, int G, int B,
                           int R_per_plot, int S_per_plot, float *ws, size_t ws_stride_words, void *stream);
/* the same, built in a given ORDER of the target rows: row_order (G*B*R) int32, per plot a permutation of 0..R-1, or NULL (then
 * exactly sn2_interp_index_group).  The lists hold the same entries; only the order inside a list, which is arrival order
 * either way, differs.  Meant for the order sn2_three_nn_xy leaves in its workspace (sn2_three_nn_xy_order_offset): walked
 * cell by cell of the source grid, a slice of 2048 rows names about a hundred sources and writes whole lines of their lists.
 * idx_sorted / w_sorted (with row_order; both or neither): the table's rows in that order (row p of plot b = row
 * row_order[b*R + p] of knn_idx / knn_w; sn2_three_nn_xy_copy writes them), read instead of a gather through row_order. */
int sn2_interp_index_ordered(const int *knn_idx, const float *knn_w, const float *src_pos, const int *row_perm,
                             const int *row_order, const int *idx_sorted, const float *w_sorted, int G, int B,
                             int R_per_plot, int S_per_plot, float *ws, size_t ws_stride_words, void *stream);
int sn2_fp_forward(const sn2_fp *p, int training, void *stream);
int sn2_fp_backward(const sn2_fp *p, void *stream);

/* per-plot max over R_per_plot rows of a*h+c -- global_max_pool, model/point_net2.py:39.
 * h has row stride C rounded up to 4.  out (B,C); arg (B,C) row attaining it; backward scatters dout into dy
 * (B*R, same stride), which the caller zeroed. */
int sn2_plot_max_forward(const float *h, const float *a, const float *c, int B, int R_per_plot, int C, float *out,
                         int *arg, void *stream);
int sn2_plot_max_backward(const float *dout, const int *arg, int B, int R_per_plot, int C, float *dy, void *stream);

/* The backward of the global level's pool in one launch (round 5): for FP3's per-row input gradients du (B*R, du_stride >= C) that
 * sn2_fp_backward left in its du_scratch (scatter_ready < 0) --
 *   dx (B,C) += sum over the plot's rows of du   (the transpose of knn_interpolate with k = 1 from the plot's one source, :137/:41),
 *   dy (B*R,C), zero-filled by the caller: dy[b R + arg[b][c]][c] = dx[b][c]   (the backward of global_max_pool, :39),
 *   dgamma, dbeta (C) += the BatchNorm sums over dy of the block whose pre-BatchNorm rows are h (B*R,C) with saved statistics
 *   mean, invstd -- B terms per channel, dy being zero elsewhere; hand the block's sn2_fp_backward a non-NULL bn_sums_done.
 * Replaces the gather inside sn2_fp_backward, sn2_plot_max_backward and the BatchNorm-sum pass of the global SA block.  C = 64. */
int sn2_global_pool_backward(const float *du, int du_stride, const int *arg, const float *h, const float *mean,
                             const float *invstd, int B, int R_per_plot, int C, float *dx, float *dy, float *dgamma,
                             float *dbeta, void *stream);

/* The reference architecture's global level in ONE launch, TRAINING mode (round 4): SA3 = MLP[35,64] on cat[x2, pos2]
 * (model/point_net2.py:133, 37-42), its BatchNorm, the plot's max (:39), FP3 = MLP[96,64] on cat[plot feature, x2] (:137,
 * 62-67) and its BatchNorm -- what sn2_fp_forward(sa3, 1), sn2_plot_max_forward and sn2_fp_forward(fp3, 1) do in five launches,
 * with the same staging, tiles and per-64-row statistics; only the two BatchNorms' sums cross workgroups (one workgroup of 16
 * waves per plot, 8-byte {tag, value} granules, every workgroup finalises the statistics itself in a fixed order).
 *   sa3, fp3: the descriptors the separate calls take (sa3: ca 32, cb 3, no 3-NN table, src = x2 (B*M2,32), skip = pos2 (B*M2,4);
 *             fp3: ca 64, cb 32, S_per_plot 1, src = x3, its 3-NN table, skip = x2; both cout 64, h_stride 64, fp32 operands);
 *             blk.stat_slots is not used;  x3 (B,64), arg3 (B,64): the plot feature and the rows attaining it;
 *   xchg: SN2_GLOBAL_XCHG_WORDS(B) 64-bit words and ctl: SN2_GLOBAL_CTL_WORDS 32-bit words, BOTH ZERO-FILLED ONCE and then left to
 *         the library (the launch epoch lives there: allocate them once, at the size of the largest batch, and never again while
 *         graphs that captured their address exist); launches that share them must be on one stream at a time.
 *   A wait for the peers' sums is bounded (HIP does not promise that the B workgroups of a launch are resident together): a
 *   workgroup whose wait runs out counts itself in ctl[1] and leaves; every workgroup takes a ticket on its way out, and the
 *   one that leaves LAST -- all its peers are gone -- finds the count changed and computes the whole level again, alone, with the
 *   same tiles and the same fixed-order sums: the results (rows, statistics, running statistics, counters) are those of an
 *   undisturbed launch, bit for bit, whatever happened (torch's BatchNorm has no such failure mode: model/point_net2.py:45-53).
 *   An undisturbed launch pays one fence and one atomic per workgroup for it.  ctl[1] stays as a sticky count a host may read
 *   where it synchronises anyway, to learn that launches are being repeated.
 * SN2_ELIMIT for other shapes, bfloat16 operands or more than SN2_GLOBAL_MAX_PLOTS plots (the collected granules of all plots
 * must fit the workgroup's LDS): use the separate calls. */
#define SN2_GLOBAL_MAX_PLOTS 28
#define SN2_GLOBAL_XCHG_WORDS(B) ((size_t)2 * (size_t)(B) * 4 * 128)
#define SN2_GLOBAL_CTL_WORDS 8
size_t sn2_global_xchg_words(int B);
int sn2_global_level_forward(const sn2_fp *sa3, const sn2_fp *fp3, float *x3, int *arg3, unsigned long long *xchg,
                             unsigned *ctl, void *stream);
/* The backward of that level in ONE launch (training mode, batch statistics, fp32 operands): FP3's BatchNorm sums (taken directly
 * over the rows of dy), FP3's backward, the pool's backward, SA3's BatchNorm sums and SA3's backward -- what sn2_fp_bn_sums (FP3's),
 * sn2_fp_backward(fp3, scatter_ready < 0), sn2_global_pool_backward and sn2_fp_backward(sa3) do in four launches.  One workgroup
 * per plot; FP3 interpolates the plot's ONE source with weight 1, so d x3[b] = (sum_rows dp) W[:, 0:64] and no per-row input
 * gradient of the interpolated part is formed; the gradient of SA3's output (B x 64 non-zeros) never reaches memory.
 *   sa3, fp3: the descriptors of the forward with the backward fields of the separate calls: fp3->dy (B*M2,64), fp3->dsrc = d x3
 *             (B,64, ACCUMULATED), fp3->dskip = sa3->dsrc = d x2 (B*M2,32, ACCUMULATED), blk.dW / db / dgamma / dbeta
 *             (ACCUMULATED); plot b adds its dW | db into image b: blk.grad_replicas >= B.  du_scratch, scatter_ws, sa3->dy and
 *             bn_sums_done are not used;  arg3 (B,64): the rows that attained the plot's max.
 *   xchg: SN2_GLOBAL_BWD_XCHG_WORDS 64-bit words and ctl: SN2_GLOBAL_BWD_CTL_WORDS 32-bit words of its OWN (not the forward's), zero-
 *         filled once and then left to the library, as above.
 *   A wait is bounded as in the forward.  Every store to a result lies behind a workgroup's last wait, so a workgroup that gives up
 *   has committed nothing; it counts itself in ctl[1] and the workgroup that leaves last finishes those plots alone: every result
 *   is committed exactly once, with the bits of an undisturbed launch.  Two runs on the same inputs give the same bits (fixed-order
 *   sums, no float atomics).
 * SN2_ELIMIT for other shapes, bfloat16 operands, frozen statistics, more than SN2_GLOBAL_MAX_PLOTS plots or fewer images than plots.
 * The entry point takes any number of rows per plot; the network's backward takes it up to SN2_GLOBAL_BWD_MAX_ROWS rows per plot
 * (one 64-row block per group of its workgroup: the instance measured against the four launches above) -- see
 * sn2_global_level_backward_route. */
#define SN2_GLOBAL_BWD_MAX_ROWS 256
#define SN2_GLOBAL_BWD_XCHG_WORDS ((size_t)2 * SN2_GLOBAL_MAX_PLOTS * 128)
#define SN2_GLOBAL_BWD_CTL_WORDS 64
int sn2_global_level_backward(const sn2_fp *sa3, const sn2_fp *fp3, const int *arg3, unsigned long long *xchg, unsigned *ctl,
                              void *stream);
/* tests only: the sweeps (~1 us each, default 2^18; 0 = back to it) an exchange wait of sn2_global_level_forward /
 * sn2_global_level_backward makes before it gives up */
int sn2_debug_global_spin_limit(unsigned sweeps);

/* ---- pointwise head: lin1+ReLU, lin2, softmax/sigmoid/product -- model/point_net2.py:141-151 ----------------
 * f (R,34) pre-BN with affine (fa,fc); coverages (R,4), proba (R,4). */
/* The loss gradient that sn2_head_backward can compute itself (the fused route, sn2_head_loss_route): what
 * sn2_projected_loss_backward takes, minus the two (R,4) buffers it writes.  The head backward then evaluates d loss / d proba and
 * d loss / d coverages of a row where it consumes them (csrc/loss_rules.h: the same two device functions as
 * sn2_projected_loss_backward's kernel, so the same bits) and the 32 B per point never travel through memory. */
#define SN2_HEAD_LOSS_MAX_PLOTS 128  /* its per-plot table (gx, gz, gw, 1/nocc) lives in what the head backward's LDS leaves free */
typedef struct sn2_loss_grad {
    const float *pred;              /* (B,4) plot-wise coverages of sn2_projected_loss_forward                    */
    const double *gt;               /* (B,4) fp64                                                                 */
    const float *proba;             /* (R,4) the STORED probabilities of the forward pass, R = B*N                */
    const double *pdf;              /* (R,3) fp64, or NULL when m = 0                                             */
    const double *grad_total;       /* device fp64 scalar: d objective / d total                                  */
    const int *arg, *nocc, *pix;    /* (B,D*D,3), (B), (R): sn2_projected_loss_forward's, sn2_plot_pixels'        */
    int B, N, D;
    double m, e;
} sn2_loss_grad;

typedef struct sn2_head {
    int R, cin, f_stride;           /* rows, 34, 36                                                              */
    const float *f, *fa, *fc;
    const float *W1, *b1, *W2, *b2; /* (16,34),(16),(5,16),(5)                                                   */
    float *coverages, *proba;
    const float *dcoverages, *dproba; /* backward in (R,4) each, either may be NULL                              */
    float *dy;                      /* backward out: d loss / d (fa*f+fc) (R,f_stride)                           */
    float *dW1, *db1, *dW2, *db2;   /* ACCUMULATED                                                               */
    int grad_replicas, grad_replica_stride; /* images of the four gradients, as in sn2_block                            */
    const int *drop_mask;           /* F.dropout between lin1 and lin2 (model/point_net2.py:142) in training: (R) words,
                                       bit j set = hidden channel j of the row is KEPT; NULL = no dropout (eval, p = 0) */
    float drop_scale;               /* 1/(1-p) applied to the kept channels (0 when p = 1)                         */
    int act_bf16;                   /* non-zero: the rows of f and dy are bfloat16 (as sn2_fp.act_bf16 of the block that wrote f) */
    float *zero_fill; long zero_fill_words; /* sn2_head_forward only, or NULL / 0: a buffer (16-byte aligned, a multiple of 4 words)
                                       that the forward kernel also clears -- the backward pass's zero-filled arena (sn2_net_bwd),
                                       so that no launch of its own has to clear it in front of the backward pass */
    const sn2_loss_grad *loss;      /* sn2_head_backward only; set by the caller, or NULL: gradients come in dcoverages / dproba as
                                       before.  Set: both of those must be NULL, R = loss->B * loss->N and
                                       sn2_head_loss_route(B, N, D) must say yes, else SN2_EINVAL */
} sn2_head;
int sn2_head_forward(const sn2_head *p, void *stream);
/* EVAL only: the per-point layer (p: the 34 + 8 -> 34 block with its 3-NN table, source-side workspace p->src_ws required) and
 * the head (hd: f / f_stride unused -- the rows never leave the CU; fa, fc = p->blk.a, p->blk.c; no dropout, fp32 rows) in one
 * pass: fp_forward(p, eval) + head_forward(hd) without the (B*N, 36) activation buffer between them (model/point_net2.py:139-151
 * under model.eval(), predict.py:96-126).  Same operations in the same order as the two calls: the same bits. */
int sn2_fp_head_eval(const sn2_fp *p, const sn2_head *hd, void *stream);
int sn2_head_backward(const sn2_head *p, void *stream);
/* tests only: the workgroups of sn2_head_backward's kernel (bf16: its bfloat16-row instantiation) that the runtime places on one
 * CU, with the LDS of a launch with (with_loss != 0) or without a descriptor -- the kernel is built for 2; < 0: -hipError_t */
int sn2_debug_head_backward_occupancy(int bf16, int with_loss);
/* After sn2_head_backward: the gradients of the BatchNorm whose output the head reads (FP1's), obtained from lin1's weight
 * and bias gradients instead of a pass over all rows (derivation in head.hip).  gamma, beta, mean, invstd: that BatchNorm's
 * parameters and saved batch statistics; dgamma, dbeta: ACCUMULATED, complete on return.  *ok (device int) = 1 when the
 * identity was used, 0 when some channel's |gamma| <= 1e-4 or |beta| > 64 |gamma| made it unusable and the kernel summed
 * over the rows itself (p->f = the BatchNorm's input rows, p->dy = the gradient of its output).  Hand `ok` to the producer's
 * sn2_fp_backward as bn_sums_done. */
int sn2_head_bn_sums(const sn2_head *p, const float *gamma, const float *beta, const float *mean, const float *invstd,
                     float *dgamma, float *dbeta, int *ok, void *stream);
/* The same for the BatchNorm whose output an FP block interpolates (its columns 0..ca-1), after that block's
 * sn2_fp_backward: the interpolation weights of a row sum to 1, so the identity carries over (p->src = the BatchNorm's
 * input rows, p->dsrc = the gradient of its output). */
int sn2_fp_bn_sums(const sn2_fp *p, const float *gamma, const float *beta, const float *mean, const float *invstd,
                   float *dgamma, float *dbeta, int *ok, void *stream);

/* ---- 2D projections -- model/project_to_2d.py -------------------------------------------------------------- */

/* P2 project_to_plotwise_coverages (:7-55): bbox-normalised diam_pix^2 grid per plot, per-pixel max of channels
 * 0,2,3 (first point wins ties), bare soil = 1 - low-veg max, mean over occupied pixels.
 * cloud_xy: plot b's normalised x row at cloud_xy + b*plot_stride, y row at + b*plot_stride + N.
 * keys (B*D*D*3) u64 workspace; pix (B*N) int32 out (x_pix*D + y_pix, bit-exact); arg (B*D*D*3) int32 out;
 * nocc (B) int32 out; pred (B,4) out.
 * DOMAIN of the tie rule (every entry point that scatters coverages: this one, _pix, sn2_raster_project,
 * sn2_projected_loss_forward, sn2_plot_losses): finite values, no NaN -- that is what "largest value, lowest point index
 * among the points that attain it" is proven on (tests/test_gpu_projection_loss.py).  The maximum is taken on the key
 * (ordered bits of the value << 32 | ~point), in which -0.0 orders BELOW +0.0 (torch_scatter's loop compares them equal and
 * keeps the first of the two) and a NaN orders by its bit pattern.  The network's coverages are sigmoid outputs, so
 * neither occurs there.  The ids are not range-checked: 0 <= pix < D*D is the caller's to keep. */
int sn2_plot_project_forward(const float *pred_pointwise, const float *cloud_xy, long plot_stride, int B, int N,
                             int D, unsigned long long *keys, int *pix, int *arg, int *nocc, float *pred,
                             void *stream);
/* The same in two parts, for callers that run their position-only kernels ahead of the feature kernels (the pixel id of a
 * point is a function of the plot's x, y only, project_to_2d.py:16-22): sn2_plot_pixels computes mm (B,4) = the plots'
 * (xmin, xmax, ymin, ymax) and pix (B*N) = the ids sn2_plot_project_forward would write; sn2_plot_project_forward_pix is the
 * rest of it from those ids -- keys: u64 workspace of SN2_P2_KEY_PARTS(N)*B*D*D*3 words (no initialisation: every slice of a
 * plot writes its own table, the finalisation takes their maximum), same arg / nocc / pred. */
#define SN2_P2_KEY_PARTS(N) (((N) + 4095) / 4096 < 1 ? 1 : (((N) + 4095) / 4096 > 64 ? 64 : ((N) + 4095) / 4096))
size_t sn2_p2_key_parts(int N);
int sn2_plot_pixels(const float *cloud_xy, long plot_stride, int B, int N, int D, float *mm, int *pix, void *stream);
int sn2_plot_project_forward_pix(const float *pred_pointwise, const int *pix, int B, int N, int D,
                                 unsigned long long *keys, int *arg, int *nocc, float *pred, void *stream);
/* d pred (B,4) -> d pred_pointwise (B*N,4): every row written (a point gets its pixel's gradient iff it is the pixel's
 * arg-max; pix, arg, nocc from the forward). */
int sn2_plot_project_backward(const float *dpred, const int *arg, const int *nocc, const int *pix, int B, int N,
                              int D, float *dpointwise, void *stream);

/* P1 project_to_2d_rasters (:58-113): fixed grid, clipped; rasters (B,3,D,D) [low,med,high], image[y,x], NaN where
 * empty, rows flipped; pix (B*N) int32 out = y_pix*D + x_pix (unflipped).  coverages (B*N,4) row-major. */
int sn2_raster_project(const float *coverages, const float *cloud_xy, long plot_stride, int B, int N, int D,
                       int diam_meters, unsigned long long *keys, int *pix, float *rasters, void *stream);

/* Parcel mosaic merge -- the plot-after-plot weighted merge of overlapping plot rasters that predict.py:136-141 obtains
 * from rasterio.merge with the callback inference/geotiff_raster.py:294-347 (_weighted_average_of_rasters), over per-plot
 * rasters carrying the radial weight band of add_weights_band_to_rasters (:103-118).  The callback's rule is ORDER
 * DEPENDENT (its weight band also sums the weights of plots whose score is no-data in a pixel), so the kernel keeps the
 * order: one thread per (band, parcel pixel) of the window folds plots 0..B-1 in sequence.
 * rasters (B,3,D,D) as produced by sn2_raster_project (NaN = no data); weights (D,D) (NaN outside the disc);
 * offsets (B,2) int32 = (row, col) of each plot's top-left pixel in the parcel grid;
 * mean, wsum (3,H,W): the running mosaic's score bands and weight bands, NaN = no data (caller fills with NaN once);
 * only parcel pixels in rows [win_y0, win_y0+win_h) x cols [win_x0, win_x0+win_w) are visited (pass the bounding window
 * of the batch, or 0,0,H,W). */
int sn2_mosaic_merge(const float *rasters, const float *weights, const int *offsets, int B, int D, int H, int W,
                     float *mean, float *wsum, int win_y0, int win_x0, int win_h, int win_w, void *stream);

/* Mosaic finalisation -- finalize_merged_raster (inference/geotiff_raster.py:262-285) up to, not including, the GIS
 * admissibility band: keep the three score bands + one weight band, insert the hard medium-vegetation band
 * (insert_hard_med_veg_raster_band :119-144: the threshold among linspace(0,1,10001) whose hard coverage is closest to the
 * mean soft coverage, first minimum), then NaN -> 0 wherever at least one score exists and NaN everywhere else.
 * mean (3,H,W) and wsum (H,W) from sn2_mosaic_merge; hist_ws SN2_MOSAIC_HIST_WORDS ints, sum_ws one double (both scratch);
 * thr_out[0] = threshold, thr_out[1] = its index; out (5,H,W) = [Vb, Vm_soft, Vh, Vm_hard, weights]. */
#define SN2_MOSAIC_HIST_WORDS 10004
int sn2_mosaic_finalize(const float *mean, const float *wsum, int H, int W, int *hist_ws, double *sum_ws, float *thr_out,
                        float *out, void *stream);

/* Parcel crop and band means of the mosaic -- crop_merged_raster (inference/geotiff_raster.py:238-253: every pixel whose centre
 * lies outside the parcel polygon becomes NaN) followed by get_parcel_predicted_values (inference/predict_utils.py:124-146: the
 * band-wise nanmean of the cropped mosaic = PRED_BASSE / PRED_INTER / PRED_HAUTE).  The rule, all of it fp64, every operation
 * rounded on its own (no fused multiply-add), the division correctly rounded:
 *   centre   of pixel (r,c): px = x_min + pix * (c + 0.5), py = y_max - pix * (r + 0.5) (the product rounded, then the sum:
 *            rasterio's xy(..., offset="center") over the geotransform of get_geotransform);
 *   edges    (E,4) fp64 = (ax, ay, bx, by), on the device: every ring edge of the polygon -- exterior, holes, all parts of a
 *            multi-part polygon (parcel.polygon_edges);
 *   crossing an edge crosses the pixel's row iff (ay > py) != (by > py), at xint = ax + ((py - ay) * (bx - ax)) / (by - ay)
 *            (a horizontal edge never crosses, so it never divides);
 *   inside   iff the number of crossing edges with px < xint is odd (parcel.polygon_keep's even-odd rule at buffer 0);
 *   crop     a pixel that is not inside becomes NaN in every band; an inside pixel keeps its bits;
 *   stats    after the crop count[k] = the non-NaN pixels of band k, mean[k] = their sum / count[k] (NaN when count[k] = 0): the
 *            values widened to fp64 and summed in fp64 (the reference's nanmean is numpy's fp32 pairwise sum).
 * bands (C,H,W) fp32, changed in place; mean (C) fp64 and count (C) int64 on the device.  E == 0 with edges == NULL: no crop,
 * bands is not written, the statistics alone.  ws: 8-byte aligned, SN2_MOSAIC_CROP_WS_WORDS(C,H,W) 32-bit words, no
 * initialisation.  Two launches on `stream`, nothing read back, no state outside ws (capturable).  DETERMINISTIC: no
 * floating-point atomics -- a workgroup takes the 256-pixel row segments blockIdx.x, + gridDim.x, ... (the grid is a function of
 * H and W alone), a thread adds its pixels in that order, the threads of a workgroup are summed in a fixed tree, and a second
 * launch of one workgroup sums the workgroups' partials in a fixed order: the same input gives the same bytes.
 * 1 <= C <= SN2_MOSAIC_CROP_MAX_BANDS, H, W >= 1, H * W < 2^31, E == 0 or 3 <= E <= SN2_MOSAIC_CROP_MAX_EDGES (beyond:
 * SN2_ELIMIT); pix > 0, x_min, y_max, pix finite.  Every workgroup walks all E edges once per row segment and keeps the xint of
 * those that cross its row: H * ceil(W/256) * E edge tests instead of H * W * E.
 * (sn2_mosaic_crop_ws_words is declared `extern`: tests/test_cabi.py holds the plain `size_t` declarations to a closed list of
 * macros; this one is held to its macro by tests/test_parcel_report_host.py.) */
#define SN2_MOSAIC_CROP_MAX_BANDS 8
#define SN2_MOSAIC_CROP_MAX_EDGES (1 << 20)
#define SN2_MOSAIC_CROP_MAX_BLOCKS 2048
#define SN2_MOSAIC_CROP_BLOCKS(H, W) \
    ((size_t)(H) * (((size_t)(W) + 255) / 256) < SN2_MOSAIC_CROP_MAX_BLOCKS ? (size_t)(H) * (((size_t)(W) + 255) / 256) \
                                                                           : (size_t)SN2_MOSAIC_CROP_MAX_BLOCKS)
#define SN2_MOSAIC_CROP_WS_WORDS(C, H, W) (4 * (size_t)(C) * SN2_MOSAIC_CROP_BLOCKS(H, W))
extern size_t sn2_mosaic_crop_ws_words(int C, int H, int W);
int sn2_mosaic_crop_stats(float *bands, int C, int H, int W, double x_min, double y_max, double pix, const double *edges, int E,
                          void *ws, double *mean, long long *count, void *stream);

/* ---- Mosaic atlas: the mosaics of K parcels in one arena, merged, finalised and cropped K canvases per launch (csrc/atlas.hip).
 * A shapefile of 1 ha parcels gives canvases of a few thousand pixels; the single-canvas calls above then pay their launches, and
 * ParcelMosaic.report its device-to-host read, once per parcel.  The atlas kernels execute the per-pixel rules of the single-canvas
 * kernels (csrc/mosaic_rules.h: the same functions), so every contract below reads "the bytes the single-canvas call gives".
 *
 * LAYOUT.  Canvas k has H_k x W_k pixels and the geotransform (x_min_k, y_max_k); base_k = the exclusive prefix of H_k W_k (int64).
 * It owns a contiguous, canvas-major slice of each arena: mean (3,H_k,W_k) at word 3 base_k, wsum the same, bands (C,H_k,W_k) at
 * C base_k (C = 5 from sn2_atlas_finalize) -- a zero-copy (C,H,W) view that the single-canvas entry points accept.
 * CANVAS TABLE.  (K+1) rows of SN2_ATLAS_CANVAS_COLS int64, written by sn2_atlas_canvas_table (host arithmetic, no device):
 *   [0] base_k  [1] H_k  [2] W_k  [3] exclusive prefix of SN2_ATLAS_FINALIZE_BLOCKS(H,W)  [4] the same of SN2_MOSAIC_CROP_BLOCKS(H,W)
 *   [5] x_min_k and [6] y_max_k as the bits of an fp64 (0.0 when x_min, y_max are NULL)  [7] 0;  row K: the three totals, 0 elsewhere.
 * Every entry point takes the table twice: `canvas_host` (checked against the rule above before any launch, it also gives the grid
 * sizes) and `canvas_dev`, the same bytes on the device (the kernels find their canvas in it by a wave-uniform binary search).
 * ERRORS, before any launch: SN2_EINVAL on a NULL pointer, K <= 0, a canvas with H or W <= 0, a non-finite geotransform or a table
 * that is not sn2_atlas_canvas_table's; SN2_ELIMIT on a canvas of H W >= 2^31 pixels or more than 2^31 - 1 workgroups in all.
 * wave64; vector stores only; no cross-workgroup spin; no floating-point atomics. */
#define SN2_ATLAS_CANVAS_COLS 8
#define SN2_ATLAS_SEG_COLS 8
#define SN2_ATLAS_FINALIZE_MAX_BLOCKS 1024
#define SN2_ATLAS_FINALIZE_BLOCKS(H, W) \
    (((size_t)(H) * (size_t)(W) + 255) / 256 < SN2_ATLAS_FINALIZE_MAX_BLOCKS ? ((size_t)(H) * (size_t)(W) + 255) / 256 \
                                                                            : (size_t)SN2_ATLAS_FINALIZE_MAX_BLOCKS)
int sn2_atlas_canvas_table(int K, const int *H, const int *W, const double *x_min, const double *y_max, long long *table);

/* Merge of one batch of plots into the atlas: ONE launch.  rasters (B,3,D,D), weights (D,D) as sn2_mosaic_merge takes them;
 * place (B,3) int32 on the device = each plot's (canvas, row, col), the plots in NON-DECREASING canvas order.  Each run of equal
 * canvas is one segment; the segment table -- `seg_host`, and `seg_dev` the same bytes on the device -- has (S+1) rows of
 * SN2_ATLAS_SEG_COLS int32:  [0] canvas (ascending)  [1] first plot  [2] last plot + 1  [3..6] y0, x0, h, w: the run's bounding
 * window (rows min row .. max row + D, columns alike) clipped to the canvas, h or w = 0 when nothing is left
 * [7] the exclusive prefix of the runs' workgroups, ceil(w/64) ceil(h/4) each;  row S: [7] = their total, 0 elsewhere.
 * A workgroup finds its run from [7] by a wave-uniform search and folds that run's plots only, in order, into its 4 x 64 tile:
 * the work is proportional to the runs' windows, not to the atlas.
 * CONTRACT: canvas by canvas, the arenas hold exactly the words sn2_mosaic_merge leaves when it is called on that canvas's view
 * with that run's plots and window; a canvas without a plot in the batch keeps its bytes.  A plot window that sticks out of its
 * canvas is clipped.  The host table is checked (runs ascending, plots [0,B) cut in order, windows inside their canvases, the
 * prefix as stated: else SN2_EINVAL), so whatever `place` holds on the device, nothing is written outside a run's canvas. */
int sn2_atlas_merge(const float *rasters, const float *weights, const int *place, int B, int D, int K, const long long *canvas_host,
                    const long long *canvas_dev, const int *seg_host, const int *seg_dev, int S, float *mean, float *wsum,
                    void *stream);

/* Finalisation of all K canvases: sn2_mosaic_finalize's four launches once instead of K times.  mean, wsum: the arenas;
 * bands: the (5,H_k,W_k) arena; thr (K,2) = threshold, its index per canvas.  ws: 8-byte aligned, SN2_ATLAS_FINALIZE_WS_WORDS(K)
 * 32-bit words, no initialisation: per canvas the histogram of k(v) over the medium band (int atomics) with the valid count, then
 * one fp64 partial sum per workgroup of the canvas.  Canvas k is cut into SN2_ATLAS_FINALIZE_BLOCKS(H_k,W_k) workgroups, workgroup
 * j takes the pixels 256 j + t, + 256 blocks, ...; its sum is a fixed tree, and the ONE threshold workgroup of the canvas (about
 * 100 KB of LDS) adds the partials in workgroup order: DETERMINISTIC, no floating-point atomics.
 * CONTRACT: histogram, count and index rule (first minimum, all-NaN -> 0) are sn2_mosaic_finalize's; bands and threshold equal
 * its bytes whenever both fp64 sums round to the same fp32 target (the single-canvas call adds its partials with an fp64 atomic,
 * in any order: the last fp64 bit of its sum may differ; sums of multiples of 2^-16 are exact in every order).
 * (The size helper returns its value through a pointer, as the carve functions do: tests/test_cabi.py and
 * tests/test_parcel_report_host.py hold the `size_t` and `extern size_t` declarations of this header to closed lists.) */
#define SN2_ATLAS_FINALIZE_CANVAS_WORDS (SN2_MOSAIC_HIST_WORDS + 2 * SN2_ATLAS_FINALIZE_MAX_BLOCKS)
#define SN2_ATLAS_FINALIZE_WS_WORDS(K) ((size_t)(K) * SN2_ATLAS_FINALIZE_CANVAS_WORDS)
int sn2_atlas_finalize_ws_words(int K, size_t *words);
int sn2_atlas_finalize(const float *mean, const float *wsum, int K, const long long *canvas_host, const long long *canvas_dev,
                       void *ws, float *thr, float *bands, void *stream);

/* Crop and band statistics of all K canvases: TWO launches.  bands: the (C,H_k,W_k) arena, changed in place; the geotransforms
 * are the table's; edges (sum E,4) fp64 on the device, ragged: canvas k owns rows edge_start[k] .. edge_start[k+1] (int32, K+1
 * entries, `edge_start_host` and the same bytes on the device).  E_k = 0: no crop for that canvas, its bands are not written, the
 * statistics alone (edges == NULL iff every E_k = 0).  mean (K,C) fp64, count (K,C) int64 on the device.
 * ws: 8-byte aligned, 4 C table[K][4] 32-bit words (= the sum of SN2_MOSAIC_CROP_WS_WORDS over the canvases), no initialisation.
 * Canvas k is cut into SN2_MOSAIC_CROP_BLOCKS(H_k,W_k) workgroups that take the row segments j, j + blocks, ... as the
 * single-canvas call's do; the second launch runs one workgroup per canvas.
 * CONTRACT: bands, means and counts of canvas k are the bytes sn2_mosaic_crop_stats gives on that canvas's view with that
 * canvas's edges -- the fp64 means too: the partition and the trees are the same.  Limits per canvas as there (C, E_k, pix). */
int sn2_atlas_crop_stats(float *bands, int C, int K, const long long *canvas_host, const long long *canvas_dev, double pix,
                         const double *edges, const int *edge_start_host, const int *edge_start_dev, void *ws, double *mean,
                         long long *count, void *stream);

/* ---- Admissibility band (csrc/admissibility.hip; the rule's functions: csrc/admissibility_rules.h): the fifth band of the
 * reference's parcel product and the source of PRED_ADM -- insert_admissibility_raster (inference/geotiff_raster.py:149-196):
 * rasterio `sieve` of the hard medium-vegetation band, `shapes` of its ones, a shapely buffer of -1.5, `geometry_mask`, then
 * max(Vb, Vm_soft) with the masked pixels set to 0.  Those libraries cannot be run beside this one, so the rule below is OURS: what
 * that chain comes to on a pixel grid (the reference passes an identity transform: its 1.5 m are 1.5 px), with the two places that
 * are a reading and not a pinned fact marked UNPINNED.  It works on one canvas of H x W pixels, on the five bands of the
 * finalisation [Vb, Vm_soft, Vh, Vm_hard, weights], BEFORE the crop (merge_geotiff_rasters finalises at :215, crops at :216).
 *   1 valid(p) = !isnan(Vm_hard(p)) (the finalisation makes the five bands NaN together);  h(p) = Vm_hard(p) > 0.
 *   2 SIEVE with size threshold s, 4-connectivity (the single pass of GDAL's sieve filter as we read it).  s <= 1: S = h.
 *     A region is a 4-connected component of valid pixels of equal h; id(R) = its smallest row-major pixel index, size(R) = its
 *     pixel count.  Two regions are neighbours when they hold 4-adjacent pixels; an invalid pixel is nobody's neighbour.
 *     big(R), for a region of size < s: the neighbour of largest size, ties to the SMALLEST id; none without a neighbour.
 *     The walk R -> big(R) -> big(big(R)) ... stops with target T at the first region of size >= s; it fails at a region without a
 *     big, or when a region comes up a second time.  Sizes are the original ones throughout: nothing cascades.
 *     S(p) = h(T) on the pixels of a small region whose walk found T;  S(p) = h(p) everywhere else.
 *     UNPINNED: s.  The reference calls sieve(..., 5, mask=isnan(...)); by rasterio's documentation a mask value of False EXCLUDES
 *     a pixel, so as written the valid pixels are excluded and nothing inside the parcel changes (s = 0); the comment beside the
 *     call, "Eliminate zones < 5 pixels", states the intent (s = 5).  Neither can be run here: s is the caller's, no default.
 *   3 H'(p) = 1 where !valid(p) (the reference sets the outside to one "to avoid border effects"), else min(h(p), S(p)): small
 *     patches of ones disappear, small holes of zeros stay zeros.
 *   4 inacc(p) iff H'(q) = 1 for every q at offset (dx,dy) with max(2|dx|-1,0)^2 + max(2|dy|-1,0)^2 < 9 (4 x the squared distance
 *     from p's centre to q's pixel square against 4 x 1.5^2); a q outside the canvas counts as 0.  In effect the 3 x 3 neighbourhood.
 *     UNPINNED: the tie.  The offsets (+-2,0), (0,+-2) sit at exactly 1.5 px, the centre ON the buffered outline; `<` counts it as
 *     inside (inaccessible).  GDAL's scanline fill treats the four sides differently.  The comparison is adm_offset_tested's.
 *   5 Adm(p) = NaN where !valid(p), 0 where inacc(p), else the larger of Vb(p), Vm_soft(p) in fp32.
 *   6 out (6,H,W) = [Vb, Vm_soft, Vh, Vm_hard, Adm, weights], the reference's band order; bands 0-3 and 5 carry the bits of the
 *     input, band 3 the UNSIEVED hard band as in the reference.
 * stats (K,4) int64 on the device, per canvas: regions, regions of size < s, pixels with S != h, valid inaccessible pixels.
 * ws: 8-byte aligned, SN2_ADM_WS_WORDS(pixels) 32-bit words for `pixels` = H W (the atlas: the sum over its canvases), no
 * initialisation: a head (the single-canvas call's one-row canvas table) and SN2_ADM_WS_WORDS_PER_PIXEL words per pixel -- union-find
 * parent, region size, sieve bit, H', and the 64-bit neighbour key.
 * PHASES, separate launches on `stream`, no cross-workgroup waiting, nothing read back (capturable): labelling by union-find with
 * atomicMin on the roots (a root is its tree's smallest index: the labels do not depend on the order of the atomics) -> flatten and
 * sizes (integer adds) -> big (one 64-bit atomicMax of (size << 32) | (0xFFFFFFFF - id) per adjacency) -> walk (one thread per
 * small region, repeat detection that terminates on any input) -> H' -> the offsets test and the six bands.  wave64; vector
 * stores and vector integer atomics only; no floating-point atomic: DETERMINISTIC, the same input gives the same bytes.
 * sn2_atlas_admissibility: bands5_arena / bands6_arena hold canvas k's (5,H_k,W_k) / (6,H_k,W_k) at word 5 base_k / 6 base_k.
 * CONTRACT: canvas k's six bands and stats are the bytes sn2_mosaic_admissibility gives on that canvas's view.
 * ERRORS, before any launch: SN2_EINVAL on a NULL pointer, H or W <= 0, K <= 0, sieve_size < 0, a misaligned ws or a table that is
 * not sn2_atlas_canvas_table's; SN2_ELIMIT on H W >= 2^31.
 * (The size helper returns its value through a pointer, as sn2_atlas_finalize_ws_words does.) */
#define SN2_ADM_WS_HEAD_WORDS (4 * SN2_ATLAS_CANVAS_COLS)
#define SN2_ADM_WS_WORDS_PER_PIXEL 6
#define SN2_ADM_WS_WORDS(pixels) (SN2_ADM_WS_HEAD_WORDS + SN2_ADM_WS_WORDS_PER_PIXEL * (size_t)(pixels))
int sn2_admissibility_ws_words(long long pixels, size_t *words);
int sn2_mosaic_admissibility(const float *bands5, int H, int W, int sieve_size, void *ws, float *bands6, long long *stats,
                             void *stream);
int sn2_atlas_admissibility(const float *bands5_arena, int K, const long long *canvas_host, const long long *canvas_dev,
                            int sieve_size, void *ws, float *bands6_arena, long long *stats, void *stream);

/* ---- Per-point scores of a parcel cloud (csrc/points.hip; the rule's functions: csrc/point_rules.h): the network's OWN pointwise
 * outputs of every batch -- what utils/visualize_predictions.py shows per plot as "Pointwise prediction" and "Score for
 * most-likely strata" -- scattered back onto the parcel's points and merged over the overlapping plots by the mosaic's radial
 * weight.  Not a reference output: the reference has no parcel-scale point product.
 *
 * CONTRIBUTION.  Sample j of plot b of a batch (B plots of N samples) contributes iff
 *   j < n_live[b]                                         (the repeats that pad a sparse plot do not count), and
 *   0 <= c = idx[b,j] < n_b = offsets[b+1] - offsets[b]   (the fake ground points appended after the plot's real points do not).
 * DESTINATION.  col = (col_base ? col_base[b] : 0) + point_index[offsets[b] + c]: the point's column in the parcel cloud, or in
 *   an arena of K parcel clouds with col_base[b] = the first column of plot b's parcel.  A (plot, point) pair contributes at
 *   most once.  offsets are the plots' positions in point_index (sum_n entries), as sn2_prepare_plots takes them.
 * VALUES.  v_1..v_4 = cov[b N + j, 0:4], v_5..v_8 = proba[b N + j, 0:4] of the eval forward, both (B N,4) fp32.
 * WEIGHT.  add_weights_band_to_rasters' 1.5 - r taken at the point instead of a pixel centre, in fp64 from the fp32 rows of
 *   xyz (B,3,N) (centred metres, as sn2_prepare_plots leaves them): dx = xyz[b,0,j], dy = xyz[b,1,j],
 *   r2 = (double)dx dx + (double)dy dy (both products exact, one rounding), r = sqrt(r2) / diam_meters, w = 1.5 - r.
 * SUMS.  64-bit integers in units of 2^-32, llrint = round to nearest even:
 *   acc[col][0] += llrint(w 2^32);   acc[col][k] += llrint(w (double)v_k 2^32), k = 1..8;   hits[col] += 1 (int32).
 *   Integer sums do not depend on the order of arrival: any batching, plot order or split into launches gives the same bytes.
 *   No floating-point atomic anywhere; the adds are vector global atomics whose result is not read.
 * FINALISATION.  scores[k-1][col] = (float)((double)acc[col][k] / (double)acc[col][0]), weight[col] = (float)((double)acc[col][0]
 *   / 2^32); a point with hits == 0 gets NaN scores and weight 0.  A single contribution returns v_k itself for v_k >= 2^-7.
 * acc: SN2_POINTS_ACC_WORDS int64 per point, hits: T int32; the caller zeroes both once.  acc is opaque between the two calls
 * (point col's word k lies at acc[9 col + k]).  scores (8,T) fp32, weight (T) fp32.
 * sn2_points_merge is ONE launch on `stream` (behind the forward that wrote cov / proba), no synchronisation, no host read;
 * sn2_points_finalize one launch, acc and hits unchanged.  Inside the kernel nothing is written for a sample whose idx is
 * outside its plot, whose plot's offsets lie outside [0, sum_n], or whose column lies outside [0, T).
 * ERRORS, before any launch: SN2_EINVAL on a NULL pointer (col_base may be NULL), B, N, T or sum_n <= 0, diam_meters <= 0 (or
 * NaN); SN2_ELIMIT on T, sum_n or B N >= 2^31. */
#define SN2_POINTS_ACC_WORDS 9
int sn2_points_merge(const float *cov, const float *proba, const float *xyz, const int *idx, const int *n_live, const int *offsets,
                     const int *point_index, long sum_n, const int *col_base, int B, int N, double diam_meters, long long *acc,
                     int *hits, long T, void *stream);
int sn2_points_finalize(const long long *acc, const int *hits, long T, float *scores, float *weight, void *stream);

/* ---- LAS point records (csrc/las.hip; the rule's functions: csrc/las_rules.h; host side las.py): the point-record block of a LAS
 * file, as the file holds it, to the ten fp32 rows of the reference's load_las_file (utils/load_data.py:149-184).  The file's
 * header stays on the host (las.read_header); `records` starts at the first record.
 * The reference reads its files through laspy 1.x (`laspy.file.File`), which laspy 2 removed and which cannot be run beside this
 * library.  So the LAYOUT below is OURS: a reading of the ASPRS LAS 1.0-1.4 specification, pinned by records typed out by hand
 * (tests/test_las_host.py) and not by the reference's library.  The arithmetic of the `reference` mode is load_las_file's own.
 *
 * RECORD LAYOUT.  Little-endian, record stride L bytes (the header's "point data record length").
 *     format   least L   fields beyond the base
 *       0        20      base
 *       1        28      + GPS time
 *       2        26      + RGB at 20
 *       3        34      + GPS time, RGB at 28
 *       6        30      base
 *       7        36      + RGB at 30
 *       8        38      + RGB at 30, NIR at 36
 *     4 / 5 / 9 / 10:  57 / 63 / 59 / 67, the waveform formats: their leading fields are those of 1 / 3 / 6 / 8.
 *   X, Y, Z: int32 at bytes 0, 4, 8.  Intensity: uint16 at byte 12.  Red, green, blue, NIR: uint16 each.
 *   Formats 0-5:  byte 14 = return number in bits 0-2, number of returns in bits 3-5; classification = byte 15.
 *   Formats 6-10: byte 14 = return number in bits 0-3, number of returns in bits 4-7; classification = byte 16.
 *   L may exceed the least length (extra bytes) and may be odd.
 * ROWS.  out[r row_stride + col0 + i], r = 0..9, of record i, all fp32: x, y, z, red, green, blue, nir, intensity, return_num,
 *   num_returns (the reference's order).  Colour rows the format does not have are written as 0.0f: four rows for formats 0, 1, 4,
 *   6, 9, the nir row for 2, 3, 5, 7.  The integer fields convert exactly.
 * COORDINATES, two modes.
 *   SN2_LAS_COORDS_REFERENCE: (float)((double)((long long)X - X0) / 100.0), the division a correctly rounded fp64 quotient; raw0 =
 *     X0, Y0, Z0 in raw integer units (host, 3 values; NULL = 0, 0, 0 = load_las_file: `las.X / 100`, then the cast of np.asarray).
 *     The header's scale and offset are NOT used, exactly as the reference ignores them.
 *   SN2_LAS_COORDS_HEADER: (float)((((double)X scale) + offset) - origin), each operation rounded to fp64 on its own (no fused
 *     multiply-add); xform (host, 9 doubles) = scale xyz, offset xyz, origin xyz in metres.  With origin 0 this is laspy's `.x`.
 *   raw0 / origin: fp32 has a step of 0.5 m at Lambert-93 northings; subtracting an origin BEFORE the rounding keeps centimetres.
 * CLASSIFICATION (optional, NULL = not wanted): classification[col0 + i] = the classification byte as the record holds it (in
 *   formats 0-5 with its three flag bits).  Nothing is filtered or compacted: a caller masks on the device.
 * ONE launch on `stream`: no atomics, no synchronisation, nothing read back, safe to capture; the same bytes in give the same
 * bytes out.  No load touches a byte at or beyond T L.  Records of at most 128 bytes are staged through LDS with 16-byte loads,
 * 256 consecutive records per workgroup; longer ones are read field by field.
 * ERRORS, before any launch: SN2_EINVAL on a NULL records / out, T <= 0, a compressed file (bit 7 or 6 of `format` set), a format
 * above 10, L below the format's least length or above 65535, n_bytes < T L, records not 16-byte aligned, col0 < 0 or
 * col0 + T > row_stride, an unknown mode, the header mode without xform, |raw0| > 2^52; SN2_ELIMIT on T >= 2^31.
 * sn2_las_record_min_length: host-only, the table above, or SN2_EINVAL.  sn2_debug_las_form(1) sends every later call through the
 * field-by-field form (measurements: scripts/bench_las.py), 0 restores the rule. */
#define SN2_LAS_COORDS_REFERENCE 0
#define SN2_LAS_COORDS_HEADER 1
#define SN2_LAS_ROWS 10
int sn2_las_record_min_length(int format);
int sn2_las_decode(const void *records, size_t n_bytes, int format, int L, long T, int mode, const double *xform,
                   const long long *raw0, float *out, long row_stride, long col0, unsigned char *classification, void *stream);
int sn2_debug_las_form(int form);

/* ---- LAS point records, written (csrc/las_write.hip; the rule's functions: csrc/las_write_rules.h; host side las.encode,
 * las.write_scored, las.write_parcels): the inverse of the decoder.  The point records of a LAS file, as the file holds them, come
 * back annotated with the network's per-point scores (sn2_points_finalize): NOTHING is re-encoded from the fp32 cloud -- every byte
 * the source record holds (coordinates, GPS time, colours, the file's own extra bytes) is copied unchanged -- and only the
 * classification field and appended extra bytes are new.  The layout is that of "LAS point records" above, OUR reading of the ASPRS
 * LAS 1.0-1.4 specification, pinned by records typed out by hand (tests/test_las_write_host.py); the header, the VLRs and the Extra
 * Bytes descriptors are written on the host (las.py).
 *
 * SOURCE AND DESTINATION.  Output record i, 0 <= i < T_out, has L_dst = L_src + E bytes.  Its source is record
 *   s = point_index ? point_index[i] : i of the T_src records of L_src bytes at `src` (format 0..10, L_src >= the format's least
 *   length; without point_index T_out <= T_src).  Its score column is c = col0 + i: scores[k score_stride + c] for rows k = 0..7 (the
 *   four coverages, then the four class probabilities), weight[c], hits[c].
 * COPIED BYTES.  Bytes [0, L_src) of the output are the source record's bytes, except the classification field.
 * CLASSIFICATION.  class_mode 0 leaves the field alone.  class_mode 1 decides it from rows 4..7 of scores, the class probabilities
 *   p[0..3] in the network's column order (low vegetation, bare soil, medium, high).  The point is scored iff hits[c] > 0.  Scored:
 *   best = 0; for k = 1..3: if (p[k] > p[best]) best = k -- strict, so ties go to the lowest index and a NaN never wins --, code =
 *   class_codes[best] (host, 4 ints).  Unscored: code = unscored_code; -1 leaves the byte as the source has it.
 *   Formats 6-10: byte 16 = code.  Formats 0-5: byte 15 = (byte 15 & 0xE0) | code, the synthetic, key-point and withheld flags kept.
 * EXTRA BYTES, chosen by the 10-bit field_mask and appended in ascending bit order.  Bits 0..7: rows 0..7 of scores, the fp32's own
 *   four bytes (the NaN of an unscored point bit for bit; no arithmetic).  Bit 8: weight[c], fp32.  Bit 9: min(hits[c], 65535) as
 *   uint16 (negative hits: 0).  E = 4 popcount(mask & 0x1FF) + 2 (mask >> 9 & 1): E need not be a multiple of 4.
 * BAD INDEX.  With point_index, an s outside [0, T_src) reads nothing, gives L_dst zero bytes and adds 1 to n_bad.
 * STATS.  SN2_LAS_STATS_BYTES of device memory, 8-byte aligned, INITIALISED BY THE CALLER (min = INT32_MAX, max = INT32_MIN, the rest
 *   0), so several launches accumulate into one file's header:
 *     byte   0  int32  min[3]         raw X, Y, Z of the records written
 *     byte  12  int32  max[3]
 *     byte  24  uint64 by_return[15]  the return number r of byte 14 (3 bits in formats 0-5, 4 bits in 6-10), bin r - 1 for 1 <= r <= 15
 *     byte 144  uint64 n_bad
 *     byte 152  uint64 n_scored       records with hits > 0 (hits NULL: none)
 *   A bad record counts in n_bad alone.  Integer atomics only, after a reduction per wave and per workgroup: the same input gives
 *   the same bytes.
 * BOUNDS.  No store touches a byte at or beyond T_out L_dst, no load a source byte at or beyond T_src L_src, no load a score
 *   column outside [col0, col0 + T_out).
 * WITHOUT SCORES.  scores, weight and hits may be NULL exactly when field_mask == 0 and class_mode == 0: a pure gather or copy.
 * ONE launch on `stream`, no synchronisation, nothing read back: safe to capture.  Records of at most
 * sn2_las_encode_stage_max() = 120 output bytes are composed in LDS, 256 consecutive ones per workgroup, and leave with 16-byte
 * stores (without point_index the source is staged with 16-byte loads as the decoder stages it; with it each lane fetches its own
 * record); longer ones are written byte by byte.  sn2_debug_las_encode_form(1) sends every later call through the byte-by-byte
 * form, 0 restores the rule.
 * ERRORS, before any launch: SN2_EINVAL on a NULL src / dst / stats, T_out <= 0, T_src <= 0, a compressed file (bit 7 or 6 of
 * `format`), a format above 10, L_src below the format's least length or above 65535, field_mask bits above bit 9, a class_mode other
 * than 0 / 1, L_dst above 65535, src_bytes < T_src L_src, dst_bytes < T_out L_dst, src or dst not 16-byte aligned, stats not 8-byte
 * aligned, T_out > T_src without point_index, col0 < 0 or col0 + T_out > score_stride, a NULL scores / weight / hits with a mask or
 * class_mode 1, class_mode 1 with class_codes NULL, a code outside 0..255 (0..31 for formats 0-5; unscored_code also -1);
 * SN2_ELIMIT on T_out or T_src >= 2^31. */
#define SN2_LAS_STATS_BYTES 160
#define SN2_LAS_FIELD_MASK_ALL 0x3FF
int sn2_las_encode(const void *src, size_t src_bytes, int format, int L_src, long T_src, const int *point_index, long T_out,
                   const float *scores, const float *weight, const int *hits, long score_stride, long col0, int field_mask,
                   int class_mode, const int *class_codes, int unscored_code, void *dst, size_t dst_bytes, void *stats, void *stream);
int sn2_las_encode_stage_max(void);
int sn2_debug_las_encode_form(int form);

/* ---- GeoTIFF image data (csrc/tiff_pack.hip; the rule's functions: csrc/tiff_rules.h; host side geotiff.pack, geotiff.write_atlas,
 * write_parcel, write_bands): the band arena of a mosaic atlas turned into the bytes its map files hold after their headers -- what
 * the reference's merge_geotiff_rasters (inference/geotiff_raster.py:199-235) leaves to GDAL.  The header (IFD, GeoKeys, GDAL
 * metadata) is assembled on the host with `struct` (geotiff.py); the layout is OUR reading of TIFF 6.0, TIFF Technical Note 3 and
 * the GeoTIFF key directory, pinned by files typed out by hand and by libtiff reading them back (tests/test_geotiff_host.py).
 * UNPINNED there: the text of the GDALMetadata tag (42112: band descriptions, STATISTICS_*), a reading of GDAL's format.
 *
 * SOURCE.  Canvas k has H x W pixels and C bands, 1 <= C <= SN2_MOSAIC_CROP_MAX_BANDS: the (C,H,W) view of a C-band arena at word
 *   C base_k -- the atlas layout and the atlas canvas table above, as they are.
 * IMAGE DATA BLOCK.  Exactly the bytes an uncompressed little-endian TIFF holds after its header, in one of two layouts:
 *                          SN2_TIFF_LAYOUT_BAND (PlanarConfiguration 2)    SN2_TIFF_LAYOUT_PIXEL (PlanarConfiguration 1)
 *     rows                 q = c H + r                                     q = r
 *     floats per row wc    W                                               W C
 *     float f of a row     bands[c][r][f]                                  bands[f % C][r][f / C]
 *     stride               1                                               C
 *   Row q occupies the 4 wc bytes at data_base_k + q 4 wc.
 * PREDICTOR 1.  Byte j of a row is byte j % 4 of float j / 4: the fp32's own bytes -- NaN payloads, -0 and denormals bit for bit, no
 *   arithmetic.
 * PREDICTOR 3, the floating-point predictor of TIFF Technical Note 3 as libtiff's fpDiff applies it on a little-endian host:
 *   t[j] = byte 3 - j / wc of float j % wc (plane 0 holds the sign and exponent bytes); out[j] = t[j] for j < stride, otherwise
 *   (t[j] - t[j - stride]) mod 256.  Each row on its own: nothing carries from one row to the next.
 *   PINNED for stride 1 (libtiff reads the files back bit for bit).  UNPINNED: stride C of the PIXEL layout -- no reader on hand
 *   opens multi-sample float files; it rests on bytes typed out by hand and on the reading of fpDiff stated here.
 * STATISTICS.  Per (k, c) SN2_TIFF_STATS_BYTES: uint64 count of the band's pixels that are not NaN; uint32 key of the smallest,
 *   uint32 key of the largest of them, key = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000) on the fp32's bit pattern, compared as
 *   uint32: -0 < +0, the infinities are ordinary values.  bits = key ^ (key >> 31 ? 0x80000000 : 0xFFFFFFFF) gives the fp32 back.
 *   INITIALISED BY THE CALLER on the stream: count 0, minimum 0xFFFFFFFF, maximum 0 -- an all-NaN band keeps them.  Integer
 *   atomics only, after a reduction per wave and per workgroup: the same input gives the same bytes.
 * PLACE TABLE.  (K+1) rows of SN2_TIFF_PLACE_COLS int64, written by sn2_tiff_place_table (host arithmetic, no device) from the
 *   canvas table and K flags (skip[k] != 0: no file; skip NULL: none flagged):
 *     [0] data_base_k, a multiple of 16: the blocks in canvas order, each rounded up to 16 bytes  [1] 1 = no file: no bytes, no
 *     workgroups  [2] the exclusive prefix of the canvases' workgroups  [3] the block's bytes C H W 4 (0 without a file);
 *     row K: [0] the offset of the statistics block, K C SN2_TIFF_STATS_BYTES bytes, canvas-major  [1] 0  [2] the workgroups in all
 *     [3] the bytes in all.  ONE staging buffer holds every block and then the statistics: one copy fetches everything.  The padding
 *   between blocks is never written.  Taken twice, `place_host` (checked before any launch) and `place_dev`, like the canvas table.
 *   The cut into workgroups follows the kernel form, so a table is made and used under the same sn2_debug_tiff_pack_form.
 * ONE launch on `stream` for all K canvases, no synchronisation, nothing read back: safe to capture.  Rows of at most
 * sn2_tiff_pack_stage_max() = 16384 bytes (4 wc) are STAGED: a workgroup gathers as many consecutive image rows as fit 16 KiB
 * of LDS from the C planes with coalesced loads, in row order, composes the byte planes and differences from LDS sixteen bytes at
 * a time and stores 16-byte words (17 KiB with the skew that keeps the lanes off each other's banks: eight to a CU's 160 KiB).
 * Longer rows take the DIRECT form: 16 KiB of a row
 * per workgroup, every output byte a function of at most two source floats read from memory.  Both give identical bytes;
 * sn2_debug_tiff_pack_form(1) sends every later table and call through the direct form, 0 restores the rule.
 * wave64; vector stores only; no floating-point atomics; no cross-workgroup waiting.
 * ERRORS, before any launch: SN2_EINVAL on a NULL pointer, K <= 0, C outside 1..SN2_MOSAIC_CROP_MAX_BANDS, an unknown layout or
 * predictor (1 or 3), dst not 16-byte aligned or a statistics offset that is no multiple of 16, a canvas table that is not
 * sn2_atlas_canvas_table's, a place table that is not sn2_tiff_place_table's, dst_bytes below the table's total; SN2_ELIMIT on a
 * block or a total of 2^32 bytes or more (classic TIFF cannot address it) or more than 2^31 - 1 workgroups. */
#define SN2_TIFF_LAYOUT_BAND 0
#define SN2_TIFF_LAYOUT_PIXEL 1
#define SN2_TIFF_PLACE_COLS 4
#define SN2_TIFF_STATS_BYTES 16
int sn2_tiff_place_table(int C, int K, const long long *canvas_host, int layout, const unsigned char *skip, long long *place);
int sn2_tiff_pack(const float *bands, int C, int K, const long long *canvas_host, const long long *canvas_dev,
                  const long long *place_host, const long long *place_dev, int layout, int predictor, void *dst, size_t dst_bytes,
                  void *stream);
int sn2_tiff_pack_stage_max(void);
int sn2_debug_tiff_pack_form(int form);

/* ---- Parcel shapefiles (host side shp.py: shp.read, shp.write_predictions; the device half below): the ESRI shapefile triple the
 * reference's parcel job starts from (`shapefile.Reader`, inference/prepare_utils.py:33) and ends with
 * (`update_shapefile_with_predictions`, inference/predict_utils.py:149-177).  The layout is OUR reading of the ESRI Shapefile
 * Technical Description (July 1998) and of dBase III, PINNED BY FILES TYPED OUT BY HAND (tests/_shp_cases.py), NOT BY pyshp: neither
 * pyshp nor shapely was at hand.
 *
 * .shp.  A header of 100 bytes: file code 9994, big-endian int32, at byte 0; the file's length in 16-bit words, big-endian int32, at
 *   byte 24; version 1000, little-endian int32, at byte 28; the shape type, little-endian int32, at byte 32 (the boxes at 36..99 are
 *   not read).  Then the records.  A record header is 8 bytes, both big-endian int32: the 1-based record number and the content
 *   length in words.  The content is little-endian: int32 shape type; for a polygon four doubles (the box: x_min, y_min, x_max,
 *   y_max), int32 NumParts, int32 NumPoints, NumParts int32 Parts[] (the first vertex of every part), NumPoints pairs of doubles
 *   (x, y).  Shape types read: 0 (null: the content is the type alone), 5 (Polygon), 15 (PolygonZ), 25 (PolygonM); the Z and M blocks
 *   that follow the points of 15 and 25 are skipped by the content length, not decoded.  Any other type is refused.  The record
 *   offsets come from walking the .shp itself; the .shx (the same header, then per record the offset and the content length in
 *   words, big-endian) is not needed to read and is only copied on write.
 * .dbf.  byte 0 the version, bytes 1..3 the date (YY MM DD), uint32 LE at byte 4 the record count, uint16 LE at byte 8 the header's
 *   length, uint16 LE at byte 10 the record length L.  From byte 32 field descriptors of 32 bytes: the name (11 bytes, NUL-padded), the
 *   type at byte 11 (C N F L D), the length at byte 16, the decimals at byte 17; the table ends with 0x0D, which is the header's last
 *   byte.  Then K records of L bytes, each begun by the deletion flag (' ' or '*'); a trailing 0x1A is optional.  The record count
 *   equals the .shp's.
 * WRITTEN.  .shp, .shx, .prj and .cpg are copied byte for byte.  The .dbf header is the source's with header_len += 32 n,
 *   record_len += n size and n descriptors of type F (length `size`, `decimal` decimals) before the 0x0D; the date stays, so the same
 *   input gives the same bytes.  Every record is the source's L bytes followed by the n fields below; one 0x1A closes the file.
 *
 * dBase records, annotated (csrc/dbf.hip; the rule's functions: csrc/dbf_rules.h; host side hip_ops.dbf_annotate).
 * OUTPUT.  Record k, 0 <= k < K, has Ld = L + n size bytes: bytes [0, L) are source record k's, then field f = 0..n-1 in `size` bytes.
 * VALUE.  row = row_of[k] (device, K int32); row < 0 or row >= R: v = missing; else v = values[row C + cols[f]] (values: device, (R,C)
 *   fp64; cols: HOST, n ints, any order).
 * FIELD.  text = the decimal expansion of the EXACT binary value of v rounded half-to-even at `decimal` places -- what CPython's
 *   format(v, ".<decimal>f") and glibc's printf("%.<decimal>f") print -- made with integer arithmetic only (mantissa and exponent
 *   from the bits, a 64 x 64 -> 128-bit product, shifts, divisions by constants): no floating-point operation touches v.  The sign is
 *   '-' whenever the sign bit is set: -0.0 and a negative that rounds to zero print -0.000...  decimal = 0 prints no point.  A NaN
 *   prints nan (either sign), the infinities inf and -inf.  field = text[:size] right-justified with spaces.  A finite
 *   |v| >= 2^53 fills the field with '*' (the dBase overflow convention; CPython would print such a value exactly, we do not) and
 *   adds 1 to the overflow count.
 * DST.  16-byte aligned; K Ld bytes of records, then on the next multiple of 8 the uint64 overflow count, INITIALISED BY THE CALLER
 *   (0) on the stream: dst_bytes >= (K Ld rounded up to 8) + 8, and ONE device-to-host read fetches records and count.  The padding
 *   before the counter is never written.
 * ONE launch on `stream`, ONE kernel form: the output is a stream of K Ld bytes cut into tiles of 16 KiB; a workgroup composes its
 * tile in LDS (the copied bytes by consecutive lanes on consecutive bytes, a lane per field) and the tile leaves with 16-byte
 * stores.  wave64; vector stores only; no floating-point atomics; the count is one integer atomic per workgroup after a per-wave
 * reduction; no cross-workgroup waiting; nothing read back: safe to capture.
 * ERRORS, before any launch: SN2_EINVAL on a NULL pointer, K <= 0, R <= 0, C <= 0, L outside 1..65535, size outside 1..254,
 * decimal outside 0..15 or decimal + 2 > size, n outside 1..255, a cols entry outside [0, C), L + n size > 65535, dst not 16-byte
 * aligned, dst_bytes too small; SN2_ELIMIT on K > 2^40, R >= 2^31 or more than 2^31 - 1 tiles. */
int sn2_dbf_annotate(const void *src_records, long K, int L, const double *values, long R, int C, const int *row_of, const int *cols,
                     int n, int size, int decimal, double missing, void *dst, size_t dst_bytes, void *stream);

/* ---- Parcel cut (csrc/cut.hip; the rule's functions: csrc/cut_rules.h; host side parcel.cut_parcels, las.load_parcels): the points
 * of a LAS tile cut into K parcel clouds by the parcels' polygons buffered by b metres -- what the reference's
 * `parcelles_dataset_20m` holds as one file per parcel (b = 20, inference/prepare_utils.py:148).
 *
 * THE RULE, that of parcel.polygon_keep (numpy, fp64).  Point i has (px, py) = its fp32 x, y widened to fp64.  Parcel k has the edges
 * (ax, ay, bx, by) in fp64 that parcel.polygon_edges lists: all rings, holes and further parts, closing edges included.
 * b2 = b * b in fp64.  Point i belongs to parcel k iff
 *   inside: the number of edges with (ay > py) != (by > py) and px < ax + ((py - ay) * (bx - ax)) / (by - ay) is odd (the
 *           quotient evaluated only where the edge crosses), or
 *   near:   for some edge, with dx = bx - ax, dy = by - ay, l2 = dx*dx + dy*dy, t = l2 > 0 ? ((px - ax)*dx + (py - ay)*dy) / l2 : 0
 *           clamped to [0, 1], ex = (ax + t*dx) - px, ey = (ay + t*dy) - py:  ex*ex + ey*ey < b2  (strict).
 * Every operation is rounded to fp64 on its own, in that association (no fused multiply-add): the boolean is numpy's, bit for bit.
 * A lane stops at its first edge within b (the answer is an OR).  A NaN or infinite x or y belongs to no parcel (numpy's
 * comparisons say so; the device gives such a point no grid cell).  A point in two parcels' buffers is copied into both.  With a
 * classification (T) uint8 and a 256-bit drop set (8 words, bit c of word c / 32), a point whose class is in the set belongs to
 * no parcel.  The buffer inherits polygon_keep's deviation from shapely (exact round joins, not 16 segments per quarter circle).
 *
 * CANDIDATE TABLE (sn2_cut_table), built on the host (hip_ops.CutTable), every array on the host AND on the device:
 *   a uniform grid of GX x GY square cells as CSR: cell_start (GX GY + 1), cell_items (n_items) parcel ids, ascending inside a cell;
 *   cell of a coordinate = floor((v - g0) * inv), the same fp64 expression on both sides.  The host lists parcel k in every cell
 *   from cell(lo_k) to cell(hi_k) of its vertices' bounding box expanded by strictly more than b; the expression is monotonic, so a
 *   point's cell list is a superset of the parcels that keep it.  The rule decides membership, the grid only prunes.
 *   edge_start (K + 1) into edges (n_edges, 4) fp64.  T: the points of the cloud.  L: points per row (a wave walks one row).
 * Before any launch every entry point checks the HOST copy (else SN2_EINVAL): K >= 1, T >= 1, b finite and >= 0, GX, GY >= 1, g0
 * finite, inv finite and > 0, both starts begin at 0, never decrease and end at n_items / n_edges, every id in [0, K) and strictly
 * ascending inside its cell, every edge coordinate finite (and at most 1e100 in magnitude: no product of the rule overflows), L a
 * positive multiple of 64.  SN2_ELIMIT: T >= 2^31, more than 2^22 cells, 2^24 list entries, 2^26 edges or 2^28 (parcel, row)
 * entries.  So no index a kernel derives from the table leaves its arrays.
 *
 * cloud (10, T) fp32, channel-major, contiguous (a ParcelClouds arena of tiles is one such cloud).
 * sn2_cut_ws_words: host only -> the 32-bit words of sn2_cut_count's workspace (the scan's block sums + K rows counts).
 * sn2_cut_count: clear + ONE pass (a wave per row of L points, 64 at a time; the wave visits its lanes' candidate parcels in
 *   ascending id and the lanes that have parcel m as a candidate run m's edges together, so the edge addresses are wave-uniform;
 *   the ballot's popcount goes to entry m rows + row) + one scan + a gather: prefix (K rows + 1) int32, parcel_start (K + 2) int64 =
 *   the first slot of every parcel, the total, and the scan's own total word.  ws 8-byte aligned.
 * sn2_cut_fill: ONE launch over the same rows in the same order.  parcel_base (K) int32, INT_MIN = parcel skipped; slot =
 *   parcel_base[m] + the entry's cursor + rank (mbcnt over the ballot); the cursor is advanced by the row's own wave only.  Ten rows
 *   are copied per hit into out (10, sum_n) and point_index[slot] = i.  A parcel's points are in ascending tile index: byte for
 *   byte cloud[:, mask_k].  Integer atomics on the row's own cursor only, no floating-point atomics: the same input gives the same
 *   bytes.  prefix is consumed.  sum_n >= 2^31: SN2_ELIMIT.
 * classification and drop are both NULL or both given (drop: host, 8 words). */
#define SN2_CUT_MAX_CELLS (1 << 22)
#define SN2_CUT_MAX_ITEMS (1 << 24)
typedef struct {
    int K, GX, GY, L;
    long long T, n_items, n_edges;
    double gx0, gy0, inv, buffer;
    const int *cell_start, *cell_items, *edge_start;                    /* host copies: what the checks read */
    const double *edges;
    const int *cell_start_dev, *cell_items_dev, *edge_start_dev;        /* device copies: what the kernels read */
    const double *edges_dev;
} sn2_cut_table;
int sn2_cut_ws_words(const sn2_cut_table *table, size_t *words);
int sn2_cut_count(const float *cloud, const unsigned char *classification, const unsigned *drop, const sn2_cut_table *table, int *ws,
                  size_t ws_words, int *prefix, long long *parcel_start, void *stream);
int sn2_cut_fill(const float *cloud, const unsigned char *classification, const unsigned *drop, const sn2_cut_table *table,
                 int *prefix, const int *parcel_base, long sum_n, float *out, int *point_index, void *stream);

/* ---- Orthoimage colours (csrc/ortho.hip; the rule's functions: csrc/ortho_rules.h; host side ortho.py: colorize, colorize_ref): the
 * rows of the (10,T) cloud that no LiDAR sensor measures -- red, green, blue, near infrared, rows 3..6 -- looked up per point in
 * georeferenced orthoimages.  The reference's files had them painted on upstream, by tools that are not part of it: the rule is OURS.
 *
 * AN IMAGE is H x W pixels of C bands, north up, no rotation.  (x0, y0) is the OUTER corner of its top-left pixel (the x_min, y_max
 * of geotiff.write_bands, the corner of a GDAL geotransform), px, py > 0 the pixel sizes in metres.  All images of a set share the
 * pixel type (SN2_ORTHO_U8 / _U16 / _F32), C and the layout: SN2_ORTHO_CHUNKY (H,W,C) or SN2_ORTHO_PLANAR (C,H,W), contiguous.
 *
 * THE RULE, that of ortho.colorize_ref (numpy, fp64).  Point i has (x, y) = rows 0 and 1 of its column, fp32 widened to fp64.
 *   u = (x - x0) / px      v = (y0 - y) / py          every operation rounded to fp64 on its own
 *   inside  <=>  u >= 0 && u < W && v >= 0 && v < H    compared in fp64 before any conversion to int: NaN and inf are outside
 *   col = (int)floor(u)    row = (int)floor(v)
 * So the nearest pixel is the pixel whose area holds the point; a point exactly on an inner pixel edge belongs to the pixel to the
 * east or to the south; x == x0 + W px is outside.  The images are tried in list order: the point takes the FIRST image that
 * covers it and whose pixel is not nodata.  With has_nodata, a pixel is nodata iff every band SAMPLED there (band[0 .. n_map))
 * equals `nodata`, the sample widened to fp64.  A point no image serves keeps the values it had and is counted as missing.  A
 * served point gets, for k < n_map, row[k] = (float)pixel[band[k]] * scale: one fp32 product from the sample's exact fp32 value.
 * Rows 0 and 1 are read and never written; the rows written are distinct and in 3..9.  A cloud in a shifted frame (the origin= of
 * las.load_las / parcel.cut_parcels): the caller subtracts the shift in metres from x0, y0 in fp64 on the host; the kernel sees
 * one frame.  UNPINNED against GDAL / pdal: the side a tie at a pixel edge falls to, and the default scale (ortho.py).
 *
 * sn2_ortho_colorize: ONE launch over the columns col0 .. col0 + T of a (10, row_stride) fp32 cloud (a ParcelClouds arena is one
 *   such cloud: all K parcels in one launch).  The set travels BY VALUE in the kernel arguments, so an image's words are scalar
 *   loads.  A lane holds one point, a wave walks the image list: the ballot of the lanes not yet served that lie inside image s
 *   decides wave-uniformly whether image s is touched; a nodata pixel leaves its lane in the walk.  covered (T) uint8 or NULL:
 *   the 1-based index of the serving image, 0 = missing, element i for column col0 + i.  missing: int64 device word, ADDED to --
 *   one integer atomic per wave, the popcount of its unserved lanes.  No floating-point atomics: the same input gives the same bytes.
 *   Pixel addresses are 64-bit.
 * Before any launch the HOST copy of the set is checked, else SN2_EINVAL and no device work: set, cloud, missing non-NULL;
 *   1 <= S <= SN2_ORTHO_MAX_IMAGES; C >= 1; dtype and layout known; 1 <= n_map <= SN2_ORTHO_MAX_MAP; 0 <= band[k] < C; row[k] in
 *   3..9 and distinct; scale finite; nodata not NaN where has_nodata; per image: x0, y0 finite, px, py finite and > 0, W, H >= 1,
 *   pixels non-NULL; T >= 0, col0 >= 0, col0 + T <= row_stride.  SN2_ELIMIT: W H C >= SN2_ORTHO_MAX_SAMPLES for an image, or
 *   T >= 2^31.  T == 0 passes the checks and launches nothing. */
#define SN2_ORTHO_MAX_IMAGES 32
#define SN2_ORTHO_MAX_MAP 4
#define SN2_ORTHO_MAX_SAMPLES (1LL << 40)
#define SN2_ORTHO_U8 0
#define SN2_ORTHO_U16 1
#define SN2_ORTHO_F32 2
#define SN2_ORTHO_CHUNKY 0
#define SN2_ORTHO_PLANAR 1
typedef struct {
    double x0, y0, px, py;
    const void *pixels;                                                 /* device */
    int W, H;
} sn2_ortho_image;
typedef struct {
    int S, C, dtype, layout, n_map, has_nodata;
    int band[SN2_ORTHO_MAX_MAP], row[SN2_ORTHO_MAX_MAP];
    double nodata;
    float scale;
    int reserved;
    sn2_ortho_image image[SN2_ORTHO_MAX_IMAGES];
} sn2_ortho_set;
int sn2_ortho_colorize(float *cloud, long row_stride, long col0, long T, const sn2_ortho_set *set, unsigned char *covered,
                       long long *missing, void *stream);

/* ---- loss block of the timed training step: learning/loss_functions.py:9-57 combined as learning/train.py:58-62,
 *   total = get_absolute_loss(pred, gt) + m * get_NLL_loss(proba, pdf_all) + e * get_entropy_loss(proba)
 * pred (B,4) fp32 plot-wise coverages, gt (B,4) fp64, proba (R,4) fp32 pointwise class probabilities, pdf (R,3) fp64 the
 * KDE-mixture densities at the points' heights (the reference evaluates them on the CPU each step, :30-42; here sn2_kde_lookup
 * over the tables of sn2_kde_fit or any other tables, so they are an input).  partials: 2*SN2_LOSS_BLOCKS fp64 workspace.  out[4] = total, absolute, NLL,
 * entropy.  Backward: grad_total = device scalar d(objective)/d(total); writes dpred (B,4), dproba (R,4).
 * A term that is switched off is SKIPPED (not multiplied by zero) and its inputs may be absent -- what the reference's loop,
 * which calls the three functions one by one (learning/train.py:58-60), needs: B = 0: no absolute term (pred, gt, dpred
 * unused); m == 0: no NLL (pdf unused: rows that are no probability vectors give no 0 * log(<= 0) = NaN); e == 0: no entropy;
 * R = 0: no pointwise term (proba, pdf, partials, dproba unused).  The skipped components of out[] are 0. */
/* KDE-mixture densities at the points' heights -- KdeMixture.predict, learning/kde_mixture.py:65-70 (three scipy
 * interp1d(kind="linear") over one knot vector), which get_NLL_loss evaluates on the CPU for all B*N points every step
 * (learning/loss_functions.py:30-42).  cloud (B,C,N) fp32, height = cloud[:, z_channel, :] * z_max formed in fp32;
 * X (K) ascending knots and Y (3,K) the three tables, fp64; pdf (B*N,3) fp64 = what sn2_loss_* take.  Heights outside
 * [X[0], X[K-1]] (scipy raises there) give NaN.  The tables are an input: sn2_kde_fit's, or a reference-fitted mixture's. */
int sn2_kde_lookup(const float *cloud, int B, int C, int N, int z_channel, float z_max, const double *X, const double *Y,
                   int K, double *pdf, void *stream);
/* Fitting those tables -- KdeMixture.fit + evaluate_kdes, learning/kde_mixture.py:50-100 (three KDEpy FFTKDE(bw=0.1) over the
 * symmetrised heights, evaluated on one grid of 5000 points, scaled by their weight sums and divided by their common maximum).
 * KDEpy's FFTKDE is linear binning followed by a convolution with the sampled kernel; the estimator, with the grid margin and
 * the kernel truncation written out (all arithmetic fp64, no fused multiply-add where an index or a fraction is decided):
 *   z (n) fp32 heights in metres (cloud[2] before rescaling), all FINITE (the caller checks: a NaN or Inf is not detected here);
 *   sample   {-z_i} u {z_i} (get_sym_sorted_z; the sort does not change the result and is not done);
 *   weights  of a sample point, from a = |z| widened to fp64, strict inequalities (:54-58):
 *              w1 = a < 0.5 ? 1 : 0.05;   w2 = 0.5 < a < 1.5 ? 1 : 0.05;   w3 = a > 1.5 ? 1 : a > 0.5 ? 0.5 : 0.05;
 *   grid     zm = max |z|, A = zm + max(0.05 * 2 * zm, 5 bw), X = linspace(-A, A, K) (X[j] = j * dx - A, X[K-1] = A),
 *            dx = 2A / (K-1): the grid covers every fitted height, so sn2_kde_lookup of one never gives NaN;
 *   binning  a sample point s, t = (s - X[0]) / dx, j = min(floor(t), K-2), f = t - j: w (1-f) onto bin j, w f onto bin j+1;
 *   kernel   g[d] = exp(-(d dx)^2 / (2 bw^2)) / (bw sqrt(2 pi)), |d| <= L = min(floor(5 bw / dx), K-1);
 *   tables   Y[k][i] = sum_{|d| <= L, 0 <= i+d < K} bins_k[i+d] g[d], then all three divided by the one maximum over them
 *            (the weight normalisation of FFTKDE and evaluate_kdes' multiplication by the weight sums cancel).
 * X (K), Y (3,K) fp64 out, the layout sn2_kde_lookup takes.  ws: 8-byte aligned, SN2_KDE_FIT_WS_WORDS(K) 32-bit words, no
 * initialisation.  Four or five launches on `stream`, nothing read back, no state outside ws (capturable, re-entrant with a ws per
 * call).  DETERMINISTIC: no floating-point atomics -- the heights are cut into at most SN2_KDE_FIT_SLICES slices by n alone; a
 * bin of a slice is summed by one workgroup, every thread over a fixed subsequence of the slice in order, the threads in a fixed
 * tree, the slices in ascending order -- so the same z, bw, K give the same bytes on every call.  Against an fp64
 * evaluation of the same estimator the tables differ by the re-association of sums of non-negative terms and a few ulp of exp.
 * 1 <= n < 2^31, 2 <= K <= SN2_KDE_FIT_MAX_K (beyond: SN2_ELIMIT); bw > 0.  Every workgroup of the binning pass scans all n
 * heights of its slice (K/8 workgroups per slice): 5e5 heights at K = 5000 is what it is sized for. */
#define SN2_KDE_FIT_MAX_K 65536
#define SN2_KDE_FIT_ABS_SLOTS 256
#define SN2_KDE_FIT_SLICES 8
#define SN2_KDE_FIT_WS_WORDS(K) \
    (2 * ((4 + 3 * SN2_KDE_FIT_SLICES) * (size_t)(K) + 3 * (((size_t)(K) + 255) / 256)) + SN2_KDE_FIT_ABS_SLOTS)
size_t sn2_kde_fit_ws_words(int K);
int sn2_kde_fit(const float *z, long n, double bw, int K, void *ws, double *X, double *Y, void *stream);
#define SN2_LOSS_BLOCKS 1024
int sn2_loss_forward(const float *pred, const double *gt, int B, const float *proba, const double *pdf, int R, double m,
                     double e, double *partials, double *out, void *stream);
int sn2_loss_backward(const float *pred, const double *gt, int B, const float *proba, const double *pdf, int R, double m,
                      double e, const double *grad_total, float *dpred, float *dproba, void *stream);

/* Projection + loss of the training step (learning/train.py:54-62) in three launches instead of seven (round 5):
 * sn2_projected_loss_forward = sn2_plot_project_forward_pix (pixel ids `pix` from sn2_plot_pixels) + sn2_loss_forward in two
 * launches -- the scatter of the coverages and the pointwise loss sums side by side, then the per-plot finalisation whose last
 * workgroup adds the loss up -- and sn2_projected_loss_backward = sn2_loss_backward + sn2_plot_project_backward in one pass over
 * the points.  Same pred / arg / nocc / dcoverages / dproba bits as the separate calls; out[4] as sn2_loss_forward's to fp64
 * re-association.  keys: SN2_P2_KEY_PARTS(N)*B*D*D*3 u64; partials: SN2_PROJECTED_LOSS_WS doubles (no initialisation). */
#define SN2_PROJECTED_LOSS_WS (2 * 512 + 2)
int sn2_projected_loss_forward(const float *coverages, const int *pix, const float *proba, const double *pdf, const double *gt,
                               int B, int N, int D, double m, double e, unsigned long long *keys, int *arg, int *nocc,
                               float *pred, double *partials, double *out, void *stream);
int sn2_projected_loss_backward(const float *pred, const double *gt, int B, const float *proba, const double *pdf, int N, int D,
                                double m, double e, const double *grad_total, const int *arg, const int *nocc, const int *pix,
                                float *dcoverages, float *dproba, void *stream);

/* Validation pass -- the per-plot losses of learning/test.py:evaluate (:52-79), which runs with batch_size = 1: its loss_abs,
 * loss_log, loss_e and get_absolute_loss_by_strata are numbers of ONE plot each, averaged over plots afterwards.  For a batch
 * of B plots of N points in one call (two launches, no backward, no arg / nocc):
 *   coverages (B*N,4), proba (B*N,4) fp32; pix (B*N) the pixel ids of sn2_plot_pixels; pdf (B*N,3) fp64; gt (B,4) fp64;
 *   pred (B,4) fp32 out: the plot-wise coverages, the bits of sn2_plot_project_forward_pix for the same inputs;
 *   out (B,7) fp64, row b over plot b's N rows only: [total, absolute, NLL, entropy, abs_low, abs_med, abs_high] with
 *     abs_s = sqrt((pred[b,s] - gt[b,s])^2 + 1e-4) for s = columns 0, 2, 3, absolute = their mean, NLL = -mean_i log(sum_k p_k
 *     pdf_k) (p_ground = p0 + p1), entropy over columns 2, 3 as get_entropy_loss, total = absolute + m NLL + e entropy; absolute
 *     and NLL in fp64, the entropy terms in fp32 (as sn2_loss_forward): row b equals what sn2_projected_loss_forward returns for
 *     a batch that holds plot b alone, to fp64 re-association.
 *   A switched-off term is SKIPPED as in sn2_loss_forward and its component is 0: m == 0: pdf may be NULL; e == 0: no entropy;
 *   m == e == 0: proba may be NULL too.
 *   ws: 8-byte aligned workspace of sn2_plot_losses_ws_words(B, N, D) 32-bit words, no initialisation.
 * Contract:
 *   - BATCH INVARIANCE: row b of out and pred depends on plot b's rows, N, D, m, e only -- the same plot at another position,
 *     in a batch of another size, gives the same bytes.  (Every plot is cut into SN2_PLOT_LOSSES_SLICES(N) slices, a function
 *     of N alone; a slice is summed by one workgroup in a fixed order, a plot's slices are added in ascending order by one
 *     thread; no floating-point atomics, no partial sum shared between plots.)
 *   - run-to-run identical bytes;
 *   - a NaN (a height outside the KDE tables: sn2_kde_lookup marks it NaN) stays in its own plot's row;
 *   - any B >= 1, N >= 1 with B*N < 2^31, D*D <= 2025 (as the other projection entry points); beyond: SN2_ELIMIT
 *     (sn2_plot_losses_ws_words returns 0); NULL pointers, non-positive sizes: SN2_EINVAL -- both before anything is launched. */
#define SN2_PLOT_LOSSES_SLICE_ROWS 2048
#define SN2_PLOT_LOSSES_SLICES(N) \
    (((N) + SN2_PLOT_LOSSES_SLICE_ROWS - 1) / SN2_PLOT_LOSSES_SLICE_ROWS < 1 ? 1 : \
     (((N) + SN2_PLOT_LOSSES_SLICE_ROWS - 1) / SN2_PLOT_LOSSES_SLICE_ROWS > 64 ? 64 : ((N) + SN2_PLOT_LOSSES_SLICE_ROWS - 1) / SN2_PLOT_LOSSES_SLICE_ROWS))
size_t sn2_plot_losses_ws_words(int B, int N, int D);
int sn2_plot_losses(const float *coverages, const int *pix, const float *proba, const double *pdf, const double *gt, int B, int N,
                    int D, double m, double e, void *ws, float *pred, double *out, void *stream);

/* Cross-validation report (csrc/indicators.hip) -- what learning/accuracy.py makes of the folds' per-plot predictions:
 * calculate_performance_indicators_V1/V2/V3 (MAE, MAE2, MAE3, Acc, Acc2, Acc3), the class indices of compute_confusion_matrix,
 * plain and after adjust_predictions_based_on_margin, and the sums that DataFrame.mean() and confusion_matrix() take over them.
 *   pred (P,4) fp32: low, soil, medium, high, as sn2_plot_losses' pred; gt (P,4) fp64.  Strata s = columns 0, 2, 3 (veg_b,
 *   veg_moy, veg_h).  EVERY comparison and difference is fp64; pred is widened exactly (the reference ran on NumPy < 1.24, where
 *   a float32 scalar against a Python float compares in fp64).
 * Constants (accuracy.py:13-42), each the double nearest its decimal literal (what floor(x * 100 + .5) / 100 yields):
 *   centres c  = {0, .10, .25, .33, .50, .75, .90, 1};
 *   class k has the borders lo = {0, .05, .18, .29, .42, .63, .83, .95}[k], hi = {.05, .18, .29, .42, .63, .83, .95, 1.05}[k];
 *   the margin is 0.1.
 * Closest class (get_closest_class_center_index): class(y) = the FIRST k, ascending, that minimises fabs(c[k] - y), each
 *   difference rounded once to fp64; on an exact tie the lower class wins (y = 0.05 -> 0, 0.625 -> 4; 0.95 -> 6, 0.175 -> 1 and
 *   0.825 -> 5 are no ties in fp64: the two differences differ in their last bits): this library's
 *   rule -- the insertion sort inside NumPy < 1.25's argsort gives it, later NumPy versions pin no tie.  Every difference NaN: 0.
 * Ground truth: relabel != 0 replaces gt[p,s] by c[class(gt[p,s])] (main.py:102-109); then, always, g = rint(gt * 1000) / 1000
 *   (the round(3) at the head of every calculate_performance_indicators_V*).  kt = the k with g == c[k] (fp64 equality), or -1.
 * Per plot and stratum, p = (double)pred:
 *   error  = fabs(p - g);                                     acc  = lo[kt] <= p && p <= hi[kt];
 *   error2 = acc ? 0 : fmin(fabs(lo[kt] - p), fabs(hi[kt] - p));   acc2 = (lo[kt] - 0.1) <= p && p <= (hi[kt] + 0.1);
 *   L = lo[max(kt-1,0)], H = hi[min(kt+1,7)]:  acc3 = L <= p && p <= H;  error3 = acc3 ? 0 : fmin(fabs(L - p), fabs(H - p)).
 *   The aggregates x_b_and_moy = (x_b + x_moy) / 2 and x_all = ((x_b + x_moy) + x_h) / 3, added in that order, with the
 *   reference's two oddities kept AS WRITTEN:  acc_all = (acc_b + acc_moy) / 2 (accuracy.py:169: two strata, not three) and
 *   error3_all = ((error3_b + error2_moy) + error3_h) / 3 (accuracy.py:242: error2 of the medium stratum).
 *   A row with some kt == -1 (a continuous ground truth; the reference raises KeyError there): every class-based entry of that
 *   row -- columns 5 .. 29 -- is NaN.
 * Outputs:
 *   rows (P,SN2_CV_COLUMNS) fp64, 16-byte aligned: V1's ten columns (error_veg_b, error_veg_moy, error_veg_h,
 *     error_veg_b_and_moy, error_all, acc_veg_b, acc_veg_moy, acc_veg_h, acc_veg_b_and_moy, acc_all), then V2's ten (error2_*,
 *     acc2_*), then V3's ten (error3_*, acc3_*): the order in which the reference adds them to its frame;
 *   cls (P,9) int32: class(g) per stratum (the confusion matrices' true class: kt wherever kt >= 0), class(p) per stratum, and per
 *     stratum the class of the margin-adjusted prediction (p := g where the row's acc2 entry == 1, so class(g) there; class(p)
 *     elsewhere, a row with some kt == -1 included: its acc2 entries are NaN);
 *   stats, SN2_CV_STATS_DOUBLES doubles: sum[SN2_CV_COLUMNS] over the plots; count[SN2_CV_COLUMNS] = the entries that are not NaN
 *     (DataFrame.mean() skips NaN: mean = sum / count); the confusion counts (2,3,8,8) = [plain | margin-adjusted][stratum]
 *     [true class][predicted class]; the number of rows with some kt == -1.  Counts are integer-valued doubles (exact: P < 2^53).
 *   ws: 8-byte aligned, SN2_CV_WS_WORDS(P) 32-bit words (sn2_cv_indicators_ws_words), no initialisation.
 * Contract:
 *   - DETERMINISTIC, no floating-point atomics, no last-workgroup-out hand-off: the plots are cut into slices of
 *     SN2_CV_SLICE_PLOTS, a function of nothing else; one workgroup sums a slice in a fixed order (a butterfly inside each wave,
 *     the waves in ascending order) into the slice's own block of ws; a SECOND launch of one workgroup adds the slices in
 *     ascending order and writes stats.  Confusion counts: integer LDS atomics inside a slice, integer sums over the slices.
 *     The same inputs give the same bytes of rows, cls and stats, whatever the grid;
 *   - rows and cls of plot p depend on plot p alone: the same plot at another position, at another P, gives the same bytes;
 *   - a NaN prediction stays in its own row: its error entries are NaN and counted out of sum and count, its accuracies are 0
 *     (every comparison fails), its class is 0;
 *   - 1 <= P <= SN2_CV_MAX_PLOTS (beyond: SN2_ELIMIT, and the size helper then gives 0 words); NULL or misaligned pointers,
 *     P < 1: SN2_EINVAL -- both before anything is launched.  Two launches on `stream`, nothing read back, capturable.
 *   - plain C++, single operations: no product feeds a sum, so nothing is contracted into an FMA.
 * Not on the training hot path: it runs once per cross-validation, over a table of a few thousand to a few million rows.
 * (The size helper returns its value through a pointer, as sn2_atlas_finalize_ws_words does: tests/test_cabi.py and
 * tests/test_parcel_report_host.py hold the `size_t` and `extern size_t` declarations of this header to closed lists.) */
#define SN2_CV_SLICE_PLOTS 1024
#define SN2_CV_COLUMNS 30
#define SN2_CV_STATS_DOUBLES (2 * SN2_CV_COLUMNS + 2 * 3 * 8 * 8 + 1)
#define SN2_CV_MAX_PLOTS (1 << 24)
#define SN2_CV_SLICES(P) (((size_t)(P) + SN2_CV_SLICE_PLOTS - 1) / SN2_CV_SLICE_PLOTS)
#define SN2_CV_WS_SLICE_WORDS (2 * SN2_CV_COLUMNS + (SN2_CV_COLUMNS + 2) + 2 * 3 * 8 * 8)
#define SN2_CV_WS_WORDS(P) (SN2_CV_SLICES(P) * SN2_CV_WS_SLICE_WORDS)
int sn2_cv_indicators_ws_words(int P, size_t *words);
int sn2_cv_indicators(const float *pred, const double *gt, int P, int relabel, double *rows, int *cls, double *stats, void *ws,
                      void *stream);

/* ---- optimiser step of the timed training step -- torch.optim.Adam as configured in learning/train.py:180-185
 * (L2 weight decay added to the gradient), on flat buffers; grad_scale multiplies the gradient first (1/world).
 * The learning rate is a by-value argument here: a launch captured into a hipGraph keeps the rate of its capture.  The ABI keeps
 * this form (same kernel as sn2_adam_step_dev with no device word and no meter; same bits). */
int sn2_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int *step_dev /* two device ints: {steps taken so far (incremented here), 0} */,
                  float grad_scale, void *stream);

/* The same step with the learning rate read from ONE device word, *lr_dev (fp32), at launch time on the device: whoever writes
 * that word in stream order between two launches -- or between two replays of a graph that holds this launch -- sets the rate of
 * the next step (torch's StepLR, learning/train.py:152,185).  For the same rate value the results are sn2_adam_step's, bit for bit.
 * Epoch meter (learning/train.py:68-79 reports the epoch means of the loss terms): n_terms > 0 adds this step's loss terms,
 * terms[0 .. n_terms) (fp64, written by kernels earlier on the stream), to meter[0 .. n_terms) and 1 to meter[SN2_METER_TERMS];
 * meter = SN2_METER_TERMS + 1 doubles = the sums, then the number of steps added.  The ONE thread of the launch that advances
 * step_dev does it, with plain loads and stores: no atomics, no launch of its own.  n_terms == 0: terms and meter may be NULL and
 * are not touched.  SN2_EINVAL before any device work: lr_dev NULL, n_terms outside 0 .. SN2_METER_TERMS, n_terms > 0 with terms
 * or meter NULL, and everything sn2_adam_step refuses. */
#define SN2_METER_TERMS 4
int sn2_adam_step_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int n, const float *lr_dev, float beta1,
                      float beta2, float eps, float weight_decay, int *step_dev, float grad_scale, const double *terms, int n_terms,
                      double *meter, void *stream);

/* ==== the whole network behind ONE call per pass (round 5) ===================================================
 * PointNet2.forward of the reference (model/point_net2.py:106-153) is ~25 of the entry points above in a fixed order, and
 * loss.backward() through it (learning/train.py:64) ~10 more.  A host that issues them one by one from Python spends more
 * time between the launches than the device needs for the kernels (the reference's training loop as written: 3.5 ms per step
 * over ~2.4 ms of kernels).  sn2_net_geometry / sn2_net_forward / sn2_net_backward issue the same entry points, with the same
 * descriptors, in the same order, from inside the library: one call each.  Nothing else changes: every buffer is the
 * caller's, nothing is allocated, freed or synchronised, all launches go to `stream` (and, for the forked geometry pass, to
 * the caller's side streams, ordered by the events of a caller-owned context).  Results are those of the separate calls, bit
 * for bit (tests/test_gpu_executor.py).
 *
 * The reference architecture only (model/point_net2.py:81-99): SA1 MLP[11,16,16], SA2 MLP[19,32], global SA MLP[35,64],
 * FP3 MLP[96,64] k=1, FP2 MLP[80,34] k=3, FP1 MLP[42,34] k=3, lin1 34->16, lin2 16->5 -- and the same architecture over
 * F = 4 point features instead of 8 (n_input_feats = 6, :77-90): SA1 MLP[7,16,16], FP1 MLP[38,34], rows0 (B*N,8).  F is read off
 * the model: sa1[0].cin - 3, and fp1.cin must be 34 + F. */

/* one (Linear -> ReLU -> BatchNorm1d) block of the model: its parameters and buffers (device), and where its four gradients
 * live inside the flat parameter gradient (offsets in floats; parameters() order of the reference module) */
typedef struct sn2_net_layer {
    int cin, cout;
    const float *W, *b, *gamma, *beta;
    float *running_mean, *running_var;
    long long *num_batches_tracked;      /* or NULL */
    int gW, gb, ggamma, gbeta;
    int mma_bf16;                        /* sn2_block.mma_bf16 of this block */
} sn2_net_layer;

typedef struct sn2_net_model {
    sn2_net_layer sa1[2], sa2, sa3, fp3, fp2, fp1;      /* model/point_net2.py:84-93 */
    const float *lin1_W, *lin1_b, *lin2_W, *lin2_b;     /* :95-99 */
    int g_lin1_W, g_lin1_b, g_lin2_W, g_lin2_b;
    int n_flat;                          /* length of the flat parameter (and gradient) vector: 14 997 */
    float r1_sq, r2_sq;                  /* fp32(r*r) of the two ball queries, r*r evaluated in double (sn2_ball_query) */
    int max_neighbors;                   /* model/point_net2.py:24 (2000) */
    float drop_p;                        /* args.drop (:142) */
    int fuse_global_level;               /* training: sn2_global_level_forward where its limits allow (else the separate calls) */
    int fuse_eval_head;                  /* eval: sn2_fp_head_eval instead of sn2_fp_forward + sn2_head_forward */
    int source_side;                     /* hand out sn2_fp.src_ws (the per-point layer's source-side form) */
    int fps_waves_shared, fps_waves_many;/* sn2_fps_waves of the level-1 FPS of a pass that shares the chip (<= 32 plots / more) */
} sn2_net_model;

typedef struct sn2_net_dims {
    int B, N, M1, M2;                    /* plots, points per plot, centroids of the two levels (ceil(fp32(n) * fp32(ratio))) */
    int cap1, cap2;                      /* row stride of nbr1 / nbr2: min(max_neighbors, N) / min(max_neighbors, M1) */
    int act_bf16;                        /* the per-point activation buffers h1 / dy1 / du1 are bfloat16 (sn2_fp.act_bf16) */
    int p2_diam_pix;                     /* > 0: the geometry pass also computes the pixel ids of sn2_plot_pixels (geo.p2_*) */
} sn2_net_dims;

/* The position-only tables of one batch -- what SAModule / FPModule obtain from torch_cluster in the reference
 * (model/point_net2.py:22-25, 63) -- and the two input-only pieces a geometry pass may also produce.  Shapes as in the
 * entry points that fill them.  sn2_net_geo_carve lays them out in one caller-owned arena. */
typedef struct sn2_net_geo {
    const float *xyz;                                    /* (B,3,N): the batch's positions */
    int *idx1; float *pos1_soa, *pos1_aos; int *ws1;     /* sn2_fps level 1; ws1 = NULL where the FPS fills no workspace */
    int *nbr1, *cnt1; unsigned long long *tot1; int *ord1;
    int *idx2; float *pos2_soa, *pos2_aos; int *ws2;
    int *nbr2, *cnt2; unsigned long long *tot2; int *ord2;
    const float *pos3;                                   /* (B,3,1) zeros: the global feature sits at the origin (:41) */
    int *knn3_idx; float *knn3_w;                        /* (B*M2,3) */
    int *knn2_idx; float *knn2_w;                        /* (B*M1,3) */
    int *knn1_idx; float *knn1_w;                        /* (B*N,3)  */
    float *inv3, *inv2, *inv1;                           /* SN2_INTERP_WS_WORDS each */
    int *nn_ws2, *nn_ws1;                                /* SN2_THREE_NN_XY_WS_WORDS or NULL (full scan) */
    const int *rank1;                                    /* sn2_fp.row_perm of FP1 or NULL */
    float *rows0;                                        /* (B*N,F+4) sn2_pack_rows_feat, F = model.sa1[0].cin - 3 (8: (B*N,12)) */
    int *p2_pix; float *p2_mm;                           /* sn2_plot_pixels or NULL */
} sn2_net_geo;

/* The buffers of one forward pass (kept for its backward pass when training). */
typedef struct sn2_net_act {
    float *aux;                          /* 4 * 260 floats: (a, c, mean, invstd) of the seven blocks, in model order */
    float *stats;                        /* SN2_STAT_SLOTS * 2 * 260 floats: their statistic slots */
    float *ext1; int *arg1; float *x1;   /* (B*M1,16) */
    float *ext2; int *arg2; float *x2;   /* (B*M2,32) */
    float *h_sa3, *h3;                   /* (B*M2,64) */
    float *x3; int *arg3;                /* (B,64) */
    float *h2;                           /* (B*M1,36) */
    void *h1;                            /* (B*N,36) fp32 / bfloat16 rows; unused by the fused eval pass */
    float *src_ws1, *src_ws2;            /* SN2_FP_SRC_WS_WORDS of FP1 / FP2, or NULL (sn2_fp.src_ws) */
    float *cov, *proba;                  /* OUT (B*N,4): coverages_pointwise, proba_pointwise -- set by the caller, not carved */
    const int *drop_mask;                /* sn2_head.drop_mask or NULL -- set by the caller */
    float *bwd_arena; long bwd_arena_words; /* set by the caller or NULL / 0 (training forward): the arena of the backward pass that will
                                            follow (sn2_net_bwd.arena, arena_words): the forward's last kernel clears it, and that
                                            backward pass is told so (sn2_net_bwd.arena_is_zero) */
} sn2_net_act;

/* The buffers of one backward pass: `arena` (zero-filled INSIDE sn2_net_backward) = SN2_NET_GRAD_IMAGES images of the flat
 * parameter gradient, image stride = n_flat rounded up to 64 floats, followed by the accumulate-into buffers; the rest is scratch. */
#define SN2_NET_GRAD_IMAGES 32
typedef struct sn2_net_bwd {
    const float *dcov, *dproba;          /* IN (B*N,4) each, either may be NULL -- set by the caller */
    float *arena; long arena_words;
    int images, image_stride;
    float *dy2, *dy3, *dx1, *dx2, *dx3, *dy_sa3;
    float *sa1_ws;                       /* sn2_sa.bwd_ws of SA1 (SN2_SA_BWD_WS_WORDS), the arena's last buffer */
    void *dy1, *du1;                     /* (B*N,36) rows of the activation type */
    float *du2, *du3;                    /* (B*M1,64), (B*M2,64) */
    int *bn_ok;                          /* 4 words */
    float *src_ws1, *src_ws2;
    int defer_grad_reduce;               /* set by the caller: leave the images unfolded (sn2_adam_step_images folds them) */
    int arena_is_zero;                   /* set by the caller: the forward pass cleared `arena` (sn2_net_act.bwd_arena) and nothing has
                                            touched it since: sn2_net_backward does not clear it again */
    int frozen_stats;                    /* set by the caller: the forward pass ran with io.training = SN2_BN_FROZEN_KEEP (every
                                            block's sn2_block.frozen_stats) */
    unsigned long long *gl_xchg; unsigned *gl_ctl;   /* set by the caller: sn2_global_level_backward's exchange area (its own, not
                                            sn2_net_io's), or NULL: the separate launches */
    const sn2_loss_grad *loss;           /* set by the caller, or NULL: gradients come in dcov / dproba as before.  Set: both of
                                            those must be NULL and sn2_head_loss_route must say yes (the caller asks first), else
                                            SN2_EINVAL; handed to the head backward (sn2_head.loss) */
} sn2_net_bwd;

#define SN2_NET_FORK 1          /* geometry: level-2 chain on io.stream_b, per-point 3-NN chain on io.stream_c (needs io.ctx) */
#define SN2_NET_SHARED 2        /* geometry: the pass shares the chip with other kernels (level-1 FPS: model.fps_waves_*) */
#define SN2_NET_INVERTED 4      /* geometry: also the inverted 3-NN tables (only a backward pass reads them) */
#define SN2_NET_DEFER_JOIN 8    /* geometry (with FORK): return without joining; the forward pass that follows joins */
#define SN2_NET_INPUT_ONLY 16   /* geometry: also rows0 (and the P2 pixel ids when dims.p2_diam_pix > 0) from io.cloud */
#define SN2_NET_HAS_ROWS0 32    /* forward: geo.rows0 is already packed */
#define SN2_NET_JOIN_PENDING 64 /* forward: the geometry pass on this ctx was launched with DEFER_JOIN: SA2 waits for chain b, FP1 for chain c */
#define SN2_NET_WITH_GEOMETRY 128 /* forward: run the geometry pass first (forked when io.ctx and the side streams are given), the
                                     row packing beside the level-1 FPS */
#define SN2_NET_HAS_INVERTED 256 /* forward (training): geo.inv* are already built (else they are built here) */
#define SN2_NET_CLOUD10 512     /* geometry, forward: io.cloud has the reference's ten rows although the model reads four features
                                   (sn2_pack_rows_feat's (10, 4) form); without it io.cloud is (B,F+2,N) */

typedef struct sn2_net_io {
    const float *cloud;                  /* (B,F+2,N) features on the device ((B,10,N) under SN2_NET_CLOUD10), or NULL where not needed */
    const int *fps_start;                /* (2,B) start indices of the two FPS calls, or NULL (= 0) */
    unsigned *fps_status;                /* sn2_fps_status's word or NULL */
    unsigned long long *gl_xchg; unsigned *gl_ctl;   /* sn2_global_level_forward's exchange area, or NULL: separate launches */
    void *stream_b, *stream_c, *stream_pack;         /* side streams of a forked pass (hipStream_t), or NULL */
    void *ctx;                           /* sn2_net_ctx_create: the events that order them, or NULL (no fork) */
    int flags;                           /* SN2_NET_* */
    int training;                        /* model.training (0 / 1), or SN2_BN_FROZEN_KEEP: eval mode with a backward to come */
    const int *fps_live;                 /* (B) sn2_fps_live's n_live of the level-1 FPS, or NULL (= N) */
    int *fps_live1;                      /* (B) scratch: level 1's n_live_out = level 2's n_live; needed when fps_live is given */
} sn2_net_io;

/* events of a forked geometry pass: created once by the caller (one per model and device), used by one pass at a time */
int sn2_net_ctx_create(void **ctx);
int sn2_net_ctx_destroy(void *ctx);
/* Lay the tables / buffers out in caller-owned arenas: every pointer of *out = base + its offset (256-byte aligned); *bytes = the
 * arena's size.  base = NULL: the pointers ARE the offsets (a host can cache them per shape).  Fields marked "set by the
 * caller" are left NULL. */
int sn2_net_geo_carve(const sn2_net_model *m, const sn2_net_dims *d, void *base, sn2_net_geo *out, size_t *bytes);
int sn2_net_act_carve(const sn2_net_model *m, const sn2_net_dims *d, int training, void *base, sn2_net_act *out, size_t *bytes);
int sn2_net_bwd_carve(const sn2_net_model *m, const sn2_net_dims *d, void *arena_base, void *scratch_base, sn2_net_bwd *out,
                      size_t *arena_bytes, size_t *scratch_bytes);
/* the position-only kernels of one batch: FPS x2, ball query x2, SA work items x2, 3-NN x3 [, inverted tables x3, rows0, P2 ids]
 * -- PointNet2._geometry; replaces the torch_cluster calls of model/point_net2.py:22-25, 63 */
int sn2_net_geometry(const sn2_net_model *m, const sn2_net_dims *d, const sn2_net_geo *g, const sn2_net_io *io, void *stream);
/* PointNet2.forward, model/point_net2.py:131-151 (training or eval by io->training) */
int sn2_net_forward(const sn2_net_model *m, const sn2_net_dims *d, const sn2_net_geo *g, const sn2_net_act *a,
                    const sn2_net_io *io, void *stream);
/* its backward pass (loss.backward(), learning/train.py:64): every parameter gradient into image 0 of b->arena */
int sn2_net_backward(const sn2_net_model *m, const sn2_net_dims *d, const sn2_net_geo *g, const sn2_net_act *a,
                     const sn2_net_bwd *b, void *stream);

/* sn2_grad_reduce + sn2_adam_step in one launch, for a step with no exchange between them: grad_images = the `replicas` images
 * of the flat gradient (image stride `stride` floats); image 0 holds the folded gradient afterwards (same additions, same order
 * as sn2_grad_reduce).  sn2_net_bwd.defer_grad_reduce makes sn2_net_backward leave the images unfolded for it.  The learning
 * rate is by value, as in sn2_adam_step: fixed at capture time. */
int sn2_adam_step_images(float *param, float *grad_images, int replicas, int stride, float *exp_avg, float *exp_avg_sq, int n,
                         float lr, float beta1, float beta2, float eps, float weight_decay, int *step_dev, float grad_scale,
                         void *stream);
/* sn2_adam_step_images with the learning rate in a device word and the optional epoch meter, exactly as sn2_adam_step_dev is to
 * sn2_adam_step (same bits for the same rate; the same additional SN2_EINVAL cases). */
int sn2_adam_step_images_dev(float *param, float *grad_images, int replicas, int stride, float *exp_avg, float *exp_avg_sq, int n,
                             const float *lr_dev, float beta1, float beta2, float eps, float weight_decay, int *step_dev,
                             float grad_scale, const double *terms, int n_terms, double *meter, void *stream);

/* ==== Routes =================================================================================================
 * Which kernel a size takes, and therefore which workspaces exist, stated ONCE: each predicate is host-only arithmetic (no HIP
 * call, no device work; 0 or 1), lives beside the dispatch it governs, and is what that dispatch itself, sn2_net_* and the Python
 * host all ask.  A caller still ANDs in its own settings and whether it holds the workspace. */
/* sn2_fps* FILLS order_ws for these sizes (given a 16-byte aligned one): the bucketed kernels -- more than 2048 points per plot
 * (at most 131 072), unless the plots are many (B > 32) and small (N <= 4096), M > 16, B*N a multiple of 4.  Otherwise the
 * brute-force kernels run and the workspace is NOT touched: nobody may hand it to sn2_ball_query / sn2_three_nn. */
int sn2_fps_fills_ws(int B, int N, int M);
/* Which kernel sn2_fps_live (and so sn2_fps, sn2_fps_waves, sn2_fps_status) launches: the plan the entry point itself runs before
 * its first launch, with have_ws = "a 16-byte aligned order_ws was given" and cus = the device's compute units.  0 and *out, or
 * the negative code of the entry point (no pointer but `out` is dereferenced): SN2_EINVAL for B, N, M <= 0, M > N or an unknown
 * `waves`, then SN2_ELIMIT for more than 32 768 points without a bucketed route (which ends at 131 072).
 *   BRUTE    !(have_ws && sn2_fps_fills_ws): fps_kernel<rung = points per thread, 64 * nw threads> -- 1, 2, 4 points on 256 threads
 *            up to 1024 points, then 2 .. 32 on 1024 threads (32: the form that keeps z in LDS); more than 32 plots of 2049 ..
 *            4096 points: 16 points on 256 threads.  `waves` only has to be a known code.
 *   CLUSTER  fps_cluster_kernel<rung, nw, p, lds_points>: p workgroups of nw waves per plot, then a REPAIR launch (SPEC with 16
 *            waves and `repair` slots, gated by the workspace's control words).  Asked for with waves = 32 + p (16 waves) or
 *            64 + p (8 waves), p = 2, 4, 8, and taken where it FITS: B * p <= cus, 2 * p * nw <= buckets <= 512 * p, buckets =
 *            ceil(N / 64); waves = 0 takes the first of p = 8, 4, 2 with 8 waves that fits.  rung = the slots per wave that hold
 *            ceil(buckets / p) buckets: 2, 4 .. 64 (16 waves: .. 32).  lds_points: the workgroup's points stay in LDS (they
 *            and the sample log fit 150 KB, at most 96 slots per workgroup).
 *   SPEC     fps_spec_kernel<rung, nw>: one workgroup per plot.  waves = 16, 8, 4; 0 and the cluster codes where nothing fits
 *            (16 waves).  4 waves exist up to 16 384 points and become 8 above, 8 exist up to 32 768 and become 16.  rung = the
 *            slots per wave that hold the buckets, at least 4 / 8 / 32 with 16 / 8 / 4 waves (.. 128 / 64 / 64).
 *   ROUND    fps_bucket_kernel<rung, 16>: waves = 1, one sample per arg-max round; rung as SPEC's with 16 waves.
 * Same indices whichever runs. */
#define SN2_FPS_FORM_BRUTE 0
#define SN2_FPS_FORM_ROUND 1
#define SN2_FPS_FORM_SPEC 2
#define SN2_FPS_FORM_CLUSTER 3
typedef struct {
    int form;       /* SN2_FPS_FORM_* */
    int nw;         /* waves per workgroup */
    int p;          /* workgroups per plot: 1 unless CLUSTER */
    int rung;       /* the template rung: bucket slots per wave (bucketed forms), points per thread (BRUTE) */
    int lds_points; /* CLUSTER: the workgroup's points stay in LDS */
    int repair;     /* CLUSTER: slots per wave of the repair launch that follows; 0: no repair launch */
    int fills_ws;   /* order_ws is filled (every form but BRUTE) */
} sn2_fps_route_t;
int sn2_fps_route(int B, int N, int M, int waves, int have_ws, int cus, sn2_fps_route_t *out);
/* the grid search of sn2_three_nn_xy (and of sn2_three_nn with ws + dst_fps_ws) applies: 128 <= S <= 8192 sources and T > 2048
 * targets; otherwise the full scan of sn2_three_nn runs */
int sn2_three_nn_uses_grid(int S, int T);
/* a dense-row block of R rows takes the 64-row matrix-core kernels of sn2_fp_forward / sn2_fp_backward in a TRAINING pass: its
 * per-workgroup statistic slots bound the rows, ceil(R / 64) <= SN2_STAT_SLOTS.  Only those kernels take bfloat16 operands
 * (sn2_block.mma_bf16). */
int sn2_fp_rows_small(long R);
/* sn2_fp.src_ws is used (the source-side form): 0 < cb <= 16, cb a multiple of 4, and more rows than sn2_fp_rows_small takes --
 * or force != 0 (sn2_fp_head_eval, which has no other form).  Only this form keeps bfloat16 rows (sn2_fp.act_bf16). */
int sn2_fp_source_side(long R, int cb, int force);
/* Which of its three kernel forms sn2_fp_forward (pass = its `training` argument, 0 / 1 / 2) or sn2_fp_backward (pass = 3)
 * takes for a descriptor: the plan those entry points themselves run before their first launch, so SN2_FP_FORM_*, or the
 * negative code the entry point would return (no pointer is dereferenced).
 *   SPLIT        the 64-row matrix-core kernels; the only form with bfloat16 operands (sn2_block.mma_bf16)
 *   SOURCE_SIDE  everything linear in the interpolation once per source row, in sn2_fp.src_ws; the only form with bfloat16
 *                rows (sn2_fp.act_bf16) and permuted gradient rows (sn2_fp.row_perm)
 *   DENSE        the grid-stride row kernels
 * Forward: SPLIT where sn2_fp_rows_small(B*R); else SOURCE_SIDE where sn2_fp_source_side(B*R, cb, 0) holds on a k-NN block that
 * has src_ws, 4-float aligned skip rows, src rows padded to 4 floats, h_stride = cout rounded up to 4 and B*R*3 < 2^31; else
 * DENSE -- but SPLIT in an eval pass (0), which writes no statistic slots.  Backward: the same rule without the eval case, and
 * SOURCE_SIDE also needs dsrc, du_scratch and scatter_ws given and dskip NULL: without them the block falls back to DENSE. */
#define SN2_FP_FORM_SPLIT 0
#define SN2_FP_FORM_SOURCE_SIDE 1
#define SN2_FP_FORM_DENSE 2
int sn2_fp_form(const sn2_fp *p, int pass);
/* sn2_net_forward / sn2_net_backward take the one-launch global level (bf16: either block has sn2_block.mma_bf16): at most
 * SN2_GLOBAL_MAX_PLOTS plots, fp32 operands; backward also batch statistics (frozen == 0) and M2 <= SN2_GLOBAL_BWD_MAX_ROWS */
int sn2_global_level_forward_route(int B, int bf16);
int sn2_global_level_backward_route(int B, int M2, int frozen, int bf16);
/* sn2_head_backward takes a loss-gradient descriptor (sn2_head.loss, sn2_net_bwd.loss) for B plots of N points on a D x D grid:
 * B <= SN2_HEAD_LOSS_MAX_PLOTS, B*N < 2^31 rows, D*D <= 2025 cells (what the projection covers).  Otherwise the caller runs
 * sn2_projected_loss_backward and hands the two gradients over */
int sn2_head_loss_route(int B, int N, int D);

#ifdef __cplusplus
}
#endif
#endif /* STRATA_HIP_H */
