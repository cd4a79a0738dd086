"""ctypes binding of libstrata_hip.so (include/strata_hip.h).  No torch C++ extension, no fallback: if the library
is missing the product path raises."""
import ctypes
import functools
import os
from ctypes import POINTER, Structure, c_double, c_float, c_int, c_long, c_longlong, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libstrata_hip.so")

# Every scalar constant of include/strata_hip.h that the Python host uses, under its macro's name.  tests/test_cabi.py prints
# the macros with a C compiler and compares: this block is the only place a value of the header is written again.
# (SN2_VERSION: added entry points keep the version.)
CONSTANTS = {
    "SN2_VERSION": 102, "SN2_EINVAL": -1, "SN2_ELIMIT": -2,
    "SN2_MAX_NEIGHBORS": 2000, "SN2_STAT_SLOTS": 1024, "SN2_BN_FROZEN_KEEP": 2,
    "SN2_FPS_WS_GRID_WORDS": 4104, "SN2_FPS_WS_CTL_WORDS": 32,
    "SN2_SUBSAMPLE_LDS": 1, "SN2_SUBSAMPLE_GLOBAL": 2, "SN2_SUBSAMPLE_COARSE": 4, "SN2_SUBSAMPLE_LDS_MAX": 16384,
    "SN2_SA_BWD_WS_WORDS": 32 * 2 * 16 * 12,
    "SN2_GLOBAL_MAX_PLOTS": 28, "SN2_GLOBAL_CTL_WORDS": 8, "SN2_GLOBAL_BWD_MAX_ROWS": 256,
    "SN2_GLOBAL_BWD_XCHG_WORDS": 2 * 28 * 128, "SN2_GLOBAL_BWD_CTL_WORDS": 64,
    "SN2_MOSAIC_HIST_WORDS": 10004, "SN2_MOSAIC_CROP_MAX_BANDS": 8, "SN2_MOSAIC_CROP_MAX_EDGES": 1 << 20,
    "SN2_MOSAIC_CROP_MAX_BLOCKS": 2048, "SN2_ATLAS_CANVAS_COLS": 8, "SN2_ATLAS_SEG_COLS": 8, "SN2_ATLAS_FINALIZE_MAX_BLOCKS": 1024,
    "SN2_ATLAS_FINALIZE_CANVAS_WORDS": 10004 + 2 * 1024, "SN2_KDE_FIT_MAX_K": 65536, "SN2_LOSS_BLOCKS": 1024, "SN2_PROJECTED_LOSS_WS": 2 * 512 + 2,
    "SN2_NET_GRAD_IMAGES": 32, "SN2_METER_TERMS": 4, "SN2_PARCELS_COLS": 16, "SN2_PARCELS_BBOX_CHUNK": 4096,
    "SN2_CV_SLICE_PLOTS": 1024, "SN2_CV_COLUMNS": 30, "SN2_CV_STATS_DOUBLES": 2 * 30 + 2 * 3 * 8 * 8 + 1, "SN2_CV_MAX_PLOTS": 1 << 24,
    "SN2_CV_WS_SLICE_WORDS": 2 * 30 + 32 + 2 * 3 * 8 * 8, "SN2_POINTS_ACC_WORDS": 9,
    "SN2_ADM_WS_HEAD_WORDS": 32, "SN2_ADM_WS_WORDS_PER_PIXEL": 6,
    "SN2_LAS_COORDS_REFERENCE": 0, "SN2_LAS_COORDS_HEADER": 1, "SN2_LAS_ROWS": 10, "SN2_LAS_STATS_BYTES": 160, "SN2_LAS_FIELD_MASK_ALL": 0x3FF,
    "SN2_TIFF_LAYOUT_BAND": 0, "SN2_TIFF_LAYOUT_PIXEL": 1, "SN2_TIFF_PLACE_COLS": 4, "SN2_TIFF_STATS_BYTES": 16,
    "SN2_CUT_MAX_CELLS": 1 << 22, "SN2_CUT_MAX_ITEMS": 1 << 24,
    "SN2_ORTHO_MAX_IMAGES": 32, "SN2_ORTHO_MAX_MAP": 4, "SN2_ORTHO_MAX_SAMPLES": 1 << 40, "SN2_ORTHO_U8": 0, "SN2_ORTHO_U16": 1, "SN2_ORTHO_F32": 2,
    "SN2_ORTHO_CHUNKY": 0, "SN2_ORTHO_PLANAR": 1,
    "SN2_FP_FORM_SPLIT": 0, "SN2_FP_FORM_SOURCE_SIDE": 1, "SN2_FP_FORM_DENSE": 2,
    "SN2_FPS_FORM_BRUTE": 0, "SN2_FPS_FORM_ROUND": 1, "SN2_FPS_FORM_SPEC": 2, "SN2_FPS_FORM_CLUSTER": 3,
    "SN2_NET_FORK": 1, "SN2_NET_SHARED": 2, "SN2_NET_INVERTED": 4, "SN2_NET_DEFER_JOIN": 8, "SN2_NET_INPUT_ONLY": 16,
    "SN2_NET_HAS_ROWS0": 32, "SN2_NET_JOIN_PENDING": 64, "SN2_NET_WITH_GEOMETRY": 128, "SN2_NET_HAS_INVERTED": 256, "SN2_NET_CLOUD10": 512,
}
globals().update(CONSTANTS)
# the names the package has used so far
MAX_NEIGHBORS, STAT_SLOTS, BN_FROZEN_KEEP = CONSTANTS["SN2_MAX_NEIGHBORS"], CONSTANTS["SN2_STAT_SLOTS"], CONSTANTS["SN2_BN_FROZEN_KEEP"]
(NET_FORK, NET_SHARED, NET_INVERTED, NET_DEFER_JOIN, NET_INPUT_ONLY, NET_HAS_ROWS0, NET_JOIN_PENDING, NET_WITH_GEOMETRY,
 NET_HAS_INVERTED, NET_CLOUD10) = (CONSTANTS["SN2_NET_" + n] for n in ("FORK", "SHARED", "INVERTED", "DEFER_JOIN", "INPUT_ONLY", "HAS_ROWS0",
                                                                       "JOIN_PENDING", "WITH_GEOMETRY", "HAS_INVERTED", "CLOUD10"))


class Block(Structure):  # sn2_block
    _fields_ = [("cin", c_int), ("cout", c_int), ("W", c_void_p), ("b", c_void_p), ("gamma", c_void_p),
                ("beta", c_void_p), ("running_mean", c_void_p), ("running_var", c_void_p), ("a", c_void_p),
                ("c", c_void_p), ("mean", c_void_p), ("invstd", c_void_p), ("stat_slots", c_void_p),
                ("dW", c_void_p), ("db", c_void_p), ("dgamma", c_void_p), ("dbeta", c_void_p),
                ("grad_replicas", c_int), ("grad_replica_stride", c_int), ("mma_bf16", c_int),
                ("num_batches_tracked", c_void_p), ("frozen_stats", c_int)]


class SA(Structure):  # sn2_sa
    _fields_ = [("B", c_int), ("Nsrc", c_int), ("M", c_int), ("cap", c_int), ("cf", c_int), ("nl", c_int),
                ("feat", c_void_p), ("feat_stride", c_int), ("spos", c_void_p), ("spos_stride", c_int),
                ("cpos", c_void_p), ("nbr", c_void_p), ("cnt", c_void_p), ("total", c_void_p), ("order", c_void_p),
                ("blk", Block * 2),
                ("ext", c_void_p), ("arg", c_void_p), ("out", c_void_p), ("dout", c_void_p), ("dfeat", c_void_p),
                ("bwd_ws", c_void_p)]


class FP(Structure):  # sn2_fp
    _fields_ = [("B", c_int), ("R_per_plot", c_int), ("S_per_plot", c_int), ("ca", c_int), ("cb", c_int),
                ("src", c_void_p), ("src_stride", c_int), ("src_a", c_void_p), ("src_c", c_void_p),
                ("knn_idx", c_void_p), ("knn_w", c_void_p), ("skip", c_void_p), ("skip_stride", c_int),
                ("blk", Block), ("h", c_void_p), ("h_stride", c_int), ("dy", c_void_p), ("dsrc", c_void_p),
                ("dsrc_stride", c_int), ("dskip", c_void_p), ("dskip_stride", c_int), ("du_scratch", c_void_p),
                ("scatter_ws", c_void_p), ("scatter_ready", c_int), ("bn_sums_done", c_void_p), ("src_ws", c_void_p),
                ("act_bf16", c_int), ("row_perm", c_void_p)]


class FpsRoute(Structure):  # sn2_fps_route_t
    _fields_ = [(n, c_int) for n in ("form", "nw", "p", "rung", "lds_points", "repair", "fills_ws")]


class LossGrad(Structure):  # sn2_loss_grad
    _fields_ = [(n, c_void_p) for n in ("pred", "gt", "proba", "pdf", "grad_total", "arg", "nocc", "pix")] + [
        ("B", c_int), ("N", c_int), ("D", c_int), ("m", c_double), ("e", c_double)]


class Head(Structure):  # sn2_head
    _fields_ = [("R", c_int), ("cin", c_int), ("f_stride", c_int), ("f", c_void_p), ("fa", c_void_p),
                ("fc", c_void_p), ("W1", c_void_p), ("b1", c_void_p), ("W2", c_void_p), ("b2", c_void_p),
                ("coverages", c_void_p), ("proba", c_void_p), ("dcoverages", c_void_p), ("dproba", c_void_p),
                ("dy", c_void_p), ("dW1", c_void_p), ("db1", c_void_p), ("dW2", c_void_p), ("db2", c_void_p),
                ("grad_replicas", c_int), ("grad_replica_stride", c_int), ("drop_mask", c_void_p), ("drop_scale", c_float),
                ("act_bf16", c_int), ("zero_fill", c_void_p), ("zero_fill_words", c_long), ("loss", POINTER(LossGrad))]


class NetLayer(Structure):  # sn2_net_layer
    _fields_ = [("cin", c_int), ("cout", c_int), ("W", c_void_p), ("b", c_void_p), ("gamma", c_void_p), ("beta", c_void_p),
                ("running_mean", c_void_p), ("running_var", c_void_p), ("num_batches_tracked", c_void_p),
                ("gW", c_int), ("gb", c_int), ("ggamma", c_int), ("gbeta", c_int), ("mma_bf16", c_int)]


class NetModel(Structure):  # sn2_net_model
    _fields_ = [("sa1", NetLayer * 2), ("sa2", NetLayer), ("sa3", NetLayer), ("fp3", NetLayer), ("fp2", NetLayer), ("fp1", NetLayer),
                ("lin1_W", c_void_p), ("lin1_b", c_void_p), ("lin2_W", c_void_p), ("lin2_b", c_void_p),
                ("g_lin1_W", c_int), ("g_lin1_b", c_int), ("g_lin2_W", c_int), ("g_lin2_b", c_int), ("n_flat", c_int),
                ("r1_sq", c_float), ("r2_sq", c_float), ("max_neighbors", c_int), ("drop_p", c_float),
                ("fuse_global_level", c_int), ("fuse_eval_head", c_int), ("source_side", c_int),
                ("fps_waves_shared", c_int), ("fps_waves_many", c_int)]


class NetDims(Structure):  # sn2_net_dims
    _fields_ = [("B", c_int), ("N", c_int), ("M1", c_int), ("M2", c_int), ("cap1", c_int), ("cap2", c_int), ("act_bf16", c_int),
                ("p2_diam_pix", c_int)]


class NetGeo(Structure):  # sn2_net_geo
    _fields_ = [(n, c_void_p) for n in (
        "xyz", "idx1", "pos1_soa", "pos1_aos", "ws1", "nbr1", "cnt1", "tot1", "ord1",
        "idx2", "pos2_soa", "pos2_aos", "ws2", "nbr2", "cnt2", "tot2", "ord2", "pos3",
        "knn3_idx", "knn3_w", "knn2_idx", "knn2_w", "knn1_idx", "knn1_w", "inv3", "inv2", "inv1", "nn_ws2", "nn_ws1",
        "rank1", "rows0", "p2_pix", "p2_mm")]


class NetAct(Structure):  # sn2_net_act
    _fields_ = [(n, c_void_p) for n in (
        "aux", "stats", "ext1", "arg1", "x1", "ext2", "arg2", "x2", "h_sa3", "h3", "x3", "arg3", "h2", "h1", "src_ws1", "src_ws2",
        "cov", "proba", "drop_mask", "bwd_arena")] + [("bwd_arena_words", c_long)]


class NetBwd(Structure):  # sn2_net_bwd
    _fields_ = [("dcov", c_void_p), ("dproba", c_void_p), ("arena", c_void_p), ("arena_words", c_long), ("images", c_int),
                ("image_stride", c_int)] + [(n, c_void_p) for n in (
                    "dy2", "dy3", "dx1", "dx2", "dx3", "dy_sa3", "sa1_ws", "dy1", "du1", "du2", "du3", "bn_ok", "src_ws1", "src_ws2")] + [
                        ("defer_grad_reduce", c_int), ("arena_is_zero", c_int), ("frozen_stats", c_int), ("gl_xchg", c_void_p),
                        ("gl_ctl", c_void_p), ("loss", POINTER(LossGrad))]


class NetIO(Structure):  # sn2_net_io
    _fields_ = [("cloud", c_void_p), ("fps_start", c_void_p), ("fps_status", c_void_p), ("gl_xchg", c_void_p), ("gl_ctl", c_void_p),
                ("stream_b", c_void_p), ("stream_c", c_void_p), ("stream_pack", c_void_p), ("ctx", c_void_p), ("flags", c_int),
                ("training", c_int), ("fps_live", c_void_p), ("fps_live1", c_void_p)]


class CutTable(Structure):  # sn2_cut_table
    _fields_ = [("K", c_int), ("GX", c_int), ("GY", c_int), ("L", c_int), ("T", c_longlong), ("n_items", c_longlong),
                ("n_edges", c_longlong), ("gx0", c_double), ("gy0", c_double), ("inv", c_double), ("buffer", c_double)] + [
                    (n, c_void_p) for n in ("cell_start", "cell_items", "edge_start", "edges", "cell_start_dev", "cell_items_dev",
                                            "edge_start_dev", "edges_dev")]


class OrthoImage(Structure):  # sn2_ortho_image
    _fields_ = [("x0", c_double), ("y0", c_double), ("px", c_double), ("py", c_double), ("pixels", c_void_p), ("W", c_int), ("H", c_int)]


class OrthoSet(Structure):  # sn2_ortho_set
    _fields_ = [(n, c_int) for n in ("S", "C", "dtype", "layout", "n_map", "has_nodata")] + [
        ("band", c_int * CONSTANTS["SN2_ORTHO_MAX_MAP"]), ("row", c_int * CONSTANTS["SN2_ORTHO_MAX_MAP"]), ("nodata", c_double),
        ("scale", c_float), ("reserved", c_int), ("image", OrthoImage * CONSTANTS["SN2_ORTHO_MAX_IMAGES"])]


# name -> argtypes; every entry point returns int (0 ok, >0 hipError_t, <0 argument error; the route predicates: 0 / 1)
SIGNATURES = {
    "sn2_version": [],
    "sn2_debug_mfma_chain": [c_void_p, c_void_p, c_void_p, c_int, c_void_p],
    "sn2_debug_spin": [c_int, c_longlong, c_void_p, c_void_p],
    "sn2_debug_fp1_backward_parts": [c_int],
    "sn2_debug_fp_rows_form": [c_int],
    "sn2_debug_fp_table_form": [c_int],
    "sn2_debug_stream_probe": [c_void_p, c_void_p, ctypes.c_size_t, c_int, c_void_p, c_void_p],
    "sn2_debug_mfma_probe": [c_int, c_int, c_void_p, POINTER(c_double), c_void_p],
    "sn2_pack_rows": [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p],
    "sn2_pack_rows_feat": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p],
    "sn2_fps": [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "sn2_fps_waves": [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p],
    "sn2_fps_status": [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p],
    "sn2_fps_live": [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                     c_void_p],
    "sn2_debug_fps_spin_limit": [ctypes.c_uint],
    "sn2_ball_query": [c_void_p, c_int, c_int, c_void_p, c_int, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                       c_void_p],
    "sn2_three_nn": [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "sn2_count_sum": [c_void_p, c_int, c_void_p, c_void_p],
    "sn2_count_sum_group": [c_void_p, c_int, c_int, c_void_p, ctypes.c_size_t, c_void_p],
    "sn2_three_nn_xy": [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "sn2_three_nn_xy_copy": [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p],
    "sn2_three_nn_xy_order_offset": [c_int, c_int, c_int, POINTER(ctypes.c_size_t), POINTER(ctypes.c_size_t)],
    "sn2_prepare_plots": [c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p,
                          c_void_p, c_void_p, c_void_p, c_long, c_float, c_void_p, c_void_p, c_void_p],
    "sn2_znorm": [c_void_p, c_void_p, c_void_p, c_int, c_float, c_float, c_float, c_float, c_float, c_void_p, c_void_p,
                  c_void_p, c_void_p],
    "sn2_parcel_count": [c_void_p, c_long, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_double, c_double,
                         c_double, c_float, c_void_p, ctypes.c_size_t, c_void_p, c_void_p, c_void_p],
    "sn2_parcel_fill": [c_void_p, c_long, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_double, c_double,
                        c_double, c_float, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p],
    "sn2_parcel_znorm": [c_void_p, c_long, c_float, c_float, c_float, c_float, c_float, c_float, c_void_p, c_void_p, c_int,
                         c_void_p, c_long, c_void_p, ctypes.c_size_t, c_void_p, c_void_p],
    # K parcels at once (csrc/parcels.hip); table_host, starts_host are host pointers
    "sn2_parcels_table": [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p,
                          POINTER(c_int), POINTER(ctypes.c_size_t), POINTER(ctypes.c_size_t)],
    "sn2_parcels_bbox": [c_void_p, c_long, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "sn2_parcels_count": [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, ctypes.c_size_t,
                          c_void_p, c_void_p, c_void_p, c_void_p],
    "sn2_parcels_fill": [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_long,
                         c_void_p, c_void_p, c_void_p],
    "sn2_parcels_znorm": [c_void_p, c_int, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                          c_long, c_void_p, ctypes.c_size_t, c_void_p, c_void_p],
    "sn2_subsample_form": [c_int, c_int],
    "sn2_subsample": [c_void_p, c_int, c_int, c_int, c_int, ctypes.c_ulonglong, c_void_p, c_int, c_void_p, ctypes.c_size_t,
                      c_void_p, c_void_p],
    "sn2_train_batch_ws_words": [c_int, c_int, c_int, POINTER(ctypes.c_size_t)],
    "sn2_train_batch": [c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
                        c_float, ctypes.c_ulonglong, c_longlong, c_void_p, c_int, c_int, c_void_p, ctypes.c_size_t, c_void_p, c_void_p,
                        c_void_p, c_void_p, c_void_p],
    "sn2_train_batch_live": [c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
                             c_float, ctypes.c_ulonglong, c_longlong, c_void_p, c_int, c_int, c_void_p, ctypes.c_size_t, c_void_p,
                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "sn2_plots_append": [c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_long, c_void_p, c_void_p,
                         c_void_p, c_int, c_int, c_long, c_void_p, c_long, c_void_p],
    "sn2_sa_order": [c_void_p, c_int, c_int, c_void_p, c_void_p],
    "sn2_sa_order_group": [c_void_p, c_int, c_int, c_int, c_void_p, ctypes.c_size_t, c_void_p],
    "sn2_sa_forward": [POINTER(SA), c_int, c_void_p],
    "sn2_sa_backward": [POINTER(SA), c_void_p],
    "sn2_grad_reduce": [c_void_p, c_int, c_int, c_int, c_void_p],
    "sn2_interp_index": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p],
    "sn2_interp_index_perm": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p],
    "sn2_interp_index_group": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, ctypes.c_size_t, c_void_p],
    "sn2_interp_index_ordered": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                 c_void_p, ctypes.c_size_t, c_void_p],
    "sn2_fp_forward": [POINTER(FP), c_int, c_void_p],
    "sn2_fp_backward": [POINTER(FP), c_void_p],
    "sn2_plot_max_forward": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p],
    "sn2_plot_max_backward": [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p],
    "sn2_global_pool_backward": [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p],
    "sn2_global_level_forward": [POINTER(FP), POINTER(FP), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "sn2_global_level_backward": [POINTER(FP), POINTER(FP), c_void_p, c_void_p, c_void_p, c_void_p],
    "sn2_debug_global_spin_limit": [ctypes.c_uint],
    "sn2_head_forward": [POINTER(Head), c_void_p],
    "sn2_fp_head_eval": [POINTER(FP), POINTER(Head), c_void_p],
    "sn2_fp_bn_sums": [POINTER(FP), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "sn2_head_bn_sums": [POINTER(Head), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "sn2_head_backward": [POINTER(Head), c_void_p],
    "sn2_debug_head_backward_occupancy": [c_int, c_int],
    "sn2_plot_project_forward": [c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p],
    "sn2_plot_pixels": [c_void_p, c_long, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p],
    "sn2_plot_project_forward_pix": [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "sn2_plot_project_backward": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p],
    "sn2_raster_project": [c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                           c_void_p],
    "sn2_mosaic_merge": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                         c_int, c_int, c_int, c_int, c_void_p],
    "sn2_mosaic_finalize": [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "sn2_mosaic_crop_stats": [c_void_p, c_int, c_int, c_int, c_double, c_double, c_double, c_void_p, c_int, c_void_p, c_void_p,
                              c_void_p, c_void_p],
    # the mosaic atlas (csrc/atlas.hip); canvas_host, seg_host, edge_start_host are host pointers
    "sn2_atlas_canvas_table": [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "sn2_atlas_finalize_ws_words": [c_int, POINTER(ctypes.c_size_t)],
    "sn2_atlas_merge": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                        c_void_p, c_void_p],
    "sn2_atlas_finalize": [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "sn2_atlas_crop_stats": [c_void_p, c_int, c_int, c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_void_p],
    # the admissibility band (csrc/admissibility.hip); canvas_host is a host pointer
    "sn2_admissibility_ws_words": [c_longlong, POINTER(ctypes.c_size_t)],
    "sn2_mosaic_admissibility": [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "sn2_atlas_admissibility": [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    # the per-point scores of a parcel cloud (csrc/points.hip)
    "sn2_points_merge": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_int, c_int, c_double,
                         c_void_p, c_void_p, c_long, c_void_p],
    "sn2_points_finalize": [c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p],
    # the LAS decoder (csrc/las.hip); xform and raw0 are host pointers
    "sn2_las_record_min_length": [c_int],
    "sn2_las_decode": [c_void_p, ctypes.c_size_t, c_int, c_int, c_long, c_int, POINTER(c_double), POINTER(c_longlong), c_void_p, c_long,
                       c_long, c_void_p, c_void_p],
    "sn2_debug_las_form": [c_int],
    # the LAS encoder (csrc/las_write.hip); class_codes is a host pointer
    "sn2_las_encode": [c_void_p, ctypes.c_size_t, c_int, c_int, c_long, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_long, c_long,
                       c_int, c_int, POINTER(c_int), c_int, c_void_p, ctypes.c_size_t, c_void_p, c_void_p],
    "sn2_las_encode_stage_max": [],
    "sn2_debug_las_encode_form": [c_int],
    # the GeoTIFF band packer (csrc/tiff_pack.hip); canvas_host, skip, place and place_host are host pointers
    "sn2_tiff_place_table": [c_int, c_int, c_void_p, c_int, c_void_p, c_void_p],
    "sn2_tiff_pack": [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, ctypes.c_size_t, c_void_p],
    "sn2_tiff_pack_stage_max": [],
    "sn2_debug_tiff_pack_form": [c_int],
    # the dBase record annotator (csrc/dbf.hip); cols is a host pointer
    "sn2_dbf_annotate": [c_void_p, c_long, c_int, c_void_p, c_long, c_int, c_void_p, POINTER(c_int), c_int, c_int, c_int, c_double, c_void_p,
                         ctypes.c_size_t, c_void_p],
    # the parcel cut (csrc/cut.hip); drop is a host pointer, the table holds host and device pointers
    "sn2_cut_ws_words": [POINTER(CutTable), POINTER(ctypes.c_size_t)],
    "sn2_cut_count": [c_void_p, c_void_p, c_void_p, POINTER(CutTable), c_void_p, ctypes.c_size_t, c_void_p, c_void_p, c_void_p],
    "sn2_cut_fill": [c_void_p, c_void_p, c_void_p, POINTER(CutTable), c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p],
    # the orthoimage colours (csrc/ortho.hip); the set is a host structure that holds device pointers
    "sn2_ortho_colorize": [c_void_p, c_long, c_long, c_long, POINTER(OrthoSet), c_void_p, c_void_p, c_void_p],
    "sn2_kde_lookup": [c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_int, c_void_p, c_void_p],
    "sn2_kde_fit": [c_void_p, c_long, c_double, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "sn2_loss_forward": [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_double, c_double, c_void_p, c_void_p,
                         c_void_p],
    "sn2_loss_backward": [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_double, c_double, c_void_p, c_void_p,
                          c_void_p, c_void_p],
    "sn2_adam_step": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float, c_float, c_float, c_float, c_float,
                      c_void_p, c_float, c_void_p],
    "sn2_adam_step_dev": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_float, c_float, c_float, c_float,
                          c_void_p, c_float, c_void_p, c_int, c_void_p, c_void_p],
    "sn2_projected_loss_forward": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_double, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "sn2_projected_loss_backward": [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_double, c_double, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "sn2_plot_losses": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_double, c_void_p, c_void_p,
                        c_void_p, c_void_p],
    # the cross-validation report (csrc/indicators.hip)
    "sn2_cv_indicators_ws_words": [c_int, POINTER(ctypes.c_size_t)],
    "sn2_cv_indicators": [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "sn2_adam_step_images": [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_float, c_float, c_float, c_float, c_float,
                             c_void_p, c_float, c_void_p],
    "sn2_adam_step_images_dev": [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_float, c_float, c_float,
                                 c_float, c_void_p, c_float, c_void_p, c_int, c_void_p, c_void_p],
    "sn2_net_ctx_create": [POINTER(c_void_p)],
    "sn2_net_ctx_destroy": [c_void_p],
    "sn2_net_geo_carve": [POINTER(NetModel), POINTER(NetDims), c_void_p, POINTER(NetGeo), POINTER(ctypes.c_size_t)],
    "sn2_net_act_carve": [POINTER(NetModel), POINTER(NetDims), c_int, c_void_p, POINTER(NetAct), POINTER(ctypes.c_size_t)],
    "sn2_net_bwd_carve": [POINTER(NetModel), POINTER(NetDims), c_void_p, c_void_p, POINTER(NetBwd), POINTER(ctypes.c_size_t),
                          POINTER(ctypes.c_size_t)],
    "sn2_net_geometry": [POINTER(NetModel), POINTER(NetDims), POINTER(NetGeo), POINTER(NetIO), c_void_p],
    "sn2_net_forward": [POINTER(NetModel), POINTER(NetDims), POINTER(NetGeo), POINTER(NetAct), POINTER(NetIO), c_void_p],
    "sn2_net_backward": [POINTER(NetModel), POINTER(NetDims), POINTER(NetGeo), POINTER(NetAct), POINTER(NetBwd), c_void_p],
    # the route predicates ("Routes" of the header): host-only arithmetic, they return 0 / 1
    "sn2_fps_fills_ws": [c_int, c_int, c_int],
    "sn2_fps_route": [c_int, c_int, c_int, c_int, c_int, c_int, POINTER(FpsRoute)],   # 0 and the route, or the entry point's negative code
    "sn2_three_nn_uses_grid": [c_int, c_int],
    "sn2_fp_rows_small": [c_long],
    "sn2_fp_source_side": [c_long, c_int, c_int],
    "sn2_fp_form": [POINTER(FP), c_int],         # SN2_FP_FORM_*, or the negative code of the entry point
    "sn2_global_level_forward_route": [c_int, c_int],
    "sn2_global_level_backward_route": [c_int, c_int, c_int, c_int],
    "sn2_head_loss_route": [c_int, c_int, c_int],
}

# workspace-size and layout helpers: name -> argtypes; they return size_t (32-bit words unless the header says otherwise; 0 =
# beyond what the kernels cover)
SIZE_HELPERS = {
    "sn2_fps_ws_words": [c_int, c_int],
    "sn2_fps_ws_grid_offset": [c_int, c_int],
    "sn2_fps_ws_ctl_offset": [c_int, c_int],
    "sn2_fps_ws_rank_offset": [c_int, c_int],
    "sn2_three_nn_ws_words": [c_int, c_int],
    "sn2_three_nn_xy_ws_words": [c_int, c_int, c_int],
    "sn2_znorm_ws_words": [c_int, c_long],
    "sn2_sa_order_words": [c_int, c_int],
    "sn2_interp_chunks": [c_int, c_int],
    "sn2_interp_ws_words": [c_int, c_int, c_int],
    "sn2_fp_src_ws_words": [c_int, c_int, c_int, c_int],
    "sn2_global_xchg_words": [c_int],
    "sn2_p2_key_parts": [c_int],
    "sn2_kde_fit_ws_words": [c_int],
    "sn2_parcel_count_ws_words": [c_int, c_int],
    "sn2_parcel_znorm_ws_words": [c_long, c_float, c_float, c_float, c_float, c_float],
    "sn2_subsample_ws_words": [c_int, c_int, c_int, c_int],
    "sn2_plot_losses_ws_words": [c_int, c_int, c_int],
}

# size helpers the header declares `extern` (outside the closed list of macros that tests/test_cabi.py walks): each is held to
# its macro by a test of its own (sn2_mosaic_crop_ws_words: tests/test_parcel_report_host.py)
EXTERN_SIZE_HELPERS = {
    "sn2_mosaic_crop_ws_words": [c_int, c_int, c_int],
}

_lib = None


class StrataHipError(RuntimeError):
    pass


def load():
    """Load libstrata_hip.so (built in-tree by `_build.build()`); raises if it is absent -- there is no CPU
    fallback in the product path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise StrataHipError(
            f"{LIB_PATH} not found: build it with `python -m stratanet2_vegetation_coverage_maps_amd._build` "
            "(or __graft_entry__.build()); the HIP library is mandatory, there is no fallback path")
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = c_int
    for name, argtypes in list(SIZE_HELPERS.items()) + list(EXTERN_SIZE_HELPERS.items()):
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = ctypes.c_size_t
    if lib.sn2_version() != SN2_VERSION:
        raise StrataHipError(f"libstrata_hip.so version {lib.sn2_version()} != binding {SN2_VERSION}: rebuild")
    _lib = lib
    return lib


@functools.lru_cache(maxsize=4096)
def host_value(name: str, *args) -> int:
    """A route predicate or size helper of the library (SIGNATURES / SIZE_HELPERS: pure functions of their integer arguments),
    remembered per argument tuple: several of them are asked once per launch on the per-call path."""
    return getattr(load(), name)(*args)


def check(rc: int, what: str):
    if rc != 0:
        kind = "hipError_t" if rc > 0 else {-1: "SN2_EINVAL", -2: "SN2_ELIMIT"}.get(rc, "error")
        raise StrataHipError(f"{what} failed: {kind} {rc}")
