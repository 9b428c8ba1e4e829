"""ctypes binding of libvqseg_hip.so (the C ABI declared in include/vqseg.h).

Torch is used only to own device memory and to name the current HIP stream; every
argument crossing the boundary is a raw pointer or a size.  Fails loudly: a missing
library, a CPU tensor, a wrong dtype or a non-zero return code raise.

Two functions carry the protocol: `tptr` is the way a tensor becomes an argument, `launch` the way
an entry point that takes a stream is called.  What is known about a call travels in its arguments;
nothing is kept between the two.
"""
from __future__ import annotations

import ctypes
import functools
import math
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_void_p
from typing import Optional, Tuple

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VQSEG_LIB") or os.path.join(_HERE, "libvqseg_hip.so")     # VQSEG_LIB: another build of the same ABI (kernel A/B runs)

# name -> (restype, argtypes); must list every symbol include/vqseg.h declares
SYMBOLS = {
    "vqseg_abi_version": (c_int, []),
    "vqseg_last_error": (c_char_p, []),
    "vqseg_kernel_name": (c_char_p, [c_char_p]),
    "vqseg_set_option": (c_int, [c_char_p, c_int]),
    "vqseg_profile_begin": (c_int, [c_int]),
    "vqseg_profile_collect": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vqseg_conv_profile_begin": (c_int, [c_int]),
    "vqseg_conv_profile_collect": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vqseg_vq_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "vqseg_vq_filter_counter_offset": (c_size_t, [c_int64, c_int, c_int]),
    "vqseg_vq_tiles_per_wave": (c_int, [c_int, c_void_p, c_void_p]),
    "vqseg_vq_forward_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_float, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "vqseg_vq_forward_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_float, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "vqseg_vq_forward_group": (c_int, [c_int, c_int] + [c_void_p] * 6 + [c_int, c_void_p] + [c_void_p] * 6 + [c_void_p]),
    "vqseg_vq_backward_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p, c_void_p]),
    "vqseg_vq_assign_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                    c_size_t, c_void_p]),
    "vqseg_vq_assign_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                     c_size_t, c_void_p]),
    "vqseg_vq_assign_s3": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                   c_size_t, c_void_p]),
    "vqseg_vq_prepared_bytes": (c_size_t, [c_int, c_int]),
    "vqseg_vq_prepare_f32": (c_int, [c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "vqseg_vq_backward_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p,
                                      c_void_p]),
    "vqseg_kmeans_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "vqseg_kmeans_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_size_t,
                                 c_void_p]),
    "vqseg_kmeans_accumulate_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                            c_size_t, c_void_p]),
    "vqseg_kmeans_finalize_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "vqseg_vq_code_sums": (c_int, [c_int, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "vqseg_vq_ema_update_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_void_p,
                                        c_void_p]),
    "vqseg_vq_revive_candidates": (c_int, [c_int, c_void_p, c_int64, c_int, c_int, ctypes.c_uint64, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                           c_void_p]),
    "vqseg_vq_ema_update_revive_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_void_p,
                                               c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "vqseg_conv_packed_elems": (c_size_t, [c_int] * 5),
    "vqseg_conv_pack_weights_f32": (c_int, [c_void_p] + [c_int] * 5 + [c_void_p, c_void_p, c_void_p]),
    "vqseg_conv_stat_slots": (c_int64, [c_int64, c_int]),
    "vqseg_conv2d_f": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p] + [c_int] * 14 + [c_void_p]),
    "vqseg_conv2d_affine_f": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p] +
                              [c_int] * 13 + [c_void_p]),
    "vqseg_conv2d_wgrad_workspace_bytes": (c_size_t, [c_int] * 9),
    "vqseg_conv2d_wgrad_f": (c_int, [c_void_p, c_void_p, c_void_p] + [c_int] * 17 + [c_void_p, c_size_t, c_void_p, c_void_p]),
    "vqseg_conv2d_wgrad2_f": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int] + [c_int] * 16 +
                              [c_void_p, c_size_t, c_void_p, c_void_p]),
    "vqseg_bn_sync_ints": (c_int, [c_int]),
    "vqseg_bn_finalize_f": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_int,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vqseg_bn_apply_f": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "vqseg_bn_backward_workspace_floats": (c_size_t, [c_int64, c_int]),
    "vqseg_bn_backward_f": (c_int, [c_int] + [c_void_p] * 8 + [c_int64, c_int, c_int, c_int, c_int] + [c_void_p] * 7),
    "vqseg_conv2d_affine_bits_f": (c_int, [c_void_p] * 7 + [c_int] * 10 + [c_void_p]),
    "vqseg_bn_apply_bits_f": (c_int, [c_void_p] * 4 + [c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "vqseg_bn_backward_bits_f": (c_int, [c_void_p] * 6 + [c_int64, c_int, c_int, c_int] + [c_void_p] * 7),
    "vqseg_maxpool3x3s2_f": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "vqseg_bilinear_f": (c_int, [c_int, c_int, c_void_p] + [c_int] * 7 + [c_void_p, c_void_p]),
    "vqseg_head1x1_forward_f": (c_int, [c_int, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "vqseg_head1x1_backward_workspace_floats": (c_size_t, [c_int64, c_int, c_int]),
    "vqseg_head1x1_backward_f": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p,
                                        c_void_p, c_void_p]),
    "vqseg_proto_loss_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "vqseg_proto_loss_forward_f": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int,
                                           c_float, c_float, c_int, c_void_p, c_size_t, c_void_p, c_void_p]),
    "vqseg_proto_loss_backward_f": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int,
                                            c_float, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "vqseg_dice_workspace_bytes": (c_size_t, [c_int, c_int, c_int64]),
    "vqseg_dice_sums_forward_f": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int, c_int, c_int64, c_int64, c_void_p, c_size_t,
                                          c_void_p, c_void_p, c_void_p]),
    "vqseg_dice_sums_backward_f": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int, c_int, c_int64, c_int64, c_void_p,
                                           c_void_p, c_void_p, c_void_p]),
    "vqseg_dice_ce_sums_forward_f": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int, c_int, c_int64, c_int64, c_void_p,
                                             c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vqseg_dice_ce_sums_backward_f": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int, c_int, c_int64, c_int64, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_void_p]),
    "vqseg_focal_workspace_bytes": (c_size_t, [c_int, c_int64]),
    "vqseg_focal_forward_f": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int, c_int, c_int64, c_int64, c_void_p, c_float, c_float,
                                      c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vqseg_focal_backward_f": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int, c_int, c_int64, c_int64, c_void_p, c_float, c_float,
                                       c_int, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "vqseg_wce_sums_forward_f": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int, c_int, c_int64, c_int64, c_void_p, c_void_p,
                                         c_size_t, c_void_p, c_void_p]),
    "vqseg_wce_sums_backward_f": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int, c_int, c_int64, c_int64, c_void_p, c_void_p,
                                          c_void_p, c_void_p]),
    "vqseg_class_weight_f": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "vqseg_softmax_stats_f": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vqseg_confusion_counts_f": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p]),
    "vqseg_order_stats_workspace_bytes": (c_size_t, []),
    "vqseg_order_stats_f": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_size_t, c_void_p, c_void_p]),
    "vqseg_im2col_f": (c_int, [c_int, c_void_p] + [c_int] * 12 + [c_void_p, c_void_p]),
    "vqseg_reflect_fold_f": (c_int, [c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "vqseg_reflect_ring_f": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "vqseg_cast_f": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p]),
    "vqseg_conv_pack_all_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vqseg_conv_packed_s2_elems": (c_size_t, [c_int, c_int, c_int]),
    "vqseg_conv_pack_weights_s2_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "vqseg_conv2d_dgrad_s2_f": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p] + [c_int] * 10 + [c_void_p]),
    "vqseg_stem7_conv_f": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p] + [c_int] * 5 + [c_void_p]),
    "vqseg_conv2d_dgrad_s2_fold_rows": (ctypes.c_int64, [c_int] * 4),
    "vqseg_cps_loss_combine_f": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_float, c_void_p, c_int, c_int,
                                         c_float, c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vqseg_conv2d_dgrad_s2_fold_f": (c_int, [c_void_p, c_void_p, c_void_p] + [c_int] * 8 + [c_void_p]),
    "vqseg_head1x1_backward_add_f": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_void_p]),
    "vqseg_maxpool3x3s2_backward_add_f": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "vqseg_conv_pack_weights_s3_f32": (c_int, [c_void_p] + [c_int] * 5 + [c_void_p, c_void_p]),
    "vqseg_s3_split_f": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "vqseg_s3_merge_f": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "vqseg_s3_maxpool3x3s2_f": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "vqseg_s3_bilinear_f": (c_int, [c_void_p] + [c_int] * 7 + [c_void_p, c_void_p]),
    "vqseg_adam_work_items": (c_int64, [c_int64, c_int, c_int, c_int]),
    "vqseg_adam_step_f32": (c_int, [c_void_p, c_void_p, c_int, c_double, c_double, c_double, c_double, c_int64, c_void_p]),
    "vqseg_adam_ema_step_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_double, c_double, c_double, c_double, c_int64, c_double, c_int,
                                        c_void_p]),
    "vqseg_batch_u8_f": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p] + [c_int] * 4 + [c_void_p] * 6),
    "vqseg_box_mix_f": (c_int, [c_int, c_int, c_void_p, c_void_p] + [c_int] * 4 + [c_int64] * 3 + [c_void_p, ctypes.c_uint64, c_void_p]),
    "vqseg_affine_warp_f": (c_int, [c_int, c_int, c_void_p, c_void_p] + [c_int] * 4 + [c_int64] * 4 + [c_void_p, ctypes.c_uint64, c_void_p]),
    "vqseg_resize_argmax_f": (c_int, [c_void_p, c_void_p, c_int] + [c_int64] * 3 + [c_int] * 6 + [c_void_p] * 5),
    "vqseg_extract_windows_f": (c_int, [c_void_p] + [c_int64] * 3 + [c_int] * 9 + [c_void_p, c_int, c_void_p, c_void_p]),
    "vqseg_merge_argmax_f": (c_int, [c_void_p, c_void_p, c_int] + [c_int64] * 3 + [c_int] * 11 + [c_void_p] * 5),
    "vqseg_render_sheet_u8": (c_int, [c_void_p] + [c_int64] * 3 + [c_int] * 2 + [c_void_p] * 2 + [c_int] * 6 + [c_void_p] * 3 + [c_int] +
                              [c_void_p] * 4 + [c_float, c_int, c_void_p, c_int64, c_int, c_int, c_void_p]),
    "vqseg_supcon_workspace_bytes": (c_size_t, [c_int64]),
    "vqseg_supcon_forward_f": (c_int, [c_int, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_float,
                                       c_void_p, c_size_t, c_void_p, c_void_p]),
    "vqseg_supcon_backward_f": (c_int, [c_int, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_float,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "vqseg_conf_ce_workspace_bytes": (c_size_t, [c_int, c_int64]),
    "vqseg_conf_ce_forward_f": (c_int, [c_void_p] + [c_int64] * 3 + [c_void_p] + [c_int64] * 3 + [c_int, c_int, c_int64, c_float, c_float, c_float,
                                        c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "vqseg_conf_ce_backward_f": (c_int, [c_void_p] + [c_int64] * 3 + [c_void_p] + [c_int64] * 3 + [c_int, c_int, c_int64, c_float, c_float, c_float,
                                         c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vqseg_crf_prepare_f": (c_int, [c_void_p] + [c_int64] * 3 + [c_void_p] + [c_int64] * 3 + [c_int] * 5 + [c_double] * 4 + [c_void_p] * 7),
    "vqseg_crf_step_f": (c_int, [c_void_p] * 6 + [c_int] * 4 + [c_double] * 6 + [c_int, c_void_p]),
    "vqseg_slic_lab_f": (c_int, [c_void_p] + [c_int64] * 3 + [c_int] * 5 + [c_void_p] * 3),
    "vqseg_slic_assign_f": (c_int, [c_void_p] * 2 + [c_int] * 5 + [c_float] + [c_void_p] * 2),
    "vqseg_slic_update_f": (c_int, [c_void_p] * 2 + [c_int] * 5 + [c_void_p] * 2),
    "vqseg_segment_sums_f": (c_int, [c_void_p] + [c_int64] * 3 + [c_void_p, c_int, c_int, c_int64, c_int] + [c_void_p] * 3),
    "vqseg_segment_broadcast_f": (c_int, [c_void_p] + [c_int64] * 3 + [c_void_p] * 3 + [c_int, c_int, c_int64, c_int, c_void_p] + [c_int64] * 3 +
                                  [c_void_p]),
    "vqseg_region_graph_f": (c_int, [c_void_p] * 2 + [c_int] * 5 + [c_void_p] * 3),
    "vqseg_rbd_weights_f": (c_int, [c_void_p] * 2 + [c_int] * 2 + [c_void_p] * 2),
    "vqseg_rbd_geodesic_f": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "vqseg_rbd_background_f": (c_int, [c_void_p] * 2 + [c_int] * 2 + [c_float] * 2 + [c_void_p] * 2),
    "vqseg_rbd_contrast_f": (c_int, [c_void_p] * 3 + [c_int] * 4 + [c_float] + [c_void_p] * 2),
    "vqseg_rbd_solve_f": (c_int, [c_void_p] * 5 + [c_int] * 2 + [c_float] * 2 + [c_void_p] * 5),
    "vqseg_rbd_paint_f": (c_int, [c_void_p] * 2 + [c_int] * 5 + [c_void_p] * 2),
    "vqseg_photometric_mean_blocks": (c_int, [c_int64]),
    "vqseg_photometric_f": (c_int, [c_void_p] * 2 + [c_int] * 3 + [c_int64] * 3 + [c_void_p] * 6),
    "vqseg_region_roots_u8": (c_int, [c_void_p] + [c_int] * 9 + [c_void_p] * 3),
    "vqseg_region_roots_i32": (c_int, [c_void_p] + [c_int] * 9 + [c_void_p] * 3),
    "vqseg_region_ids_partials": (c_int64, [c_int, c_int]),
    "vqseg_region_ids_i32": (c_int, [c_void_p] + [c_int] * 3 + [c_void_p] * 4),
    "vqseg_region_table_i32": (c_int, [c_void_p, c_int, c_void_p, c_void_p] + [c_int] * 4 + [c_void_p] * 3),
    "vqseg_region_areas_i32": (c_int, [c_void_p] + [c_int] * 3 + [c_void_p] * 2),
    "vqseg_region_filter_u8": (c_int, [c_void_p] * 3 + [c_int] * 6 + [c_void_p] * 2),
    "vqseg_region_filter_i32": (c_int, [c_void_p] * 3 + [c_int] * 6 + [c_void_p] * 2),
    "vqseg_instance_vote_bits": (c_int, [c_int]),
    "vqseg_instance_vote_i32": (c_int, [c_void_p] * 3 + [c_int] * 10 + [c_void_p] * 3),
    "vqseg_instance_overlap_i32": (c_int, [c_void_p] * 4 + [c_int] * 4 + [c_void_p] * 3),
    "vqseg_instance_match_i32": (c_int, [c_void_p] * 6 + [c_int] * 2 + [c_void_p] * 5),
    "vqseg_instance_tally_i32": (c_int, [c_void_p] * 9 + [c_int] * 3 + [c_void_p] * 4),
    "vqseg_boundary_seeds_u8": (c_int, [c_void_p] + [c_int] * 9 + [c_void_p] * 2),
    "vqseg_boundary_seeds_i32": (c_int, [c_void_p] + [c_int] * 9 + [c_void_p] * 2),
    "vqseg_boundary_edt_rows_u8": (c_int, [c_void_p] + [c_int] * 3 + [c_void_p] * 3),
    "vqseg_boundary_edt_cols_i32": (c_int, [c_void_p] * 2 + [c_int] * 3 + [c_void_p] * 2),
    "vqseg_boundary_counts_i32": (c_int, [c_void_p, c_int, c_void_p, c_int] + [c_void_p] * 4 + [c_int] * 11 + [c_void_p] * 2),
    "vqseg_channel_keep_f": (c_int, [c_void_p, c_int64, ctypes.c_uint64, c_int64, ctypes.c_uint64, c_int64, c_float, c_void_p]),
    "vqseg_channel_dropout_cat_f": (c_int, [c_int] + [c_void_p] * 3 + [c_int] * 5 + [c_void_p]),
    "vqseg_channel_dropout_fold_f": (c_int, [c_int] + [c_void_p] * 3 + [c_int] * 5 + [c_void_p]),
}

_lib: Optional[ctypes.CDLL] = None


class HipLibraryError(RuntimeError):
    pass


def _bind_symbols(handle: ctypes.CDLL) -> ctypes.CDLL:
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(handle, name)              # AttributeError if the symbol is missing
        fn.restype, fn.argtypes = res, args
    return handle


def lib() -> ctypes.CDLL:
    """Load (once) and return the HIP library; raise if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"(or `make -C vq_seg_amd/csrc`). There is no CPU fallback.")
        handle = _bind_symbols(ctypes.CDLL(LIB_PATH))
        if handle.vqseg_abi_version() != 1:
            raise HipLibraryError("libvqseg_hip.so ABI version mismatch")
        for kv in filter(None, os.environ.get("VQSEG_OPTS", "").split(",")):     # dispatch tunables for A/B runs: "key=value,..."
            key, _, val = kv.partition("=")
            if key.strip().startswith("py_"):                # host-side switches (A/B runs of the Python layer): PY_OPTS
                PY_OPTS[key.strip()] = int(val)
                continue
            if handle.vqseg_set_option(key.strip().encode(), int(val)) < 0:
                raise HipLibraryError(f"VQSEG_OPTS: unknown option {key!r}")
        _lib = handle
    return _lib


PY_OPTS: dict = {}
FILTER_DIAG = None            # set to a list to collect (n, c, k, open-row counter) of every bf16 grouped VQ forward (diagnostics only)


_BF_DTYPE = {0: torch.float32, 1: torch.bfloat16, 2: torch.bfloat16}      # the `bf16` flag of the entry points (2: split-3 [hi | lo] rows)


def tptr(t, name: str, dtype=None, numel: Optional[int] = None, bf: Optional[int] = None, at_least: bool = False, dense: bool = True):
    """THE way a tensor crosses the C ABI: returns its address after checking what the untyped `void*` on the other side cannot --
    the element type (`dtype`: one torch dtype or a tuple; or `bf`: the 0 / 1 / 2 activation-type flag that is passed to the SAME
    entry point, so flag and buffer cannot disagree), dense memory (not with `dense=False`: a view addressed through explicit
    strides that are passed along, which a valid torch view bounds by construction), the element count the sizes passed along
    imply (`numel`, exact unless `at_least`), and a 'cuda' (ROCm) device.  A bf16 buffer behind an f32 flag is a 2x out-of-bounds
    read on the GPU (it happened: DESIGN 2, r2); here it is a Python exception.  Type, density and size errors are raised HERE;
    a tensor that is right in all of these but not on the GPU comes back as a _NotOnGpu marker that `launch` refuses, so the
    call's other tensors still get their type / size checks first and the CPU test suite can feed every wrapper the wrong type
    (tests/test_abi_cpu.py).  None passes through as a null pointer."""
    if t is None:
        return None
    if bf is not None:
        dtype = _BF_DTYPE[bf]
    try:                                                     # fast path: everything in order (one short-circuit expression per launch argument)
        if (dtype is None or t.dtype is dtype or (type(dtype) is tuple and t.dtype in dtype)) and t.is_cuda and \
                (numel is None or (t.numel() >= numel if at_least else t.numel() == numel)) and \
                (not dense or t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))):
            return t.data_ptr()
    except AttributeError:
        pass
    return _tptr_report(t, name, dtype, numel, at_least, dense)


def _tptr_report(t, name, dtype, numel, at_least, dense):
    """slow path of tptr: say exactly what is wrong (type, density, size before the device)"""
    def bad(msg):
        return HipLibraryError(f"{name}: {msg}")
    if not isinstance(t, torch.Tensor):
        raise bad(f"expected a tensor, got {type(t).__name__}")
    if dtype is not None and (t.dtype not in dtype if isinstance(dtype, tuple) else t.dtype != dtype):
        if dense:
            raise bad(f"expected {dtype}, got {t.dtype}")
        names = " or ".join(str(d).removeprefix("torch.") for d in (dtype if isinstance(dtype, tuple) else (dtype,)))
        raise bad(f"expected a {names} tensor, got {t.dtype}")           # the strided logits' wording, kept
    if dense and not t.is_contiguous() and not (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)):
        raise bad(f"expected a dense (contiguous) tensor, got strides {tuple(t.stride())} for shape {tuple(t.shape)}")
    if numel is not None and (t.numel() < numel if at_least else t.numel() != numel):
        raise bad(f"the sizes passed along need {'at least ' if at_least else ''}{numel} elements, the tensor has {t.numel()} (shape {tuple(t.shape)})")
    if not t.is_cuda:
        return _NotOnGpu(f"{name}: the HIP path needs a tensor on a 'cuda' (ROCm) device; got {t.device}. There is no CPU fallback.")
    return t.data_ptr()


class _NotOnGpu:
    """What tptr returns instead of an address for a tensor that is not on the GPU.  The fact travels with the argument: the marker
    has no `_as_parameter_`, so ctypes refuses it for a `void*` parameter before the foreign function is entered, and `launch`
    turns that refusal into the marker's message.  `+ offset` (an address inside a weight image) keeps the marker."""
    __slots__ = ("msg",)

    def __init__(self, msg: str):
        self.msg = msg

    def __add__(self, _offset):
        return self


def on_gpu(ptr):
    """a tptr() result that reaches the kernel some other way than as an argument of `launch` (inside a pointer array, a launch
    table): the marker of a tensor that is not on the GPU raises here"""
    if type(ptr) is _NotOnGpu:
        raise HipLibraryError(ptr.msg)
    return ptr


def _dev(t: torch.Tensor, dtype: torch.dtype, name: str, numel: Optional[int] = None):
    if t is None:
        raise HipLibraryError(f"{name}: expected a tensor, got None")
    return tptr(t, name, dtype=dtype, numel=numel)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _failed(L, name: str, rc: int) -> HipLibraryError:
    return HipLibraryError(f"{name} failed (code {rc}): {L.vqseg_last_error().decode(errors='replace')}")


def launch(name: str, dev, *args, handle=None) -> None:
    """THE way a kernel is launched: entry point `name` of lib() (or of `handle`, another build of the same ABI) with `args` and,
    as its last argument, the current stream of `dev`, under that device's guard.  A non-zero return code raises HipLibraryError
    with `name` and vqseg_last_error().  A tensor that is not on the GPU raises before the entry point is entered -- tptr's marker
    among `args` is refused by ctypes itself -- so nothing is enqueued, and a null pointer can only mean an absent argument.  For a
    `dev` that is no GPU the marker's message is raised before any stream is asked for (a box without a GPU has none); on a 'cuda'
    device the stream handle is read while the arguments are put together, which enqueues nothing."""
    L = handle or lib()
    if type(dev) is not torch.device:
        dev = torch.device(dev)
    if dev.type == "cuda":
        try:
            with torch.cuda.device(dev):
                rc = getattr(L, name)(*args, _stream())
        except ctypes.ArgumentError:                         # costs the success path nothing
            for a in args:
                on_gpu(a)
            raise
        if rc != 0:
            raise _failed(L, name, rc)
        return
    for a in args:
        on_gpu(a)
    raise HipLibraryError(f"{name}: the HIP path needs tensors on a 'cuda' (ROCm) device; got {dev}. There is no CPU fallback.")


def _workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------------------------------
def vq_prepare(codebook: torch.Tensor) -> torch.Tensor:
    """Build the kernel-side image of a codebook (K, C); reuse it until the codebook changes."""
    L = lib()
    k, c = codebook.shape
    wp = _dev(codebook, torch.float32, "codebook")
    nbytes = L.vqseg_vq_prepared_bytes(c, k)
    blob = _workspace(nbytes, codebook.device)
    launch("vqseg_vq_prepare_f32", codebook.device, wp, c, k, blob.data_ptr(), nbytes)
    return blob


def vq_forward(rows: torch.Tensor, codebook: torch.Tensor, training: bool, commitment_weight: float,
               want_dmin: bool = False, prepared: Optional[torch.Tensor] = None):
    """rows (N, C) f32, codebook (K, C) f32 -> quant (N, C), idx (N,) i64, loss (1,), dead_pct (), [dmin (N,)]."""
    L = lib()
    n, c = rows.shape
    k = codebook.shape[0]
    bf16 = rows.dtype == torch.bfloat16                      # bf16 activations: same fp32 arithmetic, bf16 quant
    xp, wp = tptr(rows, "rows", bf=int(bf16), numel=n * c), _dev(codebook, torch.float32, "codebook", k * c)
    dev = rows.device
    quant = torch.empty_like(rows)
    idx = torch.empty(n, dtype=torch.int64, device=dev)
    scal = torch.empty(2, dtype=torch.float32, device=dev)
    dmin = torch.empty(n, dtype=torch.float32, device=dev) if want_dmin else None
    nbytes = L.vqseg_vq_workspace_bytes(n, c, k)
    ws = _workspace(nbytes, dev)
    launch("vqseg_vq_forward_bf16" if bf16 else "vqseg_vq_forward_f32", dev, xp, wp,               # the entry point must match the row type
           tptr(prepared, "prepared codebook", dtype=torch.uint8, numel=L.vqseg_vq_prepared_bytes(c, k)), n, c, k,
           int(bool(training)), float(commitment_weight), quant.data_ptr(), idx.data_ptr(), scal.data_ptr(), scal.data_ptr() + 4,
           dmin.data_ptr() if want_dmin else None, ws.data_ptr(), nbytes)
    out = (quant, idx, scal[0:1], scal[1])
    return out + (dmin,) if want_dmin else out


def bind(path: str) -> ctypes.CDLL:
    """another build of the same ABI (the per-workgroup timeline build) as a SECOND handle next to lib(): measurement code only"""
    return _bind_symbols(ctypes.CDLL(path))


def vq_forward_group(rows_list, codebooks, prepared_list, training: bool, commitment_weights, handle=None, s3: bool = False):
    """vq_forward for several independent layers with ONE distance + argmin launch (vqseg_vq_forward_group).
    -> list of (quant, idx, loss (1,), dead_pct ()) per level; bit-identical to per-level vq_forward calls.
    `handle`: another build of the library (bind()), for measurement code.
    `s3`: the rows are split-3 rows (N, 2C) bf16 = [hi | lo] (nnf.S3.rows, eval only); quant comes back in the same form."""
    L = handle or lib()
    nl = len(rows_list)
    bf16 = 2 if s3 else int(rows_list[0].dtype == torch.bfloat16)
    if s3 and training:
        raise HipLibraryError("vq_forward_group: split-3 rows are an eval-mode format (training must be False)")
    dev = rows_list[0].device
    ptr = lambda ps: (c_void_p * nl)(*map(on_gpu, ps))         # the pointers travel inside a host array: a CPU tensor raises here
    ns = np.array([r.shape[0] for r in rows_list], dtype=np.int64)
    cs = np.array([w.shape[1] for w in codebooks], dtype=np.int32)            # logical channels (a split-3 row holds twice as many elements)
    ks = np.array([w.shape[0] for w in codebooks], dtype=np.int32)
    cw = np.array([float(w) for w in commitment_weights], dtype=np.float32)
    xs, wps, preps, quants, idxs, scals, wss = [], [], [], [], [], [], []
    for r, w in zip(rows_list, codebooks):
        if r.dtype != rows_list[0].dtype:
            raise HipLibraryError("vq_forward_group: one row type per call")
        if w.dim() != 2 or r.dim() != 2 or r.shape[1] != (2 if s3 else 1) * w.shape[1]:
            raise HipLibraryError(f"vq_forward_group: rows {tuple(r.shape)} do not match a codebook {tuple(w.shape)}" + (" (split-3 rows: 2C columns)" if s3 else ""))
        xs.append(tptr(r, "rows", bf=bf16, numel=r.shape[0] * r.shape[1]))
        wps.append(_dev(w, torch.float32, "codebook", w.shape[0] * w.shape[1]))
        quants.append(torch.empty_like(r))
        idxs.append(torch.empty(r.shape[0], dtype=torch.int64, device=dev))
        scals.append(torch.empty(2, dtype=torch.float32, device=dev))
        wss.append(_workspace(L.vqseg_vq_workspace_bytes(r.shape[0], w.shape[1], w.shape[0]), dev))
    for w, p_ in zip(codebooks, prepared_list):
        preps.append(tptr(p_, "prepared codebook", dtype=torch.uint8, numel=L.vqseg_vq_prepared_bytes(w.shape[1], w.shape[0])))
    wsb = (c_size_t * nl)(*[w.numel() for w in wss])
    launch("vqseg_vq_forward_group", dev, nl, bf16, ptr(xs), ptr(wps), ptr(preps), ns.ctypes.data, cs.ctypes.data, ks.ctypes.data,
           int(bool(training)), cw.ctypes.data, ptr(q.data_ptr() for q in quants), ptr(i.data_ptr() for i in idxs),
           ptr(s.data_ptr() for s in scals), ptr(s.data_ptr() + 4 for s in scals), ptr(w.data_ptr() for w in wss),
           ctypes.cast(wsb, c_void_p), handle=handle)
    if FILTER_DIAG is not None and bf16:                     # diagnostics (tools/vq_filter_diag.py): per level (rows, channels, codes, counter of candidate pairs)
        for r, w, ws_ in zip(rows_list, codebooks, wss):
            off = L.vqseg_vq_filter_counter_offset(r.shape[0], w.shape[1], w.shape[0])
            FILTER_DIAG.append((r.shape[0], w.shape[1], w.shape[0], ws_[off:off + 256].view(torch.int32) if off else None))
    return [(q, i, s[0:1], s[1]) for q, i, s in zip(quants, idxs, scals)]


def set_option(key: str, value: int) -> int:
    """vqseg_set_option: returns the previous value"""
    prev = lib().vqseg_set_option(key.encode(), int(value))
    if prev < 0:
        raise HipLibraryError(f"vqseg_set_option: unknown option {key!r} or bad value {value}")
    return prev


def vq_tiles_per_wave(n_rows, n_codes) -> int:
    """vqseg_vq_tiles_per_wave: the code tiles per wave the distance launch of these levels (one int each, or sequences) takes"""
    rows = [n_rows] if isinstance(n_rows, int) else list(n_rows)
    codes = [n_codes] if isinstance(n_codes, int) else list(n_codes)
    if len(rows) != len(codes):
        raise ValueError("vq_tiles_per_wave: one code count per row count")
    t = lib().vqseg_vq_tiles_per_wave(len(rows), (ctypes.c_int64 * len(rows))(*rows), (c_int * len(codes))(*codes))
    if t < 0:
        raise _failed(lib(), "vqseg_vq_tiles_per_wave", t)
    return t


def vq_assign(rows: torch.Tensor, codebook: torch.Tensor, want_dmin: bool = False,
              prepared: Optional[torch.Tensor] = None, want_filter_count: bool = False, s3: bool = False, want_filter_state: bool = False):
    """`s3`: rows are split-3 rows (N, 2C) bf16 = [hi | lo]; the result is that of the merged fp32 rows.
    `want_filter_state` (diagnostics, tests): appends the candidate filter's 65 int32 words of this call -- the 64 sub-list counters of
    (row, code) pairs handed to the exact re-score, then the overflow flag (the exact kernel served the level) -- or None (no filter)."""
    L = lib()
    n, c = rows.shape
    k = codebook.shape[0]
    bf16 = rows.dtype == torch.bfloat16                      # bf16 activations: same fp32 arithmetic, bf16 quant
    if s3:
        if c != 2 * codebook.shape[1]:
            raise HipLibraryError(f"vq_assign: split-3 rows {tuple(rows.shape)} do not match a codebook {tuple(codebook.shape)} (2C columns)")
        c //= 2
    xp, wp = tptr(rows, "rows", bf=2 if s3 else int(bf16), numel=n * c * (2 if s3 else 1)), _dev(codebook, torch.float32, "codebook", k * c)
    dev = rows.device
    idx = torch.empty(n, dtype=torch.int64, device=dev)
    dmin = torch.empty(n, dtype=torch.float32, device=dev) if want_dmin else None
    nbytes = L.vqseg_vq_workspace_bytes(n, c, k)
    ws = _workspace(nbytes, dev)
    launch("vqseg_vq_assign_s3" if s3 else "vqseg_vq_assign_bf16" if bf16 else "vqseg_vq_assign_f32", dev, xp, wp,   # the entry point must match the row type
           tptr(prepared, "prepared codebook", dtype=torch.uint8, numel=L.vqseg_vq_prepared_bytes(c, k)), n, c, k,
           idx.data_ptr(), dmin.data_ptr() if want_dmin else None, ws.data_ptr(), nbytes)
    if want_filter_count:                                    # diagnostics: candidate pairs the bf16 filter handed to the exact re-score (None: no filter)
        off = L.vqseg_vq_filter_counter_offset(n, c, k) if bf16 else 0
        amb = ws[off:off + 256].view(torch.int32).sum() if off else None      # 64 sub-list counters
        return (idx, dmin, amb) if want_dmin else (idx, amb)
    if want_filter_state:
        off = L.vqseg_vq_filter_counter_offset(n, c, k) if bf16 else 0
        state = ws[off:off + 260].view(torch.int32).clone() if off else None
        return (idx, dmin, state) if want_dmin else (idx, state)
    return (idx, dmin) if want_dmin else idx


def vq_backward(grad_quant: torch.Tensor, grad_loss: Optional[torch.Tensor], rows: torch.Tensor, quant: torch.Tensor,
                commitment_weight: float) -> torch.Tensor:
    n, c = rows.shape
    gq = _dev(grad_quant, torch.float32, "grad_quant", n * c)
    gl = _dev(grad_loss, torch.float32, "grad_loss", 1) if grad_loss is not None else None
    gx = torch.empty_like(rows)
    launch("vqseg_vq_backward_f32", rows.device, gq, gl, _dev(rows, torch.float32, "rows", n * c), _dev(quant, torch.float32, "quant", n * c),
           n, c, float(commitment_weight), gx.data_ptr())
    return gx


def vq_backward_bf16(grad_quant: torch.Tensor, grad_loss: Optional[torch.Tensor], rows: torch.Tensor, idx: torch.Tensor,
                     codebook: torch.Tensor, commitment_weight: float) -> torch.Tensor:
    """bf16 activations: grad_x = grad_quant + (2 w grad_loss / (N C)) (x - codebook[idx]), e re-read in fp32."""
    n, c = rows.shape
    gq = _dev(grad_quant, torch.bfloat16, "grad_quant", n * c)
    gl = _dev(grad_loss, torch.float32, "grad_loss", 1) if grad_loss is not None else None
    gx = torch.empty_like(rows)
    if codebook.dim() != 2 or codebook.shape[1] != c:
        raise HipLibraryError(f"codebook: expected (K, {c}), got {tuple(codebook.shape)}")
    launch("vqseg_vq_backward_bf16", rows.device, gq, gl, _dev(rows, torch.bfloat16, "rows", n * c), _dev(idx, torch.int64, "idx", n),
           _dev(codebook, torch.float32, "codebook"), n, c, float(commitment_weight), gx.data_ptr())
    return gx


def kmeans(samples: torch.Tensor, means: torch.Tensor, iters: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Lloyd iterations in place on `means` (K, C); returns (means, bins (K,) i64)."""
    L = lib()
    n, c = samples.shape
    k = means.shape[0]
    sp, mp = _dev(samples, torch.float32, "samples", n * c), _dev(means, torch.float32, "means", k * c)
    bins = torch.zeros(k, dtype=torch.int64, device=samples.device)
    nbytes = L.vqseg_kmeans_workspace_bytes(n, c, k)
    ws = _workspace(nbytes, samples.device)
    launch("vqseg_kmeans_f32", samples.device, sp, mp, bins.data_ptr(), n, c, k, int(iters), ws.data_ptr(), nbytes)
    return means, bins


def kmeans_accumulate(samples: torch.Tensor, means: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """This rank's per-cluster sums (K, C) f32 and counts (K,) i64 for one Lloyd iteration."""
    L = lib()
    n, c = samples.shape
    k = means.shape[0]
    sp, mp = _dev(samples, torch.float32, "samples", n * c), _dev(means, torch.float32, "means", k * c)
    sums = torch.empty(k, c, dtype=torch.float32, device=samples.device)
    counts = torch.empty(k, dtype=torch.int64, device=samples.device)
    nbytes = L.vqseg_kmeans_workspace_bytes(n, c, k)
    ws = _workspace(nbytes, samples.device)
    launch("vqseg_kmeans_accumulate_f32", samples.device, sp, mp, n, c, k, sums.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes)
    return sums, counts


def kmeans_finalize(sums: torch.Tensor, counts: torch.Tensor, means: torch.Tensor) -> torch.Tensor:
    k, c = means.shape
    launch("vqseg_kmeans_finalize_f32", means.device, _dev(sums, torch.float32, "sums", k * c), _dev(counts, torch.int64, "counts", k),
           _dev(means, torch.float32, "means", k * c), c, k)
    return means


def vq_code_sums(rows: torch.Tensor, idx: torch.Tensor, k: int, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-code sums (K, C) f32 and counts (K,) i64 of rows (N, C) f32 / bf16 under the assignment idx (N,) i64.  `out`: the tensor the
    sums are written to (a dense (K, C) f32 view of a larger buffer, say)."""
    L = lib()
    n, c = rows.shape
    if rows.dtype not in (torch.float32, torch.bfloat16):
        raise HipLibraryError(f"rows: expected torch.float32 or torch.bfloat16, got {rows.dtype}")
    ip = _dev(idx, torch.int64, "idx", n)
    sums = torch.empty(k, c, dtype=torch.float32, device=rows.device) if out is None else out
    counts = torch.empty(k, dtype=torch.int64, device=rows.device)
    nbytes = L.vqseg_kmeans_workspace_bytes(n, c, k)
    ws = _workspace(nbytes, rows.device)
    bf = int(rows.dtype == torch.bfloat16)
    launch("vqseg_vq_code_sums", rows.device, bf, tptr(rows, "rows", bf=bf, numel=n * c), ip, n, c, k,
           sums.data_ptr() if out is None else _dev(out, torch.float32, "out", k * c), counts.data_ptr(), ws.data_ptr(), nbytes)
    return sums, counts


def vq_revive_candidates(rows: torch.Tensor, seed: int, counter: torch.Tensor, k: int, rank: int, world: int, out=None):
    """The rows of this rank that expired codes would take (include/vqseg.h: vqseg_vq_revive_candidates): -> cand (K, C) f32, ok (K,) f32.
    `counter`: the device int64 count of EMA updates so far (read on the device); `out`: a (cand, ok) pair to write into."""
    n, c = rows.shape
    if rows.dtype not in (torch.float32, torch.bfloat16):
        raise HipLibraryError(f"rows: expected torch.float32 or torch.bfloat16, got {rows.dtype}")
    bf = int(rows.dtype == torch.bfloat16)
    xp, tp = tptr(rows, "rows", bf=bf, numel=n * c), _dev(counter, torch.int64, "counter", 1)
    if out is None:
        out = (torch.empty(k, c, dtype=torch.float32, device=rows.device), torch.empty(k, dtype=torch.float32, device=rows.device))
    cand, ok = out
    launch("vqseg_vq_revive_candidates", rows.device, bf, xp, n, c, k, int(seed) & 0xFFFFFFFFFFFFFFFF, tp, int(rank), int(world),
           _dev(cand, torch.float32, "candidates", k * c), _dev(ok, torch.float32, "ok", k))
    return cand, ok


def vq_ema_update(cluster_size: torch.Tensor, embed_avg: torch.Tensor, codebook: torch.Tensor, sums: torch.Tensor,
                  counts: torch.Tensor, decay: float, eps: float, candidates: Optional[torch.Tensor] = None,
                  ok: Optional[torch.Tensor] = None, threshold: float = 0.0, counter: Optional[torch.Tensor] = None,
                  revived: Optional[torch.Tensor] = None) -> None:
    """In place: moving counts / sums and the codebook they imply (include/vqseg.h: vqseg_vq_ema_update_f32).  With `threshold` > 0 the
    dead-code revival is fused in (vqseg_vq_ema_update_revive_f32): codes whose updated count lies below it take their row of
    `candidates` where `ok` is set, `revived` (device int64) receives their number and `counter` (device int64) advances by one."""
    k, c = codebook.shape
    if cluster_size.shape != (k,) or embed_avg.shape != (k, c) or sums.shape != (k, c) or counts.shape != (k,):
        raise ValueError("vq_ema_update: shapes must be (K,), (K, C), (K, C), (K, C), (K,)")
    if threshold == 0:
        scratch = torch.empty(1, dtype=torch.float32, device=codebook.device)
        launch("vqseg_vq_ema_update_f32", codebook.device, _dev(cluster_size, torch.float32, "cluster_size"),
               _dev(embed_avg, torch.float32, "embed_avg"), _dev(codebook, torch.float32, "codebook"), _dev(sums, torch.float32, "sums"),
               _dev(counts, torch.int64, "counts"), c, k, float(decay), float(eps), scratch.data_ptr())
        return
    scratch = torch.empty(1 + k, dtype=torch.float32, device=codebook.device)
    launch("vqseg_vq_ema_update_revive_f32", codebook.device, _dev(cluster_size, torch.float32, "cluster_size"),
           _dev(embed_avg, torch.float32, "embed_avg"), _dev(codebook, torch.float32, "codebook"), _dev(sums, torch.float32, "sums"),
           _dev(counts, torch.int64, "counts"), c, k, float(decay), float(eps), scratch.data_ptr(),
           _dev(candidates, torch.float32, "candidates", k * c), _dev(ok, torch.float32, "ok", k), float(threshold),
           _dev(counter, torch.int64, "counter", 1), _dev(revived, torch.int64, "revived", 1))


def batch_u8(img_cache: torch.Tensor, img_offsets, hw: Tuple[int, int], f32_lut: torch.Tensor, img_out: torch.Tensor,
             mask_cache: Optional[torch.Tensor] = None, mask_offsets=None, mask_hw: Tuple[int, int] = (0, 0),
             label_lut: Optional[torch.Tensor] = None, target_out: Optional[torch.Tensor] = None,
             label_out: Optional[torch.Tensor] = None) -> None:
    """Gather n cached uint8 samples into a batch (include/vqseg.h: vqseg_batch_u8_f): img_out (n, 3, h, w) f32 channels_last,
    target_out (n, mh, mw) u8, label_out (n, mh, mw) i64.  Offsets are host sequences of byte offsets into the caches."""
    n = len(img_offsets)
    (h, w), (mh, mw) = hw, mask_hw
    io = np.ascontiguousarray(img_offsets, dtype=np.int64)
    mo = np.ascontiguousarray(mask_offsets, dtype=np.int64) if mask_offsets is not None else None
    if n and (int(io.min()) < 0 or int(io.max()) + h * w * 3 > img_cache.numel()):
        raise HipLibraryError("batch_u8: an image offset lies outside the image cache")
    if mask_cache is not None:
        if mo is None or len(mo) != n:
            raise HipLibraryError("batch_u8: one mask offset per sample required")
        if n and (int(mo.min()) < 0 or int(mo.max()) + mh * mw > mask_cache.numel()):
            raise HipLibraryError("batch_u8: a mask offset lies outside the mask cache")
    if img_out.dim() != 4 or not img_out.is_contiguous(memory_format=torch.channels_last):
        raise HipLibraryError("batch_u8: img_out must be a channels_last (n, 3, h, w) tensor")
    launch("vqseg_batch_u8_f", img_out.device, n, tptr(img_cache, "img_cache", dtype=torch.uint8), tptr(mask_cache, "mask_cache", dtype=torch.uint8),
           io.ctypes.data, mo.ctypes.data if mo is not None else None, h, w, mh, mw,
           tptr(f32_lut, "f32_lut", dtype=torch.float32, numel=256), tptr(label_lut, "label_lut", dtype=torch.int64, numel=256),
           tptr(img_out, "img_out", dtype=torch.float32, numel=n * 3 * h * w),
           tptr(target_out, "target_out", dtype=torch.uint8, numel=n * mh * mw),
           tptr(label_out, "label_out", dtype=torch.int64, numel=n * mh * mw))


BOX_MIX_DTYPES = (torch.uint8, torch.bfloat16, torch.float32, torch.int64)       # element widths 1, 2, 4, 8: the kernel selects by bits
BOX_MIX_CALLS = 0             # calls of box_mix that reached the library (tests assert the kernel path through it; never read by the product)


def box_mix(src: torch.Tensor, boxes, mode: str = "mix", fill=0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """CutMix / CutOut of a batch (include/vqseg.h: vqseg_box_mix_f): for src (n, P, h, w) -- NCHW-contiguous or channels_last -- or
    (n, h, w), out[s] = src[s] outside box[s] and, inside it, src[(s + 1) % n] (`mode` "mix") or `fill` ("fill").  `boxes`: n host rows
    (y1, x1, cut_h, cut_w).  Out of place: returns `out` (default: a new tensor of src's layout); src is not written."""
    global BOX_MIX_CALLS
    if mode not in ("mix", "fill"):
        raise HipLibraryError(f"box_mix: mode must be 'mix' or 'fill', got {mode!r}")
    if not isinstance(src, torch.Tensor) or src.dim() not in (3, 4):
        raise HipLibraryError("box_mix: src must be a (n, P, h, w) or (n, h, w) tensor")
    n, (h, w) = src.shape[0], src.shape[-2:]
    planes = src.shape[1] if src.dim() == 4 else 1
    bx = np.ascontiguousarray(boxes, dtype=np.int32)
    if bx.shape != (n, 4):
        raise HipLibraryError(f"box_mix: one (y1, x1, cut_h, cut_w) box per sample required: {n} samples, boxes of shape {bx.shape}")
    if n and (int(bx.min()) < 0 or int((bx[:, 0] + bx[:, 2]).max()) > h or int((bx[:, 1] + bx[:, 3]).max()) > w):
        raise HipLibraryError(f"box_mix: a box lies outside the {h} x {w} image")
    if out is None:
        out = torch.empty_like(src)                          # dense src: the same strides
    elif not isinstance(out, torch.Tensor) or out.shape != src.shape or out.stride() != src.stride():
        raise HipLibraryError("box_mix: out must have src's shape and layout")
    numel = n * planes * h * w
    sp, op = tptr(src, "src", dtype=BOX_MIX_DTYPES, numel=numel), tptr(out, "out", dtype=src.dtype, numel=numel)
    if numel == 0:
        raise HipLibraryError("box_mix: empty tensor")
    # tptr admits two dense layouts; the strides are stated from the layout (a size-1 dimension's own stride is arbitrary)
    strides = (planes * h * w, h * w, 1) if src.is_contiguous() else (planes * h * w, 1, planes)
    bits = int.from_bytes(torch.tensor([fill], dtype=src.dtype).view(torch.uint8).numpy().tobytes(), "little") if mode == "fill" else 0
    launch("vqseg_box_mix_f", src.device, int(mode == "fill"), src.element_size(), sp, op, n, planes, h, w, *strides, bx.ctypes.data, bits)
    BOX_MIX_CALLS += 1
    return out


AFFINE_WARP_BILINEAR_DTYPES = (torch.float32, torch.bfloat16)
AFFINE_WARP_NEAREST_DTYPES = (torch.uint8, torch.int8, torch.bool, torch.int16, torch.bfloat16, torch.float16, torch.int32, torch.float32, torch.int64,
                              torch.float64)             # element widths 1, 2, 4, 8: nearest selects by bits
AFFINE_WARP_CALLS = 0         # calls of affine_warp that reached the library (as BOX_MIX_CALLS: for tests, never read by the product)


def affine_warp(src: torch.Tensor, matrices, mode: str = "bilinear", fill=0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A batch resampled through one 2 x 2 matrix per sample (include/vqseg.h: vqseg_affine_warp_f): src (n, P, h, w) -- NCHW-contiguous
    or channels_last -- or (n, h, w); `matrices`: n host rows (M00, M01, 0, M10, M11, 0) mapping an output pixel's offset from the image
    centre to its source's.  `mode` "bilinear" (float32 / bfloat16, zero padding) or "nearest" (any 1 / 2 / 4 / 8-byte dtype, by bits;
    a source outside the image gives `fill`).  Out of place: returns `out` (default: a new tensor of src's layout; a given `out` has
    src's shape and per-sample layout and may have a larger sample stride); src is not written."""
    global AFFINE_WARP_CALLS
    if mode not in ("bilinear", "nearest"):
        raise HipLibraryError(f"affine_warp: mode must be 'bilinear' or 'nearest', got {mode!r}")
    if not isinstance(src, torch.Tensor) or src.dim() not in (3, 4):
        raise HipLibraryError("affine_warp: src must be a (n, P, h, w) or (n, h, w) tensor")
    n, (h, w) = src.shape[0], src.shape[-2:]
    planes = src.shape[1] if src.dim() == 4 else 1
    try:
        mats = np.ascontiguousarray(matrices, dtype=np.float32)
    except (TypeError, ValueError):
        raise HipLibraryError("affine_warp: matrices must be n rows of six numbers") from None
    if mats.shape != (n, 6):
        raise HipLibraryError(f"affine_warp: one (M00, M01, 0, M10, M11, 0) row per sample required: {n} samples, matrices of shape {mats.shape}")
    if not np.isfinite(mats).all():
        raise HipLibraryError("affine_warp: a matrix entry is not finite")
    if mats[:, (2, 5)].any():
        raise HipLibraryError("affine_warp: the translation slots (entries 2 and 5 of a row) are reserved and must be 0")
    dtypes = AFFINE_WARP_BILINEAR_DTYPES if mode == "bilinear" else AFFINE_WARP_NEAREST_DTYPES
    numel = n * planes * h * w
    sp = tptr(src, "src", dtype=dtypes, numel=numel)
    if numel == 0:
        raise HipLibraryError("affine_warp: empty tensor")
    # tptr admits two dense layouts; the strides are stated from the layout (a size-1 dimension's own stride is arbitrary)
    planar = src.is_contiguous()
    inner = (h * w, 1) if planar else (1, planes)
    out_stride = planes * h * w
    if out is None:
        out = torch.empty_like(src)                          # dense src: the same strides
        op = tptr(out, "out", dtype=src.dtype, numel=numel)
    else:
        if not isinstance(out, torch.Tensor) or out.shape != src.shape:
            raise HipLibraryError("affine_warp: out must have src's shape and layout")
        one = out[:1]                                        # a sample of out: dense in src's layout; samples at least a sample apart
        if (one.is_contiguous() if planar else (one.dim() == 4 and one.is_contiguous(memory_format=torch.channels_last))) and \
                (n == 1 or out.stride(0) >= out_stride):
            out_stride = out.stride(0) if n > 1 else out_stride
        else:
            raise HipLibraryError("affine_warp: out must have src's shape and layout")
        op = tptr(out, "out", dtype=src.dtype, numel=numel, dense=False)
        if type(sp) is int and type(op) is int and sp == op:
            raise HipLibraryError("affine_warp: out of place only")
    bits = int.from_bytes(torch.tensor([fill], dtype=src.dtype).view(torch.uint8).numpy().tobytes(), "little") if mode == "nearest" else 0
    launch("vqseg_affine_warp_f", src.device, int(mode == "nearest"), src.element_size(), sp, op, n, planes, h, w, planes * h * w, out_stride,
           *inner, mats.ctypes.data, bits)
    AFFINE_WARP_CALLS += 1
    return out


PHOTOMETRIC_CALLS = 0         # calls of photometric that reached the library (as BOX_MIX_CALLS: for tests, never read by the product)
PHOTOMETRIC_MAX_RADIUS = 8    # include/vqseg.h: R = ceil(3 sigma) <= 8
PHOTOMETRIC_ARG_SAMPLES = 32  # parameter rows per launch (csrc/photometric_kernels.hip: PHOTO_ARG_SAMPLES)
PHOTOMETRIC_MEAN_THREADS = 256        # the mean pass: pixel q of a sample goes to thread q % (256 P), P = photometric_mean_blocks(h w)
PHOTOMETRIC_MEAN_FOLD_LEVELS = 6 + 2 + 6      # wave shuffle tree, the workgroup's four wave sums pairwise, the main pass's tree over the P partials


def photometric_mean_blocks(pixels: int) -> int:
    """vqseg_photometric_mean_blocks: the workgroups (1..64) that share one sample's mean reduction, a function of h * w alone"""
    p = lib().vqseg_photometric_mean_blocks(int(pixels))
    if p <= 0:
        raise _failed(lib(), "vqseg_photometric_mean_blocks", p)
    return p


def photometric_mean_run(pixels: int) -> int:
    """the longest run of values one thread of the mean pass adds in sequence"""
    per = PHOTOMETRIC_MEAN_THREADS * photometric_mean_blocks(pixels)
    return (int(pixels) + per - 1) // per


def photometric_radius(sigma: float) -> int:
    """R = ceil(3 sigma) in float64 (0 for sigma = 0)"""
    return int(math.ceil(3.0 * float(sigma)))


@functools.lru_cache(maxsize=4096)
def _half_taps(sigma: float):
    """(R, [w_0 .. w_R]) in float64: exp(-i^2 / 2 sigma^2) over the exactly rounded sum of all 2R + 1 of them (math.fsum: no order of
    addition to state).  Plain Python floats: a step draws one sigma per sample, and this runs on the host inside the step."""
    if not (math.isfinite(sigma) and sigma >= 0.0):
        raise ValueError(f"photometric_taps: sigma must be finite and >= 0, got {sigma!r}")
    r = photometric_radius(sigma)
    if r > PHOTOMETRIC_MAX_RADIUS:
        raise ValueError(f"photometric_taps: sigma {sigma} gives the radius ceil(3 sigma) = {r}, above {PHOTOMETRIC_MAX_RADIUS}")
    if r == 0:
        return 0, (1.0,)
    e = [math.exp(-(i * i) / (2.0 * sigma * sigma)) for i in range(r + 1)]
    total = math.fsum(e + e[1:])
    return r, tuple(v / total for v in e)


def photometric_taps(sigma: float) -> np.ndarray:
    """the 2R + 1 float32 taps of the blur, R = ceil(3 sigma): exp(-i^2 / 2 sigma^2) normalised, computed in float64 and rounded once;
    symmetric by construction.  sigma = 0: the single tap 1."""
    r, half = _half_taps(float(sigma))
    return np.asarray(half[:0:-1] + half, dtype=np.float32)


def photometric_rows(params, n: int, h: int, w: int):
    """-> (params float32 (n, 6), radii int32 (n,), taps float32 (n, 9)) of n host rows (b, c, sat, hue, gray, sigma), checked: what
    both the kernel and the torch-op form of the definition are handed.  The rows are rounded to float32 FIRST: a sample's taps are
    those of its float32 sigma.  ValueError for what the definition excludes."""
    try:
        rows = np.ascontiguousarray(params, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError("photometric: params must be n rows of six numbers (b, c, sat, hue, gray, sigma)") from None
    if rows.shape != (n, 6):
        raise ValueError(f"photometric: one (b, c, sat, hue, gray, sigma) row per sample required: {n} samples, params of shape {rows.shape}")
    if not np.isfinite(rows).all():
        raise ValueError("photometric: a parameter is not finite")
    if (rows[:, (0, 1, 2, 5)] < 0).any():
        raise ValueError("photometric: brightness, contrast, saturation and sigma must be >= 0")
    if (np.abs(rows[:, 3]) > 0.5).any():
        raise ValueError("photometric: |hue| must be <= 0.5")
    if not np.isin(rows[:, 4], (0.0, 1.0)).all():
        raise ValueError("photometric: gray must be 0 or 1")
    radii, taps, pad = [], [], (0.0,) * PHOTOMETRIC_MAX_RADIUS
    for sigma in rows[:, 5].tolist():
        r, half = _half_taps(sigma) if sigma else (0, (1.0,))                # ValueError for R > 8
        if r > min(h, w) - 1:
            raise ValueError(f"photometric: sigma {sigma} gives the radius {r}, above min(h, w) - 1 = {min(h, w) - 1} (reflect-101 borders)")
        radii.append(r)
        taps.append((half + pad)[:PHOTOMETRIC_MAX_RADIUS + 1])
    return rows, np.asarray(radii, dtype=np.int32), np.asarray(taps, dtype=np.float32).reshape(n, PHOTOMETRIC_MAX_RADIUS + 1)


def photometric(src: torch.Tensor, params, out: Optional[torch.Tensor] = None, return_means: bool = False):
    """The photometric strong augmentation of a batch (include/vqseg.h: vqseg_photometric_f): src (n, 3, h, w) float32, NCHW-contiguous or
    channels_last; `params`: n host rows (b, c, sat, hue, gray, sigma).  Out of place: returns `out` (default: a new tensor of src's
    layout); src is not written.  `return_means`: -> (out, means), means (n,) float32 holding the contrast op's per-sample mean for the
    rows with c != 1 and 0 elsewhere."""
    global PHOTOMETRIC_CALLS
    if not isinstance(src, torch.Tensor) or src.dim() != 4 or src.shape[1] != 3:
        raise ValueError("photometric: src must be a (n, 3, h, w) tensor of RGB planes")
    if src.dtype != torch.float32:
        raise ValueError(f"photometric: src must be float32, got {src.dtype}")
    n, _c, h, w = src.shape
    rows, radii, taps = photometric_rows(params, n, h, w)
    numel = n * 3 * h * w
    sp = tptr(src, "src", dtype=torch.float32, numel=numel)
    if numel == 0:
        raise HipLibraryError("photometric: empty tensor")
    if out is None:
        out = torch.empty_like(src)                          # dense src: the same strides
    elif not isinstance(out, torch.Tensor) or out.shape != src.shape or out.stride() != src.stride():
        raise HipLibraryError("photometric: out must have src's shape and layout")
    op = tptr(out, "out", dtype=torch.float32, numel=numel)
    if type(sp) is int and type(op) is int and sp == op:
        raise HipLibraryError("photometric: out of place only")
    strides = (3 * h * w, h * w, 1) if src.is_contiguous() else (3 * h * w, 1, 3)
    need_mean = bool((rows[:, 1] != 1.0).any())
    partials = means = None
    if src.is_cuda and (need_mean or return_means):
        if need_mean:
            partials = torch.empty(n * photometric_mean_blocks(h * w), dtype=torch.float32, device=src.device)
        if return_means:
            means = torch.zeros(n, dtype=torch.float32, device=src.device)
    launch("vqseg_photometric_f", src.device, sp, op, n, h, w, *strides, rows.ctypes.data, radii.ctypes.data, taps.ctypes.data,
           partials.data_ptr() if partials is not None else None, means.data_ptr() if means is not None else None)
    PHOTOMETRIC_CALLS += 1
    return (out, means) if return_means else out


RENDER_KINDS = {"image": 0, "target": 1, "pred": 2, "detail": 3, "mix_pred": 4, "mix_detail": 5, "fill": 6}     # include/vqseg.h: vqseg_render_sheet_u8
RENDER_SHEET_CALLS = 0        # calls of render_sheet that reached the library (as BOX_MIX_CALLS: for tests, never read by the product)


def render_sheet(canvas: torch.Tensor, panels, size, num_classes: int, palette, fill=(1.0, 1.0, 1.0), image: Optional[torch.Tensor] = None,
                 pred: Optional[torch.Tensor] = None, target: Optional[torch.Tensor] = None, alpha: float = 0.4, box2: bool = False,
                 cols: Optional[int] = None) -> torch.Tensor:
    """The RGB bytes of a panel sheet (include/vqseg.h: vqseg_render_sheet_u8) written into `canvas`, a (rows, cols, 3) uint8 tensor
    whose pixels are dense (strides (pitch, 3, 1): a view of a larger canvas qualifies) -- the full-resolution sheet of b * ho rows, or
    with `box2` its half in both directions.  `panels`: (kind, x0, width) rows, kind a key of RENDER_KINDS, x0 / width in full-resolution
    columns; `size` = (b, ho, wo); `palette`: (2 C + 1, 3) floats in [0, 1] (C class colours, C "wrong" colours, the ignore colour),
    taken in float64 for the byte rows; `image` (b, 3, h, w) f32 NCHW-contiguous or channels_last, `pred` (b, ho, wo) u8, `target`
    (b, ht, wt) i64: each only where a panel needs it.  `cols`: the full-resolution sheet's width (default: the canvas's, doubled with
    box2).  Returns `canvas`; bytes outside the panels keep their value.  There is no CPU path."""
    global RENDER_SHEET_CALLS
    E = HipLibraryError
    b, ho, wo = (int(v) for v in size)
    c = int(num_classes)
    rows = b * ho
    if not isinstance(canvas, torch.Tensor) or canvas.dim() != 3 or canvas.shape[2] != 3:
        raise E("render_sheet: canvas must be a (rows, cols, 3) uint8 tensor")
    orows, ocols = int(canvas.shape[0]), int(canvas.shape[1])
    cols = ocols * (2 if box2 else 1) if cols is None else int(cols)
    if box2 and (rows % 2 or cols % 2):
        raise E(f"render_sheet: box2 needs a sheet of even height and width, got {rows} x {cols}")
    if (orows, ocols) != ((rows // 2, cols // 2) if box2 else (rows, cols)):
        raise E(f"render_sheet: a {rows} x {cols} sheet{' halved by box2' if box2 else ''} needs a canvas of "
                f"{(rows // 2, cols // 2) if box2 else (rows, cols)} pixels, got {(orows, ocols)}")
    if orows == 0 or ocols == 0:
        raise E("render_sheet: empty canvas")
    if canvas.stride(2) != 1 or (ocols > 1 and canvas.stride(1) != 3) or (orows > 1 and canvas.stride(0) < 3 * ocols):
        raise E(f"render_sheet: canvas pixels must be dense RGB bytes with rows at least a row apart, got strides {tuple(canvas.stride())}")
    pitch = canvas.stride(0) if orows > 1 else 3 * ocols
    rows_ = [(RENDER_KINDS.get(k, -1) if isinstance(k, str) else int(k), int(x), int(wd)) for k, x, wd in panels]
    if any(k < 0 for k, _, _ in rows_):
        raise E(f"render_sheet: panel kinds are {sorted(RENDER_KINDS)}, got {[p[0] for p in panels]}")
    pal = np.ascontiguousarray(palette, dtype=np.float64)
    if pal.shape != (2 * c + 1, 3):
        raise E(f"render_sheet: the palette of {c} classes has {2 * c + 1} rows of 3 (class, wrong, ignore), got shape {pal.shape}")
    fil = np.ascontiguousarray(fill, dtype=np.float64).reshape(-1)
    if fil.shape != (3,):
        raise E("render_sheet: fill is one RGB colour")
    pal_f, fil_f = pal.astype(np.float32), fil.astype(np.float32)
    pal_u, fil_u = (np.floor(np.clip(a, 0.0, 1.0) * 255.0).astype(np.uint8) for a in (pal, fil))      # float64: float32(230 / 255) * 255 < 230
    ip = pp = tp = None
    strides, (h, w), (ht, wt) = (0, 0, 0), (0, 0), (0, 0)
    if image is not None:
        if not isinstance(image, torch.Tensor) or image.dim() != 4 or image.shape[0] != b or image.shape[1] != 3:
            raise E(f"render_sheet: image must be a ({b}, 3, h, w) tensor")
        h, w = int(image.shape[2]), int(image.shape[3])
        ip = tptr(image, "image", dtype=torch.float32, numel=b * 3 * h * w)
        # tptr admits two dense layouts; the strides are stated from the layout (a size-1 dimension's own stride is arbitrary)
        strides = (3 * h * w, h * w, 1) if image.is_contiguous() else (3 * h * w, 1, 3)
    if pred is not None:
        if not isinstance(pred, torch.Tensor) or tuple(pred.shape) != (b, ho, wo):
            raise E(f"render_sheet: pred must have the shape {(b, ho, wo)}, got {tuple(getattr(pred, 'shape', ()))}")
        pp = tptr(pred, "pred", dtype=torch.uint8, numel=b * ho * wo)
    if target is not None:
        if not isinstance(target, torch.Tensor) or target.dim() != 3 or target.shape[0] != b:
            raise E(f"render_sheet: target must be a ({b}, ht, wt) tensor")
        ht, wt = int(target.shape[1]), int(target.shape[2])
        tp = tptr(target, "target", dtype=torch.int64, numel=b * ht * wt)
    cp = tptr(canvas, "canvas", dtype=torch.uint8, numel=orows * ocols * 3, dense=False)
    arr = np.ascontiguousarray(rows_, dtype=np.int32).reshape(-1, 3).T.copy()           # kinds, x0s, widths
    launch("vqseg_render_sheet_u8", canvas.device, ip, *strides, h, w, pp, tp, ht, wt, b, ho, wo, c, arr[0].ctypes.data, arr[1].ctypes.data,
           arr[2].ctypes.data, len(rows_), pal_f.ctypes.data, pal_u.ctypes.data, fil_f.ctypes.data, fil_u.ctypes.data, float(alpha), int(bool(box2)),
           cp, pitch, rows, cols)
    RENDER_SHEET_CALLS += 1
    return canvas


def _checked(name: str, *args, counts: bool = False) -> int:
    """an entry point that takes no stream: any non-zero return code is an error (a HIP error code is positive); with `counts`
    the entry point answers a count (>= 0) and only a negative code is one"""
    rc = getattr(lib(), name)(*args)
    if rc < 0 or (rc and not counts):
        raise _failed(lib(), name, rc)
    return rc


def profile_begin(capacity: int = 4096) -> None:
    _checked("vqseg_profile_begin", int(capacity))


def conv_profile_begin(capacity: int = 65536) -> None:
    _checked("vqseg_conv_profile_begin", int(capacity))


def conv_profile_collect(capacity: int = 65536, with_shape: bool = False):
    """-> list of (algorithmic flops, kind = KH * 100 + {0 bf16, 1 precise, 2 split-3}, milliseconds) per convolution launch"""
    fl = np.zeros(capacity, dtype=np.float64)
    kd = np.zeros(capacity, dtype=np.int32)
    ms = np.zeros(capacity, dtype=np.float32)
    sh = np.zeros((capacity, 4), dtype=np.int32)
    cnt = _checked("vqseg_conv_profile_collect", capacity, fl.ctypes.data, kd.ctypes.data, ms.ctypes.data, sh.ctypes.data if with_shape else None, counts=True)
    if with_shape:
        return [(float(fl[i]), int(kd[i]), float(ms[i]), tuple(int(v) for v in sh[i])) for i in range(cnt)]
    return [(float(fl[i]), int(kd[i]), float(ms[i])) for i in range(cnt)]


def profile_collect(capacity: int = 4096, with_kind: bool = False):
    """-> list of (n_rows, channels, n_codes, milliseconds[, kind]) for every assign launch since profile_begin
    (kind 0: exact kernel on f32 rows, 1: exact kernel on bf16 rows, 2: bf16 candidate filter + exact re-score)."""
    n = np.zeros(capacity, dtype=np.int64)
    c = np.zeros(capacity, dtype=np.int32)
    k = np.zeros(capacity, dtype=np.int32)
    ms = np.zeros(capacity, dtype=np.float32)
    kd = np.zeros(capacity, dtype=np.int32)
    cnt = _checked("vqseg_profile_collect", capacity, n.ctypes.data, c.ctypes.data, k.ctypes.data, ms.ctypes.data, kd.ctypes.data, counts=True)
    if with_kind:
        return [(int(n[i]), int(c[i]), int(k[i]), float(ms[i]), int(kd[i])) for i in range(cnt)]
    return [(int(n[i]), int(c[i]), int(k[i]), float(ms[i])) for i in range(cnt)]
