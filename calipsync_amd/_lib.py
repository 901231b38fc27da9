"""ctypes binding of libcasync_hip.so (include/casync_hip.h).

The product path has NO fallback: if the library is missing or a call fails, a
RuntimeError is raised with the library's own message."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import build as _build

_lib: Optional[C.CDLL] = None

c_f32p = C.c_void_p       # device pointers travel as integers
c_i64 = C.c_int64


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("kernel", C.c_char * 64), ("ms", C.c_float), ("ms_raw", C.c_float), ("flops", C.c_double),
                ("bytes", C.c_double)]


_PROTOS = {
    "casync_abi_version": (C.c_int, []),
    "casync_last_error": (C.c_char_p, []),
    "casync_packed_count": (C.c_int, []),
    "casync_packed_name": (C.c_char_p, [C.c_int]),
    "casync_packed_offset": (c_i64, [C.c_int]),
    "casync_packed_size": (c_i64, [C.c_int]),
    "casync_packed_total": (c_i64, []),
    "casync_packed_count_m": (C.c_int, [C.c_int]),
    "casync_packed_name_m": (C.c_char_p, [C.c_int, C.c_int]),
    "casync_packed_offset_m": (c_i64, [C.c_int, C.c_int]),
    "casync_packed_size_m": (c_i64, [C.c_int, C.c_int]),
    "casync_packed_total_m": (c_i64, [C.c_int]),
    "casync_workspace_bytes": (c_i64, [C.c_int]),
    "casync_workspace_bytes_dt": (c_i64, [C.c_int, C.c_int]),
    "casync_workspace_bytes_h": (c_i64, [C.c_void_p, C.c_int]),
    "casync_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "casync_get_option": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]),
    "casync_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "casync_create_ex": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "casync_create_mode": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "casync_destroy": (None, [C.c_void_p]),
    "casync_load_weights_host": (C.c_int, [C.c_void_p, C.c_void_p, c_i64]),
    "casync_load_weights_device": (C.c_int, [C.c_void_p, c_f32p, c_i64]),
    "casync_forward": (C.c_int, [C.c_void_p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_void_p, c_i64,
                                 C.c_void_p]),
    "casync_forward_windows": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, C.c_void_p, c_f32p, C.c_int,
                                         C.c_void_p, c_i64, C.c_void_p]),
    "casync_tap": (c_i64, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, c_f32p, c_i64, C.c_void_p]),
    "casync_profile_forward": (C.c_int, [C.c_void_p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_void_p,
                                         c_i64, C.c_void_p, C.POINTER(KernelTime), C.c_int]),
    "casync_op_set_dtype": (C.c_int, [C.c_int]),
    "casync_debug_gemm_stamps": (C.c_int, [C.c_void_p]),
    "casync_debug_ir_stamps": (C.c_int, [C.c_void_p]),
    "casync_debug_launch_log": (C.c_int, [C.c_int]),
    "casync_debug_launched": (C.c_int, [C.c_char_p, C.c_int]),
    "casync_op_pw_gemm": (C.c_int, [c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_int, c_f32p, C.c_int, c_f32p, c_f32p,
                                    C.c_int, c_f32p, c_f32p, C.c_void_p]),
    "casync_op_dw3x3": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int,
                                  C.c_int, C.c_int, C.c_void_p]),
    "casync_op_dw3x3_ups": (C.c_int, [c_f32p, c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p]),
    "casync_op_pw_dw": (C.c_int, [c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_int, C.c_int, c_f32p, C.c_int, C.c_void_p]),
    "casync_op_pw_dw_rect": (C.c_int, [c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_pw_gemm_ups": (C.c_int, [c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        c_f32p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_ir_fused": (C.c_int, [c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p,
                                     c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_void_p]),
    "casync_op_ir_fused_up": (C.c_int, [c_f32p, C.c_int, C.c_int, c_f32p, C.c_int, c_f32p, c_f32p, c_f32p,
                                        c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_ir_fused_upg": (C.c_int, [c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p,
                                         c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p]),
    "casync_op_upsample2x": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p]),
    "casync_op_cross_attention": (C.c_int, [c_f32p, C.c_int, c_f32p, C.c_int, c_f32p, C.c_int,
                                            c_f32p, C.c_int, c_f32p, c_f32p, C.c_int, C.c_int,
                                            C.c_void_p]),
    "casync_op_conv3x3": (C.c_int, [C.c_void_p, C.c_void_p, c_f32p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_conv3x3_ex": (C.c_int, [C.c_void_p, C.c_void_p, c_f32p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    # host only: (tile, tap) pairs of that conv with all nine taps / as walked with conv_skip
    "casync_conv3x3_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(c_i64),
                                     C.POINTER(c_i64)]),
    "casync_op_audio_windows": (C.c_int, [c_f32p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_crop_to_input": (C.c_int, [C.c_void_p, c_f32p, C.c_int, C.c_void_p]),
    "casync_op_pred_to_u8": (C.c_int, [c_f32p, C.c_void_p, C.c_int, C.c_void_p]),
    "casync_frame_prepare": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, c_f32p, C.c_void_p]),
    "casync_frame_paste_back": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_f32p, C.c_int,
                                          C.c_int, C.c_int, C.c_int, c_i64, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "casync_op_nchw_to_nhwc": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_inc": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_outc": (C.c_int, [c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int, C.c_void_p]),
    # HuBERT feature extractor (ABI 8)
    "casync_hubert_packed_count": (C.c_int, [C.c_int]),
    "casync_hubert_packed_name": (C.c_char_p, [C.c_int, C.c_int]),
    "casync_hubert_packed_offset": (c_i64, [C.c_int, C.c_int]),
    "casync_hubert_packed_size": (c_i64, [C.c_int, C.c_int]),
    "casync_hubert_packed_total": (c_i64, [C.c_int]),
    "casync_hubert_tokens": (c_i64, [c_i64]),
    "casync_hubert_workspace_bytes": (c_i64, [C.c_int, c_i64]),
    "casync_hubert_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "casync_hubert_destroy": (None, [C.c_void_p]),
    "casync_hubert_load_weights_host": (C.c_int, [C.c_void_p, C.c_void_p, c_i64]),
    "casync_hubert_load_weights_device": (C.c_int, [C.c_void_p, c_f32p, c_i64]),
    "casync_hubert_forward": (C.c_int, [C.c_void_p, c_f32p, C.c_int, c_i64, c_f32p, C.c_void_p, c_i64, C.c_void_p]),
    "casync_hubert_forward_tap": (C.c_int, [C.c_void_p, c_f32p, C.c_int, c_i64, C.c_int, C.c_int, c_f32p, C.c_void_p, c_i64,
                                            C.c_void_p]),
    "casync_op_hubert_conv0": (C.c_int, [c_f32p, C.c_int, C.c_int, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p]),
    "casync_op_hubert_layernorm": (C.c_int, [c_f32p, C.c_int, c_f32p, C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, C.c_float,
                                             C.c_int, C.c_void_p]),
    "casync_op_hubert_posconv": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_hubert_attention": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_rows_gemm": (C.c_int, [c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      c_f32p, C.c_int, C.c_void_p]),
    # HuBERT, bf16 precision (ABI 10); c_f32p is c_void_p: bf16 buffers pass the same way
    "casync_hubert_create_ex": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "casync_hubert_workspace_bytes_h": (c_i64, [C.c_void_p, C.c_int, c_i64]),
    "casync_op_hubert16_conv0": (C.c_int, [c_f32p, C.c_int, C.c_int, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_void_p]),
    "casync_op_hubert16_layernorm512": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, c_f32p, c_f32p, C.c_float,
                                                  C.c_int, C.c_int, C.c_void_p]),
    "casync_op_hubert16_layernorm1024": (C.c_int, [c_f32p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                   c_f32p, c_f32p, C.c_float, C.c_int, C.c_void_p]),
    "casync_op_hubert16_gelu": (C.c_int, [C.c_void_p, c_i64, C.c_void_p]),
    "casync_op_hubert16_widen": (C.c_int, [C.c_void_p, c_f32p, c_i64, C.c_void_p]),
    "casync_op_hubert16_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_rows_gemm_bf16": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, c_f32p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p]),
    # PFLD_GhostOne landmark network (ABI 11)
    "casync_pfld_packed_count": (C.c_int, []),
    "casync_pfld_packed_name": (C.c_char_p, [C.c_int]),
    "casync_pfld_packed_offset": (c_i64, [C.c_int]),
    "casync_pfld_packed_size": (c_i64, [C.c_int]),
    "casync_pfld_packed_total": (c_i64, []),
    "casync_pfld_workspace_bytes": (c_i64, [C.c_int]),
    "casync_pfld_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "casync_pfld_destroy": (None, [C.c_void_p]),
    "casync_pfld_load_weights_host": (C.c_int, [C.c_void_p, C.c_void_p, c_i64]),
    "casync_pfld_load_weights_device": (C.c_int, [C.c_void_p, c_f32p, c_i64]),
    "casync_pfld_forward": (C.c_int, [C.c_void_p, c_f32p, C.c_int, c_f32p, C.c_void_p, c_i64, C.c_void_p]),
    "casync_pfld_forward_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, c_f32p, C.c_void_p, c_i64, C.c_void_p]),
    "casync_pfld_forward_tap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, c_f32p, C.c_void_p, c_i64,
                                          C.c_void_p]),
    "casync_op_pfld_stem": (C.c_int, [C.c_void_p, C.c_int, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int,
                                      C.c_int, C.c_int, C.c_void_p]),
    "casync_op_pfld_ghost": (C.c_int, [c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, c_f32p, C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_pfld_dw_s2": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_pfld_head": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), c_f32p, c_f32p, c_f32p,
                                      c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_void_p]),
    # S3FD face detector (ABI 12)
    "casync_s3fd_packed_count": (C.c_int, []),
    "casync_s3fd_packed_name": (C.c_char_p, [C.c_int]),
    "casync_s3fd_packed_offset": (c_i64, [C.c_int]),
    "casync_s3fd_packed_size": (c_i64, [C.c_int]),
    "casync_s3fd_packed_total": (c_i64, []),
    "casync_s3fd_priors": (c_i64, [C.c_int, C.c_int]),
    "casync_s3fd_map_size": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "casync_s3fd_workspace_bytes": (c_i64, [C.c_int, C.c_int, C.c_int]),
    "casync_s3fd_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "casync_s3fd_destroy": (None, [C.c_void_p]),
    "casync_s3fd_load_weights_host": (C.c_int, [C.c_void_p, C.c_void_p, c_i64]),
    "casync_s3fd_load_weights_device": (C.c_int, [C.c_void_p, c_f32p, c_i64]),
    "casync_s3fd_forward": (C.c_int, [C.c_void_p, c_f32p, C.c_int, C.c_int, C.c_int, c_f32p, C.c_void_p, c_i64, C.c_void_p]),
    "casync_s3fd_forward_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, c_f32p, C.c_void_p, c_i64, C.c_void_p]),
    "casync_s3fd_forward_tap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, C.c_void_p,
                                          c_i64, C.c_void_p]),
    "casync_op_s3fd_stem": (C.c_int, [C.c_void_p, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_s3fd_maxpool": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_s3fd_im2col_dil": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_s3fd_relu": (C.c_int, [c_f32p, c_i64, C.c_void_p]),
    "casync_op_s3fd_l2norm": (C.c_int, [c_f32p, c_f32p, c_i64, C.c_int, C.c_void_p]),
    "casync_op_s3fd_head": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_void_p]),
    "casync_op_s3fd_decode": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    # S3FD, bf16 precision (ABI 13); bf16 buffers pass as c_void_p
    "casync_s3fd_create_ex": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "casync_s3fd_precision": (C.c_int, [C.c_void_p]),
    "casync_s3fd_workspace_bytes_ex": (c_i64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "casync_op_s3fd16_stem": (C.c_int, [C.c_void_p, C.c_int, c_f32p, c_f32p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_s3fd16_maxpool": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_s3fd16_im2col_dil": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_s3fd16_relu": (C.c_int, [C.c_void_p, c_i64, C.c_void_p]),
    "casync_op_s3fd16_widen": (C.c_int, [C.c_void_p, c_f32p, c_i64, C.c_void_p]),
    "casync_op_s3fd16_l2norm": (C.c_int, [C.c_void_p, C.c_void_p, c_i64, C.c_int, C.c_void_p]),
    "casync_op_s3fd16_head": (C.c_int, [C.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_void_p]),
    # face pipeline between the two networks (additive to ABI 13); geom is HOST memory, everything else device
    "casync_op_resize_linear_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double,
                                             C.c_void_p]),
    "casync_op_face_crops192": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "casync_op_s3fd_candidates": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, c_f32p, C.c_void_p]),
    "casync_op_landmarks_finalize": (C.c_int, [c_f32p, c_f32p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    # S3FD's two NMS passes behind s3fd_candidates (additive to ABI 13); faces is float64, detect_out / detect_n may be null
    "casync_op_s3fd_nms": (C.c_int, [c_f32p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, c_f32p,
                                     C.c_void_p, C.c_void_p]),
    # a clip resident on the device (additive to ABI 13); rec is HOST memory: [batch][8] int32 = {frame, y0, x0, h, w, valid, region
    # byte offset, 0}
    "casync_op_clip_gather": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, c_i64, C.c_void_p]),
    "casync_op_clip_compose": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, c_i64, C.c_void_p,
                                         C.c_void_p]),
    # baseline JPEG of finished frames (additive to ABI 13); jpeg_header is host only and returns the header's length, scratch is
    # casync_op_jpeg_workspace_bytes long, offsets int64 [batch + 1] and status int32 [batch] on the device
    "casync_op_jpeg_header": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "casync_op_jpeg_workspace_bytes": (c_i64, [C.c_int, C.c_int, C.c_int, c_i64]),
    "casync_op_jpeg_encode": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, c_i64, C.c_void_p, c_i64, C.c_void_p, c_i64,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    # the same trio for 4:2:0 (additive to ABI 13): rows are rows of 16 x 16 MCUs
    "casync_op_jpeg420_header": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "casync_op_jpeg420_workspace_bytes": (c_i64, [C.c_int, C.c_int, C.c_int, c_i64]),
    "casync_op_jpeg420_encode": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, c_i64, C.c_void_p, c_i64, C.c_void_p, c_i64,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    # baseline JPEG files -> frames (additive to ABI 13); rec is HOST memory, [batch][16] int32 (include/casync_hip.h), data holds the
    # files' scans, segment lists and table blocks on the device, status int32 [batch] on the device
    "casync_op_jpegdec_workspace_bytes": (c_i64, [C.c_int, C.c_int, C.c_int, C.c_int, c_i64]),
    "casync_op_jpegdec_decode": (C.c_int, [C.c_void_p, c_i64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, c_i64,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    # Motion-JPEG files -> frames (additive to ABI 13): the same record, its sampling word 0 (4:4:4), 1 (4:2:2), 2 (4:2:0) or 3 (gray)
    "casync_op_mjpegdec_workspace_bytes": (c_i64, [C.c_int, C.c_int, C.c_int, c_i64]),
    "casync_op_mjpegdec_decode": (C.c_int, [C.c_void_p, c_i64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, c_i64, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    # SyncNet_color, the lip-sync judge (additive to ABI 13); mode is AUDIO_MODES' number
    "casync_sync_packed_count": (C.c_int, [C.c_int]),
    "casync_sync_packed_name": (C.c_char_p, [C.c_int, C.c_int]),
    "casync_sync_packed_offset": (c_i64, [C.c_int, C.c_int]),
    "casync_sync_packed_size": (c_i64, [C.c_int, C.c_int]),
    "casync_sync_packed_total": (c_i64, [C.c_int]),
    "casync_sync_workspace_bytes": (c_i64, [C.c_int, C.c_int]),
    "casync_sync_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "casync_sync_destroy": (None, [C.c_void_p]),
    "casync_sync_load_weights_host": (C.c_int, [C.c_void_p, C.c_void_p, c_i64]),
    "casync_sync_load_weights_device": (C.c_int, [C.c_void_p, c_f32p, c_i64]),
    "casync_sync_forward": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, c_f32p, c_f32p, C.c_void_p, c_i64, C.c_void_p]),
    "casync_sync_forward_tap": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, C.c_int, c_f32p, C.c_void_p, c_i64, C.c_void_p]),
    "casync_op_sync_stem7": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_sync_conv5": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_sync_conv3": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.c_void_p]),
    "casync_op_sync_relu": (C.c_int, [c_f32p, c_i64, C.c_void_p]),
    "casync_op_sync_to_nchw": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_sync_embed": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_void_p]),
    "casync_op_sync_curve": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, c_f32p, C.c_void_p]),
    # its bf16 precision (additive to ABI 13); precision is SYNC_PRECISIONS' number, pointers typed c_void_p are bf16
    "casync_syncnet_create_ex": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "casync_syncnet_precision": (C.c_int, [C.c_void_p]),
    "casync_syncnet_workspace_bytes_ex": (c_i64, [C.c_int, C.c_int, C.c_int]),
    "casync_op_sync16_stem7": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_sync16_conv5": (C.c_int, [C.c_void_p, C.c_void_p, c_f32p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_sync16_conv3": (C.c_int, [C.c_void_p, C.c_void_p, c_f32p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_sync16_conv1": (C.c_int, [C.c_void_p, C.c_void_p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_sync16_to_nchw": (C.c_int, [C.c_void_p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    # the audio front end, WAV bytes -> the normalised 16 kHz waveform (additive to ABI 13); audio_out_samples is host only, mono is
    # calipsync_amd/audio.py MONO's number, the workspace holds float64 {mean, variance} at its head once audio_normalize has run
    "casync_audio_out_samples": (c_i64, [c_i64, C.c_int]),
    "casync_op_audio_workspace_bytes": (c_i64, [c_i64]),
    "casync_op_audio_resample": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_i64, C.c_int, C.c_int, C.c_int, c_f32p, c_i64, c_f32p, c_i64,
                                           C.c_void_p]),
    "casync_op_audio_normalize": (C.c_int, [c_f32p, c_i64, C.c_void_p, c_f32p, C.c_void_p]),
}

# include/casync_train.h (additive to ABI 13, a header of its own); rec is HOST memory: [batch][12] int32 = {t, y0, x0, h, w, r, ry0,
# rx0, rh, rw, 0, 0}
_PROTOS_TRAIN = {
    "casync_op_train_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, c_f32p, c_f32p, C.c_void_p]),
}

# include/casync_ploss.h (additive to ABI 13, a header of its own): the trainer's loss, L1 + VGG19 perceptual, with its gradient.
# partials are float64 on the device; grad_out_dev is a device scalar
_PROTOS_PLOSS = {
    "casync_ploss_packed_count": (C.c_int, []),
    "casync_ploss_packed_name": (C.c_char_p, [C.c_int]),
    "casync_ploss_packed_offset": (c_i64, [C.c_int]),
    "casync_ploss_packed_size": (c_i64, [C.c_int]),
    "casync_ploss_packed_total": (c_i64, []),
    "casync_ploss_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "casync_ploss_destroy": (None, [C.c_void_p]),
    "casync_ploss_load_weights_host": (C.c_int, [C.c_void_p, C.c_void_p, c_i64]),
    "casync_ploss_load_weights_device": (C.c_int, [C.c_void_p, c_f32p, c_i64]),
    "casync_ploss_saved_bytes": (c_i64, [C.c_int, C.c_int, C.c_int]),
    "casync_ploss_scratch_bytes": (c_i64, [C.c_int, C.c_int, C.c_int]),
    "casync_ploss_forward": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, c_f32p, C.c_void_p, c_i64,
                                       C.c_void_p, c_i64, C.c_void_p]),
    "casync_ploss_backward": (C.c_int, [C.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p,
                                        c_i64, C.c_void_p, c_i64, C.c_void_p]),
    "casync_ploss_tap_floats": (c_i64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "casync_ploss_forward_tap": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, C.c_void_p, c_i64, C.c_void_p]),
    "casync_ploss_backward_tap": (C.c_int, [C.c_void_p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, c_i64,
                                            C.c_int, c_f32p, C.c_void_p, c_i64, C.c_void_p]),
    "casync_op_ploss_stem": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_ploss_pool": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_ploss_weight_transform": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_ploss_split": (C.c_int, [c_f32p, c_f32p, c_i64, C.c_int, C.c_void_p]),
    "casync_op_ploss_combine": (C.c_int, [c_f32p, C.c_int, c_f32p, c_f32p, c_i64, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_ploss_relu_bwd": (C.c_int, [c_f32p, c_f32p, c_i64, C.c_void_p]),
    "casync_op_ploss_pool_bwd": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "casync_op_ploss_stem_bwd": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                           C.c_void_p]),
    "casync_ploss_partials": (C.c_int, [c_i64]),
    "casync_op_ploss_sqdiff": (C.c_int, [c_f32p, c_f32p, c_f32p, c_i64, C.c_void_p, C.c_void_p]),
    "casync_op_ploss_absdiff": (C.c_int, [c_f32p, c_f32p, c_i64, C.c_void_p, C.c_void_p]),
    "casync_op_ploss_finish": (C.c_int, [C.c_void_p, C.c_int, c_i64, C.c_void_p, C.c_int, c_i64, C.c_float, C.c_float, c_f32p, C.c_void_p]),
}

EXPORTS = tuple(_PROTOS)                 # what include/casync_hip.h declares
EXPORTS_TRAIN = tuple(_PROTOS_TRAIN)     # what include/casync_train.h declares
EXPORTS_PLOSS = tuple(_PROTOS_PLOSS)     # what include/casync_ploss.h declares
ABI_VERSION = 13         # == CASYNC_ABI_VERSION of include/casync_hip.h this file was written against


def lib_path() -> str:
    """The in-tree library; CASYNC_LIB names another build of the same ABI (A/B runs of two kernel versions in one
    GPU session: tools/experiments).  An override is never rebuilt."""
    return os.environ.get("CASYNC_LIB") or _build.LIB_PATH


def load() -> C.CDLL:
    """Load the engine library or raise -- there is no CPU / eager fallback."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own libamdhip64: it must be in the process before this library resolves its
    # HIP dependency, or two HIP runtimes get loaded and the second one sees no device
    # ("create: no HIP device visible" when the engine was loaded before `import torch`).
    import torch  # noqa: F401
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"casync HIP engine not built: {path} is missing. Run `python -c 'import "
            "__graft_entry__ as g; g.build()'` (needs hipcc). There is no CPU fallback.")
    if path == _build.LIB_PATH and _build.is_stale():
        # a library older than its sources can carry an old struct stride / prototype: rebuild where a
        # compiler exists (the build container, the GPU box), refuse it otherwise
        try:
            _build.build()
        except Exception as exc:
            raise RuntimeError(f"{path} is older than calipsync_amd/csrc and could not be rebuilt: {exc}") from exc
    lib = C.CDLL(path)
    for name, (res, args) in {**_PROTOS, **_PROTOS_TRAIN, **_PROTOS_PLOSS}.items():
        fn = getattr(lib, name)       # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    got = lib.casync_abi_version()
    if got != ABI_VERSION:
        raise RuntimeError(f"{path} has ABI version {got}, this binding needs {ABI_VERSION}: rebuild it "
                           "(python -c 'import __graft_entry__ as g; g.build()')")
    _lib = lib
    return lib


def set_option(name: str, value: int, handle=None) -> None:
    """Set an engine switch by name (include/casync_hip.h, casync_set_option): on `handle`, or on the
    process defaults (single-operator calls and engines created later) when handle is None."""
    check(load().casync_set_option(handle, name.encode(), int(value)), f"casync_set_option({name})")


def get_option(name: str, handle=None) -> int:
    v = C.c_int()
    check(load().casync_get_option(handle, name.encode(), C.byref(v)), f"casync_get_option({name})")
    return v.value


def check(status: int, what: str) -> int:
    if status < 0:
        msg = load().casync_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (status {status}): {msg}")
    return status


# audio encoders (include/casync_hip.h CASYNC_AUDIO_*): the reference Model's `mode`
AUDIO_MODES = {"hubert": 0, "wenet": 1}


def _layout(prefix: str, *args, suffix: str = ""):
    """[(name, offset, size)] in floats, and the total, of the packed buffer that
    casync_<prefix>packed_{count,name,offset,size,total}<suffix>(*args, ...) describe."""
    lib = load()
    count, name, offset, size, total = (getattr(lib, f"casync_{prefix}packed_{f}{suffix}")
                                        for f in ("count", "name", "offset", "size", "total"))
    return [(name(*args, i).decode(), offset(*args, i), size(*args, i)) for i in range(count(*args))], total(*args)


def packed_layout(mode: str = "hubert"):
    """The layout of one audio mode of the U-Net -- the engine owns the layout."""
    return _layout("", AUDIO_MODES[mode], suffix="_m")


def hubert_layout(layers: int):
    """The layout of the HuBERT engine's packed buffer for `layers` layers."""
    if load().casync_hubert_packed_count(layers) <= 0:
        raise ValueError(f"HuBERT engine: no packed layout for {layers} layers")
    return _layout("hubert_", layers)


def pfld_layout():
    """The layout of the PFLD landmark engine's packed buffer."""
    return _layout("pfld_")


def s3fd_layout():
    """The layout of the S3FD face-detector engine's packed buffer."""
    return _layout("s3fd_")


def ploss_layout():
    """The layout of the loss handle's packed buffer (include/casync_ploss.h)."""
    return _layout("ploss_")


def sync_layout(mode: str = "hubert"):
    """The layout of the SyncNet_color engine's packed buffer for one audio mode."""
    return _layout("sync_", AUDIO_MODES[mode])


def pack_named(named: dict, layout) -> np.ndarray:
    """{name: array} -> the flat float32 buffer of `layout` (items, total).  `named` is emptied; ValueError for a tensor of
    another size than the layout's and for names the layout does not hold."""
    items, total = layout
    buf = np.zeros(total, dtype=np.float32)
    for name, off, size in items:
        a = named.pop(name).reshape(-1)
        if a.size != size:
            raise ValueError(f"packed tensor {name}: {a.size} floats, the engine expects {size}")
        buf[off:off + size] = a
    if named:
        raise ValueError(f"tensors the engine layout does not name: {sorted(named)}")
    return buf


def unpack_named(buf: np.ndarray, layout) -> dict:
    """Inverse of pack_named (flat shapes, views of buf)."""
    return {name: buf[off:off + size] for name, off, size in layout[0]}
