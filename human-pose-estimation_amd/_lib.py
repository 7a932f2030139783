"""ctypes binding of libhpe_hip.so (include/hpe.h).  No torch types cross this boundary: only raw
device/host pointers, sizes and a hipStream_t.  The library must exist (``hpe_amd.build.build()``);
there is no CPU fallback -- a missing library or a non-gfx950 device raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libhpe_hip.so")

NUM_CONV = 53
NUM_DENSE = 3
NUM_CRITIC_DENSE = 9
NUM_VERTS = 6890
THETA_DIM = 85
FEATURE_DIM = 2048


class HpeError(RuntimeError):
    pass


class HpeConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int),  # sizeof(HpeConfig); hpe_config_init writes it, hpe_create checks it
        ("device", C.c_int),
        ("max_batch", C.c_int),
        ("num_stage", C.c_int),
        ("bn_eps", C.c_float),
        ("encoder_dtype", C.c_int),
        # plan options (-1 = default: environment variable, else built-in); see include/hpe.h
        ("n_streams", C.c_int),
        ("dual_gemm", C.c_int),
        ("stem_fused", C.c_int),
        ("wino_min_c", C.c_int),
        ("wino_min_items", C.c_int),
        ("wino_fused", C.c_int),
        ("wino_fused_min_hw", C.c_int),
        ("mesh_a2b", C.c_int),
        ("wino_f4", C.c_int),
        ("wino4_fused", C.c_int),
        ("bf16_p8", C.c_int),
        ("wino4_ksplit", C.c_int),
        ("chain_fuse", C.c_int),
        ("halo3", C.c_int),
        ("f32_split", C.c_int),
    ]


PLAN_OPTIONS = ("n_streams", "dual_gemm", "stem_fused", "wino_min_c", "wino_min_items", "wino_fused", "wino_fused_min_hw", "mesh_a2b", "wino_f4", "wino4_fused", "bf16_p8", "wino4_ksplit", "chain_fuse", "halo3", "f32_split")


class HpeSmplModel(C.Structure):
    _fields_ = [
        ("v_template", C.c_void_p),
        ("shapedirs", C.c_void_p),
        ("posedirs", C.c_void_p),
        ("J_regressor", C.c_void_p),
        ("weights", C.c_void_p),
        ("kp_regressor", C.c_void_p),
        ("parents", C.c_void_p),
        ("num_kp", C.c_int),
    ]


class HpeCriticModel(C.Structure):
    _fields_ = [("kernel", C.c_void_p * NUM_CRITIC_DENSE), ("bias", C.c_void_p * NUM_CRITIC_DENSE)]


class HpeRenderParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int),  # sizeof(HpeRenderParams); hpe_render_params_init writes it, every render call checks it
        ("color_id", C.c_int),
        ("do_alpha", C.c_int),
        ("rot_axis", C.c_int),
        ("rot_deg", C.c_float),
        ("near", C.c_float),
        ("far", C.c_float),
    ]


class HpeAugmentFrame(C.Structure):
    """one table entry of hpe_augment_plan / hpe_augment_batch (include/hpe.h), 64 bytes"""
    _fields_ = [("frame_offset", C.c_longlong), ("seg_offset", C.c_longlong), ("H", C.c_int), ("W", C.c_int), ("newH", C.c_int),
                ("newW", C.c_int), ("cx", C.c_int), ("cy", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("flip", C.c_int),
                ("inside", C.c_int), ("rx", C.c_float), ("ry", C.c_float)]


class HpeJpegInfo(C.Structure):
    """what hpe_jpeg_info fills per stream (include/hpe.h), 72 bytes"""
    _fields_ = [("status", C.c_int), ("H", C.c_int), ("W", C.c_int), ("ncomp", C.c_int), ("hs", C.c_int * 3), ("vs", C.c_int * 3),
                ("blocks_w", C.c_int * 3), ("blocks_h", C.c_int * 3), ("coefs", C.c_longlong)]


class HpeJpegImage(C.Structure):
    """one table entry of hpe_jpeg_decode / hpe_jpeg_backend (include/hpe.h), 304 bytes"""
    _fields_ = [("coef_offset", C.c_longlong * 3), ("plane_offset", C.c_longlong * 3), ("out_offset", C.c_longlong), ("H", C.c_int),
                ("W", C.c_int), ("ncomp", C.c_int), ("channels", C.c_int), ("hmax", C.c_int), ("vmax", C.c_int), ("blocks_w", C.c_int * 3),
                ("blocks_h", C.c_int * 3), ("idct_group0", C.c_int), ("store_group0", C.c_int), ("quant", (C.c_ubyte * 64) * 3)]


class HpeJpegEncImage(C.Structure):
    """one table entry of hpe_jpeg_encode_layout / hpe_jpeg_forward / hpe_jpeg_entropy_encode (include/hpe.h), 232 bytes"""
    _fields_ = [("frame_offset", C.c_longlong), ("coef_offset", C.c_longlong * 3), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int),
                ("hmax", C.c_int), ("vmax", C.c_int), ("blocks_w", C.c_int * 3), ("blocks_h", C.c_int * 3), ("real_w", C.c_int * 3),
                ("real_h", C.c_int * 3), ("group0", C.c_int), ("quant", (C.c_ubyte * 64) * 2)]


class HpePngImage(C.Structure):
    """one table entry of hpe_png_backend (include/hpe.h), 64 bytes"""
    _fields_ = [("raw_offset", C.c_longlong), ("pal_offset", C.c_longlong), ("work_offset", C.c_longlong), ("out_offset", C.c_longlong),
                ("H", C.c_int), ("W", C.c_int), ("color_type", C.c_int), ("depth", C.c_int), ("channels", C.c_int), ("rowbytes", C.c_int),
                ("bpp", C.c_int), ("store_group0", C.c_int)]


class HpePngFilterImage(C.Structure):
    """one table entry of hpe_png_filter (include/hpe.h), 32 bytes"""
    _fields_ = [("frame_offset", C.c_longlong), ("scan_offset", C.c_longlong), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("row0", C.c_int)]


def record_dtype(struct):
    """the numpy record dtype of a table entry's ctypes structure: its names, offsets and itemsize; a nested array such as
    (c_ubyte * 64) * 3 becomes ONE sub-array field of shape (3, 64), where numpy alone nests a (64,) sub-array in a (3,) one"""
    d = np.dtype(struct)
    formats = []
    for name in d.names:
        t, shape = d.fields[name][0], ()
        while t.subdtype:
            t, shape = t.subdtype[0], shape + t.subdtype[1]
        formats.append((t, shape))
    return np.dtype({"names": list(d.names), "formats": formats, "offsets": [d.fields[n][1] for n in d.names], "itemsize": d.itemsize})


GEMM_DENSE, GEMM_STRIDED, GEMM_CONV3, GEMM_DUAL = 0, 1, 2, 4  # HpeDebugGemm.mode
GEMM_TILES = ((128, 128), (128, 64), (64, 64), (64, 128), (128, 128), (128, 64), (256, 128))  # (BM, BN) of tile 0..6; 4..6 run 8 waves


class HpeDebugGemm(C.Structure):
    """arguments of hpe_debug_gemm_ex (include/hpe.h)"""
    _fields_ = [("struct_size", C.c_int), ("mode", C.c_int), ("tile", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
                ("lda", C.c_int), ("ldw", C.c_int), ("ldy", C.c_int), ("ldres", C.c_int), ("w_rows", C.c_int), ("relu", C.c_int),
                ("Hi", C.c_int), ("Wi", C.c_int), ("Cin", C.c_int), ("Ho", C.c_int), ("Wo", C.c_int), ("stride", C.c_int),
                ("k1_slabs", C.c_int), ("y_slab8", C.c_int), ("use_splitk", C.c_int), ("reserved", C.c_int),
                ("x", C.c_void_p), ("x2", C.c_void_p), ("wt", C.c_void_p), ("residual", C.c_void_p), ("scale", C.c_void_p),
                ("shift", C.c_void_p), ("y", C.c_void_p), ("split_k", C.POINTER(C.c_int))]


# HpeConvRoute.kernel (include/hpe.h: HPE_CONV_K_*) and .join
CONV_KERNELS = ("f32", "f32s", "bf16", "bf16_p8", "halo3", "wino", "wino_fused", "wino4", "wino4_fused")
BLOCK_JOINS = ("separate", "dual", "chain")


class HpeConvRoute(C.Structure):
    """what hpe_debug_conv_route fills (include/hpe.h)"""
    _fields_ = [("struct_size", C.c_int), ("kernel", C.c_int), ("mode", C.c_int), ("tile", C.c_int), ("in_slab8", C.c_int), ("out_slab8", C.c_int),
                ("join", C.c_int), ("join_kernel", C.c_int), ("join_tile", C.c_int), ("next_slab8", C.c_int), ("packs", C.c_uint), ("reserved", C.c_int)]


def conv_route(lib, cfg, idx, B, concurrent=False, residual=False, workspace=True):
    """hpe_debug_conv_route on an HpeConfig: no context, no GPU"""
    r = HpeConvRoute(struct_size=C.sizeof(HpeConvRoute))
    check(lib.hpe_debug_conv_route(C.byref(cfg), int(idx), int(B), int(concurrent), int(residual), int(workspace), C.byref(r)))
    return r


# `which` of hpe_debug_encoder_packing (include/hpe.h: HPE_PACK_*)
ENCODER_PACKINGS = ("w", "w_split", "wino_u", "wino4_u", "stem_w", "scale", "shift", "w_dual", "w_dual_split", "shift_dual", "dxw", "flat")

OUTPUT_FIELDS = ("verts", "joints", "cams", "theta", "J_transformed", "kp2d", "verts2d", "Rs")


class HpeOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in OUTPUT_FIELDS]


# hpe_reduce_fn (include/hpe.h): (user, dev_buf, count, stream) -> 0, or nonzero for a failure.  ctypes takes the GIL for the callback
REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p)

_PROTOS = {
    "hpe_last_error": (C.c_char_p, []),
    "hpe_version": (C.c_char_p, []),
    "hpe_conv_layer_name": (C.c_char_p, [C.c_int]),
    "hpe_bn_layer_name": (C.c_char_p, [C.c_int]),
    "hpe_conv_layer_geometry": (C.c_int, [C.c_int, C.POINTER(C.c_int)]),
    "hpe_config_init": (None, [C.POINTER(HpeConfig)]),
    "hpe_create": (C.c_int, [C.POINTER(HpeConfig), C.POINTER(C.c_void_p)]),
    "hpe_destroy": (C.c_int, [C.c_void_p]),
    "hpe_load_smpl": (C.c_int, [C.c_void_p, C.POINTER(HpeSmplModel)]),
    "hpe_load_conv": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 6),
    "hpe_load_dense": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_load_mean_theta": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hpe_finalize": (C.c_int, [C.c_void_p]),
    "hpe_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(HpeOutputs), C.c_int, C.c_void_p]),
    "hpe_forward_pipelined": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(HpeOutputs), C.c_int, C.c_void_p]),
    "hpe_join": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hpe_tail": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(HpeOutputs), C.c_int, C.c_void_p]),
    "hpe_tail_stream": (C.c_void_p, [C.c_void_p]),
    "hpe_encoder": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_regress_stage": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_smpl": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(HpeOutputs), C.c_void_p]),
    "hpe_smpl_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(HpeOutputs), C.c_void_p, C.c_void_p]),
    "hpe_orth_proj": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_reproject_vertices": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "hpe_preprocess_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]),
    "hpe_preprocess_u8_batch": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int),
                                          C.c_void_p, C.c_void_p]),
    "hpe_augment_plan": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_augment_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_adam_advance": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p]),
    "hpe_adam_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "hpe_adam_set_step": (C.c_int, [C.c_void_p, C.c_longlong, C.c_double, C.c_double, C.c_void_p]),
    "hpe_debug_adam_power": (C.c_int, [C.c_double, C.c_longlong, C.POINTER(C.c_double)]),
    "hpe_grad_stats_chunk": (C.c_int, []),
    "hpe_grad_stats_workspace_bytes": (C.c_longlong, [C.c_longlong, C.c_int]),
    "hpe_grad_stats": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "hpe_adam_guard": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int,
                                 C.c_void_p]),
    "hpe_adam_apply_guarded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                         C.c_float, C.c_void_p]),
    "hpe_jpeg_info": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_jpeg_decode": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_jpeg_backend": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong,
                                   C.c_void_p]),
    "hpe_jpeg_encode_layout": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_jpeg_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p]),
    "hpe_jpeg_entropy_encode": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_longlong,
                                          C.c_void_p, C.c_void_p]),
    "hpe_png_backend": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong,
                                  C.c_void_p]),
    "hpe_png_filter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p]),
    "hpe_draw_panels": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_draw_skeleton": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "hpe_get_original": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_float, C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_kp_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_kp_loss_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_mesh_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_mesh_loss_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "hpe_val_losses": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int,
                                 C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_eval_scores": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int,
                                  C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_pose3d_scores": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_debug_procrustes3": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "hpe_critic_layer_name": (C.c_char_p, [C.c_int]),
    "hpe_critic_layer_shape": (C.c_int, [C.c_int, C.POINTER(C.c_int)]),
    "hpe_load_critic": (C.c_int, [C.c_void_p, C.POINTER(HpeCriticModel)]),
    "hpe_critic": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_critic_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_critic_param_floats": (C.c_int, []),
    "hpe_critic_param_offset": (C.c_int, [C.c_int, C.c_int]),
    "hpe_critic_weight_grad_ws_floats": (C.c_longlong, [C.c_int]),
    "hpe_critic_reserve": (C.c_int, [C.c_void_p, C.c_int]),
    "hpe_critic_weight_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_critic_get_params": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_critic_set_params_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_regressor_param_floats": (C.c_int, []),
    "hpe_regressor_param_offset": (C.c_int, [C.c_int, C.c_int]),
    "hpe_regressor_get_params": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_regressor_set_params_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_regressor_forward_train": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_regressor_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_encoder_param_floats": (C.c_int, []),
    "hpe_encoder_param_offset": (C.c_int, [C.c_int, C.c_int]),
    "hpe_encoder_train_reserve": (C.c_int, [C.c_void_p, C.c_int]),
    "hpe_encoder_train_ws_floats": (C.c_longlong, [C.c_int]),
    "hpe_encoder_wg_slices": (C.c_int, [C.c_int, C.c_int]),
    "hpe_encoder_forward_train": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_encoder_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_encoder_get_params": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_encoder_set_params": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hpe_encoder_set_params_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_debug_encoder_packing_bytes": (C.c_longlong, [C.c_void_p, C.c_int, C.c_int]),
    "hpe_debug_encoder_packing": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_debug_conv_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_debug_maxpool_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_debug_avgpool_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_debug_encoder_stash": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_debug_encoder_stash_batch": (C.c_int, [C.c_void_p]),
    "hpe_encoder_stat_floats": (C.c_int, []),
    "hpe_encoder_stat_offset": (C.c_int, [C.c_int, C.c_int]),
    "hpe_encoder_train_reserve_batchnorm": (C.c_int, [C.c_void_p, C.c_int]),
    "hpe_encoder_train_ws_floats_batchnorm": (C.c_longlong, [C.c_int]),
    "hpe_debug_encoder_bn_slices": (C.c_int, [C.c_int, C.c_int]),
    "hpe_encoder_forward_batchnorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_encoder_backward_batchnorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_encoder_get_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_encoder_update_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p]),
    "hpe_encoder_set_stats_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_debug_conv_batchnorm": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_debug_conv_backward_batchnorm": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                    C.c_void_p]),
    "hpe_debug_encoder_stash_raw": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_debug_encoder_batch_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_encoder_set_reduce": (C.c_int, [C.c_void_p, REDUCE_FN, C.c_void_p, C.c_int]),
    "hpe_debug_bn_sums": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_debug_bn_finish": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "hpe_debug_bn_backward_sums": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p,
                                             C.c_void_p]),
    "hpe_debug_bn_backward_finish": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_device_status": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hpe_debug_conv": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_debug_chain": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]),
    "hpe_debug_stem": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_debug_gemm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_debug_gemm_ex": (C.c_int, [C.c_void_p, C.POINTER(HpeDebugGemm), C.c_void_p]),
    "hpe_debug_gemm_check": (C.c_int, [C.POINTER(HpeDebugGemm), C.c_int, C.c_int]),
    "hpe_debug_gemm_launch": (C.c_int, [C.c_void_p, C.POINTER(HpeDebugGemm), C.c_int, C.c_int, C.c_void_p]),
    "hpe_debug_conv_route": (C.c_int, [C.POINTER(HpeConfig), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(HpeConvRoute)]),
    "hpe_debug_conv_stream1x1": (C.c_int, [C.POINTER(HpeConfig), C.c_int, C.c_int, C.c_int, C.c_int]),
    "hpe_debug_dual": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_debug_stream_chain": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "hpe_debug_maxpool": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_debug_avgpool": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_debug_joint_regress": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hpe_enable_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "hpe_get_timings": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "hpe_get_span_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "hpe_get_loss_timings": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "hpe_debug_set_loss_counter": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hpe_get_conv_timings": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "hpe_render_params_init": (None, [C.POINTER(HpeRenderParams)]),
    "hpe_renderer_create": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "hpe_renderer_destroy": (C.c_int, [C.c_void_p]),
    "hpe_render": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(HpeRenderParams), C.c_void_p,
                             C.c_void_p]),
    "hpe_debug_render_ids": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(HpeRenderParams), C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "hpe_debug_render_vertices": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(HpeRenderParams),
                                            C.c_void_p, C.c_void_p]),
}

# The entry points of encoder training by role: (with frozen BatchNorm statistics, with batch statistics); None: no such call in
# that mode.  Each exists in fp32 under this name and for the mixed-precision walks under this name + "_mixed", with the same argument
# list (bf16 buffers cross the ABI as void*), so the *_mixed prototypes are derived here, not listed.
ENCODER_ENTRY = {
    "reserve": ("hpe_encoder_train_reserve", "hpe_encoder_train_reserve_batchnorm"),
    "ws_floats": ("hpe_encoder_train_ws_floats", "hpe_encoder_train_ws_floats_batchnorm"),
    "forward": ("hpe_encoder_forward_train", "hpe_encoder_forward_batchnorm"),
    "backward": ("hpe_encoder_backward", "hpe_encoder_backward_batchnorm"),
    "stash": ("hpe_debug_encoder_stash", "hpe_debug_encoder_stash"),
    "stash_batch": ("hpe_debug_encoder_stash_batch", "hpe_debug_encoder_stash_batch"),
    "stash_raw": (None, "hpe_debug_encoder_stash_raw"),
    "conv_batchnorm": (None, "hpe_debug_conv_batchnorm"),
    "conv_backward": ("hpe_debug_conv_backward", "hpe_debug_conv_backward_batchnorm"),
    "maxpool_backward": ("hpe_debug_maxpool_backward", "hpe_debug_maxpool_backward"),
    "avgpool_backward": ("hpe_debug_avgpool_backward", "hpe_debug_avgpool_backward"),
}
_PROTOS.update({name + "_mixed": _PROTOS[name] for pair in ENCODER_ENTRY.values() for name in pair if name})

# The 3-D supervision extension (include/hpe_loss3d.h, which include/hpe.h includes): a table of its own, bound by load() like the core
# table; ``declared_symbols`` stays the core list of include/hpe.h, ``loss3d_symbols`` is this header's.
_PROTOS_LOSS3D = {
    "hpe_loss3d": (C.c_int, [C.POINTER(C.c_void_p)] * 3 + [C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpe_loss3d_backward": (C.c_int, [C.POINTER(C.c_void_p)] * 3 + [C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p] +
                            [C.POINTER(C.c_void_p)] * 3 + [C.c_void_p]),
}


def encoder_symbol(role, batch, suffix=""):
    """the C symbol of ENCODER_ENTRY[role] with (batch) or without batch statistics; suffix "_mixed": its mixed-precision twin"""
    name = ENCODER_ENTRY[role][bool(batch)]
    if name is None:
        raise ValueError("%s exists with batch statistics only" % role)
    return name + suffix


_lib = None


def load():
    """dlopen the in-tree library and bind every symbol of include/hpe.h and include/hpe_loss3d.h.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HpeError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % LIB_PATH
        )
    # The HIP runtime must be the one torch already mapped (same SONAME libamdhip64.so.7), so that torch
    # device pointers / streams are valid in our launches: import torch first if it is going to be used.
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - the library itself does not need torch
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in list(_PROTOS.items()) + list(_PROTOS_LOSS3D.items()):
        fn = getattr(lib, name)  # AttributeError here == header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def declared_symbols():
    return sorted(_PROTOS)


def loss3d_symbols():
    """the entry points of include/hpe_loss3d.h"""
    return sorted(_PROTOS_LOSS3D)


def check(rc):
    if rc != 0:
        msg = load().hpe_last_error()
        raise HpeError("libhpe_hip error %d: %s" % (rc, msg.decode() if msg else "?"))


def f32(a):
    """contiguous float32 host array + its pointer (keeps the array alive via the return value)"""
    arr = np.ascontiguousarray(a, dtype=np.float32)
    return arr, arr.ctypes.data_as(C.c_void_p)
