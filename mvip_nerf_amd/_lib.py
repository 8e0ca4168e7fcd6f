"""ctypes binding of libmvipnerf.so (the C ABI declared in include/mvip_nerf.h).

The product path has no CPU fallback: if the library is missing or a call fails, this raises.
PyTorch is used above this layer only for device memory, streams and autograd plumbing.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# MVIP_LIB_PATH: another build of the same library (tools/: the -DMVIP_EXPERIMENT_* timing builds live in lib_experiment/)
LIB_PATH = os.environ.get('MVIP_LIB_PATH') or os.path.join(_HERE, 'lib', 'libmvipnerf.so')

_c_f = ctypes.c_void_p      # device pointers travel as integers
_i64 = ctypes.c_int64
_int = ctypes.c_int
_flt = ctypes.c_float

_SIGNATURES = {
    'mvip_abi_version': (_int, []),
    'mvip_build_is_experiment': (_int, []),
    'mvip_strerror': (ctypes.c_char_p, [_int]),
    'mvip_last_hip_error': (ctypes.c_char_p, []),
    'mvip_device_info': (_int, [ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.c_char_p, _int]),
    'mvip_get_rays': (_int, [_c_f, _int, _int, _flt, _int, _int, _int, _int, _c_f, _c_f, _c_f]),
    'mvip_ray_rows': (_int, [_c_f, _c_f, _c_f, _flt, _flt, _i64, _c_f, _c_f]),
    'mvip_ray_rows_from_pose': (_int, [_c_f, _int, _int, _flt, _flt, _flt, _c_f, _i64, _c_f, _c_f]),
    'mvip_stratified_z': (_int, [_c_f, _int, _i64, _int, _c_f, _int, _c_f, _c_f, _c_f]),
    'mvip_posenc': (_int, [_c_f, _i64, _int, _c_f, _c_f]),
    'mvip_mlp_packed_floats': (_i64, []),
    'mvip_mlp_pack': (_int, [ctypes.POINTER(ctypes.c_void_p), _c_f, _c_f]),
    'mvip_mlp_pack_f16x3': (_int, [ctypes.POINTER(ctypes.c_void_p), _c_f, _c_f, _c_f]),
    'mvip_mlp_forward_rays_f16x3': (_int, [_c_f, _c_f, _c_f, _i64, _int, _c_f, _c_f]),
    'mvip_mlp_forward_points_f16x3': (_int, [_c_f, _c_f, _c_f, _i64, _c_f, _c_f]),
    'mvip_mlp_pack_f16x3_w16': (_int, [ctypes.POINTER(ctypes.c_void_p), _c_f, _c_f, _c_f]),
    'mvip_mlp_forward_rays_f16x3_w16': (_int, [_c_f, _c_f, _c_f, _i64, _int, _c_f, _c_f]),
    'mvip_mlp_forward_points_f16x3_w16': (_int, [_c_f, _c_f, _c_f, _i64, _c_f, _c_f]),
    'mvip_mlp_forward_rays_stash_f16x3_w16': (_int, [_c_f, _c_f, _c_f, _i64, _int, _c_f, _c_f, _c_f]),
    'mvip_mlp_forward_rays': (_int, [_c_f, _c_f, _c_f, _i64, _int, _c_f, _int, _c_f]),
    'mvip_mlp_forward_points': (_int, [_c_f, _c_f, _c_f, _i64, _c_f, _int, _c_f]),
    'mvip_mlp_pack16': (_int, [ctypes.POINTER(ctypes.c_void_p), _c_f, _c_f, _c_f]),
    'mvip_mlp_forward_rays16': (_int, [_c_f, _c_f, _c_f, _i64, _int, _c_f, _c_f]),
    'mvip_mlp_forward_rays_stash16': (_int, [_c_f, _c_f, _c_f, _i64, _int, _c_f, _c_f, _c_f]),
    'mvip_mlp_forward_points16': (_int, [_c_f, _c_f, _c_f, _i64, _c_f, _c_f]),
    'mvip_mlp_encode16_probe': (_int, [_c_f, _c_f, _i64, _c_f, _c_f, _c_f]),
    'mvip_render_coarse_fused': (_int, [_c_f, _c_f, _i64, _c_f, _int, _c_f, _c_f, _c_f, _int, _int, _int, _c_f, _c_f, _c_f, _c_f,
                                        _c_f, _c_f, _c_f, _c_f, _c_f]),
    'mvip_render_fine_fused': (_int, [_c_f, _c_f, _c_f, _i64, _c_f, _int, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'mvip_mlp_packed_fold_floats': (_i64, []),
    'mvip_mlp_fold_pack16': (_int, [ctypes.POINTER(ctypes.c_void_p), _c_f, _c_f]),
    'mvip_mlp_forward_rays16_fold': (_int, [_c_f, _c_f, _c_f, _i64, _int, _c_f, _c_f]),
    'mvip_mlp_forward_points16_fold': (_int, [_c_f, _c_f, _c_f, _i64, _c_f, _c_f]),
    'mvip_render_coarse_fused_fold': (_int, [_c_f, _c_f, _i64, _c_f, _int, _c_f, _c_f, _c_f, _int, _int, _int, _c_f, _c_f, _c_f,
                                             _c_f, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'mvip_render_fine_fused_fold': (_int, [_c_f, _c_f, _c_f, _i64, _c_f, _int, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'mvip_mlp_backward_workspace_bytes': (_i64, [_i64]),
    'mvip_mlp_backward_rays': (_int, [_c_f, _c_f, _c_f, _i64, _int, _c_f, ctypes.POINTER(ctypes.c_void_p), _c_f, _i64,
                                      _int, _c_f]),
    'mvip_mlp_backward_points': (_int, [_c_f, _c_f, _c_f, _i64, _c_f, ctypes.POINTER(ctypes.c_void_p), _c_f, _i64, _int,
                                        _c_f]),
    'mvip_mlp_stash_floats': (_i64, [_i64]),
    'mvip_mlp_forward_rays_stash': (_int, [_c_f, _c_f, _c_f, _i64, _int, _c_f, _c_f, _int, _c_f]),
    'mvip_mlp_forward_points_stash': (_int, [_c_f, _c_f, _c_f, _i64, _c_f, _c_f, _int, _c_f]),
    'mvip_mlp_backward_stash': (_int, [_c_f, _c_f, _i64, _c_f, ctypes.POINTER(ctypes.c_void_p), _c_f, _i64, _int, _c_f]),
    'mvip_mlp_unpack_grads': (_int, [_c_f, ctypes.POINTER(ctypes.c_void_p), _int, _c_f]),
    'mvip_composite_forward': (_int, [_c_f, _c_f, _c_f, _int, _c_f, _i64, _int, _int, _c_f, _c_f, _c_f, _c_f,
                                      _c_f, _c_f, _c_f]),
    'mvip_composite_backward': (_int, [_c_f, _c_f, _c_f, _int, _c_f, _i64, _int, _int, _c_f, _c_f, _c_f, _c_f,
                                       _c_f, _c_f, _c_f, _c_f]),
    'mvip_sample_pdf_merge': (_int, [_c_f, _c_f, _c_f, _int, _i64, _int, _int, _c_f, _c_f, _c_f, _c_f, _c_f,
                                     _c_f]),
    'mvip_sample_pdf': (_int, [_c_f, _c_f, _c_f, _int, _i64, _int, _int, _c_f, _c_f, _c_f, _c_f]),
    'mvip_depth2xyz': (_int, [_c_f, _int, _int, _flt, _flt, _flt, _flt, _c_f, _c_f]),
    'mvip_depth2xyz_backward': (_int, [_c_f, _int, _int, _flt, _flt, _flt, _flt, _c_f, _c_f]),
    'mvip_normal_fit_forward': (_int, [_c_f, _int, _int, _int, _c_f, _c_f, _c_f, _c_f]),
    'mvip_normal_fit_backward': (_int, [_c_f, _c_f, _c_f, _c_f, _int, _int, _int, _c_f, _c_f, _c_f]),
    'mvip_sds_add_noise': (_int, [_c_f, _c_f, _flt, _flt, _i64, _c_f, _c_f]),
    'mvip_sds_grad': (_int, [_c_f, _c_f, _c_f, _flt, _flt, _i64, _int, _c_f, _c_f]),
    'mvip_sds_add_noise_dev': (_int, [_c_f, _c_f, _c_f, _i64, _c_f, _c_f]),
    'mvip_sds_grad_dev': (_int, [_c_f, _c_f, _c_f, _flt, _c_f, _i64, _int, _c_f, _c_f]),
    'mvip_vae_sample': (_int, [_c_f, _c_f, _flt, _i64, _i64, _i64, _c_f, _c_f]),
    'mvip_vae_sample_backward': (_int, [_c_f, _c_f, _c_f, _flt, _i64, _i64, _i64, _c_f, _c_f]),
    'mvip_timestep_sincos': (_int, [_c_f, _c_f, _i64, _i64, _c_f, _c_f]),
    'mvip_vae_decoder_head': (_int, [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _i64, _i64, _i64, _i64, _int, _int, _c_f, _c_f,
                                     _int, _c_f]),
    'mvip_ddim_cfg_step': (_int, [_c_f, _int, _c_f, _c_f, _i64, _c_f, _i64, _c_f, _c_f]),
    'mvip_resize_bilinear': (_int, [_c_f, _i64, _i64, _i64, _i64, _i64, _c_f, _c_f]),
    'mvip_resize_bilinear_backward': (_int, [_c_f, _i64, _i64, _i64, _i64, _i64, _c_f, _c_f]),
    'mvip_groupnorm_workspace_bytes': (_i64, [_i64, _i64, _i64]),
    'mvip_groupnorm_forward': (_int, [_c_f, _c_f, _c_f, _i64, _i64, _i64, _int, _flt, _int, _int, _c_f, _c_f, _c_f, _c_f,
                                      _c_f]),
    'mvip_groupnorm_stats': (_int, [_c_f, _i64, _i64, _i64, _int, _flt, _int, _c_f, _c_f, _c_f, _c_f]),
    'mvip_conv3x3_supported': (_int, [_i64, _i64, _i64, _i64]),
    'mvip_conv3x3_packed_bytes': (_i64, [_i64, _i64]),
    'mvip_conv3x3_pack': (_int, [_c_f, _i64, _i64, _int, _c_f, _c_f]),
    'mvip_packed_weights_two_product': (_int, [_c_f, _i64, ctypes.POINTER(_int), _c_f]),
    'mvip_absmax_scale': (_int, [_c_f, _i64, _c_f, _c_f, _c_f]),
    'mvip_split_planes': (_int, [_c_f, _i64, _i64, _i64, _c_f, _c_f, _int, _c_f]),
    'mvip_groupnorm_split_planes': (_int, [_c_f, _c_f, _c_f, _c_f, _c_f, _i64, _i64, _i64, _int, _int, _c_f, _int, _c_f]),
    'mvip_conv3x3_f16x3': (_int, [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _i64, _i64, _i64, _i64, _i64, _c_f, _int, _c_f]),
    'mvip_conv3x3_workspace_bytes': (_i64, [_i64, _i64, _i64, _i64, _i64]),
    'mvip_conv3x3_f16x3_ws': (_int, [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _i64, _i64, _i64, _i64, _i64, _c_f, _c_f, _int, _c_f]),
    'mvip_hashgrid_forward': (_int, [_c_f, _c_f, _c_f, _i64, _flt, _c_f, _c_f]),
    'mvip_hashgrid_backward': (_int, [_c_f, _c_f, _c_f, _i64, _flt, _c_f, _c_f]),
    'mvip_sh4': (_int, [_c_f, _i64, _c_f, _c_f]),
    'mvip_hashgrid_backward_half2': (_int, [_c_f, _c_f, _c_f, _i64, _flt, _c_f, _c_f, _c_f, _c_f]),
    'mvip_hashgrid_mlp_packed_floats': (_i64, []),
    'mvip_hashgrid_mlp_pack': (_int, [_c_f, _c_f, _c_f, _c_f]),
    'mvip_hashgrid_nerf_forward': (_int, [_c_f, _c_f, _c_f, _c_f, _c_f, _i64, _flt, _c_f, _c_f]),
    'mvip_skinny_wgrad_slabs': (_i64, [_i64]),
    'mvip_skinny_wgrad': (_int, [_c_f, _c_f, _i64, _i64, _i64, _c_f, _c_f]),
    'mvip_skinny_linear': (_int, [_c_f, _i64, _i64, _c_f, _i64, _i64, _i64, _int, _c_f, _c_f]),
    'mvip_gemm_packed_bytes': (_i64, [_i64, _i64]),
    'mvip_gemm_pack_a': (_int, [_c_f, _i64, _i64, _i64, _i64, _c_f, _c_f]),
    'mvip_split_planes_strided': (_int, [_c_f, _i64, _i64, _i64, _i64, _i64, _i64, _c_f, _c_f, _int, _c_f]),
    'mvip_split_planes_upsample2': (_int, [_c_f, _i64, _i64, _i64, _i64, _c_f, _c_f, _int, _c_f]),
    'mvip_softmax_rows': (_int, [_c_f, _i64, _i64, _flt, _c_f, _c_f]),
    'mvip_softmax_rows_backward': (_int, [_c_f, _c_f, _i64, _i64, _flt, _c_f, _c_f]),
    'mvip_gemm_f16x3': (_int, [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _i64, _i64, _i64, _i64, _c_f, _int, _c_f]),
    'mvip_gemm_geglu_f16x3': (_int, [_c_f, _c_f, _c_f, _c_f, _i64, _i64, _i64, _i64, _i64, _c_f, _c_f, _c_f, _int, _c_f]),
    'mvip_im2col_split_planes': (_int, [_c_f, _i64, _i64, _i64, _i64, _int, _int, _int, _int, _int, _i64, _i64, _i64, _i64,
                                        _c_f, _c_f, _int, _c_f]),
    'mvip_col2im': (_int, [_c_f, _i64, _i64, _i64, _i64, _int, _int, _int, _int, _int, _i64, _i64, _i64, _i64, _c_f, _c_f]),
    'mvip_gemm_workspace_bytes': (_i64, [_i64, _i64, _i64, _i64]),
    'mvip_gemm_f16x3_ws': (_int, [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _i64, _i64, _i64, _i64, _c_f, _c_f, _int, _c_f]),
    'mvip_gemm_ln_segments': (_i64, [_i64, _i64, _i64, _i64, _int]),
    'mvip_gemm_f16x3_ws_ln': (_int, [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _i64, _i64, _i64, _i64, _c_f, _c_f, _c_f, _int, _c_f]),
    'mvip_layernorm_split_planes_stats': (_int, [_c_f, _c_f, _c_f, _c_f, _i64, _i64, _i64, _i64, _i64, _flt, _flt, _c_f, _int, _c_f]),
    'mvip_gemm_f16x3_cfg': (_int, [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _i64, _i64, _i64, _i64, _c_f, _int, _int, _c_f]),
    'mvip_attention_supported': (_int, [_i64]),
    'mvip_attention_v_bytes': (_i64, [_i64, _i64, _i64, _i64]),
    'mvip_attention_pack_v': (_int, [_c_f, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _c_f, _c_f, _int, _c_f]),
    'mvip_absmax_scale_sections': (_int, [_c_f, _i64, _i64, _i64, _c_f, _c_f, _c_f]),
    'mvip_attention_f16x3': (_int, [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _flt, _int,
                                    _c_f, _int, _c_f]),
    'mvip_gemm_f16x3_sinks': (_int, [_c_f, _c_f, _c_f, _c_f, _i64, _i64, _i64, _i64, _int, ctypes.POINTER(_i64),
                                     ctypes.POINTER(_int), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(_flt), _int, _int, _c_f]),
    'mvip_gemm_f16x3_planes_ws': (_int, [_c_f, _c_f, _c_f, _c_f, _c_f, _i64, _i64, _i64, _i64, _c_f, _flt, _c_f, _int, _c_f]),
    'mvip_gemm_geglu_f16x3_sink': (_int, [_c_f, _c_f, _c_f, _c_f, _i64, _i64, _i64, _i64, _i64, _c_f, _flt, _int, _c_f]),
    'mvip_attention_f16x3_sink': (_int, [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
                                         _i64, _i64, _flt, _int, _c_f, _int, _c_f]),
    'mvip_layernorm_workspace_bytes': (_i64, [_i64, _i64, _i64]),
    'mvip_layernorm_split_planes': (_int, [_c_f, _c_f, _c_f, _i64, _i64, _i64, _i64, _flt, _flt, _c_f, _c_f, _int, _c_f]),
    'mvip_geglu': (_int, [_c_f, _i64, _i64, _i64, _i64, _c_f, _c_f, _c_f, _c_f]),
    'mvip_linear_small': (_int, [_c_f, _c_f, _c_f, _i64, _i64, _i64, _int, _c_f, _c_f]),
    'mvip_linear_small_grouped': (_int, [_c_f, _c_f, _c_f, _i64, _i64, _i64, _int, _c_f, _i64, _c_f, _c_f]),
    'mvip_groupnorm_backward': (_int, [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _i64, _i64, _i64, _int, _int, _int, _c_f, _c_f,
                                       _c_f]),
    'mvip_conv3x3_row_moments_doubles': (_i64, [_i64, _i64, _i64, _i64, _i64]),
    'mvip_conv3x3_tile_moments_scratch_bytes': (_i64, [_i64, _i64, _i64, _i64, _i64]),
    'mvip_conv3x3_f16x3_tile_moments': (_int, [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _i64, _i64, _i64, _i64, _i64, _c_f, _c_f, _c_f,
                                               _int, _c_f]),
    'mvip_conv3x3_f16x3_ws_moments': (_int, [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _i64, _i64, _i64, _i64, _i64, _c_f, _c_f, _c_f,
                                             _int, _c_f]),
    'mvip_groupnorm_backward_maxima': (_i64, [_i64, _i64, _i64]),
    'mvip_groupnorm_backward_fused': (_int, [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _i64, _i64, _i64, _int, _int, _int, _c_f, _c_f,
                                             _c_f, _c_f, _c_f]),
    'mvip_absmax_scale_from_maxima': (_int, [_c_f, _i64, _c_f, _c_f]),
    'mvip_groupnorm_split_planes_moments': (_int, [_c_f, _c_f, _c_f, _c_f, _flt, _i64, _i64, _i64, _int, _int, _c_f, _int,
                                                   _c_f]),
    'mvip_groupnorm_split_planes_moments_out': (_int, [_c_f, _c_f, _c_f, _c_f, _flt, _i64, _i64, _i64, _int, _int, _c_f, _c_f, _c_f,
                                                       _int, _c_f]),
    'mvip_mcubes_groups': (_i64, [_int, _int, _int]),
    'mvip_mcubes_count': (_int, [_c_f, _int, _int, _int, _flt, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'mvip_mcubes_emit': (_int, [_c_f, _int, _int, _int, _flt, _flt, _flt, _flt, _flt, _flt, _flt, _c_f, _c_f, _c_f, _i64, _i64,
                                _c_f, _c_f, _c_f, _c_f, _c_f]),
    'mvip_mcubes_count_valid': (_int, [_c_f, _c_f, _int, _int, _int, _flt, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'mvip_occupancy_build': (_int, [_c_f, _int, _int, _int, _int, _flt, _c_f, _c_f]),
    'mvip_occupancy_dilate': (_int, [_c_f, _int, _int, _int, _c_f, _c_f]),
    'mvip_occupancy_groups': (_i64, [_i64, _int]),
    'mvip_occupancy_count': (_int, [_c_f, _c_f, _i64, _int, ctypes.POINTER(_flt), ctypes.POINTER(_int), _c_f, _c_f, _c_f, _c_f,
                                    _c_f, _c_f]),
    'mvip_occupancy_emit': (_int, [_c_f, _c_f, _i64, _int, ctypes.POINTER(_flt), ctypes.POINTER(_int), _c_f, _c_f, _i64, _c_f,
                                   _c_f, _c_f, _c_f]),
    'mvip_scatter_raw': (_int, [_c_f, _c_f, _i64, _i64, _c_f, _c_f]),
    'mvip_occupancy_lookup': (_int, [_c_f, _i64, ctypes.POINTER(_flt), ctypes.POINTER(_int), _c_f, _c_f, _c_f]),
    'mvip_region_mark': (_int, [_c_f, _i64, ctypes.POINTER(_flt), ctypes.POINTER(_int), _c_f, _c_f]),
    'mvip_region_accumulate': (_int, [_c_f, _c_f, _c_f, _i64, _int, ctypes.POINTER(_flt), ctypes.POINTER(_int), _c_f, _c_f, _c_f]),
    'mvip_region_lookup': (_int, [_c_f, _i64, ctypes.POINTER(_flt), ctypes.POINTER(_int), _c_f, _c_f, _c_f]),
    'mvip_components_pack': (_int, [_c_f, _i64, _flt, _c_f, _c_f]),
    'mvip_components_groups': (_i64, [_int, _int, _int]),
    'mvip_components_label': (_int, [_c_f, _int, _int, _int, _int, _c_f, _c_f, _c_f, _c_f]),
    'mvip_components_rank': (_int, [_c_f, _int, _int, _int, _c_f, _i64, _c_f, _c_f, _c_f, _c_f]),
    'mvip_components_select': (_int, [_c_f, _i64, _c_f, _i64, _c_f, _c_f]),
    'mvip_distortion_loss': (_int, [_c_f, _int, _c_f, _c_f, _i64, _int, _int, _c_f, _c_f, _c_f]),
    'mvip_harmonic_tiles': (_i64, [_int, _int]),
    'mvip_harmonic_workspace_bytes': (_i64, [_i64, _int, _int]),
    'mvip_harmonic_setup': (_int, [_c_f, _c_f, _i64, _int, _int, _c_f, _c_f, _c_f, _c_f]),
    'mvip_harmonic_init': (_int, [_c_f, _i64, _int, _int, _c_f, _c_f, _c_f, _i64, _c_f]),
    'mvip_poisson_init': (_int, [_c_f, _c_f, _c_f, _i64, _int, _int, _c_f, _c_f, _c_f, _i64, _c_f]),
    'mvip_harmonic_iterate': (_int, [_i64, _int, _int, _c_f, _c_f, _c_f, _i64, _int, _int, _flt, _c_f]),
    'mvip_harmonic_finish': (_int, [_i64, _int, _int, _c_f, _c_f, _c_f, _i64, _flt, _c_f]),
    'mvip_mask_dilate2d': (_int, [_c_f, _i64, _int, _int, _c_f, _c_f]),
    'mvip_warp_views': (_int, [_c_f, _c_f, _c_f, _i64, _int, _int, _c_f, _c_f, _c_f, _int, _c_f, _flt, _flt, _c_f, _c_f, _c_f, _c_f]),
    'mvip_ssim_tiles': (_i64, [_int, _int]),
    'mvip_ssim_forward': (_int, [_c_f, _c_f, _c_f, _i64, _int, _int, _int, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'mvip_ssim_backward': (_int, [_c_f, _c_f, _c_f, _c_f, _c_f, _i64, _int, _int, _int, _c_f, _c_f]),
    'mvip_exemplar_levels': (_int, [_int, _int, _int, _int]),
    'mvip_exemplar_meta_words': (_i64, [_i64]),
    'mvip_exemplar_workspace_bytes': (_i64, [_i64, _int, _int, _int, _int]),
    'mvip_exemplar_setup': (_int, [_c_f, _c_f, _c_f, _i64, _int, _int, _int, _int, _c_f, _c_f, _c_f]),
    'mvip_exemplar_lists': (_int, [_i64, _int, _int, _int, _int, _c_f, _c_f, _c_f, _i64, _c_f]),
    'mvip_exemplar_level': (_int, [_i64, _int, _int, _int, _int, _int, _i64, _i64, _int, _int, ctypes.c_uint, _c_f, _c_f, _c_f, _c_f]),
    'mvip_exemplar_finish': (_int, [_c_f, _i64, _int, _int, _int, _int, _int, _int, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'mvip_tsdf_fuse': (_int, [_c_f, _c_f, _c_f, _int, _int, _int, _flt, _int, _int, _int, _flt, _flt, _flt, _flt, _flt, _flt, _flt,
                              _c_f, _c_f, _c_f]),
    'mvip_mesh_list_scratch_words': (_i64, [_i64, _i64]),
    'mvip_mesh_corner_table': (_int, [_c_f, _i64, _i64, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'mvip_mesh_vertex_normals': (_int, [_c_f, _c_f, _i64, _i64, _c_f, _c_f, _c_f, _c_f]),
    'mvip_mesh_smooth_pass': (_int, [_c_f, _c_f, _i64, _i64, _c_f, _c_f, ctypes.c_double, _c_f, _c_f]),
    'mvip_mesh_rank_groups': (_i64, [_i64]),
    'mvip_mesh_cluster_assign': (_int, [_c_f, _i64, ctypes.POINTER(_flt), ctypes.POINTER(_int), _c_f, _c_f, _c_f, _c_f, _c_f, _c_f,
                                        _c_f, _c_f]),
    'mvip_mesh_gather': (_int, [_c_f, _i64, _c_f, _i64, _c_f, _c_f]),
    'mvip_mesh_cluster_place': (_int, [_c_f, _c_f, _c_f, _i64, _i64, ctypes.POINTER(_flt), ctypes.POINTER(_int), ctypes.c_double,
                                       _i64, _c_f, _c_f, _c_f, _c_f, _c_f, _int, _c_f, _c_f, _c_f]),
    'mvip_mesh_cluster_faces': (_int, [_c_f, _i64, _i64, _c_f, _c_f, _int, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'mvip_mesh_cluster_emit': (_int, [_c_f, _i64, _c_f, _c_f, _c_f, _c_f, _i64, _c_f, _c_f, _i64, _i64, _i64, _c_f, _c_f, _c_f, _c_f,
                                      _c_f]),
    'mvip_raster_fragments': (_int, [_c_f, _c_f, _i64, _i64, _c_f, _i64, _int, _int, ctypes.c_double, ctypes.c_double, _int, _c_f,
                                     _c_f, _c_f, _c_f]),
    'mvip_raster_resolve': (_int, [_c_f, _c_f, _c_f, _c_f, _i64, _i64, _c_f, _i64, _int, _int, ctypes.c_double, ctypes.c_double,
                                   _c_f, _c_f, _c_f, _c_f]),
    'mvip_texture_bake_points': (_int, [_c_f, _c_f, _i64, _c_f, _c_f, _c_f, _c_f, _i64, _int, _int, ctypes.c_double, ctypes.c_double,
                                        ctypes.c_double, _int, _int, _c_f, _c_f, _c_f, _c_f]),
    'mvip_texture_bake_atlas': (_int, [_c_f, _c_f, _i64, _i64, _int, _int, _c_f, _c_f, _c_f, _c_f, _i64, _int, _int, ctypes.c_double,
                                       ctypes.c_double, ctypes.c_double, _int, _int, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'mvip_texture_resolve': (_int, [_c_f, _c_f, _c_f, _i64, _i64, _c_f, _int, _c_f, _i64, _int, _int, ctypes.c_double, ctypes.c_double,
                                    _c_f, _c_f]),
    'mvip_mesh_distance_grid_count': (_int, [_c_f, _c_f, _i64, _i64, ctypes.POINTER(_flt), ctypes.POINTER(_int), _c_f, _c_f, _c_f,
                                             _c_f]),
    'mvip_mesh_distance_grid_scratch_words': (_i64, [_i64, ctypes.POINTER(_int)]),
    'mvip_mesh_distance_grid_fill': (_int, [_c_f, _c_f, _i64, _i64, ctypes.POINTER(_flt), ctypes.POINTER(_int), _c_f, _i64, _c_f,
                                            _c_f, _c_f, _c_f]),
    'mvip_mesh_distance_query': (_int, [_c_f, _i64, _c_f, _c_f, _i64, _i64, ctypes.POINTER(_flt), ctypes.POINTER(_int), _c_f, _c_f,
                                        _i64, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'mvip_mesh_sample_faces': (_int, [_c_f, _c_f, _i64, _i64, _int, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'mvip_mesh_raycast': (_int, [_c_f, _c_f, _c_f, _c_f, _flt, _flt, _c_f, _i64, _c_f, _c_f, _i64, _i64, ctypes.POINTER(_flt),
                                 ctypes.POINTER(_int), ctypes.POINTER(_flt), _c_f, _c_f, _i64, _int, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'mvip_mesh_face_openness': (_int, [_c_f, _c_f, _i64, _i64, ctypes.POINTER(_flt), ctypes.POINTER(_int), ctypes.POINTER(_flt),
                                       _c_f, _c_f, _i64, _c_f, _int, _flt, _c_f, _c_f, _c_f]),
    'mvip_ray_quantile_depth': (_int, [_c_f, _c_f, _i64, _int, ctypes.POINTER(_flt), _int, _c_f, _c_f]),
    'mvip_depth_consistency': (_int, [_c_f, _c_f, _int, _int, _int, _flt, _flt, _c_f, _c_f, _c_f]),
    'mvip_mesh_topology_keys': (_int, [_c_f, _i64, _i64, _c_f, _c_f, _c_f]),
    'mvip_mesh_topology_edges_find': (_int, [_c_f, _i64, _i64] + [_c_f] * 11),
    'mvip_mesh_topology_edges_emit': (_int, [_c_f, _i64, _c_f, _c_f, _c_f, _c_f, _i64] + [_c_f] * 6),
    'mvip_mesh_topology_components_label': (_int, [_c_f, _i64, _i64, _int] + [_c_f] * 9),
    'mvip_mesh_topology_components_emit': (_int, [_c_f, _i64, _i64, _c_f, _c_f, _i64] + [_c_f] * 8),
    'mvip_mesh_topology_loops_label': (_int, [_c_f, _i64, _i64] + [_c_f] * 12),
    'mvip_mesh_topology_loops_emit': (_int, [_i64, _c_f, _c_f, _c_f, _i64] + [_c_f] * 5),
    'mvip_mesh_topology_cap_plan': (_int, [_i64, _c_f, _i64, _c_f, _c_f, _i64] + [_c_f] * 8),
    'mvip_mesh_topology_cap_emit': (_int, [_c_f, _c_f, _c_f, _i64, _i64, _i64] + [_c_f] * 6 + [_i64, _i64] + [_c_f] * 4),
    'mvip_voxel_scratch_words': (_i64, [ctypes.POINTER(_int), _int]),
    'mvip_voxel_surface': (_int, [_c_f, _c_f, _i64, _i64, ctypes.POINTER(_flt), ctypes.POINTER(_int), _c_f, _c_f, _c_f]),
    'mvip_voxel_crossings': (_int, [_c_f, _c_f, _i64, _i64, ctypes.POINTER(_flt), ctypes.POINTER(_int), _int, _c_f, _c_f, _c_f]),
    'mvip_voxel_fill': (_int, [_c_f, ctypes.POINTER(_int), _int, _c_f, _c_f, _c_f]),
    'mvip_mesh_vertex_pseudonormals': (_int, [_c_f, _c_f, _i64, _i64, _c_f, _c_f, _c_f, _c_f]),
    'mvip_mesh_signed_distance': (_int, [_c_f, ctypes.POINTER(_flt), ctypes.POINTER(_flt), ctypes.POINTER(_int), _i64, _c_f, _c_f, _i64,
                                         _i64, ctypes.POINTER(_flt), ctypes.POINTER(_int), _c_f, _c_f, _i64, _c_f, _c_f,
                                         ctypes.c_double, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f]),
}

# every symbol include/mvip_nerf.h declares; tests check the built library exports all of them
DECLARED_SYMBOLS = tuple(_SIGNATURES)

_lib = None
ABI_VERSION = 5


class MvipError(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes handle.  Raises if the HIP library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MvipError(
            f'{LIB_PATH} not found: build it with `python -m mvip_nerf_amd.csrc.build` '
            '(or __graft_entry__.build()).  There is no CPU fallback.')
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)       # AttributeError if the .so is stale
        fn.restype = res
        fn.argtypes = args
    if lib.mvip_abi_version() != ABI_VERSION:
        raise MvipError('libmvipnerf.so ABI version mismatch')
    if lib.mvip_build_is_experiment() and os.environ.get('MVIP_ALLOW_EXPERIMENT_BUILD') != '1':
        raise MvipError(f'{LIB_PATH} was compiled with -DMVIP_EXPERIMENT_* (timing experiment, wrong results): rebuild with '
                        '`python -m mvip_nerf_amd.csrc.build`, or set MVIP_ALLOW_EXPERIMENT_BUILD=1 for the experiment itself')
    _lib = lib
    return lib


def check(code, what=''):
    if code != 0:
        lib = load()
        msg = lib.mvip_strerror(code).decode()
        if code == -2:
            msg += ': ' + lib.mvip_last_hip_error().decode()
        raise MvipError(f'{what or "mvip call"} failed: {msg}')


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t, dtype=torch.float32):
    """Device pointer of a dense tensor (None -> NULL)."""
    if t is None:
        return ctypes.c_void_p(0)
    if not t.is_cuda:
        raise MvipError('expected a CUDA/HIP tensor (the HIP path has no CPU fallback)')
    if t.dtype != dtype:
        raise MvipError(f'expected dtype {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise MvipError('expected a contiguous tensor')
    return ctypes.c_void_p(t.data_ptr())


def ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = ptr(t).value
    return arr


def call(name, *args):
    lib = load()
    check(getattr(lib, name)(*args), name)
