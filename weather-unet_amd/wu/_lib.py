"""ctypes binding of libwu_kernels.so -- the C ABI declared in include/wu_kernels.h.

There is deliberately NO fallback: if the shared library is missing or a call fails, the product
raises.  (The CPU oracle under oracle/ is test infrastructure and is never imported from here.)
"""
import ctypes
import os

from ctypes import c_char_p, c_double, c_float, c_int, c_size_t, c_uint64, c_void_p, POINTER

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG, "lib", "libwu_kernels.so")

F32, BF16 = 0, 1
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
OPT_CONV_V2, OPT_CONV_PERSISTENT, OPT_WGRAD_V2 = 0, 1, 2
FAM_CONV_FWD, FAM_WGRAD, FAM_CONV_DGRAD, FAM_CONV_S2, FAM_WGRAD_S2, FAM_CONV1X1 = 1, 2, 3, 4, 5, 6
FAM_GRID = 7         # the launches of wu_grid_compose (wu/grid.py)
FAMILY_KERNEL = {1: "conv3x3_mfma_v2_kernel (forward + data-gradient convs; generic conv3x3_mfma_kernel for fp32 / narrow images)",
                 2: "conv3x3_wgrad_v2_kernel (generic conv3x3_wgrad_kernel for fp32 / narrow images)",
                 3: "conv3x3_mfma_kernel<T,1,true> (in-kernel gated dgrad; unused by the fused graph)",
                 4: "stride-2 3x3 conv forward + data gradient: conv1x1_pw3_kernel<.., CONV> (gathered rows); conv3x3_mfma_kernel<T,2,false> / tap-list classes for 64-cout and fp32",
                 5: "conv3x3_wgrad_kernel<T,2>",
                 6: "pointwise convs (estimator): conv1x1_pw3_kernel; conv1x1_mfma_kernel<T> for strided / small / fp32"}

P, I, F, U64, SZ = c_void_p, c_int, c_float, c_uint64, c_size_t

# name -> (restype, argtypes); mirrors include/wu_kernels.h one to one
SIGNATURES = {
    "wu_last_error": (c_char_p, []),
    "wu_version": (I, []),
    "wu_cu_count": (I, []),
    "wu_set_option": (I, [I, I]),
    "wu_set_debug_buffer": (I, [P]),
    "wu_stream_create_cu_mask": (I, [P, I, P]),
    "wu_stream_destroy": (I, [P]),
    "wu_spectral_norm_scratch_floats": (SZ, [I, I]),
    "wu_spectral_norm_fwd": (I, [P, I, I, P, P, I, F, P, P, P, P]),
    "wu_spectral_norm_bwd": (I, [P, P, P, P, P, P, I, I, P, P]),
    "wu_event_create": (I, [P]),
    "wu_event_destroy": (I, [P]),
    "wu_stream_order_after": (I, [P, P, P]),
    "wu_spectral_norm_fwd_multi": (I, [I, P, P, P, P, P, I, F, P, P, P, P, P, P]),
    "wu_spectral_norm_bwd_multi": (I, [I, P, P, P, P, P, P, P, P, P, P]),
    "wu_pack_conv3x3": (I, [P, P, P, I, I, P, I, P]),
    "wu_pack_conv3x3_multi": (I, [I, P, P, P, P, P, I, P]),
    "wu_conv3x3_fwd": (I, [P, I, P, P, P, I, I, I, I, I, I, I, I, P, I, I, P, I, I, I, P]),
    "wu_conv3x3_gate_bits_supported": (I, [I, I, I, I, I, I, I]),
    "wu_gate_bits_bytes": (SZ, [I, I, I, I]),
    "wu_conv3x3_fwd_bits": (I, [P, I, P, P, P, I, P, P, I, I, I, I, I, I, I, P]),
    "wu_conv3x3_relu_pool_fwd": (I, [P, I, P, P, P, I, P, I, I, I, I, I, I, I, P]),
    "wu_conv3x3_relu_pool_bits_fwd": (I, [P, I, P, P, P, I, P, I, P, P, I, I, I, I, I, I, P]),
    "wu_conv3x3_small_supported": (I, [I, I, I, I, I, I, I, I]),
    "wu_conv3x3_small_fwd": (I, [P, I, P, P, P, I, P, I, I, I, I, I, I, I, I, P]),
    "wu_conv3x3_relu_head_supported": (I, [I, I, I, I, I, I, I]),
    "wu_conv3x3_relu_head_fwd": (I, [P, I, P, P, P, I, P, P, P, I, I, I, I, I, I, P]),
    "wu_maxpool2_bwd_bits": (I, [P, P, P, I, P, I, P, I, I, I, I, I, I, P]),
    "wu_conv3x3_wgrad_workspace": (SZ, [I, I, I, I, I, I, I]),
    "wu_conv3x3_wgrad": (I, [P, I, P, I, P, I, I, P, P, P, SZ, I, I, I, I, I, I, I, I, P]),
    "wu_conv3x3_s2_dgrad_workspace": (SZ, [I, I, I, I, I]),
    "wu_conv3x3_s2_dgrad": (I, [P, I, P, I, I, P, P, I, P, SZ, P, I, I, I, I, I, I, I, I, P]),
    "wu_act_gate": (I, [P, I, P, I, P, I, I, I, I, I, I, I, P]),
    "wu_conv3x3_c3_fwd": (I, [P, P, P, P, P, I, I, I, I, I, I, I, I, I, P]),
    "wu_conv3x3_c3_gate_bits_supported": (I, [I, I, I, I, I, P, I]),
    "wu_conv3x3_c3_fwd_bits": (I, [P, P, P, P, P, I, P, I, I, I, I, I, I, P]),
    "wu_conv3x3_c3_wgrad": (I, [P, P, I, I, P, I, I, P, P, P, SZ, I, I, I, I, I, I, I, P]),
    "wu_thin_workspace_bytes": (SZ, []),
    "wu_conv3x3_c3_dgrad": (I, [P, I, I, P, I, I, P, P, P, I, I, I, I, I, I, I, P]),
    "wu_conv1x1_tanh_fwd": (I, [P, I, P, P, P, I, I, I, I, I, P]),
    "wu_conv1x1_tanh_bwd": (I, [P, P, P, I, P, P, I, P, P, P, SZ, I, I, I, I, I, I, I, P]),
    "wu_maxpool2_fwd": (I, [P, I, P, I, I, I, I, I, I, P]),
    "wu_maxpool2_bwd": (I, [P, I, P, I, P, I, P, I, I, I, I, I, I, I, P]),
    "wu_adain_style_fwd": (I, [P, P, P, F, P, P, P, I, I, I, P]),
    "wu_adain_style_bwd": (I, [P, P, P, P, P, P, P, P, I, I, I, I, P]),
    "wu_adain_style_fwd_multi": (I, [I, P, P, P, P, P, P, P, I, P, I, P]),
    "wu_adain_style_bwd_multi": (I, [I, P, P, P, P, P, P, P, P, I, P, I, I, P]),
    "wu_adain_stats": (I, [P, I, P, P, I, I, I, I, F, I, P]),
    "wu_adain_stats_as_batch": (I, [P, I, P, P, I, I, I, I, F, I, I, P]),
    "wu_adain_upcat_fwd": (I, [P, I, P, P, P, P, I, I, I, I, I, F, U64, P, P, I, I, P]),
    "wu_adain_upcat_sweep_fwd": (I, [P, I, I, P, P, P, P, I, I, I, P, I, I, I, I, I, F, U64, P, I, P]),
    "wu_adain_upcat_bwd": (I, [P, I, P, I, P, P, P, I, P, P, P, P, I, I, I, I, F, U64, P, I, I, P]),
    "wu_dropout_mask": (I, [P, I, I, I, I, F, U64, P]),
    "wu_l1_mean_scratch_floats": (SZ, []),
    "wu_l1_mean": (I, [P, P, P, P, P, ctypes.c_longlong, P]),
    "wu_sumpool_fwd": (I, [P, I, P, I, I, I, I, I, P]),
    "wu_sumpool_bwd": (I, [P, P, I, I, I, I, I, I, P]),
    "wu_nhwc_to_nchw_f32": (I, [P, I, P, I, I, I, I, I, P]),
    "wu_nchw_f32_to_nhwc": (I, [P, P, I, I, I, I, I, I, P]),
    "wu_conv1x1_fwd": (I, [P, I, P, P, P, I, P, I, I, I, I, I, I, I, I, I, I, I, I, I, P, I, I, I, P]),
    "wu_conv1x1_chain_supported": (I, [I, I, I, I]),
    "wu_conv1x1_chain": (I, [P, I, P, P, P, I, I, P, I, I, P, I, P, P, I, P, I, I, P, I, ctypes.c_longlong, I, I, I, I, P]),
    "wu_stem7x7_fwd": (I, [P, P, P, P, I, I, I, I, I, I, P]),
    "wu_stem7x7_dgrad": (I, [P, I, P, P, I, I, I, I, I, P]),
    "wu_maxpool3s2_fwd": (I, [P, I, P, I, P, I, I, I, I, I, P]),
    "wu_maxpool3s2_bwd": (I, [P, I, P, P, I, P, I, I, I, I, I, I, I, P]),
    "wu_bn_stats_workspace": (SZ, [ctypes.c_longlong, I, I]),
    "wu_bn_stats": (I, [P, I, ctypes.c_longlong, I, F, F, P, P, P, P, P, SZ, I, P]),
    "wu_bn_apply": (I, [P, I, P, P, P, P, I, P, P, P, P, I, P, I, ctypes.c_longlong, I, I, I, P]),
    "wu_bn_bwd_workspace": (SZ, [ctypes.c_longlong, I, I]),
    "wu_bn_bwd": (I, [P, I, P, I, I, P, I, P, P, P, P, P, I, P, I, P, P, P, P, P, I, P, I, ctypes.c_longlong, I, P, SZ, I, P]),
    "wu_conv1x1_wgrad_workspace": (SZ, [ctypes.c_longlong, I, I]),
    "wu_conv1x1_wgrad": (I, [P, I, P, I, P, P, SZ, I, I, I, I, I, I, I, I, I, I, P]),
    "wu_stem7x7_wgrad_workspace": (SZ, [I, I, I]),
    "wu_stem7x7_wgrad": (I, [P, P, I, P, P, SZ, I, I, I, I, I, P]),
    "wu_image_geo_bytes": (SZ, []),
    "wu_image_workspace_bytes": (SZ, [I, I, I]),
    "wu_image_geometry": (I, [P, P, P, SZ, P, P, I, I, I, I, P]),
    "wu_image_color_jitter": (I, [P, P, P, P, I, I, P]),
    "wu_jpeg_info_bytes": (SZ, []),
    "wu_jpeg_parse": (I, [P, SZ, P]),
    "wu_jpeg_parse_ex": (I, [P, SZ, P, I]),
    "wu_jpeg_entropy_decode": (I, [P, SZ, P, P, SZ, P]),
    "wu_jpeg_max_block_l1": (I, []),
    "wu_jpeg_desc_bytes": (SZ, []),
    "wu_jpeg_workspace_bytes": (SZ, [ctypes.c_longlong]),
    "wu_jpeg_reconstruct": (I, [P, P, P, P, P, SZ, P, I, I, I, I, P]),
    "wu_jpeg_scan_stage_bytes": (SZ, [P, SZ, I]),
    "wu_jpeg_scan_segments": (I, [P]),
    "wu_jpeg_scan_stage": (I, [P, SZ, P, I, P, SZ, P, SZ, P, P, P]),
    "wu_jpeg_huff_desc_bytes": (SZ, []),
    "wu_jpeg_huff_decode": (I, [P, P, P, P, P, P, P, I, I, P]),
    "wu_jpeg_enc_header_bytes": (SZ, []),
    "wu_jpeg_enc_header": (I, [I, I, I, I, P, SZ]),
    "wu_jpeg_enc_qtables": (I, [I, P]),
    "wu_jpeg_enc_desc_bytes": (SZ, []),
    "wu_jpeg_enc_workspace_bytes": (SZ, [I, I, I, I, ctypes.c_longlong]),
    "wu_jpeg_enc_out_stride": (SZ, [ctypes.c_longlong]),
    "wu_jpeg_enc_workspace_layout": (I, [I, I, I, I, ctypes.c_longlong, P]),
    "wu_jpeg_enc_encode": (I, [P, I, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, P, P, P, I, P, SZ, P, SZ, P, I, I, I, I, ctypes.c_longlong, P]),
    "wu_png_enc_desc_bytes": (SZ, []),
    "wu_png_enc_segment_bytes": (SZ, []),
    "wu_png_enc_workspace_bytes": (SZ, [I, I, I]),
    "wu_png_enc_out_stride": (SZ, [I, I]),
    "wu_png_enc_encode": (I, [P, I, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, P, P, SZ, P, SZ, P, I, I, I, P]),
    "wu_png_enc_workspace_bytes_ex": (SZ, [I, I, I, I]),
    "wu_png_enc_seginfo_offset": (SZ, [I, I, I]),
    "wu_png_enc_encode_ex": (I, [P, I, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, P, P, SZ, P, SZ, P, I, I, I, I, P]),
    "wu_gif_enc_segment_pixels": (SZ, []),
    "wu_gif_enc_workspace_bytes": (SZ, [I, I, I]),
    "wu_gif_enc_block_stride": (SZ, [I, I]),
    "wu_gif_enc_encode": (I, [P, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, P, SZ, P, SZ, P, I, I, I, I, P]),
    "wu_gif_enc_workspace_bytes_ex": (SZ, [I, I, I, I]),
    "wu_gif_enc_block_stride_ex": (SZ, [I, I, I]),
    "wu_gif_enc_encode_ex": (I, [P, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, P, SZ, P, SZ, P, I, I, I, I, I, P, P,
                                 P]),
    "wu_grid_cell_bytes": (SZ, []),
    "wu_grid_workspace_bytes": (SZ, [I, I]),
    "wu_grid_workspace_layout": (I, [I, I, P]),
    "wu_grid_compose": (I, [P, I, I, P, SZ, P, SZ, I, I, I, I, F, P]),
    "wu_png_dec_info_bytes": (SZ, []),
    "wu_png_dec_max_chunk_bytes": (SZ, []),
    "wu_png_dec_parse": (I, [P, SZ, ctypes.c_longlong, P, P, I]),
    "wu_png_dec_desc_bytes": (SZ, []),
    "wu_png_dec_seg_bytes": (SZ, []),
    "wu_png_dec_workspace_bytes": (SZ, [I, I, I, ctypes.c_longlong]),
    "wu_png_dec_decode": (I, [P, SZ, P, SZ, P, SZ, I, P, SZ, P, SZ, P, SZ, I, I, I, P]),
    "wu_conv_kxk_packed_bytes":(SZ, [I, I, I, I, I]),
    "wu_pack_conv_kxk": (I, [P, P, I, I, I, I, I, I, P]),
    "wu_conv_kxk_fwd": (I, [P, I, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, I, I, P]),
    "wu_pool3x3_fwd": (I, [P, I, P, I, I, I, I, I, I, I, I, I, P]),
    "wu_global_avgpool_fwd": (I, [P, I, P, I, I, I, I, I, I, P]),
    "wu_inception_input": (I, [P, I, I, I, I, F, F, I, P, I, I, I, I, I, P]),
    "wu_feature_stats_update": (I, [P, I, I, I, P, I, P, P, P]),
    "wu_kid_workspace_bytes": (SZ, [I, I]),
    "wu_kid_mmd": (I, [P, I, I, P, I, I, P, I, I, I, I, c_double, c_double, P, P, P, P]),
    "wu_prdc_workspace_bytes": (SZ, [I, I, I, I]),
    "wu_knn_radii": (I, [P, I, I, I, I, I, P, P, P]),
    "wu_prdc_counts": (I, [P, I, I, P, P, I, I, P, I, P, P, P, P, P]),
    "wu_nn_workspace_bytes": (SZ, [I, I, I, I]),
    "wu_nn_topk": (I, [P, I, I, P, I, I, I, I, I, I, P, SZ, P, P, P]),
    "wu_nn_radius_workspace_bytes": (SZ, [I, I, I]),
    "wu_nn_radius_count": (I, [P, I, I, P, I, I, I, c_double, I, I, I, P, SZ, P, P]),
    "wu_nn_radius_fill": (I, [P, I, I, P, I, I, I, c_double, I, I, I, P, SZ, P, ctypes.c_longlong, P, P, P]),
    "wu_nn_ball_workspace_bytes": (SZ, [I, I, I]),
    "wu_nn_ball_scores": (I, [P, I, I, P, I, I, I, P, I, I, P, SZ, P, P, P, P, P, P, P]),
    "wu_fd_ld": (I, [I, I]),
    "wu_fd_workspace_bytes": (SZ, [I, I, I]),
    "wu_fd_cross_gram": (I, [P, I, I, P, I, I, I, P, P]),
    "wu_fd_moments": (I, [P, I, I, I, P, P, P, P]),
    "wu_fd_jacobi_sweep": (I, [P, I, I, I, P, P]),
    "wu_fd_finish": (I, [P, I, I, I, P, P, P]),
    "wu_ssim_workspace_bytes": (SZ, [I, I, I, I, I, I, I]),
    "wu_ssim_tile_h": (I, []),
    "wu_ssim_tile_w": (I, []),
    "wu_ssim_pairs": (I, [P] + [ctypes.c_longlong] * 4 + [P] + [ctypes.c_longlong] * 5 + [I] * 6 + [c_double] * 5 + [P, I, I, P, P, P, P, P, P]),
    "wu_swd_sort_block": (I, []),
    "wu_swd_pyramid_workspace_bytes": (SZ, [I, I, I, I, I]),
    "wu_swd_descriptors": (I, [P] + [ctypes.c_longlong] * 4 + [I, I, I, I, c_double, c_double, I, P, I, P, P, P]),
    "wu_swd_stats_workspace_bytes": (SZ, [I]),
    "wu_swd_normalize": (I, [P, I, P, P, P, P]),
    "wu_swd_workspace_bytes": (SZ, [I, I, I]),
    "wu_swd_project_sort": (I, [P, I, P, I, I, P, P, P]),
    "wu_swd_sort_columns": (I, [P, I, I, P, P]),
    "wu_swd_distance": (I, [P, P, I, I, P, P]),
    "wu_swd_distance_unequal": (I, [P, I, P, I, I, P, P]),
    "wu_spectrum_bins": (I, [I, I]),
    "wu_spectrum_workspace_bytes": (SZ, [I, I, I]),
    "wu_spectrum_luma": (I, [P] + [ctypes.c_longlong] * 4 + [I, I, I, I, I, c_double, c_double, c_double, P, P, P, P]),
    "wu_spectrum_profiles_planes": (I, [P, I, I, I, P, P, P, P, I, P, P, P, P]),
    "wu_spectrum_profiles": (I, [P] + [ctypes.c_longlong] * 4 + [I, I, I, I, I, c_double, c_double, c_double] + [P] * 6 + [I, P, P, P, P]),
    "wu_colour_ot_workspace_bytes": (SZ, [I, I, I, I]),
    "wu_colour_ot_load": (I, [P] + [ctypes.c_longlong] * 4 + [I, I, I, I, c_double, c_double, c_double, ctypes.c_longlong, I, P, P]),
    "wu_colour_ot_palette_keys": (I, [P, I, I, P, P, P, P]),
    "wu_colour_ot_step": (I, [P, I, I, P, I, I, P, P, c_double, P, P]),
    "wu_colour_ot_store": (I, [P, ctypes.c_longlong, I, P] + [ctypes.c_longlong] * 5 + [I, I, I, I, c_double, c_double, I, P]),
    "wu_colour_regrain_workspace_bytes": (SZ, [I, I, I, I]),
    "wu_colour_regrain_levels": (I, [I, I, I, I]),
    "wu_colour_regrain": (I, [P, P, I, I, I, I, P, c_double, P, P]),
    "wu_colour_moments_workspace_bytes": (SZ, [I, I]),
    "wu_colour_moments": (I, [P, ctypes.c_longlong, ctypes.c_longlong, I, I, P, P, P]),
    "wu_colour_linear_apply": (I, [P, I, I, P, P, I, P, I, c_double, P]),
    "wu_lpips_tile_pixels": (I, []),
    "wu_lpips_workspace_bytes": (SZ, [I, I, I, I, I]),
    "wu_lpips_input": (I, [P] + [ctypes.c_longlong] * 4 + [I, I, I, I, c_float, c_float, P, I, P]),
    "wu_lpips_head": (I, [P, I, P, I, ctypes.c_longlong, P, I, I, I, I, I, I, P, P, I, P]),
    "wu_lpips_pairs": (I, [P, I, ctypes.c_longlong, P, I, I, I, I, I, I, P, P, I, P]),
    "wu_guided_workspace_bytes": (SZ, [I, I, I, I]),
    "wu_guided_tile_h": (I, []),
    "wu_guided_tile_w": (I, []),
    "wu_guided_coeffs": (I, [P] + [ctypes.c_longlong] * 4 + [c_double, c_double, P] + [ctypes.c_longlong] * 5 + [I, c_double, c_double]
                         + [I] * 5 + [c_double, P, P, P]),
    "wu_guided_apply": (I, [P, I, I, I, I, P, I, I, P, P, P, P, P]),
    "wu_resample_desc_bytes": (SZ, []),
    "wu_resample_max_band": (I, []),
    "wu_resample_workspace_bytes": (SZ, [I, SZ]),
    "wu_resample": (I, [P, I, P, P, SZ, I, I, I, P, I, I, I, I, P]),
    "wu_prof_begin": (I, [ctypes.c_uint, I]),
    "wu_prof_query": (I, [I, POINTER(c_int), POINTER(c_double), POINTER(c_double), POINTER(c_double)]),
    "wu_prof_end": (I, []),
}

_lib = None
LOADED_PATH = None       # the file load() actually opened (bench.py reports it when it is not the in-tree library)


def load():
    """Load the shared library (once).  Raises if it has not been built -- no silent fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python weather-unet_amd/wu/_build.py` "
                "(or __graft_entry__.build()).  There is no CPU / PyTorch fallback for the hot path.")
        # torch bundles its own libamdhip64 (same soname as /opt/rocm's): import it FIRST so the dynamic
        # loader binds this library to the HIP runtime instance torch initialises -- two runtime copies in
        # one process do not share devices, streams or allocations.
        import torch  # noqa: F401
        # WU_AB_LIB: benchmark harness only (scratch/): run the whole product path on ANOTHER build of the library (a baseline
        # revision, scratch/build_baseline_lib.sh) for same-box A/B timing of the full step; entry points that build lacks stay unbound
        ab = os.environ.get("WU_AB_LIB")
        if not ab:
            _check_not_stale()
        else:
            # never silently: a leftover variable would run training on a stale baseline build (advisor, round 3)
            import sys
            print(f"[wu] WARNING: WU_AB_LIB is set -- running on {ab} instead of {LIB_PATH}; no staleness check, entry points "
                  "that build lacks stay unbound.  Benchmark A/B harness only (scratch/ab_lib.py).", file=sys.stderr, flush=True)
        global LOADED_PATH
        LOADED_PATH = ab or LIB_PATH
        lib = ctypes.CDLL(LOADED_PATH)
        for name, (res, args) in SIGNATURES.items():
            if ab and not hasattr(lib, name):
                continue
            fn = getattr(lib, name)       # AttributeError if the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        # WU_SET_OPTIONS="key=value,...": diagnostic switches of the library (include/wu_kernels.h, wu_set_option) from the environment --
        # same-box A/B runs of a whole benchmark (scratch/ab_gan_env.sh); announced, never silent
        opts = os.environ.get("WU_SET_OPTIONS")
        if opts:
            import sys
            print(f"[wu] WU_SET_OPTIONS={opts}", file=sys.stderr, flush=True)
            for kv in opts.split(","):
                k, _, v = kv.partition("=")
                if lib.wu_set_option(int(k), int(v)) != 0:
                    raise RuntimeError(f"WU_SET_OPTIONS: wu_set_option({k}, {v}) refused")
    return _lib


def _check_not_stale():
    """A library built from other sources than the ones in the tree must never run silently: compare the content hash the
    build recorded with the tree's (skipped when the sources did not travel with the library)."""
    from . import _build
    if not os.path.isdir(_build.CSRC):
        return
    if _build.is_stale():
        if os.environ.get("WU_ALLOW_STALE_LIB"):
            return
        raise RuntimeError(f"{LIB_PATH} was not built from the sources in {_build.CSRC} (content hash mismatch): "
                           "run `python weather-unet_amd/wu/_build.py` (or __graft_entry__.build()); "
                           "WU_ALLOW_STALE_LIB=1 overrides")


def check(rc, what):
    if rc != 0:
        msg = load().wu_last_error()
        raise RuntimeError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")


def call(name, *args):
    """Call an int-returning entry point and raise on a non-zero return."""
    check(getattr(load(), name)(*args), name)


def prof_begin(families, max_launches):
    mask = 0
    for f in families:
        mask |= 1 << f
    call("wu_prof_begin", mask, int(max_launches))


def prof_query(family):
    n, ms, fl, by = c_int(0), c_double(0), c_double(0), c_double(0)
    call("wu_prof_query", family, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by))
    return {"launches": n.value, "ms": ms.value, "flops": fl.value, "bytes": by.value}


def prof_end():
    call("wu_prof_end")
