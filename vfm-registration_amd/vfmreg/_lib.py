"""ctypes loader for libvfmreg_hip.so (the C ABI declared in include/vfmreg.h).

The product path has NO CPU fallback: if the HIP library is missing this module raises, and every
op in ``vfmreg.ops`` refuses to run without a ROCm device.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_PATH = _HERE / "lib" / "libvfmreg_hip.so"
_lib = None

c_i64 = C.c_int64
c_vp = C.c_void_p


class VitConfig(C.Structure):
    _fields_ = [("dim", C.c_int), ("depth", C.c_int), ("heads", C.c_int), ("mlp_dim", C.c_int),
                ("patch", C.c_int), ("patch_h", C.c_int), ("patch_w", C.c_int)]


class LiftCamera(C.Structure):  # vfm_lift_camera
    _fields_ = [("mode", C.c_int), ("mats", C.c_double * 48), ("fc", C.c_double * 4), ("subsample", C.c_double),
                ("win", C.c_int64 * 4), ("H", C.c_int64), ("W", C.c_int64), ("proj_image", C.c_void_p),
                ("grid", C.c_void_p), ("raw_image", C.c_void_p), ("gh", C.c_int), ("gw", C.c_int), ("Hup", C.c_int),
                ("Wup", C.c_int), ("rot_mode", C.c_int)]


class RectifyCamera(C.Structure):  # vfm_rectify_camera
    _fields_ = [("mosaic", C.c_void_p), ("H", C.c_int64), ("W", C.c_int64), ("pattern", C.c_int), ("table", C.c_void_p),
                ("crop_bottom", C.c_int64), ("subsample", C.c_int), ("out", C.c_void_p)]


# name -> (restype, argtypes); mirrors include/vfmreg.h one to one
SIGNATURES = {
    "vfm_last_error": (C.c_char_p, []),
    "vfm_build_info": (C.c_char_p, []),
    "vfm_config_create": (C.c_int, [C.POINTER(c_vp)]),
    "vfm_config_destroy": (C.c_int, [c_vp]),
    "vfm_config_set": (C.c_int, [c_vp, C.c_char_p, c_i64]),
    "vfm_config_get": (C.c_int, [c_vp, C.c_char_p, C.POINTER(c_i64)]),
    "vfm_config_use": (C.c_int, [c_vp]),
    "vfm_l2norm_rows_f32": (C.c_int, [c_vp, c_i64, C.c_int, c_vp, c_vp]),
    "vfm_match_ip_top1_workspace_bytes": (C.c_size_t, [c_i64, c_i64, C.c_int, C.c_int]),
    "vfm_match_ip_top1": (C.c_int, [c_vp, c_i64, c_vp, c_i64, C.c_int, C.c_int, c_vp, c_vp, c_vp, C.c_size_t, c_vp]),
    "vfm_match_ip_top1_gated": (C.c_int, [c_vp, c_i64, c_vp, c_i64, C.c_int, C.c_int, C.c_float, c_vp, c_vp, c_vp, C.c_size_t,
                                          c_vp]),
    "vfm_match_ip_topk_workspace_bytes": (C.c_size_t, [c_i64, c_i64, C.c_int, C.c_int, C.c_int]),
    "vfm_match_ip_topk": (C.c_int, [c_vp, c_i64, c_vp, c_i64, C.c_int, C.c_int, C.c_int, c_vp, c_vp, c_vp, c_vp, C.c_size_t, c_vp]),
    "vfm_match_ip_topk_prepared_workspace_bytes": (C.c_size_t, [c_i64, C.c_int, C.c_int]),
    "vfm_match_ip_topk_prepared": (C.c_int, [c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, C.c_int, C.c_int, c_vp, c_vp, c_vp, c_vp, C.c_size_t, c_vp]),
    "vfm_match_prepared_bytes": (C.c_size_t, [c_i64, C.c_int]),
    "vfm_match_prepare": (C.c_int, [c_vp, c_i64, C.c_int, c_vp, c_vp]),
    "vfm_match_prepare2": (C.c_int, [c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, C.c_int, c_vp]),
    "vfm_match_prepare2_gated": (C.c_int, [c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, C.c_int, c_vp]),
    "vfm_match_prepare2_gated_p": (C.c_int, [c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, C.c_int, C.c_int, c_vp]),
    "vfm_match_prepare2_gated_z": (C.c_int, [c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, C.c_int, C.c_int, c_vp, C.c_size_t, c_i64, c_i64, c_vp]),
    "vfm_match_prepare2_gated_t": (C.c_int, [c_vp, C.c_int, c_i64, c_vp, c_vp, C.c_int, c_i64, c_vp, C.c_int, C.c_int, c_vp]),
    "vfm_match_search_finish_gated_t": (C.c_int, [c_vp, C.c_int, c_vp, c_i64, c_vp, C.c_int, c_vp, c_i64, C.c_int, c_vp, c_vp, c_vp,
                                                  C.c_size_t, C.c_float, C.c_int, c_vp]),
    "vfm_match_search_workspace_bytes": (C.c_size_t, [c_i64, c_i64, C.c_int]),
    "vfm_match_search_prepared": (C.c_int, [c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, C.c_int, c_vp, c_vp, c_vp,
                                            C.c_size_t, c_vp]),
    "vfm_match_search_coarse": (C.c_int, [c_vp, c_i64, c_vp, c_i64, C.c_int, c_vp, C.c_size_t, c_vp]),
    "vfm_match_search_rescans_async": (C.c_int, [c_vp, c_i64, c_i64, c_vp, c_vp]),
    "vfm_match_search_probe_half": (C.c_int, [c_vp, c_i64, c_vp, c_i64, C.c_int, c_vp, C.c_size_t, C.c_float, c_vp, c_vp]),
    "vfm_match_search_coarse_gated": (C.c_int, [c_vp, c_i64, c_vp, c_i64, C.c_int, c_vp, C.c_size_t, c_vp]),
    "vfm_match_search_coarse_gated_r": (C.c_int, [c_vp, c_i64, c_vp, c_i64, C.c_int, c_vp, C.c_size_t, C.c_int, c_vp]),
    "vfm_match_search_coarse_gated_g": (C.c_int, [c_vp, c_i64, c_vp, c_i64, C.c_int, c_vp, C.c_size_t, C.c_int, C.c_float, c_vp]),
    "vfm_match_search_finish_gated_r": (C.c_int, [c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, C.c_int, c_vp, c_vp, c_vp,
                                                  C.c_size_t, C.c_float, C.c_int, c_vp]),
    "vfm_match_search_finish": (C.c_int, [c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, C.c_int, c_vp, c_vp, c_vp,
                                          C.c_size_t, c_vp]),
    "vfm_match_search_finish_gated": (C.c_int, [c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, C.c_int, c_vp, c_vp, c_vp,
                                                C.c_size_t, C.c_float, c_vp]),
    "vfm_threshold_compact": (C.c_int, [c_vp, c_vp, c_i64, C.c_double, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "vfm_match_mutual_l2_workspace_bytes": (C.c_size_t, [c_i64, c_i64, C.c_int, C.c_int, C.c_int]),
    "vfm_match_mutual_l2": (C.c_int, [c_vp, c_i64, c_vp, c_i64, C.c_int, C.c_int, c_vp, c_vp, c_vp, c_vp, C.c_size_t,
                                      c_vp]),
    "vfm_match_mutual_pairs_workspace_bytes": (C.c_size_t, [c_i64, c_i64, C.c_int]),
    "vfm_match_mutual_pairs": (C.c_int, [c_vp, c_i64, c_vp, c_i64, C.c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, C.c_size_t, c_vp]),
    "vfm_ransac_workspace_bytes": (C.c_size_t, [c_i64, C.c_int32]),
    "vfm_ransac_corr": (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, C.c_double, C.c_int32, C.c_uint64, c_vp, c_vp, c_vp,
                                  c_vp, c_vp, c_vp, C.c_size_t, c_vp]),
    "vfm_ransac_corr_bounded": (C.c_int, [c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_i64, C.c_double, C.c_int32, C.c_uint64, c_vp, c_vp, c_vp,
                                          c_vp, c_vp, c_vp, c_vp, C.c_size_t, c_vp]),
    "vfm_kabsch_batched": (C.c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, C.c_double, c_vp, c_vp, c_vp]),
    "vfm_project_workspace_bytes": (C.c_size_t, [c_i64]),
    "vfm_project_pinhole_f64": (C.c_int, [C.c_int, c_vp, c_i64, c_vp, c_vp, C.c_double, c_vp, c_vp, c_i64, c_i64,
                                          c_vp, c_vp, c_vp, c_vp, c_vp, C.c_size_t, c_vp]),
    "vfm_lift_multicam": (C.c_int, [c_vp, c_i64, C.c_int, c_vp, C.c_int, c_vp, c_vp, c_vp]),
    "vfm_gather_bilinear_patchgrid": (C.c_int, [c_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_vp, c_vp,
                                                c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "vfm_demosaic_bilinear": (C.c_int, [c_vp, c_i64, c_i64, C.c_int, c_vp, c_vp]),
    "vfm_undistort_lut": (C.c_int, [c_vp, C.c_int, c_i64, c_i64, C.c_int, c_vp, c_vp, c_vp]),
    "vfm_rectify_bayer_workspace_bytes": (C.c_size_t, [C.c_int, c_vp]),
    "vfm_rectify_bayer": (C.c_int, [C.c_int, c_vp, c_vp, C.c_size_t, c_vp]),
    "vfm_transform_xyz_f64": (C.c_int, [c_vp, c_i64, c_vp, c_vp, c_vp]),
    "vfm_voxel_first_workspace_bytes": (C.c_size_t, [c_i64]),
    "vfm_voxel_first": (C.c_int, [c_vp, c_i64, c_i64, C.c_double, C.c_int32, c_vp, c_vp, c_vp, C.c_size_t, c_vp]),
    "vfm_voxel_robin_workspace_bytes": (C.c_size_t, [c_i64]),
    "vfm_voxel_robin": (C.c_int, [c_vp, c_i64, c_i64, C.c_double, C.c_int32, C.c_uint32, c_i64, c_vp, c_vp, c_vp, c_vp,
                                  C.c_size_t, c_vp]),
    "vfm_voxel_robin_level": (C.c_int, [c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, C.c_double, C.c_uint32, c_vp, c_vp, c_vp, c_vp, c_vp, C.c_size_t, c_vp]),
    "vfm_icp_nearest": (C.c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, C.c_int32, C.c_double, C.c_double, c_vp, c_vp, c_vp]),
    "vfm_icp_grid_workspace_bytes": (C.c_size_t, [c_i64]),
    "vfm_icp_grid_build": (C.c_int, [c_vp, c_i64, C.c_double, C.c_int32, c_vp, c_vp, c_vp, c_vp, c_vp, C.c_size_t, c_vp]),
    "vfm_icp_step_nearest": (C.c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, C.c_int32, C.c_double, C.c_double, c_vp, c_vp, c_vp]),
    "vfm_icp_build_system": (C.c_int, [c_vp, c_vp, c_vp, c_i64, C.c_double, c_vp, c_vp]),
    "vfm_icp_desc_stats": (C.c_int, [c_vp, c_i64, C.c_int32, c_vp, c_vp, c_vp]),
    "vfm_icp_step_nearest_desc": (C.c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, C.c_int32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, C.c_int32,
                                            C.c_double, C.c_double, c_vp, c_vp, c_vp]),
    "vfm_icp_rows_stats": (C.c_int, [c_vp, C.c_int32, c_i64, C.c_int32, c_vp, c_vp, c_vp]),
    "vfm_icp_step_nearest_rows": (C.c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, C.c_int32, C.c_int32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                            C.c_int32, C.c_double, C.c_double, c_vp, c_vp, c_vp]),
    "vfm_range_crop": (C.c_int, [c_vp, c_i64, c_i64, C.c_double, C.c_double, c_vp, c_vp, c_vp]),
    "vfm_deskew_scan": (C.c_int, [c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "vfm_icp_grid_update_workspace_bytes": (C.c_size_t, [C.c_int32, c_i64, c_i64]),
    "vfm_icp_grid_update": (C.c_int, [c_vp, c_vp, c_vp, C.c_int32, c_i64, c_vp, c_i64, c_vp, C.c_double, C.c_int32, c_vp, C.c_double,
                                      c_vp, c_vp, c_vp, c_vp, c_vp, C.c_size_t, c_vp]),
    "vfm_icp_grid_update_src": (C.c_int, [c_vp, c_vp, c_vp, C.c_int32, c_i64, c_vp, c_i64, c_vp, C.c_double, C.c_int32, c_vp, C.c_double,
                                          c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, C.c_size_t, c_vp]),
    "vfm_rows_merge": (C.c_int, [c_vp, c_i64, c_vp, c_i64, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp]),
    "vfm_fpfh_workspace_bytes": (C.c_size_t, [c_i64]),
    "vfm_fpfh_grid_build": (C.c_int, [c_vp, c_i64, C.c_double, c_vp, c_vp, c_vp, C.c_size_t, c_vp]),
    "vfm_fpfh_search_hybrid": (C.c_int, [c_vp, c_i64, c_vp, c_vp, C.c_double, C.c_int32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "vfm_fpfh_normals": (C.c_int, [c_vp, c_i64, c_vp, c_vp, C.c_int32, c_vp, c_vp]),
    "vfm_fpfh_voxel_down_sample": (C.c_int, [c_vp, c_vp, c_i64, C.c_double, c_vp, c_vp, c_vp, c_vp, C.c_size_t, c_vp]),
    "vfm_fpfh_spfh": (C.c_int, [c_vp, c_vp, c_i64, c_vp, c_vp, C.c_int32, c_vp, c_vp]),
    "vfm_fpfh_fpfh": (C.c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, C.c_int32, c_vp, c_vp]),
    "vfm_nn3_workspace_bytes": (C.c_size_t, [c_i64]),
    "vfm_nn3_build": (C.c_int, [c_vp, c_i64, C.c_double, c_vp, c_vp, c_vp, c_vp, C.c_size_t, c_vp]),
    "vfm_nn3_query": (C.c_int, [c_vp, c_vp, c_vp, c_i64, C.c_double, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "vfm_nn3_knn": (C.c_int, [c_vp, c_vp, c_vp, c_i64, C.c_double, c_vp, c_i64, C.c_int, C.c_double, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "vfm_mreach_mst_workspace_bytes": (C.c_size_t, [c_i64]),
    "vfm_mreach_mst": (C.c_int, [c_vp, c_vp, c_vp, c_i64, C.c_double, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, C.c_size_t, c_vp]),
    "vfm_hdbscan_labels_host": (C.c_int, [c_vp, c_vp, c_vp, c_i64, C.c_int, c_vp]),
    "vfm_teaser_graph": (C.c_int, [c_vp, c_vp, c_i64, C.c_double, C.c_double, c_vp, c_vp, c_vp]),
    "vfm_teaser_reduce_workspace_bytes": (C.c_size_t, [c_i64]),
    "vfm_teaser_reduce": (C.c_int, [c_vp, c_vp, c_i64, C.c_int32, c_vp, c_vp, c_vp, C.c_size_t, c_vp]),
    "vfm_teaser_submatrix": (C.c_int, [c_vp, c_i64, c_vp, c_i64, c_vp, c_vp]),
    "vfm_teaser_max_clique_host": (C.c_int, [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, C.POINTER(c_i64)]),
    "vfm_teaser_gnc_workspace_bytes": (C.c_size_t, [c_i64]),
    "vfm_teaser_gnc": (C.c_int, [c_vp, c_vp, c_i64, c_vp, c_i64, C.c_double, C.c_double, C.c_int32, C.c_double, c_vp, c_vp, c_vp, c_vp, c_vp,
                                 C.c_size_t, c_vp]),
    "vfm_teaser_tls_translation_host": (C.c_int, [c_vp, c_i64, C.c_double, c_vp, c_vp]),
    "vfm_pca_moments_workspace_bytes": (C.c_size_t, [C.c_int]),
    "vfm_pca_moments": (C.c_int, [c_vp, C.c_int, c_i64, C.c_int, c_vp, c_vp, c_vp, C.c_size_t, c_vp]),
    "vfm_pca_project_workspace_bytes": (C.c_size_t, []),
    "vfm_pca_project": (C.c_int, [c_vp, C.c_int, c_i64, C.c_int, c_vp, c_vp, C.c_int, c_vp, c_vp, c_vp, c_vp, c_vp, C.c_size_t, c_vp]),
    "vfm_pca_colours": (C.c_int, [c_vp, c_vp, c_i64, C.c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "vfm_colour_gate": (C.c_int, [c_vp, c_i64, c_vp, C.c_int, C.c_double, c_vp, c_vp, c_vp]),
    "vfm_vit_weights_bytes": (C.c_size_t, [C.POINTER(VitConfig)]),
    "vfm_vit_weights_layout": (C.c_int, [C.POINTER(VitConfig), C.POINTER(c_i64), C.POINTER(c_i64), C.c_int]),
    "vfm_vit_workspace_bytes": (C.c_size_t, [C.POINTER(VitConfig), C.c_int]),
    "vfm_vit_forward": (C.c_int, [C.POINTER(VitConfig), c_vp, c_vp, C.c_int, C.c_int, C.c_int, c_vp, c_vp,
                                  C.c_size_t, c_vp]),
}


# include/vfmreg_debug.h: measurement hooks (not part of the drop-in contract)
DEBUG_SIGNATURES = {
    "vfm_prof_events_create": (C.c_int, [C.POINTER(c_vp), C.POINTER(c_vp)]),
    "vfm_prof_arm": (C.c_int, [c_vp, c_vp]),
    "vfm_prof_elapsed_ms": (C.c_int, [c_vp, c_vp, C.POINTER(C.c_float)]),
    "vfm_prof_events_destroy": (C.c_int, [c_vp, c_vp]),
    "vfm_debug_last_coarse_kernel": (C.c_int, [C.c_char_p, C.c_int]),
    "vfm_debug_coarse_kernel_names": (C.c_int, [C.c_char_p, C.c_int]),
    "vfm_debug_search_plan": (C.c_int, [C.c_int, C.c_int, c_i64, c_i64, C.c_int, C.c_char_p, C.c_int]),
    "vfm_debug_coarse_plan": (C.c_int, [C.c_int, C.c_int, c_i64, c_i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]),
    "vfm_debug_prepare_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, c_i64, C.c_int, c_i64, C.c_int, C.c_int, C.c_char_p, C.c_int]),
    "vfm_debug_match_stats": (C.c_int, [c_vp, c_i64, c_i64, c_vp]),
    "vfm_debug_i8_rows": (C.c_int, [c_vp, c_i64, C.c_int, c_vp, c_vp, c_vp, c_vp]),
    "vfm_debug_mx6_rows": (C.c_int, [c_vp, c_i64, C.c_int, c_vp, c_vp, c_vp]),
    "vfm_debug_mx6_half_err": (C.c_int, [c_vp, c_i64, C.c_int, c_vp, c_vp]),
    "vfm_debug_voxel_trace": (C.c_int, [c_vp, c_i64, c_vp]),
    "vfm_debug_ransac_counts": (C.c_int, [c_vp, c_i64, C.c_int, c_vp]),
    "vfm_debug_ransac_state": (C.c_int, [c_vp, c_i64, C.c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "vfm_debug_vit_workspace_layout": (C.c_int, [C.POINTER(VitConfig), C.c_int, C.POINTER(c_i64), C.POINTER(c_i64)]),
    "vfm_debug_vit_plan": (C.c_int, [C.POINTER(VitConfig), C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]),
    "vfm_debug_l2_narrow_slices": (C.c_int, [c_i64, c_i64]),
    "vfm_debug_l2_narrow_evals": (C.c_int, [c_vp, C.POINTER(c_i64)]),
}


def load() -> C.CDLL:
    """Load the HIP library (after torch, so that both share one libamdhip64 runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python vfm-registration_amd/build.py` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    import torch  # noqa: F401  -- loads torch's libamdhip64.so first (same soname => one runtime)
    lib = C.CDLL(str(LIB_PATH))
    for name, (res, args) in list(SIGNATURES.items()) + list(DEBUG_SIGNATURES.items()):
        fn = getattr(lib, name)  # AttributeError => the .so does not export what the header declares
        fn.restype = res
        fn.argtypes = args
    _install_tool_names(lib)
    _lib = lib
    return lib


# ---------------------------------------------------------------------------------------------------------------------------------
# Kernel policy (include/vfmreg.h, vfm_config_*): a caller-owned object bound per THREAD; the library keeps no process-global switches.
# ---------------------------------------------------------------------------------------------------------------------------------
import threading as _threading

_tls = _threading.local()


class Config:
    """A vfm_config_t: factory settings + what ``set`` changed.  ``use()`` binds it to the calling thread (every library call made from
    this thread afterwards reads its policy from it); ``with cfg.bound():`` binds it for a block and restores the previous binding."""

    def __init__(self, **settings):
        h = c_vp()
        check(load().vfm_config_create(C.byref(h)), "config_create")
        self._h = h
        for k, v in settings.items():
            self.set(k, v)

    def set(self, key: str, value: int) -> "Config":
        check(load().vfm_config_set(self._h, key.encode(), int(value)), f"config_set({key})")
        return self

    def get(self, key: str) -> int:
        v = c_i64()
        check(load().vfm_config_get(self._h, key.encode(), C.byref(v)), f"config_get({key})")
        return int(v.value)

    def use(self) -> "Config":
        check(load().vfm_config_use(self._h), "config_use")
        _tls.bound = self
        return self

    def bound(self):
        return using(self)

    def __del__(self):
        try:
            if getattr(_tls, "bound", None) is self:
                _lib.vfm_config_use(None)
                _tls.bound = None
            _lib.vfm_config_destroy(self._h)
        except Exception:
            pass


def current() -> "Config | None":
    """The Config bound to the calling thread (None: factory settings)."""
    return getattr(_tls, "bound", None)


class using:
    """``with using(cfg):`` -- cfg (or None = factory settings) bound to this thread inside the block, the previous binding after it.
    Helper threads that call the library on behalf of a caller bind the caller's ``current()`` this way (vfmreg/vit.py)."""

    def __init__(self, cfg):
        self.cfg = cfg

    def __enter__(self):
        self.prev = current()
        load().vfm_config_use(self.cfg._h if self.cfg is not None else None)
        _tls.bound = self.cfg
        return self.cfg

    def __exit__(self, *exc):
        load().vfm_config_use(self.prev._h if self.prev is not None else None)
        _tls.bound = self.prev
        return False


def policy(key: str) -> int:
    """What the library's entry points would read for ``key`` if called from this thread now (its bound Config, or the factory setting)."""
    v = c_i64()
    check(load().vfm_config_get(None, key.encode(), C.byref(v)), f"config_get({key})")
    return int(v.value)


def thread_config() -> Config:
    """The calling thread's Config, created and bound on first use: what the tools' ``lib.vfm_debug_set_*`` names write to."""
    cfg = current()
    if cfg is None:
        cfg = Config().use()
    return cfg


def _install_tool_names(lib) -> None:
    """Rounds 1 - 5 exported process-global setters (vfm_debug_set_*); ~140 scripts under tools/ and the A/B tests call them as
    ``lib.vfm_debug_set_coarse_variant(43)``.  The library no longer has them: these PYTHON functions of the same names set the calling
    thread's Config (``thread_config()``) -- same effect for a single-threaded script, no effect on any other thread.  (The ViT's code
    table ``vfm_debug_set_vit_gemm`` is gone with its key: the ViT tools set the named ``vit_*`` keys under ``using(Config().set(...))``.)"""
    def setter(key):
        def f(value):
            thread_config().set(key, value)
            return 0
        return f
    lib.vfm_debug_set_coarse_variant = setter("coarse_variant")
    lib.vfm_debug_set_coarse_slices = setter("coarse_slices")
    lib.vfm_debug_set_match_stats = setter("match_stats")
    lib.vfm_debug_set_i8_min_queries = setter("i8_min_queries")
    lib.vfm_debug_set_prep_grid = setter("prep_grid")
    lib.vfm_debug_set_voxel_small = setter("voxel_small")
    lib.vfm_debug_set_ransac_exact_only = setter("ransac_exact_only")


def last_coarse_kernel() -> str:
    """The coarse kernel the calling thread's last search launched (include/vfmreg_debug.h), "" if none."""
    buf = C.create_string_buffer(256)
    check(load().vfm_debug_last_coarse_kernel(buf, len(buf)), "last_coarse_kernel")
    return buf.value.decode()


def coarse_kernel_names() -> list:
    """Every name ``last_coarse_kernel`` can return: one per launcher instantiation in the library, sorted."""
    buf = C.create_string_buffer(1 << 14)
    check(load().vfm_debug_coarse_kernel_names(buf, len(buf)), "coarse_kernel_names")
    return buf.value.decode().split("\n") if buf.value else []


def search_plan(records: int, d: int, n: int, m: int, gated: bool = True) -> dict:
    """What a search of these arguments would do under the calling thread's Config (include/vfmreg_debug.h, vfm_debug_search_plan):
    {"pass": str, "kind": int, "half" / "fused" / "top2" / "pilot" / "bins" / "no_i8": bool, "finish": [kernel names in launch order]}.
    Raises RuntimeError with the library's message where the search itself would refuse.  Touches no device."""
    buf = C.create_string_buffer(1024)
    check(load().vfm_debug_search_plan(records, d, n, m, int(gated), buf, len(buf)), "search_plan")
    plan = dict(item.split("=", 1) for item in buf.value.decode().split(" "))
    out = {k: bool(int(v)) for k, v in plan.items() if k not in ("pass", "kind", "finish")}
    out.update({"pass": plan["pass"], "kind": int(plan["kind"]), "finish": plan["finish"].split(",")})
    return out


def coarse_plan(records: int, d: int, n: int, m: int, gated: bool = True, inner_product: bool = True, row_bias: bool = False,
                compute_units: int = 0) -> dict:
    """The launch of that search's coarse pass (include/vfmreg_debug.h, vfm_debug_coarse_plan; compute_units 0: the current device's):
    {"kernel": the name last_coarse_kernel() reports after it, "nqb", "nslices", "seed", "block", "lds", "tune": int}.  Raises
    RuntimeError with the library's message where the search itself would refuse.  Touches no device."""
    buf = C.create_string_buffer(1024)
    check(load().vfm_debug_coarse_plan(records, d, n, m, int(gated), int(inner_product), int(row_bias), compute_units, buf, len(buf)), "coarse_plan")
    plan = dict(item.split("=", 1) for item in buf.value.decode().split(" "))
    return {k: (v if k == "kernel" else int(v)) for k, v in plan.items()}


def prepare_plan(entry: int, schedule: int, d: int, rows1: int, rows2: int = 0, dtype1: int = 0, dtype2: int = 0, zero: bool = False) -> dict:
    """What a preparation would do under the calling thread's Config (include/vfmreg_debug.h, vfm_debug_prepare_plan; entry: a
    VFM_PREP_ENTRY_* value): {"images": [...], "kernels": [launch order], "grid": str, "zero": "none" | "inside" | "behind"}.
    Raises RuntimeError with the library's message where the entry itself would refuse.  Touches no device."""
    buf = C.create_string_buffer(1024)
    check(load().vfm_debug_prepare_plan(entry, schedule, d, rows1, dtype1, rows2, dtype2, int(zero), buf, len(buf)), "prepare_plan")
    plan = dict(item.split("=", 1) for item in buf.value.decode().split(" "))
    # (template arguments hold commas: a new kernel starts where "prep_" does)
    return {"images": plan["images"].split(","), "kernels": plan["kernels"].replace(",prep_", " prep_").split(" "), "grid": plan["grid"],
            "zero": plan["zero"]}


VIT_STAGES = ("pre", "patch", "qkv", "att", "proj", "fc1", "fc2")


def vit_plan(cfg, B: int, W: int = 1600, compute_units: int = 0) -> dict:
    """What vfm_vit_forward(cfg, B images W pixels wide) would launch under the calling thread's Config (include/vfmreg_debug.h,
    vfm_debug_vit_plan; cfg: a VitConfig; compute_units 0: the current device's): {stage: "<kernel>@<grid>x<block>+<lds bytes>", or None
    where the stage is inside the kernel before it, for each of VIT_STAGES; "launches": int; "trace": the stage whose launch gets
    "vit_trace_buffer", or None}.  Raises RuntimeError with the library's message where the forward itself would refuse.  Touches no device."""
    buf = C.create_string_buffer(1024)
    check(load().vfm_debug_vit_plan(C.byref(cfg), B, W, compute_units, buf, len(buf)), "vit_plan")
    plan = dict(item.split("=", 1) for item in buf.value.decode().split(" "))
    out = {s: (None if plan[s] == "-" else plan[s]) for s in VIT_STAGES}
    out.update({"launches": int(plan["launches"]), "trace": None if plan["trace"] == "none" else plan["trace"]})
    return out


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().vfm_last_error().decode()
        raise RuntimeError(f"libvfmreg_hip {what} failed ({rc}): {msg}")
