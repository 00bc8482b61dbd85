"""Loader for the HIP/C-ABI library (csrc/libgs2m_raster.so, include/gs2m_raster.h).

There is NO CPU or PyTorch fallback: if the shared library is missing or cannot be
loaded, every entry point raises.  The library is built in-tree by `build()` (hipcc,
--offload-arch=gfx950) so that it travels with the repository snapshot.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("GS2M_LIB", os.path.join(CSRC, "libgs2m_raster.so"))  # GS2M_LIB: A/B builds

ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_size_t, C.c_void_p)


class Prealloc(C.Structure):
    """include/gs2m_raster.h: gs2m_prealloc (user block of gs2m_prealloc_alloc)"""
    _fields_ = [("ptr", C.c_void_p), ("capacity", C.c_size_t), ("fallback", ALLOC_FN), ("fallback_user", C.c_void_p),
                ("used_fallback", C.c_int), ("requested", C.c_size_t)]


class Layout(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "geom_bytes", "rec", "tiles_touched", "depth_key", "rect", "gauss_rows", "clamped", "wave_rowbase", "counters",
        "binning_bytes", "point_list", "tile_keys", "qlist", "qrow",
        "image_bytes", "final_T", "n_contrib", "ranges", "qcount")]


class STREAM(C.c_void_p):
    """`void* stream` as an entry point's LAST parameter: the function enqueues GPU work (call it through `launch`)."""


# Every exported function: name -> (restype, argtypes), header by header in the headers' order of declaration.
# tests/test_cabi.py compares each entry with the prototype in include/.
p, i, f, d, ll, ull, A, s = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_longlong, C.c_ulonglong, ALLOC_FN, STREAM
SIGNATURES = {
    # include/gs2m_raster.h
    "gs2m_raster_forward": (i, [A, p, A, p, A, p, i, i, i, p, i, i, p, p, p, p, p, f, p, p, p, p, p, p, f, f, i, i, p,
                                p, p, p, s]),
    "gs2m_raster_backward": (i, [i, i, i, i, p, i, i, p, p, p, p, f, p, p, p, p, p, p, f, f, p, p, p, p, p, i, p, p, p,
                                 p, p, p, p, p, p, p, p, p, A, p, s]),
    "gs2m_raster_mark_visible": (i, [i, p, p, p, p, s]),
    "gs2m_knn_dist2": (i, [i, p, p, A, p, s]),
    "gs2m_debug_layout": (i, [i, i, i, i, C.POINTER(Layout)]),
    "gs2m_set_reference_binning": (i, [i]),
    "gs2m_raster_forward_split_sh": (i, [A, p, A, p, A, p, i, i, i, p, i, i, p, p, p, p, p, p, f, p, p, p, p, p, p, f,
                                         f, i, i, p, p, p, p, s]),
    "gs2m_raster_backward_split_sh": (i, [i, i, i, i, p, i, i, p, p, p, p, p, f, p, p, p, p, p, p, f, f, p, p, p, p, p,
                                          i, p, p, p, p, p, p, p, p, p, p, p, p, p, A, p, s]),
    "gs2m_pack_features_forward": (i, [i, p, p, p, p, p, p, p, p, i, i, p, s]),
    "gs2m_pack_features_backward": (i, [i, p, p, p, p, p, i, i, p, p, p, p, p, p, s]),
    "gs2m_gbuffer_post_forward": (i, [i, i, p, p, p, i, p, p, p, s]),
    "gs2m_gbuffer_post_backward": (i, [i, i, p, p, p, i, p, p, p, s]),
    "gs2m_gbuffer_maps_backward": (i, [i, i, p, p, p, i, p, p, p, p, p, p, p, p, p, s]),
    "gs2m_sobel_normal_forward": (i, [i, i, p, p, p, p, f, f, f, f, p, s]),
    "gs2m_sobel_normal_backward": (i, [i, i, p, p, p, p, f, f, f, f, p, p, p, s]),
    "gs2m_activate_forward": (i, [i, p, p, p, p, p, p, p, p, p, p, p, p, s]),
    "gs2m_activate_backward": (i, [i, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, s]),
    "gs2m_set_spin_wait": (i, [i]),
    "gs2m_set_sort_tickets": (i, [i]),
    "gs2m_set_tile_sort_policy": (i, [i]),
    "gs2m_prealloc_alloc": (p, [C.c_size_t, p]),  # a ready-made ALLOC_FN: only ever cast to that type
    "gs2m_set_debug": (i, [i]),
    "gs2m_set_markers": (i, [i]),
    "gs2m_stage_name": (C.c_char_p, [i]),
    "gs2m_raster_forward_token": (ull, []),
    "gs2m_raster_dense_rows": (ll, [ull]),
    "gs2m_raster_backward_rows_hint": (i, [ll]),
    "gs2m_debug_tile_sort": (i, [i, p, p, p, p, p, p, p, p, p, p, s]),
    "gs2m_debug_radix_temp_bytes": (i, [ll, i, C.POINTER(ull)]),
    "gs2m_debug_radix_plan": (i, [i, C.POINTER(i), C.POINTER(i), C.POINTER(i)]),
    "gs2m_debug_radix_sort": (i, [ll, i, p, p, p, p, p, p, p, ull, i, p, p, s]),
    "gs2m_debug_block_scans": (i, [ll, p, p, p, p, ll, p, p, p, p, s]),
    "gs2m_debug_emit": (i, [i, i, i, i, i, i, i, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, s]),
    "gs2m_debug_preprocess": (i, [i, i, i, p, p, f, p, p, p, p, p, p, p, p, p, p, i, i, f, f, i, p, p, p, p, p, p, p, p, p, p, p, ull, s]),
    "gs2m_debug_blend_forward": (i, [i, i, i, p, p, p, p, p, p, p, p, p, p, p, s]),
    "gs2m_debug_blend_backward": (i, [i, i, i, p, p, p, p, p, p, p, p, p, p, p, p, s]),
    "gs2m_debug_gaussian_bwd": (i, [i, i, i, p, p, p, p, p, f, p, p, p, p, p, i, i, f, f, p, i, p, p, p, p, p, p, p, p, p, i, ll, i, p, p, p, p, p, p,
                                    p, p, p, p, p, s]),
    "gs2m_debug_row_floats": (i, [i]),
    "gs2m_profile_mode": (i, [i]),
    "gs2m_profile_sampling": (i, [i]),
    "gs2m_profile_collect": (i, [C.POINTER(C.c_float), C.POINTER(C.c_int), i]),
    "gs2m_version": (C.c_char_p, []),
    # include/gs2m_texture.h
    "gs2m_texture_cube_forward": (i, [i, i, i, p, p, p, p, p, s]),
    "gs2m_texture_cube_backward": (i, [i, i, i, p, p, p, p, p, i, s]),
    "gs2m_texture_2d_clamp_forward": (i, [i, i, i, i, p, p, p, s]),
    "gs2m_texture_2d_clamp_backward": (i, [i, i, i, i, p, p, p, s]),
    # include/gs2m_cubemap.h
    "gs2m_diffuse_cubemap_forward": (i, [i, p, p, s]),
    "gs2m_diffuse_cubemap_backward": (i, [i, p, p, s]),
    "gs2m_cubemap_texel_table": (i, [i, p, s]),
    "gs2m_specular_cubemap_forward": (i, [i, f, f, p, p, p, s]),
    "gs2m_specular_cubemap_backward": (i, [i, f, f, p, p, p, s]),
    "gs2m_specular_cubemap_route": (i, [i, f, i]),
    "gs2m_specular_cubemap_normalized_forward": (i, [i, f, f, p, p, p, p, s]),
    "gs2m_specular_cubemap_normalized_backward": (i, [i, f, f, p, p, p, p, p, s]),
    # include/gs2m_pbr.h
    "gs2m_pbr_shade_forward": (i, [i, p, p, p, p, p, p, i, i, p, i, i, p, p, f, f, p, p, p, p, s]),
    "gs2m_pbr_shade_backward": (i, [i, p, p, p, p, p, p, i, i, p, i, i, p, p, f, f, p, p, p, p, p, i, s]),
    "gs2m_pbr_inputs_forward": (i, [i, i, p, p, p, p, p, f, f, p, p, p, p, s]),
    "gs2m_pbr_inputs_backward": (i, [i, i, p, p, p, s]),
    # include/gs2m_mvs.h
    "gs2m_patch_ncc_forward": (i, [i, p, p, p, p, p, i, i, p, p, p, f, i, p, s]),
    "gs2m_patch_ncc_backward": (i, [i, p, p, p, p, p, i, i, p, p, p, f, i, p, p, p, s]),
    "gs2m_patch_ncc_roughness": (i, [i, p, p, p, p, p, i, i, p, p, p, f, i, p, p, p, s]),
    "gs2m_mvs_set_deterministic": (None, [i]),
    "gs2m_mvs_get_deterministic": (i, []),
    "gs2m_grid_sample_border_forward": (i, [i, i, i, i, p, p, p, s]),
    "gs2m_grid_sample_border_backward": (i, [i, i, i, i, p, p, p, p, p, s]),
    "gs2m_mv_geo_forward": (i, [i, i, i, i, p, p, p, p, p, p, p, p, p, p, f, p, p, p, s]),
    "gs2m_mv_geo_backward": (i, [i, i, i, i, p, p, p, p, p, p, p, p, p, p, f, p, p, p, p, p, p, s]),
    # include/gs2m_optim.h
    "gs2m_adam_step": (i, [i, p, d, d, d, s]),
    # include/gs2m_ssim.h
    "gs2m_ssim_forward": (i, [i, i, i, i, f, f, p, p, p, p, p, p, s]),
    "gs2m_ssim_backward": (i, [i, i, i, i, p, p, p, p, p, p, p, s]),
    "gs2m_ssim_backward_uniform": (i, [i, i, i, i, p, p, p, f, f, p, p, p, p, s]),
    "gs2m_ssim_strip_rows": (i, [i, i, i, i]),
    # include/gs2m_loss.h
    "gs2m_loss_workspace_bytes": (i, []),
    "gs2m_edge_gradient": (i, [i, i, p, p, p, p, s]),
    "gs2m_image_loss_forward": (i, [i, i, p, i, p, p, p, p, p, p, p, p, f, f, p, p, p, s]),
    "gs2m_image_loss_backward": (i, [i, i, p, i, p, p, p, p, p, p, p, f, f, p, p, p, p, p, s]),
    "gs2m_tv_loss_forward": (i, [i, i, i, p, p, p, i, f, p, p, s]),
    "gs2m_tv_loss_backward": (i, [i, i, i, p, p, p, i, f, p, p, s]),
    "gs2m_mv_geo_loss_forward": (i, [i, p, p, p, f, f, f, f, p, p, p, p, s]),
    "gs2m_mv_geo_loss_backward": (i, [i, p, p, p, f, f, f, f, p, p, p, p, s]),
    "gs2m_mv_take_forward": (i, [i, p, i, i, p, p, p, p, p, p, p, s]),
    "gs2m_mv_take_backward": (i, [i, p, i, i, p, p, p, p, s]),
    "gs2m_ncc_tail_forward": (i, [i, p, p, p, p, s]),
    "gs2m_ncc_tail_backward": (i, [i, p, p, p, p, p, s]),
    "gs2m_subset_thin": (i, [i, p, i, ull, p, i, p, p, s]),
    "gs2m_subset_remove": (i, [i, i, ull, p, p, s]),
    "gs2m_affine_mean": (i, [ll, p, f, f, p, p, s]),
    "gs2m_plane_loss_forward": (i, [i, p, i, p, f, p, p, s]),
    "gs2m_plane_loss_backward": (i, [i, p, i, p, f, p, p, p, s]),
    "gs2m_densification_stats": (i, [i, p, p, p, p, p, p, p, p, s]),
    # include/gs2m_mesh.h
    "gs2m_tsdf_workspace_bytes": (i, [p, i, p, p]),
    "gs2m_tsdf_points_aabb": (i, [i, i, p, f, f, f, f, f, p, p, s]),
    "gs2m_tsdf_touch": (i, [p, f, f, i, i, p, f, f, f, f, f, p, i, p, p, p, p, p, p, s]),
    "gs2m_tsdf_integrate": (i, [f, f, i, i, p, p, f, f, f, f, f, p, i, p, p, p, p, p, s]),
    "gs2m_tsdf_mesh_count": (i, [p, i, p, p, p, p, p, p, s]),
    "gs2m_tsdf_mesh_emit": (i, [p, f, i, p, p, p, p, p, ll, ll, p, p, p, s]),
    "gs2m_tsdf_block_coords": (i, [i, p, p, s]),
    "gs2m_mesh_post_workspace_bytes": (i, [ll, ll, p, p]),
    "gs2m_mesh_cluster_triangles": (i, [ll, ll, p, p, p, p, p, s]),
    "gs2m_mesh_keep_clusters": (i, [ll, p, p, i, p, s]),
    "gs2m_mesh_compact": (i, [ll, ll, p, p, p, p, p, p, p, p, p, s]),
    # include/gs2m_simplify.h
    "gs2m_simplify_workspace_bytes": (i, [ll, ll, i, p]),
    "gs2m_simplify_count": (i, [ll, ll, p, p, d, p, p, s]),
    "gs2m_simplify": (i, [ll, ll, p, p, i, p, p, d, p, p, p, p, p, p, p, s]),
    "gs2m_simplify_set_timing": (i, [i]),
    "gs2m_simplify_stage_ms": (i, [p]),
    # include/gs2m_eval.h
    "gs2m_eval_transform": (i, [ll, p, d, p, p, s]),
    "gs2m_eval_sample_workspace_bytes": (i, [ll, ll, p, p]),
    "gs2m_eval_sample_rows": (i, [ll, p, ll, p, d, p, p, s]),
    "gs2m_eval_sample_count": (i, [ll, ll, p, p, p, s]),
    "gs2m_eval_sample_emit": (i, [ll, p, ll, p, ll, p, p, ll, p, s]),
    "gs2m_eval_gather": (i, [ll, p, p, p, s]),
    "gs2m_eval_grid_bytes": (i, [ll, p, p]),
    "gs2m_eval_grid_build": (i, [ll, p, d, p, p, s]),
    "gs2m_eval_thin_workspace_bytes": (i, [ll, p]),
    "gs2m_eval_thin": (i, [ll, p, p, d, p, p, p, s]),
    "gs2m_eval_filter": (i, [ll, p, p, p, p, d, p, p, p, s]),
    "gs2m_eval_above_plane": (i, [ll, p, p, p, s]),
    "gs2m_eval_scan_workspace_bytes": (i, [ll, p]),
    "gs2m_eval_compact": (i, [ll, p, p, i, p, p, p, s]),
    "gs2m_eval_nearest": (i, [ll, p, ll, d, p, d, p, s]),
    "gs2m_eval_nearest_index": (i, [ll, p, ll, d, p, d, p, p, s]),
    "gs2m_eval_masked_mean": (i, [ll, p, d, p, p, p, s]),
    "gs2m_eval_dilate_bytes": (i, [i, i, i, p]),
    "gs2m_eval_dilate_disk": (i, [i, i, i, p, i, p, s]),
    "gs2m_eval_cull_flags": (i, [ll, p, i, p, i, i, p, i, i, p, s]),
    "gs2m_eval_cull_workspace_bytes": (i, [ll, ll, p]),
    "gs2m_eval_cull_triangles": (i, [ll, p, ll, p, p, p, p, s]),
    # include/gs2m_tnt.h
    "gs2m_tnt_mesh_points": (i, [ll, p, ll, p, p, p, s]),
    "gs2m_tnt_transform": (i, [ll, p, p, p, s]),
    "gs2m_tnt_crop_flags": (i, [ll, p, i, d, d, i, p, p, s]),
    "gs2m_tnt_voxel_workspace_bytes": (i, [ll, p]),
    "gs2m_tnt_voxel_downsample": (i, [ll, p, d, p, p, p, s]),
    "gs2m_tnt_stride_gather": (i, [ll, p, ll, p, s]),
    "gs2m_tnt_icp_workspace_bytes": (i, [p]),
    "gs2m_tnt_icp_moments": (i, [ll, p, ll, p, p, p, p, p, s]),
    "gs2m_tnt_histogram": (i, [ll, p, i, p, p, s]),
    "gs2m_tnt_knn_normals_workspace_bytes": (i, [ll, p]),
    "gs2m_tnt_knn_normals": (i, [ll, p, d, p, i, p, p, p, s]),
    "gs2m_tnt_distance_colors": (i, [ll, p, d, p, p, s]),
    # include/gs2m_metrics.h
    "gs2m_image_metrics_workspace_bytes": (i, [i, i, i, i, p]),
    "gs2m_image_metrics": (i, [i, i, i, i, p, p, p, ll, p, p, s]),
    # include/gs2m_maps.h
    "gs2m_order_stats_workspace_bytes": (i, [ll, i, p]),
    "gs2m_order_stats": (i, [ll, p, i, p, p, ll, p, p, s]),
    "gs2m_depth_colorize": (i, [i, i, p, p, f, f, p, s]),
    "gs2m_pack_image": (i, [i, i, i, i, p, p, p, p, p, i, i, p, s]),
    # include/gs2m_visibility.h
    "gs2m_meshdepth_workspace_bytes": (i, [ll, i, p]),
    "gs2m_meshdepth_render": (i, [ll, p, ll, p, i, p, d, d, d, d, i, i, d, d, p, p, s]),
    "gs2m_visibility_votes": (i, [ll, p, i, p, d, d, d, d, i, i, p, d, i, p, s]),
    "gs2m_visibility_keep": (i, [ll, p, i, p, s]),
    "gs2m_visibility_referenced": (i, [ll, p, ll, p, p, s]),
    # include/gs2m_ingest.h
    "gs2m_resize_plan_bytes": (i, [i, i, p, p]),
    "gs2m_resize_plan": (i, [i, i, p]),
    "gs2m_image_max_u8": (i, [ll, p, p, s]),
    "gs2m_image_mask_u8": (i, [i, i, p, p, p, p, s]),
    "gs2m_image_resize_workspace_bytes": (i, [i, i, i, i, i, p]),
    "gs2m_image_resize_u8": (i, [i, i, i, p, i, i, p, p, p, p, s]),
    "gs2m_image_unpack": (i, [i, i, i, p, p, p, p, p, p, s]),
    # include/gs2m_meshview.h
    "gs2m_meshview_workspace_bytes": (i, [ll, i, p]),
    "gs2m_meshview_visibility": (i, [ll, p, ll, p, i, p, d, d, d, d, i, i, i, d, d, p, p, s]),
    "gs2m_meshview_normals_workspace_bytes": (i, [p]),
    "gs2m_meshview_normals": (i, [ll, p, ll, p, p, p, p, s]),
    "gs2m_meshview_shade": (i, [ll, p, ll, p, i, p, d, d, d, d, i, i, i, p, p, p, d, d, d, d, d, i, p, p, p, s]),
    "gs2m_meshview_gbuffer": (i, [ll, p, ll, p, i, p, d, d, d, d, i, i, i, p, p, p, p, p, p, p, p, p, p, p, s]),
    "gs2m_meshview_gbuffer_textured": (i, [ll, p, ll, p, p, i, p, d, d, d, d, i, i, i, p, p, i, i, p, i, p, p, p, p, p, p, p, p, s]),
    "gs2m_meshview_resolve_rgb": (i, [i, i, i, i, p, p, i, p, p, s]),
    # include/gs2m_meshbake.h
    "gs2m_meshbake_accumulate": (i, [ll, p, p, i, p, d, d, d, d, i, i, p, i, p, p, d, i, p, p, s]),
    "gs2m_meshbake_resolve": (i, [ll, i, p, p, d, p, p, p, s]),
    "gs2m_texbake_accumulate": (i, [ll, p, p, p, i, p, d, d, d, d, i, i, p, i, p, p, d, i, p, p, s]),
    "gs2m_texbake_resolve": (i, [ll, i, i, i, p, p, d, p, p, ll, p, p, ll, p, p, p, s]),
    "gs2m_texture_pack": (i, [ll, i, p, i, p, p, s]),
    "gs2m_texture_normals": (i, [ll, p, p, ll, p, p, ll, p, i, i, p, p, p, s]),
    # include/gs2m_meshao.h
    "gs2m_bvh_bytes": (i, [ll, p]),
    "gs2m_bvh_build": (i, [ll, p, ll, p, p, ll, s]),
    "gs2m_bvh_occluded": (i, [p, ll, ll, p, ll, p, ll, p, p, d, d, p, p, s]),
    "gs2m_bvh_closest": (i, [p, ll, ll, p, ll, p, ll, p, p, d, d, p, i, p, p, p, s]),
    "gs2m_bvh_ao": (i, [p, ll, ll, p, ll, p, ll, p, p, p, i, i, p, d, d, ll, ll, p, s]),
    "gs2m_texture_occlusion": (i, [ll, p, p, i, p, s]),
    # include/gs2m_meshtransfer.h
    "gs2m_mesh_transfer": (i, [p, ll, ll, p, ll, p, ll, p, p, p, d, i, i, p, p, i, i, p, p, p, s]),
    # include/gs2m_atlas.h
    "gs2m_atlas_workspace_bytes": (i, [ll, p]),
    "gs2m_atlas_count": (i, [ll, ll, p, p, d, p, p, p, s]),
    "gs2m_atlas_build": (i, [ll, ll, p, p, d, p, p, p, p, p, p, p, s]),
    "gs2m_atlas_texels": (i, [ll, p, p, ll, p, p, p, i, i, i, i, p, p, p, p, s]),
    # include/gs2m_png.h
    "gs2m_png_plan": (i, [i, i, i, i, p, p, p, p]),
    "gs2m_png_filter": (i, [i, i, i, i, p, p, s]),
    "gs2m_png_encode": (i, [i, i, i, i, p, p, ll, p, ll, p, s]),
    # include/gs2m_lpips.h
    "gs2m_lpips_pack_conv": (i, [i, i, p, p, p, s]),
    "gs2m_lpips_pack_weights": (i, [p, p, p, p, s]),
    "gs2m_lpips_workspace_bytes": (i, [i, i, i, p]),
    "gs2m_lpips": (i, [i, i, i, p, p, p, p, ll, p, p, s]),
    "gs2m_lpips_conv3x3": (i, [i, i, i, i, i, p, p, p, s]),
    "gs2m_lpips_maxpool2x2": (i, [i, i, i, i, p, p, s]),
    "gs2m_lpips_tap_workspace_bytes": (i, [i, i, i, p]),
    "gs2m_lpips_tap_distance": (i, [i, i, i, i, p, p, p, p, ll, p, s]),
    # include/gs2m_envmap.h
    "gs2m_hdr_scan": (i, [p, ll, i, i, p]),
    "gs2m_hdr_decode": (i, [p, ll, i, i, p, p, s]),
    "gs2m_hdr_encode": (i, [i, i, p, p, s]),
    "gs2m_latlong_to_cubemap": (i, [i, i, p, i, i, f, f, p, s]),
    # include/gs2m_undistort.h
    "gs2m_undistort_camera": (i, [i, i, i, p, d, d, d, p, p, p]),
    "gs2m_undistort_images_u8": (i, [i, p, i, i, i, i, p, p, i, i, p, p, s]),
    "gs2m_undistort_points": (i, [ll, p, i, p, p, p, p, s]),
}
del p, i, f, d, ll, ull, A, s
EXPORTS = tuple(SIGNATURES)

STAGES = ("preprocess", "unused1", "scan", "emit", "tile_sort", "lists", "blend_fwd", "unused7", "blend_bwd",
          "gaussian_bwd")

_lib = None


def build(jobs=8, force=False):
    """Compile every HIP translation unit for gfx950 and link libgs2m_raster.so."""
    cmd = ["make", "-C", CSRC, "-j", str(jobs)]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"gs2m: HIP extension not built: {LIB_PATH} is missing. Run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (needs hipcc, --offload-arch=gfx950). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


ERRORS = {-1: "invalid argument", -2: "HIP runtime error", -3: "scratch allocation failed", -4: "unsupported size",
          -5: "Point culled! This point should have been prefiltered (prefiltered=True and a Gaussian has view z <= 0.2; the reference traps the device here, cuda_rasterizer/auxiliary.h:155-158)"}


class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def device_guard(device):
    """`with torch.cuda.device(device)` without its cost when `device` is already the current one (every call of every
    wrapper: ~10 us of host time each, 0.2 ms per training iteration)."""
    import torch
    idx = device.index if hasattr(device, "index") else device
    if idx is None or idx == torch.cuda.current_device():
        return _NO_GUARD
    return torch.cuda.device(device)


def stream_ptr(device=None):
    """The raw hipStream_t of torch's current stream on `device` (the current device when None) as an int -- one C call
    instead of building a torch.cuda.Stream object per launch."""
    import torch
    idx = None if device is None else (device.index if hasattr(device, "index") else device)
    if idx is None:
        idx = torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(idx)


def check(rc, what):
    if rc <= -100:  # debug mode: GS2M_ERR_STAGE(stage)
        raise RuntimeError(f"gs2m: {what} failed in stage `{lib().gs2m_stage_name(-100 - rc).decode()}` (debug mode)")
    if rc < 0:
        raise RuntimeError(f"gs2m: {what} failed: {ERRORS.get(rc, rc)}")
    return rc


def launch(name, device, *args):
    """Call the entry point `name` -- one whose last parameter is the stream, i.e. one that enqueues GPU work -- with `args`
    and torch's current stream on `device`, under `device_guard(device)`; a failure is raised under that name."""
    fn = getattr(lib(), name)
    if fn.argtypes[-1] is not STREAM:
        raise TypeError(f"gs2m: {name} takes no stream: call it as check(lib().{name}(...), ...)")
    with device_guard(device):
        return check(fn(*args, stream_ptr(device)), name)


def ptr(t):
    """Device address of tensor `t`; None (NULL) for None and for an empty tensor, the reference's 'missing optional'."""
    return None if t is None or t.numel() == 0 else t.data_ptr()


def f32(t, name, shape=None, *, who, optional=False):
    """`t` made contiguous, after checking that it is a float32 tensor on a HIP device (of `shape`, when given); the
    RuntimeError starts with the wrapper's name `who`.  `optional`: None and empty tensors pass through as they are."""
    import torch
    if optional and (t is None or t.numel() == 0):
        return t
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{who}: `{name}` must be a CUDA tensor on a HIP device; there is no CPU path")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{who}: `{name}` must be float32, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{who}: `{name}` must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.contiguous()


def set_debug(on):
    """1: synchronize and check the stream after every pipeline stage; a fault is raised naming the stage."""
    check(lib().gs2m_set_debug(int(bool(on))), "gs2m_set_debug")


def set_markers(on):
    """1: roctx ranges around the pipeline stages (rocprofv3 --marker-trace)."""
    check(lib().gs2m_set_markers(int(bool(on))), "gs2m_set_markers")


def reset_modes():
    """Every process-wide switch back to its default (tests/conftest.py calls this after each test)."""
    L = lib()
    L.gs2m_set_reference_binning(0); L.gs2m_set_spin_wait(1); L.gs2m_set_debug(0); L.gs2m_set_sort_tickets(0); L.gs2m_set_tile_sort_policy(0)
    L.gs2m_set_markers(0); L.gs2m_profile_mode(0)


def debug_layout(P, R, W, H):
    lay = Layout()
    check(lib().gs2m_debug_layout(P, R, W, H, C.byref(lay)), "gs2m_debug_layout")
    return lay


def set_sort_tickets(on):
    """True: the tile sort takes its tile ids from an atomic ticket (other kernels -- RCCL's -- may be resident on the device)."""
    check(lib().gs2m_set_sort_tickets(int(bool(on))), "gs2m_set_sort_tickets")


def set_tile_sort_policy(policy):
    """0: by tile count (default); 1: a workgroup per tile; 2: a wave per tile (spans of up to 1024 entries); 3: a wave per tile, the
    spans of 513 .. 1024 entries left to the workgroup kernel that takes the longer ones (0 and 2 choose that by themselves in a frame
    whose average span is at most 400 entries)."""
    check(lib().gs2m_set_tile_sort_policy(int(policy)), "gs2m_set_tile_sort_policy")


def set_spin_wait(on):
    """Forward: poll the pinned num_rendered (default) or sleep in hipStreamSynchronize."""
    check(lib().gs2m_set_spin_wait(int(bool(on))), "gs2m_set_spin_wait")


def profile_mode(mode, every=1):
    """0 off, 1 blend kernels only, 2 every stage, 3 backward blend only (HIP events on the launch stream); `every`: mode 3
    brackets every `every`-th launch (an event pair leaves ~12 us of bubble around the kernel)."""
    check(lib().gs2m_profile_sampling(int(every)), "gs2m_profile_sampling")
    check(lib().gs2m_profile_mode(int(mode)), "gs2m_profile_mode")


def profile_collect():
    """-> {stage: (total_ms, launches)} since the last collect."""
    n = len(STAGES)
    ms = (C.c_float * n)()
    cnt = (C.c_int * n)()
    check(lib().gs2m_profile_collect(ms, cnt, n), "gs2m_profile_collect")
    return {STAGES[k]: (float(ms[k]), int(cnt[k])) for k in range(n)}


def set_reference_binning(on):
    """True: emit exactly the reference's tile rectangles (bit-identical sorted lists, for the parity tests
    of the integer artefacts); False (default): drop tiles the alpha >= 1/255 ellipse cannot reach."""
    check(lib().gs2m_set_reference_binning(1 if on else 0), "gs2m_set_reference_binning")
