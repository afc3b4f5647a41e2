"""ctypes binding of libptcore.so (include/ptcore.h).

The library is the product; there is no Python or CPU fallback.  Importing this module fails loudly
when the shared object has not been built (``__graft_entry__.build()`` or ``make -C csrc``).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PTCORE_LIB: development hook for A/B runs of differently compiled libraries (tools/ab.py); always a libptcore build
LIB_PATH = os.environ.get("PTCORE_LIB") or os.path.join(_HERE, "libptcore.so")

PTC_MAX_BOUNCES_CAP = 64

PTC_OK = 0
PTC_ERR_INVALID = -1
PTC_ERR_NO_DEVICE = -2
PTC_ERR_HIP = -3
PTC_ERR_OOM = -4
PTC_ERR_BVH = -5
PTC_ERR_STACK = -6
PTC_ERR_NO_SCENE = -7

METHOD_MEGAKERNEL = 0
METHOD_STREAMING = 1

DISPLAY_FINAL, DISPLAY_COLOR, DISPLAY_NORMAL, DISPLAY_DEPTH = 0, 1, 2, 3
BUF_COLOR, BUF_NORMAL, BUF_DEPTH, BUF_FINAL = 0, 1, 2, 3
CURVE_CLAMP, CURVE_REINHARD, CURVE_ACES = 0, 1, 2


class ptc_object(C.Structure):
    _fields_ = [("type", C.c_uint32), ("index", C.c_uint32), ("m", C.c_float * 16), ("inv_m", C.c_float * 16),
                ("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3)]


class ptc_sphere(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("radius", C.c_float)]


class ptc_material(C.Structure):
    _fields_ = [("type", C.c_int32), ("p", C.c_float * 4)]


class ptc_bvh_node(C.Structure):
    _fields_ = [("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3),
                ("first_child_or_primitive", C.c_uint32), ("primitive_count", C.c_uint32)]


class ptc_mesh_range(C.Structure):
    _fields_ = [("first_vertex", C.c_uint32), ("vertex_count", C.c_uint32), ("first_index", C.c_uint32),
                ("index_count", C.c_uint32), ("first_bvh_node", C.c_uint32), ("bvh_node_count", C.c_uint32)]


class ptc_scene_desc(C.Structure):
    _fields_ = [("objects", C.POINTER(ptc_object)), ("object_count", C.c_uint32),
                ("object_material_indices", C.POINTER(C.c_uint32)),
                ("spheres", C.POINTER(ptc_sphere)), ("sphere_count", C.c_uint32),
                ("materials", C.POINTER(ptc_material)), ("material_count", C.c_uint32),
                ("positions", C.POINTER(C.c_float)), ("vertex_count", C.c_uint32),
                ("indices", C.POINTER(C.c_uint32)), ("index_count", C.c_uint32),
                ("bvh", C.POINTER(ptc_bvh_node)), ("bvh_node_count", C.c_uint32),
                ("meshes", C.POINTER(ptc_mesh_range)), ("mesh_count", C.c_uint32)]


class ptc_camera(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("rotation_wxyz", C.c_float * 4), ("vfov", C.c_float)]


class ptc_denoiser_params(C.Structure):
    _fields_ = [("filter_size", C.c_int32), ("color_weight", C.c_float), ("normal_weight", C.c_float),
                ("position_weight", C.c_float)]


class ptc_band_handle(C.Structure):
    _fields_ = [("ipc_mem", C.c_uint8 * 64), ("pix_count", C.c_uint32), ("pix_begin", C.c_uint32), ("width", C.c_uint32),
                ("rank", C.c_uint32), ("nranks", C.c_uint32), ("block_rows", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class ptc_config(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_bounces", C.c_int32), ("method", C.c_int32), ("reserved", C.c_int32)]


class ptc_stats(C.Structure):
    _fields_ = [("rays_total", C.c_uint64), ("frames", C.c_uint64), ("last_live", C.c_uint32 * PTC_MAX_BOUNCES_CAP),
                ("bvh_node_count", C.c_uint32), ("bvh_max_depth", C.c_uint32), ("triangle_count", C.c_uint32),
                ("stack_capacity", C.c_uint32)]


class ptc_profile(C.Structure):
    _fields_ = [("paths", C.c_uint64 * PTC_MAX_BOUNCES_CAP), ("box_tests", C.c_uint64 * PTC_MAX_BOUNCES_CAP),
                ("tri_tests", C.c_uint64 * PTC_MAX_BOUNCES_CAP), ("trace_ms", C.c_double * PTC_MAX_BOUNCES_CAP),
                ("trace_launches", C.c_uint32 * PTC_MAX_BOUNCES_CAP), ("max_box_tests", C.c_uint32 * PTC_MAX_BOUNCES_CAP),
                ("listed_rays", C.c_uint64 * PTC_MAX_BOUNCES_CAP),
                ("slow_rays", C.c_uint64 * PTC_MAX_BOUNCES_CAP),
                ("node_visits", C.c_uint64 * PTC_MAX_BOUNCES_CAP), ("denoise_ms", C.c_double),
                ("denoise_passes", C.c_uint32), ("persist_launches", C.c_uint32)]


class ptc_occlusion_stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("occluded", C.c_uint64), ("redone", C.c_uint64), ("kernel_ms", C.c_double),
                ("launches", C.c_uint32)]


class ptc_light(C.Structure):
    _fields_ = [("p0", C.c_float * 3), ("e1", C.c_float * 3), ("e2", C.c_float * 3), ("n", C.c_float * 3), ("cdf", C.c_float),
                ("inv_pdf", C.c_float), ("object", C.c_uint32), ("kind_material", C.c_uint32)]


class ptc_light_info(C.Structure):
    _fields_ = [("lights", C.c_uint32), ("sphere_lights", C.c_uint32), ("triangle_lights", C.c_uint32),
                ("emissive_objects", C.c_uint32), ("total_area", C.c_double), ("total_weight", C.c_double)]


class ptc_direct_stats(C.Structure):
    _fields_ = [("points", C.c_uint64), ("sampled", C.c_uint64), ("unoccluded", C.c_uint64), ("kernel_ms", C.c_double),
                ("launches", C.c_uint32)]


class ptc_direct_loop_stats(C.Structure):
    _fields_ = [("diffuse_hits", C.c_uint64), ("shadow_rays", C.c_uint64), ("unoccluded", C.c_uint64)]


class ptc_environment_light_loop_stats(C.Structure):
    _fields_ = [("diffuse_hits", C.c_uint64), ("shadow_rays", C.c_uint64), ("unoccluded", C.c_uint64)]


class ptc_mis_loop_stats(C.Structure):
    _fields_ = [("weighted_emitter_hits", C.c_uint64), ("weighted_misses", C.c_uint64)]


class ptc_smooth_loop_stats(C.Structure):
    _fields_ = [("shading_normals", C.c_uint64), ("fallbacks", C.c_uint64), ("absorbed", C.c_uint64), ("culled_light_samples", C.c_uint64)]


class ptc_texture_loop_stats(C.Structure):
    _fields_ = [("lookups", C.c_uint64), ("fallbacks", C.c_uint64)]


class ptc_denoise_albedo_stats(C.Structure):
    _fields_ = [("pixels", C.c_uint64), ("surface_hits", C.c_uint64), ("texel_lookups", C.c_uint64), ("floored", C.c_uint64),
                ("stage_ms", C.c_double)]


class ptc_denoise_variance_stats(C.Structure):
    _fields_ = [("pixels", C.c_uint64), ("floored", C.c_uint64), ("stage_ms", C.c_double)]


class ptc_normal_map_loop_stats(C.Structure):
    _fields_ = [("bent", C.c_uint64), ("kept", C.c_uint64)]


class ptc_texture_desc(C.Structure):
    _fields_ = [("rgba8", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("encoding", C.c_uint32), ("filter", C.c_uint32),
                ("wrap", C.c_uint32)]


ptc_environment_light_stats = ptc_direct_stats  # the same five fields (include/ptcore.h)


class ptc_display_params(C.Structure):
    _fields_ = [("curve", C.c_int32), ("metering", C.c_int32), ("exposure", C.c_float), ("key", C.c_float), ("white", C.c_float),
                ("low_permille", C.c_uint32), ("high_permille", C.c_uint32)]


class ptc_exposure_info(C.Structure):
    _fields_ = [("pixels", C.c_uint32), ("counted", C.c_uint32), ("below", C.c_uint32), ("rejected", C.c_uint32),
                ("level_bin", C.c_int32), ("level", C.c_float), ("scale", C.c_float), ("histogram", C.c_uint32 * 256)]


class ptc_upload_times(C.Structure):
    _fields_ = [("bvh_build_ms", C.c_float), ("layout_ms", C.c_float), ("triangles_ms", C.c_float), ("copy_ms", C.c_float),
                ("total_ms", C.c_float), ("bvh_on_device", C.c_uint32), ("layout_on_device", C.c_uint32)]


class ptc_frame_plan(C.Structure):
    _fields_ = [("frames", C.c_int32), ("batch", C.c_int32), ("big_slots", C.c_int32), ("single_slots", C.c_int32),
                ("staged", C.c_int32)]


# every symbol include/ptcore.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SIGNATURES = {
    "ptc_abi_version": (C.c_int, []),
    "ptc_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "ptc_create": (C.c_int, [C.POINTER(ptc_config), C.POINTER(_P)]),
    "ptc_destroy": (None, [_P]),
    "ptc_last_error": (C.c_char_p, [_P]),
    "ptc_set_stream": (C.c_int, [_P, _P]),
    "ptc_upload_scene": (C.c_int, [_P, C.POINTER(ptc_scene_desc)]),
    "ptc_resize": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "ptc_set_rows": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "ptc_set_interleave": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32]),
    "ptc_restart": (C.c_int, [_P]),
    "ptc_iteration": (C.c_int, [_P]),
    "ptc_set_iteration": (C.c_int, [_P, C.c_int]),
    "ptc_set_max_iterations": (C.c_int, [_P, C.c_int]),
    "ptc_set_method": (C.c_int, [_P, C.c_int]),
    "ptc_set_max_bounces": (C.c_int, [_P, C.c_int]),
    "ptc_set_trace_variant": (C.c_int, [_P, C.c_int]),
    "ptc_set_param": (C.c_int, [_P, C.c_char_p, C.c_int]),
    "ptc_set_lens": (C.c_int, [_P, C.c_float, C.c_float]),
    "ptc_get_lens": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "ptc_generate_rays": (C.c_int, [_P, C.POINTER(ptc_camera), C.c_uint32, C.c_void_p, C.c_uint64]),
    "ptc_set_denoiser_params": (C.c_int, [_P, C.POINTER(ptc_denoiser_params)]),
    "ptc_trace": (C.c_int, [_P, C.POINTER(ptc_camera)]),
    "ptc_trace_begin": (C.c_int, [_P, C.POINTER(ptc_camera)]),
    "ptc_trace_bounce": (C.c_int, [_P, C.c_int, _P]),
    "ptc_trace_end": (C.c_int, [_P]),
    "ptc_live_count_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P)]),
    "ptc_copy_live_count": (C.c_int, [_P, C.c_int, _P]),
    "ptc_read_live_count": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint32)]),
    "ptc_denoise": (C.c_int, [_P]),
    "ptc_denoise_albedo": (C.c_int, [_P, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ptc_get_denoise_albedo_stats": (C.c_int, [_P, C.POINTER(ptc_denoise_albedo_stats)]),
    "ptc_check_demodulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "ptc_set_denoise_variance": (C.c_int, [_P, C.c_float]),
    "ptc_get_denoise_variance": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "ptc_denoise_variance": (C.c_int, [_P, C.c_void_p, C.c_void_p]),
    "ptc_get_denoise_variance_stats": (C.c_int, [_P, C.POINTER(ptc_denoise_variance_stats)]),
    "ptc_check_denoise_variance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_float,
                                             C.c_void_p, C.c_void_p]),
    "ptc_present_rgba8": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "ptc_download": (C.c_int, [_P, C.c_int, _P, C.c_int]),
    "ptc_band_export": (C.c_int, [_P, C.POINTER(ptc_band_handle)]),
    "ptc_band_import": (C.c_int, [_P, C.c_uint32, C.POINTER(ptc_band_handle)]),
    "ptc_band_publish": (C.c_int, [_P, C.c_int]),
    "ptc_gather_frame": (C.c_int, [_P, C.c_int, _P, C.c_int]),
    "ptc_gather_present_rgba8": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "ptc_gather_last_us": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "ptc_synchronize": (C.c_int, [_P]),
    "ptc_get_stats": (C.c_int, [_P, C.POINTER(ptc_stats)]),
    "ptc_set_profiling": (C.c_int, [_P, C.c_int, C.c_int]),
    "ptc_reset_profile": (C.c_int, [_P]),
    "ptc_get_profile": (C.c_int, [_P, C.POINTER(ptc_profile)]),
    "ptc_intersect_rays": (C.c_int, [_P, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                      C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]),
    "ptc_occluded_rays": (C.c_int, [_P, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint8)]),
    "ptc_get_occlusion_stats": (C.c_int, [_P, C.POINTER(ptc_occlusion_stats)]),
    "ptc_light_table": (C.c_int, [C.POINTER(ptc_scene_desc), C.POINTER(ptc_light), C.c_uint32, C.POINTER(ptc_light_info)]),
    "ptc_get_light_info": (C.c_int, [_P, C.POINTER(ptc_light_info)]),
    "ptc_direct_light": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_int]),
    "ptc_get_direct_stats": (C.c_int, [_P, C.POINTER(ptc_direct_stats)]),
    "ptc_get_direct_loop_stats": (C.c_int, [_P, C.POINTER(ptc_direct_loop_stats)]),
    "ptc_get_upload_times": (C.c_int, [_P, C.POINTER(ptc_upload_times)]),
    "ptc_download_layout": (C.c_int, [_P, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "ptc_build_bvh_device": (C.c_int, [_P, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32,
                                       C.POINTER(ptc_bvh_node), C.POINTER(C.c_uint32)]),
    "ptc_build_bvh": (C.c_int, [C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32,
                                 C.POINTER(ptc_bvh_node), C.POINTER(C.c_uint32)]),
    "ptc_make_object": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_float), C.POINTER(ptc_sphere),
                                   C.POINTER(C.c_float), C.POINTER(ptc_object)]),
    "ptc_check_traversal_layout": (C.c_int, [C.POINTER(ptc_bvh_node), C.c_uint32, C.POINTER(C.c_uint64)]),
    "ptc_check_beam": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                 C.POINTER(C.c_uint64), C.c_void_p]),
    "ptc_check_beam_frustum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]),
    "ptc_debug_beam_entries": (C.c_int, [_P, C.POINTER(ptc_camera), C.c_void_p, C.c_uint64]),
    "ptc_debug_sphere_lanes": (C.c_int, [_P, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ptc_debug_persist": (C.c_int, [_P, C.c_int, C.c_void_p, C.c_uint64]),
    "ptc_check_feed": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "ptc_check_frame_plan": (C.c_int, [C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(ptc_frame_plan)]),
    "ptc_check_megakernel_instance": (C.c_int, [C.c_int] * 11 + [C.c_char_p, C.c_uint32, C.POINTER(C.c_int)]),
    "ptc_check_megakernel_instance2": (C.c_int, [C.c_int] * 12 + [C.c_char_p, C.c_uint32, C.POINTER(C.c_int)]),
    "ptc_selftest_math": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_float),
                                     C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "ptc_selftest_rng": (C.c_int, [_P, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "ptc_check_rng": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "ptc_set_environment": (C.c_int, [_P, C.c_void_p, C.c_uint32]),
    "ptc_get_environment": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "ptc_sample_environment": (C.c_int, [_P, C.c_void_p, C.c_uint32, C.c_void_p]),
    "ptc_environment_from_equirect": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p]),
    "ptc_check_environment": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "ptc_check_environment_apron": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "ptc_environment_light": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_int]),
    "ptc_get_environment_light_stats": (C.c_int, [_P, C.POINTER(ptc_direct_stats)]),
    "ptc_get_environment_light_loop_stats": (C.c_int, [_P, C.POINTER(ptc_environment_light_loop_stats)]),
    "ptc_check_environment_light_table": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "ptc_environment_light_pdf": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_int]),
    "ptc_light_material_pdf": (C.c_int, [C.POINTER(ptc_scene_desc), _P, C.c_uint32]),
    "ptc_get_mis_loop_stats": (C.c_int, [_P, C.POINTER(ptc_mis_loop_stats)]),
    "ptc_set_vertex_normals": (C.c_int, [_P, C.c_void_p, C.c_uint32]),
    "ptc_get_vertex_normals": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "ptc_compute_vertex_normals": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "ptc_hit_attributes": (C.c_int, [_P, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ptc_get_smooth_loop_stats": (C.c_int, [_P, C.POINTER(ptc_smooth_loop_stats)]),
    "ptc_set_textures": (C.c_int, [_P, C.POINTER(ptc_texture_desc), C.c_uint32, C.c_void_p, C.c_uint32]),
    "ptc_get_textures": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "ptc_set_texcoords": (C.c_int, [_P, C.c_void_p, C.c_uint32]),
    "ptc_get_texcoords": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "ptc_texture_decode_table": (C.c_int, [C.c_uint32, C.c_void_p]),
    "ptc_sample_texture": (C.c_int, [_P, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "ptc_hit_surface": (C.c_int, [_P, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "ptc_get_texture_loop_stats": (C.c_int, [_P, C.POINTER(ptc_texture_loop_stats)]),
    "ptc_check_texture_lookup": (C.c_int, [C.POINTER(ptc_texture_desc), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "ptc_set_normal_maps": (C.c_int, [_P, C.c_void_p, C.c_uint32]),
    "ptc_get_normal_maps": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "ptc_normal_map_decode_table": (C.c_int, [C.c_void_p]),
    "ptc_hit_shading_normal": (C.c_int, [_P, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "ptc_get_normal_map_loop_stats": (C.c_int, [_P, C.POINTER(ptc_normal_map_loop_stats)]),
    "ptc_check_normal_map": (C.c_int, [C.POINTER(ptc_texture_desc)] + [C.c_void_p] * 12 + [C.c_uint32, C.c_void_p, C.c_void_p]),
    "ptc_check_shading_normal": (C.c_int, [C.c_void_p] * 8 + [C.c_uint32, C.c_void_p, C.c_void_p]),
    "ptc_check_environment_light_pdf": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "ptc_check_environment_light": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "ptc_check_light_sample": (C.c_int, [C.POINTER(ptc_scene_desc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "ptc_set_display": (C.c_int, [_P, C.POINTER(ptc_display_params)]),
    "ptc_get_display": (C.c_int, [_P, C.POINTER(ptc_display_params)]),
    "ptc_get_exposure_info": (C.c_int, [_P, C.POINTER(ptc_exposure_info)]),
    "ptc_tonemap_buffer": (C.c_int, [_P, C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                     C.POINTER(ptc_exposure_info)]),
    "ptc_check_display_params": (C.c_int, [C.POINTER(ptc_display_params), C.c_char_p, C.c_uint32]),
    "ptc_check_display_meter": (C.c_int, [C.POINTER(ptc_display_params), C.c_void_p, C.c_int, C.c_uint32, C.POINTER(ptc_exposure_info)]),
    "ptc_check_display_map": (C.c_int, [C.POINTER(ptc_display_params), C.c_float, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]),
}

_lib = None


def lib():
    """Load libptcore.so (once).  Raises if it is missing: there is no fallback implementation."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C cuda-path-tracer_amd/csrc` (there is no CPU/Python fallback)")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


class PtcError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"ptcore error {code}: {message}")
        self.code = code


def check(rc, ctx=None):
    if rc < 0:
        msg = lib().ptc_last_error(ctx)
        raise PtcError(rc, msg.decode() if msg else "")
    return rc
