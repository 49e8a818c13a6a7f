"""ctypes bindings of the C ABI (include/acgpt.h) and of the host-side mirror library.

The product path is libacgpt_hip.so and nothing else: if it is missing or fails to load,
importing this module's `hip()` raises — there is no fallback.
"""
import ctypes as C
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))


class Float3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]

    def __init__(self, x=0.0, y=0.0, z=0.0):
        super().__init__(float(x), float(y), float(z))

    def tuple(self):
        return (self.x, self.y, self.z)


class Material(C.Structure):
    """Material, PathTracer_Optix/TinyObjWrapper.h:33-40."""
    _fields_ = [("diffuse", Float3), ("emission", Float3), ("roughness", C.c_float),
                ("metallic", C.c_float), ("ior", C.c_float), ("bsdfType", C.c_int32)]


class AreaLight(C.Structure):
    """AreaLight, PathTracer_Optix/pathTracer.h:77-83."""
    _fields_ = [("corner", Float3), ("v1", Float3), ("v2", Float3), ("normal", Float3), ("emission", Float3)]


class PathTraceParams(C.Structure):
    """PathTraceParams, PathTracer_Optix/pathTracer.h:85-108 (168 bytes)."""
    _fields_ = [("currentFrameIdx", C.c_uint32),
                ("accumulationBuffer", C.c_void_p),
                ("frameBuffer", C.c_void_p),
                ("width", C.c_uint32), ("height", C.c_uint32),
                ("samplesPerPixel", C.c_uint32), ("maxDepth", C.c_uint32),
                ("cameraEye", Float3), ("cameraU", Float3), ("cameraV", Float3), ("cameraW", Float3),
                ("areaLight", AreaLight),
                ("handle", C.c_uint64),
                ("useDirectLighting", C.c_uint8), ("useImportanceSampling", C.c_uint8)]


class Stats(C.Structure):
    _fields_ = [("radiance_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("paths", C.c_uint64),
                ("kernel_ms", C.c_float), ("launch_ms", C.c_float), ("pixels", C.c_uint32), ("grid_blocks", C.c_uint32), ("sample_chunks", C.c_uint32), ("variant", C.c_uint32),
                ("trav_wave_steps", C.c_uint64), ("trav_lane_steps", C.c_uint64),
                ("shade_wave_rounds", C.c_uint64), ("shade_lane_rounds", C.c_uint64), ("culled_rays", C.c_uint64),
                ("math_mode", C.c_uint32), ("reserved", C.c_uint32)]


class TreeInfo(C.Structure):
    """pt_tree_info of include/acgpt_test.h (pt_debug_read_tree; not part of the ABI)"""
    _fields_ = [("n_tris", C.c_uint32), ("n_nodes", C.c_uint32), ("max_depth", C.c_uint32), ("mode", C.c_int32), ("pad_abs", C.c_float),
                ("hspace", C.c_float * 8), ("scene_lo", C.c_float * 3), ("scene_hi", C.c_float * 3),
                ("n_wrecs", C.c_uint32), ("n_wnodes", C.c_uint32), ("wide_depth", C.c_uint32), ("held", C.c_uint32)]


class BuildStats(C.Structure):
    """pt_build_stats of include/acgpt_test.h (pt_debug_build_stats; not part of the ABI)"""
    _fields_ = [("opt_area_before", C.c_float), ("opt_area_after", C.c_float), ("opt_ms", C.c_float),
                ("opt_passes", C.c_uint32), ("build_iterations", C.c_uint32), ("mode", C.c_int32)]


class BvhInfo(C.Structure):
    _fields_ = [("n_tris", C.c_uint32), ("n_nodes", C.c_uint32), ("max_depth", C.c_uint32), ("stack_entries", C.c_uint32),
                ("scene_lo", C.c_float * 3), ("scene_hi", C.c_float * 3), ("build_ms", C.c_float),
                ("node_bytes", C.c_uint32), ("tri_bytes", C.c_uint32),
                ("wide_nodes", C.c_uint32), ("wide_depth", C.c_uint32), ("wide_bytes", C.c_uint32), ("wide_ms", C.c_float),
                ("half_node_bytes", C.c_uint32), ("half_area_ratio", C.c_float), ("half_box_inflation", C.c_float),
                ("device_bytes", C.c_uint64)]


class WindingInfo(C.Structure):
    """pt_winding_info (include/acgpt.h)."""
    _fields_ = [("built", C.c_uint32), ("n_nodes", C.c_uint32), ("bytes", C.c_uint64)]


class UpdateInfo(C.Structure):
    """pt_update_info (include/acgpt.h)."""
    _fields_ = [("ms", C.c_float), ("area_ratio", C.c_float), ("rebuilt", C.c_uint32), ("reserved", C.c_uint32)]


class DisplayParams(C.Structure):
    """pt_display_params (include/acgpt.h)."""
    _fields_ = [("tone_curve", C.c_uint32), ("exposure", C.c_float), ("key", C.c_float), ("white", C.c_float),
                ("lo_permille", C.c_uint32), ("hi_permille", C.c_uint32), ("min_exposure", C.c_float), ("max_exposure", C.c_float),
                ("prev_exposure", C.c_float), ("adapt", C.c_float)]


DISPLAY_BINS = 320                                                 # PT_DISPLAY_BINS


class DisplayInfo(C.Structure):
    """pt_display_info (include/acgpt.h)."""
    _fields_ = [("exposure", C.c_float), ("metered_luminance", C.c_float), ("metered_pixels", C.c_uint32), ("unmetered_pixels", C.c_uint32),
                ("histogram", C.c_uint32 * DISPLAY_BINS)]


class ConvergenceParams(C.Structure):
    """pt_convergence_params (include/acgpt.h)."""
    _fields_ = [("lum_floor", C.c_float), ("threshold", C.c_float), ("quantile_permille", C.c_uint32), ("reserved", C.c_uint32)]


CONVERGENCE_BINS, CONVERGENCE_TILE = 256, 16                       # PT_CONVERGENCE_BINS, PT_CONVERGENCE_TILE


class ConvergenceInfo(C.Structure):
    """pt_convergence_info (include/acgpt.h)."""
    _fields_ = [("frames", C.c_uint32), ("measured_pixels", C.c_uint32), ("unmeasured_pixels", C.c_uint32), ("invalid_pixels", C.c_uint32),
                ("converged_pixels", C.c_uint32), ("max_error", C.c_float), ("quantile_error", C.c_float), ("reserved", C.c_uint32),
                ("histogram", C.c_uint32 * CONVERGENCE_BINS)]


class FireflyParams(C.Structure):
    """pt_firefly_params (include/acgpt.h)."""
    _fields_ = [("ratio", C.c_float), ("floor", C.c_float), ("rank", C.c_uint32), ("radius", C.c_uint32)]


class FireflyInfo(C.Structure):
    """pt_firefly_info (include/acgpt.h)."""
    _fields_ = [("clamped_pixels", C.c_uint32), ("replaced_pixels", C.c_uint32), ("passed_pixels", C.c_uint32), ("reserved", C.c_uint32),
                ("total_luma_q16", C.c_uint64), ("removed_luma_q16", C.c_uint64), ("max_ratio", C.c_float), ("reserved2", C.c_uint32)]


class BloomParams(C.Structure):
    """pt_bloom_params (include/acgpt.h)."""
    _fields_ = [("threshold", C.c_float), ("knee", C.c_float), ("clamp", C.c_float), ("intensity", C.c_float), ("spread", C.c_float),
                ("levels", C.c_uint32)]


class BloomInfo(C.Structure):
    """pt_bloom_info (include/acgpt.h)."""
    _fields_ = [("levels", C.c_uint32), ("bright_pixels", C.c_uint32), ("invalid_pixels", C.c_uint32), ("reserved", C.c_uint32),
                ("total_luma_q16", C.c_uint64), ("bright_luma_q16", C.c_uint64), ("max_luma", C.c_float), ("reserved2", C.c_uint32)]


class AoParams(C.Structure):
    """pt_ao_params (include/acgpt.h)."""
    _fields_ = [("samples", C.c_uint32), ("radius", C.c_float), ("bias", C.c_float), ("seed", C.c_uint32), ("accumulate", C.c_uint32),
                ("total_samples", C.c_uint32), ("reserved", C.c_uint32 * 2)]


AO_MAX_SAMPLES = 256                                               # pt_ao_params.samples

assert C.sizeof(PathTraceParams) == 168
assert C.sizeof(Material) == 40
assert C.sizeof(AreaLight) == 60
assert C.sizeof(Stats) == 96 and C.sizeof(BvhInfo) == 88          # ABI version 4 (include/acgpt.h)
ABI_VERSION = 4
assert C.sizeof(UpdateInfo) == 16
UPDATE_REFIT, UPDATE_REBUILD, UPDATE_AUTO = 0, 1, 2                # pt_update_vertices
UPDATE_AUTO_AREA_RATIO = 1.25                                      # PT_UPDATE_AUTO_AREA_RATIO
MATH_IEEE, MATH_FAST = 0, 1                                        # pt_set_math_mode
MATERIALS_REFERENCE, MATERIALS_MICROFACET = 0, 1                   # pt_set_material_model
TONE_LINEAR, TONE_REINHARD, TONE_ACES = 0, 1, 2                    # pt_display_params.tone_curve
assert C.sizeof(DisplayParams) == 40 and C.sizeof(DisplayInfo) == 16 + 4 * DISPLAY_BINS
assert C.sizeof(ConvergenceParams) == 16 and C.sizeof(ConvergenceInfo) == 32 + 4 * CONVERGENCE_BINS
assert C.sizeof(FireflyParams) == 16 and C.sizeof(FireflyInfo) == 40
assert C.sizeof(BloomParams) == 24 and C.sizeof(BloomInfo) == 40
assert C.sizeof(AoParams) == 32
QUERY_MULTI_MAX = 8                                                # PT_QUERY_MULTI_MAX
QUERY_OVERLAP_MAX = 8                                              # PT_QUERY_OVERLAP_MAX
QUERY_NEAREST_MAX = 8                                              # PT_QUERY_NEAREST_MAX
WINDING_BETA_DEFAULT = 2.0                                         # PT_WINDING_BETA_DEFAULT
assert C.sizeof(WindingInfo) == 16
QUERY_TRIANGLES_MAX = 8                                            # PT_QUERY_TRIANGLES_MAX
LIST_REGISTER, LIST_SORT_LDS, LIST_SCAN_TILE, LIST_SCAN_RUNS = 8, 4096, 2048, 256   # kListRegister, kListSortLds, kListScanTile, kListScanRuns (csrc/lists.h)
QUERY_MESH_MAX = 1 << 20                                           # PT_QUERY_MESH_MAX
POSES_NO_EARLY, POSES_POSE_MAJOR = 1, 2                        # pt_debug_query_poses flags (csrc/poses.h)
BLOOM_MAX_LEVELS = 8                                               # pt_bloom_params.levels

# every symbol include/acgpt.h declares (the drop-in boundary) ...
ABI_SYMBOLS = [
    "pt_create", "pt_create_multi", "pt_device_count", "pt_destroy", "pt_last_error", "pt_set_scene", "pt_set_build_mode", "pt_scene_handle", "pt_get_bvh_info",
    "pt_launch", "pt_launch_frames", "pt_resolve_framebuffer", "pt_set_partition", "pt_set_sample_chunks", "pt_set_light_mode", "pt_set_math_mode", "pt_set_scratch_limit", "pt_set_tuning",
    "pt_variant_name", "pt_variant_kernel", "pt_kernel_source_hash", "pt_set_stream", "pt_get_stats",
    "pt_trace_closest", "pt_trace_any", "pt_query_closest", "pt_query_any", "pt_query_multi", "pt_query_nearest", "pt_query_overlap", "pt_query_overlap_any", "pt_query_sweep", "pt_query_sweep_any", "pt_query_capsule_cast", "pt_query_capsule_cast_any", "pt_query_box_cast", "pt_query_box_cast_any", "pt_query_triangles", "pt_query_triangles_any", "pt_list_offsets", "pt_query_overlap_lists", "pt_query_triangles_lists", "pt_query_overlap_oriented", "pt_query_overlap_oriented_any", "pt_query_overlap_oriented_lists", "pt_pose_boxes", "pt_query_segments", "pt_query_triangle_distance", "pt_set_query_mesh", "pt_get_query_mesh", "pt_pose_triangles", "pt_query_poses_any", "pt_query_poses_distance", "pt_query_triangle_cast", "pt_query_triangle_cast_any", "pt_query_poses_cast", "pt_query_nearest_k", "pt_query_within_any", "pt_query_winding", "pt_get_winding_info", "pt_ao_points", "pt_ao_image", "pt_render_features", "pt_denoise", "pt_temporal_blend", "pt_temporal_blend_motion", "pt_update_vertices", "pt_update_materials", "pt_set_environment",
    "pt_set_material_model", "pt_display_transform", "pt_convergence_update", "pt_firefly_filter", "pt_bloom",
    "pt_device_malloc", "pt_device_free", "pt_device_memset", "pt_copy_to_host", "pt_copy_to_device",
    "pt_host_malloc_mapped", "pt_host_free_mapped", "pt_abi_version",
]
# pt_box_cast_hit: {t, prim, feature, material | n.xyz, pad | c.xyz, pad}
BOX_CAST_DTYPE = np.dtype({"names": ["t", "prim", "feature", "material", "normal", "point"],
                           "formats": [np.float32, np.uint32, np.float32, np.uint32, (np.float32, 3), (np.float32, 3)],
                           "offsets": [0, 4, 8, 12, 16, 32], "itemsize": 48})
# ... and include/acgpt_test.h (test hooks and diagnostics; same library)
TEST_SYMBOLS = ["pt_bench_traversal", "pt_selftest", "pt_debug_wave_times", "pt_debug_queue_progress", "pt_debug_window_moves", "pt_debug_queue_order", "pt_debug_pixel_classes", "pt_debug_row_spans", "pt_read_morton", "pt_debug_environment", "pt_debug_environment_tables", "pt_debug_microfacet", "pt_debug_nearest_visits", "pt_debug_overlap_visits", "pt_debug_overlap_oriented_visits", "pt_debug_overlap_oriented_visits_cross", "pt_debug_sweep_visits", "pt_debug_capsule_cast_visits", "pt_debug_box_cast_visits", "pt_debug_triangles_visits", "pt_debug_segments_visits", "pt_debug_triangle_distance_visits", "pt_debug_nearest_k_visits", "pt_debug_winding_visits", "pt_debug_list_phases", "pt_debug_query_poses", "pt_debug_triangle_cast_visits", "pt_debug_query_poses_cast", "pt_debug_read_winding", "pt_debug_read_tree", "pt_debug_build_stats",
                "pt_debug_small_kernel", "pt_debug_small_kernel_path", "pt_debug_small_ref", "pt_debug_small_budget",
                "pt_debug_small_shape", "pt_debug_small_float_budget", "pt_debug_small_staged"]

_hip = None
_host = None


def hip_library_path():
    # ACGPT_EXPERIMENTS=1 (tools/sweep_variants.py only): the build that also carries the kernel variants that were
    # measured and not adopted.  Same sources, same ABI; never what tests, smoke() or bench.py load by default.
    if os.environ.get("ACGPT_HIP_LIB"):          # A/B measurements of differently built libraries (tools/ only)
        return os.path.join(PKG, os.environ["ACGPT_HIP_LIB"])
    if os.environ.get("ACGPT_EXPERIMENTS") == "1":
        return os.path.join(PKG, "libacgpt_hip_exp.so")
    return os.path.join(PKG, "libacgpt_hip.so")


def host_library_path():
    return os.path.join(PKG, "libacgpt_host.so")


def _torch_first():
    """The load-order rule of INTEGRATION.md section 5, enforced instead of documented only.  PyTorch's ROCm wheel carries its own
    HIP / HSA runtime; libacgpt_hip.so links against /opt/rocm's.  With torch's runtime up first the two coexist; in a process
    that loaded this library first, a later torch.cuda.init() reports "No HIP GPUs are available".  So, before the library is
    loaded: a torch that is already imported gets its GPU side initialised; a torch that is installed but not imported yet is
    imported and initialised (ACGPT_TORCH_FIRST=1, the default), left alone (=0: a process that will never use torch and does
    not want the import), or refused with the reason (=error)."""
    import importlib.util
    import sys
    mode = os.environ.get("ACGPT_TORCH_FIRST", "1")
    if "torch" not in sys.modules:
        if mode == "0" or importlib.util.find_spec("torch") is None:
            return
        if mode == "error":
            raise RuntimeError("libacgpt_hip.so is about to be loaded before PyTorch's GPU runtime: `import torch; torch.cuda.is_available()` "
                               "must come first in a process that uses both (INTEGRATION.md section 5), or set ACGPT_TORCH_FIRST=0 "
                               "if this process never touches torch.cuda")
    import torch
    torch.cuda.is_available()


def hip():
    """The HIP library.  Raises if it is not built or cannot be loaded (no fallback)."""
    global _hip
    if _hip is not None:
        return _hip
    path = hip_library_path()
    if not os.path.exists(path):
        raise RuntimeError("libacgpt_hip.so is not built (run __graft_entry__.build()); there is no CPU fallback")
    _torch_first()
    L = C.CDLL(path)
    vp, sz, u32p, f32p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    L.pt_create.argtypes = [C.POINTER(vp), C.c_int]; L.pt_create.restype = C.c_int
    L.pt_create_multi.argtypes = [C.POINTER(vp), C.POINTER(C.c_int), C.c_int]; L.pt_create_multi.restype = C.c_int
    L.pt_device_count.argtypes = [vp]; L.pt_device_count.restype = C.c_int
    L.pt_variant_kernel.argtypes = [C.c_int, C.c_int]; L.pt_variant_kernel.restype = C.c_char_p
    L.pt_kernel_source_hash.argtypes = []; L.pt_kernel_source_hash.restype = C.c_char_p
    L.pt_destroy.argtypes = [vp]; L.pt_destroy.restype = None
    L.pt_last_error.argtypes = [vp]; L.pt_last_error.restype = C.c_char_p
    L.pt_set_scene.argtypes = [vp, vp, sz, vp, sz, vp, vp, sz]; L.pt_set_scene.restype = C.c_int
    L.pt_set_build_mode.argtypes = [vp, C.c_int]; L.pt_set_build_mode.restype = C.c_int
    L.pt_scene_handle.argtypes = [vp]; L.pt_scene_handle.restype = C.c_uint64
    L.pt_get_bvh_info.argtypes = [vp, C.POINTER(BvhInfo)]; L.pt_get_bvh_info.restype = C.c_int
    L.pt_launch.argtypes = [vp, C.POINTER(PathTraceParams)]; L.pt_launch.restype = C.c_int
    L.pt_launch_frames.argtypes = [vp, C.POINTER(PathTraceParams), C.c_uint32]; L.pt_launch_frames.restype = C.c_int
    L.pt_resolve_framebuffer.argtypes = [vp, vp, vp, sz]; L.pt_resolve_framebuffer.restype = C.c_int
    L.pt_set_partition.argtypes = [vp, C.c_int, C.c_int]; L.pt_set_partition.restype = C.c_int
    L.pt_set_sample_chunks.argtypes = [vp, C.c_int]; L.pt_set_sample_chunks.restype = C.c_int
    L.pt_set_light_mode.argtypes = [vp, C.c_int]; L.pt_set_light_mode.restype = C.c_int
    L.pt_set_math_mode.argtypes = [vp, C.c_int]; L.pt_set_math_mode.restype = C.c_int
    L.pt_set_scratch_limit.argtypes = [vp, C.c_size_t]; L.pt_set_scratch_limit.restype = C.c_int
    L.pt_set_tuning.argtypes = [vp, C.c_int, C.c_int]; L.pt_set_tuning.restype = C.c_int
    L.pt_variant_name.argtypes = [C.c_int]; L.pt_variant_name.restype = C.c_char_p
    L.pt_set_stream.argtypes = [vp, vp]; L.pt_set_stream.restype = C.c_int
    L.pt_get_stats.argtypes = [vp, C.POINTER(Stats)]; L.pt_get_stats.restype = C.c_int
    L.pt_trace_closest.argtypes = [vp, vp, sz, vp, vp]; L.pt_trace_closest.restype = C.c_int
    L.pt_trace_any.argtypes = [vp, vp, sz, vp]; L.pt_trace_any.restype = C.c_int
    L.pt_query_closest.argtypes = [vp, vp, sz, vp]; L.pt_query_closest.restype = C.c_int
    L.pt_query_any.argtypes = [vp, vp, sz, vp]; L.pt_query_any.restype = C.c_int
    L.pt_query_multi.argtypes = [vp, vp, sz, C.c_uint32, vp, vp]; L.pt_query_multi.restype = C.c_int
    L.pt_query_nearest.argtypes = [vp, vp, sz, vp]; L.pt_query_nearest.restype = C.c_int
    L.pt_debug_nearest_visits.argtypes = [vp, vp, sz, vp, vp]; L.pt_debug_nearest_visits.restype = C.c_int
    L.pt_query_nearest_k.argtypes = [vp, vp, sz, C.c_uint32, vp, vp]; L.pt_query_nearest_k.restype = C.c_int
    L.pt_query_within_any.argtypes = [vp, vp, sz, vp]; L.pt_query_within_any.restype = C.c_int
    L.pt_debug_nearest_k_visits.argtypes = [vp, vp, sz, C.c_uint32, vp, vp, vp, vp]; L.pt_debug_nearest_k_visits.restype = C.c_int
    L.pt_query_winding.argtypes = [vp, vp, sz, C.c_float, vp]; L.pt_query_winding.restype = C.c_int
    L.pt_get_winding_info.argtypes = [vp, C.POINTER(WindingInfo)]; L.pt_get_winding_info.restype = C.c_int
    L.pt_debug_winding_visits.argtypes = [vp, vp, sz, C.c_float, vp, vp]; L.pt_debug_winding_visits.restype = C.c_int
    L.pt_debug_read_winding.argtypes = [vp, vp, sz]; L.pt_debug_read_winding.restype = C.c_int
    L.pt_query_segments.argtypes = [vp, vp, sz, vp]; L.pt_query_segments.restype = C.c_int
    L.pt_debug_segments_visits.argtypes = [vp, vp, sz, vp, vp, C.c_uint32]; L.pt_debug_segments_visits.restype = C.c_int
    L.pt_query_triangle_distance.argtypes = [vp, vp, sz, vp]; L.pt_query_triangle_distance.restype = C.c_int
    L.pt_debug_triangle_distance_visits.argtypes = [vp, vp, sz, vp, vp, C.c_uint32]; L.pt_debug_triangle_distance_visits.restype = C.c_int
    L.pt_set_query_mesh.argtypes = [vp, vp, sz]; L.pt_set_query_mesh.restype = C.c_int
    L.pt_get_query_mesh.argtypes = [vp, C.POINTER(sz), C.POINTER(sz)]; L.pt_get_query_mesh.restype = C.c_int
    L.pt_pose_triangles.argtypes = [vp, vp, sz, vp]; L.pt_pose_triangles.restype = C.c_int
    L.pt_query_poses_any.argtypes = [vp, vp, sz, vp, vp]; L.pt_query_poses_any.restype = C.c_int
    L.pt_query_poses_distance.argtypes = [vp, vp, sz, C.c_float, vp]; L.pt_query_poses_distance.restype = C.c_int
    L.pt_debug_query_poses.argtypes = [vp, vp, sz, C.c_float, vp, vp, vp, C.c_uint32]; L.pt_debug_query_poses.restype = C.c_int
    L.pt_query_overlap.argtypes = [vp, vp, sz, C.c_uint32, vp, vp]; L.pt_query_overlap.restype = C.c_int
    L.pt_query_overlap_any.argtypes = [vp, vp, sz, vp]; L.pt_query_overlap_any.restype = C.c_int
    L.pt_debug_overlap_visits.argtypes = [vp, vp, sz, vp, vp]; L.pt_debug_overlap_visits.restype = C.c_int
    L.pt_query_triangle_cast.argtypes = [vp, vp, sz, vp]; L.pt_query_triangle_cast.restype = C.c_int
    L.pt_query_triangle_cast_any.argtypes = [vp, vp, sz, vp]; L.pt_query_triangle_cast_any.restype = C.c_int
    L.pt_debug_triangle_cast_visits.argtypes = [vp, vp, sz, vp, vp]; L.pt_debug_triangle_cast_visits.restype = C.c_int
    L.pt_query_poses_cast.argtypes = [vp, vp, vp, sz, vp]; L.pt_query_poses_cast.restype = C.c_int
    L.pt_debug_query_poses_cast.argtypes = [vp, vp, vp, sz, vp, C.c_uint32]; L.pt_debug_query_poses_cast.restype = C.c_int
    L.pt_query_sweep.argtypes = [vp, vp, sz, vp]; L.pt_query_sweep.restype = C.c_int
    L.pt_query_sweep_any.argtypes = [vp, vp, sz, vp]; L.pt_query_sweep_any.restype = C.c_int
    L.pt_debug_sweep_visits.argtypes = [vp, vp, sz, vp, vp]; L.pt_debug_sweep_visits.restype = C.c_int
    L.pt_query_capsule_cast.argtypes = [vp, vp, sz, vp]; L.pt_query_capsule_cast.restype = C.c_int
    L.pt_query_capsule_cast_any.argtypes = [vp, vp, sz, vp]; L.pt_query_capsule_cast_any.restype = C.c_int
    L.pt_debug_capsule_cast_visits.argtypes = [vp, vp, sz, vp, vp, C.c_uint32]; L.pt_debug_capsule_cast_visits.restype = C.c_int
    L.pt_query_box_cast.argtypes = [vp, vp, sz, vp]; L.pt_query_box_cast.restype = C.c_int
    L.pt_query_box_cast_any.argtypes = [vp, vp, sz, vp]; L.pt_query_box_cast_any.restype = C.c_int
    L.pt_debug_box_cast_visits.argtypes = [vp, vp, sz, vp, vp, C.c_uint32]; L.pt_debug_box_cast_visits.restype = C.c_int
    L.pt_query_triangles.argtypes = [vp, vp, sz, C.c_uint32, vp, vp]; L.pt_query_triangles.restype = C.c_int
    L.pt_query_triangles_any.argtypes = [vp, vp, sz, vp]; L.pt_query_triangles_any.restype = C.c_int
    L.pt_debug_triangles_visits.argtypes = [vp, vp, sz, vp, vp]; L.pt_debug_triangles_visits.restype = C.c_int
    L.pt_list_offsets.argtypes = [vp, vp, sz, vp, C.POINTER(C.c_uint64)]; L.pt_list_offsets.restype = C.c_int
    L.pt_query_overlap_lists.argtypes = [vp, vp, sz, vp, vp, sz, vp]; L.pt_query_overlap_lists.restype = C.c_int
    L.pt_query_overlap_oriented.argtypes = [vp, vp, sz, C.c_uint32, vp, vp]; L.pt_query_overlap_oriented.restype = C.c_int
    L.pt_query_overlap_oriented_any.argtypes = [vp, vp, sz, vp]; L.pt_query_overlap_oriented_any.restype = C.c_int
    L.pt_query_overlap_oriented_lists.argtypes = [vp, vp, sz, vp, vp, sz, vp]; L.pt_query_overlap_oriented_lists.restype = C.c_int
    L.pt_debug_overlap_oriented_visits.argtypes = [vp, vp, sz, vp, vp]; L.pt_debug_overlap_oriented_visits.restype = C.c_int
    L.pt_debug_overlap_oriented_visits_cross.argtypes = [vp, vp, sz, vp, vp]; L.pt_debug_overlap_oriented_visits_cross.restype = C.c_int
    L.pt_pose_boxes.argtypes = [vp, vp, sz, C.POINTER(C.c_float), vp]; L.pt_pose_boxes.restype = C.c_int
    L.pt_query_triangles_lists.argtypes = [vp, vp, sz, vp, vp, sz, vp]; L.pt_query_triangles_lists.restype = C.c_int
    L.pt_debug_list_phases.argtypes = [vp, C.c_uint32]; L.pt_debug_list_phases.restype = C.c_int
    L.pt_ao_points.argtypes = [vp, vp, sz, vp, C.POINTER(AoParams), vp, vp]; L.pt_ao_points.restype = C.c_int
    L.pt_ao_image.argtypes = [vp, C.POINTER(PathTraceParams), vp, vp, C.POINTER(AoParams), vp, vp]; L.pt_ao_image.restype = C.c_int
    L.pt_render_features.argtypes = [vp, C.POINTER(PathTraceParams), vp, vp]; L.pt_render_features.restype = C.c_int
    L.pt_denoise.argtypes = [vp, C.POINTER(PathTraceParams), vp, vp, vp, C.c_uint32]; L.pt_denoise.restype = C.c_int
    L.pt_temporal_blend.argtypes = [vp, C.POINTER(PathTraceParams), C.c_uint32, vp, vp, C.POINTER(PathTraceParams), vp, vp, vp, C.c_float, vp]
    L.pt_temporal_blend.restype = C.c_int
    L.pt_temporal_blend_motion.argtypes = [vp, C.POINTER(PathTraceParams), C.c_uint32, vp, vp, C.POINTER(PathTraceParams), vp, vp, vp, vp, vp,
                                           sz, C.c_float, C.c_float, vp]
    L.pt_temporal_blend_motion.restype = C.c_int
    L.pt_update_vertices.argtypes = [vp, vp, sz, C.c_int, C.POINTER(UpdateInfo)]; L.pt_update_vertices.restype = C.c_int
    L.pt_update_materials.argtypes = [vp, vp, sz, vp, sz, C.POINTER(UpdateInfo)]; L.pt_update_materials.restype = C.c_int
    L.pt_set_environment.argtypes = [vp, vp, C.c_uint32, C.c_uint32, Float3]; L.pt_set_environment.restype = C.c_int
    L.pt_debug_environment.argtypes = [vp, C.c_int, vp, sz, vp]; L.pt_debug_environment.restype = C.c_int
    L.pt_debug_environment_tables.argtypes = [vp, vp, vp, vp, vp, vp]; L.pt_debug_environment_tables.restype = C.c_int
    L.pt_set_material_model.argtypes = [vp, C.c_int]; L.pt_set_material_model.restype = C.c_int
    L.pt_display_transform.argtypes = [vp, vp, sz, C.POINTER(DisplayParams), vp, vp, C.POINTER(DisplayInfo)]; L.pt_display_transform.restype = C.c_int
    L.pt_convergence_update.argtypes = [vp, C.POINTER(PathTraceParams), C.c_uint32, C.POINTER(ConvergenceParams), vp, vp, vp, C.POINTER(ConvergenceInfo)]
    L.pt_convergence_update.restype = C.c_int
    L.pt_firefly_filter.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(FireflyParams), vp, C.POINTER(FireflyInfo)]; L.pt_firefly_filter.restype = C.c_int
    L.pt_bloom.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(BloomParams), vp, C.POINTER(BloomInfo)]; L.pt_bloom.restype = C.c_int
    L.pt_debug_microfacet.argtypes = [vp, C.c_int, vp, sz, vp]; L.pt_debug_microfacet.restype = C.c_int
    L.pt_bench_traversal.argtypes = [vp, vp, sz, C.c_int, C.c_int, vp, vp, C.POINTER(C.c_float), vp]; L.pt_bench_traversal.restype = C.c_int
    L.pt_selftest.argtypes = [vp, C.c_int, vp, sz, vp]; L.pt_selftest.restype = C.c_int
    L.pt_debug_wave_times.argtypes = [vp, vp, sz]; L.pt_debug_wave_times.restype = C.c_int
    L.pt_debug_queue_progress.argtypes = [vp, vp]; L.pt_debug_queue_progress.restype = C.c_int
    L.pt_read_morton.argtypes = [vp, vp, vp]; L.pt_read_morton.restype = C.c_int
    L.pt_debug_read_tree.argtypes = [vp, C.c_int, vp, sz, C.POINTER(TreeInfo)]; L.pt_debug_read_tree.restype = C.c_int
    L.pt_debug_build_stats.argtypes = [vp, C.POINTER(BuildStats)]; L.pt_debug_build_stats.restype = C.c_int
    L.pt_debug_window_moves.argtypes = [vp, vp]; L.pt_debug_window_moves.restype = C.c_int
    L.pt_debug_small_kernel.argtypes = [vp, C.c_int]; L.pt_debug_small_kernel.restype = C.c_int
    L.pt_debug_small_kernel_path.argtypes = [vp]; L.pt_debug_small_kernel_path.restype = C.c_int
    L.pt_debug_small_ref.argtypes = [vp, sz, vp, vp, vp]; L.pt_debug_small_ref.restype = C.c_int
    L.pt_debug_small_budget.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, vp]; L.pt_debug_small_budget.restype = C.c_int
    L.pt_debug_small_shape.argtypes = [vp, C.c_int]; L.pt_debug_small_shape.restype = C.c_int
    L.pt_debug_small_float_budget.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, vp]; L.pt_debug_small_float_budget.restype = C.c_int
    L.pt_debug_small_staged.argtypes = [vp, vp, sz]; L.pt_debug_small_staged.restype = C.c_int
    if hasattr(L, "pt_debug_node_order"):      # experiments library only
        L.pt_debug_node_order.argtypes = [vp, C.c_int]; L.pt_debug_node_order.restype = C.c_int
    if hasattr(L, "pt_debug_wf"):      # experiments library only
        L.pt_debug_wf.argtypes = [vp, vp]; L.pt_debug_wf.restype = C.c_int
    L.pt_debug_queue_order.argtypes = [vp, C.c_int]; L.pt_debug_queue_order.restype = C.c_int
    L.pt_debug_pixel_classes.argtypes = [vp, C.c_int]; L.pt_debug_pixel_classes.restype = C.c_int
    L.pt_debug_row_spans.argtypes = [C.POINTER(PathTraceParams), vp, vp, vp]; L.pt_debug_row_spans.restype = C.c_int
    L.pt_device_malloc.argtypes = [vp, C.POINTER(vp), sz]; L.pt_device_malloc.restype = C.c_int
    L.pt_device_free.argtypes = [vp, vp]; L.pt_device_free.restype = C.c_int
    L.pt_device_memset.argtypes = [vp, vp, C.c_int, sz]; L.pt_device_memset.restype = C.c_int
    L.pt_copy_to_host.argtypes = [vp, vp, vp, sz]; L.pt_copy_to_host.restype = C.c_int
    L.pt_copy_to_device.argtypes = [vp, vp, vp, sz]; L.pt_copy_to_device.restype = C.c_int
    L.pt_host_malloc_mapped.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), sz]; L.pt_host_malloc_mapped.restype = C.c_int
    L.pt_host_free_mapped.argtypes = [vp, vp]; L.pt_host_free_mapped.restype = C.c_int
    L.pt_abi_version.argtypes = []; L.pt_abi_version.restype = C.c_uint32
    if L.pt_abi_version() != ABI_VERSION:
        raise RuntimeError("libacgpt_hip.so has ABI version %d, this binding expects %d: rebuild (__graft_entry__.build())" % (L.pt_abi_version(), ABI_VERSION))
    _hip = L
    return L


def host():
    """The host-side mirror library (OBJ ingest, Camera, Trackball): plain C++ on the CPU."""
    global _host
    if _host is not None:
        return _host
    path = host_library_path()
    if not os.path.exists(path):
        raise RuntimeError("libacgpt_host.so is not built (run __graft_entry__.build())")
    L = C.CDLL(path)
    vp, sz = C.c_void_p, C.c_size_t
    L.pth_obj_load.argtypes = [C.c_char_p]; L.pth_obj_load.restype = vp
    L.pth_obj_ok.argtypes = [vp]; L.pth_obj_ok.restype = C.c_int
    L.pth_obj_error.argtypes = [vp]; L.pth_obj_error.restype = C.c_char_p
    L.pth_obj_warning.argtypes = [vp]; L.pth_obj_warning.restype = C.c_char_p
    L.pth_obj_sizes.argtypes = [vp] + [C.POINTER(sz)] * 4; L.pth_obj_sizes.restype = None
    L.pth_obj_fill.argtypes = [vp, vp, vp, vp, vp]; L.pth_obj_fill.restype = None
    L.pth_obj_free.argtypes = [vp]; L.pth_obj_free.restype = None
    L.pth_camera_uvw.argtypes = [vp, vp, vp, C.c_float, C.c_float, vp, vp, vp]; L.pth_camera_uvw.restype = None
    L.pth_trackball_script.argtypes = [vp, vp, vp, C.c_float, C.c_float, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, vp, sz, vp]
    L.pth_trackball_script.restype = None
    L.pth_save_image.argtypes = [C.c_char_p, vp, C.c_int, C.c_int]; L.pth_save_image.restype = C.c_int
    L.pth_save_pfm.argtypes = [C.c_char_p, vp, C.c_int, C.c_int, C.c_int]; L.pth_save_pfm.restype = C.c_int
    L.pth_load_environment.argtypes = [C.c_char_p, vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, sz]; L.pth_load_environment.restype = C.c_int
    _host = L
    return L
