"""ctypes binding of libcloudtrace.so (include/cloudtrace.h).  There is NO fallback: if the
HIP library is missing this raises, and every call that needs a GPU fails with the library's
own error code when no device is present."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

PKG = Path(__file__).resolve().parent
# CT_LIBRARY: another build of the same library beside the product's (python -m deepestscatter_amd.build --variant ...): the
# experiments build libcloudtrace_exp.so (tests/test_exchange.py, tools/) or an A/B build.  File name only, always in-tree.
LIB_PATH = PKG / os.path.basename(os.environ.get("CT_LIBRARY", "libcloudtrace.so"))

CT_ABI_VERSION = 1
CT_OK, CT_E_INVAL, CT_E_HIP, CT_E_NOMEM, CT_E_STATE, CT_E_NODEVICE, CT_E_RCCL = 0, -1, -2, -3, -4, -5, -6
CT_MODE_SUN_AND_SKY_ALL_SCATTER, CT_MODE_SUN_MULTIPLE_SCATTER, CT_MODE_SUN_SINGLE_SCATTER = 0, 1, 2
CT_EST_MARCH, CT_EST_DELTA = 0, 1
CT_BUF_MEAN, CT_BUF_M2, CT_BUF_FRAME, CT_BUF_SCREEN, CT_BUF_INSCATTER, CT_BUF_DENSITY = range(6)
CT_FLAG_NONE, CT_FLAG_SIMPLE_KERNEL, CT_FLAG_LIGHT_NORMALIZED, CT_FLAG_SPARSE_BRICKS, CT_FLAG_VMM_BRICKS = 0, 1, 2, 4, 8
(CT_LAYOUT_DENSITY_BRICKS, CT_LAYOUT_SHADOW_BRICKS, CT_LAYOUT_MARCH_BRICKS, CT_LAYOUT_MARCH_ROWS, CT_LAYOUT_MARCH_COARSE,
 CT_LAYOUT_TWIN_BRICKS, CT_LAYOUT_MAJORANT_CELLS, CT_LAYOUT_MAJORANT_CODES, CT_LAYOUT_MIP_PYRAMID) = range(9)   # ct_debug_layout
CT_FLAG_TEX_FIXED8 = 16   # filter weights in 1.8 fixed point, like the reference's texture unit (include/cloudtrace.h)
CT_NET_OUT_LINEAR, CT_NET_OUT_EXPM1 = 0, 1   # CtNetworkRender.transform, low byte
CT_NET_ADD_SINGLE_SCATTER = 0x100            # CtNetworkRender.transform, bit 8: add the sun's single-scatter term

# every symbol include/cloudtrace.h declares (tests check the library exports all of them)
EXPORTS = [
    "ct_create", "ct_destroy", "ct_last_error", "ct_set_stream", "ct_set_camera", "ct_set_light", "ct_render_subframe",
    "ct_accumulate", "ct_render_accumulate", "ct_render_accumulate_async", "ct_synchronize", "ct_copy_to_device_async", "ct_point_radiance_launch", "ct_collector_create", "ct_collector_update", "ct_collector_info", "ct_collector_download", "ct_collector_destroy", "ct_adaptive_frame_create", "ct_adaptive_frame_update", "ct_adaptive_frame_raise_cap", "ct_adaptive_frame_info", "ct_adaptive_frame_download", "ct_adaptive_frame_device_ptr", "ct_adaptive_frame_destroy", "ct_generate_scatter_samples", "ct_collect_descriptors", "ct_descriptor_frame", "ct_debug_descriptor_frame_time", "ct_network_create", "ct_network_destroy", "ct_network_eval", "ct_debug_network_time", "ct_network_render_subframe", "ct_network_render_accumulate", "ct_network_render_shard_subframe", "ct_network_render_shard_accumulate", "ct_debug_network_scratch", "ct_debug_network_aux", "ct_debug_network_render_time", "ct_network_bake", "ct_bake_update", "ct_bake_destroy", "ct_bake_info", "ct_bake_probes", "ct_bake_download", "ct_debug_bake_lookup", "ct_network_bake_sparse", "ct_bake_sparse_info", "ct_bake_mask", "ct_network_bake_compact", "ct_bake_storage_info", "ct_bake_slots", "ct_bake_download_stored", "ct_bake_traced", "ct_bake_trace_more", "ct_bake_retrace", "ct_bake_trace_info", "ct_bake_directions", "ct_bake_traced_adaptive", "ct_bake_trace_adaptive_more", "ct_bake_retrace_adaptive", "ct_bake_adaptive_info", "ct_bake_download_counts", "ct_debug_bake_mask", "ct_baked_render_subframe", "ct_baked_render_accumulate", "ct_baked_render_shard_subframe", "ct_baked_render_shard_accumulate", "ct_debug_baked_render_time", "ct_reset", "ct_tonemap", "ct_tonemap_async", "ct_set_render_ahead", "ct_rendered_subframes", "ct_set_stop_when_converged", "ct_converged_at", "ct_is_converged", "ct_tonemap_buffer", "ct_is_converged_buffers", "ct_download", "ct_upload",
    "ct_buffer_bytes", "ct_copy_to_device", "ct_device_ptr", "ct_subframes", "ct_set_subframes", "ct_counters", "ct_kernel_time",
    "ct_debug_cdf_inversion", "ct_debug_math_selftest", "ct_debug_math_eval", "ct_debug_fetch_probe", "ct_debug_fetch_probe_ws", "ct_debug_track_lines", "ct_debug_touched_lines", "ct_debug_stats", "ct_debug_stats_ex", "ct_debug_suspended", "ct_debug_timeline", "ct_debug_invariants", "ct_debug_pixel_classes", "ct_debug_pixel_class_plane", "ct_debug_memory", "ct_debug_delta_grid", "ct_debug_march_meta", "ct_debug_layout", "ct_fetch_counters", "ct_calculate_camera_variables", "ct_quantize_volume", "ct_load_vdb", "ct_generate_mipmaps",
    "ct_tile_owner", "ct_shard_tiles", "ct_debug_allocations", "ct_make_procedural_cloud",
    "ct_group_create", "ct_group_destroy", "ct_group_last_error", "ct_group_size", "ct_group_handle", "ct_group_set_camera", "ct_group_set_light",
    "ct_group_render_accumulate", "ct_group_reset", "ct_group_merge", "ct_group_download", "ct_group_tonemap",
    "ct_group_is_converged", "ct_group_counters",
    "ct_group_network_create", "ct_group_network_destroy", "ct_group_network_render_accumulate",
    "ct_adaptive_frame_create_shard", "ct_group_adaptive_frame_create", "ct_group_adaptive_frame_update", "ct_group_adaptive_frame_raise_cap",
    "ct_group_adaptive_frame_info", "ct_group_adaptive_frame_shard", "ct_group_adaptive_frame_merge", "ct_group_adaptive_frame_download",
    "ct_group_adaptive_frame_device_ptr", "ct_group_adaptive_frame_destroy",
    "ct_bake_save", "ct_bake_file_info", "ct_bake_load", "ct_debug_volume_hash", "ct_bake_half", "ct_bake_format", "ct_bake_download_half",
    "ct_debug_half_round",
    "ct_group_network_bake", "ct_group_bake_traced", "ct_group_bake_traced_adaptive", "ct_group_bake_load", "ct_group_bake_update",
    "ct_group_bake_trace_more", "ct_group_bake_retrace", "ct_group_bake_trace_adaptive_more", "ct_group_bake_retrace_adaptive",
    "ct_group_bake_shard", "ct_group_bake_spans", "ct_group_baked_render_accumulate", "ct_group_bake_destroy", "ct_debug_group_bake_exchange",
    "ct_debug_bake_shard",
    "ct_baked_render_hybrid_subframe", "ct_baked_render_hybrid_accumulate", "ct_baked_render_hybrid_shard_subframe",
    "ct_baked_render_hybrid_shard_accumulate", "ct_group_baked_render_hybrid_accumulate",
]
# ... and the declared symbols whose names have digits (the list above is matched by name pattern)
DEBUG_EXPORTS = ["ct_debug_bf16_round"]
DIGIT_EXPORTS = DEBUG_EXPORTS + ["ct_bake_download_m2"]


class CtScene(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("dims", C.c_uint32 * 3),
        ("density_host", C.c_void_p),
        ("cloud_size_m", C.c_float),
        ("mean_free_path_m", C.c_float),
        ("sample_step", C.c_float),
        ("mode", C.c_int32),
        ("estimator", C.c_int32),
        ("max_depth", C.c_uint32),
        ("light_direction", C.c_float * 3),
        ("light_color", C.c_float * 3),
        ("light_intensity", C.c_float),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("mie_host", C.c_void_p),
        ("chopped_mie_host", C.c_void_p),
        ("mie_count", C.c_uint32),
        ("device", C.c_int32),
        ("shard_index", C.c_uint32),
        ("shard_count", C.c_uint32),
        ("flags", C.c_uint32),
    ]


class CtCounters(C.Structure):
    _fields_ = [
        ("paths", C.c_uint64),
        ("box_hits", C.c_uint64),
        ("density_lookups", C.c_uint64),
        ("inscatter_lookups", C.c_uint64),
        ("scatter_events", C.c_uint64),
        ("depth_capped", C.c_uint64),
    ]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class CtNetworkDesc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("blocks", C.c_uint32),
        ("width", C.c_uint32),
        ("aux", C.c_uint32),
        ("head_layers", C.c_uint32),
        ("weights_host", C.c_void_p),
        ("weight_count", C.c_size_t),
    ]


class CtNetworkRender(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("transform", C.c_int32),
        ("rgb_scale", C.c_float * 3),
        ("band_pixels", C.c_uint32),
    ]


class CtBakeDesc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("grid", C.c_uint32 * 3),
        ("azimuths", C.c_uint32),
        ("cosines", C.c_uint32),
    ]


class CtBakeInfo(C.Structure):
    _fields_ = [
        ("grid", C.c_uint32 * 3),
        ("azimuths", C.c_uint32),
        ("cosines", C.c_uint32),
        ("entries", C.c_uint64),
        ("light", C.c_float * 3),
        ("axis_a", C.c_float * 3),
        ("axis_b", C.c_float * 3),
        ("cosine", C.c_float * 64),
        ("current", C.c_uint32),
        ("gather_ms", C.c_double),
        ("network_ms", C.c_double),
    ]


class CtBakeSparseInfo(C.Structure):
    _fields_ = [
        ("sparse", C.c_uint32),
        ("margin_texels", C.c_uint32),
        ("nodes", C.c_uint64),
        ("active_nodes", C.c_uint64),
        ("probes_baked", C.c_uint64),
        ("mask_ms", C.c_double),
    ]


class CtBakeStorageInfo(C.Structure):
    _fields_ = [
        ("compact", C.c_uint32),
        ("reserved", C.c_uint32),
        ("slots", C.c_uint64),
        ("stored_entries", C.c_uint64),
        ("table_bytes", C.c_uint64),
        ("index_bytes", C.c_uint64),
    ]


class CtBakeTraceInfo(C.Structure):
    _fields_ = [
        ("traced", C.c_uint32),
        ("samples", C.c_uint32),
        ("paths", C.c_uint64),
        ("trace_ms", C.c_double),
        ("fold_ms", C.c_double),
    ]


CT_BAKE_DENSE, CT_BAKE_SPARSE, CT_BAKE_COMPACT = 0, 1, 2   # ct_bake_traced's kind


class CtBakeAdaptive(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("round_samples", C.c_uint32),
        ("max_samples", C.c_uint32),
        ("zero_samples", C.c_uint32),
        ("rel_tol", C.c_float),
        ("abs_tol", C.c_float),
    ]


class CtBakeAdaptiveInfo(C.Structure):
    _fields_ = [
        ("adaptive", C.c_uint32),
        ("round_samples", C.c_uint32),
        ("max_samples", C.c_uint32),
        ("zero_samples", C.c_uint32),
        ("rel_tol", C.c_float),
        ("abs_tol", C.c_float),
        ("rounds", C.c_uint32),
        ("reserved", C.c_uint32),
        ("entries_active", C.c_uint64),
        ("converged", C.c_uint64),
        ("capped", C.c_uint64),
        ("paths", C.c_uint64),
        ("trace_ms", C.c_double),
        ("fold_ms", C.c_double),
        ("test_ms", C.c_double),
    ]


CT_BAKE_F32, CT_BAKE_F16 = 0, 1   # a bake's format (ct_bake_format, CtBakeFileHeader.format)
CT_BAKE_FILE_MAGIC = b"CTBAKE\r\n"
CT_BAKE_FILE_VERSION = 1


class CtBakeFileHeader(C.Structure):
    _fields_ = [
        ("magic", C.c_uint8 * 8),
        ("version", C.c_uint32),
        ("header_bytes", C.c_uint32),
        ("kind", C.c_uint32),
        ("format", C.c_uint32),
        ("traced", C.c_uint32),
        ("adaptive", C.c_uint32),
        ("grid", C.c_uint32 * 3),
        ("azimuths", C.c_uint32),
        ("cosines", C.c_uint32),
        ("margin_texels", C.c_uint32),
        ("entries", C.c_uint64),
        ("stored_entries", C.c_uint64),
        ("active_nodes", C.c_uint64),
        ("light", C.c_float * 3),
        ("axis_a", C.c_float * 3),
        ("axis_b", C.c_float * 3),
        ("dims", C.c_uint32 * 3),
        ("sample_step_bits", C.c_uint32),
        ("mean_free_path_bits", C.c_uint32),
        ("cloud_size_bits", C.c_uint32),
        ("estimator", C.c_int32),
        ("tex_fixed8", C.c_uint32),
        ("light_color_bits", C.c_uint32 * 3),
        ("light_intensity_bits", C.c_uint32),
        ("samples", C.c_uint32),
        ("volume_hash", C.c_uint64),
        ("paths", C.c_uint64),
        ("round_samples", C.c_uint32),
        ("max_samples", C.c_uint32),
        ("zero_samples", C.c_uint32),
        ("rel_tol_bits", C.c_uint32),
        ("abs_tol_bits", C.c_uint32),
        ("rounds", C.c_uint32),
        ("converged", C.c_uint64),
        ("capped", C.c_uint64),
        ("reserved", C.c_uint8 * 32),
    ]


class CtBakeFileInfo(C.Structure):
    _fields_ = [
        ("header", CtBakeFileHeader),
        ("file_bytes", C.c_uint64),
        ("nodes_offset", C.c_uint64),
        ("table_offset", C.c_uint64),
        ("m2_offset", C.c_uint64),
        ("counts_offset", C.c_uint64),
        ("checksum_offset", C.c_uint64),
        ("checksum", C.c_uint64),
    ]


class CtCollectorDesc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("max_thread_count", C.c_uint32),
        ("launches_per_update", C.c_uint32),
        ("zero_samples", C.c_uint32),
        ("rel_tol", C.c_float),
        ("abs_tol", C.c_float),
    ]


class CtCollectorInfo(C.Structure):
    _fields_ = [
        ("batch", C.c_uint32),
        ("remaining", C.c_uint32),
        ("converged", C.c_uint32),
        ("updates", C.c_uint32),
        ("frame_id", C.c_uint32),
        ("repeat_count", C.c_uint32),
        ("threads", C.c_uint32),
        ("completed", C.c_uint32),
        ("paths", C.c_uint64),
        ("trace_ms", C.c_double),
        ("fold_ms", C.c_double),
        ("test_ms", C.c_double),
    ]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


CT_ADAPTIVE_MEAN, CT_ADAPTIVE_M2, CT_ADAPTIVE_COUNTS = 0, 1, 2   # ct_adaptive_frame_download / _device_ptr


class CtAdaptiveFrameDesc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("round_samples", C.c_uint32),
        ("min_samples", C.c_uint32),
        ("max_samples", C.c_uint32),
        ("rel_tol", C.c_float),
        ("abs_tol", C.c_float),
        ("chunk_pixels", C.c_uint32),
        ("pass_subframes", C.c_uint32),
    ]


class CtAdaptiveFrameInfo(C.Structure):
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("round_samples", C.c_uint32),
        ("min_samples", C.c_uint32),
        ("max_samples", C.c_uint32),
        ("rounds", C.c_uint32),
        ("rel_tol", C.c_float),
        ("abs_tol", C.c_float),
        ("pixels", C.c_uint64),
        ("live", C.c_uint64),
        ("converged", C.c_uint64),
        ("capped", C.c_uint64),
        ("paths", C.c_uint64),
        ("trace_ms", C.c_double),
        ("fold_ms", C.c_double),
        ("test_ms", C.c_double),
    ]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class CtFetchCounters(C.Structure):
    _fields_ = [("density_fetches", C.c_uint64), ("inscatter_fetches", C.c_uint64)]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class CloudTraceError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"libcloudtrace error {code}: {message}")
        self.code = code
        self.message = message


_LIB = None


def load():
    """Load the HIP library; raises if it has not been built (python -m deepestscatter_amd.build)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not LIB_PATH.exists():
        raise FileNotFoundError(
            f"{LIB_PATH} is missing: build the HIP extension with `python -m deepestscatter_amd.build` "
            "(there is no CPU fallback)")
    L = C.CDLL(str(LIB_PATH))
    vp, u32, i32, f32 = C.c_void_p, C.c_uint32, C.c_int32, C.c_float
    sig = {
        "ct_create": (i32, [C.POINTER(CtScene), C.POINTER(vp)]),
        "ct_destroy": (i32, [vp]),
        "ct_last_error": (C.c_char_p, [vp]),
        "ct_set_stream": (i32, [vp, vp]),
        "ct_set_camera": (i32, [vp, vp, vp, vp, vp]),
        "ct_set_light": (i32, [vp, vp, vp, f32]),
        "ct_render_subframe": (i32, [vp, u32, vp]),
        "ct_accumulate": (i32, [vp, u32, vp]),
        "ct_render_accumulate": (i32, [vp, u32, u32]),
        "ct_render_accumulate_async": (i32, [vp, u32, u32]),
        "ct_synchronize": (i32, [vp]),
        "ct_point_radiance_launch": (i32, [vp, vp, u32, u32, u32]),
        "ct_collector_create": (i32, [vp, C.POINTER(CtCollectorDesc), vp, vp, u32, C.POINTER(vp)]),
        "ct_collector_update": (i32, [vp, vp, u32]),
        "ct_collector_info": (i32, [vp, C.POINTER(CtCollectorInfo)]),
        "ct_collector_download": (i32, [vp, vp, vp, u32]),
        "ct_collector_destroy": (i32, [vp]),
        "ct_adaptive_frame_create": (i32, [vp, C.POINTER(CtAdaptiveFrameDesc), C.POINTER(vp)]),
        "ct_adaptive_frame_update": (i32, [vp, u32]),
        "ct_adaptive_frame_raise_cap": (i32, [vp, u32]),
        "ct_adaptive_frame_info": (i32, [vp, C.POINTER(CtAdaptiveFrameInfo)]),
        "ct_adaptive_frame_download": (i32, [vp, u32, vp, C.c_size_t]),
        "ct_adaptive_frame_device_ptr": (i32, [vp, u32, C.POINTER(vp)]),
        "ct_adaptive_frame_destroy": (i32, [vp]),
        "ct_generate_scatter_samples": (i32, [vp, u32, u32, vp, vp]),
        "ct_collect_descriptors": (i32, [vp, vp, vp, u32, vp]),
        "ct_descriptor_frame": (i32, [vp, u32, vp, u32, vp, vp, vp, vp, C.POINTER(u32)]),
        "ct_debug_descriptor_frame_time": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "ct_network_create": (i32, [vp, C.POINTER(CtNetworkDesc), C.POINTER(vp)]),
        "ct_network_destroy": (i32, [vp]),
        "ct_network_eval": (i32, [vp, vp, vp, vp, u32, vp]),
        "ct_debug_network_time": (i32, [vp, C.POINTER(C.c_double)]),
        "ct_debug_bf16_round": (f32, [f32]),
        "ct_network_render_subframe": (i32, [vp, vp, C.POINTER(CtNetworkRender), u32, vp]),
        "ct_network_render_accumulate": (i32, [vp, vp, C.POINTER(CtNetworkRender), u32, u32]),
        "ct_network_render_shard_subframe": (i32, [vp, vp, C.POINTER(CtNetworkRender), u32, vp]),
        "ct_network_render_shard_accumulate": (i32, [vp, vp, C.POINTER(CtNetworkRender), u32, u32]),
        "ct_debug_network_scratch": (i32, [vp, C.POINTER(C.c_uint64)]),
        "ct_debug_network_aux": (i32, [vp, vp, u32, vp]),
        "ct_debug_network_render_time": (i32, [vp, C.POINTER(C.c_double)]),
        "ct_network_bake": (i32, [vp, vp, C.POINTER(CtBakeDesc), C.POINTER(vp)]),
        "ct_bake_update": (i32, [vp, vp, vp]),
        "ct_bake_destroy": (i32, [vp]),
        "ct_bake_info": (i32, [vp, C.POINTER(CtBakeInfo)]),
        "ct_bake_probes": (i32, [vp, C.c_uint64, u32, vp, vp]),
        "ct_bake_download": (i32, [vp, vp, C.c_size_t]),
        "ct_debug_bake_lookup": (i32, [vp, vp, vp, vp, u32, vp]),
        "ct_network_bake_sparse": (i32, [vp, vp, C.POINTER(CtBakeDesc), C.POINTER(vp)]),
        "ct_bake_sparse_info": (i32, [vp, C.POINTER(CtBakeSparseInfo)]),
        "ct_bake_mask": (i32, [vp, vp, C.c_size_t]),
        "ct_debug_bake_mask": (i32, [vp, vp, vp, vp, vp, u32, C.POINTER(u32)]),
        "ct_network_bake_compact": (i32, [vp, vp, C.POINTER(CtBakeDesc), C.POINTER(vp)]),
        "ct_bake_storage_info": (i32, [vp, C.POINTER(CtBakeStorageInfo)]),
        "ct_bake_slots": (i32, [vp, vp, C.c_size_t]),
        "ct_bake_download_stored": (i32, [vp, vp, C.c_size_t]),
        "ct_bake_traced": (i32, [vp, C.POINTER(CtBakeDesc), u32, u32, C.POINTER(vp)]),
        "ct_bake_trace_more": (i32, [vp, vp, u32]),
        "ct_bake_retrace": (i32, [vp, vp, u32]),
        "ct_bake_trace_info": (i32, [vp, C.POINTER(CtBakeTraceInfo)]),
        "ct_bake_directions": (i32, [vp, vp, C.c_size_t]),
        "ct_bake_traced_adaptive": (i32, [vp, C.POINTER(CtBakeDesc), u32, C.POINTER(CtBakeAdaptive), C.POINTER(vp)]),
        "ct_bake_trace_adaptive_more": (i32, [vp, vp, u32]),
        "ct_bake_retrace_adaptive": (i32, [vp, vp]),
        "ct_bake_adaptive_info": (i32, [vp, C.POINTER(CtBakeAdaptiveInfo)]),
        "ct_bake_download_counts": (i32, [vp, vp, C.c_size_t]),
        "ct_bake_download_m2": (i32, [vp, vp, C.c_size_t]),
        "ct_bake_save": (i32, [vp, C.c_char_p]),
        "ct_bake_file_info": (i32, [C.c_char_p, C.POINTER(CtBakeFileInfo)]),
        "ct_bake_load": (i32, [vp, C.c_char_p, C.POINTER(vp)]),
        "ct_debug_volume_hash": (i32, [vp, C.POINTER(C.c_uint64)]),
        "ct_bake_half": (i32, [vp, vp, C.POINTER(vp)]),
        "ct_bake_format": (i32, [vp, C.POINTER(u32)]),
        "ct_bake_download_half": (i32, [vp, vp, C.c_size_t]),
        "ct_debug_half_round": (C.c_uint16, [f32]),
        "ct_baked_render_subframe": (i32, [vp, vp, C.POINTER(CtNetworkRender), u32, vp]),
        "ct_baked_render_accumulate": (i32, [vp, vp, C.POINTER(CtNetworkRender), u32, u32]),
        "ct_baked_render_shard_subframe": (i32, [vp, vp, C.POINTER(CtNetworkRender), u32, vp]),
        "ct_baked_render_shard_accumulate": (i32, [vp, vp, C.POINTER(CtNetworkRender), u32, u32]),
        "ct_debug_baked_render_time": (i32, [vp, C.POINTER(C.c_double)]),
        "ct_baked_render_hybrid_subframe": (i32, [vp, vp, C.POINTER(CtNetworkRender), u32, u32, vp]),
        "ct_baked_render_hybrid_accumulate": (i32, [vp, vp, C.POINTER(CtNetworkRender), u32, u32, u32]),
        "ct_baked_render_hybrid_shard_subframe": (i32, [vp, vp, C.POINTER(CtNetworkRender), u32, u32, vp]),
        "ct_baked_render_hybrid_shard_accumulate": (i32, [vp, vp, C.POINTER(CtNetworkRender), u32, u32, u32]),
        "ct_reset": (i32, [vp]),
        "ct_tonemap": (i32, [vp, f32, vp, C.POINTER(f32)]),
        "ct_tonemap_async": (i32, [vp, f32]),
        "ct_set_render_ahead": (i32, [vp, u32]),
        "ct_rendered_subframes": (i32, [vp, C.POINTER(u32)]),
        "ct_set_stop_when_converged": (i32, [vp, u32, u32]),
        "ct_converged_at": (i32, [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_uint64)]),
        "ct_is_converged": (i32, [vp, C.POINTER(i32), C.POINTER(C.c_uint64)]),
        "ct_tonemap_buffer": (i32, [vp, vp, f32, vp, C.POINTER(f32)]),
        "ct_is_converged_buffers": (i32, [vp, vp, vp, u32, C.POINTER(i32), C.POINTER(C.c_uint64)]),
        "ct_download": (i32, [vp, i32, vp, C.c_size_t]),
        "ct_upload": (i32, [vp, i32, vp, C.c_size_t]),
        "ct_buffer_bytes": (i32, [vp, i32, C.POINTER(C.c_size_t)]),
        "ct_copy_to_device": (i32, [vp, i32, vp, C.c_size_t]),
        "ct_copy_to_device_async": (i32, [vp, i32, vp, C.c_size_t]),
        "ct_debug_suspended": (i32, [vp, vp]),
        "ct_debug_timeline": (i32, [vp, vp, u32]),
        "ct_device_ptr": (i32, [vp, i32, C.POINTER(vp)]),
        "ct_subframes": (i32, [vp, C.POINTER(u32)]),
        "ct_set_subframes": (i32, [vp, u32]),
        "ct_counters": (i32, [vp, C.POINTER(CtCounters)]),
        "ct_kernel_time": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
        "ct_debug_cdf_inversion": (i32, [vp, u32, u32, vp]),
        "ct_debug_math_selftest": (i32, [vp, i32, vp]),
        "ct_debug_math_eval": (i32, [vp, i32, vp, u32, vp]),
        "ct_debug_stats": (i32, [vp, vp]),
        "ct_debug_stats_ex": (i32, [vp, vp, C.c_uint32]),
        "ct_debug_invariants": (i32, [vp, vp]),
        "ct_debug_pixel_classes": (i32, [vp, vp]),
        "ct_debug_pixel_class_plane": (i32, [vp, vp, C.c_size_t]),
        "ct_debug_memory": (i32, [vp, vp]),
        "ct_debug_delta_grid": (i32, [vp, vp]),
        "ct_debug_march_meta": (i32, [vp, vp, vp, C.c_size_t]),
        "ct_debug_layout": (i32, [vp, i32, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
        "ct_fetch_counters": (i32, [vp, C.POINTER(CtFetchCounters)]),
        "ct_debug_fetch_probe": (i32, [i32, u32, u32, C.POINTER(C.c_uint64)]),
        "ct_debug_fetch_probe_ws": (i32, [i32, u32, C.c_uint64, u32, C.POINTER(C.c_uint64)]),
        "ct_debug_track_lines": (i32, [vp, i32]),
        "ct_debug_touched_lines": (i32, [vp, C.POINTER(C.c_uint64), i32]),
        "ct_calculate_camera_variables": (i32, [vp, vp, vp, f32, f32, vp, vp, vp]),
        "ct_quantize_volume": (i32, [vp, vp, vp]),
        "ct_load_vdb": (i32, [C.c_char_p, vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]),
        "ct_generate_mipmaps": (i32, [vp, vp, vp, C.c_size_t, C.POINTER(u32), C.POINTER(C.c_size_t), vp]),
        "ct_debug_allocations": (i32, [C.POINTER(C.c_uint64)]),
        "ct_tile_owner": (u32, [u32, u32, u32]),
        "ct_shard_tiles": (i32, [u32, u32, u32, u32, vp, u32, C.POINTER(u32)]),
        "ct_group_create": (i32, [C.POINTER(CtScene), vp, u32, C.POINTER(vp)]),
        "ct_group_destroy": (i32, [vp]),
        "ct_group_last_error": (C.c_char_p, [vp]),
        "ct_group_size": (i32, [vp, C.POINTER(u32)]),
        "ct_group_handle": (i32, [vp, u32, C.POINTER(vp)]),
        "ct_group_set_camera": (i32, [vp, vp, vp, vp, vp]),
        "ct_group_set_light": (i32, [vp, vp, vp, f32]),
        "ct_group_render_accumulate": (i32, [vp, u32, u32]),
        "ct_group_reset": (i32, [vp]),
        "ct_group_merge": (i32, [vp]),
        "ct_group_download": (i32, [vp, i32, vp, C.c_size_t]),
        "ct_group_tonemap": (i32, [vp, f32, vp, C.POINTER(f32)]),
        "ct_group_is_converged": (i32, [vp, C.POINTER(i32), C.POINTER(C.c_uint64)]),
        "ct_group_counters": (i32, [vp, C.POINTER(CtCounters)]),
        "ct_group_network_create": (i32, [vp, C.POINTER(CtNetworkDesc), C.POINTER(vp)]),
        "ct_group_network_destroy": (i32, [vp]),
        "ct_group_network_render_accumulate": (i32, [vp, vp, C.POINTER(CtNetworkRender), u32, u32]),
        "ct_make_procedural_cloud": (i32, [u32, u32, vp]),
        "ct_adaptive_frame_create_shard": (i32, [vp, C.POINTER(CtAdaptiveFrameDesc), C.POINTER(vp)]),
        "ct_group_adaptive_frame_create": (i32, [vp, C.POINTER(CtAdaptiveFrameDesc), C.POINTER(vp)]),   # -> CtGroupAdaptiveFrame
        "ct_group_adaptive_frame_update": (i32, [vp, u32]),
        "ct_group_adaptive_frame_raise_cap": (i32, [vp, u32]),
        "ct_group_adaptive_frame_info": (i32, [vp, C.POINTER(CtAdaptiveFrameInfo)]),
        "ct_group_adaptive_frame_shard": (i32, [vp, u32, C.POINTER(vp)]),
        "ct_group_adaptive_frame_merge": (i32, [vp]),
        "ct_group_adaptive_frame_download": (i32, [vp, u32, vp, C.c_size_t]),
        "ct_group_adaptive_frame_device_ptr": (i32, [vp, u32, C.POINTER(vp)]),
        "ct_group_adaptive_frame_destroy": (i32, [vp]),
        "ct_group_network_bake": (i32, [vp, vp, C.POINTER(CtBakeDesc), u32, C.POINTER(vp)]),   # -> CtGroupBake
        "ct_group_bake_traced": (i32, [vp, C.POINTER(CtBakeDesc), u32, u32, C.POINTER(vp)]),
        "ct_group_bake_traced_adaptive": (i32, [vp, C.POINTER(CtBakeDesc), u32, C.POINTER(CtBakeAdaptive), C.POINTER(vp)]),
        "ct_group_bake_load": (i32, [vp, C.c_char_p, C.POINTER(vp)]),
        "ct_group_bake_update": (i32, [vp, vp]),
        "ct_group_bake_trace_more": (i32, [vp, u32]),
        "ct_group_bake_retrace": (i32, [vp, u32]),
        "ct_group_bake_trace_adaptive_more": (i32, [vp, u32]),
        "ct_group_bake_retrace_adaptive": (i32, [vp]),
        "ct_group_bake_shard": (i32, [vp, u32, C.POINTER(vp)]),
        "ct_group_bake_spans": (i32, [vp, vp, C.c_size_t]),
        "ct_group_baked_render_accumulate": (i32, [vp, vp, C.POINTER(CtNetworkRender), u32, u32]),
        "ct_group_baked_render_hybrid_accumulate": (i32, [vp, vp, C.POINTER(CtNetworkRender), u32, u32, u32]),
        "ct_group_bake_destroy": (i32, [vp]),
        "ct_debug_group_bake_exchange": (i32, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
        "ct_debug_bake_shard": (i32, [vp, C.POINTER(CtBakeDesc), u32, u32, C.POINTER(CtBakeAdaptive), u32, u32, C.POINTER(vp)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _LIB = L
    return L


def check(rc: int, handle=None):
    if rc != CT_OK:
        msg = load().ct_last_error(handle)
        raise CloudTraceError(rc, msg.decode("utf-8", "replace") if msg else "")
