"""ctypes binding of libfspt.so (include/fspt.h, include/fspt_tuning.h).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc, gfx950).
There is no fallback: if the shared object is missing this module raises, and
every device entry point raises ``FsptError`` when no HIP device is present.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FSPT_LIB") or os.path.join(_HERE, "libfspt.so")  # FSPT_LIB: A/B builds of the same ABI
ABI_VERSION = 4  # include/fspt.h FSPT_ABI_VERSION this binding was written against (tests/test_abi.py pins the two)


class FsptError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libfspt error {code}: {msg}")
        self.code = code


class SceneDesc(C.Structure):
    _fields_ = [
        ("bvh", C.POINTER(C.c_float)), ("n_nodes", C.c_uint32),
        ("tri", C.POINTER(C.c_float)), ("n_tris", C.c_uint32),
        ("mat", C.POINTER(C.c_float)),
        ("norm", C.POINTER(C.c_float)),
        ("uv", C.POINTER(C.c_float)),
        ("atlas", C.POINTER(C.c_uint8)), ("atlas_res", C.c_uint32), ("atlas_layers", C.c_uint32),
        ("env", C.POINTER(C.c_uint8)), ("env_w", C.c_uint32), ("env_h", C.c_uint32),
        ("bins", C.POINTER(C.c_uint32)), ("n_bins", C.c_uint32),
        ("leaf_size", C.c_uint32),
    ]


class CameraParams(C.Structure):
    _fields_ = [
        ("P", C.c_float * 3), ("I", C.c_float * 3), ("fov_scale", C.c_float),
        ("lens", C.c_float * 2), ("env_theta", C.c_float), ("num_bounces", C.c_uint32),
    ]


class DenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float)]


class TemporalParams(C.Structure):
    _fields_ = [("alpha", C.c_float), ("max_history", C.c_float), ("depth_tol", C.c_float), ("normal_cos", C.c_float)]


class ExposureParams(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("key", "low", "high", "adapt_up", "adapt_down", "min_log2", "max_log2")]


class ExposureState(C.Structure):
    _fields_ = [("exposure", C.c_float), ("valid", C.c_uint32), ("metered", C.c_uint32), ("reserved", C.c_uint32),
                ("log2_exposure", C.c_double), ("log2_mean", C.c_double)]


class BloomParams(C.Structure):
    _fields_ = [("intensity", C.c_float), ("scatter", C.c_float), ("levels", C.c_uint32)]


class CameraModelParams(C.Structure):
    _fields_ = [("model", C.c_int), ("angle", C.c_float), ("ipd", C.c_float)]


class SkinDesc(C.Structure):
    """fspt_skin_desc: host pointers"""
    _fields_ = [("joints", C.POINTER(C.c_uint16)), ("weights", C.POINTER(C.c_float)), ("n_joints", C.c_uint32),
                ("tri", C.POINTER(C.c_float)), ("norm", C.POINTER(C.c_float)), ("morph", C.POINTER(C.c_float)),
                ("morph_norm", C.POINTER(C.c_float)), ("n_morph", C.c_uint32)]


class MeshDesc(C.Structure):
    """fspt_mesh_desc: host pointers"""
    _fields_ = [("vertex", C.POINTER(C.c_uint32)), ("n_vertices", C.c_uint32), ("uv", C.POINTER(C.c_double)),
                ("smooth", C.POINTER(C.c_uint8)), ("rank", C.POINTER(C.c_uint32)), ("tri", C.POINTER(C.c_float)), ("norm", C.POINTER(C.c_float))]


MESH_STATIC = 0xFFFFFFFF


class SkyParams(C.Structure):
    """fspt_sky_params"""
    _fields_ = [("sun_dir", C.c_float * 3), ("turbidity", C.c_float), ("sun_intensity", C.c_float), ("sun_radius", C.c_float),
                ("gain", C.c_float), ("ground_albedo", C.c_float * 3), ("view_samples", C.c_uint32), ("light_samples", C.c_uint32)]


class TextureImage(C.Structure):
    """fspt_texture_image: RGBA8, row 0 = top; host memory, or the scene's device memory in the _device entries"""
    _fields_ = [("rgba", C.c_void_p), ("w", C.c_uint32), ("h", C.c_uint32)]


class TextureLayer(C.Structure):
    _fields_ = [("kind", C.c_int32), ("color", C.c_float * 3), ("image", C.c_uint32), ("corrected", C.c_uint32), ("swizzle", C.c_uint8 * 4)]


class TexturePack(C.Structure):
    _fields_ = [("images", C.POINTER(TextureImage)), ("n_images", C.c_uint32), ("layers", C.POINTER(TextureLayer)), ("n_layers", C.c_uint32),
                ("res", C.c_uint32)]


TEXLAYER_COLOR, TEXLAYER_IMAGE, TEXLAYER_PIXELS = 0, 1, 2


class JpegParams(C.Structure):
    """fspt_jpeg_params: quality 1..100, subsampling 0 = 4:4:4 / 1 = 4:2:0, MCUs per restart interval (0 = one MCU row)"""
    _fields_ = [("quality", C.c_uint32), ("subsampling", C.c_uint32), ("restart_mcus", C.c_uint32)]


class PngParams(C.Structure):
    """fspt_png_params: channels 3 = RGB / 4 = RGBA, filter 0..4 or 5 = adaptive, bytes of the filtered stream per deflate chunk (0 = FSPT_PNG_CHUNK)"""
    _fields_ = [("channels", C.c_uint32), ("filter", C.c_uint32), ("chunk_bytes", C.c_uint32)]


class ExrParams(C.Structure):
    """fspt_exr_params: compression 0 = none / 2 = ZIPS / 3 = ZIP, pixel type 1 = HALF / 2 = FLOAT, layer bits (1 alpha, 2 albedo, 4 normal, 8 depth), bytes of a block's predicted stream per deflate chunk (0 = FSPT_EXR_CHUNK)"""
    _fields_ = [("compression", C.c_uint32), ("pixel_type", C.c_uint32), ("layers", C.c_uint32), ("chunk_bytes", C.c_uint32)]


class ExrMattes(C.Structure):
    """fspt_exr_mattes, by kind (0 object, 1 material): the ranks (W*H*12 floats), the manifest's bytes and their length"""
    _fields_ = [("ranks", C.c_void_p * 2), ("manifest", C.c_char_p * 2), ("manifest_len", C.c_size_t * 2)]


class AdaptiveParams(C.Structure):
    _fields_ = [("target_rel_mse", C.c_double), ("max_ticks", C.c_uint32), ("min_ticks", C.c_uint32), ("round_ticks", C.c_uint32)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("samples", "rays", "steps", "leaves", "shades", "env_lookups")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class PropDesc(C.Structure):
    _fields_ = [
        ("rotate", C.POINTER(C.c_double)), ("n_rotate", C.c_uint32),
        ("scale", C.c_double), ("translate", C.c_double * 3),
        ("normals_mode", C.c_uint32),
        ("diffuse_layer", C.c_double), ("emissive_layer", C.c_double),
        ("normal_layer", C.c_double), ("mr_layer", C.c_double),
        ("emittance", C.c_double * 3),
        ("ior", C.c_double), ("dielectric", C.c_double),
    ]


class WorldTransform(C.Structure):
    _fields_ = [
        ("rotate", C.POINTER(C.c_double)), ("n_rotate", C.c_uint32), ("has_rotate", C.c_uint32),
        ("translate", C.c_double * 3), ("has_translate", C.c_uint32),
    ]


class GroupMaterial(C.Structure):
    _fields_ = [
        ("diffuse_layer", C.c_double), ("emissive_layer", C.c_double),
        ("normal_layer", C.c_double), ("mr_layer", C.c_double),
        ("emittance", C.c_double * 3),
        ("ior", C.c_double), ("dielectric", C.c_double),
    ]


# every symbol include/fspt.h declares: name -> (restype, argtypes)
_VP = C.c_void_p
_F = C.POINTER(C.c_float)
_U32 = C.POINTER(C.c_uint32)
SIGNATURES = {
    "fspt_scene_create": (C.c_int, [C.POINTER(SceneDesc), C.c_int, C.POINTER(_VP)]),
    "fspt_scene_destroy": (C.c_int, [_VP]),
    "fspt_set_texture_interleave_budget": (C.c_int, [C.c_uint64]),
    "fspt_scene_depth": (C.c_int, [_VP, _U32]),
    "fspt_scene_update_geometry": (C.c_int, [_VP, _F, _F]),
    "fspt_scene_update_geometry_device": (C.c_int, [_VP, _VP, _VP]),
    "fspt_scene_sah_cost": (C.c_int, [_VP, C.POINTER(C.c_double)]),
    "fspt_scene_last_update_ms": (C.c_int, [_VP, _F, _U32]),
    "fspt_multi_update_geometry": (C.c_int, [_VP, _F, _F]),
    "fspt_scene_set_pose": (C.c_int, [_VP, _U32, C.c_uint32, _F, _F]),
    "fspt_scene_update_transforms": (C.c_int, [_VP, _F, C.c_uint32]),
    "fspt_multi_set_pose": (C.c_int, [_VP, _U32, C.c_uint32, _F, _F]),
    "fspt_multi_update_transforms": (C.c_int, [_VP, _F, C.c_uint32]),
    "fspt_scene_read_pose": (C.c_int, [_VP, _F, _F]),
    "fspt_scene_last_pose_ms": (C.c_int, [_VP, _F, _F, _U32]),
    "fspt_pose_matrices_eval": (C.c_int, [_F, C.c_uint32, _F, _U32]),
    "fspt_scene_set_skin": (C.c_int, [_VP, C.POINTER(SkinDesc)]),
    "fspt_scene_update_skin": (C.c_int, [_VP, _F, C.c_uint32, _F, C.c_uint32]),
    "fspt_scene_update_skin_device": (C.c_int, [_VP, _VP, C.c_uint32, _VP, C.c_uint32]),
    "fspt_multi_set_skin": (C.c_int, [_VP, C.POINTER(SkinDesc)]),
    "fspt_multi_update_skin": (C.c_int, [_VP, _F, C.c_uint32, _F, C.c_uint32]),
    "fspt_scene_read_skin": (C.c_int, [_VP, _F, _F]),
    "fspt_scene_last_skin_ms": (C.c_int, [_VP, _F, _F, _U32, C.POINTER(C.c_uint64)]),
    "fspt_skin_check_eval": (C.c_int, [C.POINTER(SkinDesc), C.c_uint32, C.POINTER(C.c_uint64)]),
    "fspt_skin_set_form": (C.c_int, [C.c_int]),
    "fspt_scene_set_mesh": (C.c_int, [_VP, C.POINTER(MeshDesc)]),
    "fspt_scene_update_vertices": (C.c_int, [_VP, _F, C.c_uint32]),
    "fspt_scene_update_vertices_device": (C.c_int, [_VP, _VP, C.c_uint32]),
    "fspt_multi_set_mesh": (C.c_int, [_VP, C.POINTER(MeshDesc)]),
    "fspt_multi_update_vertices": (C.c_int, [_VP, _F, C.c_uint32]),
    "fspt_scene_read_mesh": (C.c_int, [_VP, _F, _F]),
    "fspt_scene_last_mesh_ms": (C.c_int, [_VP, _F, _F, _U32, C.POINTER(C.c_uint64)]),
    "fspt_scene_last_mesh_pass_ms": (C.c_int, [_VP, _F]),
    "fspt_mesh_frames_eval": (C.c_int, [C.c_int, C.POINTER(MeshDesc), C.c_uint32, _F, _F, _F]),
    "fspt_f64_probe_eval": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_double)]),
    "fspt_builder_get_mesh": (C.c_int, [_VP, _U32, C.POINTER(C.c_double), _U32, _F]),
    "fspt_logic_set_stash": (C.c_int, [C.c_int]),
    "fspt_scene_rebuild_geometry": (C.c_int, [_VP, _F, _F, _U32]),
    "fspt_scene_rebuild_geometry_device": (C.c_int, [_VP, _VP, _VP, _VP]),
    "fspt_scene_last_rebuild_ms": (C.c_int, [_VP, _F, _F, _F, _U32, _U32]),
    "fspt_multi_rebuild_geometry": (C.c_int, [_VP, _F, _F, _U32]),
    "fspt_scene_update_materials": (C.c_int, [_VP, _F, _F, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32]),
    "fspt_scene_update_environment": (C.c_int, [_VP, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, _U32, C.c_uint32]),
    "fspt_multi_update_materials": (C.c_int, [_VP, _F, _F, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32]),
    "fspt_multi_update_environment": (C.c_int, [_VP, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, _U32, C.c_uint32]),
    "fspt_texture_decode_tables": (C.c_int, [_F, _F]),
    "fspt_atlas_pack_gpu": (C.c_int, [C.c_int, C.POINTER(TexturePack), C.POINTER(C.c_uint8)]),
    "fspt_atlas_pack_last_ms": (C.c_int, [_F, _F, _F]),
    "fspt_texture_pack_check_eval": (C.c_int, [C.POINTER(TexturePack), _U32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "fspt_scene_update_textures": (C.c_int, [_VP, _F, _F, C.POINTER(TexturePack)]),
    "fspt_scene_update_textures_device": (C.c_int, [_VP, _F, _F, C.POINTER(TexturePack)]),
    "fspt_scene_patch_textures": (C.c_int, [_VP, _U32, C.c_uint32, C.POINTER(TexturePack)]),
    "fspt_scene_patch_textures_device": (C.c_int, [_VP, _U32, C.c_uint32, C.POINTER(TexturePack)]),
    "fspt_multi_update_textures": (C.c_int, [_VP, _F, _F, C.POINTER(TexturePack)]),
    "fspt_multi_patch_textures": (C.c_int, [_VP, _U32, C.c_uint32, C.POINTER(TexturePack)]),
    "fspt_scene_read_appearance": (C.c_int, [_VP, C.c_int, _VP, C.c_uint64, C.POINTER(C.c_uint64)]),
    "fspt_scene_last_appearance_ms": (C.c_int, [_VP, _F, _U32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fspt_texset_classify_eval": (C.c_int, [_F, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8), _U32, _U32, _U32, _U32, C.c_uint32]),
    "fspt_target_create": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.POINTER(_VP)]),
    "fspt_target_destroy": (C.c_int, [_VP]),
    "fspt_target_set_viewport": (C.c_int, [_VP, C.c_uint32, C.c_uint32]),
    "fspt_target_set_sampler": (C.c_int, [_VP, C.c_int, C.c_uint32]),
    "fspt_target_get_sampler": (C.c_int, [_VP, C.POINTER(C.c_int), _U32]),
    "fspt_target_set_lights": (C.c_int, [_VP, C.c_int, C.c_float]),
    "fspt_target_get_lights": (C.c_int, [_VP, C.POINTER(C.c_int), _F]),
    "fspt_scene_light_count": (C.c_int, [_VP, _U32]),
    "fspt_target_set_shard": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.c_uint32]),
    "fspt_target_bind_accumulator": (C.c_int, [_VP, _VP]),
    "fspt_target_accumulator": (C.c_int, [_VP, C.POINTER(_VP)]),
    "fspt_target_size": (C.c_int, [_VP, _U32, _U32]),
    "fspt_camera": (C.c_int, [_VP, _F, _F, C.c_float, _F, C.c_float]),
    "fspt_set_rays": (C.c_int, [_VP, _F, _F]),
    "fspt_read_rays": (C.c_int, [_VP, _F, _F]),
    "fspt_set_rays_device": (C.c_int, [_VP, _VP, _VP]),
    "fspt_target_set_camera_model": (C.c_int, [_VP, C.POINTER(CameraModelParams)]),
    "fspt_target_get_camera_model": (C.c_int, [_VP, C.POINTER(CameraModelParams)]),
    "fspt_camera_model_time": (C.c_int, [_VP, C.POINTER(CameraParams), C.c_uint32, _F]),
    "fspt_trace": (C.c_int, [_VP, C.c_uint32, C.c_float, C.c_float, C.c_uint32]),
    "fspt_trace_test": (C.c_int, [_VP, C.c_uint32]),
    "fspt_render": (C.c_int, [_VP, C.POINTER(CameraParams), C.c_uint32, C.c_uint32, C.c_uint64]),
    "fspt_render_adaptive": (C.c_int, [_VP, C.POINTER(CameraParams), C.POINTER(AdaptiveParams), C.c_uint64]),
    "fspt_read_sample_counts": (C.c_int, [_VP, _U32]),
    "fspt_adaptive_last_stats": (C.c_int, [_VP, _U32, C.POINTER(C.c_uint64), C.POINTER(C.c_double), _U32, C.c_uint32]),
    "fspt_rand_base_next": (C.c_float, [C.POINTER(C.c_uint64)]),
    "fspt_clear": (C.c_int, [_VP]),
    "fspt_sync": (C.c_int, [_VP]),
    "fspt_read_radiance": (C.c_int, [_VP, _F]),
    "fspt_draw": (C.c_int, [_VP, C.c_float, C.c_float, C.c_int, C.c_float, C.POINTER(C.c_uint8)]),
    "fspt_draw_scaled": (C.c_int, [_VP, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_uint8)]),
    "fspt_present": (C.c_int, [_VP, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)]),
    "fspt_features": (C.c_int, [_VP, C.POINTER(CameraParams), C.c_uint32, C.c_uint64]),
    "fspt_read_features": (C.c_int, [_VP, _F]),
    "fspt_denoise": (C.c_int, [_VP, C.POINTER(DenoiseParams), _F]),
    "fspt_draw_denoised": (C.c_int, [_VP, C.c_float, C.c_float, C.POINTER(C.c_uint8)]),
    "fspt_temporal_accumulate": (C.c_int, [_VP, C.POINTER(CameraParams), C.POINTER(TemporalParams), _F]),
    "fspt_temporal_reset": (C.c_int, [_VP]),
    "fspt_temporal_denoise": (C.c_int, [_VP, C.POINTER(DenoiseParams), _F]),
    "fspt_temporal_draw": (C.c_int, [_VP, C.c_float, C.c_float, C.c_int, C.POINTER(C.c_uint8)]),
    "fspt_temporal_read_gbuffer": (C.c_int, [_VP, _F, _F]),
    "fspt_temporal_last_ms": (C.c_int, [_VP, _F]),
    "fspt_temporal_eval": (C.c_int, [C.c_int, _F, _F, _F, _F, _F, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(TemporalParams), _F]),
    "fspt_scene_slot_triangles": (C.c_int, [_VP, _U32, _U32]),
    "fspt_temporal_set_moments": (C.c_int, [_VP, C.c_int]),
    "fspt_temporal_denoise_variance": (C.c_int, [_VP, C.POINTER(DenoiseParams), _F]),
    "fspt_temporal_read_variance": (C.c_int, [_VP, _F, _F]),
    "fspt_svgf_last_ms": (C.c_int, [_VP, _F]),
    "fspt_svgf_eval": (C.c_int, [C.c_int, _F, _F, _F, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(DenoiseParams), _F, _F, _F]),
    "fspt_temporal_set_clamp": (C.c_int, [_VP, C.c_int, C.c_float, C.c_float]),
    "fspt_temporal_read_fast": (C.c_int, [_VP, _F]),
    "fspt_temporal_clamp_last_ms": (C.c_int, [_VP, _F]),
    "fspt_temporal_clamp_eval": (C.c_int, [C.c_int, _F, _F, C.c_uint32, C.c_uint32, C.c_float, _F, _F, _F]),
    "fspt_target_set_auto_exposure": (C.c_int, [_VP, C.c_int, C.POINTER(ExposureParams)]),
    "fspt_exposure_reset": (C.c_int, [_VP]),
    "fspt_exposure_get": (C.c_int, [_VP, _F, _F, _U32]),
    "fspt_exposure_last_ms": (C.c_int, [_VP, _F]),
    "fspt_exposure_last_draw_ms": (C.c_int, [_VP, _F]),
    "fspt_exposure_set_form": (C.c_int, [C.c_int]),
    "fspt_exposure_eval": (C.c_int, [C.c_int, _F, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(ExposureParams),
                                     C.POINTER(ExposureState), _U32, C.POINTER(ExposureState)]),
    "fspt_target_set_bloom": (C.c_int, [_VP, C.c_int, C.POINTER(BloomParams)]),
    "fspt_target_get_bloom": (C.c_int, [_VP, C.POINTER(C.c_int), C.POINTER(BloomParams)]),
    "fspt_bloom_eval": (C.c_int, [C.c_int, _F, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(BloomParams), _U32, _F, _F, _F, _F]),
    "fspt_bloom_texels": (C.c_uint64, [C.c_uint32, C.c_uint32, C.c_uint32, _U32]),
    "fspt_bloom_set_form": (C.c_int, [C.c_int]),
    "fspt_bloom_set_tail_texels": (C.c_int, [C.c_uint32]),
    "fspt_bloom_last_ms": (C.c_int, [_VP, _F]),
    "fspt_scene_motion_begin": (C.c_int, [_VP]),
    "fspt_scene_motion_end": (C.c_int, [_VP]),
    "fspt_intersect": (C.c_int, [_VP, _F, C.c_uint32, _F, C.POINTER(C.c_int32), _U32, _U32]),
    "fspt_intersect_form": (C.c_int, [_VP, C.c_int, _F, C.c_uint32, _F, C.POINTER(C.c_int32), _U32, _U32]),
    "fspt_scene_two_level_nodes": (C.c_int, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    "fspt_target_set_node_form": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, C.c_int64]),
    "fspt_enable_counters": (C.c_int, [_VP, C.c_int]),
    "fspt_get_counters": (C.c_int, [_VP, C.POINTER(Counters)]),
    "fspt_counters_reset": (C.c_int, [_VP]),
    "fspt_get_trace_lds_steps": (C.c_int, [_VP, C.POINTER(C.c_uint64)]),
    "fspt_math_eval": (C.c_int, [C.c_int, C.c_int, _F, _F, C.c_uint32, _F]),
    "fspt_sampler_eval": (C.c_int, [C.c_int, C.c_uint32, _U32, _U32, _U32, C.c_uint32, _F]),
    "fspt_denoise_eval": (C.c_int, [C.c_int, _F, _F, C.c_uint32, C.c_uint32, C.POINTER(DenoiseParams), _F]),
    "fspt_scene_light_table": (C.c_int, [_VP, _U32, _U32, _U32, _F, _F, _U32, _U32, _F, _U32]),
    "fspt_light_sample_eval": (C.c_int, [_VP, _F, C.c_uint32, C.POINTER(C.c_int32), _F]),
    "fspt_light_alias_table": (C.c_int, [_F, C.c_uint32, _F, _U32]),
    "fspt_scene_set_light_builder": (C.c_int, [_VP, C.c_int]),
    "fspt_scene_get_light_builder": (C.c_int, [_VP, C.POINTER(C.c_int)]),
    "fspt_light_alias_table_gpu": (C.c_int, [C.c_int, _F, C.c_uint32, _F, _U32, _F]),
    "fspt_scene_light_build_stats": (C.c_int, [_VP, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _F]),
    "fspt_last_kernel_ms": (C.c_int, [_VP, _F, _U32]),
    "fspt_target_set_pipeline": (C.c_int, [_VP, C.c_int, C.c_uint32]),
    "fspt_target_set_primary_form": (C.c_int, [_VP, C.c_int]),
    "fspt_target_get_primary_form": (C.c_int, [_VP, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "fspt_target_set_pool": (C.c_int, [_VP, C.c_uint32, C.c_int, C.c_uint32, C.c_int]),
    "fspt_target_set_trace_budget": (C.c_int, [_VP, C.c_uint32]),
    "fspt_last_stage_ms": (C.c_int, [_VP, _F, _U32]),
    "fspt_target_set_stage_timing": (C.c_int, [_VP, C.c_int]),
    "fspt_target_prepare": (C.c_int, [_VP]),
    "fspt_target_set_tail": (C.c_int, [_VP, C.c_int]),
    "fspt_target_set_deferred": (C.c_int, [_VP, C.c_int]),
    "fspt_target_live_paths": (C.c_int, [_VP, C.POINTER(C.c_double), C.c_uint32]),
    "fspt_target_set_memory_limit": (C.c_int, [_VP, C.c_uint64]),
    "fspt_target_path_state_bytes": (C.c_int, [_VP, C.POINTER(C.c_uint64), _U32]),
    "fspt_multi_create": (C.c_int, [C.POINTER(SceneDesc), C.POINTER(C.c_int), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_VP)]),
    "fspt_multi_destroy": (C.c_int, [_VP]),
    "fspt_multi_target": (C.c_int, [_VP, C.c_uint32, C.POINTER(_VP)]),
    "fspt_multi_camera": (C.c_int, [_VP, _F, _F, C.c_float, _F, C.c_float]),
    "fspt_multi_trace": (C.c_int, [_VP, C.c_uint32, C.c_float, C.c_float, C.c_uint32]),
    "fspt_multi_render": (C.c_int, [_VP, C.POINTER(CameraParams), C.c_uint32, C.c_uint32, C.c_uint64]),
    "fspt_multi_clear": (C.c_int, [_VP]),
    "fspt_multi_sync": (C.c_int, [_VP]),
    "fspt_multi_read_radiance": (C.c_int, [_VP, _F]),
    "fspt_multi_draw": (C.c_int, [_VP, C.c_float, C.c_float, C.c_int, C.c_float, C.POINTER(C.c_uint8)]),
    "fspt_multi_last_gather_bytes": (C.c_int, [_VP, C.POINTER(C.c_uint64)]),
    "fspt_multi_size": (C.c_int, [_VP, _U32, _U32]),
    "fspt_multi_peer_access": (C.c_int, [_VP, C.c_uint32, C.POINTER(C.c_int)]),
    "fspt_multi_set_exchange": (C.c_int, [_VP, C.c_int]),
    "fspt_multi_get_exchange": (C.c_int, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fspt_target_shard_slots": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    "fspt_target_pack_tiles": (C.c_int, [_VP, _VP, C.c_uint32]),
    "fspt_target_unpack_tiles": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint32, C.c_uint32]),
    "fspt_builder_create": (C.c_int, [C.POINTER(_VP)]),
    "fspt_builder_destroy": (C.c_int, [_VP]),
    "fspt_builder_add_obj": (C.c_int, [_VP, C.c_char_p, C.c_size_t, C.POINTER(PropDesc)]),
    "fspt_builder_parse_obj": (C.c_int, [_VP, C.c_char_p, C.c_size_t, C.POINTER(PropDesc), C.POINTER(WorldTransform),
                                         C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32, _U32]),
    "fspt_builder_group_info": (C.c_int, [_VP, C.c_uint32, C.POINTER(C.c_char_p), _U32, C.POINTER(C.c_int32)]),
    "fspt_builder_mtllib_name": (C.c_int, [_VP, C.c_uint32, C.POINTER(C.c_char_p)]),
    "fspt_builder_commit_obj": (C.c_int, [_VP, C.POINTER(GroupMaterial), C.c_uint32]),
    "fspt_builder_normalize": (C.c_int, [_VP, C.c_double]),
    "fspt_builder_build": (C.c_int, [_VP, C.c_uint32]),
    "fspt_builder_build_gpu": (C.c_int, [_VP, C.c_uint32, C.c_int]),
    "fspt_builder_gpu_stats": (C.c_int, [_VP, _F, _U32, _U32]),
    "fspt_builder_tri_order": (C.c_int, [_VP, _U32]),
    "fspt_builder_geometry": (C.c_int, [_VP, _U32, _F, _F, _F, _F]),
    "fspt_builder_counts": (C.c_int, [_VP, _U32, _U32, _U32]),
    "fspt_builder_autofocus": (C.c_int, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "fspt_builder_get": (C.c_int, [_VP, _F, _F, _F, _F, _F]),
    "fspt_env_bins": (C.c_int, [C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, _U32, C.c_uint32, _U32]),
    "fspt_env_bins_gpu": (C.c_int, [C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, C.c_int, _U32, C.c_uint32, _U32]),
    "fspt_sky_generate": (C.c_int, [C.c_int, C.POINTER(SkyParams), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8), _F]),
    "fspt_scene_update_environment_auto": (C.c_int, [_VP, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32]),
    "fspt_scene_update_environment_device": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint32]),
    "fspt_scene_update_sky": (C.c_int, [_VP, C.POINTER(SkyParams), C.c_uint32, C.c_uint32]),
    "fspt_scene_last_sky_ms": (C.c_int, [_VP, _F, _F, _F, _U32, _U32, _U32]),
    "fspt_multi_update_environment_auto": (C.c_int, [_VP, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32]),
    "fspt_multi_update_sky": (C.c_int, [_VP, C.POINTER(SkyParams), C.c_uint32, C.c_uint32]),
    "fspt_env_box_sums_eval": (C.c_int, [C.c_int, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, _U32, C.c_uint32, C.POINTER(C.c_double)]),
    "fspt_jpeg_bound": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(JpegParams), C.POINTER(C.c_size_t)]),
    "fspt_jpeg_encode": (C.c_int, [C.c_int, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, C.c_int, C.POINTER(JpegParams), C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t)]),
    "fspt_jpeg_encode_device": (C.c_int, [C.c_int, _VP, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(JpegParams), C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t)]),
    "fspt_jpeg_coefficients_eval": (C.c_int, [C.c_int, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, C.c_int, C.POINTER(JpegParams), C.POINTER(C.c_int16)]),
    "fspt_jpeg_last_ms": (C.c_int, [_F, C.POINTER(C.c_uint64)]),
    "fspt_draw_jpeg": (C.c_int, [_VP, C.c_int, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float, C.POINTER(JpegParams), C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t)]),
    "fspt_present_jpeg": (C.c_int, [_VP, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float, C.POINTER(JpegParams), C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32)]),
    "fspt_png_bound": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(PngParams), C.POINTER(C.c_size_t)]),
    "fspt_png_encode": (C.c_int, [C.c_int, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, C.c_int, C.POINTER(PngParams), C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t)]),
    "fspt_png_encode_device": (C.c_int, [C.c_int, _VP, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(PngParams), C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t)]),
    "fspt_png_filtered_eval": (C.c_int, [C.c_int, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, C.c_int, C.POINTER(PngParams), C.POINTER(C.c_uint8)]),
    "fspt_png_last_ms": (C.c_int, [_F, C.POINTER(C.c_uint64)]),
    "fspt_draw_png": (C.c_int, [_VP, C.c_int, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float, C.POINTER(PngParams), C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t)]),
    "fspt_exr_bound": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(ExrParams), C.POINTER(C.c_size_t)]),
    "fspt_exr_encode": (C.c_int, [C.c_int, _F, _F, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(ExrParams), C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t)]),
    "fspt_exr_encode_device": (C.c_int, [C.c_int, _VP, _VP, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(ExrParams), C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t)]),
    "fspt_exr_set_form": (C.c_int, [C.c_int]),
    "fspt_exr_last_ms": (C.c_int, [_F, C.POINTER(C.c_uint64)]),
    "fspt_draw_exr": (C.c_int, [_VP, C.c_int, C.POINTER(ExrParams), C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t)]),
    "fspt_matte_hash": (C.c_uint32, [C.c_char_p, C.c_size_t]),
    "fspt_scene_set_matte_ids": (C.c_int, [_VP, C.c_int, _U32]),
    "fspt_scene_set_matte_manifest": (C.c_int, [_VP, C.c_int, C.c_char_p, C.c_size_t]),
    "fspt_mattes": (C.c_int, [_VP, C.POINTER(CameraParams), C.c_uint32, C.c_uint64]),
    "fspt_read_mattes": (C.c_int, [_VP, C.c_int, _F]),
    "fspt_mattes_lost": (C.c_int, [_VP, C.c_int, C.POINTER(C.c_uint64)]),
    "fspt_exr_bound_mattes": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(ExrParams), C.POINTER(ExrMattes), C.POINTER(C.c_size_t)]),
    "fspt_exr_encode_mattes": (C.c_int, [C.c_int, _F, _F, C.POINTER(ExrMattes), C.c_uint32, C.c_uint32, C.c_int, C.POINTER(ExrParams), C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t)]),
    "fspt_exr_encode_mattes_device": (C.c_int, [C.c_int, _VP, _VP, C.POINTER(ExrMattes), C.c_uint32, C.c_uint32, C.c_int, C.POINTER(ExrParams), C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t)]),
    "fspt_multi_last_stage_ms": (C.c_int, [_VP, _F, C.c_uint32]),
    "fspt_device_memory": (C.c_int, [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fspt_last_error": (C.c_char_p, []),
    "fspt_abi_version": (C.c_int, []),
    "fspt_device_count": (C.c_int, []),
}

_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm bundles its own libamdhip64 (same soname as /opt/rocm's, but
    libtorch_hip asks for it by file name): if libfspt pulled in /opt/rocm's copy first, a later `import torch`
    would load a second runtime and find "No HIP GPUs".  Loading torch's copy first (without importing torch)
    makes both bind to the same one, whatever the import order; bound accumulators (torch tensors) then live
    in the runtime that launches the kernels."""
    if os.environ.get("FSPT_OWN_HIP_RUNTIME"):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec and spec.submodule_search_locations:
            path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
            if os.path.exists(path):
                C.CDLL(path, mode=C.RTLD_GLOBAL)
    except Exception:
        pass  # no torch: libfspt uses the system runtime


def lib():
    """Load libfspt.so (once).  Raises if the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FsptError(-100, f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _share_hip_runtime_with_torch()
        l = C.CDLL(LIB_PATH)
        try:
            l.fspt_abi_version.restype = C.c_int
            have = l.fspt_abi_version()
        except AttributeError:
            have = None
        if have != ABI_VERSION:
            raise FsptError(-101, f"{LIB_PATH} has ABI version {have}, this binding needs {ABI_VERSION}: stale build - "
                                  "run `python -c 'import __graft_entry__ as g; g.build()'`")
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc):
    if rc != 0:
        raise FsptError(rc, lib().fspt_last_error().decode("utf-8", "replace"))


def fptr(a):
    return a.ctypes.data_as(_F)


def u32ptr(a):
    return a.ctypes.data_as(_U32)


def u8ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))
