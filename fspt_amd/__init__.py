"""fspt_amd — MI355X-native path-trace hot path of apbodnar/FSPT.

Product code only: the HIP kernels + C ABI (csrc/, libfspt.so), the ctypes
binding (_lib), the host mirror of the reference's frame driver (tracer) and
the scene assembly helpers (scene).  Nothing here imports oracle/.
"""
from ._lib import FsptError, lib  # noqa: F401
from .scene import SceneArrays, build_scene, bunny_scene, BUNNY_CAMERA  # noqa: F401
from .tracer import MultiPathTracer, PathTracer, Scene, bloom_eval, bloom_set_form, bloom_set_tail_texels, bytes_per_sample, denoise_eval, device_memory, exposure_eval, exposure_set_form, exr_bound, exr_encode, exr_last_ms, exr_set_form, jpeg_bound, jpeg_coefficients_eval, jpeg_encode, jpeg_last_ms, light_alias_table, light_alias_table_gpu, logic_set_stash, matte_hash, matte_manifest, png_bound, png_encode, png_filtered_eval, png_last_ms, sampler_eval, set_texture_interleave_budget, skin_set_form, svgf_eval, temporal_clamp_eval, temporal_eval  # noqa: F401
