// fspt_camera.hip - ray generation under an opt-in camera model (fspt_target_set_camera_model).
//   k_camera_model<SMP, MODEL>   one tick's rays (fspt_camera_model.hpp model_ray) into the target's ray buffers
// The pinhole camera is fused into the path kernels (camera_ray, fspt_kernels.hip); every other model runs here, once per
// tick, in front of the existing single-tick trace from the ray buffers.
// Shape: one thread per pixel of the target in row order, 256-thread blocks; a lane stores two float4 (pos, dir), so a
// wave's stores are two contiguous 1 KB runs.  Nothing is loaded from memory but the kernel arguments, nothing is shared
// between lanes: no LDS.  Pixels outside the viewport are not written, as in k_camera.  The model and the sampler are
// template parameters chosen by the launcher: no switch in the kernel.
#include "fspt_camera_model.hpp"

namespace fspt {
namespace {

template <int SMP, int MODEL>
__global__ __launch_bounds__(256) void k_camera_model(uint32_t W, uint32_t H, uint32_t vw, uint32_t vh, CameraP cam, CameraModelP cm,
                                                      float randBase, uint32_t sseed, uint32_t sample, float4 *__restrict__ pos,
                                                      float4 *__restrict__ dir) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= W * H) return;
  const uint32_t x = i % W, y = i / W;
  if (x >= vw || y >= vh) return; // outside the viewport: the ray buffers keep what they hold
  fm::V3 o, d;
  model_ray<SMP, MODEL>(x, y, W, H, cam, cm, randBase, sseed, sample, o, d);
  pos[i] = make_float4(o.x, o.y, o.z, 1.0f);
  dir[i] = make_float4(d.x, d.y, d.z, 1.0f);
}

template <int SMP>
hipError_t launch_model(const CameraModelP &cm, dim3 g, dim3 b, hipStream_t stream, uint32_t W, uint32_t H, uint32_t vw, uint32_t vh,
                        const CameraP &cam, float rb, uint32_t sseed, uint32_t sample, float4 *pos, float4 *dir) {
  switch (cm.model) {
    case CAM_ORTHO: hipLaunchKernelGGL((k_camera_model<SMP, CAM_ORTHO>), g, b, 0, stream, W, H, vw, vh, cam, cm, rb, sseed, sample, pos, dir); break;
    case CAM_FISHEYE: hipLaunchKernelGGL((k_camera_model<SMP, CAM_FISHEYE>), g, b, 0, stream, W, H, vw, vh, cam, cm, rb, sseed, sample, pos, dir); break;
    case CAM_EQUIRECT: hipLaunchKernelGGL((k_camera_model<SMP, CAM_EQUIRECT>), g, b, 0, stream, W, H, vw, vh, cam, cm, rb, sseed, sample, pos, dir); break;
    case CAM_STEREO: hipLaunchKernelGGL((k_camera_model<SMP, CAM_STEREO>), g, b, 0, stream, W, H, vw, vh, cam, cm, rb, sseed, sample, pos, dir); break;
    default: return hipErrorInvalidValue; // (the pinhole camera has no kernel here; a missing model is an error)
  }
  return hipGetLastError();
}

} // namespace

hipError_t launch_camera_model(uint32_t W, uint32_t H, uint32_t vw, uint32_t vh, const CameraP &cam, const CameraModelP &cm, float rand_base,
                               float4 *pos, float4 *dir, hipStream_t stream, uint32_t sampler, uint32_t smp_seed, uint32_t sample) {
  const uint32_t n = W * H;
  if (n == 0) return hipSuccess;
  const dim3 g((n + 255u) / 256u), b(256);
  // (the reference sampler takes no seed and no sample number)
  if (sampler == 1u) return launch_model<1>(cm, g, b, stream, W, H, vw, vh, cam, rand_base, smp_seed, sample, pos, dir);
  if (sampler == 0u) return launch_model<0>(cm, g, b, stream, W, H, vw, vh, cam, rand_base, 0u, 0u, pos, dir);
  return hipErrorInvalidValue;
}

} // namespace fspt
