// fspt_pose.hip - GPU part transforms (fspt_scene_set_pose / fspt_scene_update_transforms): the scene keeps a
// rest mesh and a part id per triangle; a frame is one 3 x 4 matrix per part.
//   k_pose_transform   rest vertices and normal frames x their part's matrices -> the refit's staging array (tri | norm)
// What the refit (fspt_refit.hip refit_run) is then fed is that staging array: the kernel below is the "deformation kernel"
// fspt_scene_update_geometry_device was designed for.
// Arithmetic (the contract of DESIGN 2: float32, an fma exactly where one is written; tests/pose_ref.py restates it):
//   vertex   p'_c = fma(a_c2, z, fma(a_c1, y, fma(a_c0, x, t_c)))
//   t, bt    d'_c = fma(D_c2, z, fma(D_c1, y, D_c0 * x))          D = float32(A / g),       g = sqrt(sum of squares / 3)
//   n        the same with N                                      N = float32(cof(A) / g^2)
// D and N come from the host in float64 (fspt_api.cpp pose_matrices); nothing is normalised here.
// Shape: one work item per float3.  The vectors of tri (3 T) and of norm (9 T) are numbered one array after the other, so a
// wave's 64 lanes read one contiguous 768-byte span and write another one: its three dword loads touch the same six
// 128-byte lines, every byte of which the wave uses (the second and third load hit what the first brought into the L1),
// and nothing is fetched twice from the L2.  A thread per triangle would stride by 144 bytes.  No LDS: staging the span
// there would make each instruction dense at the price of two LDS round trips and a barrier for a kernel that moves 292
// bytes per triangle once.  The 30 matrix floats of a part are read through the scalar / L1 path of whoever shares the
// part: triangles of one prop are neighbours in leaf order far more often than not.
#include "fspt_internal.hpp"

namespace fspt {
namespace {

__global__ __launch_bounds__(256) void k_pose_transform(const float *__restrict__ rest_tri, const float *__restrict__ rest_norm,
                                                        const uint32_t *__restrict__ part, const float *__restrict__ mats, uint32_t T,
                                                        uint32_t n_parts, float *__restrict__ out_tri, float *__restrict__ out_norm) {
  const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nv = (size_t)T * 3, nf = rest_norm ? (size_t)T * 9 : 0;
  if (id >= nv + nf) return;
  const bool vert = id < nv;
  const size_t w = vert ? id : id - nv;       // vector w of its array
  const uint32_t t = (uint32_t)(vert ? w / 3 : w / 9);
  const uint32_t p = part[t];
  if (p >= n_parts) return;                   // (set_pose checked the ids: never taken)
  const float *m = mats + (size_t)p * 30;
  const float *src = (vert ? rest_tri : rest_norm) + w * 3;
  float *dst = (vert ? out_tri : out_norm) + w * 3;
  const float x = src[0], y = src[1], z = src[2];
  if (vert) {
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c] = __fmaf_rn(m[4 * c + 2], z, __fmaf_rn(m[4 * c + 1], y, __fmaf_rn(m[4 * c], x, m[4 * c + 3])));
  } else {
    const float *d = m + ((uint32_t)(w % 9) % 3 == 0 ? 21 : 12); // frame vector j of its triangle: j % 3 == 0 is the normal
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c] = __fmaf_rn(d[3 * c + 2], z, __fmaf_rn(d[3 * c + 1], y, d[3 * c] * x));
  }
}

} // namespace

void pose_release(fspt_scene *s) {
  fspt_scene::Pose &P = s->pose;
  hipFree(P.part); hipFree(P.rest); hipFree(P.mats);
  for (hipEvent_t &e : P.ev) if (e) { hipEventDestroy(e); e = nullptr; }
  P = fspt_scene::Pose();
}

int pose_run(fspt_scene *s, const float *mats_host) {
  fspt_scene::Pose &P = s->pose;
  const uint32_t T = s->n_tris, BS = 256;
  if (P.mats_cap < P.n_parts) {
    hipFree(P.mats); P.mats = nullptr; P.mats_cap = 0;
    HIP_TRY(hipMalloc((void **)&P.mats, (size_t)P.n_parts * 30 * 4));
    P.mats_cap = P.n_parts;
  }
  for (hipEvent_t &e : P.ev) if (!e) HIP_TRY(hipEventCreate(&e));
  HIP_TRY(hipMemcpy(P.mats, mats_host, (size_t)P.n_parts * 30 * 4, hipMemcpyHostToDevice));
  const size_t n = (size_t)T * (P.has_norm ? 12 : 3);
  hipStream_t st = nullptr;
  HIP_TRY(hipEventRecord(P.ev[0], st));
  if (n)
    hipLaunchKernelGGL(k_pose_transform, dim3((uint32_t)((n + BS - 1) / BS)), dim3(BS), 0, st, P.rest, P.has_norm ? P.rest + (size_t)T * 9 : nullptr,
                       P.part, P.mats, T, P.n_parts, s->rf.stage, s->rf.stage + (size_t)T * 9);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(P.ev[1], st));
  HIP_TRY(hipEventSynchronize(P.ev[1]));
  HIP_TRY(hipEventElapsedTime(&P.last_ms, P.ev[0], P.ev[1]));
  P.posed = true;
  return FSPT_OK;
}

} // namespace fspt
