// fspt_pose.hip - everything that writes the refit's staging array (tri | norm) from a rest mesh the scene keeps.
// GPU part transforms (fspt_scene_set_pose / fspt_scene_update_transforms): a part id per triangle; a frame is
// one 3 x 4 matrix per part.
//   k_pose_transform   rest vertices and normal frames x their part's matrices -> the staging array
// GPU skinning (fspt_scene_set_skin / fspt_scene_update_skin): four joints and weights per triangle corner
// and optional morph targets; a frame is one 3 x 4 matrix per joint and one weight per target.
//   k_skin_transform   morph, blend, vertex and normal frame per corner -> the staging array (further down)
// What the refit (fspt_refit.hip refit_run) is then fed is that staging array: the kernel below is the "deformation kernel"
// fspt_scene_update_geometry_device was designed for.
// Arithmetic (the contract of DESIGN 2: float32, an fma exactly where one is written; tests/pose_ref.py restates it):
//   vertex   p'_c = fma(a_c2, z, fma(a_c1, y, fma(a_c0, x, t_c)))
//   t, bt    d'_c = fma(D_c2, z, fma(D_c1, y, D_c0 * x))          D = float32(A / g),       g = sqrt(sum of squares / 3)
//   n        the same with N                                      N = float32(cof(A) / g^2)
// D and N come from the host in float64 (fspt_scene_update.cpp pose_matrices); nothing is normalised here.
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

// ---------------------------------------------------------------------------
// k_skin_transform (tests/skin_ref.py restates the arithmetic).  Per corner c (3 T of them), float32, an fma
// exactly where one is written:
//   morph    r = fma(w_m, morph_m, r) for m = 0 .. n_morph - 1 in order, the frame vectors alike with morph_norm
//   blend    B_e = w_0 J0_e, then fma(w_k, Jk_e, B_e) for k = 1, 2, 3            (12 entries, row-major 3 x 4)
//   vertex   p'_i = fma(B_i2, z, fma(B_i1, y, fma(B_i0, x, B_i3)))
//   frame    q = B00 B00, fma(B_ij, B_ij, q) over the other eight in row-major order; g2 = q / 3; ig = 1 / sqrt(g2); ig2 = 1 / g2
//            C = the signed cofactors, C_ij = fma(B_i1j1, B_i2j2, -(B_i1j2 B_i2j1))
//            t, bt    d'_i = fma(B_i2, z, fma(B_i1, y, B_i0 x)) ig;     n    the same with C and ig2
// Nothing is normalised; a blend that collapses (q == 0) gives inf / NaN, which the refit's check refuses.
// Shape: one work item per corner - B is blended once and serves the vertex and its three frame vectors.  A lane reads 8
// bytes of joint ids, 16 of weights, 12 of rest vertex and 36 of rest frame, and writes 12 + 36: lane after lane these
// are contiguous, so every load and store of a wave covers one dense span (512 B to 2 304 B) and no byte is fetched
// twice.  The morph slices ([n_morph][T][9] / [27]) are read the same way, target after target; the morph weights are
// uniform (scalar loads).  What is NOT dense is the joint table: 48 bytes per joint, four joints per lane, as three
// 16-byte loads each.  JT_LDS = false reads it where it is (n_joints x 48 bytes: 768 B to 3 MB, L1 / L2 resident after
// the first touch); JT_LDS = true stages it once per block in LDS (fspt_skin_set_form; the bits are the same).
template <bool NORM, bool MORPH, bool JT_LDS>
__global__ __launch_bounds__(256) void k_skin_transform(const uint2 *__restrict__ joints, const float4 *__restrict__ weights,
                                                        const float *__restrict__ rest_tri, const float *__restrict__ rest_norm,
                                                        const float *__restrict__ morph, const float *__restrict__ morph_norm,
                                                        const float *__restrict__ morph_w, uint32_t n_morph, const float4 *__restrict__ xf,
                                                        uint32_t n_joints, uint32_t T, float *__restrict__ out_tri, float *__restrict__ out_norm) {
  extern __shared__ float4 jt_lds[];
  if (JT_LDS) {
    for (uint32_t i = threadIdx.x; i < n_joints * 3u; i += 256u) jt_lds[i] = xf[i];
    __syncthreads();
  }
  const size_t c = (size_t)blockIdx.x * 256u + threadIdx.x;
  const size_t nc = (size_t)T * 3;
  if (c >= nc) return;
  const uint2 jj = joints[c];
  const uint32_t id[4] = {jj.x & 0xFFFFu, jj.x >> 16, jj.y & 0xFFFFu, jj.y >> 16};
  if (id[0] >= n_joints || id[1] >= n_joints || id[2] >= n_joints || id[3] >= n_joints) return; // (set_skin checked the ids: never taken)
  const float4 w4 = weights[c];
  const float w[4] = {w4.x, w4.y, w4.z, w4.w};
  float r[3], f[9];
#pragma unroll
  for (int k = 0; k < 3; ++k) r[k] = rest_tri[c * 3 + k];
  if (NORM) {
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = rest_norm[c * 9 + k];
  }
  if (MORPH) {
    const float *mp = morph + c * 3, *mn = NORM && morph_norm ? morph_norm + c * 9 : nullptr;
    for (uint32_t m = 0; m < n_morph; ++m, mp += nc * 3) {
      const float wm = morph_w[m];
#pragma unroll
      for (int k = 0; k < 3; ++k) r[k] = __fmaf_rn(wm, mp[k], r[k]);
      if (NORM && mn) {
#pragma unroll
        for (int k = 0; k < 9; ++k) f[k] = __fmaf_rn(wm, mn[k], f[k]);
        mn += nc * 9;
      }
    }
  }
  float B[12];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float4 *J = (JT_LDS ? (const float4 *)jt_lds : xf) + (size_t)id[k] * 3;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float4 row = J[i];
      const float e[4] = {row.x, row.y, row.z, row.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) B[4 * i + j] = k == 0 ? w[0] * e[j] : __fmaf_rn(w[k], e[j], B[4 * i + j]);
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) out_tri[c * 3 + i] = __fmaf_rn(B[4 * i + 2], r[2], __fmaf_rn(B[4 * i + 1], r[1], __fmaf_rn(B[4 * i], r[0], B[4 * i + 3])));
  if (NORM) {
    float q = B[0] * B[0];
#pragma unroll
    for (int e = 1; e < 9; ++e) { const float b = B[4 * (e / 3) + e % 3]; q = __fmaf_rn(b, b, q); }
    const float g2 = q / 3.0f;
    const float ig = 1.0f / __builtin_sqrtf(g2), ig2 = 1.0f / g2; // (fspt_math.hpp's sqrt_: correctly rounded)
    float Cf[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
        Cf[3 * i + j] = __fmaf_rn(B[4 * i1 + j1], B[4 * i2 + j2], -(B[4 * i1 + j2] * B[4 * i2 + j1]));
      }
    float o[9];
#pragma unroll
    for (int v = 0; v < 3; ++v) { // the corner's n, t, bt
      const float x = f[3 * v], y = f[3 * v + 1], z = f[3 * v + 2];
#pragma unroll
      for (int i = 0; i < 3; ++i)
        o[3 * v + i] = v == 0 ? __fmaf_rn(Cf[3 * i + 2], z, __fmaf_rn(Cf[3 * i + 1], y, Cf[3 * i] * x)) * ig2
                              : __fmaf_rn(B[4 * i + 2], z, __fmaf_rn(B[4 * i + 1], y, B[4 * i] * x)) * ig;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) out_norm[c * 9 + k] = o[k];
  }
}

template <bool NORM, bool MORPH>
void skin_launch(bool lds, uint32_t blocks, hipStream_t st, const fspt_scene::Skin &K, const float *xf, const float *mw, uint32_t T, float *stage) {
  const float *rn = NORM ? K.rest + (size_t)T * 9 : nullptr;
  if (lds)
    hipLaunchKernelGGL((k_skin_transform<NORM, MORPH, true>), dim3(blocks), dim3(256), (size_t)K.n_joints * 48, st, (const uint2 *)K.joints, (const float4 *)K.weights,
                       K.rest, rn, K.morph, K.morph_norm, mw, K.n_morph, (const float4 *)xf, K.n_joints, T, stage, stage + (size_t)T * 9);
  else
    hipLaunchKernelGGL((k_skin_transform<NORM, MORPH, false>), dim3(blocks), dim3(256), 0, st, (const uint2 *)K.joints, (const float4 *)K.weights,
                       K.rest, rn, K.morph, K.morph_norm, mw, K.n_morph, (const float4 *)xf, K.n_joints, T, stage, stage + (size_t)T * 9);
}

} // namespace

int g_skin_form = SKIN_FORM; // the shipped joint-table form, or fspt_skin_set_form's

void skin_release(fspt_scene *s) {
  fspt_scene::Skin &K = s->skin;
  hipFree(K.joints); hipFree(K.weights); hipFree(K.rest); hipFree(K.morph); hipFree(K.morph_norm); hipFree(K.frame);
  for (hipEvent_t &e : K.ev) if (e) { hipEventDestroy(e); e = nullptr; }
  K = fspt_scene::Skin();
}

int skin_run(fspt_scene *s, const float *xf, const float *morph_w, bool on_device) {
  fspt_scene::Skin &K = s->skin;
  const uint32_t T = s->n_tris;
  for (hipEvent_t &e : K.ev) if (!e) HIP_TRY(hipEventCreate(&e));
  if (!on_device) { // the frame goes to the skin's own buffer: n_joints x 12 floats | n_morph weights
    HIP_TRY(hipMemcpy(K.frame, xf, (size_t)K.n_joints * 48, hipMemcpyHostToDevice));
    if (K.n_morph) HIP_TRY(hipMemcpy(K.frame + (size_t)K.n_joints * 12, morph_w, (size_t)K.n_morph * 4, hipMemcpyHostToDevice));
    xf = K.frame; morph_w = K.frame + (size_t)K.n_joints * 12;
  }
  const bool lds = g_skin_form == 1 && (size_t)K.n_joints * 48 <= SKIN_LDS_MAX_BYTES;
  const uint32_t blocks = (uint32_t)(((size_t)T * 3 + 255) / 256);
  hipStream_t st = nullptr;
  HIP_TRY(hipEventRecord(K.ev[0], st));
  if (blocks) {
    if (K.has_norm) { if (K.n_morph) skin_launch<true, true>(lds, blocks, st, K, xf, morph_w, T, s->rf.stage); else skin_launch<true, false>(lds, blocks, st, K, xf, morph_w, T, s->rf.stage); }
    else { if (K.n_morph) skin_launch<false, true>(lds, blocks, st, K, xf, morph_w, T, s->rf.stage); else skin_launch<false, false>(lds, blocks, st, K, xf, morph_w, T, s->rf.stage); }
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(K.ev[1], st));
  HIP_TRY(hipEventSynchronize(K.ev[1]));
  HIP_TRY(hipEventElapsedTime(&K.last_ms, K.ev[0], K.ev[1]));
  K.skinned = true;
  s->pose.posed = false; // (the staging array no longer holds a pose's output)
  return FSPT_OK;
}

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
  s->skin.skinned = false; // (the staging array no longer holds a skin's output)
  return FSPT_OK;
}

} // namespace fspt
