// fspt_pose.hip - everything that writes the refit's staging array (tri | norm) from a rest mesh the scene keeps.
// GPU part transforms (fspt_scene_set_pose / fspt_scene_update_transforms): a part id per triangle; a frame is
// one 3 x 4 matrix per part.
//   k_pose_transform   rest vertices and normal frames x their part's matrices -> the staging array
// GPU skinning (fspt_scene_set_skin / fspt_scene_update_skin): four joints and weights per triangle corner
// and optional morph targets; a frame is one 3 x 4 matrix per joint and one weight per target.
//   k_skin_transform   morph, blend, vertex and normal frame per corner -> the staging array (further down)
// Vertex-position update (fspt_scene_set_mesh / fspt_scene_update_vertices): an indexed mesh; a frame is one
// float32 position per vertex, and the normal frames are derived again by the reference's rules in float64.
//   k_mesh_faces, k_mesh_vertex_normals, k_mesh_smooth_frames   positions -> the staging array (last in this file)
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

// ---------------------------------------------------------------------------
// Vertex-position update (fspt_scene_set_mesh / fspt_scene_update_vertices; tests/mesh_ref.py restates the
// arithmetic).  A frame is pos[n_vertices][3] float32; the staging array is derived from it by obj_loader.js's rules in the
// reference's float64: every position promoted exactly, every operation the one vector.js / scene_build.cpp writes, in that
// order, no fma (-ffp-contract=off), sqrt and / correctly rounded (tests/test_mesh_gpu.py probes both), one float64 ->
// float32 conversion per output.
//   k_mesh_faces        tri = the three positions; n_f = normalize(cross(p1 - p0, p2 - p0)) to fnorm[face id] when a later
//                       pass needs it; flat triangles get their three frames here (n_0 = n_1 = n_2 = n_f: one frame, and
//                       the isNaN quirk can only replace all three); static triangles copy their rest 9 + 27 floats
//   k_mesh_vertex_normals  per vertex: total = (0,0,0) + the face normals of its incident corners in ascending rank (the
//                       CSR rows set_mesh sorted), then total * (1.0 / count); not renormalised; no atomics
//   k_mesh_smooth_frames   smooth triangles: the corner's frame from its vertex normal, then the quirk (below)
// A flat-only mesh runs the first kernel alone.
// Shape: one lane per corner, 63 corners per wave (lane 63 idles, 1.6 % of the lanes), so a wave holds 21 whole triangles and
// a corner reaches its triangle's other corners by __shfl instead of gathering their positions again or going through
// LDS.  A lane writes 12 B of tri and 36 B of norm at c * 12 / c * 36: each store instruction of a wave covers one dense
// span (756 B / 2 268 B; the spans of consecutive waves abut, so the partial lines at their ends are completed by the
// neighbour).  The per-triangle constants (24 B) and face words are read by the three lanes of a triangle from the same
// address.  What is NOT dense are the gathers by vertex index - 12 B of pos per corner in the first kernel, 24 B of vnorm per
// corner in the third, 24 B of fnorm per incident corner in the second.  Done about them: each is issued once per corner (the
// other two positions come by shuffle; the third kernel re-reads the positions from the tri it wrote, densely), and the
// per-vertex pass sums a vertex of valence 6 once, not 18 times.  Left: no reordering of vertices - a mesh whose index
// order scatters a triangle's vertices over pos pays a 64-byte sector per 12 bytes used; pos is 12 B per vertex and stays
// L2-resident between the corners that share it.
struct V3 { double x, y, z; };
__device__ inline V3 v3(double x, double y, double z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ inline V3 v_sub(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ inline V3 v_add(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ inline V3 v_scale(V3 a, double s) { return v3(a.x * s, a.y * s, a.z * s); }
__device__ inline double v_dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline V3 v_cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, -(a.x * b.z - a.z * b.x), a.x * b.y - a.y * b.x); } // vector.js:112-117
__device__ inline V3 v_normalize(V3 v) { // vector.js:6-13
  const double m = __builtin_sqrt(v.x * v.x + v.y * v.y + v.z * v.z);
  return v_scale(v, 1.0 / m);
}
__device__ inline V3 v_shfl(V3 a, int src) { return v3(__shfl(a.x, src), __shfl(a.y, src), __shfl(a.z, src)); }

// calcTangents' loop body for one corner (obj_loader.js:88-97): the pushed tangent / bitangent, whether the reference's
// isNaN test fires, and what it then assigns
struct MeshFrame { V3 t, b, ft, fb; bool nan; };
__device__ inline MeshFrame mesh_frame(V3 n, V3 pre_tangent) {
  MeshFrame f;
  const V3 pre_bt = v_normalize(v_cross(n, pre_tangent));
  f.t = v_normalize(v_cross(pre_bt, n));
  f.b = v_normalize(v_cross(n, f.t));
  const double d = v_dot(f.t, f.b);
  f.nan = d != d;
  f.ft = v_cross(n, v3(0.0, 1.0, 0.0));
  f.fb = v_cross(f.ft, n);
  return f;
}
// deltaPos0 / deltaPos1 and the triangle's constants k = (du1[1], du0[1], r) -> preTangent (obj_loader.js:85)
__device__ inline V3 mesh_pre_tangent(V3 dp0, V3 dp1, const double *k) {
  return v_normalize(v_scale(v_sub(v_scale(dp0, k[0]), v_scale(dp1, k[1])), k[2]));
}
__device__ inline void mesh_store_frame(float *o, V3 n, V3 t, V3 b) {
  o[0] = (float)n.x; o[1] = (float)n.y; o[2] = (float)n.z;
  o[3] = (float)t.x; o[4] = (float)t.y; o[5] = (float)t.z;
  o[6] = (float)b.x; o[7] = (float)b.y; o[8] = (float)b.z;
}

// corner c of the launch, 63 per wave: false for the idle lane and past the end
__device__ inline bool mesh_corner(uint32_t T, size_t *c, uint32_t *lane) {
  *lane = threadIdx.x & 63u;
  *c = ((size_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 63u + *lane;
  return *lane < 63u && *c < (size_t)T * 3;
}

__global__ __launch_bounds__(256) void k_mesh_faces(const uint32_t *__restrict__ vertex, const double *__restrict__ cst, const uint32_t *__restrict__ face,
                                                    const float *__restrict__ rest, const float *__restrict__ pos, uint32_t n_vertices, uint32_t T,
                                                    double *__restrict__ fnorm, float *__restrict__ out_tri, float *__restrict__ out_norm) {
  size_t c; uint32_t lane;
  const bool live = mesh_corner(T, &c, &lane);
  const uint32_t vi = live ? vertex[c] : FSPT_MESH_STATIC;
  const bool moves = vi < n_vertices; // (set_mesh checked the indices: a live corner is this or static)
  float p[3] = {0.0f, 0.0f, 0.0f};
  if (moves) { p[0] = pos[(size_t)vi * 3]; p[1] = pos[(size_t)vi * 3 + 1]; p[2] = pos[(size_t)vi * 3 + 2]; }
  const uint32_t i = lane % 3u; // (63 = 21 x 3: the corner's place in its triangle)
  const int b = (int)(lane - i);
  V3 q[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) q[k] = v3((double)__shfl(p[0], b + k), (double)__shfl(p[1], b + k), (double)__shfl(p[2], b + k));
  if (!live) return;
  const size_t t = c / 3;
  if (!moves) { // a static triangle: its rest copy
    if (vi != FSPT_MESH_STATIC || !rest) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) out_tri[c * 3 + k] = rest[c * 3 + k];
    const float *rn = rest + (size_t)T * 9 + c * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) out_norm[c * 9 + k] = rn[k];
    return;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) out_tri[c * 3 + k] = p[k];
  const V3 e1 = v_sub(q[1], q[0]), e2 = v_sub(q[2], q[0]);
  const V3 n = v_normalize(v_cross(e1, e2)); // obj_loader.js:40-44
  const uint32_t fw = face[t], f = fw & 0x7FFFFFFFu;
  if (fnorm && f < T) fnorm[(size_t)f * 3 + i] = i == 0 ? n.x : (i == 1 ? n.y : n.z); // (the triangle's three lanes hold the same n)
  if (fw >> 31) return; // smooth: k_mesh_smooth_frames writes its frames
  const MeshFrame fr = mesh_frame(n, mesh_pre_tangent(e1, e2, cst + t * 3));
  // the three corners share n, so they share the test: the quirk assigns all of 0..2 or none
  mesh_store_frame(out_norm + c * 9, n, fr.nan ? fr.ft : fr.t, fr.nan ? fr.fb : fr.b);
}

__global__ __launch_bounds__(256) void k_mesh_vertex_normals(const uint32_t *__restrict__ adj_off, const uint32_t *__restrict__ adj_face, uint32_t n_adj,
                                                             const double *__restrict__ fnorm, uint32_t T, uint32_t n_vertices, double *__restrict__ vnorm) {
  const size_t v = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (v >= n_vertices) return;
  const uint32_t lo = adj_off[v], hi = adj_off[v + 1];
  if (lo >= hi || hi > n_adj) return; // no incident corner: nothing reads it
  V3 total = v3(0.0, 0.0, 0.0);
  for (uint32_t k = lo; k < hi; ++k) { // obj_loader.js:46-52, in the order the faces were pushed
    const uint32_t f = adj_face[k];
    if (f >= T) return; // (set_mesh made the rows: never taken)
    total = v_add(total, v3(fnorm[(size_t)f * 3], fnorm[(size_t)f * 3 + 1], fnorm[(size_t)f * 3 + 2]));
  }
  const V3 m = v_scale(total, 1.0 / (double)(hi - lo));
  vnorm[v * 3] = m.x; vnorm[v * 3 + 1] = m.y; vnorm[v * 3 + 2] = m.z;
}

// The quirk of obj_loader.js:93-99, literally.  `triangle.tangents` starts empty; corner i pushes its tangent, and when
// its isNaN test fires it first ASSIGNS the fallback at index i (growing the array to i + 1 when it is shorter).  With f
// the first corner whose test fires, the array's entries 0..2 - what the record takes - are therefore
//   i < f: T_i      i == f: fallback_i      i > f: fallback_i if corner i's test fires, else T_(i-1) (pushed one place late)
// and the bitangents alike.  Patterns {2}, {1,2}, {0,1,2} end finite; {0}, {0,2} leave T_0's NaN at corner 1 and {1},
// {0,1} leave T_1's at corner 2, which the refit's check then refuses.
__global__ __launch_bounds__(256) void k_mesh_smooth_frames(const uint32_t *__restrict__ vertex, const double *__restrict__ cst, const uint32_t *__restrict__ face,
                                                            const double *__restrict__ vnorm, uint32_t n_vertices, uint32_t T,
                                                            const float *__restrict__ out_tri, float *__restrict__ out_norm) {
  size_t c; uint32_t lane;
  const bool live = mesh_corner(T, &c, &lane);
  const size_t t = c / 3;
  const uint32_t vi = live ? vertex[c] : FSPT_MESH_STATIC;
  const bool smooth = live && vi < n_vertices && (face[t] >> 31);
  if (!__any(smooth)) return; // (wave-uniform)
  float p[3] = {0.0f, 0.0f, 0.0f};
  if (smooth) { p[0] = out_tri[c * 3]; p[1] = out_tri[c * 3 + 1]; p[2] = out_tri[c * 3 + 2]; } // the positions k_mesh_faces copied: dense
  const uint32_t i = lane % 3u;
  const int b = (int)(lane - i);
  V3 q[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) q[k] = v3((double)__shfl(p[0], b + k), (double)__shfl(p[1], b + k), (double)__shfl(p[2], b + k));
  V3 n = v3(0.0, 0.0, 0.0);
  MeshFrame fr;
  fr.t = fr.b = fr.ft = fr.fb = n;
  fr.nan = false;
  if (smooth) {
    n = v3(vnorm[(size_t)vi * 3], vnorm[(size_t)vi * 3 + 1], vnorm[(size_t)vi * 3 + 2]);
    fr = mesh_frame(n, mesh_pre_tangent(v_sub(q[1], q[0]), v_sub(q[2], q[0]), cst + t * 3));
  }
  V3 et = fr.t, eb = fr.b; // entry i of the arrays when no test fired before corner i
  if (__any(fr.nan)) { // (wave-uniform; rare)
    const int fired = fr.nan ? 1 : 0;
    const int n0 = __shfl(fired, b), n1 = __shfl(fired, b + 1), n2 = __shfl(fired, b + 2);
    const int prev = lane ? (int)lane - 1 : 0;
    const V3 pt = v_shfl(fr.t, prev), pb = v_shfl(fr.b, prev);
    const uint32_t first = n0 ? 0u : (n1 ? 1u : (n2 ? 2u : 3u));
    if (fr.nan) { et = fr.ft; eb = fr.fb; }   // i == first, or a later corner whose own test fires
    else if (i > first) { et = pt; eb = pb; } // the push of corner i - 1, one place late
  }
  if (smooth) mesh_store_frame(out_norm + c * 9, n, et, eb);
}

// f64 sqrt (op 0) and / (op 1) as this file's kernels compile them (fspt_f64_probe_eval)
__global__ __launch_bounds__(256) void k_f64_probe(int op, const double *__restrict__ a, const double *__restrict__ b, uint32_t n, double *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  out[i] = op == 0 ? __builtin_sqrt(a[i]) : a[i] / b[i];
}

} // namespace

uint32_t mesh_run(const fspt_scene::Mesh &M, uint32_t T, const float *pos, float *stage, hipEvent_t *between) {
  if (!T) return 0;
  hipStream_t st = nullptr;
  const size_t waves = ((size_t)T * 3 + 62) / 63;
  const uint32_t blocks = (uint32_t)((waves + 3) / 4);
  float *out_tri = stage, *out_norm = stage + (size_t)T * 9;
  const bool smooth = M.adj_off != nullptr;
  hipLaunchKernelGGL(k_mesh_faces, dim3(blocks), dim3(256), 0, st, M.vertex, M.cst, M.face, M.rest, pos, M.n_vertices, T, smooth ? M.fnorm : nullptr, out_tri, out_norm);
  if (!smooth) return 1;
  if (between) (void)hipEventRecord(between[0], st);
  hipLaunchKernelGGL(k_mesh_vertex_normals, dim3((M.n_vertices + 255u) / 256u), dim3(256), 0, st, M.adj_off, M.adj_face, M.n_adj, M.fnorm, T, M.n_vertices, M.vnorm);
  if (between) (void)hipEventRecord(between[1], st);
  hipLaunchKernelGGL(k_mesh_smooth_frames, dim3(blocks), dim3(256), 0, st, M.vertex, M.cst, M.face, M.vnorm, M.n_vertices, T, out_tri, out_norm);
  return 3;
}

int f64_probe_run(int op, const double *a, const double *b, uint32_t n, double *out) {
  double *d = nullptr;
  HIP_TRY(hipMalloc((void **)&d, (size_t)n * 24));
  struct Free { double *p; ~Free() { hipFree(p); } } guard{d};
  HIP_TRY(hipMemcpy(d, a, (size_t)n * 8, hipMemcpyHostToDevice));
  if (op == 1) HIP_TRY(hipMemcpy(d + n, b, (size_t)n * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_f64_probe, dim3((n + 255u) / 256u), dim3(256), 0, nullptr, op, d, d + n, n, d + 2 * (size_t)n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, d + 2 * (size_t)n, (size_t)n * 8, hipMemcpyDeviceToHost));
  return FSPT_OK;
}

int g_skin_form = SKIN_FORM; // the shipped joint-table form, or fspt_skin_set_form's

uint32_t skin_run(fspt_scene *s, const float *xf, const float *morph_w) {
  const fspt_scene::Skin &K = s->skin;
  const uint32_t T = s->n_tris;
  const bool lds = g_skin_form == 1 && (size_t)K.n_joints * 48 <= SKIN_LDS_MAX_BYTES;
  const uint32_t blocks = (uint32_t)(((size_t)T * 3 + 255) / 256);
  hipStream_t st = nullptr;
  if (blocks) {
    if (K.has_norm) { if (K.n_morph) skin_launch<true, true>(lds, blocks, st, K, xf, morph_w, T, s->rf.stage); else skin_launch<true, false>(lds, blocks, st, K, xf, morph_w, T, s->rf.stage); }
    else { if (K.n_morph) skin_launch<false, true>(lds, blocks, st, K, xf, morph_w, T, s->rf.stage); else skin_launch<false, false>(lds, blocks, st, K, xf, morph_w, T, s->rf.stage); }
  }
  return blocks ? 1u : 0u;
}

int skin_upload(fspt_scene::Skin &K, const float *xf, const float *morph_w) {
  HIP_TRY(hipMemcpy(K.frame, xf, (size_t)K.n_joints * 48, hipMemcpyHostToDevice));
  if (K.n_morph) HIP_TRY(hipMemcpy(K.frame + (size_t)K.n_joints * 12, morph_w, (size_t)K.n_morph * 4, hipMemcpyHostToDevice));
  return FSPT_OK;
}

uint32_t pose_run(fspt_scene *s) {
  const fspt_scene::Pose &P = s->pose;
  const uint32_t T = s->n_tris, BS = 256;
  const size_t n = (size_t)T * (P.has_norm ? 12 : 3);
  hipStream_t st = nullptr;
  if (n)
    hipLaunchKernelGGL(k_pose_transform, dim3((uint32_t)((n + BS - 1) / BS)), dim3(BS), 0, st, P.rest, P.has_norm ? P.rest + (size_t)T * 9 : nullptr,
                       P.part, P.mats, T, P.n_parts, s->rf.stage, s->rf.stage + (size_t)T * 9);
  return n ? 1u : 0u;
}

int pose_upload(fspt_scene::Pose &P, const float *mats_host) {
  if (P.mats_cap < P.n_parts) {
    hipFree(P.mats); P.mats = nullptr; P.mats_cap = 0;
    HIP_TRY(hipMalloc((void **)&P.mats, (size_t)P.n_parts * 30 * 4));
    P.mats_cap = P.n_parts;
  }
  HIP_TRY(hipMemcpy(P.mats, mats_host, (size_t)P.n_parts * 30 * 4, hipMemcpyHostToDevice));
  return FSPT_OK;
}

// The arrays of each deformer, in the order a rebuild permutes them (ids and float64 constants go as words).  The mesh's
// vertex -> face rows and the face normals they index are in face ids, which a rebuild does not change: they do not follow.
std::vector<DeformArray> deform_arrays(fspt_scene::Pose &P, size_t T) {
  return {{(void **)&P.part, T, {1u, 0u}, 1, true}, {(void **)&P.rest, T, {9u, P.has_norm ? 27u : 0u}, 1, true}, {(void **)&P.mats, P.mats_cap, {30u, 0u}, 1, false}};
}

std::vector<DeformArray> deform_arrays(fspt_scene::Skin &K, size_t T) {
  return {{(void **)&K.joints, T, {6u, 0u}, 1, true}, {(void **)&K.weights, T, {12u, 0u}, 1, true}, {(void **)&K.rest, T, {9u, K.has_norm ? 27u : 0u}, 1, true},
          {(void **)&K.morph, T, {9u, 0u}, K.n_morph, true}, {(void **)&K.morph_norm, T, {27u, 0u}, K.n_morph, true},
          {(void **)&K.frame, 1, {K.n_joints * 12u + K.n_morph, 0u}, 1, false}};
}

std::vector<DeformArray> deform_arrays(fspt_scene::Mesh &M, size_t T) {
  const size_t nv = M.n_vertices;
  return {{(void **)&M.vertex, T, {3u, 0u}, 1, true}, {(void **)&M.cst, T, {6u, 0u}, 1, true}, {(void **)&M.face, T, {1u, 0u}, 1, true}, {(void **)&M.rest, T, {9u, 27u}, 1, true},
          {(void **)&M.pos, nv, {3u, 0u}, 1, false}, {(void **)&M.adj_off, nv + 1, {1u, 0u}, 1, false}, {(void **)&M.adj_face, M.n_adj ? M.n_adj : 1u, {1u, 0u}, 1, false},
          {(void **)&M.fnorm, T, {6u, 0u}, 1, false}, {(void **)&M.vnorm, nv, {6u, 0u}, 1, false}};
}

uint64_t deform_bytes(const std::vector<DeformArray> &arrays) {
  uint64_t bytes = 0;
  for (const DeformArray &a : arrays) if (*a.p) bytes += (uint64_t)a.rows * (a.span[0] + a.span[1]) * 4u * a.slices;
  return bytes;
}

static void arrays_free(const std::vector<DeformArray> &arrays) { for (const DeformArray &a : arrays) hipFree(*a.p); }

void mesh_release(fspt_scene::Mesh &M) { arrays_free(deform_arrays(M, 0)); M = fspt_scene::Mesh(); }

void deformer_release(fspt_scene *s, fspt_scene::StageOwner who) {
  if (who == fspt_scene::STAGE_POSE) { arrays_free(deform_arrays(s->pose, 0)); s->pose = fspt_scene::Pose(); }
  if (who == fspt_scene::STAGE_SKIN) { arrays_free(deform_arrays(s->skin, 0)); s->skin = fspt_scene::Skin(); }
  if (who == fspt_scene::STAGE_MESH) mesh_release(s->mesh);
  stage_disown(s, who);
}

} // namespace fspt
