// fspt_texpack.hip - the texture packer on the GPU: the raw atlas - RGBA8, layer-major, GL rows, the form
// fspt_scene_update_materials takes and Appearance::raw retains - made from decoded sources.
//   k_tex_resample  per layer one record: a flat colour, a res x res image copied as given, or an image resampled
//                   bilinearly (REPEAT in s, CLAMP_TO_EDGE in t), sRGB-decoded, swizzled and premultiplied
// One thread per OUTPUT texel in output order, the layer on grid.y: a wave's stores are one contiguous run of 256 bytes,
// and its four 4-byte taps are runs of two source rows (under magnification neighbouring lanes read the same texels, under
// minification a row at a fixed stride).  The two 256-entry decode tables are committed data (fspt_texpack_tables.hpp) and
// are staged once per block in LDS (2 KiB): a lane's 16 look-ups are indexed by texel bytes, which no scalar load serves.
// Float32, every operation rounded on its own (the library is built with -ffp-contract=off and nothing here is an fma):
// the statement is scene.resample_image's and fspt.js resampleImage's, op for op.  What follows the raw atlas - the flags,
// the tiling, the interleave, the hit records - is fspt_appearance.hip's, unchanged.
#include "fspt_internal.hpp"
#include "fspt_texpack_check.hpp"
#include "fspt_texpack_tables.hpp"

#include <chrono>

namespace fspt {
namespace {

const uint32_t TP_BS = 256;
__device__ const uint32_t d_tex_tables[512] = {
#define TEX_ROW8(t, r) t[r], t[r + 1], t[r + 2], t[r + 3], t[r + 4], t[r + 5], t[r + 6], t[r + 7]
#define TEX_ROW64(t, r) TEX_ROW8(t, r), TEX_ROW8(t, r + 8), TEX_ROW8(t, r + 16), TEX_ROW8(t, r + 24), TEX_ROW8(t, r + 32), TEX_ROW8(t, r + 40), TEX_ROW8(t, r + 48), TEX_ROW8(t, r + 56)
#define TEX_ALL(t) TEX_ROW64(t, 0), TEX_ROW64(t, 64), TEX_ROW64(t, 128), TEX_ROW64(t, 192)
  TEX_ALL(TEX_LIN_BITS), TEX_ALL(TEX_SRGB_BITS)
};

// one channel of a bilinear footprint: the four taps' bytes through a table, then top / bottom / across
__device__ __forceinline__ float tex_filter(const float *tab, uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, int shift, float a, float b) {
  const float na = 1.0f - a, nb = 1.0f - b;
  const float top = tab[(p00 >> shift) & 255u] * na + tab[(p01 >> shift) & 255u] * a;
  const float bot = tab[(p10 >> shift) & 255u] * na + tab[(p11 >> shift) & 255u] * a;
  return top * nb + bot * b;
}

__device__ __forceinline__ float tex_pick(float c0, float c1, float c2, float c3, uint32_t k) {
  return k == 0u ? c0 : k == 1u ? c1 : k == 2u ? c2 : c3;
}

__device__ __forceinline__ uint32_t tex_quantise(float c, float alpha) {
  const float q = floorf(c * alpha * 255.0f + 0.5f);
  return (uint32_t)fminf(fmaxf(q, 0.0f), 255.0f);
}

// raw: the atlas, res x res texels per layer; blockIdx.y = the record (rec + the launch's first); a record's layer is rec.dst
__global__ void __launch_bounds__(TP_BS) k_tex_resample(const TexLayerRec *__restrict__ rec, uint32_t res, uint32_t *__restrict__ raw) {
  __shared__ float s_tab[512]; // lin | srgb
  s_tab[threadIdx.x] = __uint_as_float(d_tex_tables[threadIdx.x]);
  s_tab[threadIdx.x + 256u] = __uint_as_float(d_tex_tables[threadIdx.x + 256u]);
  __syncthreads();
  const TexLayerRec r = rec[blockIdx.y];
  const uint32_t per_layer = res * res; // (res <= 16384: 2^28 texels at most, and a stride of 2^20 more does not wrap)
  uint32_t *dst = raw + (size_t)r.dst * per_layer;
  const uint32_t *src = (const uint32_t *)r.src;
  const uint32_t kind = r.flags & 3u;
  const float *rgb_tab = (r.flags & 4u) ? s_tab + 256 : s_tab;
  const int w = (int)r.w, h = (int)r.h;
  const float fw = (float)r.w, fh = (float)r.h, fres = (float)res;
  for (uint32_t o = blockIdx.x * TP_BS + threadIdx.x; o < per_layer; o += gridDim.x * TP_BS) {
    if (kind == (uint32_t)FSPT_TEXLAYER_COLOR) { dst[o] = r.color; continue; }
    if (kind == (uint32_t)FSPT_TEXLAYER_PIXELS) { dst[o] = src[o]; continue; }
    const uint32_t y = o / res, x = o - y * res;
    const float px = ((float)x + 0.5f) / fres, py = ((float)y + 0.5f) / fres;
    const float u = px * fw - 0.5f, v = (1.0f - py) * fh - 0.5f;
    const float fu = floorf(u), fv = floorf(v);
    const float a = u - fu, b = v - fv;
    // columns wrap: floor(u) lies in [-1, w - 1]
    const int iu = (int)fu, iv = (int)fv;
    int i0 = iu < 0 ? iu + w : iu, i1 = iu + 1 >= w ? iu + 1 - w : iu + 1;
    i0 = min(max(i0, 0), w - 1); i1 = min(max(i1, 0), w - 1); // (no index leaves the image, whatever the rounding)
    const int j0 = min(max(iv, 0), h - 1), j1 = min(max(iv + 1, 0), h - 1);
    const uint32_t *row0 = src + (size_t)j0 * r.w, *row1 = src + (size_t)j1 * r.w;
    const uint32_t p00 = row0[i0], p01 = row0[i1], p10 = row1[i0], p11 = row1[i1];
    const float c0 = tex_filter(rgb_tab, p00, p01, p10, p11, 0, a, b);
    const float c1 = tex_filter(rgb_tab, p00, p01, p10, p11, 8, a, b);
    const float c2 = tex_filter(rgb_tab, p00, p01, p10, p11, 16, a, b);
    const float c3 = tex_filter(s_tab, p00, p01, p10, p11, 24, a, b); // alpha is never decoded
    const float alpha = tex_pick(c0, c1, c2, c3, (r.flags >> 14) & 3u);
    const uint32_t R = tex_quantise(tex_pick(c0, c1, c2, c3, (r.flags >> 8) & 3u), alpha);
    const uint32_t G = tex_quantise(tex_pick(c0, c1, c2, c3, (r.flags >> 10) & 3u), alpha);
    const uint32_t B = tex_quantise(tex_pick(c0, c1, c2, c3, (r.flags >> 12) & 3u), alpha);
    dst[o] = R | (G << 8) | (B << 16) | 0xFF000000u;
  }
}

struct PackTimes { float upload_ms = 0.0f, kernel_ms = 0.0f, readback_ms = 0.0f; } g_pack_times;

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

} // namespace

hipError_t texpack_launch(Hold &hold, const fspt_texture_pack *p, bool on_device, const uint32_t *layer_ids, uint32_t *raw, hipStream_t st,
                          hipEvent_t ev_begin, uint64_t *uploaded, uint32_t *launches) {
  std::vector<TexLayerRec> rec;
  std::vector<uint64_t> src_off;
  uint64_t src_bytes = 0;
  texpack_records(p, on_device, layer_ids, rec, src_off, &src_bytes);
  void *d_src = nullptr, *d_rec = nullptr;
  hipError_t e = hold.make(&d_rec, rec.size() * sizeof(TexLayerRec));
  if (!on_device) {
    if (e == hipSuccess) e = hold.make(&d_src, src_bytes);
    for (uint32_t i = 0; e == hipSuccess && i < p->n_images; ++i)
      if (src_off[i] != UINT64_MAX) e = hipMemcpy((uint8_t *)d_src + src_off[i], p->images[i].rgba, (size_t)p->images[i].w * p->images[i].h * 4, hipMemcpyHostToDevice);
    for (uint32_t l = 0; l < p->n_layers; ++l)
      if ((rec[l].flags & 3u) != (uint32_t)FSPT_TEXLAYER_COLOR) rec[l].src += (uint64_t)(uintptr_t)d_src;
    *uploaded += src_bytes;
  }
  if (e == hipSuccess) e = hipMemcpy(d_rec, rec.data(), rec.size() * sizeof(TexLayerRec), hipMemcpyHostToDevice);
  *uploaded += rec.size() * sizeof(TexLayerRec);
  if (e == hipSuccess && ev_begin) e = hipEventRecord(ev_begin, st);
  if (e != hipSuccess) return e;
  const size_t per_layer = (size_t)p->res * p->res;
  const uint32_t bx = (uint32_t)std::min<size_t>((per_layer + TP_BS - 1) / TP_BS, 4096u);
  for (uint32_t l0 = 0; l0 < p->n_layers; l0 += 65535u) { // (grid.y <= 65535)
    const uint32_t nl = std::min<uint32_t>(p->n_layers - l0, 65535u);
    hipLaunchKernelGGL(k_tex_resample, dim3(bx, nl), dim3(TP_BS), 0, st, (const TexLayerRec *)d_rec + l0, p->res, raw);
    ++*launches;
  }
  return hipGetLastError();
}

int atlas_pack_run(const fspt_texture_pack *p, uint8_t *atlas_out) {
  const char *fn = "fspt_atlas_pack_gpu";
  Hold hold;
  void *raw = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  uint64_t uploaded = 0;
  uint32_t launches = 0;
  PackTimes t;
  const size_t bytes = (size_t)p->res * p->res * p->n_layers * 4;
  hipError_t e = hold.make(&raw, bytes);
  for (hipEvent_t &x : ev) if (e == hipSuccess) e = hipEventCreate(&x);
  auto t0 = std::chrono::steady_clock::now();
  if (e == hipSuccess) e = texpack_launch(hold, p, false, nullptr, (uint32_t *)raw, nullptr, ev[0], &uploaded, &launches);
  t.upload_ms = (float)ms_since(t0);
  if (e == hipSuccess) e = hipEventRecord(ev[1], nullptr);
  if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
  if (e == hipSuccess) e = hipEventElapsedTime(&t.kernel_ms, ev[0], ev[1]);
  t0 = std::chrono::steady_clock::now();
  if (e == hipSuccess) e = hipMemcpy(atlas_out, raw, bytes, hipMemcpyDeviceToHost);
  t.readback_ms = (float)ms_since(t0);
  if (e != hipSuccess) (void)hipDeviceSynchronize(); // (the sources outlive whatever was launched)
  for (hipEvent_t x : ev) if (x) hipEventDestroy(x);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    fspt_set_error("%s: %s", fn, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? FSPT_E_NOMEM : FSPT_E_HIP;
  }
  g_pack_times = t;
  return FSPT_OK;
}

void atlas_pack_times(float *upload_ms, float *kernel_ms, float *readback_ms) {
  if (upload_ms) *upload_ms = g_pack_times.upload_ms;
  if (kernel_ms) *kernel_ms = g_pack_times.kernel_ms;
  if (readback_ms) *readback_ms = g_pack_times.readback_ms;
}

} // namespace fspt

extern "C" int fspt_texture_decode_tables(float lin[256], float srgb[256]) {
  if (!lin || !srgb) { fspt_set_error("fspt_texture_decode_tables: NULL argument"); return FSPT_E_INVALID; }
  std::memcpy(lin, fspt::TEX_LIN_BITS, sizeof fspt::TEX_LIN_BITS);
  std::memcpy(srgb, fspt::TEX_SRGB_BITS, sizeof fspt::TEX_SRGB_BITS);
  return FSPT_OK;
}
