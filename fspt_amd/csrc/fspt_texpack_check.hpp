// fspt_texpack_check.hpp - the host side of the texture packer that needs no device: the argument checks of
// fspt_atlas_pack_gpu / fspt_scene_update_textures / fspt_scene_patch_textures, and a description's per-layer records as the
// kernel reads them.  Plain C++ over include/fspt.h, so that a stand-alone program can run it under a sanitizer
// (tools/texpack_sanitize.sh).
#pragma once
#include "../../include/fspt.h"

#include <cmath>
#include <cstdint>
#include <vector>

void fspt_set_error(const char *fmt, ...);

namespace fspt {

static const uint32_t TEX_MAX_SIDE = 16384u;

// What k_tex_resample reads per layer.  flags: bits 0-1 the kind, bit 2 corrected, bits 8-15 the swizzle (2 bits per
// output channel).  src: an offset in bytes into the uploaded sources (host form) until texpack_run makes it a pointer.
struct TexLayerRec {
  uint64_t src;
  uint32_t w, h, flags, color;
  uint32_t dst, pad; // the layer of the raw atlas it writes
};

// A flat colour's texel: floor(min(max(c, 0), 1) * 255 + 0.5) per channel in float64, alpha 255 (both hosts' get_pixels)
inline uint32_t tex_color_texel(const float c[3]) {
  uint32_t px = 0xFF000000u;
  for (int k = 0; k < 3; ++k) {
    const double v = std::floor(std::fmin(std::fmax((double)c[k], 0.0), 1.0) * 255.0 + 0.5);
    px |= (uint32_t)v << (8 * k);
  }
  return px;
}

// FSPT_E_INVALID with the error set, or FSPT_OK.  on_device: the images' pointers are device memory (alignment is all
// that is looked at).  layer_ids / n_ids: a patch's layers (NULL: a whole atlas) against a retained atlas of raw_layers
// layers of raw_res^2 texels.
inline int texpack_check(const char *fn, const fspt_texture_pack *p, bool on_device, const uint32_t *layer_ids = nullptr, uint32_t n_ids = 0,
                         uint32_t raw_layers = 0, uint32_t raw_res = 0, bool patch = false) {
  if (!p || !p->layers || (p->n_images && !p->images)) { fspt_set_error("%s: NULL description, layers or images", fn); return FSPT_E_INVALID; }
  if (p->res == 0 || p->res > TEX_MAX_SIDE) { fspt_set_error("%s: res = %u, must lie in [1, %u]", fn, p->res, TEX_MAX_SIDE); return FSPT_E_INVALID; }
  if (p->n_layers == 0) { fspt_set_error("%s: a description must have at least one layer", fn); return FSPT_E_INVALID; }
  for (uint32_t i = 0; i < p->n_images; ++i) {
    const fspt_texture_image &im = p->images[i];
    if (!im.rgba) { fspt_set_error("%s: images[%u].rgba is NULL", fn, i); return FSPT_E_INVALID; }
    if (im.w == 0 || im.w > TEX_MAX_SIDE || im.h == 0 || im.h > TEX_MAX_SIDE) {
      fspt_set_error("%s: images[%u] is %u x %u, each side must lie in [1, %u]", fn, i, im.w, im.h, TEX_MAX_SIDE);
      return FSPT_E_INVALID;
    }
    if (on_device && (uintptr_t)im.rgba % 4) { fspt_set_error("%s: images[%u].rgba must be 4-byte aligned", fn, i); return FSPT_E_INVALID; }
  }
  for (uint32_t l = 0; l < p->n_layers; ++l) {
    const fspt_texture_layer &y = p->layers[l];
    if (y.kind == FSPT_TEXLAYER_COLOR) {
      for (int k = 0; k < 3; ++k)
        if (!std::isfinite(y.color[k])) { fspt_set_error("%s: layers[%u].color[%d] is not finite", fn, l, k); return FSPT_E_INVALID; }
      continue;
    }
    if (y.kind != FSPT_TEXLAYER_IMAGE && y.kind != FSPT_TEXLAYER_PIXELS) { fspt_set_error("%s: layers[%u].kind = %d is no FSPT_TEXLAYER_*", fn, l, (int)y.kind); return FSPT_E_INVALID; }
    if (y.image >= p->n_images) { fspt_set_error("%s: layers[%u].image = %u, the description has %u images", fn, l, y.image, p->n_images); return FSPT_E_INVALID; }
    if (y.kind == FSPT_TEXLAYER_PIXELS) {
      const fspt_texture_image &im = p->images[y.image];
      if (im.w != p->res || im.h != p->res) { fspt_set_error("%s: layers[%u] copies image %u of %u x %u texels, res is %u", fn, l, y.image, im.w, im.h, p->res); return FSPT_E_INVALID; }
      continue;
    }
    for (int k = 0; k < 4; ++k)
      if (y.swizzle[k] > 3) { fspt_set_error("%s: layers[%u].swizzle[%d] = %u, must lie in [0, 3]", fn, l, k, (unsigned)y.swizzle[k]); return FSPT_E_INVALID; }
  }
  if (!patch) return FSPT_OK;
  if (!layer_ids) { fspt_set_error("%s: NULL layer_ids", fn); return FSPT_E_INVALID; }
  if (n_ids != p->n_layers) { fspt_set_error("%s: %u layer ids for a description of %u layers", fn, n_ids, p->n_layers); return FSPT_E_INVALID; }
  if (!raw_layers) return FSPT_OK; // (no retained atlas: the caller answers FSPT_E_STATE)
  if (p->res != raw_res) { fspt_set_error("%s: res = %u, the retained atlas has %u", fn, p->res, raw_res); return FSPT_E_INVALID; }
  std::vector<uint8_t> seen(raw_layers, 0);
  for (uint32_t k = 0; k < n_ids; ++k) {
    if (layer_ids[k] >= raw_layers) { fspt_set_error("%s: layer_ids[%u] = %u, the retained atlas has %u layers", fn, k, layer_ids[k], raw_layers); return FSPT_E_INVALID; }
    if (seen[layer_ids[k]]) { fspt_set_error("%s: layer_ids[%u] = %u is listed twice", fn, k, layer_ids[k]); return FSPT_E_INVALID; }
    seen[layer_ids[k]] = 1;
  }
  return FSPT_OK;
}

// The records of a checked description.  src_off[i] = where image i lies in the upload of the host form (only the images a
// layer uses are uploaded, each once; UINT64_MAX: unused), *src_bytes = the upload's size.  Device form: src = the pointer.
// layer_ids (a patch; NULL: layer l) = the layers of the raw atlas the records write.
inline void texpack_records(const fspt_texture_pack *p, bool on_device, const uint32_t *layer_ids, std::vector<TexLayerRec> &rec, std::vector<uint64_t> &src_off, uint64_t *src_bytes) {
  src_off.assign(p->n_images, UINT64_MAX);
  rec.assign(p->n_layers, TexLayerRec{0, 0, 0, 0, 0, 0, 0});
  uint64_t at = 0;
  for (uint32_t l = 0; l < p->n_layers; ++l) {
    const fspt_texture_layer &y = p->layers[l];
    TexLayerRec &r = rec[l];
    r.flags = (uint32_t)y.kind;
    r.dst = layer_ids ? layer_ids[l] : l;
    if (y.kind == FSPT_TEXLAYER_COLOR) { r.color = tex_color_texel(y.color); continue; }
    const fspt_texture_image &im = p->images[y.image];
    if (src_off[y.image] == UINT64_MAX) { src_off[y.image] = at; at += (uint64_t)im.w * im.h * 4; }
    r.src = on_device ? (uint64_t)(uintptr_t)im.rgba : src_off[y.image];
    r.w = im.w; r.h = im.h;
    if (y.kind != FSPT_TEXLAYER_IMAGE) continue;
    if (y.corrected) r.flags |= 4u;
    for (int k = 0; k < 4; ++k) r.flags |= (uint32_t)y.swizzle[k] << (8 + 2 * k);
  }
  *src_bytes = at;
}

} // namespace fspt
