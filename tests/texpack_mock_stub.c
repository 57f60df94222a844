/* texpack_mock_stub.c - fspt_texture_pack_check_eval, fspt_atlas_pack_gpu, fspt_scene_update_textures, fspt_scene_patch_textures
 * and fspt_scene_sah_cost for the addon built against tests/napi_mock/libfspt_mock.c (tests/test_texpack_cpu.py): they validate
 * like the library and count what reaches them - the "cost" is 1 per update_textures (+ 2 with uvs) + 100 per
 * patched layer + 10000 x the retained res + the last description's source bytes / 1000000.  A packed atlas is, per layer,
 * res^2 texels of (kind, image or the colour's red byte, corrected, 128 + device). */
#include <math.h>
#include <stdint.h>
#include "fspt.h"
#include "fspt_tuning.h"

static double g_seen;
static uint32_t g_res, g_layers;
static uint64_t g_bytes;

static int pack_ok(const fspt_texture_pack *p) {
  if (!p || !p->layers || (p->n_images && !p->images)) return 0;
  if (p->res == 0 || p->res > 16384 || p->n_layers == 0) return 0;
  for (uint32_t i = 0; i < p->n_images; ++i)
    if (!p->images[i].rgba || p->images[i].w == 0 || p->images[i].w > 16384 || p->images[i].h == 0 || p->images[i].h > 16384) return 0;
  for (uint32_t l = 0; l < p->n_layers; ++l) {
    const fspt_texture_layer *y = &p->layers[l];
    if (y->kind == FSPT_TEXLAYER_COLOR) { if (!isfinite(y->color[0]) || !isfinite(y->color[1]) || !isfinite(y->color[2])) return 0; continue; }
    if (y->kind != FSPT_TEXLAYER_IMAGE && y->kind != FSPT_TEXLAYER_PIXELS) return 0;
    if (y->image >= p->n_images) return 0;
    if (y->kind == FSPT_TEXLAYER_PIXELS) { if (p->images[y->image].w != p->res || p->images[y->image].h != p->res) return 0; continue; }
    for (int k = 0; k < 4; ++k) if (y->swizzle[k] > 3) return 0;
  }
  return 1;
}
static uint64_t source_bytes(const fspt_texture_pack *p) {
  uint64_t n = 0;
  for (uint32_t i = 0; i < p->n_images; ++i) n += (uint64_t)p->images[i].w * p->images[i].h * 4;
  return n;
}
static int patch_ok(const fspt_texture_pack *p, const uint32_t *ids, uint32_t n, uint32_t raw_layers, uint32_t raw_res) {
  if (!ids || n != p->n_layers) return FSPT_E_INVALID;
  if (!raw_layers) return FSPT_E_STATE;
  if (p->res != raw_res) return FSPT_E_INVALID;
  for (uint32_t k = 0; k < n; ++k) {
    if (ids[k] >= raw_layers) return FSPT_E_INVALID;
    for (uint32_t j = 0; j < k; ++j) if (ids[j] == ids[k]) return FSPT_E_INVALID;
  }
  return FSPT_OK;
}
int fspt_texture_pack_check_eval(const fspt_texture_pack *p, const uint32_t *layer_ids, uint32_t n, uint32_t raw_layers, uint32_t raw_res) {
  if (!pack_ok(p)) return FSPT_E_INVALID;
  return (layer_ids || n) ? patch_ok(p, layer_ids, n, raw_layers, raw_res) : FSPT_OK;
}
int fspt_atlas_pack_gpu(int device, const fspt_texture_pack *p, uint8_t *atlas_out) {
  if (!pack_ok(p) || !atlas_out) return FSPT_E_INVALID;
  const uint64_t per = (uint64_t)p->res * p->res;
  for (uint32_t l = 0; l < p->n_layers; ++l) {
    const fspt_texture_layer *y = &p->layers[l];
    for (uint64_t i = 0; i < per; ++i) {
      uint8_t *o = atlas_out + (l * per + i) * 4;
      o[0] = (uint8_t)y->kind;
      o[1] = y->kind == FSPT_TEXLAYER_COLOR ? (uint8_t)floor(fmin(fmax((double)y->color[0], 0.0), 1.0) * 255.0 + 0.5) : (uint8_t)y->image;
      o[2] = (uint8_t)(y->corrected * 16 + (y->kind == FSPT_TEXLAYER_IMAGE ? y->swizzle[1] : 0));
      o[3] = (uint8_t)(128 + device);
    }
  }
  return FSPT_OK;
}
int fspt_scene_update_textures(fspt_scene *s, const float *mat, const float *uv, const fspt_texture_pack *p) {
  if (!s || !mat || !pack_ok(p)) return FSPT_E_INVALID;
  g_seen += 1 + (uv ? 2 : 0); g_res = p->res; g_layers = p->n_layers; g_bytes = source_bytes(p);
  return FSPT_OK;
}
int fspt_scene_patch_textures(fspt_scene *s, const uint32_t *layer_ids, uint32_t n, const fspt_texture_pack *p) {
  if (!s || !pack_ok(p)) return FSPT_E_INVALID;
  const int rc = patch_ok(p, layer_ids, n, g_layers, g_res);
  if (rc) return rc;
  g_seen += 100.0 * n; g_bytes = source_bytes(p);
  return FSPT_OK;
}
int fspt_scene_sah_cost(fspt_scene *s, double *cost) {
  if (!s || !cost) return FSPT_E_INVALID;
  *cost = g_seen + 10000.0 * g_res + (double)g_bytes / 1000000.0;
  return FSPT_OK;
}
