/* matte_mock_stub.c - the ID-matte entries (include/fspt.h) for the addon built against
 * tests/napi_mock/libfspt_mock.c (tests/test_matte_cpu.py).  The hash is the real rule (the JS host's manifests can be
 * compared with the Python host's); everything else records what reached it: the ids and the manifest of the last
 * set_matte call come back through fspt_read_mattes / fspt_mattes_lost, and the EXR entries write a recognisable 12-byte
 * "file" - a tag, the layer bits, which ranks and how many manifest bytes came along. */
#include <stdint.h>
#include <string.h>
#include "fspt.h"
#include "fspt_tuning.h"

static uint32_t g_ids[2][8], g_n_ids[2], g_manifest_len[2], g_manifest_sum[2], g_samples;
static uint64_t g_seed;

static uint32_t rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
uint32_t fspt_matte_hash(const char *name, size_t len) {
  const uint8_t *d = (const uint8_t *)name;
  uint32_t h = 0, k;
  size_t i;
  for (i = 0; i + 4 <= len; i += 4) {
    k = (uint32_t)d[i] | (uint32_t)d[i + 1] << 8 | (uint32_t)d[i + 2] << 16 | (uint32_t)d[i + 3] << 24;
    k *= 0xcc9e2d51u; k = rotl(k, 15); k *= 0x1b873593u;
    h ^= k; h = rotl(h, 13); h = h * 5u + 0xe6546b64u;
  }
  k = 0;
  if ((len & 3) >= 3) k ^= (uint32_t)d[i + 2] << 16;
  if ((len & 3) >= 2) k ^= (uint32_t)d[i + 1] << 8;
  if ((len & 3) >= 1) { k ^= d[i]; k *= 0xcc9e2d51u; k = rotl(k, 15); k *= 0x1b873593u; h ^= k; }
  h ^= (uint32_t)len;
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  k = (h >> 23) & 255u;
  return k == 0 || k == 255u ? h ^ (1u << 23) : h;
}

int fspt_scene_set_matte_ids(fspt_scene *s, int kind, const uint32_t *ids) {
  if (!s || kind < 0 || kind > 1) return FSPT_E_INVALID;
  g_n_ids[kind] = ids ? 1u : 0u; /* (the mock's scenes have one triangle) */
  if (ids) g_ids[kind][0] = ids[0];
  return FSPT_OK;
}
int fspt_scene_set_matte_manifest(fspt_scene *s, int kind, const char *json, size_t len) {
  if (!s || kind < 0 || kind > 1) return FSPT_E_INVALID;
  g_manifest_len[kind] = (uint32_t)len; g_manifest_sum[kind] = 0;
  for (size_t i = 0; json && i < len; ++i) g_manifest_sum[kind] += (uint8_t)json[i];
  return FSPT_OK;
}
int fspt_mattes(fspt_target *t, const fspt_camera_params *cam, uint32_t samples, uint64_t seed) {
  if (!t || !cam) return FSPT_E_INVALID;
  if (!g_n_ids[0] && !g_n_ids[1]) return FSPT_E_STATE;
  g_samples = samples; g_seed = seed;
  return FSPT_OK;
}
int fspt_read_mattes(fspt_target *t, int kind, float *out) { /* id, 1.0, then what the calls before left */
  if (!t || !out || kind < 0 || kind > 1) return FSPT_E_INVALID;
  if (!g_n_ids[kind]) return FSPT_E_STATE;
  memcpy(out, &g_ids[kind][0], 4);
  out[1] = 1.0f; out[2] = (float)g_samples; out[3] = (float)g_seed; out[4] = (float)g_manifest_len[kind]; out[5] = (float)g_manifest_sum[kind];
  return FSPT_OK;
}
int fspt_mattes_lost(fspt_target *t, int kind, uint64_t *lost) {
  if (!t || !lost || kind < 0 || kind > 1) return FSPT_E_INVALID;
  *lost = 1000u + (uint64_t)kind;
  return FSPT_OK;
}

static size_t bound_of(uint32_t w, uint32_t h, const fspt_exr_mattes *m) {
  return 3000u + (size_t)w * h * 140u + (m ? m->manifest_len[0] + m->manifest_len[1] : 0u);
}
int fspt_exr_bound(uint32_t w, uint32_t h, const fspt_exr_params *p, size_t *bytes) {
  if (!bytes || !w || !h || (p && (p->layers & ~15u))) return FSPT_E_INVALID;
  *bytes = bound_of(w, h, NULL);
  return FSPT_OK;
}
int fspt_exr_bound_mattes(uint32_t w, uint32_t h, const fspt_exr_params *p, const fspt_exr_mattes *m, size_t *bytes) {
  (void)p;
  if (!bytes || !w || !h) return FSPT_E_INVALID;
  *bytes = bound_of(w, h, m);
  return FSPT_OK;
}
static int put(uint8_t tag, uint8_t a, const fspt_exr_params *p, const fspt_exr_mattes *m, uint8_t *out, size_t cap, size_t *bytes_out) {
  const uint8_t f[12] = {tag, a, (uint8_t)(p ? p->compression : 3), (uint8_t)(p ? p->pixel_type : 1), (uint8_t)(p ? p->layers : 0), (uint8_t)(m && m->ranks[0] ? 1 : 0),
                         (uint8_t)(m && m->ranks[1] ? 1 : 0), (uint8_t)(m ? m->manifest_len[0] : 0), (uint8_t)(m ? m->manifest_len[1] : 0),
                         (uint8_t)(m && m->manifest[0] ? m->manifest[0][0] : 0), (uint8_t)(m && m->manifest[1] ? m->manifest[1][0] : 0), 'X'};
  *bytes_out = sizeof f;
  if (cap < sizeof f) return FSPT_E_INVALID;
  memcpy(out, f, sizeof f);
  return FSPT_OK;
}
int fspt_exr_encode_mattes(int device, const float *rgba, const float *features, const fspt_exr_mattes *m, uint32_t w, uint32_t h, int bottom_up, const fspt_exr_params *p, uint8_t *out, size_t cap, size_t *bytes_out) {
  (void)device; (void)h; (void)features;
  if (!rgba || !out || !bytes_out) return FSPT_E_INVALID;
  return put('M', (uint8_t)(w * 2 + (bottom_up ? 1 : 0)), p, m, out, cap, bytes_out);
}
int fspt_draw_exr(fspt_target *t, int source, const fspt_exr_params *p, uint8_t *out, size_t cap, size_t *bytes_out) {
  if (!t || !out || !bytes_out) return FSPT_E_INVALID;
  return put('D', (uint8_t)source, p, NULL, out, cap, bytes_out);
}
