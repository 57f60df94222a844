/* appearance_mock_stub.c - fspt_scene_update_materials, fspt_scene_update_environment and fspt_scene_sah_cost for the addon
 * built against tests/napi_mock/libfspt_mock.c (tests/test_appearance_cpu.py): they validate like the library and count what
 * reaches them - the "cost" is 1 per materials update (+ 2 with uvs, + 10 with an atlas) + 100 per environment update
 * (+ 1000 when the map is NULL) + 10000 x the last n_bins. */
#include <stdint.h>
#include "fspt.h"

static double g_seen;
static uint32_t g_bins;

int fspt_scene_update_materials(fspt_scene *s, const float *mat, const float *uv, const uint8_t *atlas, uint32_t atlas_res, uint32_t atlas_layers) {
  if (!s || !mat) return FSPT_E_INVALID;
  if (atlas && (atlas_res == 0 || atlas_layers == 0)) return FSPT_E_INVALID;
  g_seen += 1 + (uv ? 2 : 0) + (atlas ? 10 : 0);
  return FSPT_OK;
}
int fspt_scene_update_environment(fspt_scene *s, const uint8_t *env, uint32_t env_w, uint32_t env_h, const uint32_t *bins, uint32_t n_bins) {
  if (!s || !bins || n_bins == 0) return FSPT_E_INVALID;
  if (env && (env_w == 0 || env_h == 0)) return FSPT_E_INVALID;
  g_seen += 100 + (env ? 0 : 1000);
  g_bins = n_bins;
  return FSPT_OK;
}
int fspt_scene_sah_cost(fspt_scene *s, double *cost) {
  if (!s || !cost) return FSPT_E_INVALID;
  *cost = g_seen + 10000.0 * g_bins;
  return FSPT_OK;
}
