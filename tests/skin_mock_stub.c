/* skin_mock_stub.c - fspt_scene_set_skin, fspt_scene_update_skin and fspt_scene_sah_cost for the addon built against
 * tests/napi_mock/libfspt_mock.c (tests/test_skin_node.py): they validate like the library and count what reaches them - the
 * "cost" is 10000 x the skin's joints (0: no skin) + 1000 x its morph targets + 100 when it has rest normals + 50 when it
 * has frame targets + 1 per update_skin. */
#include <stdint.h>
#include "fspt.h"

static uint32_t g_joints, g_morph;
static int g_norm, g_mnorm, g_updates;

int fspt_scene_set_skin(fspt_scene *s, const fspt_skin_desc *d) {
  if (!s) return FSPT_E_INVALID;
  if (!d) { g_joints = g_morph = 0; g_norm = g_mnorm = 0; return FSPT_OK; }
  if (!d->joints || !d->weights || !d->tri || d->n_joints < 1 || d->n_joints > 65535 || d->n_morph > 64) return FSPT_E_INVALID;
  if ((d->n_morph && !d->morph) || (d->morph_norm && (!d->norm || !d->n_morph))) return FSPT_E_INVALID;
  g_joints = d->n_joints; g_morph = d->n_morph;
  g_norm = d->norm != 0; g_mnorm = d->morph_norm != 0;
  return FSPT_OK;
}
int fspt_scene_update_skin(fspt_scene *s, const float *xf, uint32_t n_joints, const float *morph_w, uint32_t n_morph) {
  if (!s || !xf) return FSPT_E_INVALID;
  if (!g_joints) return FSPT_E_STATE;
  if (n_joints != g_joints || n_morph != g_morph || (n_morph && !morph_w)) return FSPT_E_INVALID;
  g_updates += 1;
  return FSPT_OK;
}
int fspt_scene_sah_cost(fspt_scene *s, double *cost) {
  if (!s || !cost) return FSPT_E_INVALID;
  *cost = 10000.0 * g_joints + 1000.0 * g_morph + 100.0 * g_norm + 50.0 * g_mnorm + g_updates;
  return FSPT_OK;
}
