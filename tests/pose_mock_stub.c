/* pose_mock_stub.c - fspt_scene_set_pose, fspt_scene_update_transforms and fspt_scene_sah_cost for the addon built against
 * tests/napi_mock/libfspt_mock.c (tests/test_pose_node.py): they validate like the library and count what reaches them - the
 * "cost" is 1000 x the pose's parts (0: no pose) + 100 when it has rest normals + 1 per update_transforms. */
#include <stdint.h>
#include "fspt.h"

static uint32_t g_parts;
static int g_norm, g_updates;

int fspt_scene_set_pose(fspt_scene *s, const uint32_t *part, uint32_t n_parts, const float *tri, const float *norm) {
  if (!s) return FSPT_E_INVALID;
  if (!part) { g_parts = 0; g_norm = 0; return FSPT_OK; }
  if (!tri || n_parts == 0) return FSPT_E_INVALID;
  g_parts = n_parts;
  g_norm = norm != 0;
  return FSPT_OK;
}
int fspt_scene_update_transforms(fspt_scene *s, const float *xf, uint32_t n_parts) {
  if (!s || !xf) return FSPT_E_INVALID;
  if (!g_parts) return FSPT_E_STATE;
  if (n_parts != g_parts) return FSPT_E_INVALID;
  g_updates += 1;
  return FSPT_OK;
}
int fspt_scene_sah_cost(fspt_scene *s, double *cost) {
  if (!s || !cost) return FSPT_E_INVALID;
  *cost = 1000.0 * g_parts + 100.0 * g_norm + g_updates;
  return FSPT_OK;
}
