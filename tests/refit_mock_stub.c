/* refit_mock_stub.c - fspt_scene_update_geometry and fspt_scene_sah_cost for the addon built against
 * tests/napi_mock/libfspt_mock.c (tests/test_refit_cpu.py): they validate like the library and count what reaches them -
 * the "cost" is 100 + 1 per update without normals + 2 per update with them. */
#include <stdint.h>
#include "fspt.h"

static int g_updates;

int fspt_scene_update_geometry(fspt_scene *s, const float *tri, const float *norm) {
  if (!s || !tri) return FSPT_E_INVALID;
  g_updates += norm ? 2 : 1;
  return FSPT_OK;
}
int fspt_scene_update_geometry_device(fspt_scene *s, const float *tri, const float *norm) {
  (void)s; (void)tri; (void)norm;
  return FSPT_E_NO_DEVICE;
}
int fspt_scene_sah_cost(fspt_scene *s, double *cost) {
  if (!s || !cost) return FSPT_E_INVALID;
  *cost = 100.0 + g_updates;
  return FSPT_OK;
}
