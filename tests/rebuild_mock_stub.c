/* rebuild_mock_stub.c - fspt_scene_rebuild_geometry for the addon built against tests/napi_mock/libfspt_mock.c
 * (tests/test_rebuild_cpu.py): validates like the library, hands back the reversed order, counts what reaches it in the
 * "cost" (100 + 10 per rebuild without normals + 20 per rebuild with them). */
#include <stdint.h>
#include "fspt.h"

static int g_rebuilds;
static uint32_t g_tris = 2; /* the mock check's scene */

int fspt_scene_update_geometry(fspt_scene *s, const float *tri, const float *norm) { (void)norm; return (!s || !tri) ? FSPT_E_INVALID : FSPT_OK; }
int fspt_scene_rebuild_geometry(fspt_scene *s, const float *tri, const float *norm, uint32_t *order_out) {
  if (!s || !tri) return FSPT_E_INVALID;
  g_rebuilds += norm ? 20 : 10;
  if (order_out) for (uint32_t k = 0; k < g_tris; ++k) order_out[k] = g_tris - 1 - k;
  return FSPT_OK;
}
int fspt_scene_sah_cost(fspt_scene *s, double *cost) {
  if (!s || !cost) return FSPT_E_INVALID;
  *cost = 100.0 + g_rebuilds;
  return FSPT_OK;
}
