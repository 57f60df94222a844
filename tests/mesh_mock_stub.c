/* mesh_mock_stub.c - fspt_scene_set_mesh, fspt_scene_update_vertices, fspt_scene_read_mesh and fspt_scene_sah_cost for the addon
 * built against tests/napi_mock/libfspt_mock.c (tests/test_mesh_node.py): they validate like the library and count what reaches
 * them - the "cost" is 10000 x the mesh's vertices (0: no mesh) + 1000 when it has smooth flags + 100 when it has ranks + 50
 * when it has a rest copy + 1 per update_vertices; read_mesh fills tri with the update count and norm with the vertex count. */
#include <stdint.h>
#include "fspt.h"
#include "fspt_tuning.h"

static uint32_t g_vertices;
static int g_smooth, g_rank, g_rest, g_updates;

int fspt_scene_set_mesh(fspt_scene *s, const fspt_mesh_desc *d) {
  if (!s) return FSPT_E_INVALID;
  if (!d) { g_vertices = 0; g_smooth = g_rank = g_rest = 0; return FSPT_OK; }
  if (!d->vertex || !d->uv || d->n_vertices == 0 || d->n_vertices == FSPT_MESH_STATIC) return FSPT_E_INVALID;
  if ((d->tri != 0) != (d->norm != 0)) return FSPT_E_INVALID;
  g_vertices = d->n_vertices;
  g_smooth = d->smooth != 0; g_rank = d->rank != 0; g_rest = d->tri != 0;
  return FSPT_OK;
}
int fspt_scene_update_vertices(fspt_scene *s, const float *pos, uint32_t n_vertices) {
  if (!s || !pos) return FSPT_E_INVALID;
  if (!g_vertices) return FSPT_E_STATE;
  if (n_vertices != g_vertices) return FSPT_E_INVALID;
  g_updates += 1;
  return FSPT_OK;
}
int fspt_scene_read_mesh(fspt_scene *s, float *tri, float *norm) {
  if (!s || (!tri && !norm)) return FSPT_E_INVALID;
  if (!g_vertices || !g_updates) return FSPT_E_STATE;
  if (tri) tri[0] = (float)g_updates;
  if (norm) norm[0] = (float)g_vertices;
  return FSPT_OK;
}
int fspt_scene_sah_cost(fspt_scene *s, double *cost) {
  if (!s || !cost) return FSPT_E_INVALID;
  *cost = 10000.0 * g_vertices + 1000.0 * g_smooth + 100.0 * g_rank + 50.0 * g_rest + g_updates;
  return FSPT_OK;
}
