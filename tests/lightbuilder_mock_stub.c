/* lightbuilder_mock_stub.c - fspt_scene_set_light_builder and fspt_scene_get_light_builder for the addon built against
 * tests/napi_mock/libfspt_mock.c (tests/test_lighttable_node.py): they validate like the library, keep the last builder
 * set and append every call that reaches set to the file named by FSPT_MOCK_LIGHTBUILDER_LOG. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "fspt.h"

static int g_builder = FSPT_LIGHT_BUILDER_HOST;

int fspt_scene_set_light_builder(fspt_scene *s, int builder) {
  if (!s || (builder != FSPT_LIGHT_BUILDER_HOST && builder != FSPT_LIGHT_BUILDER_GPU)) return FSPT_E_INVALID;
  const char *path = getenv("FSPT_MOCK_LIGHTBUILDER_LOG");
  FILE *fp = path ? fopen(path, "a") : NULL;
  if (fp) { fprintf(fp, "%d\n", builder); fclose(fp); }
  g_builder = builder;
  return FSPT_OK;
}
int fspt_scene_get_light_builder(fspt_scene *s, int *builder) {
  if (!s || !builder) return FSPT_E_INVALID;
  *builder = g_builder;
  return FSPT_OK;
}
