/* lights_mock_stub.c - fspt_target_set_lights for the addon built against tests/napi_mock/libfspt_mock.c
 * (tests/test_lights_cpu.py): validates like the library and appends every call that reaches it to the file named by
 * FSPT_MOCK_LIGHTS_LOG, so that the JS host's setLights() can be followed through the addon. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "fspt.h"

int fspt_target_set_lights(fspt_target *t, int mode, float f) {
  if (!t || (mode != FSPT_LIGHTS_OFF && mode != FSPT_LIGHTS_EMITTERS) || !(f > 0.0f && f <= 1.0f)) return FSPT_E_INVALID;
  const char *path = getenv("FSPT_MOCK_LIGHTS_LOG");
  FILE *fp = path ? fopen(path, "a") : NULL;
  if (fp) { fprintf(fp, "%d %.3f\n", mode, (double)f); fclose(fp); }
  return FSPT_OK;
}
