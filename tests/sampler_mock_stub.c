/* sampler_mock_stub.c - fspt_target_set_sampler for the addon built against tests/napi_mock/libfspt_mock.c
 * (tests/test_sampler_cpu.py): validates like the library and appends every call that reaches it to the file named by
 * FSPT_MOCK_SAMPLER_LOG, so that the JS host's setSampler() can be followed through the addon. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "fspt.h"

int fspt_target_set_sampler(fspt_target *t, int sampler, uint32_t seed) {
  if (!t || (sampler != FSPT_SAMPLER_REFERENCE && sampler != FSPT_SAMPLER_SOBOL)) return FSPT_E_INVALID;
  const char *path = getenv("FSPT_MOCK_SAMPLER_LOG");
  FILE *f = path ? fopen(path, "a") : NULL;
  if (f) { fprintf(f, "%d %u\n", sampler, seed); fclose(f); }
  return FSPT_OK;
}
