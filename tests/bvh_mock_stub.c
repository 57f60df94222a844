/* bvh_mock_stub.c - fspt_builder_build_gpu for the addon built against tests/napi_mock/libfspt_mock.c
 * (tests/test_bvh_build_cpu.py): validates like the library and appends every call that reaches it to the file named by
 * FSPT_MOCK_BVH_LOG, so that buildScene({bvh: 'gpu'}) can be followed through the addon. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "fspt.h"

int fspt_builder_build_gpu(fspt_builder *b, uint32_t leaf_size, int device) {
  if (!b || leaf_size == 0 || leaf_size > 64 || device < 0) return FSPT_E_INVALID;
  const char *path = getenv("FSPT_MOCK_BVH_LOG");
  FILE *fp = path ? fopen(path, "a") : NULL;
  if (fp) { fprintf(fp, "%u %d\n", leaf_size, device); fclose(fp); }
  return FSPT_OK;
}
