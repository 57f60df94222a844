/* bloom_mock_stub.c - the bloom entry points for the addon built against tests/napi_mock/libfspt_mock.c
 * (tests/test_bloom_cpu.py): validates like the library and records what reaches it; fspt_target_get_bloom reports the mode
 * and the parameters of the last accepted call, with levels + 100 x (accepted set calls) so that the calls can be counted. */
#include <math.h>
#include <stdint.h>
#include "fspt.h"
#include "fspt_tuning.h"

static int g_on, g_sets;
static fspt_bloom_params g_p = {FSPT_BLOOM_INTENSITY, FSPT_BLOOM_SCATTER, FSPT_BLOOM_LEVELS};

int fspt_target_set_bloom(fspt_target *t, int on, const fspt_bloom_params *p) {
  if (!t) return FSPT_E_INVALID;
  if (on) {
    if (!p) return FSPT_E_INVALID; /* (the JS host always passes all three) */
    if (!(isfinite(p->intensity) && isfinite(p->scatter) && p->intensity >= 0.0f && p->intensity <= 1.0f && p->scatter >= 0.0f && p->scatter <= 1.0f &&
          p->levels >= 1u && p->levels <= (uint32_t)FSPT_BLOOM_MAX_LEVELS)) return FSPT_E_INVALID;
    g_p = *p;
  }
  ++g_sets; g_on = on != 0;
  return FSPT_OK;
}
int fspt_target_get_bloom(fspt_target *t, int *on, fspt_bloom_params *p) {
  if (!t || !on || !p) return FSPT_E_INVALID;
  *on = g_on; *p = g_p;
  p->levels += 100u * (uint32_t)g_sets;
  return FSPT_OK;
}
