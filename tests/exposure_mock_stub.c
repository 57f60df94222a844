/* exposure_mock_stub.c - the auto-exposure entry points for the addon built against tests/napi_mock/libfspt_mock.c
 * (tests/test_exposure_cpu.py): validates like the library and records what reaches it; fspt_exposure_get reports the
 * record: exposure = key (or 1 after a reset), log2_mean = adapt_down, metered = 1000 x set calls + 10 x resets + mode. */
#include <math.h>
#include <stdint.h>
#include "fspt.h"
#include "fspt_tuning.h"

static int g_on, g_sets, g_resets;
static fspt_exposure_params g_p;
static float g_exposure = 1.0f;

int fspt_target_set_auto_exposure(fspt_target *t, int on, const fspt_exposure_params *p) {
  if (!t) return FSPT_E_INVALID;
  if (on) {
    if (!p) return FSPT_E_INVALID; /* (the JS host always passes all seven) */
    const float f[7] = {p->key, p->low, p->high, p->adapt_up, p->adapt_down, p->min_log2, p->max_log2};
    for (int k = 0; k < 7; ++k) if (!isfinite(f[k])) return FSPT_E_INVALID;
    if (!(p->key > 0.0f && p->low >= 0.0f && p->low < p->high && p->high <= 1.0f && p->adapt_up > 0.0f && p->adapt_up <= 1.0f &&
          p->adapt_down > 0.0f && p->adapt_down <= 1.0f && p->min_log2 <= p->max_log2)) return FSPT_E_INVALID;
    g_p = *p; g_exposure = p->key;
  }
  ++g_sets; g_on = on != 0;
  return FSPT_OK;
}
int fspt_exposure_reset(fspt_target *t) {
  if (!t) return FSPT_E_INVALID;
  if (!g_on) return FSPT_E_STATE;
  ++g_resets; g_exposure = 1.0f;
  return FSPT_OK;
}
int fspt_exposure_get(fspt_target *t, float *exposure, float *log2_mean, uint32_t *metered) {
  if (!t) return FSPT_E_INVALID;
  if (!g_on) return FSPT_E_STATE;
  if (exposure) *exposure = g_exposure;
  if (log2_mean) *log2_mean = g_p.adapt_down;
  if (metered) *metered = 1000u * (uint32_t)g_sets + 10u * (uint32_t)g_resets + (uint32_t)g_on;
  return FSPT_OK;
}
