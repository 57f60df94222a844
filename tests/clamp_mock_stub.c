/* clamp_mock_stub.c - fspt_temporal_set_clamp for the addon built against tests/napi_mock/libfspt_mock.c
 * (tests/test_clamp_cpu.py): validates like the library and records what reaches it.  Its own fspt_temporal_accumulate
 * (tests/temporal_mock_stub.c is not linked beside it) returns that record as the history: (mode, fast_history,
 * sigma_scale, set_clamp calls) in pixel 0. */
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "fspt.h"
#include "fspt_tuning.h"

static int g_on, g_sets;
static float g_fast, g_sigma;
static uint32_t g_px = 3 * 2; /* the mock check's target */

int fspt_temporal_set_clamp(fspt_target *t, int on, float fast_history, float sigma_scale) {
  if (!t) return FSPT_E_INVALID;
  if (on && (!(fast_history >= 1.0f && fast_history < INFINITY) || !(sigma_scale >= 0.0f))) return FSPT_E_INVALID;
  ++g_sets;
  g_on = on != 0;
  if (on) { g_fast = fast_history; g_sigma = sigma_scale; }
  return FSPT_OK;
}
int fspt_temporal_accumulate(fspt_target *t, const fspt_camera_params *cam, const fspt_temporal_params *p, float *out) {
  (void)p;
  if (!t || !cam) return FSPT_E_INVALID;
  if (out) {
    memset(out, 0, (size_t)g_px * 16);
    out[0] = (float)g_on; out[1] = g_fast; out[2] = g_sigma; out[3] = (float)g_sets;
  }
  return FSPT_OK;
}
