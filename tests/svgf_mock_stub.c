/* svgf_mock_stub.c - fspt_temporal_set_moments and fspt_temporal_denoise_variance for the addon built against
 * tests/napi_mock/libfspt_mock.c and tests/temporal_mock_stub.c (tests/test_svgf_cpu.py): validates like the library and
 * records what reaches it.  The frame a denoise call returns is (iterations, sigma_color, sigma_normal, sigma_depth) of the
 * call (-1 and zeros for NULL) in pixel 0 and (moments mode, set_moments calls) in pixel 1. */
#include <stdint.h>
#include <string.h>
#include "fspt.h"
#include "fspt_tuning.h"

static int g_on, g_sets;
static uint32_t g_px = 3 * 2; /* the mock check's target */

int fspt_temporal_set_moments(fspt_target *t, int on) {
  if (!t) return FSPT_E_INVALID;
  g_on = on != 0; ++g_sets;
  return FSPT_OK;
}
int fspt_temporal_denoise_variance(fspt_target *t, const fspt_denoise_params *p, float *out) {
  if (!t) return FSPT_E_INVALID;
  if (p && (p->iterations > 16u || !(p->sigma_color >= 0.0f) || !(p->sigma_depth > 0.0f) || !(p->sigma_normal >= 0.0f && p->sigma_normal < 1e38f))) return FSPT_E_INVALID;
  if (!g_on) return FSPT_E_STATE;
  if (out) {
    memset(out, 0, (size_t)g_px * 16);
    out[0] = p ? (float)p->iterations : -1.0f;
    if (p) { out[1] = p->sigma_color; out[2] = p->sigma_normal; out[3] = p->sigma_depth; }
    out[4] = (float)g_on; out[5] = (float)g_sets;
  }
  return FSPT_OK;
}
