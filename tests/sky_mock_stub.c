/* sky_mock_stub.c - fspt_scene_update_sky, fspt_scene_update_environment_auto, fspt_sky_generate, fspt_env_bins_gpu and
 * fspt_scene_sah_cost for the addon built against tests/napi_mock/libfspt_mock.c (tests/test_sky_cpu.py): they validate like the
 * library and count what reaches them - the "cost" is 1 per sky update + 100 per auto environment + 10000 x the last map's
 * width + the last sky's turbidity / 1000.  A generated sky is w * h texels of (view_samples, light_samples, 7, 128 + device);
 * the GPU's bins are the one box (0, 0, w, h) followed by (device, 0, 0, 0). */
#include <math.h>
#include <stdint.h>
#include "fspt.h"

static double g_seen;
static uint32_t g_w;
static float g_turbidity;

static int sky_ok(const fspt_sky_params *p, uint32_t w, uint32_t h) {
  if (!p || w < 1 || w > 65535 || h < 1 || h > 65535) return 0;
  if (!(p->turbidity >= 0.0f && p->turbidity <= 64.0f) || !(p->sun_radius > 0.0f && p->sun_radius <= 0.5f)) return 0;
  if (p->view_samples < 1 || p->view_samples > 64 || p->light_samples < 1 || p->light_samples > 32) return 0;
  return p->sun_dir[0] != 0.0f || p->sun_dir[1] != 0.0f || p->sun_dir[2] != 0.0f;
}
int fspt_scene_update_sky(fspt_scene *s, const fspt_sky_params *p, uint32_t w, uint32_t h) {
  if (!s || !sky_ok(p, w, h)) return FSPT_E_INVALID;
  g_seen += 1; g_w = w; g_turbidity = p->turbidity;
  return FSPT_OK;
}
int fspt_scene_update_environment_auto(fspt_scene *s, const uint8_t *env, uint32_t w, uint32_t h) {
  if (!s || !env || w < 1 || w > 65535 || h < 1 || h > 65535) return FSPT_E_INVALID;
  g_seen += 100; g_w = w;
  return FSPT_OK;
}
int fspt_sky_generate(int device, const fspt_sky_params *p, uint32_t w, uint32_t h, uint8_t *rgbe_out, float *linear_out) {
  if (!sky_ok(p, w, h)) return FSPT_E_INVALID;
  (void)linear_out;
  for (uint64_t i = 0; rgbe_out && i < (uint64_t)w * h; ++i) {
    rgbe_out[4 * i] = (uint8_t)p->view_samples; rgbe_out[4 * i + 1] = (uint8_t)p->light_samples; rgbe_out[4 * i + 2] = 7; rgbe_out[4 * i + 3] = (uint8_t)(128 + device);
  }
  return FSPT_OK;
}
int fspt_env_bins_gpu(const uint8_t *rgbe, uint32_t w, uint32_t h, int device, uint32_t *bins, uint32_t cap, uint32_t *n_bins) {
  if (!rgbe || !w || !h || !n_bins) return FSPT_E_INVALID;
  *n_bins = 2;
  if (bins && cap > 0) { bins[0] = 0; bins[1] = 0; bins[2] = w; bins[3] = h; }
  if (bins && cap > 1) { bins[4] = (uint32_t)device; bins[5] = 0; bins[6] = 0; bins[7] = 0; }
  return FSPT_OK;
}
int fspt_scene_sah_cost(fspt_scene *s, double *cost) {
  if (!s || !cost) return FSPT_E_INVALID;
  *cost = g_seen + 10000.0 * g_w + (double)g_turbidity / 1000.0;
  return FSPT_OK;
}
