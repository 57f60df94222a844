/* adaptive_mock_stub.c - fspt_render_adaptive, fspt_adaptive_last_stats and fspt_read_sample_counts for the addon built
 * against tests/napi_mock/libfspt_mock.c (tests/test_adaptive_cpu.py): they validate like the library, append every
 * render_adaptive call that reaches them to the file named by FSPT_MOCK_ADAPTIVE_LOG, and "run" every tile to max_ticks
 * in the bottom row of pixels (the rest: outside a one-row viewport). */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "fspt.h"
#include "fspt_tuning.h"

static uint32_t g_rounds, g_max, g_valid;

int fspt_render_adaptive(fspt_target *t, const fspt_camera_params *cam, const fspt_adaptive_params *q, uint64_t seed) {
  if (!t || !cam || !q) return FSPT_E_INVALID;
  const uint32_t r = q->round_ticks;
  if (r < 2 || r > 128 || q->min_ticks % r || q->min_ticks < 2 * r || q->max_ticks % r || q->max_ticks < q->min_ticks ||
      !isfinite(q->target_rel_mse) || q->target_rel_mse < 0.0)
    return FSPT_E_INVALID;
  uint32_t W, H;
  fspt_target_size(t, &W, &H); /* (aborts on a handle that is no target) */
  const char *path = getenv("FSPT_MOCK_ADAPTIVE_LOG");
  FILE *fp = path ? fopen(path, "a") : NULL;
  if (fp) { fprintf(fp, "%.6f %u %u %u %llu\n", q->target_rel_mse, q->max_ticks, q->min_ticks, r, (unsigned long long)seed); fclose(fp); }
  g_rounds = q->max_ticks / r; g_max = q->max_ticks; g_valid = 1;
  return FSPT_OK;
}

int fspt_adaptive_last_stats(fspt_target *t, uint32_t *rounds, uint64_t *samples, double *tile_err, uint32_t *tile_ticks, uint32_t cap) {
  (void)tile_err; (void)tile_ticks; (void)cap;
  if (!t) return FSPT_E_INVALID;
  if (!g_valid) return FSPT_E_STATE;
  if (rounds) *rounds = g_rounds;
  if (samples) *samples = 0;
  return FSPT_OK;
}

int fspt_read_sample_counts(fspt_target *t, uint32_t *out) {
  if (!t || !out) return FSPT_E_INVALID;
  if (!g_valid) return FSPT_E_STATE;
  uint32_t W, H;
  fspt_target_size(t, &W, &H);
  for (uint32_t i = 0; i < W * H; ++i) out[i] = i < W ? g_max : 0u;
  return FSPT_OK;
}
