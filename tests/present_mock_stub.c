/* present_mock_stub.c - fspt_present for the addon built against tests/napi_mock/libfspt_mock.c (tests/test_present_cpu.py):
 * reports 7 ticks and fills the frame with 0xAB, so that the JS host's present() can be followed through the addon. */
#include <stdint.h>
#include <string.h>
#include "fspt.h"

int fspt_present(fspt_target *t, float exposure, float saturation, int denoise, float max_sigma, float scale,
                 uint8_t *out_rgba8, uint32_t *ticks_out) {
  uint32_t W = 0, H = 0;
  (void)exposure; (void)saturation; (void)denoise; (void)max_sigma; (void)scale;
  if (!t || !out_rgba8 || !ticks_out) return FSPT_E_INVALID;
  fspt_target_size(t, &W, &H);
  memset(out_rgba8, 0xAB, (size_t)W * H * 4);
  *ticks_out = 7;
  return FSPT_OK;
}
