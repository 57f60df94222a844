/* jpeg_mock_stub.c - the JPEG entries (include/fspt.h) for the addon built against tests/napi_mock/libfspt_mock.c
 * (tests/test_jpeg_cpu.py): every call writes a recognisable 8-byte "file" - SOI, a tag naming the entry, three of its arguments,
 * EOI - so that the JS host's drawJpeg / presentJpeg / jpegEncode can be followed through the addon; a buffer below 8 bytes is
 * refused the library's way (FSPT_E_INVALID, the size needed, nothing written). */
#include <stdint.h>
#include <string.h>
#include "fspt.h"

static int put(uint8_t tag, uint8_t a, const fspt_jpeg_params *p, uint8_t *out, size_t cap, size_t *bytes_out) {
  const uint8_t f[8] = {0xFF, 0xD8, tag, a, (uint8_t)(p ? p->quality : 85), (uint8_t)(p ? p->subsampling * 16 + p->restart_mcus : 0x10), 0xFF, 0xD9};
  *bytes_out = sizeof f;
  if (cap < sizeof f) return FSPT_E_INVALID;
  memcpy(out, f, sizeof f);
  return FSPT_OK;
}

int fspt_jpeg_bound(uint32_t w, uint32_t h, const fspt_jpeg_params *p, size_t *bytes) {
  (void)p;
  if (!bytes || !w || !h) return FSPT_E_INVALID;
  *bytes = 1000u + (size_t)w * h;
  return FSPT_OK;
}

int fspt_jpeg_encode(int device, const uint8_t *rgba8, uint32_t w, uint32_t h, int bottom_up, const fspt_jpeg_params *p, uint8_t *out, size_t cap, size_t *bytes_out) {
  (void)device; (void)h;
  if (!rgba8 || !out || !bytes_out) return FSPT_E_INVALID;
  return put('E', (uint8_t)(w * 2 + (bottom_up ? 1 : 0)), p, out, cap, bytes_out);
}

int fspt_draw_jpeg(fspt_target *t, int source, float exposure, float saturation, int denoise, float max_sigma, float scale, const fspt_jpeg_params *p, uint8_t *out, size_t cap, size_t *bytes_out) {
  (void)exposure; (void)saturation; (void)denoise; (void)max_sigma; (void)scale;
  if (!t || !out || !bytes_out) return FSPT_E_INVALID;
  return put('D', (uint8_t)source, p, out, cap, bytes_out);
}

int fspt_present_jpeg(fspt_target *t, float exposure, float saturation, int denoise, float max_sigma, float scale, const fspt_jpeg_params *p, uint8_t *out, size_t cap, size_t *bytes_out, uint32_t *ticks_out) {
  (void)exposure; (void)saturation; (void)max_sigma;
  if (!t || !out || !bytes_out || !ticks_out) return FSPT_E_INVALID;
  *ticks_out = 0; *bytes_out = 0;
  if (scale < 0.5f) return FSPT_OK; /* "nothing to present" */
  *ticks_out = 7;
  return put('P', (uint8_t)denoise, p, out, cap, bytes_out);
}
