/* png_mock_stub.c - the PNG entries (include/fspt.h) for the addon built against tests/napi_mock/libfspt_mock.c
 * (tests/test_png_cpu.py): every call writes a recognisable 8-byte "file" - a tag naming the entry, one of its arguments, the
 * three parameters, three closing bytes - so that the JS host's drawPng / pngEncode / pngFilteredEval can be followed through
 * the addon; a buffer below 8 bytes is refused the library's way (FSPT_E_INVALID, the size needed, nothing written). */
#include <stdint.h>
#include <string.h>
#include "fspt.h"
#include "fspt_tuning.h"

static int put(uint8_t tag, uint8_t a, const fspt_png_params *p, uint8_t *out, size_t cap, size_t *bytes_out) {
  const uint8_t f[8] = {tag, a, (uint8_t)(p ? p->channels : 3), (uint8_t)(p ? p->filter : 5), (uint8_t)(p ? p->chunk_bytes >> 8 : 0), 'I', 'E', 'N'};
  *bytes_out = sizeof f;
  if (cap < sizeof f) return FSPT_E_INVALID;
  memcpy(out, f, sizeof f);
  return FSPT_OK;
}

int fspt_png_bound(uint32_t w, uint32_t h, const fspt_png_params *p, size_t *bytes) {
  (void)p;
  if (!bytes || !w || !h) return FSPT_E_INVALID;
  *bytes = 2000u + (size_t)w * h;
  return FSPT_OK;
}

int fspt_png_encode(int device, const uint8_t *rgba8, uint32_t w, uint32_t h, int bottom_up, const fspt_png_params *p, uint8_t *out, size_t cap, size_t *bytes_out) {
  (void)device; (void)h;
  if (!rgba8 || !out || !bytes_out) return FSPT_E_INVALID;
  return put('E', (uint8_t)(w * 2 + (bottom_up ? 1 : 0)), p, out, cap, bytes_out);
}

int fspt_png_filtered_eval(int device, const uint8_t *rgba8, uint32_t w, uint32_t h, int bottom_up, const fspt_png_params *p, uint8_t *stream_out) {
  (void)device; (void)bottom_up;
  if (!rgba8 || !stream_out || !p) return FSPT_E_INVALID;
  memset(stream_out, (int)(p->channels * 16 + p->filter), (size_t)h * (1u + (size_t)w * p->channels));
  return FSPT_OK;
}

int fspt_draw_png(fspt_target *t, int source, float exposure, float saturation, int denoise, float max_sigma, float scale, const fspt_png_params *p, uint8_t *out, size_t cap, size_t *bytes_out) {
  (void)exposure; (void)saturation; (void)denoise; (void)max_sigma; (void)scale;
  if (!t || !out || !bytes_out) return FSPT_E_INVALID;
  return put('D', (uint8_t)source, p, out, cap, bytes_out);
}
