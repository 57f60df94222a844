/* exr_mock_stub.c - the OpenEXR entries (include/fspt.h) for the addon built against tests/napi_mock/libfspt_mock.c
 * (tests/test_exr_cpu.py): every call writes a recognisable 8-byte "file" - a tag naming the entry, one of its arguments, the
 * four parameters, whether features came along, a closing byte - so that the JS host's drawExr / exrEncode can be followed
 * through the addon; a buffer below 8 bytes is refused the library's way (FSPT_E_INVALID, the size needed, nothing written). */
#include <stdint.h>
#include <string.h>
#include "fspt.h"
#include "fspt_tuning.h"

static int put(uint8_t tag, uint8_t a, const fspt_exr_params *p, int feat, uint8_t *out, size_t cap, size_t *bytes_out) {
  const uint8_t f[8] = {tag, a, (uint8_t)(p ? p->compression : 3), (uint8_t)(p ? p->pixel_type : 1), (uint8_t)(p ? p->layers : 0), (uint8_t)(p ? p->chunk_bytes >> 8 : 0), (uint8_t)feat, 'X'};
  *bytes_out = sizeof f;
  if (cap < sizeof f) return FSPT_E_INVALID;
  memcpy(out, f, sizeof f);
  return FSPT_OK;
}

int fspt_exr_bound(uint32_t w, uint32_t h, const fspt_exr_params *p, size_t *bytes) {
  (void)p;
  if (!bytes || !w || !h) return FSPT_E_INVALID;
  *bytes = 3000u + (size_t)w * h * 44u;
  return FSPT_OK;
}

int fspt_exr_encode(int device, const float *rgba, const float *features, uint32_t w, uint32_t h, int bottom_up, const fspt_exr_params *p, uint8_t *out, size_t cap, size_t *bytes_out) {
  (void)device; (void)h;
  if (!rgba || !out || !bytes_out) return FSPT_E_INVALID;
  return put('E', (uint8_t)(w * 2 + (bottom_up ? 1 : 0)), p, features ? 1 : 0, out, cap, bytes_out);
}

int fspt_draw_exr(fspt_target *t, int source, const fspt_exr_params *p, uint8_t *out, size_t cap, size_t *bytes_out) {
  if (!t || !out || !bytes_out) return FSPT_E_INVALID;
  return put('D', (uint8_t)source, p, 0, out, cap, bytes_out);
}
