/* camera_model_mock_stub.c - fspt_target_set_camera_model / _get_camera_model for the addon built against
 * tests/napi_mock/libfspt_mock.c (tests/test_camera_model_cpu.py, tests/test_camera_model_node.py): they validate like the
 * library (include/fspt.h) and keep what reached them; g_cm_calls counts the calls that did. */
#include <math.h>
#include <stdint.h>
#include "fspt.h"

static fspt_camera_model_params g_cm = {FSPT_CAMERA_PINHOLE, 3.14159265f, 0.064f};
static int g_cm_calls;

int fspt_target_set_camera_model(fspt_target *t, const fspt_camera_model_params *p) {
  fspt_camera_model_params m = {FSPT_CAMERA_PINHOLE, 3.14159265f, 0.064f};
  uint32_t W = 0, H = 0;
  if (!t) return FSPT_E_INVALID;
  g_cm_calls += 1;
  if (p) m = *p;
  if (m.model < FSPT_CAMERA_PINHOLE || m.model > FSPT_CAMERA_STEREO) return FSPT_E_INVALID;
  if (m.model == FSPT_CAMERA_FISHEYE && !(isfinite(m.angle) && m.angle > 0.0f && m.angle <= 6.2831855f)) return FSPT_E_INVALID;
  if (m.model == FSPT_CAMERA_STEREO && !(isfinite(m.ipd) && m.ipd >= 0.0f)) return FSPT_E_INVALID;
  fspt_target_size(t, &W, &H);
  if (m.model == FSPT_CAMERA_STEREO && (H & 1u)) return FSPT_E_INVALID;
  g_cm = m;
  return FSPT_OK;
}
int fspt_target_get_camera_model(fspt_target *t, fspt_camera_model_params *p) {
  if (!t || !p) return FSPT_E_INVALID;
  *p = g_cm;
  p->ipd = p->ipd + 1000.0f * (float)g_cm_calls; /* (the calls that reached the library, readable through the getter) */
  return FSPT_OK;
}
