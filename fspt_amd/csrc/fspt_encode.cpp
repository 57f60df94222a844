// fspt_encode.cpp - the host code the three image encoders share (fspt_jpeg.hip, fspt_png.hip, fspt_exr.hip):
// the output buffers and events of an encoder, the delivery of a finished file, the stage times behind fspt_*_last_ms and
// the sequence of a stand-alone entry.  What a format decides for itself - its plan, its header, its work buffers, its
// launches - stays in its own file.
#include "fspt_internal.hpp"

namespace fspt {

EncFormat g_jpeg_format = {"frame", 4u, {0.0f, 0.0f, 0.0f}, 0}, g_png_format = {"file", 4u, {0.0f, 0.0f, 0.0f}, 0}, g_exr_format = {"file", 8u, {0.0f, 0.0f, 0.0f}, 0};

hipError_t enc_ensure_out(EncCommon &c, int n_out, size_t out_bytes) {
  hipError_t err = hipSuccess;
  if (out_bytes > c.out_bytes) { // the buffers only grow, all of them together: every one that is there has c.out_bytes
    for (uint8_t *&o : c.out) { hipFree(o); o = nullptr; }
    c.out_bytes = out_bytes;
  }
  for (int k = 0; k < n_out && err == hipSuccess; ++k)
    if (!c.out[k] && (err = hipMalloc((void **)&c.out[k], c.out_bytes)) != hipSuccess) c.out[k] = nullptr;
  for (hipEvent_t &ev : c.ev) if (!ev && err == hipSuccess) err = hipEventCreate(&ev);
  return err;
}

void enc_replan(EncCommon &c) {
  c.work.clear();
  c.valid = false;
}

void enc_release(EncCommon &c) {
  enc_replan(c);
  for (uint8_t *&o : c.out) { hipFree(o); o = nullptr; }
  for (hipEvent_t &ev : c.ev) { if (ev) hipEventDestroy(ev); ev = nullptr; }
  c.out_bytes = 0;
}

int enc_deliver(const uint8_t *dev, uint64_t n, uint8_t *out, size_t cap, size_t *bytes_out, hipStream_t st, const char *fn, EncFormat &f) {
  *bytes_out = (size_t)n;
  if (cap < n) { fspt_set_error("%s: the %s takes %llu bytes, the buffer holds %zu", fn, f.noun, (unsigned long long)n, cap); return FSPT_E_INVALID; }
  hipError_t err = hipMemcpyAsync(out, dev, (size_t)n, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) { fspt_set_error("%s: %s", fn, hipGetErrorString(err)); return FSPT_E_HIP; }
  f.bus_bytes = n + f.len_bytes;
  return FSPT_OK;
}

int enc_collect(const void *len_dev, const uint8_t *dev, uint8_t *out, size_t cap, size_t *bytes_out, hipStream_t st, const char *fn, EncFormat &f) {
  uint64_t n64 = 0;
  uint32_t n32 = 0;
  hipError_t err = hipMemcpyAsync(f.len_bytes == 8u ? (void *)&n64 : (void *)&n32, len_dev, f.len_bytes, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) { fspt_set_error("%s: %s", fn, hipGetErrorString(err)); return FSPT_E_HIP; }
  return enc_deliver(dev, f.len_bytes == 8u ? n64 : n32, out, cap, bytes_out, st, fn, f);
}

void enc_note_ms(const EncCommon &c, EncFormat &f) {
  for (int k = 0; k < 3; ++k) if (hipEventElapsedTime(&f.ms[k], c.ev[k], c.ev[k + 1]) != hipSuccess) f.ms[k] = 0.0f;
  (void)hipGetLastError();
}

int enc_last_ms(const EncFormat &f, const char *fn, float ms[3], uint64_t *bus_bytes) {
  if (!ms) { fspt_set_error("%s: NULL argument", fn); return FSPT_E_INVALID; }
  std::memcpy(ms, f.ms, sizeof f.ms);
  if (bus_bytes) *bus_bytes = f.bus_bytes;
  return FSPT_OK;
}

hipError_t enc_upload(Hold &hold, const void *host, size_t bytes, const void **dev) {
  void *d = nullptr;
  hipError_t err = hold.make(&d, bytes);
  if (err == hipSuccess) err = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
  *dev = d;
  return err;
}

int enc_enter(const char *fn, int device) {
  if (fspt_device_count() <= 0) { fspt_set_error("%s: no HIP device available; libfspt has no CPU fallback", fn); return FSPT_E_NO_DEVICE; }
  return check_device(device);
}

int enc_fail(const char *fn, hipError_t err) {
  (void)hipDeviceSynchronize(); (void)hipGetLastError();
  fspt_set_error("%s: %s", fn, hipGetErrorString(err));
  return err == hipErrorOutOfMemory ? FSPT_E_NOMEM : FSPT_E_HIP;
}

} // namespace fspt
