// fspt_encode_device.hpp - device code the encoders' kernels share (fspt_jpeg.hip, fspt_png.hip, fspt_exr.hip); for .hip
// files only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace fspt {

// The inclusive scan of one value per thread of a workgroup of 256 (Hillis-Steele, in LDS), of N arrays side by side under
// one pair of barriers a step: thread t leaves v[k] in s[k][t] and finds the sum of the threads 0..t there afterwards,
// s[k][255] being the tile's total.  Ends with a barrier; the caller puts one between its last read of s and the next call.
template <class T, int N>
__device__ __forceinline__ void enc_scan256(T *const (&s)[N], const T (&v)[N]) {
  const uint32_t t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < N; ++k) s[k][t] = v[k];
  __syncthreads();
  for (uint32_t d = 1; d < 256u; d <<= 1) {
    T o[N];
#pragma unroll
    for (int k = 0; k < N; ++k) o[k] = t >= d ? s[k][t - d] : T(0);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) s[k][t] += o[k];
    __syncthreads();
  }
}
template <class T>
__device__ __forceinline__ void enc_scan256(T *s, T v) {
  T *const a[1] = {s};
  const T b[1] = {v};
  enc_scan256(a, b);
}

} // namespace fspt
