// ob_bf16.h — bf16 bit helpers shared by ob_kernels_bf16.hip,
// ob_gemm_bf16.hip and ob_flash_bf16.hip.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float bf2f(__bf16 h) { return (float)h; }

__device__ __forceinline__ unsigned bf_bits(__bf16 h) {
  return (unsigned)__builtin_bit_cast(unsigned short, h);
}
__device__ __forceinline__ __bf16 bits_bf(unsigned u) {
  return __builtin_bit_cast(__bf16, (unsigned short)(u & 0xffffu));
}

__device__ __forceinline__ __bf16 bf_extract(const uint4& v, int j) {
  // j is a compile-time constant at every call site (unrolled loops)
  const unsigned word = (j < 2) ? v.x : (j < 4) ? v.y : (j < 6) ? v.z : v.w;
  return bits_bf((j & 1) ? (word >> 16) : word);
}

__device__ __forceinline__ uint4 bf_pack8(const float* v) {
  uint4 o;
  o.x = bf_bits((__bf16)v[0]) | (bf_bits((__bf16)v[1]) << 16);
  o.y = bf_bits((__bf16)v[2]) | (bf_bits((__bf16)v[3]) << 16);
  o.z = bf_bits((__bf16)v[4]) | (bf_bits((__bf16)v[5]) << 16);
  o.w = bf_bits((__bf16)v[6]) | (bf_bits((__bf16)v[7]) << 16);
  return o;
}
