// ob_flash_common.h — what the flash kernel files share (ob_flash_bf16.hip:
// head_dim 64; ob_flash_hd128_bf16.hip: head_dim 128): the MFMA fragment
// types, the P -> A-fragment pack-and-exchange, the accumulator row map, and
// the C++ launchers of the hd-128 kernels that the public entries in
// ob_flash_bf16.hip dispatch to.
//
// v_mfma_f32_32x32x16_bf16 fragment layout (pinned by tests/test_gpu_bf16.py),
// il = lane&31, kh = lane>>5:
//   A: lane holds A[i = il][k = 8*kh + j], j = 0..7
//   B: lane holds B[k = 8*kh + j][n = il]
//   C/D: col = il, row = acc_row(r, kh)
#pragma once
#include "ob_bf16.h"

using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;

__device__ __forceinline__ unsigned bf_pk2(float a, float b) {
  return bf_bits((__bf16)a) | (bf_bits((__bf16)b) << 16);
}

// pack-and-exchange: acc-held values (rows pattern) -> A-fragment k-runs
__device__ __forceinline__ bf16x8 bf_dance(const float* pv8) {
  unsigned x0 = bf_pk2(pv8[0], pv8[1]);
  unsigned x1 = bf_pk2(pv8[2], pv8[3]);
  unsigned y0 = bf_pk2(pv8[4], pv8[5]);
  unsigned y1 = bf_pk2(pv8[6], pv8[7]);
  {
    auto r2 = __builtin_amdgcn_permlane32_swap(x0, y0, false, false);
    x0 = r2[0];
    y0 = r2[1];
  }
  {
    auto r2 = __builtin_amdgcn_permlane32_swap(x1, y1, false, false);
    x1 = r2[0];
    y1 = r2[1];
  }
  uint4 fr;
  fr.x = x0;
  fr.y = x1;
  fr.z = y0;
  fr.w = y1;
  return __builtin_bit_cast(bf16x8, fr);
}

// tile row of accumulator element r in lane half kh (the C/D layout above)
__device__ __forceinline__ int acc_row(int r, int kh) {
  return (r & 3) + 8 * (r >> 2) + 4 * kh;
}

// head_dim 128 launchers (ob_flash_hd128_bf16.hip).  Shapes are checked by
// the public entries: H == 128 * nh, S % 128 == 0.  0, or 1 with ob_fail set.
int ob_flash_hd128_fwd(const void* qkv, void* O, void* lse, int64_t B,
                       int64_t Sq, int64_t H, int64_t nh, float scale,
                       void* stream);
// O == nullptr: D is an input.  Otherwise the dq kernel forms D from O and
// dO and writes it to D for the dkdv launch that follows.
int ob_flash_hd128_bwd(const void* qkv, const void* O, const void* dO,
                       const void* lse, void* D, void* dqkv, void* dbias_qkv,
                       int64_t B, int64_t Sq, int64_t H, int64_t nh,
                       float scale, void* stream);
