// ob_flash_common.h — what the flash kernel files share (ob_flash_bf16.hip:
// head_dim 64; ob_flash_hd128_bf16.hip: head_dim 128): the MFMA fragment
// types, the P -> A-fragment pack-and-exchange, the accumulator row map, and
// the in-register attention dropout mask helpers, and the C++ launchers of
// the hd-128 kernels that the public entries in ob_flash_bf16.hip dispatch
// to.
//
// v_mfma_f32_32x32x16_bf16 fragment layout (pinned by tests/test_gpu_bf16.py),
// il = lane&31, kh = lane>>5:
//   A: lane holds A[i = il][k = 8*kh + j], j = 0..7
//   B: lane holds B[k = 8*kh + j][n = il]
//   C/D: col = il, row = acc_row(r, kh)
#pragma once
#include "ob_bf16.h"
#include "ob_philox.h"

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

// Attention dropout.  The mask
// is ob_philox.h's, site OB_DROP_ATTN: element e = (z*S + q)*S + kv of the
// full [B*nh, S, S] square, word e & 3 of ob_drop_words(key, e >> 2), and
// ob_drop_factor's rule (word >= thr keeps, kept values times key.scale).
// It does not depend on the head size.
// No mask touches memory: a Philox call covers four consecutive, 4-aligned
// kv of one q row, S % 4 == 0, and e < 2^34 (checked by the entries), so
//   e >> 2 = (z*S + q) * (S/4) + (kv >> 2)   fits 32 bits.
// The kernels keep the keep bits of a tile in one register and apply
// `bit ? key.scale : 0` where ob_drop_factor would.  Only elements at or
// below the diagonal ever reach a product that matters: masked P is 0
// before the factor multiplies it.  The mask code is plain VALU (plus one
// quad exchange in dkdv) under wave-uniform control and holds no
// transposed read and no barrier.
//
// forward / dq orientation: a lane holds q = myq and, per 32-kv sub-tile u,
// the kv rows kv0 + 32u + acc_row(r, kh): group g = r>>2 is the 4-aligned
// run kv0 + 32u + 8g + 4kh, i.e. exactly one Philox call, counter
// crow + 8u + 2g with crow = drop_crow(z, S, myq, kh) + kv0/4.  Bit 16u + r
// = keep of sub-tile u, element r.  kCalls = 8 draws a 64-kv tile, kCalls =
// 4 one 32-kv sub-tile (crow advanced by 8u), in a rolled loop: unrolled,
// the temporaries push the kernels into scratch.
__device__ __forceinline__ uint32_t drop_crow(int z, int Sq, int q, int kh) {
  return (uint32_t)(z * Sq + q) * (uint32_t)(Sq >> 2) + (uint32_t)kh;
}
template <int kCalls = 8>
__device__ __forceinline__ uint32_t drop_bits_q(const ob_drop_key& key,
                                                uint32_t crow) {
  uint32_t bits = 0;
#pragma unroll 1
  for (int i = 0; i < kCalls; ++i) {  // i = 4u + g
    const ob_philox4 w = ob_drop_words(key, crow + 2 * i);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      bits |= (uint32_t)(w.w[j] >= key.thr) << (4 * i + j);
  }
  return bits;
}
__device__ __forceinline__ float drop_factor_bit(const ob_drop_key& key,
                                                 uint32_t bits, int i) {
  return ((bits >> i) & 1u) ? key.scale : 0.f;
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
