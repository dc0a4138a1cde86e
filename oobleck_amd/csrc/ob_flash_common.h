// ob_flash_common.h — what the flash kernel files share (ob_flash_bf16.hip:
// head_dim 64; ob_flash_hd128_bf16.hip: head_dim 128; ob_flash_win_bf16.hip:
// the locally banded kernels of both sizes; ob_flash_hd96_bf16.hip: head_dim
// 80 and 96, dense and banded): the MFMA fragment
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

// LDS images of a row-major bf16 tile and the transposed (column-wise) B
// fragment read from it.  nt_*: [rows][64], 128-byte rows, derived in
// ob_flash_bf16.hip; hd_*: [rows][128], 256-byte rows, derived in
// ob_flash_hd128_bf16.hip.  The transposed read needs EXEC all ones.
__device__ __forceinline__ int nt_key(int row) {
  return (((row >> 1) & 1) << 2) | ((row >> 2) & 3);
}
// element offset of 16-byte chunk `ch` (0..7) of row `row`
__device__ __forceinline__ int nt_off(int row, int ch) {
  return row * 64 + ((ch ^ nt_key(row)) << 3);
}
// B fragment (32x32x16, k-slab rows r0..r0+7, r0 % 8 == 0) of column
// 32*dhalf + (lane&31) from the row-major tile: two transposed reads of
// the 4x16 blocks at rows r0 / r0+4, first column 32*dhalf + 16*(il>>4).
// Lane i = lane&15 supplies row (i>>2), columns 4*(i&3)..+3 of its block.
__device__ __forceinline__ bf16x8 nt_tr_frag(const __bf16* tile, int lane,
                                             int r0, int dhalf) {
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  const int i = lane & 15;
  const int row = r0 + (i >> 2);
  const int ch = 4 * dhalf + 2 * ((lane >> 4) & 1) + ((i >> 1) & 1);
  const int sub = 4 * (i & 1);
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (lds_bf16x4*)(tile + nt_off(row, ch) + sub));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (lds_bf16x4*)(tile + nt_off(row + 4, ch) + sub));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

__device__ __forceinline__ int hd_key(int row) {
  return ((row & 3) << 2) | ((row >> 2) & 3);
}
// element offset of 16-byte chunk `ch` (0..15) of row `row`
__device__ __forceinline__ int hd_off(int row, int ch) {
  return row * 128 + ((ch ^ hd_key(row)) << 3);
}
// B fragment (32x32x16, k-slab rows r0..r0+7, r0 % 8 == 0) of column
// 32*dq + (lane&31) from the row-major tile: two transposed reads of the
// 4x16 blocks at rows r0 / r0+4, first column 32*dq + 16*(il>>4).  Lane
// i = lane&15 supplies row (i>>2), columns 4*(i&3)..+3 of its block.
__device__ __forceinline__ bf16x8 hd_tr_frag(const __bf16* tile, int lane,
                                             int r0, int dq) {
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  const int i = lane & 15;
  const int row = r0 + (i >> 2);
  const int ch = 4 * dq + 2 * ((lane >> 4) & 1) + ((i >> 1) & 1);
  const int sub = 4 * (i & 1);
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (lds_bf16x4*)(tile + hd_off(row, ch) + sub));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (lds_bf16x4*)(tile + hd_off(row + 4, ch) + sub));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// h96_*: [rows][96], 192-byte rows of twelve 16-byte chunks: the image of the
// head_dim 80 and 96 kernels (ob_flash_hd96_bf16.hip; at 80 chunks 10 and 11
// are padding).  Twelve is no power of two, so an XOR key over the whole chunk
// index (nt_key, hd_key) would leave the row; the key here flips the low two
// chunk bits only and stays inside an aligned group of 4 chunks:
//   chunk ch of row r lives at chunk slot  ch ^ key(r),  key(r) = (r>>2)&3.
// Bank = (byte/4) % 64: a 256-byte sweep holds sixteen 16-byte slots, and row
// r starts at slot 12r % 16 = 4 * ((-r) & 3).  So chunk ch of row r has sweep
// slot bits 3:2 = ((ch>>2) - r) & 3 and bits 1:0 = (ch&3) ^ ((r>>2)&3): the
// unpadded pitch rotates the groups of 4 by the row's low bits, the key
// permutes inside a group by the next two.
//  * transposed read, one 32-lane half = rows r0..r0+3 (r0 % 4 == 0) x one
//    aligned group of 4 chunks: bits 3:2 take one value per row, bits 1:0 are
//    a permutation inside the group -> 16 distinct slots, conflict-free.
//  * ds_read_b128 row read (lane il -> row il, one chunk index per half): its
//    16-lane groups hold rows {0-3,12-15,20-27} / {4-11,16-19,28-31}, four
//    aligned runs of 4 rows whose (r>>2)&3 are 0,3,1,2 / 1,2,0,3.  Inside a
//    run bits 3:2 take all four values; across the runs bits 1:0 do -> 16
//    distinct slots, conflict-free.
// key has period 16 in r, as hd_key.
__device__ __forceinline__ int h96_key(int row) { return (row >> 2) & 3; }
// element offset of 16-byte chunk `ch` (0..11) of row `row`
__device__ __forceinline__ int h96_off(int row, int ch) {
  return row * 96 + ((ch ^ h96_key(row)) << 3);
}
// B fragment (32x32x16, k-slab rows r0..r0+7, r0 % 8 == 0) of column
// 32*dt + (lane&31), dt = 0..2, from the row-major tile: the two transposed
// reads of hd_tr_frag.
__device__ __forceinline__ bf16x8 h96_tr_frag(const __bf16* tile, int lane,
                                              int r0, int dt) {
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  const int i = lane & 15;
  const int row = r0 + (i >> 2);
  const int ch = 4 * dt + 2 * ((lane >> 4) & 1) + ((i >> 1) & 1);
  const int sub = 4 * (i & 1);
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (lds_bf16x4*)(tile + h96_off(row, ch) + sub));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (lds_bf16x4*)(tile + h96_off(row + 4, ch) + sub));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
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
