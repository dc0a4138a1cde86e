// ob_flash_hd96_bf16.hip — causal flash attention, bf16, head_dim 80 and 96
// (GPT-3 2.7B and 760M), dense and locally banded.
// Query row i attends the keys j with i - W < j <= i; dense is W = S.  Three
// kernels, each a template on HD in {80, 96}: forward (O and the row LSE of
// the scaled scores), dQ (forming D = rowsum(dO * O) the way
// ob_flash_bwd_nt_d_bf16 does) and dK/dV; the backward recomputes P from Q, K
// and LSE.
//
// The arithmetic is the other flash files': v_mfma_f32_32x32x16_bf16, swapped
// QK^T so a lane owns one q column, bf_dance into the PV / dS A fragment,
// transposed B operands read column-wise from the row-major LDS tile,
// double-buffered tiles under one barrier per tile, `scale` folded in the
// same places, and the masked-row rules of ob_flash_win_bf16.hip's forward
// (rescale test `mt > m + 8`, factor 1 where the max did not move, a masked P
// is 0 without an exp).  What is this file's own:
//
// A head size that is no multiple of 32.  Chains that contract over the head
// dim (QK^T, dP = dO V^T) take HD/16 k-steps: 6, or exactly 5.  Chains that
// produce the head dim (PV, dQ, dK, dV) take 3 accumulators of 32 columns;
// at HD = 80 the upper 16 columns of the third are padding, about 20 % more
// MFMAs on those chains than 80 columns need.  They come from B-operand
// columns 80..95 of the LDS tile (chunks 10 and 11 of a row, which no staging
// store touches) and reach only accumulator columns 80..95.  h96_zero_pad
// clears those chunks once before the first barrier; every store, the D sum
// and the dbias sums stop at column HD.
//
// LDS image.  Rows of 96 elements (192 bytes) at both head sizes, h96_off /
// h96_tr_frag of ob_flash_common.h, where the bank pattern is derived.
//
// Staging.  A [ROWS][HD] tile is ROWS * HD/8 16-byte chunks dealt to the 256
// threads in order: 3 per thread for 64 x 96; 2.5 for 64 x 80 and 1.5 / 1.25
// for the 32-row tiles, where the last load is guarded.  The guard's boundary
// is a multiple of 64 threads, so it is wave-uniform.  All loads are issued
// before the first store.
//
// One body, two block maps.  A wave carries its first row and the tile range
// its rows reach; the block stages the union of its waves' ranges.
//   dense (W >= S): the fold of ob_flash_fold.h (ob_fold_q_row0 /
//     ob_fold_kv_row0): a light piece and its mirror-image heavy piece;
//   banded: consecutive rows, the map and ranges of ob_flash_win_bf16.hip.
// Both use the same range formulas (win_first_tile / win_last_qtile below,
// which give 0 and the last tile at W = S), the linear-id map ob_fold_id, and
// one mask: `(unsigned)(q - kv) < W`, the causal and the band test in one
// compare, on edge tiles only.
//
// The kernels are compiled without packed fp32 VALU ops, like the banded and
// dropout kernels; the bodies are forceinline device templates under
// attributed __global__ wrappers for the reason given in
// ob_flash_hd128_bf16.hip.  Resources: profiles/flash_hd96_resources.txt.
//
// Attention dropout (the mask definition and helpers are
// ob_flash_common.h's).  Each body is also a template on kDrop, under a `_drop`
// __global__ wrapper that takes the ob_drop_key by value; the kDrop = false
// instantiations compile to the resources they had
// (profiles/flash_band_drop_resources.txt).  m, l and the LSE come from the
// undropped, masked P; the factor multiplies the PV operand only, in fp32 just
// before bf_dance, so a masked P stays an exact 0 and bits drawn outside the
// band are harmless.
//   forward: the tile's 32 keep bits (drop_bits_q<8>, counter from the tile's
//     true kv0) are drawn at the top of the iteration, before the staging
//     loads, and only in the tiles the wave computes;
//   dQ: a sub-tile's 16 bits (drop_bits_q<4>) just before its S and dP chains,
//     inside the wave-uniform band test, so a skipped sub-tile draws nothing;
//     dS = P * (f * dP - D);
//   dK/dV: role 0 makes the quad-shared draw of the dense kernels (four Philox
//     calls per lane, packed bits exchanged within the quad) at the top of an
//     iteration its pair computes, and hands the keep bit to role 1 as the
//     sign of the fp32 P it writes to xch (P >= 0, a masked P is +0 or -0 and
//     multiplies to 0 either way); role 1 draws nothing.
// At HD = 80 the factor multiplies P, never V: accumulator columns 80..95 keep
// receiving zeros and every store still stops at column HD.
//
// Out of scope: the fp32 and materialized-P banded routes.
#include "ob_flash_common.h"
#include "ob_internal.h"
#include "ob_flash_fold.h"

#include <cmath>

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

#define OB_HD96_KERNEL __attribute__((target("no-packed-fp32-ops")))

// ---- tile ranges (the banded kernels' formulas; W = S gives the dense ones) -
// first 64-row kv tile a q row reaches: floor((row - W + 1) / 64), clamped
__device__ __forceinline__ int h96_first_tile(int row, int W) {
  const int lo = row - W + 1;
  return lo > 0 ? lo / 64 : 0;
}
// last 32-row q tile that reaches a 32-row kv tile starting at kv0: its last
// row kv0 + 31 is seen by the q rows up to kv0 + 31 + W - 1
__device__ __forceinline__ int h96_last_qtile(int kv0, int W, int Sq) {
  const int64_t hi = (int64_t)kv0 + 31 + W - 1;
  return hi >= Sq ? Sq / 32 - 1 : (int)(hi / 32);
}

// Stages two [ROWS][HD] tiles (rows lda / ldb elements apart in memory) into
// their h96 images: chunk e = tid + 256 i is chunk e % (HD/8) of row
// e / (HD/8).  All the loads are issued before the first store.
template <int HD, int ROWS>
__device__ __forceinline__ void h96_stage2(__bf16* da, const __bf16* a,
                                           int64_t lda, __bf16* db,
                                           const __bf16* b, int64_t ldb,
                                           int tid) {
  constexpr int CH = HD / 8, TOT = ROWS * CH, N = (TOT + 255) / 256;
  static_assert(TOT % 64 == 0, "the tail guard must be wave-uniform");
  bf16x8 ra[N], rb[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int e = tid + 256 * i, sr = e / CH, sc = e % CH;
    if (256 * (i + 1) <= TOT || e < TOT) {
      ra[i] = *reinterpret_cast<const bf16x8*>(a + sr * lda + sc * 8);
      rb[i] = *reinterpret_cast<const bf16x8*>(b + sr * ldb + sc * 8);
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int e = tid + 256 * i, sr = e / CH, sc = e % CH;
    if (256 * (i + 1) <= TOT || e < TOT) {
      *reinterpret_cast<bf16x8*>(da + h96_off(sr, sc)) = ra[i];
      *reinterpret_cast<bf16x8*>(db + h96_off(sr, sc)) = rb[i];
    }
  }
}

// HD = 80: clears chunks 10 and 11 of the `rows` rows at `t` (both buffers of
// a tile pair are contiguous).  The key keeps them inside chunks 8..11, away
// from what h96_stage2 writes.
template <int HD>
__device__ __forceinline__ void h96_zero_pad(__bf16* t, int rows, int tid) {
  if constexpr (HD == 80) {
    for (int e = tid; e < 2 * rows; e += 256)
      *reinterpret_cast<bf16x8*>(t + h96_off(e >> 1, 10 + (e & 1))) = bf16x8{};
  }
}

// ===========================================================================
// Forward.  Block: 4 waves x 32 q rows; 64-row kv tiles.
// LDS: 2 x (K + V tile) x 64 x 96 x 2 B + bcast = 48.5 KB.
// ===========================================================================
template <int HD, bool kDrop>
__device__ __forceinline__ void h96_fwd_body(
    const __bf16* __restrict__ qkv, __bf16* __restrict__ Obase,
    float* __restrict__ lse, int Sq, int H, int nh, int Z, int W,
    float scale, const ob_drop_key& key) {
  constexpr int NS = HD / 16;
  __shared__ __attribute__((aligned(16))) __bf16 kbuf[2][64 * 96];
  __shared__ __attribute__((aligned(16))) __bf16 vbuf[2][64 * 96];
  __shared__ float bcast[128];
  int blk, z;
  if (!ob_fold_id(blockIdx.x, Sq / 128, Z, &blk, &z))
    return;  // block-uniform: grid padding
  const int b = z / nh, h = z % nh;
  const int64_t ld = 3 * (int64_t)H;
  const __bf16* Qp = qkv + (int64_t)b * Sq * ld + h * HD;
  const __bf16* Kp = Qp + H;
  const __bf16* Vp = Qp + 2 * H;
  __bf16* Op = Obase + (int64_t)b * Sq * H + h * HD;
  float* lsep = lse + (int64_t)z * Sq;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int il = lane & 31, kh = lane >> 5;
  const bool dense = W >= Sq;  // kernel-uniform
  const int q0 = dense ? ob_fold_q_row0(Sq, blk, w) : 128 * blk + 32 * w;
  const int myq = q0 + il;
  // wave-uniform computed range; the block stages wave 0's first tile (its
  // rows are the block's lowest in both maps) to wave 3's diagonal
  const int w_lo = h96_first_tile(q0, W), w_hi = (q0 + 31) >> 6;
  const int t_lo =
      h96_first_tile(dense ? ob_fold_q_row0(Sq, blk, 0) : 128 * blk, W);
  const int t_hi =
      ((dense ? ob_fold_q_row0(Sq, blk, 3) : 128 * blk + 96) + 31) >> 6;

  bf16x8 qf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s)
    qf[s] = *reinterpret_cast<const bf16x8*>(Qp + myq * ld + s * 16 + kh * 8);

  h96_zero_pad<HD>(vbuf[0], 128, tid);
  h96_stage2<HD, 64>(kbuf[0], Kp + t_lo * 64 * ld, ld, vbuf[0],
                     Vp + t_lo * 64 * ld, ld, tid);
  __syncthreads();

  f32x16 o[3] = {};
  float m = -INFINITY, l = 0.f;
  for (int kvt = t_lo; kvt <= t_hi; ++kvt) {
    const int kv0 = kvt * 64;
    const int buf = (kvt - t_lo) & 1;
    [[maybe_unused]] uint32_t keep = 0;  // bit 16u + r, as drop_bits_q
    if constexpr (kDrop)
      if (kvt >= w_lo && kvt <= w_hi)  // wave-uniform
        keep = drop_bits_q(key, drop_crow(z, Sq, myq, kh) + (kv0 >> 2));
    if (kvt < t_hi)
      h96_stage2<HD, 64>(kbuf[buf ^ 1], Kp + (kv0 + 64) * ld, ld,
                         vbuf[buf ^ 1], Vp + (kv0 + 64) * ld, ld, tid);
    if (kvt >= w_lo && kvt <= w_hi) {  // wave-uniform
      const __bf16* kb = kbuf[buf];
      const __bf16* vb = vbuf[buf];
      f32x16 sacc0 = {}, sacc1 = {};
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int ch = s * 2 + kh;
        const bf16x8 ka =
            *reinterpret_cast<const bf16x8*>(&kb[h96_off(il, ch)]);
        const bf16x8 kb2 =
            *reinterpret_cast<const bf16x8*>(&kb[h96_off(32 + il, ch)]);
        sacc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qf[s], sacc0, 0,
                                                        0, 0);
        sacc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kb2, qf[s], sacc1,
                                                        0, 0, 0);
      }
      float sv[32];
      // interior: every kv of the tile <= every q of the wave, and the
      // tile's first kv inside the band of the wave's last row
      if (kv0 + 63 <= q0 && kv0 > q0 + 31 - W) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          sv[r] = sacc0[r] * scale;
          sv[16 + r] = sacc1[r] * scale;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const unsigned dist = (unsigned)(myq - (kv0 + acc_row(r, kh)));
          sv[r] = dist < (unsigned)W ? sacc0[r] * scale : -INFINITY;
          sv[16 + r] =
              dist - 32u < (unsigned)W ? sacc1[r] * scale : -INFINITY;
        }
      }
      float mx[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        mx[j] = fmaxf(fmaxf(sv[j], sv[8 + j]),
                      fmaxf(sv[16 + j], sv[24 + j]));
      float mt = fmaxf(fmaxf(fmaxf(mx[0], mx[1]), fmaxf(mx[2], mx[3])),
                       fmaxf(fmaxf(mx[4], mx[5]), fmaxf(mx[6], mx[7])));
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
      // m may be -inf here (a row fully masked so far)
      if (__any(mt > m + 8.f)) {
        const float mnew = fmaxf(m, mt);
        const float af = (mnew == m) ? 1.f : __expf(m - mnew);
        m = mnew;
        if (kh == 0) bcast[w * 32 + il] = af;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float a = bcast[w * 32 + acc_row(r, kh)];
#pragma unroll
          for (int d = 0; d < 3; ++d) o[d][r] *= a;
        }
        l *= af;
      }
      float ps[8] = {};
#pragma unroll
      for (int r = 0; r < 32; ++r) {
        sv[r] = (sv[r] == -INFINITY) ? 0.f : __expf(sv[r] - m);
        ps[r & 7] += sv[r];
      }
      float psum = ((ps[0] + ps[1]) + (ps[2] + ps[3])) +
                   ((ps[4] + ps[5]) + (ps[6] + ps[7]));
      psum += __shfl_xor(psum, 32, 64);
      l += psum;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if constexpr (kDrop) {
#pragma unroll
          for (int r = 8 * t; r < 8 * t + 8; ++r)
            sv[r] *= drop_factor_bit(key, keep, r);
        }
        const bf16x8 pa = bf_dance(sv + t * 8);
        // B[k = kv 16t+8kh..+7][n = d]: columns of the row-major V tile
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const bf16x8 vf = h96_tr_frag(vb, lane, t * 16 + kh * 8, d);
          o[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa, vf, o[d], 0, 0,
                                                         0);
        }
      }
    }
    __syncthreads();
  }

  if (kh == 0) {
    bcast[w * 32 + il] = 1.f / l;
    lsep[myq] = m + __logf(l);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = acc_row(r, kh);
    const float inv = bcast[w * 32 + row];
#pragma unroll
    for (int d = 0; d < 3; ++d)
      if (32 * d + il < HD)  // HD = 80: the third group's upper half is pad
        Op[(int64_t)(q0 + row) * H + 32 * d + il] = (__bf16)(o[d][r] * inv);
  }
}
template <int HD>
__global__ OB_HD96_KERNEL __launch_bounds__(256, 2) void k_flash_fwd_hd96(
    const __bf16* __restrict__ qkv, __bf16* __restrict__ Obase,
    float* __restrict__ lse, int Sq, int H, int nh, int Z, int W,
    float scale) {
  h96_fwd_body<HD, false>(qkv, Obase, lse, Sq, H, nh, Z, W, scale,
                          ob_drop_key{});
}
template <int HD>
__global__ OB_HD96_KERNEL __launch_bounds__(256, 2) void k_flash_fwd_hd96_drop(
    const __bf16* __restrict__ qkv, __bf16* __restrict__ Obase,
    float* __restrict__ lse, int Sq, int H, int nh, int Z, int W, float scale,
    ob_drop_key key) {
  h96_fwd_body<HD, true>(qkv, Obase, lse, Sq, H, nh, Z, W, scale, key);
}

// ===========================================================================
// dQ: the forward's blocks, ranges and K/V staging.  The two 32-row kv
// sub-tiles of a tile run one after the other; a sub-tile wholly outside the
// wave's band is skipped, wave-uniformly.  D is formed from the resident dO
// fragments and O loaded in the same layout (columns < HD only), used, and
// written to Dout for the dK/dV launch that follows.
// LDS: 2 x (K + V tile) + red = 49.5 KB.
// ===========================================================================
template <int HD, bool kDrop>
__device__ __forceinline__ void h96_dq_body(
    const __bf16* __restrict__ qkv, const __bf16* __restrict__ dO,
    const float* __restrict__ lse, const __bf16* __restrict__ O,
    float* __restrict__ Dout, __bf16* __restrict__ dqkv,
    float* __restrict__ dbias, int Sq, int H, int nh, int Z, int W,
    float scale, const ob_drop_key& key) {
  constexpr int NS = HD / 16;
  __shared__ __attribute__((aligned(16))) __bf16 kbuf[2][64 * 96];
  __shared__ __attribute__((aligned(16))) __bf16 vbuf[2][64 * 96];
  __shared__ float red[4 * 96];
  int blk, z;
  if (!ob_fold_id(blockIdx.x, Sq / 128, Z, &blk, &z))
    return;  // block-uniform: grid padding
  const int b = z / nh, h = z % nh;
  const int64_t ld = 3 * (int64_t)H;
  const int64_t base = (int64_t)b * Sq * ld + h * HD;
  const __bf16* Qp = qkv + base;
  const __bf16* Kp = Qp + H;
  const __bf16* Vp = Qp + 2 * H;
  const int64_t obase = (int64_t)b * Sq * H + h * HD;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int il = lane & 31, kh = lane >> 5;
  const bool dense = W >= Sq;  // kernel-uniform
  const int q0 = dense ? ob_fold_q_row0(Sq, blk, w) : 128 * blk + 32 * w;
  const int myq = q0 + il;
  const int t_lo =
      h96_first_tile(dense ? ob_fold_q_row0(Sq, blk, 0) : 128 * blk, W);
  const int t_hi =
      ((dense ? ob_fold_q_row0(Sq, blk, 3) : 128 * blk + 96) + 31) >> 6;
  const float mylse = lse[(int64_t)z * Sq + myq];

  bf16x8 qf[NS], df[NS];
  float part = 0.f;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    qf[s] = *reinterpret_cast<const bf16x8*>(Qp + myq * ld + s * 16 + kh * 8);
    df[s] = *reinterpret_cast<const bf16x8*>(dO + obase + (int64_t)myq * H +
                                             s * 16 + kh * 8);
    const bf16x8 ov = *reinterpret_cast<const bf16x8*>(
        O + obase + (int64_t)myq * H + s * 16 + kh * 8);
    float c = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) c += bf2f(ov[j]) * bf2f(df[s][j]);
    part += c;
  }
  const float myD = part + __shfl_xor(part, 32, 64);
  if (kh == 0) Dout[(int64_t)z * Sq + myq] = myD;

  h96_zero_pad<HD>(kbuf[0], 128, tid);  // K is this kernel's B operand
  h96_stage2<HD, 64>(kbuf[0], Kp + t_lo * 64 * ld, ld, vbuf[0],
                     Vp + t_lo * 64 * ld, ld, tid);
  __syncthreads();

  f32x16 dq[3] = {};
  for (int kvt = t_lo; kvt <= t_hi; ++kvt) {
    const int kv0 = kvt * 64;
    const int buf = (kvt - t_lo) & 1;
    if (kvt < t_hi)
      h96_stage2<HD, 64>(kbuf[buf ^ 1], Kp + (kv0 + 64) * ld, ld,
                         vbuf[buf ^ 1], Vp + (kv0 + 64) * ld, ld, tid);
    const __bf16* kb = kbuf[buf];
    const __bf16* vb = vbuf[buf];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int kvu = kv0 + 32 * u;
      // wave-uniform: the sub-tile starts at or below the wave's last row
      // and ends inside the band of its first row
      if (kvu <= q0 + 31 && kvu + 31 > q0 - W) {
        [[maybe_unused]] uint32_t keep = 0;  // bit r of this sub-tile
        if constexpr (kDrop)
          keep = drop_bits_q<4>(
              key, drop_crow(z, Sq, myq, kh) + (kv0 >> 2) + 8 * u);
        f32x16 sa = {}, pa = {};
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const int ch = s * 2 + kh;
          const bf16x8 ka = *reinterpret_cast<const bf16x8*>(
              &kb[h96_off(32 * u + il, ch)]);
          const bf16x8 va = *reinterpret_cast<const bf16x8*>(
              &vb[h96_off(32 * u + il, ch)]);
          sa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qf[s], sa, 0, 0,
                                                       0);
          pa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, df[s], pa, 0, 0,
                                                       0);
        }
        float dsv[16];
        // dS = P * (dP - D); a masked P is 0 without an exp.  Interior
        // sub-tile (all of it inside the band of all 32 rows): no mask
        if (kvu + 31 <= q0 && kvu > q0 + 31 - W) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            // kDrop: dS = P * (f * dP - D)
            float dp = pa[r];
            if constexpr (kDrop) dp *= drop_factor_bit(key, keep, r);
            dsv[r] = __expf(sa[r] * scale - mylse) * (dp - myD);
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const bool ok =
                (unsigned)(myq - (kvu + acc_row(r, kh))) < (unsigned)W;
            float dp = pa[r];
            if constexpr (kDrop) dp *= drop_factor_bit(key, keep, r);
            dsv[r] = ok ? __expf(sa[r] * scale - mylse) * (dp - myD) : 0.f;
          }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const bf16x8 da = bf_dance(dsv + t * 8);
          // B[k = kv 32u+16t+8kh..+7][n = d]: columns of the K tile
#pragma unroll
          for (int d = 0; d < 3; ++d) {
            const bf16x8 kt =
                h96_tr_frag(kb, lane, 32 * u + 16 * t + kh * 8, d);
            dq[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da, kt, dq[d], 0,
                                                            0, 0);
          }
        }
      }
    }
    __syncthreads();
  }
  __bf16* dQp = dqkv + base;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int q = q0 + acc_row(r, kh);
#pragma unroll
    for (int d = 0; d < 3; ++d)
      if (32 * d + il < HD)
        dQp[q * ld + 32 * d + il] = (__bf16)(scale * dq[d][r]);
  }
  if (dbias) {  // kernel-uniform
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      float c = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) c += scale * dq[d][r];
      c += __shfl_xor(c, 32, 64);
      if (kh == 0 && 32 * d + il < HD) red[w * HD + 32 * d + il] = c;
    }
    __syncthreads();
    if (tid < HD)
      atomicAdd(dbias + h * HD + tid,
                (red[tid] + red[HD + tid]) +
                    (red[2 * HD + tid] + red[3 * HD + tid]));
  }
}
template <int HD>
__global__ OB_HD96_KERNEL __launch_bounds__(256, 2) void k_flash_bwd_dq_hd96(
    const __bf16* __restrict__ qkv, const __bf16* __restrict__ dO,
    const float* __restrict__ lse, const __bf16* __restrict__ O,
    float* __restrict__ Dout, __bf16* __restrict__ dqkv,
    float* __restrict__ dbias, int Sq, int H, int nh, int Z, int W,
    float scale) {
  h96_dq_body<HD, false>(qkv, dO, lse, O, Dout, dqkv, dbias, Sq, H, nh, Z, W,
                         scale, ob_drop_key{});
}
template <int HD>
__global__ OB_HD96_KERNEL __launch_bounds__(256, 2) void
k_flash_bwd_dq_hd96_drop(const __bf16* __restrict__ qkv,
                         const __bf16* __restrict__ dO,
                         const float* __restrict__ lse,
                         const __bf16* __restrict__ O,
                         float* __restrict__ Dout, __bf16* __restrict__ dqkv,
                         float* __restrict__ dbias, int Sq, int H, int nh,
                         int Z, int W, float scale, ob_drop_key key) {
  h96_dq_body<HD, true>(qkv, dO, lse, O, Dout, dqkv, dbias, Sq, H, nh, Z, W,
                        scale, key);
}

// ===========================================================================
// dK/dV: split-duty wave pairs (role 0: K resident, S -> P -> dV; role 1: V
// resident, dP -> dS -> dK; only P crosses the pair, through xch) over 32-row
// q tiles.  A pair idles, staging and meeting the barrier only, before its
// diagonal tile and after the last tile its rows' bands reach.  The B
// fragments are read before the iteration's barrier: after it a fast wave
// already stages tile qt+2 into this buffer.  Both staged tiles (Q and dO) are
// B operands here.
// LDS: xch 16 KB + 2 x (Q + dO tile) x 32 x 96 x 2 B + red = 41.5 KB.
// ===========================================================================
template <int HD, bool kDrop>
__device__ __forceinline__ void h96_dkdv_body(
    const __bf16* __restrict__ qkv, const __bf16* __restrict__ dO,
    const float* __restrict__ lse, const float* __restrict__ D,
    __bf16* __restrict__ dqkv, float* __restrict__ dbias, int Sq, int H,
    int nh, int Z, int W, float scale, const ob_drop_key& key) {
  constexpr int NS = HD / 16;
  __shared__ float xch[2][2][32 * 32];  // [buffer][pair][P tile]
  __shared__ __attribute__((aligned(16))) __bf16 qbuf[2][32 * 96];
  __shared__ __attribute__((aligned(16))) __bf16 obuf[2][32 * 96];
  __shared__ float red[4 * 96];
  int blk, z;
  if (!ob_fold_id(blockIdx.x, Sq / 64, Z, &blk, &z))
    return;  // block-uniform: grid padding
  const int b = z / nh, h = z % nh;
  const int64_t ld = 3 * (int64_t)H;
  const int64_t base = (int64_t)b * Sq * ld + h * HD;
  const __bf16* Qp = qkv + base;
  const __bf16* dOp = dO + (int64_t)b * Sq * H + h * HD;
  const float* lsep = lse + (int64_t)z * Sq;
  const float* Dp = D + (int64_t)z * Sq;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int pair = w >> 1, role = w & 1;
  const int il = lane & 31, kh = lane >> 5;
  const bool dense = W >= Sq;  // kernel-uniform
  const int kv0 = dense ? ob_fold_kv_row0(Sq, blk, pair) : 64 * blk + 32 * pair;
  const int mykv = kv0 + il;
  // pair-uniform computed range; the block stages pair 0's diagonal (its
  // rows are the lower ones in both maps) to pair 1's last tile
  const int p_lo = kv0 >> 5, p_hi = h96_last_qtile(kv0, W, Sq);
  const int qt_lo = (dense ? ob_fold_kv_row0(Sq, blk, 0) : 64 * blk) >> 5;
  const int qt_hi = h96_last_qtile(
      dense ? ob_fold_kv_row0(Sq, blk, 1) : 64 * blk + 32, W, Sq);

  const __bf16* KV = Qp + (role ? 2 * H : H);
  bf16x8 of[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s)
    of[s] = *reinterpret_cast<const bf16x8*>(KV + mykv * ld + s * 16 + kh * 8);

  h96_zero_pad<HD>(qbuf[0], 64, tid);
  h96_zero_pad<HD>(obuf[0], 64, tid);
  h96_stage2<HD, 32>(qbuf[qt_lo & 1], Qp + qt_lo * 32 * ld, ld,
                     obuf[qt_lo & 1], dOp + (int64_t)qt_lo * 32 * H, H, tid);
  __syncthreads();

  f32x16 acc[3] = {};  // role 0: dV d groups; role 1: dK d groups
  for (int qt = qt_lo; qt <= qt_hi; ++qt) {
    const int q0 = qt * 32;
    // bit r: keep of element r (q row q0 + acc_row(r, kh), column mykv)
    [[maybe_unused]] uint32_t keep = 0;
    if constexpr (kDrop) {
      if (role == 0 && qt >= p_lo && qt <= p_hi) {  // wave-uniform
        // Philox counter of q row q0 + 4*kh at this lane's kv quad
        const uint32_t sq4 = (uint32_t)(Sq >> 2);
        const uint32_t c0 = (uint32_t)(z * Sq + q0 + 4 * kh) * sq4 +
                            (uint32_t)(mykv >> 2);
        uint32_t mine = 0;  // rows r = 4g + (il & 3): bit 4g + word
#pragma unroll 1
        for (int g = 0; g < 4; ++g) {
          const ob_philox4 w4 =
              ob_drop_words(key, c0 + (uint32_t)((il & 3) + 8 * g) * sq4);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            mine |= (uint32_t)(w4.w[j] >= key.thr) << (4 * g + j);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          // quad lane j drew rows 4g + j; take this lane's word of each
          const uint32_t theirs =
              (uint32_t)__shfl((int)mine, (lane & ~3) | j, 64) >> (il & 3);
#pragma unroll
          for (int g = 0; g < 4; ++g)
            keep |= ((theirs >> (4 * g)) & 1u) << (4 * g + j);
        }
      }
    }
    if (qt < qt_hi)
      h96_stage2<HD, 32>(qbuf[(qt + 1) & 1], Qp + (q0 + 32) * ld, ld,
                         obuf[(qt + 1) & 1], dOp + (int64_t)(q0 + 32) * H, H,
                         tid);
    // wave-uniform; each wave meets exactly one barrier per iteration on
    // either side of the branch
    if (qt < p_lo || qt > p_hi) {
      __syncthreads();
      continue;
    }
    // own tile's A image, and the B image: role 0 multiplies P^T by dO,
    // role 1 dS^T by Q
    const __bf16* ab = role ? obuf[qt & 1] : qbuf[qt & 1];
    const __bf16* bb = role ? qbuf[qt & 1] : obuf[qt & 1];
    bf16x8 bf[2][3];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int d = 0; d < 3; ++d)
        bf[t][d] = h96_tr_frag(bb, lane, 16 * t + kh * 8, d);
    // own tile: S (role 0, A = Q rows) or dP (role 1, A = dO rows)
    f32x16 own = {};
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const bf16x8 af =
          *reinterpret_cast<const bf16x8*>(&ab[h96_off(il, s * 2 + kh)]);
      own = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, of[s], own, 0, 0, 0);
    }
    float pv[16];
    float* ptile = xch[qt & 1][pair];
    if (role == 0) {
      const float lse_t = lsep[q0 + il];
      // interior: the tile's first q at or past the pair's last kv, its
      // last q inside the band of the pair's first kv
      const bool inner = q0 >= kv0 + 31 && q0 + 31 - kv0 < W;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qoff = acc_row(r, kh);
        const bool ok =
            inner || (unsigned)(q0 + qoff - mykv) < (unsigned)W;
        const float lse_q = __shfl(lse_t, qoff, 64);
        pv[r] = ok ? __expf(own[r] * scale - lse_q) : 0.f;
        if constexpr (kDrop) {
          // the keep bit rides to role 1 as the sign of P (P >= 0)
          const bool kept = (keep >> r) & 1u;
          ptile[qoff * 32 + il] = kept ? pv[r] : -pv[r];
          pv[r] = kept ? pv[r] * key.scale : 0.f;
        } else {
          ptile[qoff * 32 + il] = pv[r];
        }
      }
    }
    __syncthreads();
    if (role == 1) {
      const float d_t = Dp[q0 + il];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qoff = acc_row(r, kh);
        const float d_q = __shfl(d_t, qoff, 64);
        // dS = P * (dP - D); masked entries have P == 0 already
        if constexpr (kDrop) {
          // dS = P * (f * dP - D): |x| is P, a set sign bit says dropped
          const float x = ptile[qoff * 32 + il];
          const float f = __builtin_signbit(x) ? 0.f : key.scale;
          pv[r] = __builtin_fabsf(x) * (f * own[r] - d_q);
        } else {
          pv[r] = ptile[qoff * 32 + il] * (own[r] - d_q);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const bf16x8 a = bf_dance(pv + t * 8);
#pragma unroll
      for (int d = 0; d < 3; ++d)
        acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bf[t][d], acc[d],
                                                         0, 0, 0);
    }
  }

  __bf16* outp = dqkv + base + (role ? H : 2 * H);  // dK or dV slice
  const float os = role ? scale : 1.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int kv = kv0 + acc_row(r, kh);
#pragma unroll
    for (int d = 0; d < 3; ++d)
      if (32 * d + il < HD)
        outp[kv * ld + 32 * d + il] = (__bf16)(os * acc[d][r]);
  }
  if (dbias) {  // kernel-uniform
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      float c = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) c += os * acc[d][r];
      c += __shfl_xor(c, 32, 64);
      if (kh == 0 && 32 * d + il < HD) red[w * HD + 32 * d + il] = c;
    }
    __syncthreads();
    if (tid < 2 * HD) {
      // waves 0/2 hold dV (role 0), waves 1/3 dK (role 1)
      const int rl = tid / HD, c = tid % HD;
      atomicAdd(dbias + (rl ? H : 2 * H) + h * HD + c,
                red[rl * HD + c] + red[(2 + rl) * HD + c]);
    }
  }
}
template <int HD>
__global__ OB_HD96_KERNEL __launch_bounds__(256, 2) void k_flash_bwd_dkdv_hd96(
    const __bf16* __restrict__ qkv, const __bf16* __restrict__ dO,
    const float* __restrict__ lse, const float* __restrict__ D,
    __bf16* __restrict__ dqkv, float* __restrict__ dbias, int Sq, int H,
    int nh, int Z, int W, float scale) {
  h96_dkdv_body<HD, false>(qkv, dO, lse, D, dqkv, dbias, Sq, H, nh, Z, W,
                           scale, ob_drop_key{});
}
template <int HD>
__global__ OB_HD96_KERNEL __launch_bounds__(256, 2) void
k_flash_bwd_dkdv_hd96_drop(const __bf16* __restrict__ qkv,
                           const __bf16* __restrict__ dO,
                           const float* __restrict__ lse,
                           const float* __restrict__ D,
                           __bf16* __restrict__ dqkv,
                           float* __restrict__ dbias, int Sq, int H, int nh,
                           int Z, int W, float scale, ob_drop_key key) {
  h96_dkdv_body<HD, true>(qkv, dO, lse, D, dqkv, dbias, Sq, H, nh, Z, W,
                          scale, key);
}

// ---- entries ----------------------------------------------------------------
// 80 or 96; 0 with ob_fail set
static int h96_head_dim(const char* who, int64_t B, int64_t Sq, int64_t H,
                        int64_t nh, int64_t window) {
  if (nh <= 0 || H % nh || (H / nh != 80 && H / nh != 96)) {
    ob_fail("%s: n_embd must be a multiple of n_head and head_dim 80 or 96",
            who);
    return 0;
  }
  if (B <= 0 || Sq <= 0 || Sq % 128) {
    ob_fail("%s: S must be a multiple of 128", who);
    return 0;
  }
  if (window < 0) {
    ob_fail("%s: window must be >= 0", who);
    return 0;
  }
  return (int)(H / nh);
}
// 0 and >= S are the same dense launch
static int h96_window(int64_t window, int64_t Sq) {
  return (int)(window == 0 || window >= Sq ? Sq : window);
}

template <int HD>
static int h96_fwd(const void* qkv, void* O, void* lse, int64_t B, int64_t Sq,
                   int64_t H, int64_t nh, int W, float scale, void* stream) {
  const int Z = (int)(B * nh);
  k_flash_fwd_hd96<HD>
      <<<ob_fold_grid((int)Sq / 128, Z), 256, 0, S(stream)>>>(
          (const __bf16*)qkv, (__bf16*)O, (float*)lse, (int)Sq, (int)H,
          (int)nh, Z, W, scale);
  OB_LAUNCH_CHECK();
  return 0;
}

extern "C" int ob_flash_fwd_hd96_bf16(const void* qkv, void* O, void* lse,
                                      int64_t B, int64_t Sq, int64_t H,
                                      int64_t nh, int64_t window, float scale,
                                      void* stream) {
  const int hd = h96_head_dim("flash_fwd_hd96", B, Sq, H, nh, window);
  if (!hd) return 1;
  const int W = h96_window(window, Sq);
  return hd == 80 ? h96_fwd<80>(qkv, O, lse, B, Sq, H, nh, W, scale, stream)
                  : h96_fwd<96>(qkv, O, lse, B, Sq, H, nh, W, scale, stream);
}

// dq first (forms D from O and dO into D_ws), then dkdv, which reads it
template <int HD>
static int h96_bwd(const void* qkv, const void* O, const void* dO,
                   const void* lse, void* D_ws, void* dqkv, void* dbias_qkv,
                   int64_t B, int64_t Sq, int64_t H, int64_t nh, int W,
                   float scale, void* stream) {
  const int Z = (int)(B * nh);
  k_flash_bwd_dq_hd96<HD>
      <<<ob_fold_grid((int)Sq / 128, Z), 256, 0, S(stream)>>>(
          (const __bf16*)qkv, (const __bf16*)dO, (const float*)lse,
          (const __bf16*)O, (float*)D_ws, (__bf16*)dqkv, (float*)dbias_qkv,
          (int)Sq, (int)H, (int)nh, Z, W, scale);
  OB_LAUNCH_CHECK();
  k_flash_bwd_dkdv_hd96<HD>
      <<<ob_fold_grid((int)Sq / 64, Z), 256, 0, S(stream)>>>(
          (const __bf16*)qkv, (const __bf16*)dO, (const float*)lse,
          (const float*)D_ws, (__bf16*)dqkv, (float*)dbias_qkv, (int)Sq,
          (int)H, (int)nh, Z, W, scale);
  OB_LAUNCH_CHECK();
  return 0;
}

extern "C" int ob_flash_bwd_hd96_d_bf16(const void* qkv, const void* O,
                                        const void* dO, const void* lse,
                                        void* D_ws, void* dqkv,
                                        void* dbias_qkv, int64_t B, int64_t Sq,
                                        int64_t H, int64_t nh, int64_t window,
                                        float scale, void* stream) {
  const int hd = h96_head_dim("flash_bwd_hd96_d", B, Sq, H, nh, window);
  if (!hd) return 1;
  const int W = h96_window(window, Sq);
  return hd == 80 ? h96_bwd<80>(qkv, O, dO, lse, D_ws, dqkv, dbias_qkv, B, Sq,
                                H, nh, W, scale, stream)
                  : h96_bwd<96>(qkv, O, dO, lse, D_ws, dqkv, dbias_qkv, B, Sq,
                                H, nh, W, scale, stream);
}

// ---- entries with attention dropout ------------------
// the plain entry's checks, then p and the mask's element count; 80 or 96, 0
// with ob_fail set
static int h96_drop_head_dim(const char* who, int64_t B, int64_t Sq, int64_t H,
                             int64_t nh, int64_t window, float p) {
  const int hd = h96_head_dim(who, B, Sq, H, nh, window);
  if (!hd) return 0;
  if (!ob_drop_p_ok(p)) {
    ob_fail("%s: p must be in [0,1)", who);
    return 0;
  }
  if (B * nh * Sq * Sq > ((int64_t)1 << 34)) {
    ob_fail("%s: B*nh*S*S exceeds the 2^34 mask elements", who);
    return 0;
  }
  return hd;
}

template <int HD>
static int h96_fwd_drop(const void* qkv, void* O, void* lse, int64_t B,
                        int64_t Sq, int64_t H, int64_t nh, int W, float scale,
                        const ob_drop_key& key, void* stream) {
  const int Z = (int)(B * nh);
  k_flash_fwd_hd96_drop<HD>
      <<<ob_fold_grid((int)Sq / 128, Z), 256, 0, S(stream)>>>(
          (const __bf16*)qkv, (__bf16*)O, (float*)lse, (int)Sq, (int)H,
          (int)nh, Z, W, scale, key);
  OB_LAUNCH_CHECK();
  return 0;
}

// ob_flash_fwd_hd96_bf16 with attention dropout (site OB_DROP_ATTN) applied
// to P before PV; p == 0 is the plain entry.
extern "C" int ob_flash_fwd_hd96_drop_bf16(const void* qkv, void* O, void* lse,
                                           int64_t B, int64_t Sq, int64_t H,
                                           int64_t nh, int64_t window,
                                           float scale, uint64_t seed,
                                           int32_t layer_id, uint64_t tick,
                                           float p, void* stream) {
  const int hd =
      h96_drop_head_dim("flash_fwd_hd96_drop", B, Sq, H, nh, window, p);
  if (!hd) return 1;
  if (p == 0.f)
    return ob_flash_fwd_hd96_bf16(qkv, O, lse, B, Sq, H, nh, window, scale,
                                  stream);
  const ob_drop_key key =
      ob_drop_make_key(seed, layer_id, OB_DROP_ATTN, tick, p);
  const int W = h96_window(window, Sq);
  return hd == 80
             ? h96_fwd_drop<80>(qkv, O, lse, B, Sq, H, nh, W, scale, key,
                                stream)
             : h96_fwd_drop<96>(qkv, O, lse, B, Sq, H, nh, W, scale, key,
                                stream);
}

// dq first (forms D from O and dO into D_ws), then dkdv, which reads it
template <int HD>
static int h96_bwd_drop(const void* qkv, const void* O, const void* dO,
                        const void* lse, void* D_ws, void* dqkv,
                        void* dbias_qkv, int64_t B, int64_t Sq, int64_t H,
                        int64_t nh, int W, float scale, const ob_drop_key& key,
                        void* stream) {
  const int Z = (int)(B * nh);
  k_flash_bwd_dq_hd96_drop<HD>
      <<<ob_fold_grid((int)Sq / 128, Z), 256, 0, S(stream)>>>(
          (const __bf16*)qkv, (const __bf16*)dO, (const float*)lse,
          (const __bf16*)O, (float*)D_ws, (__bf16*)dqkv, (float*)dbias_qkv,
          (int)Sq, (int)H, (int)nh, Z, W, scale, key);
  OB_LAUNCH_CHECK();
  k_flash_bwd_dkdv_hd96_drop<HD>
      <<<ob_fold_grid((int)Sq / 64, Z), 256, 0, S(stream)>>>(
          (const __bf16*)qkv, (const __bf16*)dO, (const float*)lse,
          (const float*)D_ws, (__bf16*)dqkv, (float*)dbias_qkv, (int)Sq,
          (int)H, (int)nh, Z, W, scale, key);
  OB_LAUNCH_CHECK();
  return 0;
}

// ob_flash_bwd_hd96_d_bf16 for a forward that ran ob_flash_fwd_hd96_drop_bf16
// with the same key; p == 0 is the plain entry.
extern "C" int ob_flash_bwd_hd96_d_drop_bf16(
    const void* qkv, const void* O, const void* dO, const void* lse,
    void* D_ws, void* dqkv, void* dbias_qkv, int64_t B, int64_t Sq, int64_t H,
    int64_t nh, int64_t window, float scale, uint64_t seed, int32_t layer_id,
    uint64_t tick, float p, void* stream) {
  const int hd =
      h96_drop_head_dim("flash_bwd_hd96_d_drop", B, Sq, H, nh, window, p);
  if (!hd) return 1;
  if (p == 0.f)
    return ob_flash_bwd_hd96_d_bf16(qkv, O, dO, lse, D_ws, dqkv, dbias_qkv, B,
                                    Sq, H, nh, window, scale, stream);
  const ob_drop_key key =
      ob_drop_make_key(seed, layer_id, OB_DROP_ATTN, tick, p);
  const int W = h96_window(window, Sq);
  return hd == 80
             ? h96_bwd_drop<80>(qkv, O, dO, lse, D_ws, dqkv, dbias_qkv, B, Sq,
                                H, nh, W, scale, key, stream)
             : h96_bwd_drop<96>(qkv, O, dO, lse, D_ws, dqkv, dbias_qkv, B, Sq,
                                H, nh, W, scale, key, stream);
}
