// ob_flash_win_bf16.hip — locally banded (sliding-window) causal flash
// attention, bf16, head_dim 64 and 128.  Query row i
// attends the keys j with i - W < j <= i: the attention pattern of GPT-3's
// and GPT-Neo's "local" layers.  Three kernels per head size, as in the dense
// production set: forward (O and the row LSE of the scaled scores), dQ
// (forming D = rowsum(dO * O) the way ob_flash_bwd_nt_d_bf16 does) and dK/dV;
// the backward recomputes P from Q, K and LSE.  One body per kernel, a
// template on the head size: the two sizes differ in the k-steps of a chain
// (HD/16), the output accumulators (HD/32) and the LDS image (win_lds).
//
// The arithmetic is the dense kernels' (ob_flash_bf16.hip,
// ob_flash_hd128_bf16.hip): swapped QK^T so a lane owns one q column,
// bf_dance into the PV / dS A fragment, transposed B operands read
// column-wise from the row-major LDS tile, double-buffered tiles under one
// barrier per tile, `scale` folded in the same places.  What is this file's
// own is which rows a block owns and which tiles it visits.
//
// Block map.  A band has no light and heavy pieces to pair (every row past W
// costs the same) and a folded block's two halves would need two disjoint
// K/V ranges, so the fold of ob_flash_fold.h is not used: blocks own
// CONSECUTIVE rows, which share one contiguous tile range.
//   forward / dQ: block a owns q rows 128a .. 128a+127, wave w the 32 rows
//     from q0 = 128a + 32w.  It stages the 64-row kv tiles
//     win_first_tile(128a) .. 2a+1 (the diagonal tile of its last row); wave
//     w computes tiles win_first_tile(q0) .. (q0+31)/64 of them.
//   dK/dV: block x owns kv rows 64x .. 64x+63, wave pair p the 32 rows from
//     kv0 = 64x + 32p.  It stages the 32-row q tiles 2x .. win_last_qtile(64x
//     + 32), clamped to the sequence; pair p computes kv0/32 ..
//     win_last_qtile(kv0).
// Only the linear-id -> (head, block) map is shared with the dense kernels
// (ob_fold_id / ob_fold_grid): the blocks of one head get ids of one XCD and
// share its L2.
//
// Tile classes, per wave: a tile wholly inside the band of all 32 rows takes
// no mask; any other takes `(unsigned)(q - kv) < W`, which is the causal
// test (q - kv >= 0) and the band test (q - kv < W) in one compare, so a
// small W that makes one tile both diagonal and lower edge needs no case of
// its own.
//
// Fully masked rows.  Tiles go in ascending kv order and a wave starts at the
// first tile its FIRST row reaches, so its later rows can be fully masked in
// the first tiles the wave computes (W = 40, rows 96..127: row 127's band
// starts at kv 88, tile 1, but the wave starts at tile 0 for row 96).  Their
// running max m is then still -inf.  The forward's rules:
//   * the rescale test is `mt > m + 8`, not `mt - m <= 8`: no inf - inf, and
//     a row that stays at -inf asks for no rescale;
//   * a rescale's factor is 1 for a row whose max did not move (which covers
//     m = mnew = -inf), else exp(m - mnew), which is 0 from m = -inf;
//   * P of a masked score is 0 without an exp.
// A finite score therefore always meets a finite m (a row at -inf with a
// finite tile max always triggers the rescale), and every row ends with its
// diagonal element, so l > 0 and the LSE is finite.  The backward has no such
// state: it reads the finite LSE and a masked P is 0.
//
// The kernels are compiled without packed fp32 VALU ops, like the dropout
// kernels of ob_flash_hd128_bf16.hip; the bodies are forceinline device
// templates under attributed __global__ wrappers for the reason given there.
// Resources: profiles/flash_win_resources.txt (no scratch).
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
//
// Out of scope: the materialized-P and fp32 routes.
// head_dim 80/96, dense and banded: ob_flash_hd96_bf16.hip.
#include "ob_flash_common.h"
#include "ob_internal.h"
#include "ob_flash_fold.h"

#include <cmath>

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

#define OB_WIN_KERNEL __attribute__((target("no-packed-fp32-ops")))

// ---- the band's tile ranges (host and device) ------------------------------
// first 64-row kv tile a q row reaches: floor((row - W + 1) / 64), clamped
OB_FOLD_HD int win_first_tile(int row, int W) {
  const int lo = row - W + 1;
  return lo > 0 ? lo / 64 : 0;
}
// last 32-row q tile that reaches a 32-row kv tile starting at kv0: its last
// row kv0 + 31 is seen by the q rows up to kv0 + 31 + W - 1
OB_FOLD_HD int win_last_qtile(int kv0, int W, int Sq) {
  const int64_t hi = (int64_t)kv0 + 31 + W - 1;
  return hi >= Sq ? Sq / 32 - 1 : (int)(hi / 32);
}

// ---- LDS image per head size ------------------------------------------------
template <int HD> struct win_lds;
template <> struct win_lds<64> {
  static __device__ __forceinline__ int off(int row, int ch) {
    return nt_off(row, ch);
  }
  static __device__ __forceinline__ bf16x8 frag(const __bf16* t, int lane,
                                                int r0, int d) {
    return nt_tr_frag(t, lane, r0, d);
  }
};
template <> struct win_lds<128> {
  static __device__ __forceinline__ int off(int row, int ch) {
    return hd_off(row, ch);
  }
  static __device__ __forceinline__ bf16x8 frag(const __bf16* t, int lane,
                                                int r0, int d) {
    return hd_tr_frag(t, lane, r0, d);
  }
};

// Stages two [ROWS][HD] tiles (rows lda / ldb elements apart in memory) into
// their LDS images: 256 threads, 16-byte chunks, thread = chunk tid % (HD/8)
// of rows tid / (HD/8) + RP*i.  Both images' keys have period 16 in the row
// and RP is 32 or 16, so a thread's LDS offsets differ by constants.  All the
// loads are issued before the first store.
template <int HD, int ROWS>
__device__ __forceinline__ void win_stage2(__bf16* da, const __bf16* a,
                                           int64_t lda, __bf16* db,
                                           const __bf16* b, int64_t ldb,
                                           int tid) {
  constexpr int CH = HD / 8, RP = 256 / CH, N = ROWS / RP;
  const int sr = tid / CH, sc = tid % CH;
  const int so = win_lds<HD>::off(sr, sc);
  bf16x8 ra[N], rb[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    ra[i] = *reinterpret_cast<const bf16x8*>(a + (sr + RP * i) * lda + sc * 8);
    rb[i] = *reinterpret_cast<const bf16x8*>(b + (sr + RP * i) * ldb + sc * 8);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    *reinterpret_cast<bf16x8*>(da + so + RP * HD * i) = ra[i];
    *reinterpret_cast<bf16x8*>(db + so + RP * HD * i) = rb[i];
  }
}

// ===========================================================================
// Forward.  LDS: 2 x (K + V tile) + bcast = 32.5 KB (hd 64), 64.5 KB (hd 128).
// ===========================================================================
template <int HD, bool kDrop>
__device__ __forceinline__ void win_fwd_body(
    const __bf16* __restrict__ qkv, __bf16* __restrict__ Obase,
    float* __restrict__ lse, int Sq, int H, int nh, int Z, int W,
    float scale, const ob_drop_key& key) {
  constexpr int NS = HD / 16, ND = HD / 32;
  using L = win_lds<HD>;
  __shared__ __attribute__((aligned(16))) __bf16 kbuf[2][64 * HD];
  __shared__ __attribute__((aligned(16))) __bf16 vbuf[2][64 * HD];
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
  const int q0 = 128 * blk + 32 * w;
  const int myq = q0 + il;
  // block-uniform staged range, wave-uniform computed range
  const int t_lo = win_first_tile(128 * blk, W), t_hi = 2 * blk + 1;
  const int w_lo = win_first_tile(q0, W), w_hi = (q0 + 31) >> 6;

  bf16x8 qf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s)
    qf[s] = *reinterpret_cast<const bf16x8*>(Qp + myq * ld + s * 16 + kh * 8);

  win_stage2<HD, 64>(kbuf[0], Kp + t_lo * 64 * ld, ld, vbuf[0],
                     Vp + t_lo * 64 * ld, ld, tid);
  __syncthreads();

  f32x16 o[ND] = {};
  float m = -INFINITY, l = 0.f;
  for (int kvt = t_lo; kvt <= t_hi; ++kvt) {
    const int kv0 = kvt * 64;
    const int buf = (kvt - t_lo) & 1;
    [[maybe_unused]] uint32_t keep = 0;  // bit 16u + r, as drop_bits_q
    if constexpr (kDrop)
      if (kvt >= w_lo && kvt <= w_hi)  // wave-uniform
        keep = drop_bits_q(key, drop_crow(z, Sq, myq, kh) + (kv0 >> 2));
    if (kvt < t_hi)
      win_stage2<HD, 64>(kbuf[buf ^ 1], Kp + (kv0 + 64) * ld, ld,
                         vbuf[buf ^ 1], Vp + (kv0 + 64) * ld, ld, tid);
    if (kvt >= w_lo && kvt <= w_hi) {  // wave-uniform
      const __bf16* kb = kbuf[buf];
      const __bf16* vb = vbuf[buf];
      f32x16 sacc0 = {}, sacc1 = {};
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int ch = s * 2 + kh;
        const bf16x8 ka =
            *reinterpret_cast<const bf16x8*>(&kb[L::off(il, ch)]);
        const bf16x8 kb2 =
            *reinterpret_cast<const bf16x8*>(&kb[L::off(32 + il, ch)]);
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
      // m may be -inf here (a row fully masked so far): see the header
      if (__any(mt > m + 8.f)) {
        const float mnew = fmaxf(m, mt);
        const float af = (mnew == m) ? 1.f : __expf(m - mnew);
        m = mnew;
        if (kh == 0) bcast[w * 32 + il] = af;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float a = bcast[w * 32 + acc_row(r, kh)];
#pragma unroll
          for (int d = 0; d < ND; ++d) o[d][r] *= a;
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
        for (int d = 0; d < ND; ++d) {
          const bf16x8 vf = L::frag(vb, lane, t * 16 + kh * 8, d);
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
    for (int d = 0; d < ND; ++d)
      Op[(int64_t)(q0 + row) * H + 32 * d + il] = (__bf16)(o[d][r] * inv);
  }
}
template <int HD>
__global__ OB_WIN_KERNEL __launch_bounds__(256, HD == 64 ? 3 : 2) void
k_flash_fwd_win(const __bf16* __restrict__ qkv, __bf16* __restrict__ Obase,
                float* __restrict__ lse, int Sq, int H, int nh, int Z, int W,
                float scale) {
  win_fwd_body<HD, false>(qkv, Obase, lse, Sq, H, nh, Z, W, scale,
                          ob_drop_key{});
}
template <int HD>
__global__ OB_WIN_KERNEL __launch_bounds__(256, HD == 64 ? 3 : 2) void
k_flash_fwd_win_drop(const __bf16* __restrict__ qkv,
                     __bf16* __restrict__ Obase, float* __restrict__ lse,
                     int Sq, int H, int nh, int Z, int W, float scale,
                     ob_drop_key key) {
  win_fwd_body<HD, true>(qkv, Obase, lse, Sq, H, nh, Z, W, scale, key);
}

// ===========================================================================
// dQ: the forward's blocks, ranges and K/V staging.  The two 32-row kv
// sub-tiles of a tile run one after the other (one S, one dP and 16 dS values
// live at a time, as at head_dim 128 in the dense kernel); a sub-tile wholly
// outside the wave's band is skipped, wave-uniformly.  D is formed from the
// resident dO fragments and O loaded in the same layout, used, and written
// to Dout for the dK/dV launch that follows.
// LDS: 2 x (K + V tile) + red = 33 KB (hd 64), 66 KB (hd 128).
// ===========================================================================
template <int HD, bool kDrop>
__device__ __forceinline__ void win_dq_body(
    const __bf16* __restrict__ qkv, const __bf16* __restrict__ dO,
    const float* __restrict__ lse, const __bf16* __restrict__ O,
    float* __restrict__ Dout, __bf16* __restrict__ dqkv,
    float* __restrict__ dbias, int Sq, int H, int nh, int Z, int W,
    float scale, const ob_drop_key& key) {
  constexpr int NS = HD / 16, ND = HD / 32;
  using L = win_lds<HD>;
  __shared__ __attribute__((aligned(16))) __bf16 kbuf[2][64 * HD];
  __shared__ __attribute__((aligned(16))) __bf16 vbuf[2][64 * HD];
  __shared__ float red[4 * HD];
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
  const int q0 = 128 * blk + 32 * w;
  const int myq = q0 + il;
  const int t_lo = win_first_tile(128 * blk, W), t_hi = 2 * blk + 1;
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

  win_stage2<HD, 64>(kbuf[0], Kp + t_lo * 64 * ld, ld, vbuf[0],
                     Vp + t_lo * 64 * ld, ld, tid);
  __syncthreads();

  f32x16 dq[ND] = {};
  for (int kvt = t_lo; kvt <= t_hi; ++kvt) {
    const int kv0 = kvt * 64;
    const int buf = (kvt - t_lo) & 1;
    if (kvt < t_hi)
      win_stage2<HD, 64>(kbuf[buf ^ 1], Kp + (kv0 + 64) * ld, ld,
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
              &kb[L::off(32 * u + il, ch)]);
          const bf16x8 va = *reinterpret_cast<const bf16x8*>(
              &vb[L::off(32 * u + il, ch)]);
          sa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qf[s], sa, 0, 0,
                                                       0);
          pa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, df[s], pa, 0, 0,
                                                       0);
        }
        float dsv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const bool ok =
              (unsigned)(myq - (kvu + acc_row(r, kh))) < (unsigned)W;
          // dS = P * (f * dP - D); a masked P is 0 without an exp
          if constexpr (kDrop)
            dsv[r] = ok ? __expf(sa[r] * scale - mylse) *
                              (drop_factor_bit(key, keep, r) * pa[r] - myD)
                        : 0.f;
          else
            dsv[r] = ok ? __expf(sa[r] * scale - mylse) * (pa[r] - myD) : 0.f;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const bf16x8 da = bf_dance(dsv + t * 8);
          // B[k = kv 32u+16t+8kh..+7][n = d]: columns of the K tile
#pragma unroll
          for (int d = 0; d < ND; ++d) {
            const bf16x8 kt = L::frag(kb, lane, 32 * u + 16 * t + kh * 8, d);
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
    for (int d = 0; d < ND; ++d)
      dQp[q * ld + 32 * d + il] = (__bf16)(scale * dq[d][r]);
  }
  if (dbias) {  // kernel-uniform
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      float c = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) c += scale * dq[d][r];
      c += __shfl_xor(c, 32, 64);
      if (kh == 0) red[w * HD + 32 * d + il] = c;
    }
    __syncthreads();
    if (tid < HD)
      atomicAdd(dbias + h * HD + tid,
                (red[tid] + red[HD + tid]) +
                    (red[2 * HD + tid] + red[3 * HD + tid]));
  }
}
template <int HD>
__global__ OB_WIN_KERNEL __launch_bounds__(256, HD == 64 ? 3 : 2) void
k_flash_bwd_dq_win(const __bf16* __restrict__ qkv,
                   const __bf16* __restrict__ dO,
                   const float* __restrict__ lse, const __bf16* __restrict__ O,
                   float* __restrict__ Dout, __bf16* __restrict__ dqkv,
                   float* __restrict__ dbias, int Sq, int H, int nh, int Z,
                   int W, float scale) {
  win_dq_body<HD, false>(qkv, dO, lse, O, Dout, dqkv, dbias, Sq, H, nh, Z, W,
                         scale, ob_drop_key{});
}
template <int HD>
__global__ OB_WIN_KERNEL __launch_bounds__(256, HD == 64 ? 3 : 2) void
k_flash_bwd_dq_win_drop(const __bf16* __restrict__ qkv,
                        const __bf16* __restrict__ dO,
                        const float* __restrict__ lse,
                        const __bf16* __restrict__ O, float* __restrict__ Dout,
                        __bf16* __restrict__ dqkv, float* __restrict__ dbias,
                        int Sq, int H, int nh, int Z, int W, float scale,
                        ob_drop_key key) {
  win_dq_body<HD, true>(qkv, dO, lse, O, Dout, dqkv, dbias, Sq, H, nh, Z, W,
                        scale, key);
}

// ===========================================================================
// dK/dV: the dense kernels' split-duty wave pairs (role 0: K resident,
// S -> P -> dV; role 1: V resident, dP -> dS -> dK; only P crosses the pair,
// through xch) over 32-row q tiles.  A pair idles, staging and meeting the
// barrier only, before its diagonal tile and after the last tile its rows'
// bands reach.  The B fragments are read before the iteration's barrier:
// after it a fast wave already stages tile qt+2 into this buffer.
// LDS: xch 16 KB + 2 x (Q + dO tile) + red = 33 KB (hd 64), 50 KB (hd 128).
// ===========================================================================
template <int HD, bool kDrop>
__device__ __forceinline__ void win_dkdv_body(
    const __bf16* __restrict__ qkv, const __bf16* __restrict__ dO,
    const float* __restrict__ lse, const float* __restrict__ D,
    __bf16* __restrict__ dqkv, float* __restrict__ dbias, int Sq, int H,
    int nh, int Z, int W, float scale, const ob_drop_key& key) {
  constexpr int NS = HD / 16, ND = HD / 32;
  using L = win_lds<HD>;
  __shared__ float xch[2][2][32 * 32];  // [buffer][pair][P tile]
  __shared__ __attribute__((aligned(16))) __bf16 qbuf[2][32 * HD];
  __shared__ __attribute__((aligned(16))) __bf16 obuf[2][32 * HD];
  __shared__ float red[4 * HD];
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
  const int kv0 = 64 * blk + 32 * pair;
  const int mykv = kv0 + il;
  // block-uniform staged range, pair-uniform computed range
  const int qt_lo = 2 * blk, qt_hi = win_last_qtile(64 * blk + 32, W, Sq);
  const int p_lo = kv0 >> 5, p_hi = win_last_qtile(kv0, W, Sq);

  const __bf16* KV = Qp + (role ? 2 * H : H);
  bf16x8 of[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s)
    of[s] = *reinterpret_cast<const bf16x8*>(KV + mykv * ld + s * 16 + kh * 8);

  win_stage2<HD, 32>(qbuf[qt_lo & 1], Qp + qt_lo * 32 * ld, ld,
                     obuf[qt_lo & 1], dOp + (int64_t)qt_lo * 32 * H, H, tid);
  __syncthreads();

  f32x16 acc[ND] = {};  // role 0: dV d groups; role 1: dK d groups
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
      win_stage2<HD, 32>(qbuf[(qt + 1) & 1], Qp + (q0 + 32) * ld, ld,
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
    bf16x8 bf[2][ND];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int d = 0; d < ND; ++d)
        bf[t][d] = L::frag(bb, lane, 16 * t + kh * 8, d);
    // own tile: S (role 0, A = Q rows) or dP (role 1, A = dO rows)
    f32x16 own = {};
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const bf16x8 af =
          *reinterpret_cast<const bf16x8*>(&ab[L::off(il, s * 2 + kh)]);
      own = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, of[s], own, 0, 0, 0);
    }
    float pv[16];
    float* ptile = xch[qt & 1][pair];
    if (role == 0) {
      const float lse_t = lsep[q0 + il];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qoff = acc_row(r, kh);
        const bool ok = (unsigned)(q0 + qoff - mykv) < (unsigned)W;
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
      for (int d = 0; d < ND; ++d)
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
    for (int d = 0; d < ND; ++d)
      outp[kv * ld + 32 * d + il] = (__bf16)(os * acc[d][r]);
  }
  if (dbias) {  // kernel-uniform
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      float c = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) c += os * acc[d][r];
      c += __shfl_xor(c, 32, 64);
      if (kh == 0) red[w * HD + 32 * d + il] = c;
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
__global__ OB_WIN_KERNEL __launch_bounds__(256, HD == 64 ? 3 : 2) void
k_flash_bwd_dkdv_win(const __bf16* __restrict__ qkv,
                     const __bf16* __restrict__ dO,
                     const float* __restrict__ lse,
                     const float* __restrict__ D, __bf16* __restrict__ dqkv,
                     float* __restrict__ dbias, int Sq, int H, int nh, int Z,
                     int W, float scale) {
  win_dkdv_body<HD, false>(qkv, dO, lse, D, dqkv, dbias, Sq, H, nh, Z, W,
                           scale, ob_drop_key{});
}
template <int HD>
__global__ OB_WIN_KERNEL __launch_bounds__(256, HD == 64 ? 3 : 2) void
k_flash_bwd_dkdv_win_drop(const __bf16* __restrict__ qkv,
                          const __bf16* __restrict__ dO,
                          const float* __restrict__ lse,
                          const float* __restrict__ D,
                          __bf16* __restrict__ dqkv, float* __restrict__ dbias,
                          int Sq, int H, int nh, int Z, int W, float scale,
                          ob_drop_key key) {
  win_dkdv_body<HD, true>(qkv, dO, lse, D, dqkv, dbias, Sq, H, nh, Z, W,
                          scale, key);
}

// ---- entries ----------------------------------------------------------------
// 64 or 128; 0 with ob_fail set.  The rules of the dense nt entries, plus
// window >= 0.
static int win_head_dim(const char* who, int64_t B, int64_t Sq, int64_t H,
                        int64_t nh, int64_t window) {
  if (nh <= 0 || H % nh || (H / nh != 64 && H / nh != 128)) {
    ob_fail("%s: n_embd must be a multiple of n_head and head_dim 64 or 128",
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

template <int HD>
static int win_fwd(const void* qkv, void* O, void* lse, int64_t B, int64_t Sq,
                   int64_t H, int64_t nh, int W, float scale, void* stream) {
  const int Z = (int)(B * nh);
  k_flash_fwd_win<HD><<<ob_fold_grid((int)Sq / 128, Z), 256, 0, S(stream)>>>(
      (const __bf16*)qkv, (__bf16*)O, (float*)lse, (int)Sq, (int)H, (int)nh,
      Z, W, scale);
  OB_LAUNCH_CHECK();
  return 0;
}

extern "C" int ob_flash_fwd_win_bf16(const void* qkv, void* O, void* lse,
                                     int64_t B, int64_t Sq, int64_t H,
                                     int64_t nh, int64_t window, float scale,
                                     void* stream) {
  const int hd = win_head_dim("flash_fwd_win", B, Sq, H, nh, window);
  if (!hd) return 1;
  if (window == 0 || window >= Sq)
    return ob_flash_fwd_nt_bf16(qkv, O, lse, B, Sq, H, nh, scale, stream);
  return hd == 64 ? win_fwd<64>(qkv, O, lse, B, Sq, H, nh, (int)window, scale,
                                stream)
                  : win_fwd<128>(qkv, O, lse, B, Sq, H, nh, (int)window,
                                 scale, stream);
}

// dq first (forms D from O and dO into D_ws), then dkdv, which reads it
template <int HD>
static int win_bwd(const void* qkv, const void* O, const void* dO,
                   const void* lse, void* D_ws, void* dqkv, void* dbias_qkv,
                   int64_t B, int64_t Sq, int64_t H, int64_t nh, int W,
                   float scale, void* stream) {
  const int Z = (int)(B * nh);
  k_flash_bwd_dq_win<HD>
      <<<ob_fold_grid((int)Sq / 128, Z), 256, 0, S(stream)>>>(
          (const __bf16*)qkv, (const __bf16*)dO, (const float*)lse,
          (const __bf16*)O, (float*)D_ws, (__bf16*)dqkv, (float*)dbias_qkv,
          (int)Sq, (int)H, (int)nh, Z, W, scale);
  OB_LAUNCH_CHECK();
  k_flash_bwd_dkdv_win<HD>
      <<<ob_fold_grid((int)Sq / 64, Z), 256, 0, S(stream)>>>(
          (const __bf16*)qkv, (const __bf16*)dO, (const float*)lse,
          (const float*)D_ws, (__bf16*)dqkv, (float*)dbias_qkv, (int)Sq,
          (int)H, (int)nh, Z, W, scale);
  OB_LAUNCH_CHECK();
  return 0;
}

extern "C" int ob_flash_bwd_win_d_bf16(const void* qkv, const void* O,
                                       const void* dO, const void* lse,
                                       void* D_ws, void* dqkv,
                                       void* dbias_qkv, int64_t B, int64_t Sq,
                                       int64_t H, int64_t nh, int64_t window,
                                       float scale, void* stream) {
  const int hd = win_head_dim("flash_bwd_win_d", B, Sq, H, nh, window);
  if (!hd) return 1;
  if (window == 0 || window >= Sq)
    return ob_flash_bwd_nt_d_bf16(qkv, O, dO, lse, D_ws, dqkv, dbias_qkv, B,
                                  Sq, H, nh, scale, stream);
  return hd == 64 ? win_bwd<64>(qkv, O, dO, lse, D_ws, dqkv, dbias_qkv, B, Sq,
                                H, nh, (int)window, scale, stream)
                  : win_bwd<128>(qkv, O, dO, lse, D_ws, dqkv, dbias_qkv, B,
                                 Sq, H, nh, (int)window, scale, stream);
}

// ---- entries with attention dropout ------------------
// the plain entry's checks, then p and the mask's element count; 64 or 128, 0
// with ob_fail set
static int win_drop_head_dim(const char* who, int64_t B, int64_t Sq, int64_t H,
                             int64_t nh, int64_t window, float p) {
  const int hd = win_head_dim(who, B, Sq, H, nh, window);
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
static int win_fwd_drop(const void* qkv, void* O, void* lse, int64_t B,
                        int64_t Sq, int64_t H, int64_t nh, int W, float scale,
                        const ob_drop_key& key, void* stream) {
  const int Z = (int)(B * nh);
  k_flash_fwd_win_drop<HD>
      <<<ob_fold_grid((int)Sq / 128, Z), 256, 0, S(stream)>>>(
          (const __bf16*)qkv, (__bf16*)O, (float*)lse, (int)Sq, (int)H,
          (int)nh, Z, W, scale, key);
  OB_LAUNCH_CHECK();
  return 0;
}

// ob_flash_fwd_win_bf16 with attention dropout (site OB_DROP_ATTN) applied to
// P before PV.  p == 0 is the plain entry; window 0 or >= Sq the dense
// dropout entry of the head size.
extern "C" int ob_flash_fwd_win_drop_bf16(const void* qkv, void* O, void* lse,
                                          int64_t B, int64_t Sq, int64_t H,
                                          int64_t nh, int64_t window,
                                          float scale, uint64_t seed,
                                          int32_t layer_id, uint64_t tick,
                                          float p, void* stream) {
  const int hd =
      win_drop_head_dim("flash_fwd_win_drop", B, Sq, H, nh, window, p);
  if (!hd) return 1;
  if (p == 0.f)
    return ob_flash_fwd_win_bf16(qkv, O, lse, B, Sq, H, nh, window, scale,
                                 stream);
  if (window == 0 || window >= Sq)
    return hd == 64 ? ob_flash_fwd_nt_drop_bf16(qkv, O, lse, B, Sq, H, nh,
                                                scale, seed, layer_id, tick,
                                                p, stream)
                    : ob_flash_fwd_drop_hd128_bf16(qkv, O, lse, B, Sq, H, nh,
                                                   scale, seed, layer_id,
                                                   tick, p, stream);
  const ob_drop_key key =
      ob_drop_make_key(seed, layer_id, OB_DROP_ATTN, tick, p);
  return hd == 64 ? win_fwd_drop<64>(qkv, O, lse, B, Sq, H, nh, (int)window,
                                     scale, key, stream)
                  : win_fwd_drop<128>(qkv, O, lse, B, Sq, H, nh, (int)window,
                                      scale, key, stream);
}

// dq first (forms D from O and dO into D_ws), then dkdv, which reads it
template <int HD>
static int win_bwd_drop(const void* qkv, const void* O, const void* dO,
                        const void* lse, void* D_ws, void* dqkv,
                        void* dbias_qkv, int64_t B, int64_t Sq, int64_t H,
                        int64_t nh, int W, float scale, const ob_drop_key& key,
                        void* stream) {
  const int Z = (int)(B * nh);
  k_flash_bwd_dq_win_drop<HD>
      <<<ob_fold_grid((int)Sq / 128, Z), 256, 0, S(stream)>>>(
          (const __bf16*)qkv, (const __bf16*)dO, (const float*)lse,
          (const __bf16*)O, (float*)D_ws, (__bf16*)dqkv, (float*)dbias_qkv,
          (int)Sq, (int)H, (int)nh, Z, W, scale, key);
  OB_LAUNCH_CHECK();
  k_flash_bwd_dkdv_win_drop<HD>
      <<<ob_fold_grid((int)Sq / 64, Z), 256, 0, S(stream)>>>(
          (const __bf16*)qkv, (const __bf16*)dO, (const float*)lse,
          (const float*)D_ws, (__bf16*)dqkv, (float*)dbias_qkv, (int)Sq,
          (int)H, (int)nh, Z, W, scale, key);
  OB_LAUNCH_CHECK();
  return 0;
}

// ob_flash_bwd_win_d_bf16 for a forward that ran ob_flash_fwd_win_drop_bf16
// with the same key; the same forwarding rules.
extern "C" int ob_flash_bwd_win_d_drop_bf16(
    const void* qkv, const void* O, const void* dO, const void* lse,
    void* D_ws, void* dqkv, void* dbias_qkv, int64_t B, int64_t Sq, int64_t H,
    int64_t nh, int64_t window, float scale, uint64_t seed, int32_t layer_id,
    uint64_t tick, float p, void* stream) {
  const int hd =
      win_drop_head_dim("flash_bwd_win_d_drop", B, Sq, H, nh, window, p);
  if (!hd) return 1;
  if (p == 0.f)
    return ob_flash_bwd_win_d_bf16(qkv, O, dO, lse, D_ws, dqkv, dbias_qkv, B,
                                   Sq, H, nh, window, scale, stream);
  if (window == 0 || window >= Sq)
    return hd == 64 ? ob_flash_bwd_nt_d_drop_bf16(qkv, O, dO, lse, D_ws, dqkv,
                                                  dbias_qkv, B, Sq, H, nh,
                                                  scale, seed, layer_id, tick,
                                                  p, stream)
                    : ob_flash_bwd_d_drop_hd128_bf16(
                          qkv, O, dO, lse, D_ws, dqkv, dbias_qkv, B, Sq, H, nh,
                          scale, seed, layer_id, tick, p, stream);
  const ob_drop_key key =
      ob_drop_make_key(seed, layer_id, OB_DROP_ATTN, tick, p);
  return hd == 64
             ? win_bwd_drop<64>(qkv, O, dO, lse, D_ws, dqkv, dbias_qkv, B, Sq,
                                H, nh, (int)window, scale, key, stream)
             : win_bwd_drop<128>(qkv, O, dO, lse, D_ws, dqkv, dbias_qkv, B,
                                 Sq, H, nh, (int)window, scale, key, stream);
}
