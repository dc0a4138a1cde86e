// ob_flash_bidir_bf16.hip — bidirectional (non-causal) flash attention, bf16,
// head_dim 64.  Every query row attends every key: the
// attention of an encoder block (Megatron-BERT, ViT) and of a prefix.  Three
// kernels, as in the causal production set: forward (O and the row LSE of the
// scaled scores), dQ (forming D = rowsum(dO * O) the way
// ob_flash_bwd_nt_d_bf16 does) and dK/dV; the backward recomputes P from Q, K
// and LSE.
//
// The per-tile arithmetic is the causal kernels' (ob_flash_bf16.hip): swapped
// QK^T so a lane owns one q column, bf_dance into the PV / dS A fragment,
// transposed B operands read column-wise from the row-major LDS tile (the
// nt_off image of ob_flash_common.h), double-buffered tiles under one barrier
// per tile, `scale` folded in the same places.  What is this file's own is
// the split of the work, which the causal triangle no longer shapes:
//   * Block map.  Every row costs the same, so there is nothing to fold
//     (ob_flash_fold.h pairs a light and a heavy piece of the triangle): a
//     block owns CONSECUTIVE rows.
//       forward / dQ: block a owns q rows 128a .. 128a+127, wave w the 32 rows
//         from 128a + 32w, and visits all S/64 kv tiles.
//       dK/dV: block x owns kv rows 64x .. 64x+63, wave pair p the 32 rows
//         from 64x + 32p, and visits all S/32 q tiles from tile 0.
//     Only the linear-id -> (head, block) map is the causal kernels'
//     (ob_fold_id / ob_fold_grid): the blocks of one head get ids of one XCD
//     and share its L2, which here holds the K/V (or Q/dO) every one of them
//     reads in full.
//   * No wave is ever inactive and every wave of a block runs the same number
//     of tiles, so the loops carry no wave-uniform activity tests: a wave
//     meets each barrier having done the same work as its neighbours.
//   * No mask: no score is -inf, so the forward's P is a bare exp, the
//     backward's P has no select, and the running max is finite after the
//     first tile (the first tile's rescale multiplies the zero accumulators
//     by exp(-inf) = 0).
// Resources: profiles/flash_bidir_resources.txt (no scratch, 3 waves/SIMD).
//
// Out of scope: head_dim 80 / 96 / 128, attention dropout, a window, a
// key-padding mask or variable lengths, the materialized-P and fp32 routes.
#include "ob_flash_common.h"
#include "ob_internal.h"
#include "ob_flash_fold.h"

#include <cmath>

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Stages two [ROWS][64] tiles (rows lda / ldb elements apart in memory) into
// their nt_off LDS images: 256 threads, 16-byte chunks, thread = chunk tid & 7
// of rows (tid >> 3) + 32i.  nt_key has period 16 in the row, so a thread's
// LDS offsets differ by constants.  All the loads are issued before the first
// store.
template <int ROWS>
__device__ __forceinline__ void bidir_stage2(__bf16* da, const __bf16* a,
                                             int64_t lda, __bf16* db,
                                             const __bf16* b, int64_t ldb,
                                             int tid) {
  constexpr int N = ROWS / 32;
  const int sr = tid >> 3, sc = tid & 7;
  const int so = nt_off(sr, sc);
  bf16x8 ra[N], rb[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    ra[i] = *reinterpret_cast<const bf16x8*>(a + (sr + 32 * i) * lda + sc * 8);
    rb[i] = *reinterpret_cast<const bf16x8*>(b + (sr + 32 * i) * ldb + sc * 8);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    *reinterpret_cast<bf16x8*>(da + so + 32 * 64 * i) = ra[i];
    *reinterpret_cast<bf16x8*>(db + so + 32 * 64 * i) = rb[i];
  }
}

// ===========================================================================
// Forward.  4 waves x 32 q rows; the block loops over all S/64 K/V tiles.
// Per tile: two independent S chains (the 32-row kv sub-tiles), tree
// reductions for the row max and sum, the O rescale skipped while no row's
// max grows by more than 8, four PV k-steps whose B fragments are columns of
// the V tile.  LDS: 2 x (K + V tile) + bcast = 32.5 KB.
// ===========================================================================
__global__ __launch_bounds__(256, 3) void k_flash_fwd_bidir(
    const __bf16* __restrict__ qkv, __bf16* __restrict__ Obase,
    float* __restrict__ lse, int Sq, int H, int nh, int Z, float scale) {
  __shared__ __attribute__((aligned(16))) __bf16 kbuf[2][64 * 64];
  __shared__ __attribute__((aligned(16))) __bf16 vbuf[2][64 * 64];
  __shared__ float bcast[128];
  int blk, z;
  if (!ob_fold_id(blockIdx.x, Sq / 128, Z, &blk, &z))
    return;  // block-uniform: grid padding
  const int b = z / nh, h = z % nh;
  const int64_t ld = 3 * (int64_t)H;
  const __bf16* Qp = qkv + (int64_t)b * Sq * ld + h * 64;
  const __bf16* Kp = Qp + H;
  const __bf16* Vp = Qp + 2 * H;
  __bf16* Op = Obase + (int64_t)b * Sq * H + h * 64;
  float* lsep = lse + (int64_t)z * Sq;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int il = lane & 31, kh = lane >> 5;
  const int q0 = 128 * blk + 32 * w;
  const int myq = q0 + il;

  bf16x8 qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
    qf[s] = *reinterpret_cast<const bf16x8*>(Qp + myq * ld + s * 16 + kh * 8);

  const int ntiles = Sq / 64;
  bidir_stage2<64>(kbuf[0], Kp, ld, vbuf[0], Vp, ld, tid);
  __syncthreads();

  f32x16 o0 = {}, o1 = {};
  float m = -INFINITY, l = 0.f;
  for (int kvt = 0; kvt < ntiles; ++kvt) {
    // tile t+1 goes into the buffer whose readers finished at the previous
    // barrier
    if (kvt + 1 < ntiles)
      bidir_stage2<64>(kbuf[(kvt + 1) & 1], Kp + (kvt + 1) * 64 * ld, ld,
                       vbuf[(kvt + 1) & 1], Vp + (kvt + 1) * 64 * ld, ld, tid);
    const __bf16* kb = kbuf[kvt & 1];
    const __bf16* vb = vbuf[kvt & 1];
    f32x16 sacc0 = {}, sacc1 = {};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int ch = s * 2 + kh;
      const bf16x8 ka = *reinterpret_cast<const bf16x8*>(&kb[nt_off(il, ch)]);
      const bf16x8 kb2 =
          *reinterpret_cast<const bf16x8*>(&kb[nt_off(32 + il, ch)]);
      sacc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qf[s], sacc0, 0, 0,
                                                      0);
      sacc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kb2, qf[s], sacc1, 0, 0,
                                                      0);
    }
    float sv[32];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      sv[r] = sacc0[r] * scale;
      sv[16 + r] = sacc1[r] * scale;
    }
    float mx[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      mx[j] = fmaxf(fmaxf(sv[j], sv[8 + j]), fmaxf(sv[16 + j], sv[24 + j]));
    float mt = fmaxf(fmaxf(fmaxf(mx[0], mx[1]), fmaxf(mx[2], mx[3])),
                     fmaxf(fmaxf(mx[4], mx[5]), fmaxf(mx[6], mx[7])));
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    // first tile: m = -inf, so every row rescales (by exp(-inf) = 0, on
    // zero accumulators) and m is finite from here on
    if (!__all(mt - m <= 8.f)) {
      const float mnew = fmaxf(m, mt);
      const float af = __expf(m - mnew);
      m = mnew;
      if (kh == 0) bcast[w * 32 + il] = af;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float a = bcast[w * 32 + acc_row(r, kh)];
        o0[r] *= a;
        o1[r] *= a;
      }
      l *= af;
    }
    float ps[8] = {};
#pragma unroll
    for (int r = 0; r < 32; ++r) {
      sv[r] = __expf(sv[r] - m);
      ps[r & 7] += sv[r];
    }
    float psum = ((ps[0] + ps[1]) + (ps[2] + ps[3])) +
                 ((ps[4] + ps[5]) + (ps[6] + ps[7]));
    psum += __shfl_xor(psum, 32, 64);
    l += psum;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const bf16x8 pa = bf_dance(sv + t * 8);
      // B[k = kv 16t+8kh..+7][n = d]: columns of the row-major V tile
      const bf16x8 v0f = nt_tr_frag(vb, lane, t * 16 + kh * 8, 0);
      const bf16x8 v1f = nt_tr_frag(vb, lane, t * 16 + kh * 8, 1);
      o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa, v0f, o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa, v1f, o1, 0, 0, 0);
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
    Op[(int64_t)(q0 + row) * H + il] = (__bf16)(o0[r] * inv);
    Op[(int64_t)(q0 + row) * H + 32 + il] = (__bf16)(o1[r] * inv);
  }
}

// ===========================================================================
// dQ: the forward's blocks and K/V staging.  Per tile two independent S / dP
// chain pairs (the 32-row kv sub-tiles), P = exp(scale * S - lse),
// dS = P * (dP - D), dQ += dS K with the K tile's columns as the B operand.
// D[q] = sum_d dO[q,d] * O[q,d] is formed from the resident dO fragments and
// O loaded in the same layout, in k_flash_dsum's summation order, used, and
// written to Dout for the dK/dV launch that follows.
// dbias (fp32 [3H], may be null): += column sums of this block's dQ tile.
// LDS: 2 x (K + V tile) + red = 33 KB.
// ===========================================================================
__global__ __launch_bounds__(256, 3) void k_flash_bwd_dq_bidir(
    const __bf16* __restrict__ qkv, const __bf16* __restrict__ dO,
    const float* __restrict__ lse, const __bf16* __restrict__ O,
    float* __restrict__ Dout, __bf16* __restrict__ dqkv,
    float* __restrict__ dbias, int Sq, int H, int nh, int Z, float scale) {
  __shared__ __attribute__((aligned(16))) __bf16 kbuf[2][64 * 64];
  __shared__ __attribute__((aligned(16))) __bf16 vbuf[2][64 * 64];
  __shared__ float red[4 * 64];
  int blk, z;
  if (!ob_fold_id(blockIdx.x, Sq / 128, Z, &blk, &z))
    return;  // block-uniform: grid padding
  const int b = z / nh, h = z % nh;
  const int64_t ld = 3 * (int64_t)H;
  const int64_t base = (int64_t)b * Sq * ld + h * 64;
  const __bf16* Qp = qkv + base;
  const __bf16* Kp = Qp + H;
  const __bf16* Vp = Qp + 2 * H;
  const int64_t obase = (int64_t)b * Sq * H + h * 64;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int il = lane & 31, kh = lane >> 5;
  const int q0 = 128 * blk + 32 * w;
  const int myq = q0 + il;
  const float mylse = lse[(int64_t)z * Sq + myq];

  bf16x8 qf[4], df[4];
  float cs[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    qf[s] = *reinterpret_cast<const bf16x8*>(Qp + myq * ld + s * 16 + kh * 8);
    df[s] = *reinterpret_cast<const bf16x8*>(dO + obase + (int64_t)myq * H +
                                             s * 16 + kh * 8);
    const bf16x8 ov = *reinterpret_cast<const bf16x8*>(
        O + obase + (int64_t)myq * H + s * 16 + kh * 8);
    float c = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) c += bf2f(ov[j]) * bf2f(df[s][j]);
    cs[s] = c;
  }
  // cs[s] = chunk 2s + kh: this half's bracket, then the other half's
  const float part = (cs[0] + cs[2]) + (cs[1] + cs[3]);
  const float myD = part + __shfl_xor(part, 32, 64);
  if (kh == 0) Dout[(int64_t)z * Sq + myq] = myD;

  const int ntiles = Sq / 64;
  bidir_stage2<64>(kbuf[0], Kp, ld, vbuf[0], Vp, ld, tid);
  __syncthreads();

  f32x16 dq0 = {}, dq1 = {};
  for (int kvt = 0; kvt < ntiles; ++kvt) {
    if (kvt + 1 < ntiles)
      bidir_stage2<64>(kbuf[(kvt + 1) & 1], Kp + (kvt + 1) * 64 * ld, ld,
                       vbuf[(kvt + 1) & 1], Vp + (kvt + 1) * 64 * ld, ld, tid);
    const __bf16* kb = kbuf[kvt & 1];
    const __bf16* vb = vbuf[kvt & 1];
    f32x16 s0 = {}, s1 = {}, p0 = {}, p1 = {};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int ch = s * 2 + kh;
      const bf16x8 ka = *reinterpret_cast<const bf16x8*>(&kb[nt_off(il, ch)]);
      const bf16x8 kb2 =
          *reinterpret_cast<const bf16x8*>(&kb[nt_off(32 + il, ch)]);
      const bf16x8 va = *reinterpret_cast<const bf16x8*>(&vb[nt_off(il, ch)]);
      const bf16x8 vb2 =
          *reinterpret_cast<const bf16x8*>(&vb[nt_off(32 + il, ch)]);
      s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qf[s], s0, 0, 0, 0);
      s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kb2, qf[s], s1, 0, 0, 0);
      p0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, df[s], p0, 0, 0, 0);
      p1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vb2, df[s], p1, 0, 0, 0);
    }
    float dsv[32];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      dsv[r] = __expf(s0[r] * scale - mylse) * (p0[r] - myD);
      dsv[16 + r] = __expf(s1[r] * scale - mylse) * (p1[r] - myD);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const bf16x8 da = bf_dance(dsv + t * 8);
      // B[k = kv 16t+8kh..+7][n = d]: columns of the row-major K tile
      const bf16x8 kt0 = nt_tr_frag(kb, lane, t * 16 + kh * 8, 0);
      const bf16x8 kt1 = nt_tr_frag(kb, lane, t * 16 + kh * 8, 1);
      dq0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da, kt0, dq0, 0, 0, 0);
      dq1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da, kt1, dq1, 0, 0, 0);
    }
    __syncthreads();
  }
  __bf16* dQp = dqkv + base;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t q = q0 + acc_row(r, kh);
    dQp[q * ld + il] = (__bf16)(scale * dq0[r]);
    dQp[q * ld + 32 + il] = (__bf16)(scale * dq1[r]);
  }
  if (dbias) {  // kernel-uniform
    float c0 = 0.f, c1 = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      c0 += scale * dq0[r];
      c1 += scale * dq1[r];
    }
    c0 += __shfl_xor(c0, 32, 64);
    c1 += __shfl_xor(c1, 32, 64);
    if (kh == 0) {
      red[w * 64 + il] = c0;
      red[w * 64 + 32 + il] = c1;
    }
    __syncthreads();
    if (tid < 64)
      atomicAdd(dbias + h * 64 + tid, (red[tid] + red[64 + tid]) +
                                          (red[128 + tid] + red[192 + tid]));
  }
}

// ===========================================================================
// dK/dV: the causal kernel's split-duty wave pairs (role 0: K resident,
// S -> P -> dV; role 1: V resident, dP -> dS -> dK; only P crosses the pair,
// through xch) over all S/32 q tiles, from tile 0: both pairs compute in
// every iteration.  The B fragments are read before the iteration's barrier:
// after it a fast wave already stages tile qt+2 into this buffer.
// dbias (fp32 [3H], may be null): += column sums of this block's dK and dV
// tiles, from the fp32 accumulators after `scale`, before rounding.
// LDS: xch 16 KB + 2 x (Q + dO tile) + red = 33 KB.
// ===========================================================================
__global__ __launch_bounds__(256, 3) void k_flash_bwd_dkdv_bidir(
    const __bf16* __restrict__ qkv, const __bf16* __restrict__ dO,
    const float* __restrict__ lse, const float* __restrict__ D,
    __bf16* __restrict__ dqkv, float* __restrict__ dbias, int Sq, int H,
    int nh, int Z, float scale) {
  __shared__ float xch[2][2][32 * 32];  // [buffer][pair][P tile]
  __shared__ __attribute__((aligned(16))) __bf16 qbuf[2][32 * 64];
  __shared__ __attribute__((aligned(16))) __bf16 obuf[2][32 * 64];
  __shared__ float red[4 * 64];
  int blk, z;
  if (!ob_fold_id(blockIdx.x, Sq / 64, Z, &blk, &z))
    return;  // block-uniform: grid padding
  const int b = z / nh, h = z % nh;
  const int64_t ld = 3 * (int64_t)H;
  const int64_t base = (int64_t)b * Sq * ld + h * 64;
  const __bf16* Qp = qkv + base;
  const __bf16* dOp = dO + (int64_t)b * Sq * H + h * 64;
  const float* lsep = lse + (int64_t)z * Sq;
  const float* Dp = D + (int64_t)z * Sq;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int pair = w >> 1, role = w & 1;
  const int il = lane & 31, kh = lane >> 5;
  const int kv0 = 64 * blk + 32 * pair;
  const int mykv = kv0 + il;

  const __bf16* KV = Qp + (role ? 2 * H : H);
  bf16x8 of[4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
    of[s] = *reinterpret_cast<const bf16x8*>(KV + mykv * ld + s * 16 + kh * 8);

  const int nqt = Sq / 32;
  bidir_stage2<32>(qbuf[0], Qp, ld, obuf[0], dOp, H, tid);
  __syncthreads();

  f32x16 acc0 = {}, acc1 = {};  // role 0: dV d-halves; role 1: dK d-halves
  for (int qt = 0; qt < nqt; ++qt) {
    const int q0 = qt * 32;
    if (qt + 1 < nqt)
      bidir_stage2<32>(qbuf[(qt + 1) & 1], Qp + (q0 + 32) * ld, ld,
                       obuf[(qt + 1) & 1], dOp + (int64_t)(q0 + 32) * H, H,
                       tid);
    // own tile's A image, and the B image: role 0 multiplies P^T by dO,
    // role 1 dS^T by Q
    const __bf16* ab = role ? obuf[qt & 1] : qbuf[qt & 1];
    const __bf16* bb = role ? qbuf[qt & 1] : obuf[qt & 1];
    const bf16x8 b00 = nt_tr_frag(bb, lane, kh * 8, 0);
    const bf16x8 b01 = nt_tr_frag(bb, lane, kh * 8, 1);
    const bf16x8 b10 = nt_tr_frag(bb, lane, 16 + kh * 8, 0);
    const bf16x8 b11 = nt_tr_frag(bb, lane, 16 + kh * 8, 1);
    // own tile: S (role 0, A = Q rows) or dP (role 1, A = dO rows)
    f32x16 own = {};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const bf16x8 af =
          *reinterpret_cast<const bf16x8*>(&ab[nt_off(il, s * 2 + kh)]);
      own = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, of[s], own, 0, 0, 0);
    }
    float pv[16];
    float* ptile = xch[qt & 1][pair];
    if (role == 0) {
      const float lse_t = lsep[q0 + il];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qoff = acc_row(r, kh);
        const float lse_q = __shfl(lse_t, qoff, 64);
        pv[r] = __expf(own[r] * scale - lse_q);
        ptile[qoff * 32 + il] = pv[r];
      }
    }
    __syncthreads();
    if (role == 1) {
      const float d_t = Dp[q0 + il];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qoff = acc_row(r, kh);
        const float d_q = __shfl(d_t, qoff, 64);
        pv[r] = ptile[qoff * 32 + il] * (own[r] - d_q);  // dS = P * (dP - D)
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const bf16x8 a = bf_dance(pv + t * 8);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, t ? b10 : b00, acc0,
                                                     0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, t ? b11 : b01, acc1,
                                                     0, 0, 0);
    }
  }

  __bf16* outp = dqkv + base + (role ? H : 2 * H);  // dK or dV slice
  const float os = role ? scale : 1.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t kv = kv0 + acc_row(r, kh);
    outp[kv * ld + il] = (__bf16)(os * acc0[r]);
    outp[kv * ld + 32 + il] = (__bf16)(os * acc1[r]);
  }
  if (dbias) {  // kernel-uniform
    float c0 = 0.f, c1 = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      c0 += os * acc0[r];
      c1 += os * acc1[r];
    }
    c0 += __shfl_xor(c0, 32, 64);
    c1 += __shfl_xor(c1, 32, 64);
    if (kh == 0) {
      red[w * 64 + il] = c0;
      red[w * 64 + 32 + il] = c1;
    }
    __syncthreads();
    if (tid < 128) {
      // waves 0/2 hold dV (role 0), waves 1/3 dK (role 1)
      const int rl = tid >> 6, c = tid & 63;
      atomicAdd(dbias + (rl ? H : 2 * H) + h * 64 + c,
                red[rl * 64 + c] + red[(2 + rl) * 64 + c]);
    }
  }
}

// ---- entries ----------------------------------------------------------------
// 0, or 1 with ob_fail set: head_dim 64, S a positive multiple of 128, and a
// head count the int block ids hold
static int bidir_args_ok(const char* who, int64_t B, int64_t Sq, int64_t H,
                         int64_t nh) {
  if (nh <= 0 || H != 64 * nh) return ob_fail("%s: head_dim must be 64", who);
  if (B <= 0 || Sq <= 0 || Sq % 128)
    return ob_fail("%s: B must be positive and S a positive multiple of 128",
                   who);
  if ((B * nh + 7) / 8 * 8 * (Sq / 64) > (int64_t)INT32_MAX)
    return ob_fail("%s: B*nh*S/64 exceeds the block ids", who);
  return 0;
}

extern "C" int ob_flash_fwd_bidir_bf16(const void* qkv, void* O, void* lse,
                                       int64_t B, int64_t Sq, int64_t H,
                                       int64_t nh, float scale, void* stream) {
  if (bidir_args_ok("flash_fwd_bidir", B, Sq, H, nh)) return 1;
  const int Z = (int)(B * nh);
  k_flash_fwd_bidir<<<ob_fold_grid((int)Sq / 128, Z), 256, 0, S(stream)>>>(
      (const __bf16*)qkv, (__bf16*)O, (float*)lse, (int)Sq, (int)H, (int)nh, Z,
      scale);
  OB_LAUNCH_CHECK();
  return 0;
}

// dq first (forms D from O and dO into D_ws), then dkdv, which reads it
extern "C" int ob_flash_bwd_bidir_d_bf16(const void* qkv, const void* O,
                                         const void* dO, const void* lse,
                                         void* D_ws, void* dqkv,
                                         void* dbias_qkv, int64_t B, int64_t Sq,
                                         int64_t H, int64_t nh, float scale,
                                         void* stream) {
  if (bidir_args_ok("flash_bwd_bidir_d", B, Sq, H, nh)) return 1;
  const int Z = (int)(B * nh);
  k_flash_bwd_dq_bidir<<<ob_fold_grid((int)Sq / 128, Z), 256, 0, S(stream)>>>(
      (const __bf16*)qkv, (const __bf16*)dO, (const float*)lse,
      (const __bf16*)O, (float*)D_ws, (__bf16*)dqkv, (float*)dbias_qkv,
      (int)Sq, (int)H, (int)nh, Z, scale);
  OB_LAUNCH_CHECK();
  k_flash_bwd_dkdv_bidir<<<ob_fold_grid((int)Sq / 64, Z), 256, 0, S(stream)>>>(
      (const __bf16*)qkv, (const __bf16*)dO, (const float*)lse,
      (const float*)D_ws, (__bf16*)dqkv, (float*)dbias_qkv, (int)Sq, (int)H,
      (int)nh, Z, scale);
  OB_LAUNCH_CHECK();
  return 0;
}
