// ob_flash_gqa_bf16.hip — fused causal flash attention with shared K/V heads
// (grouped-query and multi-query attention), bf16, head_dim 128 (DESIGN.md §8
// item 25).  n_kv K/V heads serve nh query heads, G = nh / n_kv per group;
// Hkv = 128 * n_kv, and the packed operand is W = H + 2 * Hkv columns wide:
//   [ Q heads 0..nh-1 (H) | K heads 0..n_kv-1 (Hkv) | V heads 0..n_kv-1 (Hkv) ]
// (GPT-BigCode's c_attn output at n_kv = 1).  O, dO, lse and D are the dense
// entries': [B, Sq, H] and [B*nh, Sq].
//
// The arithmetic definition is ob_flash_hd128_bf16.hip's: swapped QK^T, online
// softmax with the defer-max skip, LSE of the scaled scores, backward
// recomputed from Q, K and LSE, dS = P*(dP - D), `scale` folded in the same
// places, dbias from the fp32 accumulators after `scale`; the LDS image is
// hd_off / hd_tr_frag of ob_flash_common.h and the block -> rows fold is
// ob_flash_fold.h, both unchanged.
//
// Forward and dQ are the hd-128 kernels with query head h reading K/V head
// h / G at row stride W.  Only the placement differs: the heads of a group
// share K/V, so gqa_place deals each XCD a contiguous run of heads (see
// there).
//
// dK/dV is the new kernel.  A K/V tile's gradient is the sum over its group's
// query heads, so a block owns (batch, kv head, part, folded kv-tile pair):
// its K or V fragments stay resident and its four accumulators persist across
// a loop over the part's G/split heads and, inside, each head's q tiles from
// the diagonal to the end.  The Q/dO staging is double-buffered over the
// flattened (head, q tile) sequence, so the first tile of the next head is
// staged while the last tile of the current one computes.  split == 1 stores
// one bf16 rounding of the fp32 group sum; split > 1 writes fp32 partials to
// the part's own slab and k_gqa_fold adds the slabs in ascending order and
// rounds once.  No atomic touches dK/dV in either form (dbias_qkv is summed
// with atomics, as everywhere on the non-deterministic path).
#include "ob_flash_common.h"
#include "ob_internal.h"
#include "ob_flash_fold.h"

#include <cmath>

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Placement of the forward / dq heads.  ob_fold_id gives linear id -> (blk,
// z') with z' % 8 the XCD; its z' -> head map (identity) would deal the G
// heads of a group round-robin over the XCDs, every L2 holding every K/V
// head.  Here XCD r takes the contiguous run of ceil(Z/8) heads starting at
// r * ceil(Z/8): heads are numbered (batch, kv head, member), so a run covers
// as few groups as a run can, and when B * n_kv % 8 == 0 every group sits in
// one XCD whole.  A bijection of [0, 8*ceil(Z/8)) onto itself; ids past Z are
// the grid padding ob_fold_grid already launches.  Speed only.
__device__ __forceinline__ bool gqa_place(unsigned id, int nblk, int Z,
                                          int* blk, int* z) {
  int zp;
  ob_fold_id(id, nblk, OB_FOLD_XCDS * ((Z + OB_FOLD_XCDS - 1) / OB_FOLD_XCDS),
             blk, &zp);
  *z = (zp % OB_FOLD_XCDS) * ((Z + OB_FOLD_XCDS - 1) / OB_FOLD_XCDS) +
       zp / OB_FOLD_XCDS;
  return *z < Z;
}

// Forward: k_flash_fwd_hd128 (4 waves x 32 q rows, the two folded 64-row
// halves, KVBLK 64, K/V double-buffered in LDS, one barrier per tile).
// LDS: 2 x (16 KB K + 16 KB V) + bcast = 64.5 KB, two blocks per CU.
__global__ __launch_bounds__(256, 2) void k_flash_fwd_gqa(
    const __bf16* __restrict__ qkv, __bf16* __restrict__ Obase,
    float* __restrict__ lse, int Sq, int H, int nh, int n_kv, int Z,
    float scale) {
  __shared__ __attribute__((aligned(16))) __bf16 kbuf[2][64 * 128];
  __shared__ __attribute__((aligned(16))) __bf16 vbuf[2][64 * 128];
  __shared__ float bcast[128];
  int blk, z;
  if (!gqa_place(blockIdx.x, ob_fold_q_nblk(Sq), Z, &blk, &z))
    return;  // block-uniform: grid padding
  const int b = z / nh, h = z % nh;
  const int Hkv = 128 * n_kv, W = H + 2 * Hkv;
  const int g = h / (nh / n_kv);
  const __bf16* Qp = qkv + (int64_t)b * Sq * W + h * 128;
  const __bf16* Kp = qkv + (int64_t)b * Sq * W + H + g * 128;
  const __bf16* Vp = Kp + Hkv;
  __bf16* Op = Obase + (int64_t)b * Sq * H + h * 128;
  float* lsep = lse + (int64_t)z * Sq;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int il = lane & 31, kh = lane >> 5;
  const int q0 = ob_fold_q_row0(Sq, blk, w);
  const int myq = q0 + il;
  const int mytiles = ob_fold_q_wave_tiles(q0);

  // staging: thread covers chunk tid&15 of rows (tid>>4) + 16i, i = 0..3
  const int sr = tid >> 4, sc = tid & 15;
  const int so = hd_off(sr, sc);
  auto stage = [&](int buf, int kv0) {
    bf16x8 kr[4], vr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      kr[i] = *reinterpret_cast<const bf16x8*>(
          Kp + (int64_t)(kv0 + sr + 16 * i) * W + sc * 8);
      vr[i] = *reinterpret_cast<const bf16x8*>(
          Vp + (int64_t)(kv0 + sr + 16 * i) * W + sc * 8);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<bf16x8*>(&kbuf[buf][so + 16 * 128 * i]) = kr[i];
      *reinterpret_cast<bf16x8*>(&vbuf[buf][so + 16 * 128 * i]) = vr[i];
    }
  };

  bf16x8 qf[8];
#pragma unroll
  for (int s = 0; s < 8; ++s)
    qf[s] = *reinterpret_cast<const bf16x8*>(Qp + (int64_t)myq * W + s * 16 +
                                             kh * 8);

  const int ntiles = ob_fold_q_block_tiles(Sq, blk);  // block-uniform
  stage(0, 0);
  __syncthreads();

  f32x16 o[4] = {};
  float m = -INFINITY, l = 0.f;
  for (int kvt = 0; kvt < ntiles; ++kvt) {
    const int kv0 = kvt * 64;
    if (kvt + 1 < ntiles) stage((kvt + 1) & 1, kv0 + 64);
    const bool active = kvt < mytiles;  // kv0 <= q0 + 31, wave-uniform
    if (active) {
      const __bf16* kb = kbuf[kvt & 1];
      const __bf16* vb = vbuf[kvt & 1];
      f32x16 sacc0 = {}, sacc1 = {};
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int ch = (s * 2 + kh);
        const bf16x8 ka =
            *reinterpret_cast<const bf16x8*>(&kb[hd_off(il, ch)]);
        const bf16x8 kb2 =
            *reinterpret_cast<const bf16x8*>(&kb[hd_off(32 + il, ch)]);
        sacc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qf[s], sacc0, 0,
                                                        0, 0);
        sacc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kb2, qf[s], sacc1,
                                                        0, 0, 0);
      }
      float sv[32];
      if (kv0 + 63 < q0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          sv[r] = sacc0[r] * scale;
          sv[16 + r] = sacc1[r] * scale;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kvr = kv0 + acc_row(r, kh);
          sv[r] = (kvr <= myq) ? sacc0[r] * scale : -INFINITY;
          sv[16 + r] = (kvr + 32 <= myq) ? sacc1[r] * scale : -INFINITY;
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
      const bool rescale = !__all(mt - m <= 8.f);
      if (rescale) {
        const float mnew = fmaxf(m, mt);
        const float af = __expf(m - mnew);
        m = mnew;
        if (kh == 0) bcast[w * 32 + il] = af;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float a = bcast[w * 32 + acc_row(r, kh)];
#pragma unroll
          for (int d = 0; d < 4; ++d) o[d][r] *= a;
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
        const bf16x8 pa = bf_dance(sv + t * 8);
        // B[k = kv 16t+8kh..+7][n = d]: columns of the row-major V tile
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const bf16x8 vf = hd_tr_frag(vb, lane, t * 16 + kh * 8, d);
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
    for (int d = 0; d < 4; ++d)
      Op[(int64_t)(q0 + row) * H + 32 * d + il] = (__bf16)(o[d][r] * inv);
  }
}

// dQ: k_flash_bwd_dq_hd128<true> (the forward's blocks and K/V staging; the
// two 32-row kv sub-tiles of a tile in turn; D formed from the resident dO
// fragments and O, used, and written to Dout for the dkdv launch).
// LDS: 2 x (16 KB K + 16 KB V) + red 2 KB = 66 KB.
__global__ __launch_bounds__(256, 2) void k_flash_bwd_dq_gqa(
    const __bf16* __restrict__ qkv, const __bf16* __restrict__ dO,
    const float* __restrict__ lse, const __bf16* __restrict__ O,
    float* __restrict__ Dout, __bf16* __restrict__ dqkv,
    float* __restrict__ dbias, int Sq, int H, int nh, int n_kv, int Z,
    float scale) {
  __shared__ __attribute__((aligned(16))) __bf16 kbuf[2][64 * 128];
  __shared__ __attribute__((aligned(16))) __bf16 vbuf[2][64 * 128];
  __shared__ float red[4 * 128];
  int blk, z;
  if (!gqa_place(blockIdx.x, ob_fold_q_nblk(Sq), Z, &blk, &z))
    return;  // block-uniform: grid padding
  const int b = z / nh, h = z % nh;
  const int Hkv = 128 * n_kv, W = H + 2 * Hkv;
  const int g = h / (nh / n_kv);
  const int64_t base = (int64_t)b * Sq * W + h * 128;
  const __bf16* Qp = qkv + base;
  const __bf16* Kp = qkv + (int64_t)b * Sq * W + H + g * 128;
  const __bf16* Vp = Kp + Hkv;
  const __bf16* dOp = dO + (int64_t)b * Sq * H + h * 128;
  const float* lsep = lse + (int64_t)z * Sq;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int il = lane & 31, kh = lane >> 5;
  const int q0 = ob_fold_q_row0(Sq, blk, w);
  const int myq = q0 + il;
  const int mytiles = ob_fold_q_wave_tiles(q0);
  const float mylse = lsep[myq];

  bf16x8 qf[8], df[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    qf[s] = *reinterpret_cast<const bf16x8*>(Qp + (int64_t)myq * W + s * 16 +
                                             kh * 8);
    df[s] = *reinterpret_cast<const bf16x8*>(dOp + (int64_t)myq * H + s * 16 +
                                             kh * 8);
  }
  float myD;
  {
    const __bf16* Orow = O + (int64_t)b * Sq * H + h * 128 + (int64_t)myq * H;
    float part = 0.f;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const bf16x8 ov =
          *reinterpret_cast<const bf16x8*>(Orow + s * 16 + kh * 8);
      float c = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) c += bf2f(ov[j]) * bf2f(df[s][j]);
      part += c;
    }
    myD = part + __shfl_xor(part, 32, 64);
    if (kh == 0) Dout[(int64_t)z * Sq + myq] = myD;
  }

  // staging: thread covers chunk tid&15 of rows (tid>>4) + 16i, i = 0..3
  const int sr = tid >> 4, sc = tid & 15;
  const int so = hd_off(sr, sc);
  auto stage = [&](int buf, int kv0) {
    bf16x8 kr[4], vr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      kr[i] = *reinterpret_cast<const bf16x8*>(
          Kp + (int64_t)(kv0 + sr + 16 * i) * W + sc * 8);
      vr[i] = *reinterpret_cast<const bf16x8*>(
          Vp + (int64_t)(kv0 + sr + 16 * i) * W + sc * 8);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<bf16x8*>(&kbuf[buf][so + 16 * 128 * i]) = kr[i];
      *reinterpret_cast<bf16x8*>(&vbuf[buf][so + 16 * 128 * i]) = vr[i];
    }
  };

  const int ntiles = ob_fold_q_block_tiles(Sq, blk);  // block-uniform
  stage(0, 0);
  __syncthreads();

  f32x16 dq[4] = {};
  for (int kvt = 0; kvt < ntiles; ++kvt) {
    const int kv0 = kvt * 64;
    if (kvt + 1 < ntiles) stage((kvt + 1) & 1, kv0 + 64);
    // wave-uniform causal skip: kv0 <= q0 + 31
    const bool active = kvt < mytiles;
    if (active) {
      const __bf16* kb = kbuf[kvt & 1];
      const __bf16* vb = vbuf[kvt & 1];
#pragma unroll
      for (int u = 0; u < 2; ++u) {  // 32-row kv sub-tiles, in turn
        f32x16 sa = {}, pa = {};
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const int ch = s * 2 + kh;
          const bf16x8 ka = *reinterpret_cast<const bf16x8*>(
              &kb[hd_off(32 * u + il, ch)]);
          const bf16x8 va = *reinterpret_cast<const bf16x8*>(
              &vb[hd_off(32 * u + il, ch)]);
          sa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qf[s], sa, 0, 0,
                                                       0);
          pa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, df[s], pa, 0, 0,
                                                       0);
        }
        float dsv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kv = kv0 + 32 * u + acc_row(r, kh);
          const bool ok = kv <= myq;
          const float p = ok ? __expf(sa[r] * scale - mylse) : 0.f;
          dsv[r] = ok ? p * (pa[r] - myD) : 0.f;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const bf16x8 da = bf_dance(dsv + t * 8);
          // B[k = kv 32u+16t+8kh..+7][n = d]: columns of the K tile
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            const bf16x8 kt =
                hd_tr_frag(kb, lane, 32 * u + 16 * t + kh * 8, d);
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
    for (int d = 0; d < 4; ++d)
      dQp[(int64_t)q * W + 32 * d + il] = (__bf16)(scale * dq[d][r]);
  }
  if (dbias) {  // kernel-uniform
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      float c = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) c += scale * dq[d][r];
      c += __shfl_xor(c, 32, 64);
      if (kh == 0) red[w * 128 + 32 * d + il] = c;
    }
    __syncthreads();
    if (tid < 128)
      atomicAdd(dbias + h * 128 + tid, (red[tid] + red[128 + tid]) +
                                           (red[256 + tid] + red[384 + tid]));
  }
}

// dK/dV: k_flash_bwd_dkdv_hd128's split-duty wave pairs (role 0: K resident,
// S -> P -> dV; role 1: V resident, dP -> dS -> dK; only P crosses the pair,
// through xch) with the accumulators carried over the heads of the block's
// part.  Unit u of the launch is (batch b, kv head g, part j) = (u / split /
// n_kv, u / split % n_kv, u % split); it owns query heads g*G + j*G/split ..
// + G/split - 1.  The blocks of a unit read the same Q/dO, so ob_fold_id's
// one-XCD-per-unit placement is kept as it is.
// The loop runs over the flattened sequence it = (head, q tile qt0..nqt-1);
// LDS buffers and the xch tile alternate on `it`, so the barrier argument is
// the dense kernel's with qt replaced by it, and staging never drains at a
// head boundary.  Everything that changes with the head (Q, dO, lse, D bases)
// is block-uniform.
// kSlab false: one bf16 store of the group sum into dqkv and the block's
// column sums added to dbias.  kSlab true: fp32 partials into slab[part]
// ([B*Sq][2*Hkv]: K head g at 128*g, V head g at Hkv + 128*g); k_gqa_fold
// finishes.
// LDS: xch 16 KB + 2 x (8 KB Q + 8 KB dO) + red 2 KB = 50 KB.
template <bool kSlab>
__global__ __launch_bounds__(256, 2) void k_flash_bwd_dkdv_gqa(
    const __bf16* __restrict__ qkv, const __bf16* __restrict__ dO,
    const float* __restrict__ lse, const float* __restrict__ D,
    __bf16* __restrict__ dqkv, float* __restrict__ dbias,
    float* __restrict__ slab, int B, int Sq, int H, int nh, int n_kv,
    int split, float scale) {
  __shared__ float xch[2][2][32 * 32];  // [buffer][pair][P tile]
  __shared__ __attribute__((aligned(16))) __bf16 qbuf[2][32 * 128];
  __shared__ __attribute__((aligned(16))) __bf16 obuf[2][32 * 128];
  __shared__ float red[4 * 128];
  int blk, u;
  if (!ob_fold_id(blockIdx.x, ob_fold_kv_nblk(Sq), B * n_kv * split, &blk, &u))
    return;  // block-uniform: grid padding
  const int part = u % split, gi = u / split;
  const int b = gi / n_kv, g = gi % n_kv;
  const int Hkv = 128 * n_kv, W = H + 2 * Hkv;
  const int nheads = nh / n_kv / split;
  const int h0 = g * (nh / n_kv) + part * nheads;
  const __bf16* Kp = qkv + (int64_t)b * Sq * W + H + g * 128;
  const __bf16* Vp = Kp + Hkv;
  // head h of this batch: Q at Qb + 128h (stride W), dO at dOb + 128h
  // (stride H), lse and D rows at (b*nh + h) * Sq
  const __bf16* Qb = qkv + (int64_t)b * Sq * W;
  const __bf16* dOb = dO + (int64_t)b * Sq * H;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int pair = w >> 1, role = w & 1;
  const int il = lane & 31, kh = lane >> 5;
  const int kv0 = ob_fold_kv_row0(Sq, blk, pair);
  const int mykv = kv0 + il;
  const int myqt0 = ob_fold_kv_pair_first(kv0);

  const __bf16* KV = role ? Vp : Kp;
  bf16x8 of[8];
#pragma unroll
  for (int s = 0; s < 8; ++s)
    of[s] = *reinterpret_cast<const bf16x8*>(KV + (int64_t)mykv * W + s * 16 +
                                             kh * 8);

  // staging: thread covers chunk tid&15 of rows tid>>4 and (tid>>4) + 16
  const int srow = tid >> 4, schunk = tid & 15;
  const int so = hd_off(srow, schunk);
  auto stage = [&](int buf, int h, int q0s) {
    const __bf16* Qp = Qb + h * 128;
    const __bf16* dOp = dOb + h * 128;
    bf16x8 qr[2], dr[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      qr[i] = *reinterpret_cast<const bf16x8*>(
          Qp + (int64_t)(q0s + srow + 16 * i) * W + schunk * 8);
      dr[i] = *reinterpret_cast<const bf16x8*>(
          dOp + (int64_t)(q0s + srow + 16 * i) * H + schunk * 8);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<bf16x8*>(&qbuf[buf][so + 16 * 128 * i]) = qr[i];
      *reinterpret_cast<bf16x8*>(&obuf[buf][so + 16 * 128 * i]) = dr[i];
    }
  };

  f32x16 acc[4] = {};  // role 0: dV d quarters; role 1: dK d quarters
  const int nqt = Sq / 32;
  const int qt0 = ob_fold_kv_block_first(blk);  // block-uniform
  const int total = nheads * (nqt - qt0);       // block-uniform
  stage(0, h0, qt0 * 32);
  __syncthreads();

  int hn = h0, qn = qt0;  // the (head, q tile) of iteration `it`
  for (int it = 0; it < total; ++it) {
    const int h = hn, qt = qn;
    const int q0 = qt * 32;
    if (++qn == nqt) qn = qt0, ++hn;  // next iteration's, across heads
    if (it + 1 < total) stage((it + 1) & 1, hn, qn * 32);
    // wave-uniform: pair 1 idles (staging and the barrier only) until the
    // head's loop reaches its diagonal, q0 + 31 >= kv0.  Each wave meets
    // exactly one barrier per iteration on either side of the branch.
    if (qt < myqt0) {
      __syncthreads();
      continue;
    }
    // own tile's A image, and the B image: role 0 multiplies P^T by dO,
    // role 1 dS^T by Q
    const __bf16* ab = role ? obuf[it & 1] : qbuf[it & 1];
    const __bf16* bb = role ? qbuf[it & 1] : obuf[it & 1];
    // B-operands early (before the barrier): 4 d quarters, k = q rows
    bf16x8 bf[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int d = 0; d < 4; ++d)
        bf[t][d] = hd_tr_frag(bb, lane, 16 * t + kh * 8, d);
    // own tile: S (role 0, A = Q rows) or dP (role 1, A = dO rows)
    f32x16 own = {};
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int ch = s * 2 + kh;
      const bf16x8 af = *reinterpret_cast<const bf16x8*>(&ab[hd_off(il, ch)]);
      own = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, of[s], own, 0, 0, 0);
    }
    float pv[16];
    float* ptile = xch[it & 1][pair];
    const int64_t rowq = (int64_t)(b * nh + h) * Sq + q0 + il;
    if (role == 0) {
      const float lse_t = lse[rowq];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qoff = acc_row(r, kh);
        const bool ok = q0 + qoff >= mykv;
        const float lse_q = __shfl(lse_t, qoff, 64);
        pv[r] = ok ? __expf(own[r] * scale - lse_q) : 0.f;
        ptile[qoff * 32 + il] = pv[r];
      }
    }
    __syncthreads();
    if (role == 1) {
      const float d_t = D[rowq];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qoff = acc_row(r, kh);
        const float d_q = __shfl(d_t, qoff, 64);
        // dS = P * (dP - D); masked entries have P == 0 already
        pv[r] = ptile[qoff * 32 + il] * (own[r] - d_q);
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const bf16x8 a = bf_dance(pv + t * 8);
#pragma unroll
      for (int d = 0; d < 4; ++d)
        acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bf[t][d], acc[d],
                                                         0, 0, 0);
    }
  }

  const float os = role ? scale : 1.f;
  if constexpr (kSlab) {
    // role 1 (dK) at column 128g, role 0 (dV) at Hkv + 128g of the part's slab
    float* outp = slab + ((int64_t)part * B + b) * Sq * 2 * Hkv +
                  (role ? 0 : Hkv) + g * 128;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kv = kv0 + acc_row(r, kh);
#pragma unroll
      for (int d = 0; d < 4; ++d)
        outp[(int64_t)kv * 2 * Hkv + 32 * d + il] = os * acc[d][r];
    }
  } else {
    const int col = H + (role ? 0 : Hkv) + g * 128;  // dK or dV slice
    __bf16* outp = dqkv + (int64_t)b * Sq * W + col;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kv = kv0 + acc_row(r, kh);
#pragma unroll
      for (int d = 0; d < 4; ++d)
        outp[(int64_t)kv * W + 32 * d + il] = (__bf16)(os * acc[d][r]);
    }
    if (dbias) {  // kernel-uniform
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        float c = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) c += os * acc[d][r];
        c += __shfl_xor(c, 32, 64);
        if (kh == 0) red[w * 128 + 32 * d + il] = c;
      }
      __syncthreads();
      {
        // waves 0/2 hold dV (role 0), waves 1/3 dK (role 1)
        const int rl = tid >> 7, c = tid & 127;
        atomicAdd(dbias + H + (rl ? 0 : Hkv) + g * 128 + c,
                  red[rl * 128 + c] + red[(2 + rl) * 128 + c]);
      }
    }
  }
}

// The fold of a split dK/dV: dqkv[row, H + c] = bf16(slab[0][row][c] + ... +
// slab[split-1][row][c]) for c < 2*Hkv, the parts added in ascending order,
// and the column sums of those fp32 sums added to dbias[H + c].  A block
// covers 16 rows x 256 columns, a thread one column: every row is a 1 KB
// coalesced read per part and a 512 B store.
constexpr int GQA_FOLD_ROWS = 16;
__global__ __launch_bounds__(256) void k_gqa_fold(
    const float* __restrict__ slab, __bf16* __restrict__ dqkv,
    float* __restrict__ dbias, int64_t rows, int H, int Hkv, int split) {
  const int c = blockIdx.y * 256 + threadIdx.x;  // < 2*Hkv: 2*Hkv % 256 == 0
  const int64_t r0 = (int64_t)blockIdx.x * GQA_FOLD_ROWS;
  const int W = H + 2 * Hkv;
  const int64_t part = rows * 2 * Hkv;
  float cs = 0.f;
#pragma unroll 4
  for (int i = 0; i < GQA_FOLD_ROWS; ++i) {
    const float* p = slab + (r0 + i) * 2 * Hkv + c;
    float v = p[0];
    for (int j = 1; j < split; ++j) v += p[j * part];
    dqkv[(r0 + i) * W + H + c] = (__bf16)v;
    cs += v;
  }
  if (dbias) atomicAdd(dbias + H + c, cs);
}

// ---- entries ----------------------------------------------------------------
// The split rule: how many parts the G heads of a group are cut into for the
// dK/dV launch.  Host-only, a pure function of its arguments.  The base design
// (1) launches B * n_kv * Sq/64 blocks, G times fewer than the dense kernel.
// A grid that already gives every CU a block keeps 1.  An underfilled grid
// takes the smallest divisor of G that fills the two blocks per CU the
// kernel's registers admit (G if none does): at (2, 16, 1, 2048) on 256 CUs,
// 64 blocks, that is 8, measured at 337 us for the whole backward against
// 1369 at split 1, 437 at 4 and 340 at 16 (profiles/flash_gqa_probe.log,
// DESIGN.md item 25, which also has the filled-grid case).
extern "C" int ob_flash_gqa_split(int64_t B, int64_t Sq, int64_t nh,
                                  int64_t n_kv, int64_t cus) {
  if (B <= 0 || Sq <= 0 || nh <= 0 || n_kv <= 0 || nh % n_kv) return 1;
  const int64_t G = nh / n_kv, blocks = B * n_kv * (Sq / 64);
  if (blocks >= cus) return 1;
  for (int64_t s = 1; s <= G; ++s)
    if (G % s == 0 && blocks * s >= 2 * cus) return (int)s;
  return (int)G;
}

static int gqa_cus() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount,
                              dev) != hipSuccess)
      return 0;
    return v;
  }();
  return n;
}

// the checks of both entries, made before any launch; 0, or 1 with ob_fail set
static int gqa_args_ok(const char* who, int64_t B, int64_t Sq, int64_t H,
                       int64_t nh, int64_t n_kv) {
  if (B <= 0 || Sq <= 0 || H <= 0 || nh <= 0 || n_kv <= 0)
    return ob_fail("%s: sizes must be positive", who);
  if (H % nh || H / nh != 128)
    return ob_fail("%s: head_dim must be 128", who);
  if (n_kv > nh || nh % n_kv)
    return ob_fail("%s: n_head must be a multiple of n_kv", who);
  if (Sq % 128) return ob_fail("%s: S must be a multiple of 128", who);
  return 0;
}

extern "C" int ob_flash_fwd_gqa_bf16(const void* qkv, void* O, void* lse,
                                     int64_t B, int64_t Sq, int64_t H,
                                     int64_t nh, int64_t n_kv, float scale,
                                     void* stream) {
  if (gqa_args_ok("flash_fwd_gqa", B, Sq, H, nh, n_kv)) return 1;
  if (n_kv == nh)  // the layouts coincide
    return ob_flash_fwd_nt_bf16(qkv, O, lse, B, Sq, H, nh, scale, stream);
  const int Z = (int)(B * nh);
  k_flash_fwd_gqa<<<ob_fold_grid(ob_fold_q_nblk((int)Sq), Z), 256, 0,
                    S(stream)>>>((const __bf16*)qkv, (__bf16*)O, (float*)lse,
                                 (int)Sq, (int)H, (int)nh, (int)n_kv, Z,
                                 scale);
  OB_LAUNCH_CHECK();
  return 0;
}

// dq first (forms D from O and dO into D_ws), then dkdv, then the fold of a
// split launch
extern "C" int ob_flash_bwd_gqa_d_bf16(
    const void* qkv, const void* O, const void* dO, const void* lse,
    void* D_ws, void* dqkv, void* dbias_qkv, int64_t B, int64_t Sq, int64_t H,
    int64_t nh, int64_t n_kv, int64_t split, void* slab, int64_t slab_floats,
    float scale, void* stream) {
  const char* who = "flash_bwd_gqa_d";
  if (gqa_args_ok(who, B, Sq, H, nh, n_kv)) return 1;
  const int64_t G = nh / n_kv, Hkv = 128 * n_kv;
  if (split < 0 || (split > 0 && G % split))
    return ob_fail("%s: split must be 0 or a divisor of n_head / n_kv", who);
  if (n_kv == nh)
    return ob_flash_bwd_nt_d_bf16(qkv, O, dO, lse, D_ws, dqkv, dbias_qkv, B,
                                  Sq, H, nh, scale, stream);
  const int64_t part = B * Sq * 2 * Hkv;  // floats of one part's slab
  if (split == 0) {
    // the rule, lowered to what the caller's slab holds
    split = ob_flash_gqa_split(B, Sq, nh, n_kv, gqa_cus());
    while (split > 1 && (G % split || !slab || slab_floats < split * part))
      --split;
  } else if (split > 1 && (!slab || slab_floats < split * part)) {
    return ob_fail("%s: slab too small: split %lld needs %lld floats", who,
                   (long long)split, (long long)(split * part));
  }
  const int Z = (int)(B * nh);
  k_flash_bwd_dq_gqa<<<ob_fold_grid(ob_fold_q_nblk((int)Sq), Z), 256, 0,
                       S(stream)>>>(
      (const __bf16*)qkv, (const __bf16*)dO, (const float*)lse,
      (const __bf16*)O, (float*)D_ws, (__bf16*)dqkv, (float*)dbias_qkv,
      (int)Sq, (int)H, (int)nh, (int)n_kv, Z, scale);
  OB_LAUNCH_CHECK();
  const unsigned gk =
      ob_fold_grid(ob_fold_kv_nblk((int)Sq), (int)(B * n_kv * split));
  if (split == 1) {
    k_flash_bwd_dkdv_gqa<false><<<gk, 256, 0, S(stream)>>>(
        (const __bf16*)qkv, (const __bf16*)dO, (const float*)lse,
        (const float*)D_ws, (__bf16*)dqkv, (float*)dbias_qkv, nullptr, (int)B,
        (int)Sq, (int)H, (int)nh, (int)n_kv, 1, scale);
    OB_LAUNCH_CHECK();
    return 0;
  }
  k_flash_bwd_dkdv_gqa<true><<<gk, 256, 0, S(stream)>>>(
      (const __bf16*)qkv, (const __bf16*)dO, (const float*)lse,
      (const float*)D_ws, nullptr, nullptr, (float*)slab, (int)B, (int)Sq,
      (int)H, (int)nh, (int)n_kv, (int)split, scale);
  OB_LAUNCH_CHECK();
  k_gqa_fold<<<dim3((unsigned)(B * Sq / GQA_FOLD_ROWS),
                    (unsigned)(2 * Hkv / 256)),
               256, 0, S(stream)>>>((const float*)slab, (__bf16*)dqkv,
                                    (float*)dbias_qkv, B * Sq, (int)H,
                                    (int)Hkv, (int)split);
  OB_LAUNCH_CHECK();
  return 0;
}
