// ob_flash_hd128_bf16.hip — fused causal flash attention, bf16, head_dim 128
// (DESIGN.md §8 item 17).  The second head size of the production "nt"
// family of ob_flash_bf16.hip: forward, dQ (optionally forming D) and dK/dV,
// reached through the same public entries (ob_flash_fwd_nt_bf16,
// ob_flash_bwd_nt_bf16, ob_flash_bwd_nt_d_bf16), which dispatch on H / nh.
//
// Same arithmetic definition as the hd-64 kernels — swapped QK^T (a lane
// owns one q column), online softmax with the defer-max skip, LSE of the
// scaled scores, backward recomputed from Q, K and LSE, dS = P*(dP - D),
// `scale` folded in the same places, dbias from the fp32 accumulators after
// `scale` — and the same block -> work map (ob_flash_fold.h, unchanged).
// What differs is the d extent: 8 k-steps per QK^T / dP chain instead of 4,
// 4 output accumulators (32-column d quarters) instead of 2, and the LDS
// image below.  All three kernels are bound to 2 waves/SIMD (256 VGPRs);
// none uses scratch (profiles/flash_hd128_resources.txt).
//
// Out of scope: attention dropout at head_dim 128 (ob_flash_*_nt_drop_bf16
// keep rejecting it; such a layer takes the materialized route), transposed-
// operand twins (torch is the reference: tests/test_gpu_flash_hd128.py),
// head_dim 80/96, fp32 flash.
//
// LDS image of a [rows][128] bf16 tile (256-byte rows = one full sweep of
// the 64 banks, sixteen 16-byte chunks):
//   chunk ch of row r lives at chunk slot  ch ^ key(r),
//   key(r) = (r&3)<<2 | ((r>>2)&3).
// A row's bank position no longer depends on the row, so the hd-64 key
// (which leans on two rows per sweep) does not carry over.
//  * transposed read, one 32-lane half = rows r0..r0+3 (r0 % 4 == 0) x one
//    aligned group of 4 chunks 4c..4c+3: slot bits 3:2 are c ^ (r&3), one
//    value per row; bits 1:0 are the chunk's low bits ^ ((r>>2)&3), a
//    permutation inside the group -> 16 distinct slots, conflict-free.
//  * ds_read_b128 row read (lane il -> row il, one chunk index per half):
//    its 16-lane groups hold rows {0-3,12-15,20-27} / {4-11,16-19,28-31};
//    each is four aligned runs of 4 rows whose (r>>2)&3 are 0,3,1,2 /
//    1,2,0,3, and inside a run r&3 takes 0..3 -> key takes all 16 values,
//    conflict-free.
// key has period 16 in r, so rows 16 apart share a swizzle and the staging
// and row-read offsets of a thread differ by constants.
// The transposed read needs EXEC all ones and 8-byte-aligned lane
// addresses: every call below sits under wave-uniform control only.
#include "ob_flash_common.h"
#include "ob_internal.h"
#include "ob_flash_fold.h"

#include <cmath>

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

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

// Forward: k_flash_fwd_nt's structure (4 waves x 32 q rows, the two folded
// 64-row halves, KVBLK 64, K/V double-buffered in LDS, one barrier per
// tile).  Q is 8 fragments, O four accumulators; the PV B fragments are
// read one d quarter at a time (16 VGPRs per k-step, not 64 for a tile).
// LDS: 2 x (16 KB K + 16 KB V) + bcast = 64.5 KB, two blocks per CU.
__global__ __launch_bounds__(256, 2) void k_flash_fwd_hd128(
    const __bf16* __restrict__ qkv, __bf16* __restrict__ Obase,
    float* __restrict__ lse, int Sq, int H, int nh, int Z, float scale) {
  __shared__ __attribute__((aligned(16))) __bf16 kbuf[2][64 * 128];
  __shared__ __attribute__((aligned(16))) __bf16 vbuf[2][64 * 128];
  __shared__ float bcast[128];
  int blk, z;
  if (!ob_fold_id(blockIdx.x, ob_fold_q_nblk(Sq), Z, &blk, &z))
    return;  // block-uniform: grid padding
  const int b = z / nh, h = z % nh;
  const int64_t qoff = (int64_t)b * Sq * 3 * H + h * 128;
  const __bf16* Qp = qkv + qoff;
  const __bf16* Kp = Qp + H;
  const __bf16* Vp = Qp + 2 * H;
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
          Kp + (int64_t)(kv0 + sr + 16 * i) * 3 * H + sc * 8);
      vr[i] = *reinterpret_cast<const bf16x8*>(
          Vp + (int64_t)(kv0 + sr + 16 * i) * 3 * H + sc * 8);
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
    qf[s] = *reinterpret_cast<const bf16x8*>(
        Qp + (int64_t)myq * 3 * H + s * 16 + kh * 8);

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

// dK/dV: k_flash_bwd_dkdv_nt's split-duty wave pairs (role 0: K resident,
// S -> P -> dV; role 1: V resident, dP -> dS -> dK; only P crosses the
// pair, through xch) over 32-row q tiles of 128 columns.  Each role holds 8
// resident fragments, 4 output accumulators and the 8 B fragments (2
// k-slabs x 4 d quarters) it reads before the iteration's barrier: after it
// a fast wave already stages tile qt+2 into this buffer.
// LDS: xch 16 KB + 2 x (8 KB Q + 8 KB dO) + red 2 KB = 50 KB.
__global__ __launch_bounds__(256, 2) void k_flash_bwd_dkdv_hd128(
    const __bf16* __restrict__ qkv, const __bf16* __restrict__ dO,
    const float* __restrict__ lse, const float* __restrict__ D,
    __bf16* __restrict__ dqkv, float* __restrict__ dbias, int Sq, int H,
    int nh, int Z, float scale) {
  __shared__ float xch[2][2][32 * 32];  // [buffer][pair][P tile]
  __shared__ __attribute__((aligned(16))) __bf16 qbuf[2][32 * 128];
  __shared__ __attribute__((aligned(16))) __bf16 obuf[2][32 * 128];
  __shared__ float red[4 * 128];
  int blk, z;
  if (!ob_fold_id(blockIdx.x, ob_fold_kv_nblk(Sq), Z, &blk, &z))
    return;  // block-uniform: grid padding
  const int b = z / nh, h = z % nh;
  const int64_t base = (int64_t)b * Sq * 3 * H + h * 128;
  const __bf16* Qp = qkv + base;
  const __bf16* Kp = Qp + H;
  const __bf16* Vp = Qp + 2 * H;
  const __bf16* dOp = dO + (int64_t)b * Sq * H + h * 128;
  const float* lsep = lse + (int64_t)z * Sq;
  const float* Dp = D + (int64_t)z * Sq;

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
    of[s] = *reinterpret_cast<const bf16x8*>(
        KV + (int64_t)mykv * 3 * H + s * 16 + kh * 8);

  // staging: thread covers chunk tid&15 of rows tid>>4 and (tid>>4) + 16
  const int srow = tid >> 4, schunk = tid & 15;
  const int so = hd_off(srow, schunk);
  auto stage = [&](int buf, int q0s) {
    bf16x8 qr[2], dr[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      qr[i] = *reinterpret_cast<const bf16x8*>(
          Qp + (int64_t)(q0s + srow + 16 * i) * 3 * H + schunk * 8);
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
  stage(qt0 & 1, qt0 * 32);
  __syncthreads();

  for (int qt = qt0; qt < nqt; ++qt) {
    const int q0 = qt * 32;
    if (qt + 1 < nqt) stage((qt + 1) & 1, q0 + 32);
    // wave-uniform: pair 1 idles (staging and the barrier only) until the
    // loop reaches its diagonal, q0 + 31 >= kv0.  Each wave meets exactly
    // one barrier per iteration on either side of the branch.
    if (qt < myqt0) {
      __syncthreads();
      continue;
    }
    // own tile's A image, and the B image: role 0 multiplies P^T by dO,
    // role 1 dS^T by Q
    const __bf16* ab = role ? obuf[qt & 1] : qbuf[qt & 1];
    const __bf16* bb = role ? qbuf[qt & 1] : obuf[qt & 1];
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
      const bf16x8 af =
          *reinterpret_cast<const bf16x8*>(&ab[hd_off(il, ch)]);
      own = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, of[s], own, 0, 0,
                                                    0);
    }
    float pv[16];
    float* ptile = xch[qt & 1][pair];
    if (role == 0) {
      const float lse_t = lsep[q0 + il];
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
      const float d_t = Dp[q0 + il];
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

  __bf16* outp = dqkv + base + (role ? H : 2 * H);  // dK or dV slice
  const float os = role ? scale : 1.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int kv = kv0 + acc_row(r, kh);
#pragma unroll
    for (int d = 0; d < 4; ++d)
      outp[(int64_t)kv * 3 * H + 32 * d + il] = (__bf16)(os * acc[d][r]);
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
      atomicAdd(dbias + (rl ? H : 2 * H) + h * 128 + c,
                red[rl * 128 + c] + red[(2 + rl) * 128 + c]);
    }
  }
}

// dQ: k_flash_bwd_dq_nt's structure (the forward's blocks and K/V staging;
// S^T, P^T, dP^T, dS^T, dQ += dS K with K^T read column-wise from the K
// tile).  With Q and dO resident (16 fragments) and 4 dQ accumulators the
// hd-64 kernel's two concurrent S/dP chain pairs would not fit 256 VGPRs,
// so the two 32-row kv sub-tiles of a tile run one after the other: one S,
// one dP and 16 dS values live at a time.  The sums keep the hd-64 order
// (k-slabs 0..3 of the tile).
// kFormD: D[q] = sum_d dO[q,d] * O[q,d] is formed from the resident dO
// fragments and O loaded in the same layout, used, and written to Dout for
// the dkdv launch that follows.
// LDS: 2 x (16 KB K + 16 KB V) + red 2 KB = 66 KB.
template <bool kFormD>
__global__ __launch_bounds__(256, 2) void k_flash_bwd_dq_hd128(
    const __bf16* __restrict__ qkv, const __bf16* __restrict__ dO,
    const float* __restrict__ lse, const float* __restrict__ D,
    const __bf16* __restrict__ O, float* __restrict__ Dout,
    __bf16* __restrict__ dqkv, float* __restrict__ dbias, int Sq, int H,
    int nh, int Z, float scale) {
  __shared__ __attribute__((aligned(16))) __bf16 kbuf[2][64 * 128];
  __shared__ __attribute__((aligned(16))) __bf16 vbuf[2][64 * 128];
  __shared__ float red[4 * 128];
  int blk, z;
  if (!ob_fold_id(blockIdx.x, ob_fold_q_nblk(Sq), Z, &blk, &z))
    return;  // block-uniform: grid padding
  const int b = z / nh, h = z % nh;
  const int64_t base = (int64_t)b * Sq * 3 * H + h * 128;
  const __bf16* Qp = qkv + base;
  const __bf16* Kp = Qp + H;
  const __bf16* Vp = Qp + 2 * H;
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
    qf[s] = *reinterpret_cast<const bf16x8*>(
        Qp + (int64_t)myq * 3 * H + s * 16 + kh * 8);
    df[s] = *reinterpret_cast<const bf16x8*>(
        dOp + (int64_t)myq * H + s * 16 + kh * 8);
  }
  float myD;
  if constexpr (kFormD) {
    const __bf16* Orow =
        O + (int64_t)b * Sq * H + h * 128 + (int64_t)myq * H;
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
  } else {
    myD = D[(int64_t)z * Sq + myq];
  }

  // staging: thread covers chunk tid&15 of rows (tid>>4) + 16i, i = 0..3
  const int sr = tid >> 4, sc = tid & 15;
  const int so = hd_off(sr, sc);
  auto stage = [&](int buf, int kv0) {
    bf16x8 kr[4], vr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      kr[i] = *reinterpret_cast<const bf16x8*>(
          Kp + (int64_t)(kv0 + sr + 16 * i) * 3 * H + sc * 8);
      vr[i] = *reinterpret_cast<const bf16x8*>(
          Vp + (int64_t)(kv0 + sr + 16 * i) * 3 * H + sc * 8);
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
      dQp[(int64_t)q * 3 * H + 32 * d + il] = (__bf16)(scale * dq[d][r]);
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

int ob_flash_hd128_fwd(const void* qkv, void* O, void* lse, int64_t B,
                       int64_t Sq, int64_t H, int64_t nh, float scale,
                       void* stream) {
  const int Z = (int)(B * nh);
  k_flash_fwd_hd128<<<ob_fold_grid(ob_fold_q_nblk((int)Sq), Z), 256, 0,
                      S(stream)>>>((const __bf16*)qkv, (__bf16*)O,
                                   (float*)lse, (int)Sq, (int)H, (int)nh, Z,
                                   scale);
  OB_LAUNCH_CHECK();
  return 0;
}

int ob_flash_hd128_bwd(const void* qkv, const void* O, const void* dO,
                       const void* lse, void* D, void* dqkv, void* dbias_qkv,
                       int64_t B, int64_t Sq, int64_t H, int64_t nh,
                       float scale, void* stream) {
  const int Z = (int)(B * nh);
  const unsigned gq = ob_fold_grid(ob_fold_q_nblk((int)Sq), Z);
  // dq first: with O given it forms the D the dkdv launch reads
  if (O)
    k_flash_bwd_dq_hd128<true><<<gq, 256, 0, S(stream)>>>(
        (const __bf16*)qkv, (const __bf16*)dO, (const float*)lse, nullptr,
        (const __bf16*)O, (float*)D, (__bf16*)dqkv, (float*)dbias_qkv,
        (int)Sq, (int)H, (int)nh, Z, scale);
  else
    k_flash_bwd_dq_hd128<false><<<gq, 256, 0, S(stream)>>>(
        (const __bf16*)qkv, (const __bf16*)dO, (const float*)lse,
        (const float*)D, nullptr, nullptr, (__bf16*)dqkv, (float*)dbias_qkv,
        (int)Sq, (int)H, (int)nh, Z, scale);
  OB_LAUNCH_CHECK();
  k_flash_bwd_dkdv_hd128<<<ob_fold_grid(ob_fold_kv_nblk((int)Sq), Z), 256, 0,
                           S(stream)>>>(
      (const __bf16*)qkv, (const __bf16*)dO, (const float*)lse,
      (const float*)D, (__bf16*)dqkv, (float*)dbias_qkv, (int)Sq, (int)H,
      (int)nh, Z, scale);
  OB_LAUNCH_CHECK();
  return 0;
}
