// ob_flash_bf16.hip — fused causal flash attention, bf16, head_dim = 64
// (SURVEY.md "hard part (i)").  The public
// nt entries live here and dispatch on H / nh: the head_dim 128 kernels are
// ob_flash_hd128_bf16.hip (item 17), the helpers both files use
// ob_flash_common.h.
//
// Two families of the same three kernels (forward, dK/dV, dQ):
//   1. production: k_flash_fwd_nt / k_flash_bwd_dkdv_nt / k_flash_bwd_dq_nt
//      (ob_flash_fwd_nt_bf16, ob_flash_bwd_nt_bf16 and, with D formed in
//      the dq kernel, ob_flash_bwd_nt_d_bf16), plus k_flash_dsum; their
//      kDrop instantiations apply attention dropout in registers
//      (ob_flash_fwd_nt_drop_bf16, ob_flash_bwd_nt_d_drop_bf16);
//   2. their transposed-operand twins k_flash_fwd_bf16_v4 /
//      k_flash_bwd_dkdv_s / k_flash_bwd_dq_v3 (ob_flash_fwd_bf16,
//      ob_flash_bwd_bf16) fed by k_transpose_bf16_b — the reference of the
//      bit-for-bit tests and the OB_FLASH_TR=0 path; see the section header.
//
// v_mfma_f32_32x32x16_bf16 fragment layout the kernels rely on (pinned by
// tests/test_gpu_bf16.py; ob_gemm_bf16.hip derives it), il = lane&31,
// kh = lane>>5:
//   A: lane holds A[i = il][k = 8*kh + j], j = 0..7 (one ds_read_b128 of a
//      [row][k] image)
//   B: lane holds B[k = 8*kh + j][n = il]
//   C/D: col = il, row = acc_row(r, kh) = (r&3) + 8*(r>>2) + 4*kh
//
// Which rows a production block owns and which linear block id is which
// (head, block) is ob_flash_fold.h: a block takes a
// light and a heavy piece of the causal triangle so all blocks of a launch
// cost the same, and the blocks of one head get ids of one XCD so they share
// its L2.  The twins keep the plain map (blockIdx.x = tile, blockIdx.z =
// head); a wave's arithmetic does not depend on the map, so the two
// families stay bit-identical (tests/test_gpu_flash_fold.py).
//
// Forward: per (b, h) blocks of 4 waves, each wave owns 32 q rows (twins:
// one 128-row q-tile; production: two 64-row halves, ob_flash_fold.h).
// QK^T is computed SWAPPED (mfma(A=K, B=Q)) so each lane holds the
// scores of ONE q column (q = il, 16 kv rows per accumulator) — the
// online-softmax row reduce is lane-local + one shfl_xor(32) partner
// combine.  P converts to the PV A-fragment with 8 pack-to-bf16 ops + 2
// permlane32_swap per k-step (bf_dance: the kh halves exchange
// kv{4..7}/{8..11} exactly as the fragment k-runs need).  O accumulates in
// fp32; per-tile rescale factors broadcast wave-locally through LDS.
// Writes O (bf16) and the per-row LSE (fp32) for the backward recompute.
//
// Backward (recompute from Q, K, LSE; no stored P):
//   D[z][q]   = sum_d dO[q,d] * O[q,d]     (k_flash_dsum; in production
//               the dq kernel forms it: ob_flash_bwd_nt_d_bf16)
//   dKdV      : blocks own 64 kv rows, loop q-tiles:
//               S = QK^T (acc col = kv), P = exp(scale*S - lse[q]),
//               dP = dO V^T-free (mfma(dO, V)), dS = P*(dP - D[q]),
//               dV += P^T dO (B operand = dO^T), dK += scale * dS^T Q
//               (B operand = Q^T)
//   dQ        : blocks own 128 q rows, loop kv-tiles (fwd orientation):
//               S^T, P^T, dP^T (mfma(V, dO)), dS^T, dQ += scale*dS K
//               (B operand = K^T)
// The B operands V^T / dO^T / Q^T / K^T are k-contiguous only in a
// transposed copy: the production kernels read them column-wise from the
// row-major LDS tile, the twins from materialized [z][64][S] transposes.
//
// Why these structures (measurements: profiles/r02_flash_probe.log,
// profiles/r02_flash_sq_counters.log, profiles/r01_*): operand tiles are
// staged in LDS and shared by the block's waves because per-wave global
// fragment loads leave load latency on the critical path, and register
// prefetch alone only turns those stalls into dependency stalls; blocks are
// 4 waves because the per-tile barrier makes a block wait for its longest
// causal diagonal.
#include "ob_bf16.h"
#include "ob_flash_common.h"
#include "ob_internal.h"
#include "ob_flash_fold.h"
#include "ob_philox.h"

#include <cmath>

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

// ===========================================================================
// Production: the "nt" flash kernels — no materialized V^T / Q^T / K^T /
// dO^T.  The MFMA B operand that needs a transposed view is read
// column-wise from the row-major LDS tile the kernel stages anyway, with
// gfx950's ds_read_b64_tr_b16 (a 16-lane group reads a 4-row x 16-column
// block and receives it column-major).  Each kernel has a twin in the
// second section that takes that operand from a transposed copy instead;
// MFMA order and operand values are the same, so the outputs are
// bit-identical to ob_flash_fwd_bf16 / ob_flash_bwd_bf16
// (tests/test_gpu_flash_nt.py).
//
// LDS image of a [rows][64] bf16 tile (128-byte rows, 16-byte chunks):
//   chunk ch of row r lives at chunk slot  ch ^ key(r),
//   key(r) = ((r>>1)&1)<<2 | ((r>>2)&3).
// Bank = (byte/4) % 64, i.e. 256 B = two rows per bank sweep.
//  * transposed read, one 32-lane half = rows r0..r0+3 (r0 % 4 == 0) x one
//    aligned group of 4 chunks: rows r and r+1 differ in byte bit 7, rows
//    r and r+2 differ in key bit 2 (the other 64 B of the row); the low
//    key bits only permute chunks inside the group -> 16 distinct 16-B
//    slots of the 256-B sweep, conflict-free.  (The twins' image,
//    key = r&7, puts rows r and r+2 in the same slots: 2-way.)
//  * ds_read_b128 row read (lane il -> row il, one chunk index per half):
//    its 16-lane groups {0-3,12-15,20-27} / {4-11,16-19,28-31} hold 8 even
//    and 8 odd rows each; over either set key(r) takes all 8 values ->
//    conflict-free (key = r&7 repeats every 8 rows: 2-way in these groups).
// The transposed read needs EXEC all ones and 8-byte-aligned lane
// addresses: every call below sits under wave-uniform control only.
// ===========================================================================
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

// Attention dropout (kDrop instantiations).  The mask
// is ob_philox.h's, site OB_DROP_ATTN: element e = (z*S + q)*S + kv of the
// full [B*nh, S, S] square, word e & 3 of ob_drop_words(key, e >> 2), and
// ob_drop_factor's rule (word >= thr keeps, kept values times key.scale).
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
// = keep of sub-tile u, element r.  8 calls per lane and 64-kv tile, in a
// rolled loop: unrolled, their temporaries push the kernels into scratch.
__device__ __forceinline__ uint32_t drop_crow(int z, int Sq, int q, int kh) {
  return (uint32_t)(z * Sq + q) * (uint32_t)(Sq >> 2) + (uint32_t)kh;
}
__device__ __forceinline__ uint32_t drop_bits_q(const ob_drop_key& key,
                                                uint32_t crow) {
  uint32_t bits = 0;
#pragma unroll 1
  for (int i = 0; i < 8; ++i) {  // i = 4u + g
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

// Forward: 4 waves x 32 q-rows = 128 q-rows per block; KVBLK = 64.
//   * K and V tiles STAGED IN LDS, double-buffered, shared by the 4 waves
//     (two coalesced 16 B chunks per thread and tile instead of each wave's
//     redundant global fragment loads), swizzled for conflict-free
//     ds_read_b128 A-fragments.
//   * two independent S chains (kv sub-tiles) per tile + tree reductions
//     instead of serial fmax/sum chains: with the loads covered the loop
//     is dependency-bound (profiles/r02_flash_sq_counters.log).
//   * one barrier per tile: tile t+1 is staged into the buffer whose
//     readers finished at the previous barrier.
//   * 128 q-rows per block, not 256: the per-tile barrier makes every wave
//     wait for the block's longest causal diagonal, and 4 waves halve that
//     spread (57 vs 71.5 us at the step shape).
//   * the 128 rows are the 64-row halves a and n64-1-a (ob_flash_fold.h):
//     waves 0,1 go inactive after the light half's diagonal and only stage
//     and barrier from there on.
//   * the O rescale is skipped while no row's max grows by more than 8;
//     tiles wholly below the diagonal skip the causal mask.
// vbuf is staged from V rows like kbuf from K rows; the PV B fragments are
// its columns.
// kDrop: m, l and the stored LSE come from the undropped P (the backward
// recomputes P from them); PV multiplies Pd = P * factor, formed in fp32
// before bf_dance packs it.  `key` is unused without kDrop.
template <bool kDrop>
__global__ __launch_bounds__(256, 3) void k_flash_fwd_nt(
    const __bf16* __restrict__ qkv, __bf16* __restrict__ Obase,
    float* __restrict__ lse, int Sq, int H, int nh, int Z, float scale,
    ob_drop_key key) {
  __shared__ __attribute__((aligned(16))) __bf16 kbuf[2][64 * 64];
  __shared__ __attribute__((aligned(16))) __bf16 vbuf[2][64 * 64];
  __shared__ float bcast[128];
  int blk, z;
  if (!ob_fold_id(blockIdx.x, ob_fold_q_nblk(Sq), Z, &blk, &z))
    return;  // block-uniform: grid padding
  const int b = z / nh, h = z % nh;
  const int64_t qoff = (int64_t)b * Sq * 3 * H + h * 64;
  const __bf16* Qp = qkv + qoff;
  const __bf16* Kp = Qp + H;
  const __bf16* Vp = Qp + 2 * H;
  __bf16* Op = Obase + (int64_t)b * Sq * H + h * 64;
  float* lsep = lse + (int64_t)z * Sq;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int il = lane & 31, kh = lane >> 5;
  const int q0 = ob_fold_q_row0(Sq, blk, w);
  const int myq = q0 + il;
  const int mytiles = ob_fold_q_wave_tiles(q0);

  // staging: thread covers chunks tid and tid+256 of the 512-slot tile
  const int sr0 = tid >> 3, sr1 = sr0 + 32, sc = tid & 7;
  const int so0 = nt_off(sr0, sc), so1 = nt_off(sr1, sc);
  auto stage = [&](int buf, int kv0) {
    *reinterpret_cast<bf16x8*>(&kbuf[buf][so0]) =
        *reinterpret_cast<const bf16x8*>(
            Kp + (int64_t)(kv0 + sr0) * 3 * H + sc * 8);
    *reinterpret_cast<bf16x8*>(&kbuf[buf][so1]) =
        *reinterpret_cast<const bf16x8*>(
            Kp + (int64_t)(kv0 + sr1) * 3 * H + sc * 8);
    *reinterpret_cast<bf16x8*>(&vbuf[buf][so0]) =
        *reinterpret_cast<const bf16x8*>(
            Vp + (int64_t)(kv0 + sr0) * 3 * H + sc * 8);
    *reinterpret_cast<bf16x8*>(&vbuf[buf][so1]) =
        *reinterpret_cast<const bf16x8*>(
            Vp + (int64_t)(kv0 + sr1) * 3 * H + sc * 8);
  };

  bf16x8 qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
    qf[s] = *reinterpret_cast<const bf16x8*>(
        Qp + (int64_t)myq * 3 * H + s * 16 + kh * 8);

  const int ntiles = ob_fold_q_block_tiles(Sq, blk);  // block-uniform
  stage(0, 0);
  __syncthreads();

  f32x16 o0 = {}, o1 = {};
  float m = -INFINITY, l = 0.f;
  for (int kvt = 0; kvt < ntiles; ++kvt) {
    const int kv0 = kvt * 64;
    // drawn (by the waves still active) before the staging loads take
    // their registers
    [[maybe_unused]] uint32_t keep = 0;
    if constexpr (kDrop)
      if (kvt < mytiles)
        keep = drop_bits_q(key, drop_crow(z, Sq, myq, kh) + (kv0 >> 2));
    if (kvt + 1 < ntiles) stage((kvt + 1) & 1, kv0 + 64);
    const bool active = kvt < mytiles;  // kv0 <= q0 + 31, wave-uniform
    if (active) {
      const __bf16* kb = kbuf[kvt & 1];
      const __bf16* vb = vbuf[kvt & 1];
      f32x16 sacc0 = {}, sacc1 = {};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int ch = (s * 2 + kh);
        const bf16x8 ka =
            *reinterpret_cast<const bf16x8*>(&kb[nt_off(il, ch)]);
        const bf16x8 kb2 =
            *reinterpret_cast<const bf16x8*>(&kb[nt_off(32 + il, ch)]);
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
          const int kvr = kv0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
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
          const float a = bcast[w * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh];
          o0[r] *= a;
          o1[r] *= a;
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
      if constexpr (kDrop) {
#pragma unroll
        for (int r = 0; r < 32; ++r) sv[r] *= drop_factor_bit(key, keep, r);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const bf16x8 pa = bf_dance(sv + t * 8);
        // B[k = kv 16t+8kh..+7][n = d]: columns of the row-major V tile
        const bf16x8 v0f = nt_tr_frag(vb, lane, t * 16 + kh * 8, 0);
        const bf16x8 v1f = nt_tr_frag(vb, lane, t * 16 + kh * 8, 1);
        o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa, v0f, o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa, v1f, o1, 0, 0, 0);
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
    const int row = (r & 3) + 8 * (r >> 2) + 4 * kh;
    const float inv = bcast[w * 32 + row];
    Op[(int64_t)(q0 + row) * H + il] = (__bf16)(o0[r] * inv);
    Op[(int64_t)(q0 + row) * H + 32 + il] = (__bf16)(o1[r] * inv);
  }
}

// head size of the nt entries: 64 (the kernels of this file) or 128
// (ob_flash_hd128_bf16.hip); 0 with ob_fail set for anything else
static int nt_head_dim(const char* who, int64_t H, int64_t nh) {
  if (nh <= 0 || H % nh) {
    ob_fail("%s: n_embd must be a multiple of n_head", who);
    return 0;
  }
  const int64_t hd = H / nh;
  if (hd != 64 && hd != 128) {
    ob_fail("%s: head_dim must be 64 or 128", who);
    return 0;
  }
  return (int)hd;
}

extern "C" int ob_flash_fwd_nt_bf16(const void* qkv, void* O, void* lse,
                                    int64_t B, int64_t Sq, int64_t H,
                                    int64_t nh, float scale, void* stream) {
  const int hd = nt_head_dim("flash_fwd_nt", H, nh);
  if (!hd) return 1;
  if (Sq % 128) return ob_fail("flash_fwd_nt: S must be a multiple of 128");
  if (hd == 128)
    return ob_flash_hd128_fwd(qkv, O, lse, B, Sq, H, nh, scale, stream);
  const int Z = (int)(B * nh);
  k_flash_fwd_nt<false><<<ob_fold_grid(ob_fold_q_nblk((int)Sq), Z), 256, 0,
                          S(stream)>>>((const __bf16*)qkv, (__bf16*)O,
                                       (float*)lse, (int)Sq, (int)H, (int)nh,
                                       Z, scale, ob_drop_key{});
  OB_LAUNCH_CHECK();
  return 0;
}

// shape and key checks shared by the two dropout entries
static int drop_args_ok(const char* who, int64_t B, int64_t Sq, int64_t H,
                        int64_t nh, float p) {
  // attention dropout exists at head_dim 64 only
  if (nh <= 0 || H % nh || H / nh != 64)
    return ob_fail("%s: head_dim must be 64", who);
  if (Sq <= 0 || Sq % 128)
    return ob_fail("%s: S must be a multiple of 128", who);
  if (!ob_drop_p_ok(p)) return ob_fail("%s: p must be in [0,1)", who);
  if (B <= 0 || B * nh * Sq * Sq > ((int64_t)1 << 34))
    return ob_fail("%s: B*nh*S*S exceeds the 2^34 mask elements", who);
  return 0;
}

// ob_flash_fwd_nt_bf16 with attention dropout (site OB_DROP_ATTN) applied
// to P before PV; p == 0 is the plain kernel.
extern "C" int ob_flash_fwd_nt_drop_bf16(const void* qkv, void* O, void* lse,
                                         int64_t B, int64_t Sq, int64_t H,
                                         int64_t nh, float scale,
                                         uint64_t seed, int32_t layer_id,
                                         uint64_t tick, float p,
                                         void* stream) {
  if (drop_args_ok("flash_fwd_nt_drop", B, Sq, H, nh, p)) return 1;
  if (p == 0.f)
    return ob_flash_fwd_nt_bf16(qkv, O, lse, B, Sq, H, nh, scale, stream);
  const int Z = (int)(B * nh);
  k_flash_fwd_nt<true><<<ob_fold_grid(ob_fold_q_nblk((int)Sq), Z), 256, 0,
                         S(stream)>>>(
      (const __bf16*)qkv, (__bf16*)O, (float*)lse, (int)Sq, (int)H, (int)nh,
      Z, scale, ob_drop_make_key(seed, layer_id, OB_DROP_ATTN, tick, p));
  OB_LAUNCH_CHECK();
  return 0;
}

// dK/dV: split-duty wave pairs.  A block owns 64 kv rows, a WAVE PAIR one
// 32-kv-row tile; each loops over the q-tiles from its diagonal down.
//   role 0: K resident, owns the whole P chain: S -> P -> BOTH d-halves of dV
//   role 1: V resident, owns the whole dS chain: dP -> dS -> BOTH d-halves
//           of dK
// One wave holding K+V residents, the S and dP accumulators and both
// d-halves of dV and dK needs 217 VGPRs (2 waves/SIMD); a pair member holds
// half of that and runs at 3 waves/SIMD.  Only P crosses the pair, through
// double-buffered LDS (one-way, layout-preserving: lane L element r of role
// 0 is exactly what lane L element r of role 1 multiplies), role 1 skips
// the exp + causal mask entirely (masked P is already 0), and each wave
// runs HALF the lse/D shuffle fan-out: 208.6 us whole-backward vs 231.2
// for pairs that exchange both S and dP (profiles/r02_flash_probe.log).
// The block's pairs own the kv tiles x and n32-1-x (ob_flash_fold.h); the
// q loop starts at pair 0's diagonal and pair 1 idles, staging and
// meeting the barrier only, until the loop reaches its own.  (The twin's
// pair 1 instead spends one masked, all-zero tile above its diagonal.)
// Q and dO tiles (the A fragments, read before the exchange barrier) are
// staged in LDS once per block, double-buffered under that ONE barrier per
// q-tile.  The dV/dK B operands (dO^T for role 0, Q^T for role 1) are
// column reads of the same obuf/qbuf tile of the current q-tile.  The reads
// stay BEFORE the iteration's barrier: after it a fast wave already stages
// tile qt+2 into this buffer.
// dbias (fp32 [3H], may be null): += column sums of this block's dK and dV
// tiles, taken from the fp32 accumulators after `scale`, before rounding.
// kDrop: dV accumulates Pd^T dO, dK accumulates dS^T Q with
// dS = P * (factor*dP - D).  Role 0 draws the mask and hands it to role 1
// inside the P exchange, as the sign bit of the fp32 P it writes to xch
// (P >= 0; a dropped P goes out negative): no extra LDS, no second Philox.
// Role 0 feeds dV with keep ? P*scale : 0; role 1 reads |x| as P and the
// sign as the keep bit.  Here a lane holds ONE kv column and 16 q rows, so
// the four lanes of a quad (il & ~3) need the same 16 Philox calls, one per
// q row, and each lane uses word il & 3 of every one.  Lane j of the quad
// makes the 4 calls of rows r = 4g + j, packs the 16 keep bits (bit
// 4g + word) and the quad exchanges the packed registers: a quarter of the
// Philox work of every lane drawing its own 16 calls, which measured 387 us
// against 280 us for the whole backward at (8, 12, 1024)
// (profiles/flash_drop_probe.log).
// Launch bound: the kDrop instantiation is bound to 2 waves/SIMD.  The
// plain body already sits at 167 VGPRs, most of them hoisted per-lane row
// and exchange addresses; with the mask on top the compiler takes 211, and
// under bound 3 it spills the dV/dK B fragments across the exchange instead
// (76 B/lane of scratch and more).
template <bool kDrop>
__global__ __launch_bounds__(256, kDrop ? 2 : 3) void k_flash_bwd_dkdv_nt(
    const __bf16* __restrict__ qkv, const __bf16* __restrict__ dO,
    const float* __restrict__ lse, const float* __restrict__ D,
    __bf16* __restrict__ dqkv, float* __restrict__ dbias, int Sq, int H,
    int nh, int Z, float scale, ob_drop_key key) {
  __shared__ float xch[2][2][32 * 32];  // [buffer][pair][P tile]
  __shared__ __attribute__((aligned(16))) __bf16 qbuf[2][32 * 64];
  __shared__ __attribute__((aligned(16))) __bf16 obuf[2][32 * 64];
  __shared__ float red[4 * 64];
  int blk, z;
  if (!ob_fold_id(blockIdx.x, ob_fold_kv_nblk(Sq), Z, &blk, &z))
    return;  // block-uniform: grid padding
  const int b = z / nh, h = z % nh;
  const int64_t base = (int64_t)b * Sq * 3 * H + h * 64;
  const __bf16* Qp = qkv + base;
  const __bf16* Kp = Qp + H;
  const __bf16* Vp = Qp + 2 * H;
  const __bf16* dOp = dO + (int64_t)b * Sq * H + h * 64;
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
  [[maybe_unused]] const uint32_t sq4 = (uint32_t)(Sq >> 2);

  const __bf16* KV = role ? Vp : Kp;
  bf16x8 of[4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
    of[s] = *reinterpret_cast<const bf16x8*>(
        KV + (int64_t)mykv * 3 * H + s * 16 + kh * 8);

  const int srow = tid >> 3, schunk = tid & 7;
  const int so = nt_off(srow, schunk);
  auto stage = [&](int buf, int q0s) {
    *reinterpret_cast<bf16x8*>(&qbuf[buf][so]) =
        *reinterpret_cast<const bf16x8*>(
            Qp + (int64_t)(q0s + srow) * 3 * H + schunk * 8);
    *reinterpret_cast<bf16x8*>(&obuf[buf][so]) =
        *reinterpret_cast<const bf16x8*>(
            dOp + (int64_t)(q0s + srow) * H + schunk * 8);
  };

  f32x16 acc0 = {}, acc1 = {};  // role 0: dV d-halves; role 1: dK d-halves
  const int nqt = Sq / 32;
  const int qt0 = ob_fold_kv_block_first(blk);  // block-uniform
  stage(qt0 & 1, qt0 * 32);
  __syncthreads();

  for (int qt = qt0; qt < nqt; ++qt) {
    const int q0 = qt * 32;
    // bit r: keep of element r (q row q0 + acc_row(r, kh), column mykv);
    // drawn by role 0 before the staging loads take their registers
    [[maybe_unused]] uint32_t keep = 0;
    if constexpr (kDrop) {
      if (role == 0 && qt >= myqt0) {  // wave-uniform
        // Philox counter of q row q0 + 4*kh at this lane's kv quad
        const uint32_t c0 = (uint32_t)(z * Sq + q0 + 4 * kh) * sq4 +
                            (uint32_t)(mykv >> 2);
        uint32_t mine = 0;  // rows r = 4g + (il & 3): bit 4g + word
#pragma unroll
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
    // B-operands early (before the barrier): both d-halves, k = q rows
    const bf16x8 b00 = nt_tr_frag(bb, lane, kh * 8, 0);
    const bf16x8 b01 = nt_tr_frag(bb, lane, kh * 8, 1);
    const bf16x8 b10 = nt_tr_frag(bb, lane, 16 + kh * 8, 0);
    const bf16x8 b11 = nt_tr_frag(bb, lane, 16 + kh * 8, 1);
    // own tile: S (role 0, A = Q rows) or dP (role 1, A = dO rows)
    f32x16 own = {};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int ch = s * 2 + kh;
      const bf16x8 af =
          *reinterpret_cast<const bf16x8*>(&ab[nt_off(il, ch)]);
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
        if constexpr (kDrop) {
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
        if constexpr (kDrop) {
          // dS = P * (factor*dP - D): |x| is P, a set sign bit says dropped
          const float x = ptile[qoff * 32 + il];
          const float f = __builtin_signbit(x) ? 0.f : key.scale;
          pv[r] = __builtin_fabsf(x) * (f * own[r] - d_q);
        } else {
          // dS = P * (dP - D); masked entries have P == 0 already
          pv[r] = ptile[qoff * 32 + il] * (own[r] - d_q);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const bf16x8 a = bf_dance(pv + t * 8);
      const bf16x8 bl = t ? b10 : b00;
      const bf16x8 bh = t ? b11 : b01;
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bl, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bh, acc1, 0, 0, 0);
    }
  }

  __bf16* outp = dqkv + base + (role ? H : 2 * H);  // dK or dV slice
  const float os = role ? scale : 1.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int kv = kv0 + acc_row(r, kh);
    outp[(int64_t)kv * 3 * H + il] = (__bf16)(os * acc0[r]);
    outp[(int64_t)kv * 3 * H + 32 + il] = (__bf16)(os * acc1[r]);
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

// dQ: the forward's structure applied to the dQ loop — blocks of 4 waves
// own 128 q rows; K and V tiles STAGED IN LDS (double-buffered, swizzled,
// shared by the 4 waves), KVBLK=64 with two independent S/dP chain pairs,
// in-lane masking.  One barrier per kv tile; stage-writes target the
// buffer whose readers finished before the previous barrier.  The dQ B
// operand (K^T) is kt0/kt1 = column reads of the K tile the S chains
// already use (LDS 32 KB; the twin's separate K^T tile makes it 48 KB).
// dbias (fp32 [3H], may be null): += column sums of this block's dQ tile.
// Bound 3 (not the twin's 2): the twin compiles to 167 VGPRs and so
// already runs 3 waves/SIMD; this body came to 169 under bound 2, which
// would have dropped it to 2.
// kFormD: D is not an input.  Each wave forms D[q] = sum_d dO[q,d] * O[q,d]
// of its 32 rows from the dO fragments it holds anyway and O loaded in the
// same layout, uses it, and writes it to Dout for the dkdv launch that
// follows.  A lane holds the 8-element chunks 2s + kh of its row; the sum
// is taken in k_flash_dsum's order (chunk sums left to right, then
// ((c0+c4)+(c2+c6)) + ((c1+c5)+(c3+c7))), so D is bit-identical to that
// kernel's: the bf16 x bf16 products are exact in fp32, so contraction to
// fma cannot move a bit either.
// kDrop: D = rowsum(dO * O) is unchanged (sum_k P_k m_k dPd_k = dO . O
// when O = Pd V); dP = factor * (V . dO) and dS = P * (dP - D) with the
// undropped P.  Mask bits as in the forward.
template <bool kFormD, bool kDrop>
__global__ __launch_bounds__(256, 3) void k_flash_bwd_dq_nt(
    const __bf16* __restrict__ qkv, const __bf16* __restrict__ dO,
    const float* __restrict__ lse, const float* __restrict__ D,
    const __bf16* __restrict__ O, float* __restrict__ Dout,
    __bf16* __restrict__ dqkv, float* __restrict__ dbias, int Sq, int H,
    int nh, int Z, float scale, ob_drop_key key) {
  __shared__ __attribute__((aligned(16))) __bf16 kbuf[2][64 * 64];
  __shared__ __attribute__((aligned(16))) __bf16 vbuf[2][64 * 64];
  __shared__ float red[4 * 64];
  int blk, z;
  if (!ob_fold_id(blockIdx.x, ob_fold_q_nblk(Sq), Z, &blk, &z))
    return;  // block-uniform: grid padding
  const int b = z / nh, h = z % nh;
  const int64_t base = (int64_t)b * Sq * 3 * H + h * 64;
  const __bf16* Qp = qkv + base;
  const __bf16* Kp = Qp + H;
  const __bf16* Vp = Qp + 2 * H;
  const __bf16* dOp = dO + (int64_t)b * Sq * H + h * 64;
  const float* lsep = lse + (int64_t)z * Sq;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int il = lane & 31, kh = lane >> 5;
  const int q0 = ob_fold_q_row0(Sq, blk, w);
  const int myq = q0 + il;
  const int mytiles = ob_fold_q_wave_tiles(q0);
  const float mylse = lsep[myq];

  bf16x8 qf[4], df[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    qf[s] = *reinterpret_cast<const bf16x8*>(
        Qp + (int64_t)myq * 3 * H + s * 16 + kh * 8);
    df[s] = *reinterpret_cast<const bf16x8*>(
        dOp + (int64_t)myq * H + s * 16 + kh * 8);
  }
  float myD;
  if constexpr (kFormD) {
    const __bf16* Orow = O + (int64_t)b * Sq * H + h * 64 + (int64_t)myq * H;
    float cs[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const bf16x8 ov =
          *reinterpret_cast<const bf16x8*>(Orow + s * 16 + kh * 8);
      float c = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) c += bf2f(ov[j]) * bf2f(df[s][j]);
      cs[s] = c;
    }
    // cs[s] = chunk 2s + kh: this half's bracket, then the other half's
    const float part = (cs[0] + cs[2]) + (cs[1] + cs[3]);
    myD = part + __shfl_xor(part, 32, 64);
    if (kh == 0) Dout[(int64_t)z * Sq + myq] = myD;
  } else {
    myD = D[(int64_t)z * Sq + myq];
  }

  // staging map: 256 threads x 2 rows each (row r and r+32), 16 B chunks
  const int srow = tid >> 3, schunk = tid & 7;  // rows 0..31
  const int so0 = nt_off(srow, schunk), so1 = nt_off(srow + 32, schunk);
  auto stage = [&](int buf, int kv0) {
    *reinterpret_cast<bf16x8*>(&kbuf[buf][so0]) =
        *reinterpret_cast<const bf16x8*>(
            Kp + (int64_t)(kv0 + srow) * 3 * H + schunk * 8);
    *reinterpret_cast<bf16x8*>(&kbuf[buf][so1]) =
        *reinterpret_cast<const bf16x8*>(
            Kp + (int64_t)(kv0 + srow + 32) * 3 * H + schunk * 8);
    *reinterpret_cast<bf16x8*>(&vbuf[buf][so0]) =
        *reinterpret_cast<const bf16x8*>(
            Vp + (int64_t)(kv0 + srow) * 3 * H + schunk * 8);
    *reinterpret_cast<bf16x8*>(&vbuf[buf][so1]) =
        *reinterpret_cast<const bf16x8*>(
            Vp + (int64_t)(kv0 + srow + 32) * 3 * H + schunk * 8);
  };

  const int ntiles = ob_fold_q_block_tiles(Sq, blk);  // block-uniform
  stage(0, 0);
  __syncthreads();

  f32x16 dq0 = {}, dq1 = {};
  for (int kvt = 0; kvt < ntiles; ++kvt) {
    const int kv0 = kvt * 64;
    // drawn (by the waves still active) before the staging loads take
    // their registers
    [[maybe_unused]] uint32_t keep = 0;
    if constexpr (kDrop)
      if (kvt < mytiles)
        keep = drop_bits_q(key, drop_crow(z, Sq, myq, kh) + (kv0 >> 2));
    if (kvt + 1 < ntiles) stage((kvt + 1) & 1, kv0 + 64);
    // wave-uniform causal skip: kv0 <= q0 + 31
    const bool active = kvt < mytiles;
    if (active) {
      const __bf16* kb = kbuf[kvt & 1];
      const __bf16* vb = vbuf[kvt & 1];
      // two kv sub-tiles: independent S and dP chains
      f32x16 s0 = {}, s1 = {}, p0 = {}, p1 = {};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int ch = s * 2 + kh;
        const bf16x8 ka =
            *reinterpret_cast<const bf16x8*>(&kb[nt_off(il, ch)]);
        const bf16x8 kb2 =
            *reinterpret_cast<const bf16x8*>(&kb[nt_off(32 + il, ch)]);
        const bf16x8 va =
            *reinterpret_cast<const bf16x8*>(&vb[nt_off(il, ch)]);
        const bf16x8 vb2 =
            *reinterpret_cast<const bf16x8*>(&vb[nt_off(32 + il, ch)]);
        s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qf[s], s0, 0, 0, 0);
        s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kb2, qf[s], s1, 0, 0,
                                                     0);
        p0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, df[s], p0, 0, 0, 0);
        p1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vb2, df[s], p1, 0, 0,
                                                     0);
      }
      float dsv[32];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kv = kv0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        const bool ok0 = kv <= myq;
        const bool ok1 = kv + 32 <= myq;
        const float pa = ok0 ? __expf(s0[r] * scale - mylse) : 0.f;
        const float pb = ok1 ? __expf(s1[r] * scale - mylse) : 0.f;
        if constexpr (kDrop) {
          const float f0 = drop_factor_bit(key, keep, r);
          const float f1 = drop_factor_bit(key, keep, 16 + r);
          dsv[r] = ok0 ? pa * (f0 * p0[r] - myD) : 0.f;
          dsv[16 + r] = ok1 ? pb * (f1 * p1[r] - myD) : 0.f;
        } else {
          dsv[r] = ok0 ? pa * (p0[r] - myD) : 0.f;
          dsv[16 + r] = ok1 ? pb * (p1[r] - myD) : 0.f;
        }
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
    }
    __syncthreads();
  }
  __bf16* dQp = dqkv + base;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int q = q0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
    dQp[(int64_t)q * 3 * H + il] = (__bf16)(scale * dq0[r]);
    dQp[(int64_t)q * 3 * H + 32 + il] = (__bf16)(scale * dq1[r]);
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

template <bool kDrop>
static int launch_dkdv_nt(const void* qkv, const void* dO, const void* lse,
                          const void* D, void* dqkv, void* dbias_qkv,
                          int64_t B, int64_t Sq, int64_t H, int64_t nh,
                          float scale, const ob_drop_key& key, void* stream) {
  const int Z = (int)(B * nh);
  k_flash_bwd_dkdv_nt<kDrop>
      <<<ob_fold_grid(ob_fold_kv_nblk((int)Sq), Z), 256, 0, S(stream)>>>(
          (const __bf16*)qkv, (const __bf16*)dO, (const float*)lse,
          (const float*)D, (__bf16*)dqkv, (float*)dbias_qkv, (int)Sq, (int)H,
          (int)nh, Z, scale, key);
  OB_LAUNCH_CHECK();
  return 0;
}

extern "C" int ob_flash_bwd_nt_bf16(const void* qkv, const void* dO,
                                    const void* lse, const void* D,
                                    void* dqkv, void* dbias_qkv, int64_t B,
                                    int64_t Sq, int64_t H, int64_t nh,
                                    float scale, void* stream) {
  const int hd = nt_head_dim("flash_bwd_nt", H, nh);
  if (!hd) return 1;
  if (Sq % 128) return ob_fail("flash_bwd_nt: S must be a multiple of 128");
  if (hd == 128)
    return ob_flash_hd128_bwd(qkv, nullptr, dO, lse, const_cast<void*>(D),
                              dqkv, dbias_qkv, B, Sq, H, nh, scale, stream);
  if (launch_dkdv_nt<false>(qkv, dO, lse, D, dqkv, dbias_qkv, B, Sq, H, nh,
                            scale, ob_drop_key{}, stream))
    return 1;
  const int Z = (int)(B * nh);
  k_flash_bwd_dq_nt<false, false>
      <<<ob_fold_grid(ob_fold_q_nblk((int)Sq), Z), 256, 0, S(stream)>>>(
          (const __bf16*)qkv, (const __bf16*)dO, (const float*)lse,
          (const float*)D, nullptr, nullptr, (__bf16*)dqkv,
          (float*)dbias_qkv, (int)Sq, (int)H, (int)nh, Z, scale,
          ob_drop_key{});
  OB_LAUNCH_CHECK();
  return 0;
}

// The backward without a separate D pass: dq first (forms D from O and dO,
// writes it to D_ws), then dkdv, which reads D_ws.
extern "C" int ob_flash_bwd_nt_d_bf16(const void* qkv, const void* O,
                                      const void* dO, const void* lse,
                                      void* D_ws, void* dqkv,
                                      void* dbias_qkv, int64_t B, int64_t Sq,
                                      int64_t H, int64_t nh, float scale,
                                      void* stream) {
  const int hd = nt_head_dim("flash_bwd_nt_d", H, nh);
  if (!hd) return 1;
  if (Sq % 128) return ob_fail("flash_bwd_nt_d: S must be a multiple of 128");
  if (hd == 128)
    return ob_flash_hd128_bwd(qkv, O, dO, lse, D_ws, dqkv, dbias_qkv, B, Sq,
                              H, nh, scale, stream);
  const int Z = (int)(B * nh);
  k_flash_bwd_dq_nt<true, false>
      <<<ob_fold_grid(ob_fold_q_nblk((int)Sq), Z), 256, 0, S(stream)>>>(
          (const __bf16*)qkv, (const __bf16*)dO, (const float*)lse, nullptr,
          (const __bf16*)O, (float*)D_ws, (__bf16*)dqkv, (float*)dbias_qkv,
          (int)Sq, (int)H, (int)nh, Z, scale, ob_drop_key{});
  OB_LAUNCH_CHECK();
  return launch_dkdv_nt<false>(qkv, dO, lse, D_ws, dqkv, dbias_qkv, B, Sq, H,
                               nh, scale, ob_drop_key{}, stream);
}

// ob_flash_bwd_nt_d_bf16 for a forward that ran ob_flash_fwd_nt_drop_bf16
// with the same key; p == 0 is the plain backward.
extern "C" int ob_flash_bwd_nt_d_drop_bf16(
    const void* qkv, const void* O, const void* dO, const void* lse,
    void* D_ws, void* dqkv, void* dbias_qkv, int64_t B, int64_t Sq, int64_t H,
    int64_t nh, float scale, uint64_t seed, int32_t layer_id, uint64_t tick,
    float p, void* stream) {
  if (drop_args_ok("flash_bwd_nt_d_drop", B, Sq, H, nh, p)) return 1;
  if (p == 0.f)
    return ob_flash_bwd_nt_d_bf16(qkv, O, dO, lse, D_ws, dqkv, dbias_qkv, B,
                                  Sq, H, nh, scale, stream);
  const ob_drop_key key =
      ob_drop_make_key(seed, layer_id, OB_DROP_ATTN, tick, p);
  const int Z = (int)(B * nh);
  k_flash_bwd_dq_nt<true, true>
      <<<ob_fold_grid(ob_fold_q_nblk((int)Sq), Z), 256, 0, S(stream)>>>(
          (const __bf16*)qkv, (const __bf16*)dO, (const float*)lse, nullptr,
          (const __bf16*)O, (float*)D_ws, (__bf16*)dqkv, (float*)dbias_qkv,
          (int)Sq, (int)H, (int)nh, Z, scale, key);
  OB_LAUNCH_CHECK();
  return launch_dkdv_nt<true>(qkv, dO, lse, D_ws, dqkv, dbias_qkv, B, Sq, H,
                              nh, scale, key, stream);
}

// Host-only queries of the ob_flash_fold.h mapping (no GPU call), for the
// tests.  kind: 0 forward, 1 dq, 2 dkdv.
// ob_flash_fold_rows: unit = wave (0..3; forward, dq) or wave pair (0..1;
// dkdv) -> its first row (it owns 32) and the tiles it computes; unit = -1
// -> the tiles the block stages (row0 = -1).  Tiles are 64-row kv tiles for
// forward and dq, 32-row q tiles for dkdv.
extern "C" int ob_flash_fold_rows(int64_t kind, int64_t Sq, int64_t block,
                                  int64_t unit, int64_t* row0,
                                  int64_t* first_tile, int64_t* n_tiles) {
  if (Sq <= 0 || Sq % 128) return ob_fail("fold_rows: S must be a multiple of 128");
  const int S_ = (int)Sq, blk = (int)block;
  if (kind == OB_FOLD_FWD || kind == OB_FOLD_DQ) {
    if (blk < 0 || blk >= ob_fold_q_nblk(S_) || unit < -1 || unit > 3)
      return ob_fail("fold_rows: block/unit out of range");
    *first_tile = 0;
    if (unit < 0) {
      *row0 = -1;
      *n_tiles = ob_fold_q_block_tiles(S_, blk);
    } else {
      *row0 = ob_fold_q_row0(S_, blk, (int)unit);
      *n_tiles = ob_fold_q_wave_tiles((int)*row0);
    }
    return 0;
  }
  if (kind == OB_FOLD_DKDV) {
    if (blk < 0 || blk >= ob_fold_kv_nblk(S_) || unit < -1 || unit > 1)
      return ob_fail("fold_rows: block/unit out of range");
    if (unit < 0) {
      *row0 = -1;
      *first_tile = ob_fold_kv_block_first(blk);
    } else {
      *row0 = ob_fold_kv_row0(S_, blk, (int)unit);
      *first_tile = ob_fold_kv_pair_first((int)*row0);
    }
    *n_tiles = S_ / 32 - *first_tile;
    return 0;
  }
  return ob_fail("fold_rows: unknown kind");
}

static int fold_nblk(int64_t kind, int64_t Sq) {
  return kind == OB_FOLD_DKDV ? ob_fold_kv_nblk((int)Sq)
                              : ob_fold_q_nblk((int)Sq);
}

// blocks in the launch of `kind` for Z = B*nh heads (padding included)
extern "C" int64_t ob_flash_fold_grid(int64_t kind, int64_t Sq, int64_t Z) {
  return (int64_t)ob_fold_grid(fold_nblk(kind, Sq), (int)Z);
}

// linear block id -> (z, block); returns 1, or 0 for a padding id
extern "C" int ob_flash_fold_id(int64_t kind, int64_t Sq, int64_t Z,
                                int64_t id, int64_t* z, int64_t* block) {
  int blk, zz;
  const bool ok =
      ob_fold_id((unsigned)id, fold_nblk(kind, Sq), (int)Z, &blk, &zz);
  *z = zz;
  *block = blk;
  return ok ? 1 : 0;
}

// D[z][q] = sum_d dO[q,d] * O[q,d]: runs before either backward family.
// HD = 64: the kernel as it always was.  HD = 128: 16 lanes per row.
template <int HD>
__global__ __launch_bounds__(256) void k_flash_dsum(
    const __bf16* __restrict__ O, const __bf16* __restrict__ dO,
    float* __restrict__ D, int Sq, int H, int nh) {
  // 8 lanes x 8 elements (uint4) per row, 32 rows per block — the
  // one-lane-per-element version's 2-B loads measured 3x off roofline
  const int z = blockIdx.z;
  const int b = z / nh, h = z % nh;
  constexpr int LPR = HD / 8;  // lanes per row
  const int row = blockIdx.x * (256 / LPR) + (threadIdx.x / LPR);
  if (row >= Sq) return;
  const int l8 = threadIdx.x & (LPR - 1);
  const int64_t off =
      (int64_t)b * Sq * H + (int64_t)row * H + h * HD + l8 * 8;
  const uint4 ov = *reinterpret_cast<const uint4*>(O + off);
  const uint4 dv = *reinterpret_cast<const uint4*>(dO + off);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    s += bf2f(bf_extract(ov, j)) * bf2f(bf_extract(dv, j));
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if (l8 == 0) D[(int64_t)z * Sq + row] = s;
}

extern "C" int ob_flash_dsum_bf16(const void* O, const void* dO, void* D,
                                  int64_t B, int64_t Sq, int64_t H, int64_t nh,
                                  void* stream) {
  if (nh > 0 && H == 128 * nh) {
    dim3 grid((unsigned)((Sq + 15) / 16), 1, (unsigned)(B * nh));
    k_flash_dsum<128><<<grid, 256, 0, S(stream)>>>(
        (const __bf16*)O, (const __bf16*)dO, (float*)D, (int)Sq, (int)H,
        (int)nh);
    OB_LAUNCH_CHECK();
    return 0;
  }
  dim3 grid((unsigned)((Sq + 31) / 32), 1, (unsigned)(B * nh));
  k_flash_dsum<64><<<grid, 256, 0, S(stream)>>>(
      (const __bf16*)O, (const __bf16*)dO, (float*)D, (int)Sq, (int)H,
      (int)nh);
  OB_LAUNCH_CHECK();
  return 0;
}

// ===========================================================================
// Transposed-operand twins: k_flash_fwd_bf16_v4, k_flash_bwd_dkdv_s and
// k_flash_bwd_dq_v3, fed by k_transpose_bf16_b.  They are
//   * the reference tests/test_gpu_flash_nt.py compares the production
//     kernels against, element for element and over a whole layer;
//   * the OB_FLASH_TR=0 path of ob_layer.hip.
// Each is its production kernel above, minus the dbias epilogue, with the
// B operand that needs a transposed view taken from a materialized
// [z][64][S] copy (V^T; Q^T and dO^T; K^T) and the LDS image keyed
// chunk ^ (row & 7).  A change to a production kernel's arithmetic is made
// here too, or the bit-for-bit tests fail.
// ===========================================================================

// batched strided transpose: out[z][C][R] = in[z-slice][R][C] where the
// input slice z starts at in + (z/n2)*sIn1 + (z%n2)*sIn2 — two-level (b,h)
// strides like the GEMMs.  Materializes V^T and the backward's
// Q^T/K^T/dO^T.
__global__ __launch_bounds__(256) void k_transpose_bf16_b(
    const __bf16* __restrict__ in, __bf16* __restrict__ out, int64_t R,
    int64_t C, int64_t sIn1, int64_t sIn2, int64_t ldin, int n2) {
  __shared__ __bf16 tile[64 * 65];
  const int z = blockIdx.z;
  const int i1 = z / n2, i2 = z % n2;
  const __bf16* src = in + (int64_t)i1 * sIn1 + (int64_t)i2 * sIn2;
  __bf16* dst = out + (int64_t)z * R * C;
  const int64_t r0 = (int64_t)blockIdx.y * 64, c0 = (int64_t)blockIdx.x * 64;
  {
    const int rr = threadIdx.x >> 3;
    const int c8 = (threadIdx.x & 7) * 8;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int r = rr + it * 32;
      uint4 v = {0, 0, 0, 0};
      if (r0 + r < R && c0 + c8 + 7 < C)
        v = *reinterpret_cast<const uint4*>(src + (r0 + r) * ldin + c0 + c8);
#pragma unroll
      for (int j = 0; j < 8; ++j) tile[r * 65 + c8 + j] = bf_extract(v, j);
    }
  }
  __syncthreads();
  {
    const int cc = threadIdx.x >> 3;
    const int r8 = (threadIdx.x & 7) * 8;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int c = cc + it * 32;
      if (c0 + c >= C) continue;
      float tmp[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        tmp[j] = bf2f(tile[(r8 + j) * 65 + c]);
      if (r0 + r8 + 7 < R)
        *reinterpret_cast<uint4*>(dst + (c0 + c) * R + r0 + r8) =
            bf_pack8(tmp);
    }
  }
}

extern "C" int ob_transpose_bf16_b(const void* in, void* out, int64_t R,
                                   int64_t C, int64_t sIn1, int64_t sIn2,
                                   int64_t ldin, int64_t n1, int64_t n2,
                                   void* stream) {
  if (R % 64 || C % 64) return ob_fail("transpose_b: R,C must be 64-multiples");
  dim3 grid((unsigned)((C + 63) / 64), (unsigned)((R + 63) / 64),
            (unsigned)(n1 * n2));
  k_transpose_bf16_b<<<grid, 256, 0, S(stream)>>>(
      (const __bf16*)in, (__bf16*)out, R, C, sIn1, sIn2, ldin, (int)n2);
  OB_LAUNCH_CHECK();
  return 0;
}

// k_flash_fwd_nt with vbuf staged from the V^T copy ([d 64][kv 64] tile):
// v0f/v1f are ds_read_b128 row reads of it.
__global__ __launch_bounds__(256, 3) void k_flash_fwd_bf16_v4(
    const __bf16* __restrict__ qkv, const __bf16* __restrict__ VT,
    __bf16* __restrict__ Obase, float* __restrict__ lse, int Sq, int H,
    int nh, float scale) {
  __shared__ __bf16 kbuf[2][64 * 64];
  __shared__ __bf16 vbuf[2][64 * 64];
  __shared__ float bcast[128];
  const int z = blockIdx.z;
  const int b = z / nh, h = z % nh;
  const int64_t qoff = (int64_t)b * Sq * 3 * H + h * 64;
  const __bf16* Qp = qkv + qoff;
  const __bf16* Kp = Qp + H;
  const __bf16* VTp = VT + (int64_t)z * 64 * Sq;
  __bf16* Op = Obase + (int64_t)b * Sq * H + h * 64;
  float* lsep = lse + (int64_t)z * Sq;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int il = lane & 31, kh = lane >> 5;
  const int q0b = blockIdx.x * 128;
  const int q0 = q0b + w * 32;
  const int myq = q0 + il;

  // staging: thread covers chunks tid and tid+256 of the 512-slot tile
  const int sr0 = tid >> 3, sc0 = tid & 7;
  const int sr1 = (tid + 256) >> 3, sc1 = (tid + 256) & 7;
  const int sw0 = sc0 ^ (sr0 & 7), sw1 = sc1 ^ (sr1 & 7);
  auto stage = [&](int buf, int kv0) {
    *reinterpret_cast<bf16x8*>(&kbuf[buf][sr0 * 64 + sw0 * 8]) =
        *reinterpret_cast<const bf16x8*>(
            Kp + (int64_t)(kv0 + sr0) * 3 * H + sc0 * 8);
    *reinterpret_cast<bf16x8*>(&kbuf[buf][sr1 * 64 + sw1 * 8]) =
        *reinterpret_cast<const bf16x8*>(
            Kp + (int64_t)(kv0 + sr1) * 3 * H + sc1 * 8);
    *reinterpret_cast<bf16x8*>(&vbuf[buf][sr0 * 64 + sw0 * 8]) =
        *reinterpret_cast<const bf16x8*>(
            VTp + (int64_t)sr0 * Sq + kv0 + sc0 * 8);
    *reinterpret_cast<bf16x8*>(&vbuf[buf][sr1 * 64 + sw1 * 8]) =
        *reinterpret_cast<const bf16x8*>(
            VTp + (int64_t)sr1 * Sq + kv0 + sc1 * 8);
  };

  bf16x8 qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
    qf[s] = *reinterpret_cast<const bf16x8*>(
        Qp + (int64_t)myq * 3 * H + s * 16 + kh * 8);

  const int ntiles = (q0b + 128) / 64;
  stage(0, 0);
  __syncthreads();

  f32x16 o0 = {}, o1 = {};
  float m = -INFINITY, l = 0.f;
  for (int kvt = 0; kvt < ntiles; ++kvt) {
    const int kv0 = kvt * 64;
    if (kvt + 1 < ntiles) stage((kvt + 1) & 1, kv0 + 64);
    const bool active = kv0 <= q0 + 31;
    if (active) {
      const __bf16* kb = kbuf[kvt & 1];
      const __bf16* vb = vbuf[kvt & 1];
      f32x16 sacc0 = {}, sacc1 = {};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int ch = (s * 2 + kh);
        const bf16x8 ka = *reinterpret_cast<const bf16x8*>(
            &kb[il * 64 + (ch ^ (il & 7)) * 8]);
        const bf16x8 kb2 = *reinterpret_cast<const bf16x8*>(
            &kb[(32 + il) * 64 + (ch ^ ((32 + il) & 7)) * 8]);
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
          const int kvr = kv0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
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
          const float a = bcast[w * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh];
          o0[r] *= a;
          o1[r] *= a;
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
        const int ch = t * 2 + kh;
        const bf16x8 v0f = *reinterpret_cast<const bf16x8*>(
            &vb[il * 64 + (ch ^ (il & 7)) * 8]);
        const bf16x8 v1f = *reinterpret_cast<const bf16x8*>(
            &vb[(32 + il) * 64 + (ch ^ ((32 + il) & 7)) * 8]);
        o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa, v0f, o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa, v1f, o1, 0, 0, 0);
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
    const int row = (r & 3) + 8 * (r >> 2) + 4 * kh;
    const float inv = bcast[w * 32 + row];
    Op[(int64_t)(q0 + row) * H + il] = (__bf16)(o0[r] * inv);
    Op[(int64_t)(q0 + row) * H + 32 + il] = (__bf16)(o1[r] * inv);
  }
}

extern "C" int ob_flash_fwd_bf16(const void* qkv, const void* VT, void* O,
                                 void* lse, int64_t B, int64_t Sq, int64_t H,
                                 int64_t nh, float scale, void* stream) {
  if (H / nh != 64) return ob_fail("flash_fwd: head_dim must be 64");
  if (Sq % 128) return ob_fail("flash_fwd: S must be a multiple of 128");
  dim3 grid((unsigned)(Sq / 128), 1, (unsigned)(B * nh));
  k_flash_fwd_bf16_v4<<<grid, 256, 0, S(stream)>>>(
      (const __bf16*)qkv, (const __bf16*)VT, (__bf16*)O, (float*)lse,
      (int)Sq, (int)H, (int)nh, scale);
  OB_LAUNCH_CHECK();
  return 0;
}

// k_flash_bwd_dkdv_nt with the dV/dK B operands b00..b11 loaded from the
// dO^T (role 0) / Q^T (role 1) copies in global memory at the top of the
// q-tile.  They stay register-held rather than LDS-staged: staging them
// too needs a second barrier per q-tile, which costs more than the shared
// loads save (302 vs 234 us whole-backward; DESIGN.md, round-2 negative
// results).
__global__ __launch_bounds__(256, 3) void k_flash_bwd_dkdv_s(
    const __bf16* __restrict__ qkv, const __bf16* __restrict__ QT,
    const __bf16* __restrict__ dOT, const __bf16* __restrict__ dO,
    const float* __restrict__ lse, const float* __restrict__ D,
    __bf16* __restrict__ dqkv, int Sq, int H, int nh, float scale) {
  __shared__ float xch[2][2][32 * 32];  // [buffer][pair][P tile]
  __shared__ __bf16 qbuf[2][32 * 64];
  __shared__ __bf16 obuf[2][32 * 64];
  const int z = blockIdx.z;
  const int b = z / nh, h = z % nh;
  const int64_t base = (int64_t)b * Sq * 3 * H + h * 64;
  const __bf16* Qp = qkv + base;
  const __bf16* Kp = Qp + H;
  const __bf16* Vp = Qp + 2 * H;
  const __bf16* dOp = dO + (int64_t)b * Sq * H + h * 64;
  const __bf16* QTp = QT + (int64_t)z * 64 * Sq;
  const __bf16* dOTp = dOT + (int64_t)z * 64 * Sq;
  const float* lsep = lse + (int64_t)z * Sq;
  const float* Dp = D + (int64_t)z * Sq;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int pair = w >> 1, role = w & 1;
  const int il = lane & 31, kh = lane >> 5;
  const int kv0 = blockIdx.x * 64 + pair * 32;
  const int mykv = kv0 + il;

  const __bf16* KV = role ? Vp : Kp;
  bf16x8 of[4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
    of[s] = *reinterpret_cast<const bf16x8*>(
        KV + (int64_t)mykv * 3 * H + s * 16 + kh * 8);

  const int srow = tid >> 3, schunk = tid & 7;
  const int swzq = schunk ^ (srow & 7);
  auto stage = [&](int buf, int q0s) {
    *reinterpret_cast<bf16x8*>(&qbuf[buf][srow * 64 + swzq * 8]) =
        *reinterpret_cast<const bf16x8*>(
            Qp + (int64_t)(q0s + srow) * 3 * H + schunk * 8);
    *reinterpret_cast<bf16x8*>(&obuf[buf][srow * 64 + swzq * 8]) =
        *reinterpret_cast<const bf16x8*>(
            dOp + (int64_t)(q0s + srow) * H + schunk * 8);
  };

  f32x16 acc0 = {}, acc1 = {};  // role 0: dV d-halves; role 1: dK d-halves
  const int nqt = Sq / 32;
  const int qt0 = (blockIdx.x * 64) / 32;
  stage(qt0 & 1, qt0 * 32);
  __syncthreads();

  for (int qt = qt0; qt < nqt; ++qt) {
    const int q0 = qt * 32;
    if (qt + 1 < nqt) stage((qt + 1) & 1, q0 + 32);
    // B-operands early: BOTH d-halves of this role's output operand
    const __bf16* Bp = role ? QTp : dOTp;
    const bf16x8 b00 = *reinterpret_cast<const bf16x8*>(
        Bp + (int64_t)il * Sq + q0 + kh * 8);
    const bf16x8 b01 = *reinterpret_cast<const bf16x8*>(
        Bp + (int64_t)(32 + il) * Sq + q0 + kh * 8);
    const bf16x8 b10 = *reinterpret_cast<const bf16x8*>(
        Bp + (int64_t)il * Sq + q0 + 16 + kh * 8);
    const bf16x8 b11 = *reinterpret_cast<const bf16x8*>(
        Bp + (int64_t)(32 + il) * Sq + q0 + 16 + kh * 8);
    // own tile: S (role 0, A = Q rows) or dP (role 1, A = dO rows)
    const __bf16* ab = role ? obuf[qt & 1] : qbuf[qt & 1];
    f32x16 own = {};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int ch = s * 2 + kh;
      const bf16x8 af = *reinterpret_cast<const bf16x8*>(
          &ab[il * 64 + (ch ^ (il & 7)) * 8]);
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
      const bf16x8 bl = t ? b10 : b00;
      const bf16x8 bh = t ? b11 : b01;
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bl, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bh, acc1, 0, 0, 0);
    }
  }

  __bf16* outp = dqkv + base + (role ? H : 2 * H);  // dK or dV slice
  const float os = role ? scale : 1.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int kv = kv0 + acc_row(r, kh);
    outp[(int64_t)kv * 3 * H + il] = (__bf16)(os * acc0[r]);
    outp[(int64_t)kv * 3 * H + 32 + il] = (__bf16)(os * acc1[r]);
  }
}

// k_flash_bwd_dq_nt with a third staged tile, tbuf = the K^T copy's
// [d 64][kv 64] tile: kt0/kt1 are ds_read_b128 row reads of it.
__global__ __launch_bounds__(256, 2) void k_flash_bwd_dq_v3(
    const __bf16* __restrict__ qkv, const __bf16* __restrict__ KT,
    const __bf16* __restrict__ dO, const float* __restrict__ lse,
    const float* __restrict__ D, __bf16* __restrict__ dqkv, int Sq, int H,
    int nh, float scale) {
  __shared__ __bf16 kbuf[2][64 * 64];
  __shared__ __bf16 vbuf[2][64 * 64];
  __shared__ __bf16 tbuf[2][64 * 64];  // K^T tile ([d 64][kv 64])
  const int z = blockIdx.z;
  const int b = z / nh, h = z % nh;
  const int64_t base = (int64_t)b * Sq * 3 * H + h * 64;
  const __bf16* Qp = qkv + base;
  const __bf16* Kp = Qp + H;
  const __bf16* Vp = Qp + 2 * H;
  const __bf16* dOp = dO + (int64_t)b * Sq * H + h * 64;
  const __bf16* KTp = KT + (int64_t)z * 64 * Sq;
  const float* lsep = lse + (int64_t)z * Sq;
  const float* Dp = D + (int64_t)z * Sq;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int il = lane & 31, kh = lane >> 5;
  const int q0 = blockIdx.x * 128 + w * 32;
  const int myq = q0 + il;
  const float mylse = lsep[myq];
  const float myD = Dp[myq];

  bf16x8 qf[4], df[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    qf[s] = *reinterpret_cast<const bf16x8*>(
        Qp + (int64_t)myq * 3 * H + s * 16 + kh * 8);
    df[s] = *reinterpret_cast<const bf16x8*>(
        dOp + (int64_t)myq * H + s * 16 + kh * 8);
  }

  // staging map: 256 threads x 2 rows each (row r and r+32), 16 B chunks
  const int srow = tid >> 3, schunk = tid & 7;  // rows 0..31
  const int swz0 = schunk ^ (srow & 7);
  const int swz1 = schunk ^ ((srow + 32) & 7);
  auto stage = [&](int buf, int kv0) {
    // K and V rows kv0+srow / kv0+srow+32; K^T rows d=srow / d=srow+32
    *reinterpret_cast<bf16x8*>(&kbuf[buf][srow * 64 + swz0 * 8]) =
        *reinterpret_cast<const bf16x8*>(
            Kp + (int64_t)(kv0 + srow) * 3 * H + schunk * 8);
    *reinterpret_cast<bf16x8*>(&kbuf[buf][(srow + 32) * 64 + swz1 * 8]) =
        *reinterpret_cast<const bf16x8*>(
            Kp + (int64_t)(kv0 + srow + 32) * 3 * H + schunk * 8);
    *reinterpret_cast<bf16x8*>(&vbuf[buf][srow * 64 + swz0 * 8]) =
        *reinterpret_cast<const bf16x8*>(
            Vp + (int64_t)(kv0 + srow) * 3 * H + schunk * 8);
    *reinterpret_cast<bf16x8*>(&vbuf[buf][(srow + 32) * 64 + swz1 * 8]) =
        *reinterpret_cast<const bf16x8*>(
            Vp + (int64_t)(kv0 + srow + 32) * 3 * H + schunk * 8);
    *reinterpret_cast<bf16x8*>(&tbuf[buf][srow * 64 + swz0 * 8]) =
        *reinterpret_cast<const bf16x8*>(
            KTp + (int64_t)srow * Sq + kv0 + schunk * 8);
    *reinterpret_cast<bf16x8*>(&tbuf[buf][(srow + 32) * 64 + swz1 * 8]) =
        *reinterpret_cast<const bf16x8*>(
            KTp + (int64_t)(srow + 32) * Sq + kv0 + schunk * 8);
  };

  const int ntiles = (blockIdx.x * 128 + 128) / 64;  // block-uniform
  stage(0, 0);
  __syncthreads();

  f32x16 dq0 = {}, dq1 = {};
  for (int kvt = 0; kvt < ntiles; ++kvt) {
    const int kv0 = kvt * 64;
    if (kvt + 1 < ntiles) stage((kvt + 1) & 1, kv0 + 64);
    const bool active = kv0 <= q0 + 31;  // wave-uniform causal skip
    if (active) {
      const __bf16* kb = kbuf[kvt & 1];
      const __bf16* vb = vbuf[kvt & 1];
      const __bf16* tb = tbuf[kvt & 1];
      // two kv sub-tiles: independent S and dP chains
      f32x16 s0 = {}, s1 = {}, p0 = {}, p1 = {};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int ch = s * 2 + kh;
        const bf16x8 ka = *reinterpret_cast<const bf16x8*>(
            &kb[il * 64 + (ch ^ (il & 7)) * 8]);
        const bf16x8 kb2 = *reinterpret_cast<const bf16x8*>(
            &kb[(32 + il) * 64 + (ch ^ ((32 + il) & 7)) * 8]);
        const bf16x8 va = *reinterpret_cast<const bf16x8*>(
            &vb[il * 64 + (ch ^ (il & 7)) * 8]);
        const bf16x8 vb2 = *reinterpret_cast<const bf16x8*>(
            &vb[(32 + il) * 64 + (ch ^ ((32 + il) & 7)) * 8]);
        s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qf[s], s0, 0, 0, 0);
        s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kb2, qf[s], s1, 0, 0,
                                                     0);
        p0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, df[s], p0, 0, 0, 0);
        p1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vb2, df[s], p1, 0, 0,
                                                     0);
      }
      float dsv[32];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kv = kv0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        const bool ok0 = kv <= myq;
        const bool ok1 = kv + 32 <= myq;
        const float pa = ok0 ? __expf(s0[r] * scale - mylse) : 0.f;
        const float pb = ok1 ? __expf(s1[r] * scale - mylse) : 0.f;
        dsv[r] = ok0 ? pa * (p0[r] - myD) : 0.f;
        dsv[16 + r] = ok1 ? pb * (p1[r] - myD) : 0.f;
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const bf16x8 da = bf_dance(dsv + t * 8);
        const int ch = t * 2 + kh;
        const bf16x8 kt0 = *reinterpret_cast<const bf16x8*>(
            &tb[il * 64 + (ch ^ (il & 7)) * 8]);
        const bf16x8 kt1 = *reinterpret_cast<const bf16x8*>(
            &tb[(32 + il) * 64 + (ch ^ ((32 + il) & 7)) * 8]);
        dq0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da, kt0, dq0, 0, 0, 0);
        dq1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da, kt1, dq1, 0, 0, 0);
      }
    }
    __syncthreads();
  }
  __bf16* dQp = dqkv + base;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int q = q0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
    dQp[(int64_t)q * 3 * H + il] = (__bf16)(scale * dq0[r]);
    dQp[(int64_t)q * 3 * H + 32 + il] = (__bf16)(scale * dq1[r]);
  }
}

extern "C" int ob_flash_bwd_bf16(const void* qkv, const void* QT,
                                 const void* KT, const void* dOT,
                                 const void* dO, const void* lse,
                                 const void* D, void* dqkv, int64_t B,
                                 int64_t Sq, int64_t H, int64_t nh,
                                 float scale, void* stream) {
  if (H / nh != 64) return ob_fail("flash_bwd: head_dim must be 64");
  if (Sq % 128) return ob_fail("flash_bwd: S must be a multiple of 128");
  dim3 gridp((unsigned)(Sq / 64), 1, (unsigned)(B * nh));
  k_flash_bwd_dkdv_s<<<gridp, 256, 0, S(stream)>>>(
      (const __bf16*)qkv, (const __bf16*)QT, (const __bf16*)dOT,
      (const __bf16*)dO, (const float*)lse, (const float*)D,
      (__bf16*)dqkv, (int)Sq, (int)H, (int)nh, scale);
  OB_LAUNCH_CHECK();
  dim3 grid((unsigned)(Sq / 128), 1, (unsigned)(B * nh));
  k_flash_bwd_dq_v3<<<grid, 256, 0, S(stream)>>>(
      (const __bf16*)qkv, (const __bf16*)KT, (const __bf16*)dO,
      (const float*)lse, (const float*)D, (__bf16*)dqkv, (int)Sq, (int)H,
      (int)nh, scale);
  OB_LAUNCH_CHECK();
  return 0;
}
