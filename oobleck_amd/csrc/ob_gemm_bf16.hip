// ob_gemm_bf16.hip — the bf16 MFMA GEMMs of the mixed-precision path: the
// generic kernel (any transposes, edges) and the three NT fast kernels
// (glds 128x128, 256-row, 256x256 8-phase), their dispatchers and the
// public ob_gemm_bf16 entry.  Which kernel a call gets is decided in
// ob_gemm_route.h.
//
// v_mfma_f32_32x32x16_bf16: fp32 accumulate, dense peak ~2.5 PF/s
// (16x the f32 matrix rate).  Fragment layout (derived from the CDNA
// pattern the guides document — f32 ops use k = lane-group index, the
// bf16 K-deep ops give each lane a CONTIGUOUS k-run of K/2 elements;
// verified empirically by tests/test_gpu_bf16.py against torch matmul):
//   A: lane l holds A[i = l&31][k = 8*(l>>5) + j], j = 0..7  (one 16-byte
//      ds_read_b128 when the LDS image is [row][k] with k contiguous)
//   B: lane l holds B[k = 8*(l>>5) + j][n = l&31]
//   C/D: col = l&31, row = (r&3) + 8*(r>>2) + 4*(l>>5)  (dtype-independent)
//
// LDS images are [row][k] (row = M-row for A, N-col for B) with the row
// stride padded to 40 halfs (80 B) so the 16-lane ds_read_b128 groups hit
// 16 distinct bank quads (bank = (20*row + 4*khalf) % 64 covers 0..60
// step 4 across a group).  Operands whose k is contiguous in memory
// (activations [M,K]; weight shadows kept in BOTH [in,out] and [out,in]
// layouts by the layer) stage directly; k-strided operands (the TN weight
// -grad case) transpose-stage through scattered 2-byte LDS writes.
#include "ob_internal.h"

#include <cmath>

#include "ob_bf16.h"
#include "ob_gemm_route.h"

using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

#define BF_LDS_K 40  // padded row stride in halfs (80 B)

// the scalar arguments every GEMM kernel takes, from an ob_bf16_gemm; the
// NT kernels append the store-row guard Mr
#define OB_GEMM_KARGS(g, nbn)                                                \
  (const __bf16*)(g).A, (const __bf16*)(g).B, (g).C,                         \
      (const float*)(g).bias, (const __bf16*)(g).residual, (int)(g).M,       \
      (int)(g).N, (int)(g).K, (g).lda, (g).ldb, (g).ldc, (g).sA1, (g).sA2,   \
      (g).sB1, (g).sB2, (g).sC1, (g).sC2, (int)(g).n2, (g).alpha, (g).beta,  \
      nbn

// pack 8 guarded scalar loads into a uint4 without an address-taken local
template <bool EDGE>
__device__ __forceinline__ uint4 bf_load8(const __bf16* p, int valid) {
  uint4 v = {0, 0, 0, 0};
  unsigned e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
    e[j] = (!EDGE || j < valid) ? bf_bits(p[j]) : 0u;
  v.x = e[0] | (e[1] << 16);
  v.y = e[2] | (e[3] << 16);
  v.z = e[4] | (e[5] << 16);
  v.w = e[6] | (e[7] << 16);
  return v;
}

// direct staging: img[row][k] = src[row][k], k contiguous in memory.
// 256 threads; NR = tile rows (64 or 128).
template <bool EDGE, int NR>
__device__ __forceinline__ void bf_stage_direct_n(__bf16* img,
                                                  const __bf16* src,
                                                  int64_t ld, int rmax,
                                                  int kmax) {
  constexpr int TPR = 1024 / (NR * 4);  // k-chunks per thread pass
  const int r = threadIdx.x / (256 / NR);
  const int kb0 = (threadIdx.x % (256 / NR)) * 8;
#pragma unroll
  for (int it = 0; it < (NR * 4) / 256; ++it) {
    const int kb = kb0 + it * (256 / NR) * 8;
    uint4 v = {0, 0, 0, 0};
    if (!EDGE || (r < rmax && kb + 7 < kmax)) {
      v = *reinterpret_cast<const uint4*>(src + (int64_t)r * ld + kb);
    } else if (r < rmax && kb < kmax) {
      v = bf_load8<EDGE>(src + (int64_t)r * ld + kb, kmax - kb);
    }
    *reinterpret_cast<uint4*>(img + r * BF_LDS_K + kb) = v;
  }
  (void)sizeof(char[TPR >= 0 ? 1 : -1]);
}

template <bool EDGE>
__device__ __forceinline__ void bf_stage_direct(__bf16* img,
                                                const __bf16* src, int64_t ld,
                                                int rmax, int kmax) {
  bf_stage_direct_n<EDGE, 128>(img, src, ld, rmax, kmax);
}

// transpose staging: img[row][k] = src[k][row] (src k-major, ld = src row
// stride).  Reads 16 B along the row dim (coalesced), writes 8 scattered
// 2-byte LDS stores.  NR = tile rows.
template <bool EDGE, int NR>
__device__ __forceinline__ void bf_stage_transpose_n(__bf16* img,
                                                     const __bf16* src,
                                                     int64_t ld, int rmax,
                                                     int kmax) {
  constexpr int RGROUPS = NR / 8;  // 8-row chunks
  const int rb = (threadIdx.x % RGROUPS) * 8;
  const int k0 = threadIdx.x / RGROUPS;
#pragma unroll
  for (int it = 0; it < (RGROUPS * 32) / 256; ++it) {
    const int k = k0 + it * (256 / RGROUPS);
    uint4 v = {0, 0, 0, 0};
    bool any = true;
    if (!EDGE || (k < kmax && rb + 7 < rmax)) {
      v = *reinterpret_cast<const uint4*>(src + (int64_t)k * ld + rb);
    } else if (k < kmax && rb < rmax) {
      v = bf_load8<EDGE>(src + (int64_t)k * ld + rb, rmax - rb);
    } else {
      any = (k < BF_BK);  // still must zero-fill the image
    }
    if (any) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        img[(rb + j) * BF_LDS_K + k] = bf_extract(v, j);
    }
  }
}

template <bool EDGE>
__device__ __forceinline__ void bf_stage_transpose(__bf16* img,
                                                   const __bf16* src,
                                                   int64_t ld, int rmax,
                                                   int kmax) {
  bf_stage_transpose_n<EDGE, 128>(img, src, ld, rmax, kmax);
}

template <bool TA, bool TB, int OUT, bool EDGE, int BN>
__global__ __launch_bounds__(256, 2) void k_gemm_bf16(
    const __bf16* __restrict__ A, const __bf16* __restrict__ B,
    void* __restrict__ Cv, const float* __restrict__ bias,
    const __bf16* __restrict__ R, int M, int N, int K, int64_t lda,
    int64_t ldb, int64_t ldc, int64_t sA1, int64_t sA2, int64_t sB1,
    int64_t sB2, int64_t sC1, int64_t sC2, int n2, float alpha, float beta,
    int nbn) {
  constexpr int FN = BN / 64;  // B fragments per wave (1 or 2)
  __shared__ __bf16 As[2][BF_BM * BF_LDS_K];
  __shared__ __bf16 Bs[2][BN * BF_LDS_K];

  const int tile = blockIdx.x;
  const int bm = tile / nbn, bn = tile % nbn;
  const int m0 = bm * BF_BM, n0 = bn * BN;

  const int z = blockIdx.z;
  const int i1 = z / n2, i2 = z % n2;
  A += (int64_t)i1 * sA1 + (int64_t)i2 * sA2;
  B += (int64_t)i1 * sB1 + (int64_t)i2 * sB2;
  float* Cf = reinterpret_cast<float*>(Cv);
  __bf16* Cb = reinterpret_cast<__bf16*>(Cv);
  const int64_t coff = (int64_t)i1 * sC1 + (int64_t)i2 * sC2;
  Cf += coff;
  Cb += coff;
  if (R) R += coff;

  const int splitk = gridDim.y;
  const int kchunk = ((K + splitk * BF_BK - 1) / (splitk * BF_BK)) * BF_BK;
  const int kbeg = blockIdx.y * kchunk;
  const int kend = min(K, kbeg + kchunk);
  if (kbeg >= kend) return;

  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int il = lane & 31, kh = lane >> 5;

#define OB_BF_STAGE(BUF, KT)                                                  \
  {                                                                           \
    const int kmax_ = min(kend - (KT), BF_BK);                                \
    if (TA)                                                                   \
      bf_stage_transpose<EDGE>(As[BUF], A + (int64_t)(KT)*lda + m0, lda,      \
                               min(M - m0, BF_BM), kmax_);                    \
    else                                                                      \
      bf_stage_direct<EDGE>(As[BUF], A + (int64_t)m0 * lda + (KT), lda,       \
                            min(M - m0, BF_BM), kmax_);                       \
    if (TB)                                                                   \
      bf_stage_direct_n<EDGE, BN>(Bs[BUF], B + (int64_t)n0 * ldb + (KT), ldb, \
                                  min(N - n0, BN), kmax_);                    \
    else                                                                      \
      bf_stage_transpose_n<EDGE, BN>(Bs[BUF], B + (int64_t)(KT)*ldb + n0,     \
                                     ldb, min(N - n0, BN), kmax_);            \
  }

  f32x16 acc00 = {}, acc01 = {}, acc10 = {}, acc11 = {};

#define OB_BF_MFMA(BUF)                                                       \
  _Pragma("unroll") for (int ks = 0; ks < BF_BK / 16; ++ks) {                 \
    const int kb = ks * 16 + kh * 8;                                          \
    const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(                       \
        As[BUF] + (wr * 64 + il) * BF_LDS_K + kb);                            \
    const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(                       \
        As[BUF] + (wr * 64 + 32 + il) * BF_LDS_K + kb);                       \
    const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(                       \
        Bs[BUF] + (wc * (BN / 2) + il) * BF_LDS_K + kb);                      \
    acc00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc00, 0, 0, 0);  \
    acc10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc10, 0, 0, 0);  \
    if (FN == 2) {                                                            \
      const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(                     \
          Bs[BUF] + (wc * (BN / 2) + 32 + il) * BF_LDS_K + kb);               \
      acc01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc01, 0, 0, 0);\
      acc11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc11, 0, 0, 0);\
    }                                                                         \
  }                                                                      \
  __builtin_amdgcn_s_setprio(0);

  OB_BF_STAGE(0, kbeg)
  __syncthreads();
  int cur = 0;
  for (int kt = kbeg; kt + BF_BK < kend; kt += BF_BK) {
    OB_BF_STAGE(cur ^ 1, kt + BF_BK)
    OB_BF_MFMA(cur)
    __syncthreads();
    cur ^= 1;
  }
  OB_BF_MFMA(cur)
#undef OB_BF_STAGE
#undef OB_BF_MFMA

  const int mw = m0 + wr * 64, nw = n0 + wc * (BN / 2);
#define OB_BF_EPI(ACC, TI, TJ)                                                \
  {                                                                           \
    const int nn = nw + (TJ)*32 + il;                                         \
    if (!EDGE || nn < N) {                                                    \
      _Pragma("unroll") for (int r = 0; r < 16; ++r) {                        \
        const int mm = mw + (TI)*32 + (r & 3) + 8 * (r >> 2) + 4 * kh;        \
        if (!EDGE || mm < M) {                                                \
          float v = alpha * ACC[r];                                           \
          if (OUT == BF_OUT_F32_ATOMIC) {                                     \
            atomicAdd(&Cf[(int64_t)mm * ldc + nn], v);                        \
          } else {                                                            \
            if (bias) v += bias[nn];                                          \
            if (R) v += bf2f(R[(int64_t)mm * ldc + nn]);                      \
            if (OUT == BF_OUT_F32) {                                          \
              if (beta != 0.f) v += beta * Cf[(int64_t)mm * ldc + nn];        \
              Cf[(int64_t)mm * ldc + nn] = v;                                 \
            } else {                                                          \
              if (beta != 0.f) v += beta * bf2f(Cb[(int64_t)mm * ldc + nn]);  \
              Cb[(int64_t)mm * ldc + nn] = (__bf16)v;                         \
            }                                                                 \
          }                                                                   \
        }                                                                     \
      }                                                                       \
    }                                                                         \
  }
  OB_BF_EPI(acc00, 0, 0)
  OB_BF_EPI(acc10, 1, 0)
  if (FN == 2) {
    OB_BF_EPI(acc01, 0, 1)
    OB_BF_EPI(acc11, 1, 1)
  }
#undef OB_BF_EPI
}

// ---------------------------------------------------------------------------
// Fast NT path (A [M,K] direct, B [N,K] direct — the fwd/dX hot shapes fed
// by the transposed weight shadows): async global_load_lds width-16 staging
// into lane-linear [row][32-half] images with a SOURCE-side slot swizzle
// (rule 21: glds writes base+lane*16, so the bank swizzle moves to the
// per-lane global address and the matching XOR on the read).  Swizzle key
// (row&3)^((row>>2)&3) makes the 16-lane ds_read_b128 fragment groups hit
// 16 distinct bank quads.  2-phase: issue next tile's glds, MFMA current,
// one __syncthreads per tile (its implicit vmcnt(0) drains the DMA —
// exactly the guide's minimum 2-phase glds recipe).  No staging registers
// -> 4 blocks/CU (the reg-staged kernel measured 62% SQ_WAIT_ANY: parked
// on HBM latency that 256-cycle bf16 MFMA segments cannot hide).
// ---------------------------------------------------------------------------

__device__ __forceinline__ int bf_xcd_swz(int bid, int nwg) {
  // T1: give each XCD a contiguous run of tiles so shared operand panels
  // stay in its private L2 (bijective variant for nwg % 8 != 0).
  const int q = nwg / 8, r = nwg % 8;
  const int xcd = bid % 8, idx = bid / 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

__device__ __forceinline__ int bf_swz_key(int row) {
  return (row & 3) ^ ((row >> 2) & 3);
}

template <int OUT>
__global__ __launch_bounds__(256, 3) void k_gemm_bf16_nt_glds(
    const __bf16* __restrict__ A, const __bf16* __restrict__ B,
    void* __restrict__ Cv, const float* __restrict__ bias,
    const __bf16* __restrict__ R, int M, int N, int K, int64_t lda,
    int64_t ldb, int64_t ldc, int64_t sA1, int64_t sA2, int64_t sB1,
    int64_t sB2, int64_t sC1, int64_t sC2, int n2, float alpha, float beta,
    int nbn, int Mr) {
  // 8 KB per operand per buffer, lane-linear; 3 buffers so two tiles'
  // DMAs stay in flight across the (raw) barrier — counted vmcnt(8)
  // waits only for the current tile's pieces (guide: 3-buf span +83%
  // over serial vs +40% for drain-per-tile).
  __shared__ __bf16 As[3][128 * 32];
  __shared__ __bf16 Bs[3][128 * 32];

  const int tile = bf_xcd_swz(blockIdx.x, gridDim.x);
  const int bm = tile / nbn, bn = tile % nbn;
  const int m0 = bm * 128, n0 = bn * 128;

  const int z = blockIdx.z;
  const int i1 = z / n2, i2 = z % n2;
  A += (int64_t)i1 * sA1 + (int64_t)i2 * sA2;
  B += (int64_t)i1 * sB1 + (int64_t)i2 * sB2;
  float* Cf = reinterpret_cast<float*>(Cv);
  __bf16* Cb = reinterpret_cast<__bf16*>(Cv);
  const int64_t coff = (int64_t)i1 * sC1 + (int64_t)i2 * sC2;
  Cf += coff;
  Cb += coff;
  if (R) R += coff;

  const int splitk = gridDim.y;
  const int kchunk = ((K + splitk * BF_BK - 1) / (splitk * BF_BK)) * BF_BK;
  const int kbeg = blockIdx.y * kchunk;
  const int kend = min(K, kbeg + kchunk);
  if (kbeg >= kend) return;

  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int il = lane & 31, kh = lane >> 5;

  // glds geometry: one 1-KiB wave instruction covers 16 rows x 64 B.
  // wave w stages rows [w*32, w*32+32) of each operand = 2 instructions.
  // lane l within an instruction: row16 = l/4, slot = l%4; the element
  // block written at [row][slot] must come from source half-range
  // (slot ^ key(row)) * 8.
  const int g_row16 = lane >> 2;        // 0..15
  const int g_slot = lane & 3;          // 16-B slot within the 64-B row
#define OB_NT_GLDS(BUF, KT)                                                   \
  {                                                                           \
    _Pragma("unroll") for (int half = 0; half < 2; ++half) {                  \
      const int row = w * 32 + half * 16 + g_row16;                           \
      const int srchalf = (g_slot ^ bf_swz_key(row)) * 8;                     \
      const __bf16* asrc = A + (int64_t)(m0 + row) * lda + (KT) + srchalf;    \
      const __bf16* bsrc = B + (int64_t)(n0 + row) * ldb + (KT) + srchalf;    \
      auto albase = (__attribute__((address_space(3))) void*)                 \
          (&As[BUF][(w * 32 + half * 16) * 32]);                              \
      auto blbase = (__attribute__((address_space(3))) void*)                 \
          (&Bs[BUF][(w * 32 + half * 16) * 32]);                              \
      __builtin_amdgcn_global_load_lds(                                       \
          (const __attribute__((address_space(1))) void*)asrc, albase, 16, 0, \
          0);                                                                 \
      __builtin_amdgcn_global_load_lds(                                       \
          (const __attribute__((address_space(1))) void*)bsrc, blbase, 16, 0, \
          0);                                                                 \
    }                                                                         \
  }

  f32x16 acc00 = {}, acc01 = {}, acc10 = {}, acc11 = {};

  // fragment read with the matching slot XOR
#define OB_NT_FRAG(IMG, ROW, SLOT)                                            \
  (*reinterpret_cast<const bf16x8*>(                                          \
      IMG + (ROW)*32 + (((SLOT) ^ bf_swz_key(ROW)) * 8)))

#define OB_NT_MFMA(BUF)                                                       \
  __builtin_amdgcn_s_setprio(1);                                              \
  _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {                          \
    const int slot = ks * 2 + kh;                                             \
    const int ra0 = wr * 64 + il, ra1 = wr * 64 + 32 + il;                    \
    const int rb0 = wc * 64 + il, rb1 = wc * 64 + 32 + il;                    \
    const bf16x8 a0 = OB_NT_FRAG(As[BUF], ra0, slot);                         \
    const bf16x8 a1 = OB_NT_FRAG(As[BUF], ra1, slot);                         \
    const bf16x8 b0 = OB_NT_FRAG(Bs[BUF], rb0, slot);                         \
    const bf16x8 b1 = OB_NT_FRAG(Bs[BUF], rb1, slot);                         \
    acc00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc00, 0, 0, 0);  \
    acc01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc01, 0, 0, 0);  \
    acc10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc10, 0, 0, 0);  \
    acc11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc11, 0, 0, 0);  \
  }

  // Prologue: two tiles in flight.  Each wave issues 4 glds per tile
  // (2 ops x 2 halves), so vmcnt(8) = "my tile-t pieces landed, tiles
  // t+1/t+2 still flying"; the raw barrier then guarantees every wave's
  // tile-t pieces landed (each waited its own count before arriving).
  OB_NT_GLDS(0, kbeg)
  const bool has1 = kbeg + BF_BK < kend;
  if (has1) OB_NT_GLDS(1, kbeg + BF_BK)
  int cur = 0;
  int kt = kbeg;
  for (; kt + 2 * BF_BK < kend; kt += BF_BK) {
    OB_NT_GLDS((cur + 2) % 3, kt + 2 * BF_BK)
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    OB_NT_MFMA(cur)
    __builtin_amdgcn_s_barrier();
    cur = (cur + 1) % 3;
  }
  // epilogue: drain the last one or two tiles
  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  OB_NT_MFMA(cur)
  if (has1) {
    __builtin_amdgcn_s_barrier();
    cur = (cur + 1) % 3;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    OB_NT_MFMA(cur)
  }
#undef OB_NT_GLDS
#undef OB_NT_FRAG
#undef OB_NT_MFMA

  const int mw = m0 + wr * 64, nw = n0 + wc * 64;
#define OB_NT_EPI(ACC, TI, TJ)                                                \
  {                                                                           \
    const int nn = nw + (TJ)*32 + il;                                         \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) {                          \
      const int mm = mw + (TI)*32 + (r & 3) + 8 * (r >> 2) + 4 * kh;          \
      if (mm >= Mr) continue;                                                 \
      float v = alpha * ACC[r];                                               \
      if (OUT == BF_OUT_F32_ATOMIC) {                                         \
        atomicAdd(&Cf[(int64_t)mm * ldc + nn], v);                            \
      } else {                                                                \
        if (bias) v += bias[nn];                                              \
        if (R) v += bf2f(R[(int64_t)mm * ldc + nn]);                          \
        if (OUT == BF_OUT_F32) {                                              \
          if (beta != 0.f) v += beta * Cf[(int64_t)mm * ldc + nn];            \
          Cf[(int64_t)mm * ldc + nn] = v;                                     \
        } else {                                                              \
          if (beta != 0.f) v += beta * bf2f(Cb[(int64_t)mm * ldc + nn]);      \
          Cb[(int64_t)mm * ldc + nn] = (__bf16)v;                             \
        }                                                                     \
      }                                                                       \
    }                                                                         \
  }
  OB_NT_EPI(acc00, 0, 0)
  OB_NT_EPI(acc01, 0, 1)
  OB_NT_EPI(acc10, 1, 0)
  OB_NT_EPI(acc11, 1, 1)
#undef OB_NT_EPI
}

int ob_gemm_bf16_nt_dispatch(const ob_bf16_gemm& g) {
  const int nbm = (int)(g.M / 128), nbn = (int)(g.N / 128);
  dim3 grid(nbm * nbn, g.splitk, (unsigned)(g.n1 * g.n2));
  dim3 block(256);
#define OB_NTG(OUT_)                                                         \
  k_gemm_bf16_nt_glds<OUT_><<<grid, block, 0, S(g.stream)>>>(                \
      OB_GEMM_KARGS(g, nbn), (int)g.Mr)
  if (g.out_kind == BF_OUT_BF16) OB_NTG(BF_OUT_BF16);
  else if (g.out_kind == BF_OUT_F32) OB_NTG(BF_OUT_F32);
  else OB_NTG(BF_OUT_F32_ATOMIC);
#undef OB_NTG
  OB_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// 256-row NT tile (BM=256, BN in {128,256}, BK=64, 8 waves): halves the
// per-operand re-read factor that bounds the 128² tile (PMC: 110 MB
// fetched vs 37.7 MB algorithmic on the fc shape) and quadruples the MFMA
// run between barriers (32 per wave per tile).  glds staging with the
// row-keyed slot swizzle (key = (row>>1)&7 over 128-B rows: the 16-lane
// ds_read_b128 groups land on 16 distinct bank quads).  2 LDS buffers,
// loads for tile t+1 in flight under tile t's MFMAs.
// ---------------------------------------------------------------------------

__device__ __forceinline__ int bf_swz_key8(int row) { return (row >> 1) & 7; }

template <int OUT, int BN>
__global__ __launch_bounds__(512, 2) void k_gemm_bf16_nt_256(
    const __bf16* __restrict__ A, const __bf16* __restrict__ B,
    void* __restrict__ Cv, const float* __restrict__ bias,
    const __bf16* __restrict__ R, int M, int N, int K, int64_t lda,
    int64_t ldb, int64_t ldc, int64_t sA1, int64_t sA2, int64_t sB1,
    int64_t sB2, int64_t sC1, int64_t sC2, int n2, float alpha, float beta,
    int nbn, int Mr) {
  constexpr int FN = BN / 128;  // N fragments per wave (1 or 2)
  __shared__ __bf16 As[2][256 * 64];
  __shared__ __bf16 Bs[2][BN * 64];

  const int tile = bf_xcd_swz(blockIdx.x, gridDim.x);
  const int bm = tile / nbn, bn = tile % nbn;
  const int m0 = bm * 256, n0 = bn * BN;

  const int z = blockIdx.z;
  const int i1 = z / n2, i2 = z % n2;
  A += (int64_t)i1 * sA1 + (int64_t)i2 * sA2;
  B += (int64_t)i1 * sB1 + (int64_t)i2 * sB2;
  float* Cf = reinterpret_cast<float*>(Cv);
  __bf16* Cb = reinterpret_cast<__bf16*>(Cv);
  const int64_t coff = (int64_t)i1 * sC1 + (int64_t)i2 * sC2;
  Cf += coff;
  Cb += coff;
  if (R) R += coff;

  const int splitk = gridDim.y;
  constexpr int BK = 64;
  const int kchunk = ((K + splitk * BK - 1) / (splitk * BK)) * BK;
  const int kbeg = blockIdx.y * kchunk;
  const int kend = min(K, kbeg + kchunk);
  if (kbeg >= kend) return;

  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;     // 0..7
  const int wr = w >> 2, wc = w & 3;  // 2 x 4 wave grid
  const int il = lane & 31, kh = lane >> 5;

  // glds: one instr = 8 rows x 128 B; lane l: row l/8, slot l%8 within it
  const int g_row8 = lane >> 3;
  const int g_slot = lane & 7;
#define OB_N2_GLDS(BUF, KT)                                                   \
  {                                                                           \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                           \
      const int row = w * 32 + i * 8 + g_row8;                                \
      const int srch = (g_slot ^ bf_swz_key8(row)) * 8;                       \
      const __bf16* asrc = A + (int64_t)(m0 + row) * lda + (KT) + srch;       \
      auto albase = (__attribute__((address_space(3))) void*)                 \
          (&As[BUF][(w * 32 + i * 8) * 64]);                                  \
      __builtin_amdgcn_global_load_lds(                                       \
          (const __attribute__((address_space(1))) void*)asrc, albase, 16, 0, \
          0);                                                                 \
    }                                                                         \
    _Pragma("unroll") for (int i = 0; i < BN / 64; ++i) {                     \
      const int row = w * (BN / 8) + i * 8 + g_row8;                          \
      const int srch = (g_slot ^ bf_swz_key8(row)) * 8;                       \
      const __bf16* bsrc = B + (int64_t)(n0 + row) * ldb + (KT) + srch;       \
      auto blbase = (__attribute__((address_space(3))) void*)                 \
          (&Bs[BUF][(w * (BN / 8) + i * 8) * 64]);                            \
      __builtin_amdgcn_global_load_lds(                                       \
          (const __attribute__((address_space(1))) void*)bsrc, blbase, 16, 0, \
          0);                                                                 \
    }                                                                         \
  }

  f32x16 acc[4][FN];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < FN; ++ni) acc[mi][ni] = (f32x16){};

#define OB_N2_FRAG(IMG, ROW, SLOT)                                            \
  (*reinterpret_cast<const bf16x8*>(                                          \
      IMG + (ROW)*64 + (((SLOT) ^ bf_swz_key8(ROW)) * 8)))

#define OB_N2_MFMA(BUF)                                                       \
  __builtin_amdgcn_s_setprio(1);                                              \
  _Pragma("unroll") for (int ks = 0; ks < 4; ++ks) {                          \
    const int slot = ks * 2 + kh;                                             \
    bf16x8 bfr[FN];                                                           \
    _Pragma("unroll") for (int ni = 0; ni < FN; ++ni) bfr[ni] =               \
        OB_N2_FRAG(Bs[BUF], wc * (BN / 4) + ni * 32 + il, slot);              \
    _Pragma("unroll") for (int mi = 0; mi < 4; ++mi) {                        \
      const bf16x8 af =                                                       \
          OB_N2_FRAG(As[BUF], wr * 128 + mi * 32 + il, slot);                 \
      _Pragma("unroll") for (int ni = 0; ni < FN; ++ni) acc[mi][ni] =         \
          __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr[ni], acc[mi][ni],   \
                                                  0, 0, 0);                   \
    }                                                                         \
  }                                                                           \
  __builtin_amdgcn_s_setprio(0);

  // counted vmcnt + raw barriers: at 1 block/CU there is no co-resident
  // block to hide the drain, so never wait the in-flight next tile.
  // per-wave glds per tile: 4 (A) + BN/64 (B: BN/8 rows, 8 per
  // instruction) = 8 (BN=256) or 6 (BN=128).
  OB_N2_GLDS(0, kbeg)
  int cur = 0;
  for (int kt = kbeg; kt + BK < kend; kt += BK) {
    OB_N2_GLDS(cur ^ 1, kt + BK)
    if (BN == 256)
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    OB_N2_MFMA(cur)
    __builtin_amdgcn_s_barrier();
    cur ^= 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  OB_N2_MFMA(cur)
#undef OB_N2_GLDS
#undef OB_N2_FRAG
#undef OB_N2_MFMA

  const int mw = m0 + wr * 128, nw = n0 + wc * (BN / 4);
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
    for (int ni = 0; ni < FN; ++ni) {
      const int nn = nw + ni * 32 + il;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int mm = mw + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (mm >= Mr) continue;
        float v = alpha * acc[mi][ni][r];
        if (OUT == BF_OUT_F32_ATOMIC) {
          atomicAdd(&Cf[(int64_t)mm * ldc + nn], v);
        } else {
          if (bias) v += bias[nn];
          if (R) v += bf2f(R[(int64_t)mm * ldc + nn]);
          if (OUT == BF_OUT_F32) {
            if (beta != 0.f) v += beta * Cf[(int64_t)mm * ldc + nn];
            Cf[(int64_t)mm * ldc + nn] = v;
          } else {
            if (beta != 0.f) v += beta * bf2f(Cb[(int64_t)mm * ldc + nn]);
            Cb[(int64_t)mm * ldc + nn] = (__bf16)v;
          }
        }
      }
    }
  }
}

int ob_gemm_bf16_nt256_dispatch(const ob_bf16_gemm& g, int BN) {
  const int nbm = (int)((g.M + 255) / 256), nbn = (int)((g.N + BN - 1) / BN);
  dim3 grid(nbm * nbn, g.splitk, (unsigned)(g.n1 * g.n2));
  dim3 block(512);
#define OB_N2G(OUT_, BN_)                                                    \
  k_gemm_bf16_nt_256<OUT_, BN_><<<grid, block, 0, S(g.stream)>>>(            \
      OB_GEMM_KARGS(g, nbn), (int)g.Mr)
  if (BN == 256) {
    if (g.out_kind == BF_OUT_BF16) OB_N2G(BF_OUT_BF16, 256);
    else if (g.out_kind == BF_OUT_F32) OB_N2G(BF_OUT_F32, 256);
    else OB_N2G(BF_OUT_F32_ATOMIC, 256);
  } else {
    if (g.out_kind == BF_OUT_BF16) OB_N2G(BF_OUT_BF16, 128);
    else if (g.out_kind == BF_OUT_F32) OB_N2G(BF_OUT_F32, 128);
    else OB_N2G(BF_OUT_F32_ATOMIC, 128);
  }
#undef OB_N2G
  OB_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// 256x256 8-phase NT GEMM (the guide's fast template: glds staging,
// st_16x32 LDS swizzle, per-phase ds_read || glds || MFMA interleave,
// counted vmcnt once per K-tile, raw barriers, 1 block/CU).
//   tile 256x256, BK=64, 512 threads = 8 waves as 2(M) x 4(N);
//   per-wave output 128x64; MFMA 16x16x32 bf16 (fp32 acc).
//   LDS = 2 buffers x 4 images x [128 rows][64 k] bf16 = 128 KiB.
//   images: 0 = A rows 0-127, 1 = A rows 128-255, 2 = B rows 0-127,
//   3 = B rows 128-255 (B = [N,K] k-major, NT).
//   st_16x32 swizzle: image byte ^= ((byte>>9)&1)<<5, applied via the
//   SOURCE-side address on the lane-linear glds write and the matching
//   XOR on ds_read (glds cannot scatter).
//   K-tile = 4 phases, one output quadrant (4 M-frags x 2 N-frags) each;
//   staging runs 3 images ahead: phase 1 stages the next tile's last
//   image, phase 4 stages tile+2's first three (into the buffer whose
//   reads completed at phase 3's closing barrier), so the per-K-tile
//   wait is vmcnt(6) = "3 images still flying".
// ---------------------------------------------------------------------------

using f32x4 = __attribute__((ext_vector_type(4))) float;

// SWZ 0: within-row 8-slot XOR, key (row>>1)&7 (the nt256 kernel's
// measured-0-conflict pattern); SWZ 1: 16-slot XOR with the bit-6 flip.
template <int OUT, int SWZ = 0>
__global__ __launch_bounds__(512, 1) void k_gemm_bf16_nt_8ph(
    const __bf16* __restrict__ A, const __bf16* __restrict__ B,
    void* __restrict__ Cv, const float* __restrict__ bias,
    const __bf16* __restrict__ R, int M, int N, int K, int64_t lda,
    int64_t ldb, int64_t ldc, int64_t sA1, int64_t sA2, int64_t sB1,
    int64_t sB2, int64_t sC1, int64_t sC2, int n2, float alpha, float beta,
    int nbn, int Mr) {
  __shared__ __bf16 lds[2][4][128 * 64];

  const int tile = bf_xcd_swz(blockIdx.x, gridDim.x);
  const int bm = tile / nbn, bn = tile % nbn;
  const int m0 = bm * 256, n0 = bn * 256;

  const int z = blockIdx.z;
  const int i1 = z / n2, i2 = z % n2;
  A += (int64_t)i1 * sA1 + (int64_t)i2 * sA2;
  B += (int64_t)i1 * sB1 + (int64_t)i2 * sB2;
  float* Cf = reinterpret_cast<float*>(Cv);
  __bf16* Cb = reinterpret_cast<__bf16*>(Cv);
  const int64_t coff = (int64_t)i1 * sC1 + (int64_t)i2 * sC2;
  Cf += coff;
  Cb += coff;
  if (R) R += coff;

  const int splitk = gridDim.y;
  constexpr int BK = 64;
  const int kchunk = ((K + splitk * BK - 1) / (splitk * BK)) * BK;
  const int kbeg = blockIdx.y * kchunk;
  const int kend = min(K, kbeg + kchunk);
  if (kbeg >= kend) return;
  const int NT = (kend - kbeg) / BK;  // K % 64 == 0 gated at dispatch

  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;     // 0..7
  const int wr = w >> 2, wc = w & 3;  // 2(M) x 4(N)
  const int l16 = lane & 15, lg = lane >> 4;

  // ---- LDS swizzle (T2, conflict-free variant): element index
  //   idx = row*64 XOR (ke XOR ((row&15)<<3))
  // The (row&8)<<3 term crosses the 64-element row boundary (it flips
  // idx bit 6 = the bank-row half), so the 16 distinct rows of a
  // ds_read_b128 fragment group land on 16 distinct 16-B slots of the
  // 256-B bank row: conflict-free (the plain in-row XOR caps at 4-way).
  // glds writes are lane-linear, so the permutation moves to the SOURCE
  // address: lane l of block blk (8 image rows, 1 KiB) fetches
  //   row = blk*8 + (l>>4)*2 + (((l>>3)&1) ^ (blk&1))
  //   ce  = (l&7)*8 ^ ((row&7)<<3)
  // (the inverse of idx at a = blk*512 + l*8).
  // stage image IMG (0/1: A half, 2/3: B half) of K-tile at element KT
#define P8_GLDS1(BUF, IMG, KT)                                                \
  {                                                                           \
    const __bf16* const src0 = (IMG) < 2 ? A : B;                             \
    const int64_t ld = (IMG) < 2 ? lda : ldb;                                 \
    const int r0 = ((IMG)&1) * 128 + ((IMG) < 2 ? m0 : n0);                   \
    _Pragma("unroll") for (int v = 0; v < 2; ++v) {                           \
      const int blk = w * 2 + v;                                              \
      const int row =                                                         \
          SWZ ? blk * 8 + ((lane >> 4) << 1) + (((lane >> 3) & 1) ^ (blk & 1))\
              : blk * 8 + (lane >> 3);                                        \
      const int ce = SWZ ? ((lane & 7) * 8) ^ ((row & 7) << 3)                \
                         : ((lane & 7) * 8) ^ (((row >> 1) & 7) << 3);        \
      const __bf16* src = src0 + (int64_t)(r0 + row) * ld + (KT) + ce;        \
      auto lbase = (__attribute__((address_space(3))) void*)                  \
          (&lds[BUF][IMG][blk * 8 * 64]);                                     \
      __builtin_amdgcn_global_load_lds(                                       \
          (const __attribute__((address_space(1))) void*)src, lbase, 16, 0,   \
          0);                                                                 \
    }                                                                         \
  }

  // ---- swizzled fragment read: row r, k-run element ke (lane's 8-run)
#define P8_FRAG(BUF, IMG, ROW, KE)                                           \
  (*reinterpret_cast<const bf16x8*>(                                         \
      &lds[BUF][IMG][SWZ ? (((ROW)*64) ^ ((KE) ^ ((((ROW)&15)) << 3)))       \
                         : ((ROW)*64 + ((KE) ^ (((((ROW) >> 1)) & 7)         \
                                                << 3)))]))

  f32x4 acc[8][4];
#pragma unroll
  for (int mi = 0; mi < 8; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = (f32x4){};

  bf16x8 Ar[4][2];     // one A half (mi, kk): a=0 read at phase 1 (used
                       // p1, p2), overwritten by a=1 at phase 3
  bf16x8 Br[2][2][2];  // BOTH N-quarters (b, ni, kk): b=0 at phase 1,
                       // b=1 at phase 2, both live through phase 4 (the
                       // B image is then free for phase-3 staging)
  const int imA = wr;            // this wave's A image
  const int imB = 2 + (wc >> 1); // this wave's B image
  const int arow0 = l16;                    // + a*64 + mi*16
  const int brow0 = (wc & 1) * 64 + l16;    // + b*32 + ni*16

#define P8_RD_A(BUF, a)                                                      \
  _Pragma("unroll") for (int mi = 0; mi < 4; ++mi)                           \
      _Pragma("unroll") for (int kk = 0; kk < 2; ++kk) Ar[mi][kk] =          \
          P8_FRAG(BUF, imA, arow0 + (a)*64 + mi * 16, kk * 32 + lg * 8);
#define P8_RD_B(BUF, b)                                                      \
  _Pragma("unroll") for (int ni = 0; ni < 2; ++ni)                           \
      _Pragma("unroll") for (int kk = 0; kk < 2; ++kk) Br[b][ni][kk] =       \
          P8_FRAG(BUF, imB, brow0 + (b)*32 + ni * 16, kk * 32 + lg * 8);

  // kk outer: 8 independent MFMAs between the two updates of each acc
#define P8_MFMA(a, b)                                                        \
  __builtin_amdgcn_s_setprio(1);                                             \
  _Pragma("unroll") for (int kk = 0; kk < 2; ++kk)                           \
      _Pragma("unroll") for (int mi = 0; mi < 4; ++mi)                       \
          _Pragma("unroll") for (int ni = 0; ni < 2; ++ni)                   \
              acc[(a)*4 + mi][(b)*2 + ni] =                                  \
      __builtin_amdgcn_mfma_f32_16x16x32_bf16(                               \
          Ar[mi][kk], Br[b][ni][kk], acc[(a)*4 + mi][(b)*2 + ni], 0, 0,     \
          0);                                                                \
  __builtin_amdgcn_s_setprio(0);

#define P8_FENCE asm volatile("" ::: "memory")
#define P8_BAR                                                               \
  P8_FENCE;                                                                  \
  __builtin_amdgcn_s_barrier();                                              \
  P8_FENCE
#define P8_LGKM asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

  // ---- prologue: tile 0 fully, then tile 1's images in steady-state
  // issue order (img2=B0 as a phase-3 would, img0/img1=A as a phase-4)
  P8_GLDS1(0, 0, kbeg)
  P8_GLDS1(0, 1, kbeg)
  P8_GLDS1(0, 2, kbeg)
  P8_GLDS1(0, 3, kbeg)
  if (NT > 1) {
    P8_GLDS1(1, 2, kbeg + BK)
    P8_GLDS1(1, 0, kbeg + BK)
    P8_GLDS1(1, 1, kbeg + BK)
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  P8_BAR;

  for (int ti = 0; ti < NT; ++ti) {
    const int buf = ti & 1;
    const int kt = kbeg + ti * BK;
    // phase 1: quad (0,0); stage next tile's last image (other buffer)
    P8_RD_A(buf, 0)
    P8_RD_B(buf, 0)
    if (ti + 1 < NT) P8_GLDS1(buf ^ 1, 3, kt + BK)
    P8_BAR;
    P8_LGKM;
    P8_MFMA(0, 0)
    P8_BAR;
    // phase 2: quad (0,1) — last B reads of this tile's buffer
    P8_RD_B(buf, 1)
    P8_BAR;
    P8_LGKM;
    P8_MFMA(0, 1)
    P8_BAR;
    // phase 3: quad (1,0) — last A reads; stage tile+2's first B image
    // into this buffer (B reads completed at phase 2's closing barrier)
    P8_RD_A(buf, 1)
    if (ti + 2 < NT) P8_GLDS1(buf, 2, kt + 2 * BK)
    P8_BAR;
    P8_LGKM;
    P8_MFMA(1, 0)
    P8_BAR;
    // phase 4: quad (1,1); stage tile+2's A images (A reads ended at
    // phase 3's closing barrier)
    if (ti + 2 < NT) {
      P8_GLDS1(buf, 0, kt + 2 * BK)
      P8_GLDS1(buf, 1, kt + 2 * BK)
    }
    P8_MFMA(1, 1)
    if (ti + 1 < NT) {
      if (ti + 2 < NT)
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    P8_BAR;
  }
#undef P8_GLDS1
#undef P8_FRAG
#undef P8_RD_A
#undef P8_RD_B
#undef P8_MFMA

  // ---- epilogue: D frag (mi, ni): row = mi*16 + lg*4 + r, col = ni*16+l16
  const int mw = m0 + wr * 128, nw = n0 + wc * 64;
#pragma unroll
  for (int mi = 0; mi < 8; ++mi) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int nn = nw + ni * 16 + l16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int mm = mw + mi * 16 + lg * 4 + r;
        if (mm >= Mr) continue;
        float v = alpha * acc[mi][ni][r];
        if (OUT == BF_OUT_F32_ATOMIC) {
          atomicAdd(&Cf[(int64_t)mm * ldc + nn], v);
        } else {
          if (bias) v += bias[nn];
          if (R) v += bf2f(R[(int64_t)mm * ldc + nn]);
          if (OUT == BF_OUT_F32) {
            if (beta != 0.f) v += beta * Cf[(int64_t)mm * ldc + nn];
            Cf[(int64_t)mm * ldc + nn] = v;
          } else {
            if (beta != 0.f) v += beta * bf2f(Cb[(int64_t)mm * ldc + nn]);
            Cb[(int64_t)mm * ldc + nn] = (__bf16)v;
          }
        }
      }
    }
  }
}

int ob_gemm_bf16_nt_8ph_dispatch(const ob_bf16_gemm& g) {
  if (g.M % 256 || g.N % 256 || g.K % 64)
    return ob_fail("nt_8ph: M,N %% 256, K %% 64 required");
  const int nbm = (int)(g.M / 256), nbn = (int)(g.N / 256);
  dim3 grid(nbm * nbn, g.splitk < 1 ? 1 : g.splitk, (unsigned)(g.n1 * g.n2));
  dim3 block(512);
  static const int swz = ob_env_int("OB_P8_SWZ", 0);
#define OB_P8(OUT_, SWZ_)                                                    \
  k_gemm_bf16_nt_8ph<OUT_, SWZ_><<<grid, block, 0, S(g.stream)>>>(           \
      OB_GEMM_KARGS(g, nbn), (int)g.Mr)
#define OB_P8S(OUT_)                                                         \
  do {                                                                       \
    if (swz == 1) OB_P8(OUT_, 1);                                            \
    else OB_P8(OUT_, 0);                                                     \
  } while (0)
  if (g.out_kind == BF_OUT_BF16) OB_P8S(BF_OUT_BF16);
  else if (g.out_kind == BF_OUT_F32) OB_P8S(BF_OUT_F32);
  else OB_P8S(BF_OUT_F32_ATOMIC);
#undef OB_P8S
#undef OB_P8
  OB_LAUNCH_CHECK();
  return 0;
}

// probe entry (tools/p8_probe.py, tests): the 8-phase kernel on its own
extern "C" int ob_gemm_bf16_nt_8ph(const void* A, const void* B, void* C,
                                   const void* bias, const void* residual,
                                   int64_t M, int64_t N, int64_t K,
                                   int64_t lda, int64_t ldb, int64_t ldc,
                                   int64_t sA1, int64_t sA2, int64_t sB1,
                                   int64_t sB2, int64_t sC1, int64_t sC2,
                                   int64_t n1, int64_t n2, float alpha,
                                   float beta, int out_kind, int splitk,
                                   void* stream, int64_t Mr) {
  ob_bf16_gemm g;
  g.A = A, g.B = B, g.C = C, g.bias = bias, g.residual = residual;
  g.M = M, g.N = N, g.K = K, g.lda = lda, g.ldb = ldb, g.ldc = ldc;
  g.sA1 = sA1, g.sA2 = sA2, g.sB1 = sB1, g.sB2 = sB2, g.sC1 = sC1, g.sC2 = sC2;
  g.n1 = n1, g.n2 = n2, g.alpha = alpha, g.beta = beta;
  g.out_kind = out_kind, g.splitk = splitk, g.Mr = Mr, g.stream = stream;
  return ob_gemm_bf16_nt_8ph_dispatch(g);
}

// ---------------------------------------------------------------------------
// ob_gemm_bf16: argument checks, the route (ob_gemm_route.h), the launch
// ---------------------------------------------------------------------------

static int gemm_bf16_generic(const ob_bf16_gemm& g, int BN, bool edge) {
  const int nbm = (int)((g.M + BF_BM - 1) / BF_BM);
  const int nbn = (int)((g.N + BN - 1) / BN);
  dim3 grid(nbm * nbn, g.splitk, (unsigned)(g.n1 * g.n2));
  dim3 block(256);
#define OB_BFG_L2(TA_, TB_, OUT_, ED_, BN_)                                  \
  k_gemm_bf16<TA_, TB_, OUT_, ED_, BN_><<<grid, block, 0, S(g.stream)>>>(    \
      OB_GEMM_KARGS(g, nbn))
#define OB_BFG_L(TA_, TB_, OUT_, ED_)                                        \
  do {                                                                       \
    if (BN == 64) OB_BFG_L2(TA_, TB_, OUT_, ED_, 64);                        \
    else OB_BFG_L2(TA_, TB_, OUT_, ED_, 128);                                \
  } while (0)
#define OB_BFG_OUT(TA_, TB_)                                                 \
  do {                                                                       \
    if (g.out_kind == BF_OUT_BF16) {                                         \
      if (edge) OB_BFG_L(TA_, TB_, BF_OUT_BF16, true);                       \
      else OB_BFG_L(TA_, TB_, BF_OUT_BF16, false);                           \
    } else if (g.out_kind == BF_OUT_F32) {                                   \
      if (edge) OB_BFG_L(TA_, TB_, BF_OUT_F32, true);                        \
      else OB_BFG_L(TA_, TB_, BF_OUT_F32, false);                            \
    } else {                                                                 \
      if (edge) OB_BFG_L(TA_, TB_, BF_OUT_F32_ATOMIC, true);                 \
      else OB_BFG_L(TA_, TB_, BF_OUT_F32_ATOMIC, false);                     \
    }                                                                        \
  } while (0)
  switch ((g.transA ? 2 : 0) | (g.transB ? 1 : 0)) {
    case 0: OB_BFG_OUT(false, false); break;
    case 1: OB_BFG_OUT(false, true); break;
    case 2: OB_BFG_OUT(true, false); break;
    case 3: OB_BFG_OUT(true, true); break;
  }
#undef OB_BFG_OUT
#undef OB_BFG_L
#undef OB_BFG_L2
  OB_LAUNCH_CHECK();
  return 0;
}

int ob_gemm_bf16_run(const ob_bf16_gemm& in) {
  if (in.M <= 0 || in.N <= 0 || in.K <= 0)
    return ob_fail("gemm_bf16: bad dims");
  if (in.splitk > 1 && in.out_kind != BF_OUT_F32_ATOMIC)
    return ob_fail("gemm_bf16: splitk needs atomic f32 out");
  // 16-byte staging requires 8-half-aligned leading dims and bases
  if ((in.lda | in.ldb) & 7)
    return ob_fail("gemm_bf16: lda/ldb must be 8-aligned");
  static const bool no_lt = ob_env_flag("OB_NO_BLASLT", false);
  static const bool no_glds = ob_env_flag("OB_BF16_NOGLDS", false);
  static const bool no256 = ob_env_flag("OB_BF16_NO256", false);
  // OB_BF16_FORCE is read per call so one process can sweep variants
  const ob_gemm_env env = {no_lt, no_glds, no256, getenv("OB_BF16_FORCE")};
  const bool aligned16 =
      ((reinterpret_cast<uintptr_t>(in.A) | reinterpret_cast<uintptr_t>(in.B)) %
           16 == 0) &&
      ((in.sA1 | in.sA2 | in.sB1 | in.sB2) % 8 == 0);
  const ob_gemm_route r =
      ob_gemm_bf16_pick(in.transA, in.transB, in.M, in.N, in.K, in.n1, in.n2,
                        in.out_kind, in.splitk, in.beta, aligned16, env);
  if (r.try_lt_first) {
    // bias rides the BIAS epilogue; a residual is folded as the C-INPUT
    // operand of D = alpha*AB + beta*C (C != D) — no copy (the round-1
    // path paid a 12.6 MB DtoD per forward projection GEMM)
    const int rc =
        in.residual
            ? ob_gemm_lt_bias_res(in.transA, in.transB, in.M, in.N, in.K,
                                  in.alpha, in.A, in.lda, in.B, in.ldb, in.C,
                                  in.ldc, 0, in.bias, in.residual, in.stream)
            : ob_gemm_lt_bias(in.transA, in.transB, in.M, in.N, in.K,
                              in.alpha, in.A, in.lda, in.B, in.ldb, 0.f, in.C,
                              in.ldc, 0, in.bias, in.stream);
    if (rc >= 0) return rc;  // -1: no algo, fall through to our kernels
  }
  ob_bf16_gemm g = in;
  g.splitk = r.splitk;
  g.Mr = g.M;
  switch (r.kernel) {
    case OB_GEMM_P8: return ob_gemm_bf16_nt_8ph_dispatch(g);
    case OB_GEMM_NT256: return ob_gemm_bf16_nt256_dispatch(g, r.BN);
    case OB_GEMM_GLDS: return ob_gemm_bf16_nt_dispatch(g);
    default: return gemm_bf16_generic(g, r.BN, r.edge);
  }
}

extern "C" int ob_gemm_bf16(int transA, int transB, int64_t M, int64_t N,
                            int64_t K, float alpha, const void* A, int64_t lda,
                            int64_t strideA1, int64_t strideA2, const void* B,
                            int64_t ldb, int64_t strideB1, int64_t strideB2,
                            float beta, void* C, int64_t ldc, int64_t strideC1,
                            int64_t strideC2, int64_t n1, int64_t n2,
                            const void* bias, const void* residual,
                            int out_kind, int splitk, void* stream) {
  ob_bf16_gemm g;
  g.transA = transA, g.transB = transB, g.M = M, g.N = N, g.K = K;
  g.alpha = alpha, g.beta = beta, g.A = A, g.B = B, g.C = C;
  g.lda = lda, g.ldb = ldb, g.ldc = ldc, g.sA1 = strideA1, g.sA2 = strideA2;
  g.sB1 = strideB1, g.sB2 = strideB2, g.sC1 = strideC1, g.sC2 = strideC2;
  g.n1 = n1, g.n2 = n2, g.bias = bias, g.residual = residual;
  g.out_kind = out_kind, g.splitk = splitk, g.stream = stream;
  return ob_gemm_bf16_run(g);
}

// host-only: the route a call would take; env_mask bit 0 OB_NO_BLASLT,
// bit 1 OB_BF16_NOGLDS, bit 2 OB_BF16_NO256; force = OB_BF16_FORCE or null.
// out = {try_lt_first, kernel, BN, edge, splitk}
extern "C" int ob_gemm_bf16_route(int transA, int transB, int64_t M, int64_t N,
                                  int64_t K, int64_t n1, int64_t n2,
                                  int out_kind, int splitk, float beta,
                                  int aligned16, int env_mask,
                                  const char* force, int32_t* out) {
  if (M <= 0 || N <= 0 || K <= 0 || n1 <= 0 || n2 <= 0 || !out)
    return ob_fail("gemm_bf16_route: bad arguments");
  const ob_gemm_env env = {(env_mask & 1) != 0, (env_mask & 2) != 0,
                           (env_mask & 4) != 0, force};
  const ob_gemm_route r =
      ob_gemm_bf16_pick(transA, transB, M, N, K, n1, n2, out_kind, splitk,
                        beta, aligned16 != 0, env);
  out[0] = r.try_lt_first, out[1] = r.kernel, out[2] = r.BN;
  out[3] = r.edge, out[4] = r.splitk;
  return 0;
}

