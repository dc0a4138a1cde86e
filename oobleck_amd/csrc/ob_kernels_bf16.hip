// ob_kernels_bf16.hip — the bf16 kernels of the mixed-precision path
// except flash attention (ob_flash_bf16.hip): MFMA GEMMs, layernorm,
// softmax, gelu, colsum, embed, cross-entropy, casts and the dW transpose
// (§8 f4: bf16 storage + fp32 master weights; the reference never
// implemented mixed precision, README.md:98).
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

using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

#define BF_BM 128
#define BF_BN 128
#define BF_BK 32
#define BF_LDS_K 40  // padded row stride in halfs (80 B)

// out-kind for the epilogue
enum { BF_OUT_BF16 = 0, BF_OUT_F32 = 1, BF_OUT_F32_ATOMIC = 2 };

__device__ __forceinline__ float bf2f(__bf16 h) { return (float)h; }

__device__ __forceinline__ unsigned bf_bits(__bf16 h) {
  return (unsigned)__builtin_bit_cast(unsigned short, h);
}
__device__ __forceinline__ __bf16 bits_bf(unsigned u) {
  return __builtin_bit_cast(__bf16, (unsigned short)(u & 0xffffu));
}

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

__device__ __forceinline__ __bf16 bf_extract(const uint4& v, int j) {
  // j is a compile-time constant at every call site (unrolled loops)
  const unsigned word = (j < 2) ? v.x : (j < 4) ? v.y : (j < 6) ? v.z : v.w;
  return bits_bf((j & 1) ? (word >> 16) : word);
}

__device__ __forceinline__ uint4 bf_pack8(const float* v) {
  uint4 o;
  o.x = bf_bits((__bf16)v[0]) | (bf_bits((__bf16)v[1]) << 16);
  o.y = bf_bits((__bf16)v[2]) | (bf_bits((__bf16)v[3]) << 16);
  o.z = bf_bits((__bf16)v[4]) | (bf_bits((__bf16)v[5]) << 16);
  o.w = bf_bits((__bf16)v[6]) | (bf_bits((__bf16)v[7]) << 16);
  return o;
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

extern "C" int ob_gemm_bf16(int transA, int transB, int64_t M, int64_t N,
                            int64_t K, float alpha, const void* A, int64_t lda,
                            int64_t strideA1, int64_t strideA2, const void* B,
                            int64_t ldb, int64_t strideB1, int64_t strideB2,
                            float beta, void* C, int64_t ldc, int64_t strideC1,
                            int64_t strideC2, int64_t n1, int64_t n2,
                            const void* bias, const void* residual,
                            int out_kind, int splitk, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0) return ob_fail("gemm_bf16: bad dims");
  if (splitk < 1) splitk = 1;
  if (splitk > 1 && out_kind != BF_OUT_F32_ATOMIC)
    return ob_fail("gemm_bf16: splitk needs atomic f32 out");
  // 16-byte staging requires 8-half-aligned leading dims and bases
  if ((lda | ldb) & 7) return ob_fail("gemm_bf16: lda/ldb must be 8-aligned");
  // probe hook (tools/fc_probe.py): OB_BF16_FORCE picks one NT kernel
  // unconditionally ("glds" | "n128" | "n256" | "8ph"); read per call so
  // one process can sweep variants.
  const char* force = getenv("OB_BF16_FORCE");
  if (force && transA == 0 && transB == 1) {
    const int64_t nbm = (M + 255) / 256;
    if (force[0] == 'g')
      return ob_gemm_bf16_nt_dispatch(A, B, C, bias, residual, M, N, K, lda,
                                      ldb, ldc, strideA1, strideA2, strideB1,
                                      strideB2, strideC1, strideC2, n1, n2,
                                      alpha, beta, out_kind, splitk, stream,
                                      M);
    if (force[0] == 'n') {
      extern int ob_gemm_bf16_nt256_dispatch(
          const void* A, const void* B, void* C, const void* bias,
          const void* residual, int64_t M, int64_t N, int64_t K, int64_t lda,
          int64_t ldb, int64_t ldc, int64_t sA1, int64_t sA2, int64_t sB1,
          int64_t sB2, int64_t sC1, int64_t sC2, int64_t n1, int64_t n2,
          float alpha, float beta, int out_kind, int splitk, void* stream,
          int64_t Mr, int BN);
      return ob_gemm_bf16_nt256_dispatch(
          A, B, C, bias, residual, M, N, K, lda, ldb, ldc, strideA1,
          strideA2, strideB1, strideB2, strideC1, strideC2, n1, n2, alpha,
          beta, out_kind, splitk, stream, M, force[1] == '2' ? 256 : 128);
    }
    if (force[0] == '8') {
      extern int ob_gemm_bf16_nt_8ph(
          const void* A, const void* B, void* C, const void* bias,
          const void* residual, int64_t M, int64_t N, int64_t K, int64_t lda,
          int64_t ldb, int64_t ldc, int64_t sA1, int64_t sA2, int64_t sB1,
          int64_t sB2, int64_t sC1, int64_t sC2, int64_t n1, int64_t n2,
          float alpha, float beta, int out_kind, int splitk, void* stream,
          int64_t Mr);
      return ob_gemm_bf16_nt_8ph(A, B, C, bias, residual, M, N, K, lda, ldb,
                                 ldc, strideA1, strideA2, strideB1, strideB2,
                                 strideC1, strideC2, n1, n2, alpha, beta,
                                 out_kind, splitk, stream, M);
    }
  }
  // plain GEMMs (no bias/residual/beta, unbatched, bf16 out) go to
  // hipBLASLt — the dX family, the bias-free lm_head family (measured
  // 815-1166 TF vs 436-692 for the hand-written kernels on those
  // shapes, tools/blas_probe.py).  Fused epilogues stay on ours.
  static const bool no_lt = [] {
    const char* e = getenv("OB_NO_BLASLT");
    return e && e[0] == '1';
  }();
  if (!no_lt && beta == 0.f && n1 == 1 && n2 == 1 && splitk == 1 &&
      out_kind == BF_OUT_BF16 && M * N >= 512 * 512) {
    // bias rides the BIAS epilogue; a residual is folded as the C-INPUT
    // operand of D = alpha*AB + beta*C (C != D) — no copy (the round-1
    // path paid a 12.6 MB DtoD per forward projection GEMM)
    int r;
    if (residual) {
      r = ob_gemm_lt_bias_res(transA, transB, M, N, K, alpha, A, lda, B,
                              ldb, C, ldc, 0, bias, residual, stream);
    } else {
      r = ob_gemm_lt_bias(transA, transB, M, N, K, alpha, A, lda, B, ldb,
                          0.f, C, ldc, 0, bias, stream);
    }
    if (r >= 0) return r;  // -1: no algo, fall through to our kernels
  }
  const int BN = (N <= 64) ? 64 : 128;  // narrow tiles for head_dim GEMMs
  const int nbm = (int)((M + BF_BM - 1) / BF_BM);
  const int nbn = (int)((N + BN - 1) / BN);
  const bool edge = (M % BF_BM) || (N % BN) || (K % BF_BK);
  dim3 grid(nbm * nbn, splitk, (unsigned)(n1 * n2));
  dim3 block(256);
#define OB_BFG_L2(TA_, TB_, OUT_, ED_, BN_)                                  \
  k_gemm_bf16<TA_, TB_, OUT_, ED_, BN_><<<grid, block, 0, S(stream)>>>(      \
      (const __bf16*)A, (const __bf16*)B, C, (const float*)bias,             \
      (const __bf16*)residual, (int)M, (int)N, (int)K, lda, ldb, ldc,        \
      strideA1, strideA2, strideB1, strideB2, strideC1, strideC2, (int)n2,   \
      alpha, beta, nbn)
#define OB_BFG_L(TA_, TB_, OUT_, ED_)                                        \
  do {                                                                       \
    if (BN == 64) OB_BFG_L2(TA_, TB_, OUT_, ED_, 64);                        \
    else OB_BFG_L2(TA_, TB_, OUT_, ED_, 128);                                \
  } while (0)
#define OB_BFG_OUT(TA_, TB_)                                                 \
  do {                                                                       \
    if (out_kind == BF_OUT_BF16) {                                           \
      if (edge) OB_BFG_L(TA_, TB_, BF_OUT_BF16, true);                       \
      else OB_BFG_L(TA_, TB_, BF_OUT_BF16, false);                           \
    } else if (out_kind == BF_OUT_F32) {                                     \
      if (edge) OB_BFG_L(TA_, TB_, BF_OUT_F32, true);                        \
      else OB_BFG_L(TA_, TB_, BF_OUT_F32, false);                            \
    } else {                                                                 \
      if (edge) OB_BFG_L(TA_, TB_, BF_OUT_F32_ATOMIC, true);                 \
      else OB_BFG_L(TA_, TB_, BF_OUT_F32_ATOMIC, false);                     \
    }                                                                        \
  } while (0)
  // fast NT path: async glds staging (ob_internal.h declares the
  // dispatch; interior 128-aligned shapes with 16-byte-aligned
  // bases/strides only)
  static const bool no_glds = [] {
    const char* e = getenv("OB_BF16_NOGLDS");
    return e && e[0] == '1';
  }();
  const bool aligned16 =
      ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B)) %
           16 == 0) &&
      ((strideA1 | strideA2 | strideB1 | strideB2) % 8 == 0);
  if (!no_glds && transA == 0 && transB == 1 && !edge && aligned16 &&
      K >= 2 * BF_BK) {
    extern int ob_gemm_bf16_nt256_dispatch(
        const void* A, const void* B, void* C, const void* bias,
        const void* residual, int64_t M, int64_t N, int64_t K, int64_t lda,
        int64_t ldb, int64_t ldc, int64_t sA1, int64_t sA2, int64_t sB1,
        int64_t sB2, int64_t sC1, int64_t sC2, int64_t n1, int64_t n2,
        float alpha, float beta, int out_kind, int splitk, void* stream,
        int64_t Mr, int BN);
    // 8-phase 256^2 kernel: wins when its grid fills whole scheduling
    // rounds (measured: lmhead 692 vs 618 TF, 4096^3 1058 vs 995; loses
    // on partial rounds — fc 1.5 rounds: 529 vs 554).  tiles >= 192 and
    // round-efficiency >= 0.9 required.  For atomic outputs (weight
    // grads accumulate, so any K split is valid) the split is CHOSEN to
    // fill rounds rather than taken from the caller.
    if (M % 256 == 0 && N % 256 == 0 && K % 64 == 0) {
      extern int ob_gemm_bf16_nt_8ph(
          const void* A, const void* B, void* C, const void* bias,
          const void* residual, int64_t M, int64_t N, int64_t K, int64_t lda,
          int64_t ldb, int64_t ldc, int64_t sA1, int64_t sA2, int64_t sB1,
          int64_t sB2, int64_t sC1, int64_t sC2, int64_t n1, int64_t n2,
          float alpha, float beta, int out_kind, int splitk, void* stream,
          int64_t Mr);
      // NOTE: an auto-splitk search for atomic outputs was tried here
      // (round-filling sk up to 16) and REGRESSED the step 360k->347k
      // tok/s: split-k multiplies the f32 atomic output traffic by sk,
      // which dominates on the (W1, W2, BS) weight-grad shapes.
      const int sk = splitk < 1 ? 1 : splitk;
      const int64_t tiles = (M / 256) * (N / 256) * n1 * n2 * sk;
      const double eff = (double)tiles / (((tiles + 255) / 256) * 256);
      if (tiles >= 192 && eff >= 0.9)
        return ob_gemm_bf16_nt_8ph(A, B, C, bias, residual, M, N, K, lda,
                                   ldb, ldc, strideA1, strideA2, strideB1,
                                   strideB2, strideC1, strideC2, n1, n2,
                                   alpha, beta, out_kind, sk, stream, M);
    }
    static const bool no256 = [] {
      const char* e = getenv("OB_BF16_NO256");
      return e && e[0] == '1';
    }();
    if (!no256 && M % 256 == 0 && K % 64 == 0 && K >= 1024) {
      // pick BN by scheduling-round efficiency (blocks / ceil-to-256):
      // e.g. fc (M=8192,N=3072): BN=256 -> 384 blocks = 1.5 rounds (75%),
      // BN=128 -> 768 blocks = 3 full rounds (100%)
      int bn2 = 0;
      double best_eff = 0.0;
      const int64_t zb = n1 * n2 * (splitk < 1 ? 1 : splitk);
      for (int cand : {256, 128}) {
        if (N % cand) continue;
        const int64_t blocks = (M / 256) * (N / cand) * zb;
        const double eff =
            (double)blocks / (((blocks + 255) / 256) * 256);
        if (eff > best_eff + 1e-9) {
          best_eff = eff;
          bn2 = cand;
        }
      }
      if (bn2) {
        const int64_t tiles = (M / 256) * (N / bn2) * zb;
        if (tiles >= 192)
          return ob_gemm_bf16_nt256_dispatch(
              A, B, C, bias, residual, M, N, K, lda, ldb, ldc, strideA1,
              strideA2, strideB1, strideB2, strideC1, strideC2, n1, n2, alpha,
              beta, out_kind, splitk, stream, M, bn2);
      }
    }
    return ob_gemm_bf16_nt_dispatch(A, B, C, bias, residual, M, N, K, lda,
                                    ldb, ldc, strideA1, strideA2, strideB1,
                                    strideB2, strideC1, strideC2, n1, n2,
                                    alpha, beta, out_kind, splitk, stream, M);
  }
  const int sel = (transA ? 2 : 0) | (transB ? 1 : 0);
  switch (sel) {
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

// ---------------------------------------------------------------------------
// f32 <-> bf16 helpers for the mixed-precision path
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_f32_to_bf16(const float* __restrict__ x,
                                                     __bf16* __restrict__ y,
                                                     int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * 256)
    y[i] = (__bf16)x[i];
}

// transposed cast: y[c][r] = x[r][c] for x [rows, cols]; y row stride
// out_ld >= rows (pad entries beyond rows are left untouched — zero the
// buffer once before the first call when out_ld > rows).
__global__ __launch_bounds__(256) void k_f32_to_bf16_t(const float* __restrict__ x,
                                                       __bf16* __restrict__ y,
                                                       int64_t rows,
                                                       int64_t cols,
                                                       int64_t out_ld) {
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < rows * cols;
       idx += (int64_t)gridDim.x * 256) {
    const int64_t r = idx / cols, c = idx % cols;
    y[c * out_ld + r] = (__bf16)x[r * cols + c];
  }
}

__global__ __launch_bounds__(256) void k_bf16_to_f32(const __bf16* __restrict__ x,
                                                     float* __restrict__ y,
                                                     int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * 256)
    y[i] = (float)x[i];
}

__host__ __device__ static inline int64_t bmin64(int64_t a, int64_t b) { return a < b ? a : b; }

extern "C" int ob_f32_to_bf16(const void* x, void* y, int64_t n, void* stream) {
  k_f32_to_bf16<<<(int)bmin64((n + 255) / 256, 4096), 256, 0, S(stream)>>>(
      (const float*)x, (__bf16*)y, n);
  OB_LAUNCH_CHECK();
  return 0;
}
extern "C" int ob_f32_to_bf16_t(const void* x, void* y, int64_t rows,
                                int64_t cols, void* stream) {
  k_f32_to_bf16_t<<<(int)bmin64((rows * cols + 255) / 256, 4096), 256, 0,
                    S(stream)>>>((const float*)x, (__bf16*)y, rows, cols,
                                 rows);
  OB_LAUNCH_CHECK();
  return 0;
}
extern "C" int ob_f32_to_bf16_t_ld(const void* x, void* y, int64_t rows,
                                   int64_t cols, int64_t out_ld,
                                   void* stream) {
  k_f32_to_bf16_t<<<(int)bmin64((rows * cols + 255) / 256, 4096), 256, 0,
                    S(stream)>>>((const float*)x, (__bf16*)y, rows, cols,
                                 out_ld);
  OB_LAUNCH_CHECK();
  return 0;
}
extern "C" int ob_bf16_to_f32(const void* x, void* y, int64_t n, void* stream) {
  k_bf16_to_f32<<<(int)bmin64((n + 255) / 256, 4096), 256, 0, S(stream)>>>(
      (const __bf16*)x, (float*)y, n);
  OB_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// bf16-I/O elementwise / reduction kernels (fp32 math, fp32 params & grads).
// Mirrors the fp32 kernels in ob_kernels.hip; separate instantiations keep
// the proven fp32 path untouched.
// ---------------------------------------------------------------------------

__device__ __forceinline__ float bwave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ float bblock_sum256(float v, float* lds4) {
  v = bwave_sum(v);
  const int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds4[wid] = v;
  __syncthreads();
  const float r = lds4[0] + lds4[1] + lds4[2] + lds4[3];
  __syncthreads();
  return r;
}
__device__ __forceinline__ float bblock_max256(float v, float* lds4) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off, 64));
  const int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds4[wid] = v;
  __syncthreads();
  const float r = fmaxf(fmaxf(lds4[0], lds4[1]), fmaxf(lds4[2], lds4[3]));
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void k_ln_fwd_bf16(
    const __bf16* __restrict__ x, const float* __restrict__ w,
    const float* __restrict__ b, __bf16* __restrict__ y,
    float* __restrict__ mean, float* __restrict__ rstd, int64_t rows, int H,
    float eps) {
  __shared__ float lds4[4];
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const __bf16* xr = x + row * H;
    float s = 0.f, sq = 0.f;
    for (int c = threadIdx.x; c < H; c += 256) {
      const float v = bf2f(xr[c]);
      s += v;
      sq += v * v;
    }
    const float mu = bblock_sum256(s, lds4) / H;
    const float var = bblock_sum256(sq, lds4) / H - mu * mu;
    const float rs = rsqrtf(var + eps);
    if (threadIdx.x == 0) {
      mean[row] = mu;
      rstd[row] = rs;
    }
    __bf16* yr = y + row * H;
    for (int c = threadIdx.x; c < H; c += 256)
      yr[c] = (__bf16)((bf2f(xr[c]) - mu) * rs * w[c] + b[c]);
    __syncthreads();
  }
}

// wave-per-row ln forward (H in [512, 1024]): no block barriers, 16-B
// loads; row reductions are wave shfl ladders (the block-per-row kernel
// measured ~4x off the HBM roofline at H=768).  COPY: the loaded row
// is also stored verbatim to xcopy (the layer's activation stash), which
// replaces a separate device-to-device copy of x.
template <bool COPY>
__global__ __launch_bounds__(256) void k_ln_fwd_bf16_w(
    const __bf16* __restrict__ x, const float* __restrict__ w,
    const float* __restrict__ b, __bf16* __restrict__ y,
    __bf16* __restrict__ xcopy, float* __restrict__ mean,
    float* __restrict__ rstd, int64_t rows, int H, float eps, int wrows) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int c0 = lane * 8, c1 = (lane + 64) * 8;
  const bool has1 = c1 < H;
  float wv0[8], bv0[8], wv1[8], bv1[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    wv0[j] = w[c0 + j];
    bv0[j] = b[c0 + j];
    wv1[j] = has1 ? w[c1 + j] : 0.f;
    bv1[j] = has1 ? b[c1 + j] : 0.f;
  }
  const int64_t r0 = (int64_t)blockIdx.x * (4 * wrows) + wid;
  // ROW PAIRS per iteration: the wave shfl reduction ladders of the two
  // rows interleave (ILP 4 on the shuffle latency) — the single-row
  // version measured 1.9 TB/s, shuffle-latency-bound, ~3x off roofline
  for (int i = 0; i < wrows; i += 2) {
    const int64_t rowa = r0 + (int64_t)i * 4;
    const int64_t rowb = r0 + (int64_t)(i + 1) * 4;
    if (rowa >= rows) return;
    const bool hb = rowb < rows;
    const __bf16* xa = x + rowa * H;
    const __bf16* xb = x + (hb ? rowb : rowa) * H;
    const uint4 xa0 = *reinterpret_cast<const uint4*>(xa + c0);
    const uint4 xb0 = *reinterpret_cast<const uint4*>(xb + c0);
    uint4 xa1 = {}, xb1 = {};
    if (has1) {
      xa1 = *reinterpret_cast<const uint4*>(xa + c1);
      xb1 = *reinterpret_cast<const uint4*>(xb + c1);
    }
    if (COPY) {
      *reinterpret_cast<uint4*>(xcopy + rowa * H + c0) = xa0;
      if (has1) *reinterpret_cast<uint4*>(xcopy + rowa * H + c1) = xa1;
      if (hb) {
        *reinterpret_cast<uint4*>(xcopy + rowb * H + c0) = xb0;
        if (has1) *reinterpret_cast<uint4*>(xcopy + rowb * H + c1) = xb1;
      }
    }
    float va0[8], va1[8], vb0[8], vb1[8];
    float sa = 0.f, sqa = 0.f, sb = 0.f, sqb = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      va0[j] = bf2f(bf_extract(xa0, j));
      vb0[j] = bf2f(bf_extract(xb0, j));
      sa += va0[j];
      sqa += va0[j] * va0[j];
      sb += vb0[j];
      sqb += vb0[j] * vb0[j];
    }
    if (has1) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        va1[j] = bf2f(bf_extract(xa1, j));
        vb1[j] = bf2f(bf_extract(xb1, j));
        sa += va1[j];
        sqa += va1[j] * va1[j];
        sb += vb1[j];
        sqb += vb1[j] * vb1[j];
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      sa += __shfl_xor(sa, o, 64);
      sqa += __shfl_xor(sqa, o, 64);
      sb += __shfl_xor(sb, o, 64);
      sqb += __shfl_xor(sqb, o, 64);
    }
    const float mua = sa / H, mub = sb / H;
    const float rsa = rsqrtf(sqa / H - mua * mua + eps);
    const float rsb = rsqrtf(sqb / H - mub * mub + eps);
    if (lane == 0) {
      mean[rowa] = mua;
      rstd[rowa] = rsa;
      if (hb) {
        mean[rowb] = mub;
        rstd[rowb] = rsb;
      }
    }
    __bf16 oa[16], ob[16];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      oa[j] = (__bf16)((va0[j] - mua) * rsa * wv0[j] + bv0[j]);
      ob[j] = (__bf16)((vb0[j] - mub) * rsb * wv0[j] + bv0[j]);
    }
    if (has1) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        oa[8 + j] = (__bf16)((va1[j] - mua) * rsa * wv1[j] + bv1[j]);
        ob[8 + j] = (__bf16)((vb1[j] - mub) * rsb * wv1[j] + bv1[j]);
      }
    }
    *reinterpret_cast<uint4*>(y + rowa * H + c0) =
        *reinterpret_cast<const uint4*>(&oa[0]);
    if (has1)
      *reinterpret_cast<uint4*>(y + rowa * H + c1) =
          *reinterpret_cast<const uint4*>(&oa[8]);
    if (hb) {
      *reinterpret_cast<uint4*>(y + rowb * H + c0) =
          *reinterpret_cast<const uint4*>(&ob[0]);
      if (has1)
        *reinterpret_cast<uint4*>(y + rowb * H + c1) =
            *reinterpret_cast<const uint4*>(&ob[8]);
    }
  }
}

// y = LN(x); when xcopy is non-null (and != x) it also receives a bit-exact
// copy of x.  x is read before either output row is written, and the kernel
// pointers are restrict-qualified: xcopy must not overlap y.
static bool ln_wave_width(int64_t H) {
  return H >= 512 && H <= 1024 && H % 8 == 0;
}

extern "C" int ob_layernorm_fwd_copy_bf16(const void* x, const void* w,
                                          const void* b, void* y, void* xcopy,
                                          void* mean, void* rstd,
                                          int64_t rows, int64_t H, float eps,
                                          void* stream) {
  if (xcopy == x) xcopy = nullptr;
  if (ln_wave_width(H)) {
    const int wrows = 4;
    const int grid = (int)((rows + 4 * wrows - 1) / (4 * wrows));
    if (xcopy)
      k_ln_fwd_bf16_w<true><<<grid, 256, 0, S(stream)>>>(
          (const __bf16*)x, (const float*)w, (const float*)b, (__bf16*)y,
          (__bf16*)xcopy, (float*)mean, (float*)rstd, rows, (int)H, eps,
          wrows);
    else
      k_ln_fwd_bf16_w<false><<<grid, 256, 0, S(stream)>>>(
          (const __bf16*)x, (const float*)w, (const float*)b, (__bf16*)y,
          nullptr, (float*)mean, (float*)rstd, rows, (int)H, eps, wrows);
    OB_LAUNCH_CHECK();
    return 0;
  }
  // other widths compose: copy, then the block-per-row kernel
  if (xcopy)
    OB_HIP(hipMemcpyAsync(xcopy, x, (size_t)(rows * H) * sizeof(__bf16),
                          hipMemcpyDeviceToDevice, S(stream)));
  return ob_layernorm_fwd_bf16(x, w, b, y, mean, rstd, rows, H, eps, stream);
}

extern "C" int ob_layernorm_fwd_bf16(const void* x, const void* w,
                                     const void* b, void* y, void* mean,
                                     void* rstd, int64_t rows, int64_t H,
                                     float eps, void* stream) {
  if (ln_wave_width(H))
    return ob_layernorm_fwd_copy_bf16(x, w, b, y, nullptr, mean, rstd, rows,
                                      H, eps, stream);
  const int grid = (int)bmin64(rows, 16384);
  k_ln_fwd_bf16<<<grid, 256, 0, S(stream)>>>(
      (const __bf16*)x, (const float*)w, (const float*)b, (__bf16*)y,
      (float*)mean, (float*)rstd, rows, (int)H, eps);
  OB_LAUNCH_CHECK();
  return 0;
}

#define BLN_CHUNK 16
template <bool DX_ACCUM>
__global__ __launch_bounds__(256) void k_ln_bwd_bf16(
    const __bf16* __restrict__ x, const float* __restrict__ w,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const __bf16* __restrict__ dy, __bf16* __restrict__ dx,
    float* __restrict__ dw, float* __restrict__ db, int64_t rows, int H) {
  __shared__ float lds4[4];
  const int64_t r0 = (int64_t)blockIdx.x * BLN_CHUNK;
  float accw[8] = {0}, accb[8] = {0};
  const int64_t rend = bmin64(rows, r0 + BLN_CHUNK);
  for (int64_t row = r0; row < rend; ++row) {
    const __bf16* xr = x + row * H;
    const __bf16* dyr = dy + row * H;
    const float mu = mean[row], rs = rstd[row];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = threadIdx.x + j * 256;
      if (c < H) {
        const float xhat = (bf2f(xr[c]) - mu) * rs;
        const float dyv = bf2f(dyr[c]);
        const float dyw = dyv * w[c];
        s1 += dyw * xhat;
        s2 += dyw;
        accw[j] += dyv * xhat;
        accb[j] += dyv;
      }
    }
    const float m1 = bblock_sum256(s1, lds4) / H;
    const float m2 = bblock_sum256(s2, lds4) / H;
    __bf16* dxr = dx + row * H;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = threadIdx.x + j * 256;
      if (c < H) {
        const float xhat = (bf2f(xr[c]) - mu) * rs;
        const float v = rs * (bf2f(dyr[c]) * w[c] - m2 - xhat * m1);
        dxr[c] = (__bf16)(DX_ACCUM ? bf2f(dxr[c]) + v : v);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = threadIdx.x + j * 256;
    if (c < H) {
      atomicAdd(&dw[c], accw[j]);
      atomicAdd(&db[c], accb[j]);
    }
  }
}

extern "C" int ob_layernorm_bwd_bf16(const void* x, const void* w,
                                     const void* mean, const void* rstd,
                                     const void* dy, void* dx, void* dw,
                                     void* db, int64_t rows, int64_t H,
                                     int dx_accum, void* stream) {
  if (H > 2048) return ob_fail("ln_bwd_bf16: H > 2048 unsupported");
  if (H % 8) return ob_fail("ln_bwd_bf16: H must be a multiple of 8");
  if (H >= 512 && H <= 1024)
    return ob_layernorm_bwd_res_bf16(x, w, mean, rstd, dy,
                                     dx_accum ? dx : nullptr, dx, dw, db,
                                     nullptr, nullptr, rows, H, stream);
  const int grid = (int)((rows + BLN_CHUNK - 1) / BLN_CHUNK);
  if (dx_accum)
    k_ln_bwd_bf16<true><<<grid, 256, 0, S(stream)>>>(
        (const __bf16*)x, (const float*)w, (const float*)mean,
        (const float*)rstd, (const __bf16*)dy, (__bf16*)dx, (float*)dw,
        (float*)db, rows, (int)H);
  else
    k_ln_bwd_bf16<false><<<grid, 256, 0, S(stream)>>>(
        (const __bf16*)x, (const float*)w, (const float*)mean,
        (const float*)rstd, (const __bf16*)dy, (__bf16*)dx, (float*)dw,
        (float*)db, rows, (int)H);
  OB_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// Fused ln backward: dx = bf16(res + v) with a separate read-only residual
// source, plus two optional bias-grad side sums taken from registers:
// sres += colsum(res), sdx += colsum(dx as rounded to bf16).  res may alias
// dx (every element is read and written by the same lane), so neither is
// restrict-qualified.
//
// Wave-per-row (H in [512, 1024]): a wave owns its rows outright, the row
// reductions are wave shfl ladders over ROW PAIRS (two rows' ladders
// interleave), 16-B vector loads throughout.  8 waves per block, two row
// pairs per wave (32 rows per block, two waves per SIMD): the kernel is
// bound by the load -> ladder -> store latency chain, not by bytes, so it
// wants more rows in flight per CU than the 4-wave, four-pairs-in-sequence
// kernel it replaces (figures in DESIGN.md).  The column accumulators (dw,
// db, sres, sdx) fold lane registers -> one LDS row per wave -> one global
// atomic per column per block.
// ---------------------------------------------------------------------------
#define BLNR_WAVES 8
#define BLNR_WROWS 4
#define BLNR_ROWS (BLNR_WAVES * BLNR_WROWS)
#define BLNR_MAXGRID 1024

template <bool HAS_RES, bool SUMS>
__global__ __launch_bounds__(64 * BLNR_WAVES) void k_ln_bwd_bf16_rs(
    const __bf16* __restrict__ x, const float* __restrict__ w,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const __bf16* __restrict__ dy, const __bf16* res, __bf16* dx,
    float* o0, float* o1, float* o2, float* o3, int64_t rows, int H) {
  constexpr int NV = SUMS ? 4 : 2;
  constexpr int UNR = (SUMS && HAS_RES) ? 1 : 2;
  __shared__ float red[BLNR_WAVES][1024];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int c0 = lane * 8, c1 = (lane + 64) * 8;
  const bool has1 = c1 < H;
  float acc[4][2][8] = {};  // dw, db, sres, sdx
  float(&accw)[2][8] = acc[0];
  float(&accb)[2][8] = acc[1];
  float(&accr)[2][8] = acc[2];
  float(&accx)[2][8] = acc[3];
  float wv0[8], wv1[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    wv0[j] = w[c0 + j];
    wv1[j] = has1 ? w[c1 + j] : 0.f;
  }
  const int64_t nchunks = (rows + BLNR_ROWS - 1) / BLNR_ROWS;
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int64_t r0 = chunk * BLNR_ROWS + wid;
    // the two pairs unroll (loads of the second hoist over the first's
    // math) except with all four accumulator sets live, which would spill
#pragma unroll UNR
    for (int i = 0; i < BLNR_WROWS; i += 2) {
      const int64_t rowa = r0 + (int64_t)i * BLNR_WAVES;
      const int64_t rowb = r0 + (int64_t)(i + 1) * BLNR_WAVES;
      if (rowa >= rows) break;
      const bool hb = rowb < rows;
      const int64_t oa = rowa * H, ob = (hb ? rowb : rowa) * H;
      const float mua = mean[rowa], rsa = rstd[rowa];
      const float mub = hb ? mean[rowb] : 0.f, rsb = hb ? rstd[rowb] : 0.f;
      const uint4 xa0 = *reinterpret_cast<const uint4*>(x + oa + c0);
      const uint4 ya0 = *reinterpret_cast<const uint4*>(dy + oa + c0);
      const uint4 xb0 = *reinterpret_cast<const uint4*>(x + ob + c0);
      const uint4 yb0 = *reinterpret_cast<const uint4*>(dy + ob + c0);
      uint4 xa1 = {}, ya1 = {}, xb1 = {}, yb1 = {};
      uint4 ra0 = {}, rb0 = {}, ra1 = {}, rb1 = {};
      if (HAS_RES) {
        ra0 = *reinterpret_cast<const uint4*>(res + oa + c0);
        rb0 = *reinterpret_cast<const uint4*>(res + ob + c0);
      }
      if (has1) {
        xa1 = *reinterpret_cast<const uint4*>(x + oa + c1);
        ya1 = *reinterpret_cast<const uint4*>(dy + oa + c1);
        xb1 = *reinterpret_cast<const uint4*>(x + ob + c1);
        yb1 = *reinterpret_cast<const uint4*>(dy + ob + c1);
        if (HAS_RES) {
          ra1 = *reinterpret_cast<const uint4*>(res + oa + c1);
          rb1 = *reinterpret_cast<const uint4*>(res + ob + c1);
        }
      }
      float s1a = 0.f, s2a = 0.f, s1b = 0.f, s2b = 0.f;
      float xha0[8], dya0[8], xha1[8], dya1[8];
      float xhb0[8], dyb0[8], xhb1[8], dyb1[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        xha0[j] = (bf2f(bf_extract(xa0, j)) - mua) * rsa;
        dya0[j] = bf2f(bf_extract(ya0, j));
        xhb0[j] = (bf2f(bf_extract(xb0, j)) - mub) * rsb;
        dyb0[j] = bf2f(bf_extract(yb0, j));
        s1a += dya0[j] * wv0[j] * xha0[j];
        s2a += dya0[j] * wv0[j];
        s1b += dyb0[j] * wv0[j] * xhb0[j];
        s2b += dyb0[j] * wv0[j];
        accw[0][j] += dya0[j] * xha0[j];
        accb[0][j] += dya0[j];
        if (hb) {
          accw[0][j] += dyb0[j] * xhb0[j];
          accb[0][j] += dyb0[j];
        }
      }
      if (has1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          xha1[j] = (bf2f(bf_extract(xa1, j)) - mua) * rsa;
          dya1[j] = bf2f(bf_extract(ya1, j));
          xhb1[j] = (bf2f(bf_extract(xb1, j)) - mub) * rsb;
          dyb1[j] = bf2f(bf_extract(yb1, j));
          s1a += dya1[j] * wv1[j] * xha1[j];
          s2a += dya1[j] * wv1[j];
          s1b += dyb1[j] * wv1[j] * xhb1[j];
          s2b += dyb1[j] * wv1[j];
          accw[1][j] += dya1[j] * xha1[j];
          accb[1][j] += dya1[j];
          if (hb) {
            accw[1][j] += dyb1[j] * xhb1[j];
            accb[1][j] += dyb1[j];
          }
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        s1a += __shfl_xor(s1a, o, 64);
        s2a += __shfl_xor(s2a, o, 64);
        s1b += __shfl_xor(s1b, o, 64);
        s2b += __shfl_xor(s2b, o, 64);
      }
      const float m1a = s1a / H, m2a = s2a / H;
      const float m1b = s1b / H, m2b = s2b / H;
      float oxa[16], oxb[16];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float ra = HAS_RES ? bf2f(bf_extract(ra0, j)) : 0.f;
        const float rb = HAS_RES ? bf2f(bf_extract(rb0, j)) : 0.f;
        // round to bf16 here: sdx sums exactly what is stored
        oxa[j] = bf2f((__bf16)(
            ra + rsa * (dya0[j] * wv0[j] - m2a - xha0[j] * m1a)));
        oxb[j] = bf2f((__bf16)(
            rb + rsb * (dyb0[j] * wv0[j] - m2b - xhb0[j] * m1b)));
        if (SUMS) {
          accr[0][j] += ra;
          accx[0][j] += oxa[j];
          if (hb) {
            accr[0][j] += rb;
            accx[0][j] += oxb[j];
          }
        }
      }
      if (has1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float ra = HAS_RES ? bf2f(bf_extract(ra1, j)) : 0.f;
          const float rb = HAS_RES ? bf2f(bf_extract(rb1, j)) : 0.f;
          oxa[8 + j] = bf2f((__bf16)(
              ra + rsa * (dya1[j] * wv1[j] - m2a - xha1[j] * m1a)));
          oxb[8 + j] = bf2f((__bf16)(
              rb + rsb * (dyb1[j] * wv1[j] - m2b - xhb1[j] * m1b)));
          if (SUMS) {
            accr[1][j] += ra;
            accx[1][j] += oxa[8 + j];
            if (hb) {
              accr[1][j] += rb;
              accx[1][j] += oxb[8 + j];
            }
          }
        }
      }
      *reinterpret_cast<uint4*>(dx + oa + c0) = bf_pack8(&oxa[0]);
      if (has1) *reinterpret_cast<uint4*>(dx + oa + c1) = bf_pack8(&oxa[8]);
      if (hb) {
        *reinterpret_cast<uint4*>(dx + ob + c0) = bf_pack8(&oxb[0]);
        if (has1) *reinterpret_cast<uint4*>(dx + ob + c1) = bf_pack8(&oxb[8]);
      }
    }
  }
  // per vector: every wave parks its lane accumulators in its own LDS row
  // (16-B stores), then the block folds the 8 rows column-wise and adds
  // one value per column to the fp32 vector (null: not asked for)
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const float(&a0)[8] = acc[v][0];
    const float(&a1)[8] = acc[v][1];
    float* const out = v == 0 ? o0 : v == 1 ? o1 : v == 2 ? o2 : o3;
    *reinterpret_cast<float4*>(&red[wid][c0]) =
        make_float4(a0[0], a0[1], a0[2], a0[3]);
    *reinterpret_cast<float4*>(&red[wid][c0 + 4]) =
        make_float4(a0[4], a0[5], a0[6], a0[7]);
    if (has1) {
      *reinterpret_cast<float4*>(&red[wid][c1]) =
          make_float4(a1[0], a1[1], a1[2], a1[3]);
      *reinterpret_cast<float4*>(&red[wid][c1 + 4]) =
          make_float4(a1[4], a1[5], a1[6], a1[7]);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < H; c += 64 * BLNR_WAVES) {
      float t = 0.f;
#pragma unroll
      for (int k = 0; k < BLNR_WAVES; ++k) t += red[k][c];
      if (out) atomicAdd(&out[c], t);
    }
    __syncthreads();
  }
}

// dx = bf16(res + ln_bwd(x, dy)) (res null: no residual; res may equal dx);
// dw/db += as ob_layernorm_bwd_bf16; sum_res += colsum(res) and sum_dx +=
// colsum(dx) when non-null.  Widths outside the wave path compose the
// unfused kernels and give the same results.
extern "C" int ob_layernorm_bwd_res_bf16(const void* x, const void* w,
                                         const void* mean, const void* rstd,
                                         const void* dy, const void* res,
                                         void* dx, void* dw, void* db,
                                         void* sum_res, void* sum_dx,
                                         int64_t rows, int64_t H,
                                         void* stream) {
  if (H > 2048) return ob_fail("ln_bwd_bf16: H > 2048 unsupported");
  if (H % 8) return ob_fail("ln_bwd_bf16: H must be a multiple of 8");
  if (sum_res && !res) return ob_fail("ln_bwd_res_bf16: sum_res needs res");
  if (rows <= 0) return 0;
  if (H >= 512 && H <= 1024) {
    const bool sums = sum_res || sum_dx;
    const int64_t nchunks = (rows + BLNR_ROWS - 1) / BLNR_ROWS;
    const int grid = (int)bmin64(nchunks, BLNR_MAXGRID);
#define OB_LNRS(R_, S_)                                                     \
  k_ln_bwd_bf16_rs<R_, S_><<<grid, 64 * BLNR_WAVES, 0, S(stream)>>>(        \
      (const __bf16*)x, (const float*)w, (const float*)mean,                \
      (const float*)rstd, (const __bf16*)dy, (const __bf16*)res,            \
      (__bf16*)dx, (float*)dw, (float*)db, (float*)sum_res, (float*)sum_dx, \
      rows, (int)H)
    if (res) {
      if (sums) OB_LNRS(true, true);
      else OB_LNRS(true, false);
    } else {
      if (sums) OB_LNRS(false, true);
      else OB_LNRS(false, false);
    }
#undef OB_LNRS
    OB_LAUNCH_CHECK();
    return 0;
  }
  // composed path: colsum(res) first (res may alias dx), copy, ln, colsum
  if (sum_res && ob_colsum_bf16(res, sum_res, rows, H, stream)) return 1;
  if (res && res != dx)
    OB_HIP(hipMemcpyAsync(dx, res, (size_t)(rows * H) * sizeof(__bf16),
                          hipMemcpyDeviceToDevice, S(stream)));
  if (ob_layernorm_bwd_bf16(x, w, mean, rstd, dy, dx, dw, db, rows, H,
                            res ? 1 : 0, stream))
    return 1;
  if (sum_dx && ob_colsum_bf16(dx, sum_dx, rows, H, stream)) return 1;
  return 0;
}

__global__ __launch_bounds__(256) void k_softmax_fwd_bf16(
    __bf16* __restrict__ scores, int Sq, float scale) {
  __shared__ float lds4[4];
  const int64_t rid = blockIdx.x;
  const int row = (int)(rid % Sq);
  __bf16* p = scores + rid * Sq;
  const int valid = row + 1;
  float v[8];
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = threadIdx.x + j * 256;
    v[j] = (c < valid) ? bf2f(p[c]) * scale : -INFINITY;
    mx = fmaxf(mx, v[j]);
  }
  mx = bblock_max256(mx, lds4);
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = (v[j] == -INFINITY) ? 0.f : __expf(v[j] - mx);
    sum += v[j];
  }
  sum = bblock_sum256(sum, lds4);
  const float inv = 1.f / sum;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = threadIdx.x + j * 256;
    if (c < Sq) p[c] = (__bf16)(v[j] * inv);
  }
}



__device__ __forceinline__ uint4 bf_pack8_(const float* v) {
  return bf_pack8(v);
}

__global__ __launch_bounds__(256) void k_softmax_fwd_bf16_v8(
    __bf16* __restrict__ scores, int Sq, float scale) {
  __shared__ float lds4[4];
  const int64_t rid = blockIdx.x;
  const int row = (int)(rid % Sq);
  __bf16* p = scores + rid * Sq;
  const int valid = row + 1;
  const int c8 = threadIdx.x * 8;
  float v[8];
  uint4 in = {0, 0, 0, 0};
  if (c8 < Sq) in = *reinterpret_cast<const uint4*>(p + c8);
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = (c8 + j < valid) ? bf2f(bf_extract(in, j)) * scale : -INFINITY;
    mx = fmaxf(mx, v[j]);
  }
  mx = bblock_max256(mx, lds4);
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = (v[j] == -INFINITY) ? 0.f : __expf(v[j] - mx);
    sum += v[j];
  }
  sum = bblock_sum256(sum, lds4);
  const float inv = 1.f / sum;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] *= inv;
  if (c8 < Sq) *reinterpret_cast<uint4*>(p + c8) = bf_pack8(v);
}

extern "C" int ob_softmax_causal_fwd_bf16(void* scores, int64_t batch,
                                          int64_t Sq, float scale,
                                          void* stream) {
  if (Sq > 2048) return ob_fail("softmax_bf16: S > 2048 unsupported");
  if (Sq % 8 == 0)
    k_softmax_fwd_bf16_v8<<<(unsigned)(batch * Sq), 256, 0, S(stream)>>>(
        (__bf16*)scores, (int)Sq, scale);
  else
    k_softmax_fwd_bf16<<<(unsigned)(batch * Sq), 256, 0, S(stream)>>>(
        (__bf16*)scores, (int)Sq, scale);
  OB_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(256) void k_softmax_bwd_bf16(
    const __bf16* __restrict__ P, __bf16* __restrict__ dP, int Sq) {
  __shared__ float lds4[4];
  const int64_t rid = blockIdx.x;
  const int row = (int)(rid % Sq);
  const __bf16* pr = P + rid * Sq;
  __bf16* dr = dP + rid * Sq;
  const int valid = row + 1;
  float pv[8], dv[8];
  float t = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = threadIdx.x + j * 256;
    pv[j] = (c < valid) ? bf2f(pr[c]) : 0.f;
    dv[j] = (c < valid) ? bf2f(dr[c]) : 0.f;
    t += pv[j] * dv[j];
  }
  t = bblock_sum256(t, lds4);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = threadIdx.x + j * 256;
    if (c < Sq) dr[c] = (__bf16)(pv[j] * (dv[j] - t));
  }
}

__global__ __launch_bounds__(256) void k_softmax_bwd_bf16_v8(
    const __bf16* __restrict__ P, __bf16* __restrict__ dP, int Sq) {
  __shared__ float lds4[4];
  const int64_t rid = blockIdx.x;
  const int row = (int)(rid % Sq);
  const __bf16* pr = P + rid * Sq;
  __bf16* dr = dP + rid * Sq;
  const int valid = row + 1;
  const int c8 = threadIdx.x * 8;
  uint4 pin = {0, 0, 0, 0}, din = {0, 0, 0, 0};
  if (c8 < Sq) {
    pin = *reinterpret_cast<const uint4*>(pr + c8);
    din = *reinterpret_cast<const uint4*>(dr + c8);
  }
  float pv[8], dv[8];
  float t = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    pv[j] = (c8 + j < valid) ? bf2f(bf_extract(pin, j)) : 0.f;
    dv[j] = (c8 + j < valid) ? bf2f(bf_extract(din, j)) : 0.f;
    t += pv[j] * dv[j];
  }
  t = bblock_sum256(t, lds4);
  float out[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) out[j] = pv[j] * (dv[j] - t);
  if (c8 < Sq) *reinterpret_cast<uint4*>(dr + c8) = bf_pack8(out);
}

extern "C" int ob_softmax_causal_bwd_bf16(const void* P, void* dP,
                                          int64_t batch, int64_t Sq,
                                          void* stream) {
  if (Sq > 2048) return ob_fail("softmax_bwd_bf16: S > 2048 unsupported");
  if (Sq % 8 == 0)
    k_softmax_bwd_bf16_v8<<<(unsigned)(batch * Sq), 256, 0, S(stream)>>>(
        (const __bf16*)P, (__bf16*)dP, (int)Sq);
  else
    k_softmax_bwd_bf16<<<(unsigned)(batch * Sq), 256, 0, S(stream)>>>(
        (const __bf16*)P, (__bf16*)dP, (int)Sq);
  OB_LAUNCH_CHECK();
  return 0;
}

#define BGELU_K 0.7978845608028654f
#define BGELU_C 0.044715f

// 8-wide (uint4) gelu: bf16 scalar loads cost ~2-2.5x (guide G13)
__global__ __launch_bounds__(256) void k_gelu_fwd_bf16(
    const __bf16* __restrict__ u, __bf16* __restrict__ g, int64_t n8) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8;
       i += (int64_t)gridDim.x * 256) {
    const uint4 in = *reinterpret_cast<const uint4*>(u + i * 8);
    float out[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float x = bf2f(bf_extract(in, j));
      const float t = tanhf(BGELU_K * (x + BGELU_C * x * x * x));
      out[j] = 0.5f * x * (1.f + t);
    }
    *reinterpret_cast<uint4*>(g + i * 8) = bf_pack8_(out);
  }
}
__global__ __launch_bounds__(256) void k_gelu_bwd_bf16(
    const __bf16* __restrict__ u, const __bf16* __restrict__ dg,
    __bf16* __restrict__ du, int64_t n8) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8;
       i += (int64_t)gridDim.x * 256) {
    const uint4 uin = *reinterpret_cast<const uint4*>(u + i * 8);
    const uint4 gin = *reinterpret_cast<const uint4*>(dg + i * 8);
    float out[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float x = bf2f(bf_extract(uin, j));
      const float t = tanhf(BGELU_K * (x + BGELU_C * x * x * x));
      const float d = 0.5f * (1.f + t) +
                      0.5f * x * (1.f - t * t) * BGELU_K *
                          (1.f + 3.f * BGELU_C * x * x);
      out[j] = bf2f(bf_extract(gin, j)) * d;
    }
    *reinterpret_cast<uint4*>(du + i * 8) = bf_pack8_(out);
  }
}
extern "C" int ob_gelu_fwd_bf16(const void* u, void* g, int64_t n,
                                void* stream) {
  if (n % 8) return ob_fail("gelu_bf16: n must be a multiple of 8");
  k_gelu_fwd_bf16<<<(int)bmin64((n / 8 + 255) / 256, 2048), 256, 0,
                    S(stream)>>>((const __bf16*)u, (__bf16*)g, n / 8);
  OB_LAUNCH_CHECK();
  return 0;
}
extern "C" int ob_gelu_bwd_bf16(const void* u, const void* dg, void* du,
                                int64_t n, void* stream) {
  if (n % 8) return ob_fail("gelu_bf16: n must be a multiple of 8");
  k_gelu_bwd_bf16<<<(int)bmin64((n / 8 + 255) / 256, 2048), 256, 0,
                    S(stream)>>>((const __bf16*)u, (const __bf16*)dg,
                                 (__bf16*)du, n / 8);
  OB_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(256) void k_colsum_bf16(
    const __bf16* __restrict__ X, float* __restrict__ db, int64_t M,
    int64_t N) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  const int64_t r0 = (int64_t)blockIdx.y * 256;
  const int64_t r1 = bmin64(M, r0 + 256);
  float acc = 0.f;
  for (int64_t r = r0; r < r1; ++r) acc += bf2f(X[r * N + c]);
  atomicAdd(&db[c], acc);
}
// vectorized: each thread owns 8 contiguous columns (one uint4 per row)
__global__ __launch_bounds__(256) void k_colsum_bf16_v8(
    const __bf16* __restrict__ X, float* __restrict__ db, int64_t M,
    int64_t N) {
  const int64_t c8 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
  if (c8 >= N) return;
  const int64_t r0 = (int64_t)blockIdx.y * 64;
  const int64_t r1 = bmin64(M, r0 + 64);
  float acc[8] = {0};
  for (int64_t r = r0; r < r1; ++r) {
    const uint4 v = *reinterpret_cast<const uint4*>(X + r * N + c8);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += bf2f(bf_extract(v, j));
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) atomicAdd(&db[c8 + j], acc[j]);
}

// two-level column sum (v9): block = 8 col-threads x 32 row-threads over
// a 64-col x 128-row tile; each thread keeps 4 independent uint4 loads
// in flight (the v8 kernel's single serial load stream measured ~640
// GB/s); wave shfl + LDS tree reduction, ONE global atomic per column
// per block.
__global__ __launch_bounds__(256) void k_colsum_bf16_v9(
    const __bf16* __restrict__ X, float* __restrict__ db, int64_t M,
    int64_t N) {
  __shared__ float red[4][64];
  const int tid = threadIdx.x;
  const int cg = tid & 7, rt = tid >> 3;       // col-thread, row-thread
  const int lane = tid & 63, w = tid >> 6;
  const int64_t c0 = (int64_t)blockIdx.x * 64 + cg * 8;
  const int64_t r0 = (int64_t)blockIdx.y * 128 + rt;
  float acc[8] = {0};
  if (c0 + 7 < N) {
    const __bf16* Xp = X + r0 * N + c0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t r = r0 + i * 32;
      if (r < M) {
        const uint4 v = *reinterpret_cast<const uint4*>(Xp + (int64_t)i * 32 * N);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += bf2f(bf_extract(v, j));
      }
    }
  } else if (c0 < N) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t r = r0 + i * 32;
      if (r < M)
        for (int j = 0; j < (int)(N - c0); ++j)
          acc[j] += bf2f(X[r * N + c0 + j]);
    }
  }
  // wave: fold the 8 row-slots (lanes cg+8*s, s=0..7)
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    acc[j] += __shfl_down(acc[j], 32, 64);
    acc[j] += __shfl_down(acc[j], 16, 64);
    acc[j] += __shfl_down(acc[j], 8, 64);
  }
  if (lane < 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[w][lane * 8 + j] = acc[j];
  }
  __syncthreads();
  // first 64 threads: fold 4 waves, one atomic per column
  if (tid < 64) {
    const int64_t c = (int64_t)blockIdx.x * 64 + tid;
    if (c < N)
      atomicAdd(&db[c],
                red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid]);
  }
}

extern "C" int ob_colsum_bf16(const void* X, void* db, int64_t M, int64_t N,
                              void* stream) {
  if (N % 8 == 0) {
    dim3 grid((unsigned)((N + 63) / 64), (unsigned)((M + 127) / 128));
    k_colsum_bf16_v9<<<grid, 256, 0, S(stream)>>>((const __bf16*)X,
                                                  (float*)db, M, N);
  } else {
    dim3 grid((unsigned)((N + 255) / 256), (unsigned)((M + 255) / 256));
    k_colsum_bf16<<<grid, 256, 0, S(stream)>>>((const __bf16*)X, (float*)db,
                                               M, N);
  }
  OB_LAUNCH_CHECK();
  return 0;
}

// gelu backward fused with the bias grad of the GEMM that produced u:
// du = dg * gelu'(u) and db[c] += sum_r du[r][c], summed over the
// bf16-rounded du (what ob_colsum_bf16(du) summed).  Block = 16 col-threads
// x 16 row-threads over a 128-col x 128-row tile; a thread owns 8 fixed
// columns and keeps 4 rows (8 independent 16-B loads) in flight.  Column
// partials go registers -> wave shfl -> LDS -> one atomic per column per
// block.  du may alias dg (same lane reads and writes an element).
#define BGC_ROWS 128
// gelu'(x) with tanh(z) = 1 - 2 / (1 + exp(2z)) on the hardware exp2 / rcp
// (about 15 VALU ops against about 45 for the branchy library tanhf: at
// [8192, 3072] the library form makes the kernel VALU-bound).
// t enters d only added to O(1) terms, so the ~1e-7 absolute error of the
// fast form is far below the bf16 rounding of du; exp2 overflow gives
// rcp(inf) = 0, t = 1, and 1 - t*t = 0 (no inf * 0).
__device__ __forceinline__ float bgelu_grad_fast(float x) {
  constexpr float L2E2 = 2.8853900817779268f;  // 2 * log2(e)
  const float x2 = x * x;
  const float e = __builtin_amdgcn_exp2f(
      x * (BGELU_K * L2E2 + BGELU_K * BGELU_C * L2E2 * x2));
  const float t = 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + e);
  return 0.5f * (1.f + t) + 0.5f * x * (1.f - t * t) *
                                (BGELU_K + 3.f * BGELU_K * BGELU_C * x2);
}
__global__ __launch_bounds__(256) void k_gelu_bwd_cs_bf16(
    const __bf16* __restrict__ u, const __bf16* dg, __bf16* du,
    float* __restrict__ db, int64_t M, int64_t N) {
  __shared__ float red[4][128];
  const int tid = threadIdx.x;
  const int cg = tid & 15, rt = tid >> 4;  // col-thread, row-thread
  const int lane = tid & 63, wv = tid >> 6;
  const int64_t c0 = (int64_t)blockIdx.x * 128 + cg * 8;
  const int64_t rbase = (int64_t)blockIdx.y * BGC_ROWS + rt;
  float acc[8] = {0};
  if (c0 < N) {  // N % 8 == 0: the whole 8-column group is in range
    for (int it = 0; it < BGC_ROWS / 64; ++it) {
      uint4 uin[4] = {}, gin[4] = {};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t r = rbase + it * 64 + i * 16;
        if (r < M) {
          uin[i] = *reinterpret_cast<const uint4*>(u + r * N + c0);
          gin[i] = *reinterpret_cast<const uint4*>(dg + r * N + c0);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t r = rbase + it * 64 + i * 16;
        if (r < M) {
          float out[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float x = bf2f(bf_extract(uin[i], j));
            const float d = bgelu_grad_fast(x);
            out[j] = bf2f((__bf16)(bf2f(bf_extract(gin[i], j)) * d));
            acc[j] += out[j];
          }
          *reinterpret_cast<uint4*>(du + r * N + c0) = bf_pack8_(out);
        }
      }
    }
  }
  // wave: fold the 4 row-slots (lanes cg + 16*s, s = 0..3)
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    acc[j] += __shfl_down(acc[j], 32, 64);
    acc[j] += __shfl_down(acc[j], 16, 64);
  }
  if (lane < 16) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[wv][lane * 8 + j] = acc[j];
  }
  __syncthreads();
  if (tid < 128) {
    const int64_t c = (int64_t)blockIdx.x * 128 + tid;
    if (c < N)
      atomicAdd(&db[c],
                red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid]);
  }
}

extern "C" int ob_gelu_bwd_colsum_bf16(const void* u, const void* dg,
                                       void* du, void* db, int64_t M,
                                       int64_t N, void* stream) {
  if (M <= 0 || N <= 0) return 0;
  if (N % 8 == 0) {
    dim3 grid((unsigned)((N + 127) / 128),
              (unsigned)((M + BGC_ROWS - 1) / BGC_ROWS));
    k_gelu_bwd_cs_bf16<<<grid, 256, 0, S(stream)>>>(
        (const __bf16*)u, (const __bf16*)dg, (__bf16*)du, (float*)db, M, N);
    OB_LAUNCH_CHECK();
    return 0;
  }
  // other widths compose the unfused kernels
  if (ob_gelu_bwd_bf16(u, dg, du, M * N, stream)) return 1;
  return ob_colsum_bf16(du, db, M, N, stream);
}

__global__ __launch_bounds__(256) void k_embed_fwd_bf16(
    const int64_t* __restrict__ ids, const float* __restrict__ wte,
    const float* __restrict__ wpe, __bf16* __restrict__ out, int64_t BS,
    int Sq, int H) {
  for (int64_t row = blockIdx.x; row < BS; row += gridDim.x) {
    const int64_t id = ids[row];
    const int s = (int)(row % Sq);
    const float* te = wte + id * H;
    const float* pe = wpe + (int64_t)s * H;
    __bf16* o = out + row * H;
    for (int c = threadIdx.x; c < H; c += 256) o[c] = (__bf16)(te[c] + pe[c]);
  }
}
extern "C" int ob_embed_fwd_bf16(const void* ids, const void* wte,
                                 const void* wpe, void* out, int64_t B,
                                 int64_t Sq, int64_t H, void* stream) {
  k_embed_fwd_bf16<<<(int)bmin64(B * Sq, 16384), 256, 0, S(stream)>>>(
      (const int64_t*)ids, (const float*)wte, (const float*)wpe, (__bf16*)out,
      B * Sq, (int)Sq, (int)H);
  OB_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(256) void k_embed_bwd_bf16(
    const int64_t* __restrict__ ids, const __bf16* __restrict__ dout,
    float* __restrict__ dwte, float* __restrict__ dwpe, int64_t BS, int Sq,
    int H) {
  for (int64_t row = blockIdx.x; row < BS; row += gridDim.x) {
    const int64_t id = ids[row];
    const int s = (int)(row % Sq);
    const __bf16* d = dout + row * H;
    for (int c = threadIdx.x; c < H; c += 256) {
      const float v = bf2f(d[c]);
      atomicAdd(&dwte[id * H + c], v);
      atomicAdd(&dwpe[(int64_t)s * H + c], v);
    }
  }
}
extern "C" int ob_embed_bwd_bf16(const void* ids, const void* dout, void* dwte,
                                 void* dwpe, int64_t B, int64_t Sq, int64_t H,
                                 void* stream) {
  k_embed_bwd_bf16<<<(int)bmin64(B * Sq, 16384), 256, 0, S(stream)>>>(
      (const int64_t*)ids, (const __bf16*)dout, (float*)dwte, (float*)dwpe,
      B * Sq, (int)Sq, (int)H);
  OB_LAUNCH_CHECK();
  return 0;
}

// CE with bf16 logits at row stride ld (padded to 8-half alignment); the
// shift/mean semantics match the fp32 kernels.
__global__ __launch_bounds__(256) void k_ce_fwd_bf16(
    const __bf16* __restrict__ logits, const int64_t* __restrict__ labels,
    float* __restrict__ lse, float* __restrict__ loss, int64_t BS, int Sq,
    int V, int64_t ld) {
  __shared__ float lmax[4], lsum[4];
  for (int64_t row = blockIdx.x; row < BS; row += gridDim.x) {
    const __bf16* lr = logits + row * ld;
    float m = -INFINITY, s = 0.f;
    // 16-B loads (scalar bf16 loads measured 3.6x off the HBM roofline);
    // pad columns (c >= V) masked out of the online max/sum
    for (int64_t c8 = (int64_t)threadIdx.x * 8; c8 < ld; c8 += 256 * 8) {
      const uint4 in = *reinterpret_cast<const uint4*>(lr + c8);
      float x[8];
      float m8 = -INFINITY;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        x[j] = (c8 + j < V) ? bf2f(bf_extract(in, j)) : -INFINITY;
        m8 = fmaxf(m8, x[j]);
      }
      if (m8 > -INFINITY) {
        const float nm = fmaxf(m, m8);
        float add = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          add += (x[j] > -INFINITY) ? __expf(x[j] - nm) : 0.f;
        s = (m > -INFINITY ? s * __expf(m - nm) : 0.f) + add;
        m = nm;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float om = __shfl_down(m, off, 64);
      const float os = __shfl_down(s, off, 64);
      const float nm = fmaxf(m, om);
      const float t1 = (m > -INFINITY) ? s * __expf(m - nm) : 0.f;
      const float t2 = (om > -INFINITY) ? os * __expf(om - nm) : 0.f;
      s = t1 + t2;
      m = nm;
    }
    const int wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
      lmax[wid] = m;
      lsum[wid] = s;
    }
    __syncthreads();
    const float bm = fmaxf(fmaxf(lmax[0], lmax[1]), fmaxf(lmax[2], lmax[3]));
    float bs = 0.f;
#pragma unroll
    for (int wi = 0; wi < 4; ++wi)
      bs += (lmax[wi] > -INFINITY) ? lsum[wi] * __expf(lmax[wi] - bm) : 0.f;
    const float l = bm + __logf(bs);
    const int s_pos = (int)(row % Sq);
    if (threadIdx.x == 0) {
      lse[row] = l;
      if (s_pos < Sq - 1) {
        const int64_t lab = labels[row + 1];
        const int64_t B = BS / Sq;
        const float inv = 1.f / (float)(B * (Sq - 1));
        atomicAdd(loss, (l - bf2f(lr[lab])) * inv);
      }
    }
    __syncthreads();
  }
}
extern "C" int ob_ce_fwd_bf16(const void* logits, const void* labels,
                              void* lse, void* loss, int64_t B, int64_t Sq,
                              int64_t V, int64_t ld, void* stream) {
  k_ce_fwd_bf16<<<(int)bmin64(B * Sq, 16384), 256, 0, S(stream)>>>(
      (const __bf16*)logits, (const int64_t*)labels, (float*)lse,
      (float*)loss, B * Sq, (int)Sq, (int)V, ld);
  OB_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(256) void k_ce_bwd_bf16(
    __bf16* __restrict__ logits, const int64_t* __restrict__ labels,
    const float* __restrict__ lse, const float* __restrict__ dloss,
    int64_t BS, int Sq, int V, int64_t ld) {
  const float dl = dloss ? *dloss : 1.f;
  const int64_t B = BS / Sq;
  const float scale = dl / (float)(B * (Sq - 1));
  for (int64_t row = blockIdx.y; row < BS; row += gridDim.y) {
    __bf16* lr = logits + row * ld;
    const int s_pos = (int)(row % Sq);
    const float l = lse[row];
    const bool valid = s_pos < Sq - 1;
    const int64_t lab = valid ? labels[row + 1] : -1;
    for (int64_t c8 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
         c8 < ld; c8 += (int64_t)gridDim.x * 256 * 8) {
      const uint4 in = *reinterpret_cast<const uint4*>(lr + c8);
      float out[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int64_t c = c8 + j;
        out[j] = (valid && c < V)
                     ? scale * (__expf(bf2f(bf_extract(in, j)) - l) -
                                (c == lab ? 1.f : 0.f))
                     : 0.f;
      }
      *reinterpret_cast<uint4*>(lr + c8) = bf_pack8(out);
    }
  }
}
extern "C" int ob_ce_bwd_bf16(void* logits, const void* labels,
                              const void* lse, const void* dloss, int64_t B,
                              int64_t Sq, int64_t V, int64_t ld,
                              void* stream) {
  if (ld % 8) return ob_fail("ce_bwd_bf16: ld must be a multiple of 8");
  dim3 grid((unsigned)bmin64((ld / 8 + 255) / 256, 256),
            (unsigned)bmin64(B * Sq, 16384));
  k_ce_bwd_bf16<<<grid, 256, 0, S(stream)>>>(
      (__bf16*)logits, (const int64_t*)labels, (const float*)lse,
      (const float*)dloss, B * Sq, (int)Sq, (int)V, ld);
  OB_LAUNCH_CHECK();
  return 0;
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

int ob_gemm_bf16_nt_dispatch(const void* A, const void* B, void* C,
                             const void* bias, const void* residual,
                             int64_t M, int64_t N, int64_t K, int64_t lda,
                             int64_t ldb, int64_t ldc, int64_t sA1,
                             int64_t sA2, int64_t sB1, int64_t sB2,
                             int64_t sC1, int64_t sC2, int64_t n1, int64_t n2,
                             float alpha, float beta, int out_kind, int splitk,
                             void* stream, int64_t Mr) {
  const int nbm = (int)(M / 128), nbn = (int)(N / 128);
  dim3 grid(nbm * nbn, splitk, (unsigned)(n1 * n2));
  dim3 block(256);
#define OB_NTG(OUT_)                                                         \
  k_gemm_bf16_nt_glds<OUT_><<<grid, block, 0, S(stream)>>>(                  \
      (const __bf16*)A, (const __bf16*)B, C, (const float*)bias,             \
      (const __bf16*)residual, (int)M, (int)N, (int)K, lda, ldb, ldc, sA1,   \
      sA2, sB1, sB2, sC1, sC2, (int)n2, alpha, beta, nbn, (int)Mr)
  if (out_kind == BF_OUT_BF16) OB_NTG(BF_OUT_BF16);
  else if (out_kind == BF_OUT_F32) OB_NTG(BF_OUT_F32);
  else OB_NTG(BF_OUT_F32_ATOMIC);
#undef OB_NTG
  OB_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// bf16 matrix transpose (out[c][r] = in[r][c]) — feeds the weight-grad
// GEMMs: materializing X^T / dY^T turns the transpose-staged TN case
// (scattered 2-byte LDS writes, measured ~150 TF) into the fast NT glds
// path, at ~2 HBM passes over the activations (~12 ms/step total).
// 64x64 tiles through LDS ([64][65]-half padding de-conflicts the
// column-gather reads).
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_transpose_bf16(
    const __bf16* __restrict__ in, __bf16* __restrict__ out, int64_t R,
    int64_t C) {
  __shared__ __bf16 tile[64 * 65];
  const int64_t tr = blockIdx.y;  // 64-row tile index
  const int64_t tc = blockIdx.x;  // 64-col tile index
  const int64_t r0 = tr * 64, c0 = tc * 64;
  // load: thread t covers rows t/8 (+32), col-octet (t%8)*8
  {
    const int rr = threadIdx.x >> 3;
    const int c8 = (threadIdx.x & 7) * 8;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int r = rr + it * 32;
      uint4 v = {0, 0, 0, 0};
      if (r0 + r < R && c0 + c8 + 7 < C) {
        v = *reinterpret_cast<const uint4*>(in + (r0 + r) * C + c0 + c8);
      } else if (r0 + r < R) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (c0 + c8 + j < C)
            reinterpret_cast<unsigned short*>(&v)[j] = __builtin_bit_cast(
                unsigned short, in[(r0 + r) * C + c0 + c8 + j]);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
        tile[r * 65 + c8 + j] = bf_extract(v, j);
    }
  }
  __syncthreads();
  // store: thread t covers out-rows (= in-cols) t/8 (+32), r-octet (t%8)*8
  {
    const int cc = threadIdx.x >> 3;
    const int r8 = (threadIdx.x & 7) * 8;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int c = cc + it * 32;
      if (c0 + c >= C) continue;
      float dummy[1];
      (void)dummy;
      unsigned e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        e[j] = bf_bits(tile[(r8 + j) * 65 + c]);
      uint4 v;
      v.x = e[0] | (e[1] << 16);
      v.y = e[2] | (e[3] << 16);
      v.z = e[4] | (e[5] << 16);
      v.w = e[6] | (e[7] << 16);
      if (r0 + r8 + 7 < R) {
        *reinterpret_cast<uint4*>(out + (c0 + c) * R + r0 + r8) = v;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (r0 + r8 + j < R)
            out[(c0 + c) * R + r0 + r8 + j] =
                bf_extract(v, j);
      }
    }
  }
}

extern "C" int ob_transpose_bf16(const void* in, void* out, int64_t R,
                                 int64_t C, void* stream) {
  dim3 grid((unsigned)((C + 63) / 64), (unsigned)((R + 63) / 64));
  k_transpose_bf16<<<grid, 256, 0, S(stream)>>>((const __bf16*)in,
                                                (__bf16*)out, R, C);
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
    _Pragma("unroll") for (int i = 0; i < BN / 128; ++i) {                    \
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
  // per-wave glds per tile: 4 (A) + BN/128*... = 8 (BN=256) or 6 (BN=128).
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

int ob_gemm_bf16_nt256_dispatch(const void* A, const void* B, void* C,
                                const void* bias, const void* residual,
                                int64_t M, int64_t N, int64_t K, int64_t lda,
                                int64_t ldb, int64_t ldc, int64_t sA1,
                                int64_t sA2, int64_t sB1, int64_t sB2,
                                int64_t sC1, int64_t sC2, int64_t n1,
                                int64_t n2, float alpha, float beta,
                                int out_kind, int splitk, void* stream,
                                int64_t Mr, int BN) {
  const int nbm = (int)((M + 255) / 256), nbn = (int)((N + BN - 1) / BN);
  dim3 grid(nbm * nbn, splitk, (unsigned)(n1 * n2));
  dim3 block(512);
#define OB_N2G(OUT_, BN_)                                                    \
  k_gemm_bf16_nt_256<OUT_, BN_><<<grid, block, 0, S(stream)>>>(              \
      (const __bf16*)A, (const __bf16*)B, C, (const float*)bias,             \
      (const __bf16*)residual, (int)M, (int)N, (int)K, lda, ldb, ldc, sA1,   \
      sA2, sB1, sB2, sC1, sC2, (int)n2, alpha, beta, nbn, (int)Mr)
  if (BN == 256) {
    if (out_kind == BF_OUT_BF16) OB_N2G(BF_OUT_BF16, 256);
    else if (out_kind == BF_OUT_F32) OB_N2G(BF_OUT_F32, 256);
    else OB_N2G(BF_OUT_F32_ATOMIC, 256);
  } else {
    if (out_kind == BF_OUT_BF16) OB_N2G(BF_OUT_BF16, 128);
    else if (out_kind == BF_OUT_F32) OB_N2G(BF_OUT_F32, 128);
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

extern "C" int ob_gemm_bf16_nt_8ph(const void* A, const void* B, void* C,
                                   const void* bias, const void* residual,
                                   int64_t M, int64_t N, int64_t K,
                                   int64_t lda, int64_t ldb, int64_t ldc,
                                   int64_t sA1, int64_t sA2, int64_t sB1,
                                   int64_t sB2, int64_t sC1, int64_t sC2,
                                   int64_t n1, int64_t n2, float alpha,
                                   float beta, int out_kind, int splitk,
                                   void* stream, int64_t Mr) {
  if (M % 256 || N % 256 || K % 64)
    return ob_fail("nt_8ph: M,N %% 256, K %% 64 required");
  const int nbm = (int)(M / 256), nbn = (int)(N / 256);
  dim3 grid(nbm * nbn, splitk < 1 ? 1 : splitk, (unsigned)(n1 * n2));
  dim3 block(512);
  static const int swz = [] {
    const char* e = getenv("OB_P8_SWZ");
    return e ? atoi(e) : 0;
  }();
#define OB_P8(OUT_, SWZ_)                                                    \
  k_gemm_bf16_nt_8ph<OUT_, SWZ_><<<grid, block, 0, S(stream)>>>(             \
      (const __bf16*)A, (const __bf16*)B, C, (const float*)bias,             \
      (const __bf16*)residual, (int)M, (int)N, (int)K, lda, ldb, ldc, sA1,   \
      sA2, sB1, sB2, sC1, sC2, (int)n2, alpha, beta, nbn, (int)Mr)
#define OB_P8S(OUT_)                                                         \
  do {                                                                       \
    if (swz == 1) OB_P8(OUT_, 1);                                            \
    else OB_P8(OUT_, 0);                                                     \
  } while (0)
  if (out_kind == BF_OUT_BF16) OB_P8S(BF_OUT_BF16);
  else if (out_kind == BF_OUT_F32) OB_P8S(BF_OUT_F32);
  else OB_P8S(BF_OUT_F32_ATOMIC);
#undef OB_P8S
#undef OB_P8
  OB_LAUNCH_CHECK();
  return 0;
}
