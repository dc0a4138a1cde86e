// ob_kernels.hip — hand-written CDNA4 (gfx950) HIP kernels for the Oobleck
// hot path, fp32.  No CUDA shims, no hipify: written for 64-wide wavefronts,
// MFMA f32 (v_mfma_f32_32x32x2_f32, the exact-f32 matrix path at the 157 TF
// f32 rate), LDS-staged tiles, coalesced HBM access.
//
// Operator content restated from the reference's layer math (HF GPT-2 eager
// ops the reference fx-splits; see oracle/gpt2_oracle.py for the per-op
// citations).  This file is the compute substrate the reference runs as
// torch eager ops inside fx GraphModules
// (/root/reference/oobleck/execution/layer.py:144-145).
#include "ob_internal.h"

#include <cmath>

static thread_local char g_err[1024] = {0};

int ob_fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return 1;
}

extern "C" const char* ob_last_error(void) { return g_err; }
extern "C" const char* ob_build_arch(void) {
#if defined(__HIP_DEVICE_COMPILE__)
  return "device";
#else
  return "gfx950";
#endif
}

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

// ---------------------------------------------------------------------------
// block reduction helpers (wave64 shfl + LDS across the block's waves)
// ---------------------------------------------------------------------------

__device__ __forceinline__ int64_t imin64d(int64_t a, int64_t b) {
  return a < b ? a : b;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;  // valid in lane 0
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off, 64));
  return v;
}

// block of 256 threads = 4 waves; result broadcast to all threads.
__device__ __forceinline__ float block_sum256(float v, float* lds4) {
  v = wave_sum(v);
  const int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds4[wid] = v;
  __syncthreads();
  const float r = lds4[0] + lds4[1] + lds4[2] + lds4[3];
  __syncthreads();
  return r;
}

__device__ __forceinline__ float block_max256(float v, float* lds4) {
  v = wave_max(v);
  const int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds4[wid] = v;
  __syncthreads();
  const float r = fmaxf(fmaxf(lds4[0], lds4[1]), fmaxf(lds4[2], lds4[3]));
  __syncthreads();
  return r;
}

// ---------------------------------------------------------------------------
// GEMM: C[M,N] (+)= alpha * op(A) @ op(B) (+ bias[n]) (+ R), fp32 MFMA.
//
// 128x128 block tile, BK=32, 4 waves; each wave computes a 64x64 sub-tile as
// 2x2 fragments of v_mfma_f32_32x32x2_f32 (A: lane l holds A[i=l&31][k=l>>5],
// B[k=l>>5][j=l&31]; C/D: col=l&31, row=(r&3)+8*(r>>2)+4*(l>>5)).
// LDS tiles are staged k-major As[k][m], Bs[k][n] with a +4-float row pad so
// both the transpose-staging writes and the fragment reads are conflict-free
// (bank = (addr/4)%32).
// ---------------------------------------------------------------------------

#define GEMM_BM 128
#define GEMM_BK 32
#define GEMM_LDT 132  // padded LDS row stride for the BM=128 A tile (floats)

// stage dst[k][c] = src[k][c] (src already offset; ld = src row stride).
// kmax/cmax = valid extents (zero-fill outside; EDGE=false skips every
// guard for interior tiles).  256 threads; NC = tile width (64 or 128).
template <int NC, bool EDGE>
__device__ __forceinline__ void stage_direct(float* dst, const float* src,
                                             int64_t ld, int kmax, int cmax) {
  constexpr int LDT = NC + 4;
  const int c4 = (threadIdx.x % (NC / 4)) * 4;
  const int k0 = threadIdx.x / (NC / 4);
  constexpr int KSTEP = 1024 / NC;  // rows covered per pass
#pragma unroll
  for (int it = 0; it < NC / 32; ++it) {
    const int k = k0 + it * KSTEP;
    if (EDGE) {
      float4 v = {0.f, 0.f, 0.f, 0.f};
      if (k < kmax) {
        if (c4 + 3 < cmax) {
          v = *reinterpret_cast<const float4*>(src + (int64_t)k * ld + c4);
        } else {
          if (c4 + 0 < cmax) v.x = src[(int64_t)k * ld + c4 + 0];
          if (c4 + 1 < cmax) v.y = src[(int64_t)k * ld + c4 + 1];
          if (c4 + 2 < cmax) v.z = src[(int64_t)k * ld + c4 + 2];
          if (c4 + 3 < cmax) v.w = src[(int64_t)k * ld + c4 + 3];
        }
      }
      *reinterpret_cast<float4*>(dst + k * LDT + c4) = v;
    } else {
      *reinterpret_cast<float4*>(dst + k * LDT + c4) =
          *reinterpret_cast<const float4*>(src + (int64_t)k * ld + c4);
    }
  }
}

// stage dst[k][c] = src[c][k] (transpose; src offset to (c0,k0); ld = src
// row stride).  Reads float4 along k (coalesced 128B per 8 lanes), writes
// columns; the +4 row pad makes the column writes conflict-free.
template <int NC, bool EDGE>
__device__ __forceinline__ void stage_transpose(float* dst, const float* src,
                                                int64_t ld, int kmax, int cmax) {
  constexpr int LDT = NC + 4;
  const int k4 = (threadIdx.x & 7) * 4;  // 0..28
  const int c0 = threadIdx.x >> 3;       // 0..31
#pragma unroll
  for (int it = 0; it < NC / 32; ++it) {
    const int c = c0 + it * 32;
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if (!EDGE || (c < cmax && k4 + 3 < kmax)) {
      v = *reinterpret_cast<const float4*>(src + (int64_t)c * ld + k4);
    } else if (c < cmax) {
      if (k4 + 0 < kmax) v.x = src[(int64_t)c * ld + k4 + 0];
      if (k4 + 1 < kmax) v.y = src[(int64_t)c * ld + k4 + 1];
      if (k4 + 2 < kmax) v.z = src[(int64_t)c * ld + k4 + 2];
      if (k4 + 3 < kmax) v.w = src[(int64_t)c * ld + k4 + 3];
    }
    dst[(k4 + 0) * LDT + c] = v.x;
    dst[(k4 + 1) * LDT + c] = v.y;
    dst[(k4 + 2) * LDT + c] = v.z;
    dst[(k4 + 3) * LDT + c] = v.w;
  }
}

// split load/write staging for the 2-phase (double-buffered) pipeline:
// loads issue at the top of iteration t for tile t+1 and land under the
// MFMAs; the write into the other LDS buffer happens after the MFMAs, one
// barrier per K-tile (T14 async-STAGE split, cdna_hip_programming.md G15).
template <int NC, bool EDGE>
struct StageRegs {
  float4 v[NC / 32];
};

template <int NC, bool EDGE>
__device__ __forceinline__ void stage_load_direct(StageRegs<NC, EDGE>& r,
                                                  const float* src, int64_t ld,
                                                  int kmax, int cmax) {
  const int c4 = (threadIdx.x % (NC / 4)) * 4;
  const int k0 = threadIdx.x / (NC / 4);
  constexpr int KSTEP = 1024 / NC;
#pragma unroll
  for (int it = 0; it < NC / 32; ++it) {
    const int k = k0 + it * KSTEP;
    if (EDGE) {
      float4 v = {0.f, 0.f, 0.f, 0.f};
      if (k < kmax) {
        if (c4 + 3 < cmax) {
          v = *reinterpret_cast<const float4*>(src + (int64_t)k * ld + c4);
        } else {
          if (c4 + 0 < cmax) v.x = src[(int64_t)k * ld + c4 + 0];
          if (c4 + 1 < cmax) v.y = src[(int64_t)k * ld + c4 + 1];
          if (c4 + 2 < cmax) v.z = src[(int64_t)k * ld + c4 + 2];
          if (c4 + 3 < cmax) v.w = src[(int64_t)k * ld + c4 + 3];
        }
      }
      r.v[it] = v;
    } else {
      r.v[it] = *reinterpret_cast<const float4*>(src + (int64_t)k * ld + c4);
    }
  }
}

template <int NC, bool EDGE>
__device__ __forceinline__ void stage_write_direct(const StageRegs<NC, EDGE>& r,
                                                   float* dst) {
  constexpr int LDT = NC + 4;
  const int c4 = (threadIdx.x % (NC / 4)) * 4;
  const int k0 = threadIdx.x / (NC / 4);
  constexpr int KSTEP = 1024 / NC;
#pragma unroll
  for (int it = 0; it < NC / 32; ++it)
    *reinterpret_cast<float4*>(dst + (k0 + it * KSTEP) * LDT + c4) = r.v[it];
}

template <int NC, bool EDGE>
__device__ __forceinline__ void stage_load_transpose(StageRegs<NC, EDGE>& r,
                                                     const float* src,
                                                     int64_t ld, int kmax,
                                                     int cmax) {
  const int k4 = (threadIdx.x & 7) * 4;
  const int c0 = threadIdx.x >> 3;
#pragma unroll
  for (int it = 0; it < NC / 32; ++it) {
    const int c = c0 + it * 32;
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if (!EDGE || (c < cmax && k4 + 3 < kmax)) {
      v = *reinterpret_cast<const float4*>(src + (int64_t)c * ld + k4);
    } else if (c < cmax) {
      if (k4 + 0 < kmax) v.x = src[(int64_t)c * ld + k4 + 0];
      if (k4 + 1 < kmax) v.y = src[(int64_t)c * ld + k4 + 1];
      if (k4 + 2 < kmax) v.z = src[(int64_t)c * ld + k4 + 2];
      if (k4 + 3 < kmax) v.w = src[(int64_t)c * ld + k4 + 3];
    }
    r.v[it] = v;
  }
}

template <int NC, bool EDGE>
__device__ __forceinline__ void stage_write_transpose(
    const StageRegs<NC, EDGE>& r, float* dst) {
  constexpr int LDT = NC + 4;
  const int k4 = (threadIdx.x & 7) * 4;
  const int c0 = threadIdx.x >> 3;
#pragma unroll
  for (int it = 0; it < NC / 32; ++it) {
    const int c = c0 + it * 32;
    dst[(k4 + 0) * LDT + c] = r.v[it].x;
    dst[(k4 + 1) * LDT + c] = r.v[it].y;
    dst[(k4 + 2) * LDT + c] = r.v[it].z;
    dst[(k4 + 3) * LDT + c] = r.v[it].w;
  }
}

// BM=128 always; BN ∈ {64,128}: 4 waves in 2x2, each owning 64 x (BN/2)
// output = 2 x (BN/64) fragments of 32x32.
template <bool TA, bool TB, bool ATOMIC, bool EDGE, int BN>
__global__ __launch_bounds__(256, 4) void k_gemm_f32(
    const float* __restrict__ A, const float* __restrict__ B,
    float* __restrict__ C, const float* __restrict__ bias,
    const float* __restrict__ R, int M, int N, int K, int64_t lda, int64_t ldb,
    int64_t ldc, int64_t sA1, int64_t sA2, int64_t sB1, int64_t sB2,
    int64_t sC1, int64_t sC2, int n2, float alpha, float beta, int nbn) {
  constexpr int FN = BN / 64;  // B fragments per wave (1 or 2)
  constexpr int LDB_T = BN + 4;
  __shared__ float As[GEMM_BK * GEMM_LDT];
  __shared__ float Bs[GEMM_BK * LDB_T];

  const int tile = blockIdx.x;
  const int bm = tile / nbn, bn = tile % nbn;
  const int m0 = bm * GEMM_BM, n0 = bn * BN;

  const int z = blockIdx.z;
  const int i1 = z / n2, i2 = z % n2;
  A += (int64_t)i1 * sA1 + (int64_t)i2 * sA2;
  B += (int64_t)i1 * sB1 + (int64_t)i2 * sB2;
  C += (int64_t)i1 * sC1 + (int64_t)i2 * sC2;
  if (R) R += (int64_t)i1 * sC1 + (int64_t)i2 * sC2;

  // split-K slice (blockIdx.y): [k0, kend)
  const int splitk = gridDim.y;
  const int kchunk = ((K + splitk * GEMM_BK - 1) / (splitk * GEMM_BK)) * GEMM_BK;
  const int kbeg = blockIdx.y * kchunk;
  const int kend = min(K, kbeg + kchunk);
  if (kbeg >= kend) return;

  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int il = lane & 31, kh = lane >> 5;

  f32x16 acc00 = {}, acc01 = {}, acc10 = {}, acc11 = {};

  for (int kt = kbeg; kt < kend; kt += GEMM_BK) {
    const int kmax = kend - kt;
    if (TA)
      stage_direct<GEMM_BM, EDGE>(As, A + (int64_t)kt * lda + m0, lda,
                                  min(kmax, GEMM_BK), min(M - m0, GEMM_BM));
    else
      stage_transpose<GEMM_BM, EDGE>(As, A + (int64_t)m0 * lda + kt, lda,
                                     min(kmax, GEMM_BK), min(M - m0, GEMM_BM));
    if (TB)
      stage_transpose<BN, EDGE>(Bs, B + (int64_t)n0 * ldb + kt, ldb,
                                min(kmax, GEMM_BK), min(N - n0, BN));
    else
      stage_direct<BN, EDGE>(Bs, B + (int64_t)kt * ldb + n0, ldb,
                             min(kmax, GEMM_BK), min(N - n0, BN));
    __syncthreads();

#pragma unroll
    for (int kk = 0; kk < GEMM_BK / 2; ++kk) {
      const float* ar = As + (kk * 2 + kh) * GEMM_LDT + wr * 64;
      const float* br = Bs + (kk * 2 + kh) * LDB_T + wc * (BN / 2);
      const float a0 = ar[il], a1 = ar[32 + il];
      const float b0 = br[il];
      acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc00, 0, 0, 0);
      acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc10, 0, 0, 0);
      if (FN == 2) {
        const float b1 = br[32 + il];
        acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc01, 0, 0, 0);
        acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc11, 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // epilogue
  const int mw = m0 + wr * 64, nw = n0 + wc * (BN / 2);
#define OB_EPI(ACC, TI, TJ)                                                   \
  {                                                                           \
    const int nn = nw + (TJ)*32 + il;                                         \
    if (!EDGE || nn < N) {                                                    \
      _Pragma("unroll") for (int r = 0; r < 16; ++r) {                        \
        const int mm = mw + (TI)*32 + (r & 3) + 8 * (r >> 2) + 4 * kh;        \
        if (!EDGE || mm < M) {                                                \
          float v = alpha * ACC[r];                                           \
          if (ATOMIC) {                                                       \
            atomicAdd(&C[(int64_t)mm * ldc + nn], v);                         \
          } else {                                                            \
            if (bias) v += bias[nn];                                          \
            if (R) v += R[(int64_t)mm * ldc + nn];                            \
            if (beta != 0.f) v += beta * C[(int64_t)mm * ldc + nn];           \
            C[(int64_t)mm * ldc + nn] = v;                                    \
          }                                                                   \
        }                                                                     \
      }                                                                       \
    }                                                                         \
  }
  OB_EPI(acc00, 0, 0)
  OB_EPI(acc10, 1, 0)
  if (FN == 2) {
    OB_EPI(acc01, 0, 1)
    OB_EPI(acc11, 1, 1)
  }
#undef OB_EPI
}

// 2-phase double-buffered variant: loads for tile t+1 issue before the
// MFMAs of tile t and land under them; LDS write + one barrier per tile.
template <bool TA, bool TB, bool ATOMIC, bool EDGE, int BN>
__global__ __launch_bounds__(256, 2) void k_gemm_f32_p2(
    const float* __restrict__ A, const float* __restrict__ B,
    float* __restrict__ C, const float* __restrict__ bias,
    const float* __restrict__ R, int M, int N, int K, int64_t lda, int64_t ldb,
    int64_t ldc, int64_t sA1, int64_t sA2, int64_t sB1, int64_t sB2,
    int64_t sC1, int64_t sC2, int n2, float alpha, float beta, int nbn) {
  constexpr int FN = BN / 64;
  constexpr int LDB_T = BN + 4;
  __shared__ float As[2][GEMM_BK * GEMM_LDT];
  __shared__ float Bs[2][GEMM_BK * LDB_T];

  const int tile = blockIdx.x;
  const int bm = tile / nbn, bn = tile % nbn;
  const int m0 = bm * GEMM_BM, n0 = bn * BN;

  const int z = blockIdx.z;
  const int i1 = z / n2, i2 = z % n2;
  A += (int64_t)i1 * sA1 + (int64_t)i2 * sA2;
  B += (int64_t)i1 * sB1 + (int64_t)i2 * sB2;
  C += (int64_t)i1 * sC1 + (int64_t)i2 * sC2;
  if (R) R += (int64_t)i1 * sC1 + (int64_t)i2 * sC2;

  const int splitk = gridDim.y;
  const int kchunk = ((K + splitk * GEMM_BK - 1) / (splitk * GEMM_BK)) * GEMM_BK;
  const int kbeg = blockIdx.y * kchunk;
  const int kend = min(K, kbeg + kchunk);
  if (kbeg >= kend) return;

  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int il = lane & 31, kh = lane >> 5;

#define OB_P2_LOAD(KT)                                                        \
  {                                                                           \
    const int kmax_ = min(kend - (KT), GEMM_BK);                              \
    if (TA)                                                                   \
      stage_load_direct<GEMM_BM, EDGE>(ra, A + (int64_t)(KT)*lda + m0, lda,   \
                                       kmax_, min(M - m0, GEMM_BM));          \
    else                                                                      \
      stage_load_transpose<GEMM_BM, EDGE>(ra, A + (int64_t)m0 * lda + (KT),   \
                                          lda, kmax_, min(M - m0, GEMM_BM));  \
    if (TB)                                                                   \
      stage_load_transpose<BN, EDGE>(rb, B + (int64_t)n0 * ldb + (KT), ldb,   \
                                     kmax_, min(N - n0, BN));                 \
    else                                                                      \
      stage_load_direct<BN, EDGE>(rb, B + (int64_t)(KT)*ldb + n0, ldb, kmax_, \
                                  min(N - n0, BN));                           \
  }
#define OB_P2_WRITE(BUF)                                                      \
  {                                                                           \
    if (TA)                                                                   \
      stage_write_direct<GEMM_BM, EDGE>(ra, As[BUF]);                         \
    else                                                                      \
      stage_write_transpose<GEMM_BM, EDGE>(ra, As[BUF]);                      \
    if (TB)                                                                   \
      stage_write_transpose<BN, EDGE>(rb, Bs[BUF]);                           \
    else                                                                      \
      stage_write_direct<BN, EDGE>(rb, Bs[BUF]);                              \
  }

  f32x16 acc00 = {}, acc01 = {}, acc10 = {}, acc11 = {};

  {
    StageRegs<GEMM_BM, EDGE> ra;
    StageRegs<BN, EDGE> rb;
    OB_P2_LOAD(kbeg)
    OB_P2_WRITE(0)
  }
  __syncthreads();

#define OB_P2_MFMA(BUF)                                                       \
  _Pragma("unroll") for (int kk = 0; kk < GEMM_BK / 2; ++kk) {                \
    const float* ar = As[BUF] + (kk * 2 + kh) * GEMM_LDT + wr * 64;           \
    const float* br = Bs[BUF] + (kk * 2 + kh) * LDB_T + wc * (BN / 2);        \
    const float a0 = ar[il], a1 = ar[32 + il];                                \
    const float b0 = br[il];                                                  \
    acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc00, 0, 0, 0);     \
    acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc10, 0, 0, 0);     \
    if (FN == 2) {                                                            \
      const float b1 = br[32 + il];                                           \
      acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc01, 0, 0, 0);   \
      acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc11, 0, 0, 0);   \
    }                                                                         \
  }

  // steady state is branch-free: the last tile is peeled out of the loop.
  int cur = 0;
  for (int kt = kbeg; kt + GEMM_BK < kend; kt += GEMM_BK) {
    StageRegs<GEMM_BM, EDGE> ra;
    StageRegs<BN, EDGE> rb;
    OB_P2_LOAD(kt + GEMM_BK)
    OB_P2_MFMA(cur)
    OB_P2_WRITE(cur ^ 1)
    __syncthreads();
    cur ^= 1;
  }
  OB_P2_MFMA(cur)
#undef OB_P2_LOAD
#undef OB_P2_WRITE
#undef OB_P2_MFMA

  const int mw = m0 + wr * 64, nw = n0 + wc * (BN / 2);
#define OB_EPI(ACC, TI, TJ)                                                   \
  {                                                                           \
    const int nn = nw + (TJ)*32 + il;                                         \
    if (!EDGE || nn < N) {                                                    \
      _Pragma("unroll") for (int r = 0; r < 16; ++r) {                        \
        const int mm = mw + (TI)*32 + (r & 3) + 8 * (r >> 2) + 4 * kh;        \
        if (!EDGE || mm < M) {                                                \
          float v = alpha * ACC[r];                                           \
          if (ATOMIC) {                                                       \
            atomicAdd(&C[(int64_t)mm * ldc + nn], v);                         \
          } else {                                                            \
            if (bias) v += bias[nn];                                          \
            if (R) v += R[(int64_t)mm * ldc + nn];                            \
            if (beta != 0.f) v += beta * C[(int64_t)mm * ldc + nn];           \
            C[(int64_t)mm * ldc + nn] = v;                                    \
          }                                                                   \
        }                                                                     \
      }                                                                       \
    }                                                                         \
  }
  OB_EPI(acc00, 0, 0)
  OB_EPI(acc10, 1, 0)
  if (FN == 2) {
    OB_EPI(acc01, 0, 1)
    OB_EPI(acc11, 1, 1)
  }
#undef OB_EPI
}

__global__ void k_gemm_f32_tn_glds(const float* __restrict__ A,
                                   const float* __restrict__ B,
                                   float* __restrict__ C, int M, int N, int K,
                                   int64_t lda, int64_t ldb, int64_t ldc,
                                   float alpha, int nbn);

extern "C" int ob_gemm_f32(int transA, int transB, int64_t M, int64_t N,
                           int64_t K, float alpha, const void* A, int64_t lda,
                           int64_t strideA1, int64_t strideA2, const void* B,
                           int64_t ldb, int64_t strideB1, int64_t strideB2,
                           float beta, void* C, int64_t ldc, int64_t strideC1,
                           int64_t strideC2, int64_t n1, int64_t n2,
                           const void* bias, const void* residual, int atomic,
                           int splitk, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0) return ob_fail("gemm: bad dims");
  if (splitk < 1) splitk = 1;
  if (splitk > 1 && !atomic)
    return ob_fail("gemm: splitk>1 requires atomic stores");
  if (atomic && (bias || residual))
    return ob_fail("gemm: atomic epilogue excludes bias/residual");
  const int BN = (N <= 64) ? 64 : 128;  // narrow tiles for head_dim GEMMs
  const int nbm = (int)((M + GEMM_BM - 1) / GEMM_BM);
  const int nbn = (int)((N + BN - 1) / BN);
  // guard-free interior variant when no tile has a tail anywhere
  const bool edge = (M % GEMM_BM) || (N % BN) || (K % GEMM_BK);
  // 2-phase double-buffered pipeline when the K loop is deep enough to
  // overlap (ob_GEMM_V1=1 in the environment falls back, for A/B runs).
  static const bool force_v1 = ob_env_flag("OB_GEMM_V1", false);
  // P2 wins on interior shapes (+3..27%) but loses on edge shapes
  // (lm_head N=50257: 113.7->103.1 TF measured) - gate on !edge.
  const bool p2 = !force_v1 && !edge && K >= 2 * GEMM_BK;
  dim3 grid(nbm * nbn, splitk, (unsigned)(n1 * n2));
  dim3 block(256);
#define OB_GEMM_LAUNCH4(TA_, TB_, AT_, ED_, BN_)                            \
  do {                                                                      \
    if (p2)                                                                 \
      k_gemm_f32_p2<TA_, TB_, AT_, ED_, BN_><<<grid, block, 0, S(stream)>>>(\
          (const float*)A, (const float*)B, (float*)C, (const float*)bias,  \
          (const float*)residual, (int)M, (int)N, (int)K, lda, ldb, ldc,    \
          strideA1, strideA2, strideB1, strideB2, strideC1, strideC2,       \
          (int)n2, alpha, beta, nbn);                                       \
    else                                                                    \
      k_gemm_f32<TA_, TB_, AT_, ED_, BN_><<<grid, block, 0, S(stream)>>>(   \
          (const float*)A, (const float*)B, (float*)C, (const float*)bias,  \
          (const float*)residual, (int)M, (int)N, (int)K, lda, ldb, ldc,    \
          strideA1, strideA2, strideB1, strideB2, strideC1, strideC2,       \
          (int)n2, alpha, beta, nbn);                                       \
  } while (0)
#define OB_GEMM_LAUNCH2(TA_, TB_, AT_)                                      \
  do {                                                                      \
    if (BN == 64) {                                                         \
      if (edge) OB_GEMM_LAUNCH4(TA_, TB_, AT_, true, 64);                   \
      else OB_GEMM_LAUNCH4(TA_, TB_, AT_, false, 64);                       \
    } else {                                                                \
      if (edge) OB_GEMM_LAUNCH4(TA_, TB_, AT_, true, 128);                  \
      else OB_GEMM_LAUNCH4(TA_, TB_, AT_, false, 128);                      \
    }                                                                       \
  } while (0)
  // fp32 TN glds-direct kernel: measured perf-neutral on the dW shapes
  // (85 TF either way — fp32 dW is tail/occupancy-bound, not
  // staging-bound), so it stays opt-in for experiments.
  static const bool tn_glds = ob_env_flag("OB_F32_TN_GLDS", false);
  if (tn_glds && transA && !transB && atomic && !edge && BN == 128 &&
      (reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B)) %
              16 == 0 &&
      (lda | ldb) % 4 == 0 && n1 * n2 == 1 && K >= 2 * GEMM_BK && !bias &&
      !residual) {
    k_gemm_f32_tn_glds<<<grid, block, 0, S(stream)>>>(
        (const float*)A, (const float*)B, (float*)C, (int)M, (int)N, (int)K,
        lda, ldb, ldc, alpha, nbn);
    OB_LAUNCH_CHECK();
    return 0;
  }
  const int sel = (transA ? 4 : 0) | (transB ? 2 : 0) | (atomic ? 1 : 0);
  switch (sel) {
    case 0: OB_GEMM_LAUNCH2(false, false, false); break;
    case 1: OB_GEMM_LAUNCH2(false, false, true); break;
    case 2: OB_GEMM_LAUNCH2(false, true, false); break;
    case 3: OB_GEMM_LAUNCH2(false, true, true); break;
    case 4: OB_GEMM_LAUNCH2(true, false, false); break;
    case 5: OB_GEMM_LAUNCH2(true, false, true); break;
    case 6: OB_GEMM_LAUNCH2(true, true, false); break;
    case 7: OB_GEMM_LAUNCH2(true, true, true); break;
  }
#undef OB_GEMM_LAUNCH2
#undef OB_GEMM_LAUNCH4
  OB_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// LayerNorm forward: one 256-thread block per row.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_ln_fwd(const float* __restrict__ x,
                                                const float* __restrict__ w,
                                                const float* __restrict__ b,
                                                float* __restrict__ y,
                                                float* __restrict__ mean,
                                                float* __restrict__ rstd,
                                                int64_t rows, int H, float eps) {
  __shared__ float lds4[4];
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const float* xr = x + row * H;
    float s = 0.f, sq = 0.f;
    for (int c = threadIdx.x; c < H; c += 256) {
      const float v = xr[c];
      s += v;
      sq += v * v;
    }
    const float mu = block_sum256(s, lds4) / H;
    const float var = block_sum256(sq, lds4) / H - mu * mu;
    const float rs = rsqrtf(var + eps);
    if (threadIdx.x == 0) {
      mean[row] = mu;
      rstd[row] = rs;
    }
    float* yr = y + row * H;
    for (int c = threadIdx.x; c < H; c += 256)
      yr[c] = (xr[c] - mu) * rs * w[c] + b[c];
    __syncthreads();
  }
}

static inline int64_t imin64(int64_t a, int64_t b) { return a < b ? a : b; }

extern "C" int ob_layernorm_fwd_f32(const void* x, const void* w, const void* b,
                                    void* y, void* mean, void* rstd,
                                    int64_t rows, int64_t H, float eps,
                                    void* stream) {
  const int grid = (int)imin64(rows, 16384);
  k_ln_fwd<<<grid, 256, 0, S(stream)>>>((const float*)x, (const float*)w,
                                        (const float*)b, (float*)y,
                                        (float*)mean, (float*)rstd, rows,
                                        (int)H, eps);
  OB_LAUNCH_CHECK();
  return 0;
}

// LayerNorm backward.  CHUNK rows per block; dw/db accumulated in registers
// per thread-owned columns, one atomicAdd per column per block.
// dx_i (+)= rstd*( dy_i*w_i − mean_c(dy*w) − xhat_i * mean_c(dy*w*xhat) )
#define LN_CHUNK 16
#define LN_MAX_H (256 * 48)

template <bool DX_ACCUM, int CPT>
__global__ __launch_bounds__(256) void k_ln_bwd(
    const float* __restrict__ x, const float* __restrict__ w,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ dy, float* __restrict__ dx,
    float* __restrict__ dw, float* __restrict__ db, int64_t rows, int H) {
  __shared__ float lds4[4];
  const int64_t r0 = (int64_t)blockIdx.x * LN_CHUNK;
  // register accumulators for CPT columns per thread, H <= 256 * CPT: 8
  // for H <= 2048 (GPT-2 H is 768/1600 — LN is only applied across
  // n_embd), 16/32/48 for the GPT-3 widths up to 12288.  Fixed-bound
  // unrolled loops keep the arrays in registers (hipcc sends runtime-indexed
  // local arrays to scratch).
  float accw[CPT] = {0}, accb[CPT] = {0};
  const int64_t rend = imin64d(rows, r0 + LN_CHUNK);
  for (int64_t row = r0; row < rend; ++row) {
    const float* xr = x + row * H;
    const float* dyr = dy + row * H;
    const float mu = mean[row], rs = rstd[row];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
      const int c = threadIdx.x + j * 256;
      if (c < H) {
        const float xhat = (xr[c] - mu) * rs;
        const float dyw = dyr[c] * w[c];
        s1 += dyw * xhat;
        s2 += dyw;
        accw[j] += dyr[c] * xhat;
        accb[j] += dyr[c];
      }
    }
    const float m1 = block_sum256(s1, lds4) / H;
    const float m2 = block_sum256(s2, lds4) / H;
    float* dxr = dx + row * H;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
      const int c = threadIdx.x + j * 256;
      if (c < H) {
        const float xhat = (xr[c] - mu) * rs;
        const float v = rs * (dyr[c] * w[c] - m2 - xhat * m1);
        if (DX_ACCUM)
          dxr[c] += v;
        else
          dxr[c] = v;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    const int c = threadIdx.x + j * 256;
    if (c < H) {
      atomicAdd(&dw[c], accw[j]);
      atomicAdd(&db[c], accb[j]);
    }
  }
}

extern "C" int ob_layernorm_bwd_f32(const void* x, const void* w,
                                    const void* mean, const void* rstd,
                                    const void* dy, void* dx, void* dw,
                                    void* db, int64_t rows, int64_t H,
                                    int dx_accum, void* stream) {
  if (H > LN_MAX_H) return ob_fail("ln_bwd: H > 12288 unsupported");
  const int grid = (int)((rows + LN_CHUNK - 1) / LN_CHUNK);
#define OB_LNF(A_, C_)                                                 \
  k_ln_bwd<A_, C_><<<grid, 256, 0, S(stream)>>>(                       \
      (const float*)x, (const float*)w, (const float*)mean,            \
      (const float*)rstd, (const float*)dy, (float*)dx, (float*)dw,    \
      (float*)db, rows, (int)H)
  // the smallest columns-per-thread count that covers H
  if (dx_accum) {
    if (H <= 2048) OB_LNF(true, 8);
    else if (H <= 4096) OB_LNF(true, 16);
    else if (H <= 8192) OB_LNF(true, 32);
    else OB_LNF(true, 48);
  } else {
    if (H <= 2048) OB_LNF(false, 8);
    else if (H <= 4096) OB_LNF(false, 16);
    else if (H <= 8192) OB_LNF(false, 32);
    else OB_LNF(false, 48);
  }
#undef OB_LNF
  OB_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// Causal softmax (fp32 scores in place).  Row r of the S×S score matrix
// keeps columns 0..r; masked entries become exactly 0 (matching exp of the
// finfo.min-masked eager path, which underflows to 0 in fp32).
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_softmax_causal_fwd(
    float* __restrict__ scores, int Sq, float scale) {
  __shared__ float lds4[4];
  const int64_t rid = blockIdx.x;        // z * S + row
  const int row = (int)(rid % Sq);
  float* p = scores + rid * Sq;
  const int valid = row + 1;
  // registers: up to 8 elements per thread (S <= 2048); fixed-bound
  // unrolled loops keep v[] in registers.
  float v[8];
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = threadIdx.x + j * 256;
    v[j] = (c < valid) ? p[c] * scale : -INFINITY;
    mx = fmaxf(mx, v[j]);
  }
  mx = block_max256(mx, lds4);
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = (v[j] == -INFINITY) ? 0.f : __expf(v[j] - mx);
    sum += v[j];
  }
  sum = block_sum256(sum, lds4);
  const float inv = 1.f / sum;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = threadIdx.x + j * 256;
    if (c < Sq) p[c] = v[j] * inv;
  }
}

extern "C" int ob_softmax_causal_fwd_f32(void* scores, int64_t batch, int64_t Sq,
                                         float scale, void* stream) {
  if (Sq > 2048) return ob_fail("softmax: S > 2048 unsupported");
  k_softmax_causal_fwd<<<(unsigned)(batch * Sq), 256, 0, S(stream)>>>(
      (float*)scores, (int)Sq, scale);
  OB_LAUNCH_CHECK();
  return 0;
}

// dS = P * (dP − sum_c dP*P), in place on dP.
__global__ __launch_bounds__(256) void k_softmax_causal_bwd(
    const float* __restrict__ P, float* __restrict__ dP, int Sq) {
  __shared__ float lds4[4];
  const int64_t rid = blockIdx.x;
  const int row = (int)(rid % Sq);
  const float* pr = P + rid * Sq;
  float* dr = dP + rid * Sq;
  const int valid = row + 1;
  float pv[8], dv[8];
  float t = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = threadIdx.x + j * 256;
    pv[j] = (c < valid) ? pr[c] : 0.f;
    dv[j] = (c < valid) ? dr[c] : 0.f;
    t += pv[j] * dv[j];
  }
  t = block_sum256(t, lds4);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = threadIdx.x + j * 256;
    if (c < Sq) dr[c] = pv[j] * (dv[j] - t);
  }
}

extern "C" int ob_softmax_causal_bwd_f32(const void* P, void* dP, int64_t batch,
                                         int64_t Sq, void* stream) {
  if (Sq > 2048) return ob_fail("softmax_bwd: S > 2048 unsupported");
  k_softmax_causal_bwd<<<(unsigned)(batch * Sq), 256, 0, S(stream)>>>(
      (const float*)P, (float*)dP, (int)Sq);
  OB_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// gelu_new (transformers NewGELUActivation):
//   g = 0.5*u*(1 + tanh(k*(u + 0.044715*u^3))), k = sqrt(2/pi)
//   dg/du = 0.5*(1+tanh(t)) + 0.5*u*(1-tanh(t)^2)*k*(1 + 3*0.044715*u^2)
// ---------------------------------------------------------------------------

#define GELU_K 0.7978845608028654f
#define GELU_C 0.044715f

__global__ __launch_bounds__(256) void k_gelu_fwd(const float* __restrict__ u,
                                                  float* __restrict__ g,
                                                  int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * 256) {
    const float x = u[i];
    const float t = tanhf(GELU_K * (x + GELU_C * x * x * x));
    g[i] = 0.5f * x * (1.f + t);
  }
}

__global__ __launch_bounds__(256) void k_gelu_bwd(const float* __restrict__ u,
                                                  const float* __restrict__ dg,
                                                  float* __restrict__ du,
                                                  int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * 256) {
    const float x = u[i];
    const float t = tanhf(GELU_K * (x + GELU_C * x * x * x));
    const float d = 0.5f * (1.f + t) +
                    0.5f * x * (1.f - t * t) * GELU_K * (1.f + 3.f * GELU_C * x * x);
    du[i] = dg[i] * d;
  }
}

extern "C" int ob_gelu_fwd_f32(const void* u, void* g, int64_t n, void* stream) {
  const int grid = (int)imin64((n + 255) / 256, 2048);
  k_gelu_fwd<<<grid, 256, 0, S(stream)>>>((const float*)u, (float*)g, n);
  OB_LAUNCH_CHECK();
  return 0;
}
extern "C" int ob_gelu_bwd_f32(const void* u, const void* dg, void* du,
                               int64_t n, void* stream) {
  const int grid = (int)imin64((n + 255) / 256, 2048);
  k_gelu_bwd<<<grid, 256, 0, S(stream)>>>((const float*)u, (const float*)dg,
                                          (float*)du, n);
  OB_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// column sum: db[n] += sum_m X[m,n]
// ---------------------------------------------------------------------------

#define CS_ROWS 256

__global__ __launch_bounds__(256) void k_colsum(const float* __restrict__ X,
                                                float* __restrict__ db,
                                                int64_t M, int64_t N) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  const int64_t r0 = (int64_t)blockIdx.y * CS_ROWS;
  const int64_t r1 = min(M, r0 + CS_ROWS);
  float acc = 0.f;
  for (int64_t r = r0; r < r1; ++r) acc += X[r * N + c];
  atomicAdd(&db[c], acc);
}

extern "C" int ob_colsum_f32(const void* X, void* db, int64_t M, int64_t N,
                             void* stream) {
  dim3 grid((unsigned)((N + 255) / 256), (unsigned)((M + CS_ROWS - 1) / CS_ROWS));
  k_colsum<<<grid, 256, 0, S(stream)>>>((const float*)X, (float*)db, M, N);
  OB_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// Embedding: out[b,s,:] = wte[ids[b,s]] + wpe[s]   (model.py wte+wpe sum)
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_embed_fwd(const int64_t* __restrict__ ids,
                                                   const float* __restrict__ wte,
                                                   const float* __restrict__ wpe,
                                                   float* __restrict__ out,
                                                   int64_t BS, int Sq, int H) {
  for (int64_t row = blockIdx.x; row < BS; row += gridDim.x) {
    const int64_t id = ids[row];
    const int s = (int)(row % Sq);
    const float* te = wte + id * H;
    const float* pe = wpe + (int64_t)s * H;
    float* o = out + row * H;
    for (int c = threadIdx.x; c < H; c += 256) o[c] = te[c] + pe[c];
  }
}

int ob_embed_fwd_f32(const int64_t* ids, const float* wte, const float* wpe,
                     float* out, int64_t B, int64_t Sq, int64_t H, void* stream) {
  const int grid = (int)imin64(B * Sq, 16384);
  k_embed_fwd<<<grid, 256, 0, S(stream)>>>(ids, wte, wpe, out, B * Sq, (int)Sq,
                                           (int)H);
  OB_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(256) void k_embed_bwd(const int64_t* __restrict__ ids,
                                                   const float* __restrict__ dout,
                                                   float* __restrict__ dwte,
                                                   float* __restrict__ dwpe,
                                                   int64_t BS, int Sq, int H) {
  for (int64_t row = blockIdx.x; row < BS; row += gridDim.x) {
    const int64_t id = ids[row];
    const int s = (int)(row % Sq);
    const float* d = dout + row * H;
    for (int c = threadIdx.x; c < H; c += 256) {
      atomicAdd(&dwte[id * H + c], d[c]);
      atomicAdd(&dwpe[(int64_t)s * H + c], d[c]);
    }
  }
}

int ob_embed_bwd_f32(const int64_t* ids, const float* dout, float* dwte,
                     float* dwpe, int64_t B, int64_t Sq, int64_t H,
                     void* stream) {
  const int grid = (int)imin64(B * Sq, 16384);
  k_embed_bwd<<<grid, 256, 0, S(stream)>>>(ids, dout, dwte, dwpe, B * Sq,
                                           (int)Sq, (int)H);
  OB_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// Cross-entropy with the GPT-2 shift (modeling_gpt2: loss over
// logits[:, :-1] vs labels[:, 1:], mean).  One block per row; single online
// (max,sum) pass over V; loss accumulated with one atomicAdd per valid row.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_ce_fwd(const float* __restrict__ logits,
                                                const int64_t* __restrict__ labels,
                                                float* __restrict__ lse,
                                                float* __restrict__ loss,
                                                int64_t BS, int Sq, int V) {
  __shared__ float lmax[4], lsum[4];
  for (int64_t row = blockIdx.x; row < BS; row += gridDim.x) {
    const float* lr = logits + row * V;
    float m = -INFINITY, s = 0.f;
    for (int c = threadIdx.x; c < V; c += 256) {
      const float x = lr[c];
      if (x > m) {
        s = s * __expf(m - x) + 1.f;
        m = x;
      } else {
        s += __expf(x - m);
      }
    }
    // combine across the wave then the block: (m,s) pairs.  A lane/wave that
    // processed no elements carries (m=-inf, s=0); guard the exp so
    // exp(-inf - -inf) never produces NaN.
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
        const int64_t lab = labels[row + 1];  // labels[b, s+1]
        const int64_t B = BS / Sq;
        const float inv = 1.f / (float)(B * (Sq - 1));
        atomicAdd(loss, (l - lr[lab]) * inv);
      }
    }
    __syncthreads();
  }
}

int ob_ce_fwd_f32(const float* logits, const int64_t* labels, float* lse,
                  float* loss, int64_t B, int64_t Sq, int64_t V, void* stream) {
  const int grid = (int)imin64(B * Sq, 16384);
  k_ce_fwd<<<grid, 256, 0, S(stream)>>>(logits, labels, lse, loss, B * Sq,
                                        (int)Sq, (int)V);
  OB_LAUNCH_CHECK();
  return 0;
}

// dlogits[m,v] = dloss/(B*(S-1)) * (softmax - onehot(label[m+1]))  for rows
// with s < S-1, else 0.  In place on the logits stash.
__global__ __launch_bounds__(256) void k_ce_bwd(float* __restrict__ logits,
                                                const int64_t* __restrict__ labels,
                                                const float* __restrict__ lse,
                                                const float* __restrict__ dloss,
                                                int64_t BS, int Sq, int V) {
  const float dl = dloss ? *dloss : 1.f;
  const int64_t B = BS / Sq;
  const float scale = dl / (float)(B * (Sq - 1));
  for (int64_t row = blockIdx.y; row < BS; row += gridDim.y) {
    float* lr = logits + row * V;
    const int s_pos = (int)(row % Sq);
    const float l = lse[row];
    const bool valid = s_pos < Sq - 1;
    const int64_t lab = valid ? labels[row + 1] : -1;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < V;
         c += (int64_t)gridDim.x * 256) {
      float g = 0.f;
      if (valid) {
        g = scale * (__expf(lr[c] - l) - (c == lab ? 1.f : 0.f));
      }
      lr[c] = g;
    }
  }
}

int ob_ce_bwd_f32(float* logits, const int64_t* labels, const float* lse,
                  const float* dloss, int64_t B, int64_t Sq, int64_t V,
                  void* stream) {
  dim3 grid((unsigned)imin64((V + 255) / 256, 256),
            (unsigned)imin64(B * Sq, 16384));
  k_ce_bwd<<<grid, 256, 0, S(stream)>>>(logits, labels, lse, dloss, B * Sq,
                                        (int)Sq, (int)V);
  OB_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// Fused AdamW over a flat buffer: 7 words/param traffic (r: p,g,m,v;
// w: p,m,v).  Matches torch.optim.AdamW (decoupled wd, bias correction,
// eps added after sqrt(v)/sqrt(bc2)).
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_adamw(float* __restrict__ p,
                                               const float* __restrict__ g,
                                               float* __restrict__ m,
                                               float* __restrict__ v, int64_t n,
                                               float wd_factor, float step_size,
                                               float inv_sqrt_bc2, float beta1,
                                               float beta2, float eps) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * 256) {
    ob_adamw_update(p, m, v, i, g[i], wd_factor, step_size, inv_sqrt_bc2,
                    beta1, beta2, eps);
  }
}

extern "C" int ob_adamw_step(void* p, const void* g, void* m, void* v,
                             int64_t n, int32_t step, float lr, float beta1,
                             float beta2, float eps, float weight_decay,
                             void* stream) {
  if (step < 1) return ob_fail("adamw: step must be >= 1");
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const int grid = (int)imin64((n + 255) / 256, 4096);
  const int prof_slot =
      ob_prof_on() ? ob_prof_beg(OB_PF_ADAMW, S(stream)) : -1;
  k_adamw<<<grid, 256, 0, S(stream)>>>(
      (float*)p, (const float*)g, (float*)m, (float*)v, n,
      1.f - lr * weight_decay, (float)(lr / bc1), (float)(1.0 / sqrt(bc2)),
      beta1, beta2, eps);
  if (prof_slot >= 0) ob_prof_end(OB_PF_ADAMW, prof_slot, S(stream));
  OB_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// fp32 TN (weight-grad) kernel with async glds staging: in the TN case BOTH
// operands are stored k-major ([K=BS, dim]), so both stage DIRECTLY into
// unpadded k-major LDS images ([32][128] f32: ds_read_b32 fragment reads
// are conflict-free without padding) via global_load_lds — no transpose
// staging, no register round-trip.  2 LDS buffers, counted vmcnt + raw
// barriers (loads for tile t+1 fly under tile t's 4096-cycle MFMA block).
// Interior shapes, atomic-f32 output (the dW pattern), split-K supported.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256, 2) void k_gemm_f32_tn_glds(
    const float* __restrict__ A, const float* __restrict__ B,
    float* __restrict__ C, int M, int N, int K, int64_t lda, int64_t ldb,
    int64_t ldc, float alpha, int nbn) {
  __shared__ float As[2][GEMM_BK * 128];
  __shared__ float Bs[2][GEMM_BK * 128];

  const int tile = blockIdx.x;
  const int bm = tile / nbn, bn = tile % nbn;
  const int m0 = bm * 128, n0 = bn * 128;

  const int splitk = gridDim.y;
  const int kchunk = ((K + splitk * GEMM_BK - 1) / (splitk * GEMM_BK)) * GEMM_BK;
  const int kbeg = blockIdx.y * kchunk;
  const int kend = min(K, kbeg + kchunk);
  if (kbeg >= kend) return;

  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int il = lane & 31, kh = lane >> 5;

  // glds: 1 KiB per wave instruction = 2 rows of 512 B; per wave per tile
  // per operand: 4 instructions (8 of 32 k-rows).
  const int g_row = lane >> 5;        // 0..1 within the instruction
  const int g_m4 = (lane & 31) * 4;   // 16-B column chunk
#define OB_TN_GLDS(BUF, KT)                                                   \
  {                                                                           \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                           \
      const int k = w * 8 + i * 2 + g_row;                                    \
      const float* asrc = A + (int64_t)((KT) + k) * lda + m0 + g_m4;          \
      const float* bsrc = B + (int64_t)((KT) + k) * ldb + n0 + g_m4;          \
      auto al = (__attribute__((address_space(3))) void*)                     \
          (&As[BUF][(w * 8 + i * 2) * 128]);                                  \
      auto bl = (__attribute__((address_space(3))) void*)                     \
          (&Bs[BUF][(w * 8 + i * 2) * 128]);                                  \
      __builtin_amdgcn_global_load_lds(                                       \
          (const __attribute__((address_space(1))) void*)asrc, al, 16, 0, 0); \
      __builtin_amdgcn_global_load_lds(                                       \
          (const __attribute__((address_space(1))) void*)bsrc, bl, 16, 0, 0); \
    }                                                                         \
  }

  f32x16 acc00 = {}, acc01 = {}, acc10 = {}, acc11 = {};
#define OB_TN_MFMA(BUF)                                                       \
  __builtin_amdgcn_s_setprio(1);                                              \
  _Pragma("unroll") for (int kk = 0; kk < GEMM_BK / 2; ++kk) {                \
    const float* ar = As[BUF] + (kk * 2 + kh) * 128 + wr * 64;                \
    const float* br = Bs[BUF] + (kk * 2 + kh) * 128 + wc * 64;                \
    const float a0 = ar[il], a1 = ar[32 + il];                                \
    const float b0 = br[il], b1 = br[32 + il];                                \
    acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc00, 0, 0, 0);     \
    acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc01, 0, 0, 0);     \
    acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc10, 0, 0, 0);     \
    acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc11, 0, 0, 0);     \
  }                                                                           \
  __builtin_amdgcn_s_setprio(0);

  OB_TN_GLDS(0, kbeg)
  int cur = 0;
  for (int kt = kbeg; kt + GEMM_BK < kend; kt += GEMM_BK) {
    OB_TN_GLDS(cur ^ 1, kt + GEMM_BK)
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    OB_TN_MFMA(cur)
    __builtin_amdgcn_s_barrier();
    cur ^= 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  OB_TN_MFMA(cur)
#undef OB_TN_GLDS
#undef OB_TN_MFMA

  const int mw = m0 + wr * 64, nw = n0 + wc * 64;
#define OB_TN_EPI(ACC, TI, TJ)                                                \
  {                                                                           \
    const int nn = nw + (TJ)*32 + il;                                         \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) {                          \
      const int mm = mw + (TI)*32 + (r & 3) + 8 * (r >> 2) + 4 * kh;          \
      atomicAdd(&C[(int64_t)mm * ldc + nn], alpha * ACC[r]);                  \
    }                                                                         \
  }
  OB_TN_EPI(acc00, 0, 0)
  OB_TN_EPI(acc01, 0, 1)
  OB_TN_EPI(acc10, 1, 0)
  OB_TN_EPI(acc11, 1, 1)
#undef OB_TN_EPI
}
