// ob_kernels_bf16.hip — the bf16 kernels of the mixed-precision path
// except the MFMA GEMMs (ob_gemm_bf16.hip) and flash attention
// (ob_flash_bf16.hip): layernorm, softmax, gelu, colsum, embed,
// cross-entropy, casts and the dW transpose (§8 f4: bf16 storage + fp32
// master weights; the reference never implemented mixed precision,
// README.md:98).
#include "ob_bf16.h"
#include "ob_internal.h"

#include <cmath>

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

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
// CPT = columns per thread: the block covers H <= 256 * CPT columns.  8 is
// the kernel as it always was (H <= 2048); 16, 32 and 48 carry wider rows
// (to 12288) with the same fixed-bound loops, so the accumulators stay in
// registers.
#define BLN_MAX_H (256 * 48)
// DET (deterministic mode): dw / db are this launch's
// partial slabs [gridDim.x][H]; the block stores its column sums to row
// blockIdx.x and ob_colpart_finish folds the rows in a fixed order.  Block b
// owns rows [16 b, 16 b + 16): a function of the shape alone.
template <bool DX_ACCUM, int CPT, bool DET = false>
__global__ __launch_bounds__(256) void k_ln_bwd_bf16(
    const __bf16* __restrict__ x, const float* __restrict__ w,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const __bf16* __restrict__ dy, __bf16* __restrict__ dx,
    float* __restrict__ dw, float* __restrict__ db, int64_t rows, int H) {
  __shared__ float lds4[4];
  const int64_t r0 = (int64_t)blockIdx.x * BLN_CHUNK;
  float accw[CPT] = {0}, accb[CPT] = {0};
  const int64_t rend = bmin64(rows, r0 + BLN_CHUNK);
  for (int64_t row = r0; row < rend; ++row) {
    const __bf16* xr = x + row * H;
    const __bf16* dyr = dy + row * H;
    const float mu = mean[row], rs = rstd[row];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
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
    for (int j = 0; j < CPT; ++j) {
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
  for (int j = 0; j < CPT; ++j) {
    const int c = threadIdx.x + j * 256;
    if (c < H) {
      if constexpr (DET) {
        dw[(int64_t)blockIdx.x * H + c] = accw[j];
        db[(int64_t)blockIdx.x * H + c] = accb[j];
      } else {
        atomicAdd(&dw[c], accw[j]);
        atomicAdd(&db[c], accb[j]);
      }
    }
  }
}

static int colpart_finish(const float* part, int64_t nblk, int64_t N,
                          int64_t ld, int64_t vstride, float* d0, float* d1,
                          float* d2, float* d3, void* stream);

// ws null: dw / db are added atomically; else (deterministic mode) through
// the slab ws, ob_det_ws_count(OB_DET_WS_LN, rows, H) floats
int ob_layernorm_bwd_ws(const void* x, const void* w, const void* mean,
                       const void* rstd, const void* dy, void* dx, void* dw,
                       void* db, int64_t rows, int64_t H, int dx_accum,
                       float* ws, void* stream) {
  if (H > BLN_MAX_H) return ob_fail("ln_bwd_bf16: H > 12288 unsupported");
  if (H % 8) return ob_fail("ln_bwd_bf16: H must be a multiple of 8");
  if (H >= 512 && H <= 1024)
    return ob_layernorm_bwd_res_ws(x, w, mean, rstd, dy, dx_accum ? dx : nullptr, dx,
                           dw, db, nullptr, nullptr, rows, H, ws, stream);
  if (ws && rows <= 0) return 0;
  const int grid = (int)((rows + BLN_CHUNK - 1) / BLN_CHUNK);
  // deterministic: the kernel's dw / db are the two slabs [grid][H]
  float* const pw = ws ? ws : (float*)dw;
  float* const pb = ws ? ws + (int64_t)grid * H : (float*)db;
#define OB_LNB(A_, C_, D_)                                               \
  k_ln_bwd_bf16<A_, C_, D_><<<grid, 256, 0, S(stream)>>>(                \
      (const __bf16*)x, (const float*)w, (const float*)mean,             \
      (const float*)rstd, (const __bf16*)dy, (__bf16*)dx, pw, pb, rows,  \
      (int)H)
  // the smallest columns-per-thread count that covers H
#define OB_LNB_H(A_, D_)                       \
  do {                                         \
    if (H <= 2048) OB_LNB(A_, 8, D_);          \
    else if (H <= 4096) OB_LNB(A_, 16, D_);    \
    else if (H <= 8192) OB_LNB(A_, 32, D_);    \
    else OB_LNB(A_, 48, D_);                   \
  } while (0)
  if (ws) {
    if (dx_accum) OB_LNB_H(true, true);
    else OB_LNB_H(false, true);
  } else {
    if (dx_accum) OB_LNB_H(true, false);
    else OB_LNB_H(false, false);
  }
#undef OB_LNB_H
#undef OB_LNB
  OB_LAUNCH_CHECK();
  if (ws)
    return colpart_finish(ws, grid, H, H, (int64_t)grid * H, (float*)dw,
                          (float*)db, nullptr, nullptr, stream);
  return 0;
}

extern "C" int ob_layernorm_bwd_bf16(const void* x, const void* w,
                                     const void* mean, const void* rstd,
                                     const void* dy, void* dx, void* dw,
                                     void* db, int64_t rows, int64_t H,
                                     int dx_accum, void* stream) {
  return ob_layernorm_bwd_ws(x, w, mean, rstd, dy, dx, dw, db, rows, H, dx_accum,
                     nullptr, stream);
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

// DET (deterministic mode): o0..o3 are partial slabs [gridDim.x][H]; the
// block stores its folded columns to row blockIdx.x.  Block b owns the
// 32-row chunks b, b + gridDim.x, ... and gridDim.x = min(chunks, 1024): a
// function of the row count alone, and every block has a chunk.
template <bool HAS_RES, bool SUMS, bool DET = false>
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
      if constexpr (DET) {
        if (out) out[(int64_t)blockIdx.x * H + c] = t;
      } else {
        if (out) atomicAdd(&out[c], t);
      }
    }
    __syncthreads();
  }
}

// dx = bf16(res + ln_bwd(x, dy)) (res null: no residual; res may equal dx);
// dw/db += as ob_layernorm_bwd_bf16; sum_res += colsum(res) and sum_dx +=
// colsum(dx) when non-null.  Widths outside the wave path compose the
// unfused kernels and give the same results.
int ob_layernorm_bwd_res_ws(const void* x, const void* w, const void* mean,
                           const void* rstd, const void* dy, const void* res,
                           void* dx, void* dw, void* db, void* sum_res,
                           void* sum_dx, int64_t rows, int64_t H, float* ws,
                           void* stream) {
  if (H > BLN_MAX_H) return ob_fail("ln_bwd_bf16: H > 12288 unsupported");
  if (H % 8) return ob_fail("ln_bwd_bf16: H must be a multiple of 8");
  if (sum_res && !res) return ob_fail("ln_bwd_res_bf16: sum_res needs res");
  if (rows <= 0) return 0;
  if (H >= 512 && H <= 1024) {
    const bool sums = sum_res || sum_dx;
    const int64_t nchunks = (rows + BLNR_ROWS - 1) / BLNR_ROWS;
    const int grid = (int)bmin64(nchunks, BLNR_MAXGRID);
    // deterministic: vector v's slab [grid][H] at ws + v * grid * H (null
    // outputs stay null)
    const int64_t vs = (int64_t)grid * H;
    float* const p0 = ws ? ws : (float*)dw;
    float* const p1 = ws ? ws + vs : (float*)db;
    float* const p2 = ws ? (sum_res ? ws + 2 * vs : nullptr) : (float*)sum_res;
    float* const p3 = ws ? (sum_dx ? ws + 3 * vs : nullptr) : (float*)sum_dx;
#define OB_LNRS(R_, S_, D_)                                                 \
  k_ln_bwd_bf16_rs<R_, S_, D_><<<grid, 64 * BLNR_WAVES, 0, S(stream)>>>(    \
      (const __bf16*)x, (const float*)w, (const float*)mean,                \
      (const float*)rstd, (const __bf16*)dy, (const __bf16*)res,            \
      (__bf16*)dx, p0, p1, p2, p3, rows, (int)H)
#define OB_LNRS_D(D_)                    \
  do {                                   \
    if (res) {                           \
      if (sums) OB_LNRS(true, true, D_); \
      else OB_LNRS(true, false, D_);     \
    } else {                             \
      if (sums) OB_LNRS(false, true, D_);\
      else OB_LNRS(false, false, D_);    \
    }                                    \
  } while (0)
    if (ws) OB_LNRS_D(true);
    else OB_LNRS_D(false);
#undef OB_LNRS_D
#undef OB_LNRS
    OB_LAUNCH_CHECK();
    if (ws)
      return colpart_finish(ws, grid, H, H, vs, (float*)dw, (float*)db,
                            (float*)sum_res, (float*)sum_dx, stream);
    return 0;
  }
  // composed path: colsum(res) first (res may alias dx), copy, ln, colsum
  // (deterministic: the three steps are stream-ordered and reuse the slab)
  if (sum_res && ob_colsum_ws(res, sum_res, rows, H, ws, stream)) return 1;
  if (res && res != dx)
    OB_HIP(hipMemcpyAsync(dx, res, (size_t)(rows * H) * sizeof(__bf16),
                          hipMemcpyDeviceToDevice, S(stream)));
  if (ob_layernorm_bwd_ws(x, w, mean, rstd, dy, dx, dw, db, rows, H, res ? 1 : 0, ws,
                  stream))
    return 1;
  if (sum_dx && ob_colsum_ws(dx, sum_dx, rows, H, ws, stream)) return 1;
  return 0;
}

extern "C" int ob_layernorm_bwd_res_bf16(const void* x, const void* w,
                                         const void* mean, const void* rstd,
                                         const void* dy, const void* res,
                                         void* dx, void* dw, void* db,
                                         void* sum_res, void* sum_dx,
                                         int64_t rows, int64_t H,
                                         void* stream) {
  return ob_layernorm_bwd_res_ws(x, w, mean, rstd, dy, res, dx, dw, db, sum_res,
                         sum_dx, rows, H, nullptr, stream);
}
extern "C" int ob_layernorm_bwd_res_det_bf16(
    const void* x, const void* w, const void* mean, const void* rstd,
    const void* dy, const void* res, void* dx, void* dw, void* db,
    void* sum_res, void* sum_dx, int64_t rows, int64_t H, void* ws,
    void* stream) {
  if (!ws) return ob_fail("ln_bwd_res_det_bf16: ws required");
  return ob_layernorm_bwd_res_ws(x, w, mean, rstd, dy, res, dx, dw, db, sum_res,
                         sum_dx, rows, H, (float*)ws, stream);
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

// DET (deterministic mode, both colsum kernels): db is the partial slab
// [gridDim.y][N]; the block stores its column sums to row blockIdx.y.  Block
// row y owns rows [T y, T y + T) (T = 256 here, 128 in v9): a function of the
// shape alone, and every (y, c < N) is written.
template <bool DET = false>
__global__ __launch_bounds__(256) void k_colsum_bf16(
    const __bf16* __restrict__ X, float* __restrict__ db, int64_t M,
    int64_t N) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  const int64_t r0 = (int64_t)blockIdx.y * 256;
  const int64_t r1 = bmin64(M, r0 + 256);
  float acc = 0.f;
  for (int64_t r = r0; r < r1; ++r) acc += bf2f(X[r * N + c]);
  if constexpr (DET) db[(int64_t)blockIdx.y * N + c] = acc;
  else atomicAdd(&db[c], acc);
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
// per block (DET: one slab store, see k_colsum_bf16).
template <bool DET = false>
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
    if (c < N) {
      const float t = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
      if constexpr (DET) db[(int64_t)blockIdx.y * N + c] = t;
      else atomicAdd(&db[c], t);
    }
  }
}

// ws null: atomic; else the deterministic form through the slab ws
// (ob_det_ws_count(OB_DET_WS_COLSUM, M, N) floats)
int ob_colsum_ws(const void* X, void* db, int64_t M, int64_t N,
                       float* ws, void* stream) {
  if (ws && (M <= 0 || N <= 0)) return 0;
  float* const dst = ws ? ws : (float*)db;
  int64_t nblk;
  if (N % 8 == 0) {
    nblk = (M + 127) / 128;
    dim3 grid((unsigned)((N + 63) / 64), (unsigned)nblk);
    if (ws)
      k_colsum_bf16_v9<true><<<grid, 256, 0, S(stream)>>>((const __bf16*)X,
                                                          dst, M, N);
    else
      k_colsum_bf16_v9<false><<<grid, 256, 0, S(stream)>>>((const __bf16*)X,
                                                           dst, M, N);
  } else {
    nblk = (M + 255) / 256;
    dim3 grid((unsigned)((N + 255) / 256), (unsigned)nblk);
    if (ws)
      k_colsum_bf16<true><<<grid, 256, 0, S(stream)>>>((const __bf16*)X, dst,
                                                       M, N);
    else
      k_colsum_bf16<false><<<grid, 256, 0, S(stream)>>>((const __bf16*)X, dst,
                                                        M, N);
  }
  OB_LAUNCH_CHECK();
  if (ws)
    return colpart_finish(ws, nblk, N, N, 0, (float*)db, nullptr, nullptr,
                          nullptr, stream);
  return 0;
}

extern "C" int ob_colsum_bf16(const void* X, void* db, int64_t M, int64_t N,
                              void* stream) {
  return ob_colsum_ws(X, db, M, N, nullptr, stream);
}
extern "C" int ob_colsum_det_bf16(const void* X, void* db, int64_t M,
                                  int64_t N, void* ws, void* stream) {
  if (!ws) return ob_fail("colsum_det_bf16: ws required");
  return ob_colsum_ws(X, db, M, N, (float*)ws, stream);
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
// DET (deterministic mode): db is the partial slab [gridDim.y][N], row
// blockIdx.y = rows [128 y, 128 y + 128), every (y, c < N) written.
template <bool DET = false>
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
    if (c < N) {
      const float t = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
      if constexpr (DET) db[(int64_t)blockIdx.y * N + c] = t;
      else atomicAdd(&db[c], t);
    }
  }
}

int ob_gelu_bwd_colsum_ws(const void* u, const void* dg, void* du,
                                void* db, int64_t M, int64_t N, float* ws,
                                void* stream) {
  if (M <= 0 || N <= 0) return 0;
  if (N % 8 == 0) {
    const int64_t nblk = (M + BGC_ROWS - 1) / BGC_ROWS;
    dim3 grid((unsigned)((N + 127) / 128), (unsigned)nblk);
    if (ws)
      k_gelu_bwd_cs_bf16<true><<<grid, 256, 0, S(stream)>>>(
          (const __bf16*)u, (const __bf16*)dg, (__bf16*)du, ws, M, N);
    else
      k_gelu_bwd_cs_bf16<false><<<grid, 256, 0, S(stream)>>>(
          (const __bf16*)u, (const __bf16*)dg, (__bf16*)du, (float*)db, M, N);
    OB_LAUNCH_CHECK();
    if (ws)
      return colpart_finish(ws, nblk, N, N, 0, (float*)db, nullptr, nullptr,
                            nullptr, stream);
    return 0;
  }
  // other widths compose the unfused kernels
  if (ob_gelu_bwd_bf16(u, dg, du, M * N, stream)) return 1;
  return ob_colsum_ws(du, db, M, N, ws, stream);
}

extern "C" int ob_gelu_bwd_colsum_bf16(const void* u, const void* dg,
                                       void* du, void* db, int64_t M,
                                       int64_t N, void* stream) {
  return ob_gelu_bwd_colsum_ws(u, dg, du, db, M, N, nullptr, stream);
}
extern "C" int ob_gelu_bwd_colsum_det_bf16(const void* u, const void* dg,
                                           void* du, void* db, int64_t M,
                                           int64_t N, void* ws,
                                           void* stream) {
  if (!ws) return ob_fail("gelu_bwd_colsum_det_bf16: ws required");
  return ob_gelu_bwd_colsum_ws(u, dg, du, db, M, N, (float*)ws, stream);
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
// shift/mean semantics match the fp32 kernels.  DET (deterministic mode):
// loss is the [BS] slab; every row stores its term (0 for the last position
// of a sequence) and k_ce_fold adds the slab to the scalar in a fixed order.
template <bool DET = false>
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
        const float term = (l - bf2f(lr[lab])) * inv;
        if constexpr (DET) loss[row] = term;
        else atomicAdd(loss, term);
      } else if constexpr (DET) {
        loss[row] = 0.f;
      }
    }
    __syncthreads();
  }
}
// loss += fold(part[0..n)): thread t adds part[t], part[t + 256], ... in
// ascending order, thread 0 then adds the 256 thread sums in ascending t
// (threads with no element skipped).  One block: the order depends on n only.
__global__ __launch_bounds__(256) void k_ce_fold(
    const float* __restrict__ part, int64_t n, float* __restrict__ loss) {
  __shared__ float red[256];
  const int t = threadIdx.x;
  float s = 0.f;
  if (t < n) {
    s = part[t];
    for (int64_t i = t + 256; i < n; i += 256) s += part[i];
  }
  red[t] = s;
  __syncthreads();
  if (t == 0) {
    float a = red[0];
    const int m = n < 256 ? (int)n : 256;
    for (int k = 1; k < m; ++k) a += red[k];
    loss[0] += a;
  }
}
// ws null: the loss is added atomically; else (deterministic mode) through
// the B * Sq float slab ws
int ob_ce_fwd_ws(const void* logits, const void* labels, void* lse,
                 void* loss, int64_t B, int64_t Sq, int64_t V, int64_t ld,
                 float* ws, void* stream) {
  if (ws && B * Sq <= 0) return 0;
  const int grid = (int)bmin64(B * Sq, 16384);
  if (ws)
    k_ce_fwd_bf16<true><<<grid, 256, 0, S(stream)>>>(
        (const __bf16*)logits, (const int64_t*)labels, (float*)lse, ws,
        B * Sq, (int)Sq, (int)V, ld);
  else
    k_ce_fwd_bf16<false><<<grid, 256, 0, S(stream)>>>(
        (const __bf16*)logits, (const int64_t*)labels, (float*)lse,
        (float*)loss, B * Sq, (int)Sq, (int)V, ld);
  OB_LAUNCH_CHECK();
  if (ws) {
    k_ce_fold<<<1, 256, 0, S(stream)>>>(ws, B * Sq, (float*)loss);
    OB_LAUNCH_CHECK();
  }
  return 0;
}
extern "C" int ob_ce_fwd_bf16(const void* logits, const void* labels,
                              void* lse, void* loss, int64_t B, int64_t Sq,
                              int64_t V, int64_t ld, void* stream) {
  return ob_ce_fwd_ws(logits, labels, lse, loss, B, Sq, V, ld, nullptr,
                      stream);
}

// ob_ce_fwd_bf16 with a run-to-run bit-stable loss; ws: B * Sq floats
extern "C" int ob_ce_fwd_det_bf16(const void* logits, const void* labels,
                                  void* lse, void* loss, int64_t B,
                                  int64_t Sq, int64_t V, int64_t ld, void* ws,
                                  void* stream) {
  if (!ws) return ob_fail("ce_fwd_det_bf16: ws required");
  return ob_ce_fwd_ws(logits, labels, lse, loss, B, Sq, V, ld, (float*)ws,
                      stream);
}

// ---------------------------------------------------------------------------
// Deterministic mode: the fixed-order fold of a partial
// slab.  dst[c] += fold(part[0..nblk)[c]) with this association, which
// depends on nblk only: group g (0..7) adds rows g, g + 8, g + 16, ... in
// ascending order starting from row g's value; the groups' sums are then
// added in ascending g starting from group 0's (groups beyond nblk do not
// exist); that total is added to dst[c].  Block = 32 columns x 8 groups;
// blockIdx.y picks one of up to four vectors whose slabs lie vstride floats
// apart (a null dst is skipped).  No atomics: one thread owns dst[c].
// ---------------------------------------------------------------------------
#define CPF_COLS 32
#define CPF_GROUPS 8
__global__ __launch_bounds__(CPF_COLS * CPF_GROUPS) void k_colpart_finish(
    const float* __restrict__ part, int nblk, int64_t N, int64_t ld,
    int64_t vstride, float* d0, float* d1, float* d2, float* d3) {
  __shared__ float red[CPF_GROUPS][CPF_COLS];
  const int v = blockIdx.y;
  float* const dst = v == 0 ? d0 : v == 1 ? d1 : v == 2 ? d2 : d3;
  if (!dst) return;  // block-uniform
  const float* p = part + (int64_t)v * vstride;
  const int cl = threadIdx.x & (CPF_COLS - 1), g = threadIdx.x / CPF_COLS;
  const int64_t c = (int64_t)blockIdx.x * CPF_COLS + cl;
  float s = 0.f;
  if (c < N && g < nblk) {
    s = p[(int64_t)g * ld + c];
    for (int b = g + CPF_GROUPS; b < nblk; b += CPF_GROUPS)
      s += p[(int64_t)b * ld + c];
  }
  red[g][cl] = s;
  __syncthreads();
  if (g == 0 && c < N) {
    float t = red[0][cl];
    const int ng = nblk < CPF_GROUPS ? nblk : CPF_GROUPS;
    for (int k = 1; k < ng; ++k) t += red[k][cl];
    dst[c] += t;
  }
}

static int colpart_finish(const float* part, int64_t nblk, int64_t N,
                          int64_t ld, int64_t vstride, float* d0, float* d1,
                          float* d2, float* d3, void* stream) {
  if (nblk <= 0 || N <= 0) return 0;
  if (nblk > INT32_MAX) return ob_fail("colpart_finish: nblk too large");
  const int nv = d3 ? 4 : d2 ? 3 : d1 ? 2 : 1;
  dim3 grid((unsigned)((N + CPF_COLS - 1) / CPF_COLS), (unsigned)nv);
  k_colpart_finish<<<grid, CPF_COLS * CPF_GROUPS, 0, S(stream)>>>(
      part, (int)nblk, N, ld, vstride, d0, d1, d2, d3);
  OB_LAUNCH_CHECK();
  return 0;
}

extern "C" int ob_colpart_finish_f32(const void* part, int64_t nblk,
                                     int64_t N, int64_t ld, void* dst,
                                     void* stream) {
  if (!part || !dst) return ob_fail("colpart_finish_f32: null arg");
  if (ld < N) return ob_fail("colpart_finish_f32: ld < N");
  return colpart_finish((const float*)part, nblk, N, ld, 0, (float*)dst,
                        nullptr, nullptr, nullptr, stream);
}

// host-only: floats of slab a _det entry needs (the grids above)
extern "C" int64_t ob_det_ws_count(int which, int64_t M, int64_t N) {
  if (M <= 0 || N <= 0) return 0;
  const int64_t cs = N % 8 == 0 ? (M + 127) / 128 * N : (M + 255) / 256 * N;
  switch (which) {
    case OB_DET_WS_COLSUM:
      return cs;
    case OB_DET_WS_GELU:
      return N % 8 == 0 ? (M + BGC_ROWS - 1) / BGC_ROWS * N : cs;
    case OB_DET_WS_LN: {
      if (N >= 512 && N <= 1024)
        return 4 * bmin64((M + BLNR_ROWS - 1) / BLNR_ROWS, BLNR_MAXGRID) * N;
      const int64_t ln = 2 * ((M + BLN_CHUNK - 1) / BLN_CHUNK) * N;
      return ln > cs ? ln : cs;
    }
    case OB_DET_WS_DROP_CS:
      return ob_drop_cs_ws_count(M, N);
    case OB_DET_WS_CE:
      return M;
  }
  return -1;
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

