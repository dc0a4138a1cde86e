// Global gradient-norm clipping fused into the AdamW step:
//   ob_sqnorm_multi_f32   per-tensor fp64 square norms of fp32 buffers
//   ob_clip_finish        total norm -> clip coefficient device record
//   ob_adamw_step_scaled  AdamW consuming g * coef (coef read on device)
//
// The square norm is deterministic by construction (heterogeneous pipeline
// replicas must arrive at the same clip coefficient bit for bit): element j
// of a tensor of n elements always lands in chunk j / SQ_CHUNK, on thread
// ((j % SQ_CHUNK) / 4) % 256, in accumulator j % 4, in ascending j.  Chunk
// partials are PLAIN stores into a caller-owned slab; a second launch adds
// each tensor's partials in a fixed order.  No atomics on any result, and
// nothing depends on the pointer's alignment, the tensor's position in the
// list or what else shares the launch.
#include "ob_internal.h"

#include <cmath>

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
static inline int64_t imin64(int64_t a, int64_t b) { return a < b ? a : b; }

#define SQ_CHUNK 16384  // elements per workgroup: 256 threads x 16 float4
#define SQ_ITERS (SQ_CHUNK / (256 * 4))
#define SQ_MAXT 64      // tensors per launch table (passed by value)

struct SqTable {
  const float* p[SQ_MAXT];
  int64_t n[SQ_MAXT];
  int32_t cstart[SQ_MAXT + 1];  // chunk prefix within this launch
  int32_t out[SQ_MAXT];
  int32_t nt;
};

// fixed-order sum of one double per thread over a 256-thread block
__device__ __forceinline__ double block_sum_f64(double s, double* sm) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
  __syncthreads();
  return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// x*x of an fp32 is exact in fp64, so the only rounding is the summation
#define SQ_ACC(a, x) a = fma((double)(x), (double)(x), a)

template <bool ALIGNED>
__device__ __forceinline__ double sq_chunk(const float* __restrict__ p,
                                           int64_t rem) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  const int tid = threadIdx.x;
  if (rem >= SQ_CHUNK) {
#pragma unroll 8
    for (int it = 0; it < SQ_ITERS; ++it) {
      const int e = (it * 256 + tid) * 4;
      float x0, x1, x2, x3;
      if (ALIGNED) {
        const float4 x = *reinterpret_cast<const float4*>(p + e);
        x0 = x.x; x1 = x.y; x2 = x.z; x3 = x.w;
      } else {
        x0 = p[e]; x1 = p[e + 1]; x2 = p[e + 2]; x3 = p[e + 3];
      }
      SQ_ACC(a0, x0); SQ_ACC(a1, x1); SQ_ACC(a2, x2); SQ_ACC(a3, x3);
    }
  } else {
    for (int it = 0; it < SQ_ITERS; ++it) {
      const int e = (it * 256 + tid) * 4;
      if (e >= rem) break;
      if (ALIGNED && e + 3 < rem) {
        const float4 x = *reinterpret_cast<const float4*>(p + e);
        SQ_ACC(a0, x.x); SQ_ACC(a1, x.y); SQ_ACC(a2, x.z); SQ_ACC(a3, x.w);
      } else {
        SQ_ACC(a0, p[e]);
        if (e + 1 < rem) SQ_ACC(a1, p[e + 1]);
        if (e + 2 < rem) SQ_ACC(a2, p[e + 2]);
        if (e + 3 < rem) SQ_ACC(a3, p[e + 3]);
      }
    }
  }
  return (a0 + a1) + (a2 + a3);
}

// one workgroup per chunk: ws[block] = that chunk's square sum
__global__ __launch_bounds__(256) void k_sqnorm_partial(
    const SqTable tb, double* __restrict__ ws) {
  __shared__ double sm[4];
  const int b = blockIdx.x;
  int lo = 0, hi = tb.nt;  // last t with cstart[t] <= b (skips empty tensors)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tb.cstart[mid] <= b) lo = mid; else hi = mid;
  }
  const int64_t base = (int64_t)(b - tb.cstart[lo]) * SQ_CHUNK;
  const float* p = tb.p[lo] + base;
  const int64_t rem = tb.n[lo] - base;
  const bool aligned = (reinterpret_cast<uintptr_t>(tb.p[lo]) & 15) == 0;
  double s = aligned ? sq_chunk<true>(p, rem) : sq_chunk<false>(p, rem);
  s = block_sum_f64(s, sm);
  if (threadIdx.x == 0) ws[b] = s;
}

// one workgroup per tensor: add its chunk partials in a fixed order
__global__ __launch_bounds__(256) void k_sqnorm_finish(
    const SqTable tb, const double* __restrict__ ws,
    double* __restrict__ out) {
  __shared__ double sm[4];
  const int t = blockIdx.x;
  const int c1 = tb.cstart[t + 1];
  double s = 0.0;
  for (int i = tb.cstart[t] + threadIdx.x; i < c1; i += 256) s += ws[i];
  s = block_sum_f64(s, sm);
  if (threadIdx.x == 0) out[tb.out[t]] = s;
}

static inline int64_t sq_chunks(int64_t n) {
  return (n + SQ_CHUNK - 1) / SQ_CHUNK;
}

extern "C" int64_t ob_sqnorm_ws_count(const int64_t* counts, int32_t n) {
  int64_t tot = 0;
  for (int32_t i = 0; i < n; ++i)
    if (counts[i] > 0) tot += sq_chunks(counts[i]);
  return tot;
}

extern "C" int ob_sqnorm_multi_f32(const void* const* ptrs,
                                   const int64_t* counts,
                                   const int32_t* out_index, int32_t n,
                                   void* ws, void* out, void* stream) {
  if (n < 0 || (n > 0 && (!ptrs || !counts || !out)))
    return ob_fail("sqnorm: null arg");
  for (int32_t i = 0; i < n; ++i) {
    if (counts[i] < 0 || (counts[i] > 0 && !ptrs[i]))
      return ob_fail("sqnorm: tensor %d: bad pointer/count", i);
    if (reinterpret_cast<uintptr_t>(ptrs[i]) & 3)
      return ob_fail("sqnorm: tensor %d not 4-byte aligned", i);
    if (out_index && out_index[i] < 0)
      return ob_fail("sqnorm: tensor %d: negative out_index", i);
  }
  if (ob_sqnorm_ws_count(counts, n) > 0 && !ws)
    return ob_fail("sqnorm: workspace required");
  const int prof_slot =
      ob_prof_on() ? ob_prof_beg(OB_PF_ADAMW, S(stream)) : -1;
  double* wsd = static_cast<double*>(ws);
  for (int32_t t0 = 0; t0 < n;) {
    SqTable tb;
    int nt = 0;
    int64_t chunks = 0;
    // fill one table: up to SQ_MAXT tensors and an int32 / grid-sized
    // chunk count (a single oversized tensor still gets a table of its own)
    while (t0 + nt < n && nt < SQ_MAXT) {
      const int64_t c = sq_chunks(counts[t0 + nt]);
      if (c > 0x7fffffff) {
        if (prof_slot >= 0) ob_prof_end(OB_PF_ADAMW, prof_slot, S(stream));
        return ob_fail("sqnorm: tensor %d too large", t0 + nt);
      }
      if (nt > 0 && chunks + c > 0x7fffffff) break;
      tb.p[nt] = static_cast<const float*>(ptrs[t0 + nt]);
      tb.n[nt] = counts[t0 + nt];
      tb.cstart[nt] = (int32_t)chunks;
      tb.out[nt] = out_index ? out_index[t0 + nt] : t0 + nt;
      chunks += c;
      ++nt;
    }
    for (int i = nt; i < SQ_MAXT; ++i) {
      tb.p[i] = nullptr;
      tb.n[i] = 0;
      tb.out[i] = 0;
    }
    for (int i = nt; i <= SQ_MAXT; ++i) tb.cstart[i] = (int32_t)chunks;
    tb.nt = nt;
    if (chunks > 0)
      k_sqnorm_partial<<<(unsigned)chunks, 256, 0, S(stream)>>>(tb, wsd);
    k_sqnorm_finish<<<nt, 256, 0, S(stream)>>>(tb, wsd,
                                               static_cast<double*>(out));
    wsd += chunks;
    t0 += nt;
  }
  if (prof_slot >= 0) ob_prof_end(OB_PF_ADAMW, prof_slot, S(stream));
  OB_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// stats = {total_sq, norm, coef, skipped_steps}; coef < 0 is the skip marker
// ---------------------------------------------------------------------------
__global__ void k_clip_finish(const double* __restrict__ sq, int n,
                              float max_norm, double* __restrict__ stats) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double tot = 0.0;
  for (int i = 0; i < n; ++i) tot += sq[i];  // index order: split-independent
  const double norm = sqrt(tot);
  stats[0] = tot;
  stats[1] = norm;
  if (!__builtin_isfinite(norm)) {  // Inf/NaN total (or a negative one)
    stats[2] = -1.0;
    stats[3] += 1.0;
  } else {
    double c = (double)max_norm / (norm + 1e-6);
    if (c > 1.0) c = 1.0;
    stats[2] = (double)(float)c;
  }
}

extern "C" int ob_clip_finish(const void* sq, int32_t n, float max_norm,
                              void* stats, void* stream) {
  if (n < 0 || (n > 0 && !sq) || !stats) return ob_fail("clip_finish: null arg");
  if (!(max_norm > 0.f)) return ob_fail("clip_finish: max_norm must be > 0");
  const int prof_slot =
      ob_prof_on() ? ob_prof_beg(OB_PF_ADAMW, S(stream)) : -1;
  k_clip_finish<<<1, 64, 0, S(stream)>>>(static_cast<const double*>(sq), n,
                                         max_norm,
                                         static_cast<double*>(stats));
  if (prof_slot >= 0) ob_prof_end(OB_PF_ADAMW, prof_slot, S(stream));
  OB_LAUNCH_CHECK();
  return 0;
}

// k_adamw with g[i] * coef in place of g[i]; same 28 B/param traffic (the
// scaled gradient is not written back).  On the skip marker nothing is
// touched.
__global__ __launch_bounds__(256) void k_adamw_scaled(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
    float* __restrict__ v, int64_t n, float wd_factor, float step_size,
    float inv_sqrt_bc2, float beta1, float beta2, float eps,
    const double* __restrict__ stats) {
  const float coef = (float)stats[2];
  if (coef < 0.f) return;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * 256) {
    ob_adamw_update(p, m, v, i, g[i] * coef, wd_factor, step_size,
                    inv_sqrt_bc2, beta1, beta2, eps);
  }
}

extern "C" int ob_adamw_step_scaled(void* p, const void* g, void* m, void* v,
                                    int64_t n, int32_t step, float lr,
                                    float beta1, float beta2, float eps,
                                    float weight_decay, const void* clip_stats,
                                    void* stream) {
  if (step < 1) return ob_fail("adamw_scaled: step must be >= 1");
  if (!clip_stats) return ob_fail("adamw_scaled: clip_stats required");
  if (n <= 0) return 0;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const int grid = (int)imin64((n + 255) / 256, 4096);
  const int prof_slot =
      ob_prof_on() ? ob_prof_beg(OB_PF_ADAMW, S(stream)) : -1;
  k_adamw_scaled<<<grid, 256, 0, S(stream)>>>(
      (float*)p, (const float*)g, (float*)m, (float*)v, n,
      1.f - lr * weight_decay, (float)(lr / bc1), (float)(1.0 / sqrt(bc2)),
      beta1, beta2, eps, static_cast<const double*>(clip_stats));
  if (prof_slot >= 0) ob_prof_end(OB_PF_ADAMW, prof_slot, S(stream));
  OB_LAUNCH_CHECK();
  return 0;
}
