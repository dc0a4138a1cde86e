// ob_blaslt.hip — hipBLASLt path for the PLAIN GEMMs of the hot path.
//
// The hand-written MFMA kernels (ob_gemm_bf16.hip) carry every FUSED
// op (bias/residual epilogues, flash attention, LN, CE); the plain
// library GEMMs — dX (activation grads), the bias-free lm_head family,
// and the TN weight-grad GEMMs (beta=1 accumulation straight into the
// fp32 flat grads, which also deletes the transpose materialization) —
// go to AMD's own hipBLASLt, per the MI355X playbook ("hipBLASLt /
// rocBLAS only for plain library GEMMs").  Measured on the hot shapes
// (tools/blas_probe.py): fc 815 TF, dX_fc 963, lm_head 1166, dW-TN 694
// vs 436-692 for our kernels.
//
// Row-major calls are expressed through the standard column-major swap:
//   C_rm[M,N] = op(A_rm) op(B_rm)  ==>  C̄(N,M) = op'(B̄) op'(Ā)
// with X̄ = the stored bytes viewed column-major (X^T).
//
// WHICH solution runs a shape: a process-wide choice
// table, keyed by ob_lt_shape, holds the solution index the tuner (lt_tune,
// below) measured best among the heuristic's candidates.  Each stream's
// plan for a shape is built from that index, so all streams run the same
// solution; a shape without an entry gets the heuristic's first candidate.
// The tuner is host code called from layer_create and the ob_gemm_lt_tune
// export, never from a step.  OB_LT_TUNE=0 disables it.
#include "ob_internal.h"
#include "ob_dw_slices.h"

#include <hipblaslt/hipblaslt-ext.hpp>
#include <hipblaslt/hipblaslt.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

namespace {

constexpr size_t kLtWs = 64u << 20;

struct Key {
  ob_lt_shape s;
  // > 1 (plan caches only): the K-slices of s as one strided-batched problem
  // of that many entries, beta = 0, each into its own [M, N] slab
  int batch = 1;
  auto tie() const {
    return std::tie(s.tA, s.tB, s.M, s.N, s.K, s.lda, s.ldb, s.ldc, s.c_f32,
                    s.beta1, s.bias, s.cin, s.ab_f32, batch);
  }
  bool operator<(const Key& o) const { return tie() < o.tie(); }
};

// descriptor + layouts of one shape
struct LtProblem {
  hipblasLtMatmulDesc_t desc = nullptr;
  hipblasLtMatrixLayout_t la = nullptr, lb = nullptr, lc = nullptr;
};

struct LtPlan {
  LtProblem p;
  hipblasLtMatmulAlgo_t algo{};
  int index = -1;
  bool ok = false;
  bool untuned = false;  // built while the choice table had no entry
  // unsliced plans: the table's slice count for this shape (1: run unsliced)
  int slices = 1;
};

// ONE FULL CONTEXT PER STREAM — handle + workspace + plan cache.
// Concurrent enqueue of Lt matmuls on different streams through a single
// shared handle stalls pathologically at queue depth (measured: the pp1
// fwd/bwd dual-stream bench never finishes a 16-microbatch step with a
// shared handle, and runs fine with hipBLASLt disabled) — the handle
// carries internal per-launch state that cross-stream reuse serializes
// against.  Streams are few (main + fwd/bwd + side) and long-lived.
struct LtCtx {
  hipblasLtHandle_t h = nullptr;
  void* ws = nullptr;
  std::map<Key, LtPlan> plans;
};
std::map<void*, LtCtx> g_lt_by_stream;

// the process-wide choice table
struct LtChoice {
  int index = -1;       // the solution every stream's plan is built from
  int top1_index = -1;  // the heuristic's first candidate
  bool tuned = false;   // false: tuning was abandoned, plans use top-1
  double us_top1 = 0, us_chosen = 0;
  int tried = 0, dropped = 0;
  double wall_ms = 0;
  double spread_top1 = 0;  // top-1's max - min over the rounds: the margin
  std::string top1_name, chosen_name;
  // every candidate that was timed: solution index, position in the
  // candidate list, median microseconds
  struct Timed {
    int index, pos;
    double us;
  };
  std::vector<Timed> timed;
  // the sliced call (ob_dw_slices.h): slices > 1 runs the shape as that many
  // K-slices with solution slice_index of the batched problem, then the fold
  int slices = 1, slice_index = -1;
  double us_sliced = 0;  // the fastest sliced pair's median, chosen or not
  double slice_ms = 0;   // host time the sliced candidates added to wall_ms
  struct Sliced {
    int slices, index, pos;
    double us;  // median of matmul + fold
  };
  std::vector<Sliced> sliced;
};
std::mutex g_tab_mu;
std::map<Key, LtChoice> g_tab;
std::atomic<int64_t> g_untuned_uses{0};

bool lt_tune_on() {
  static const bool on = ob_env_flag("OB_LT_TUNE", true);
  // deterministic mode: the tuned choice is a per-process measurement, so
  // every plan is the heuristic's top-1, as with OB_LT_TUNE=0
  return on && !ob_deterministic();
}

LtCtx* lt_ctx(void* stream) {
  auto it = g_lt_by_stream.find(stream);
  if (it != g_lt_by_stream.end()) return &it->second;
  LtCtx ctx;
  if (hipblasLtCreate(&ctx.h) != HIPBLAS_STATUS_SUCCESS) return nullptr;
  if (hipMalloc(&ctx.ws, kLtWs) != hipSuccess) return nullptr;
  return &g_lt_by_stream.emplace(stream, ctx).first->second;
}

void lt_problem_create(const ob_lt_shape& k0, const void* bias, LtProblem* p,
                       int batch = 1) {
  // batch > 1: entry i is K-slice i of k0, rows i*K/batch on of A and B, and
  // writes slab i of a dense [batch, M, N] output
  ob_lt_shape k = k0;
  if (batch > 1) k.K = k0.K / batch, k.ldc = k0.N;
  // column-major swap: A-slot <- B bytes, B-slot <- A bytes
  const hipblasOperation_t opA = k.tB ? HIPBLAS_OP_T : HIPBLAS_OP_N;
  const hipblasOperation_t opB = k.tA ? HIPBLAS_OP_T : HIPBLAS_OP_N;
  // cm dims of the A-slot (B̄): stored rm [K,N] or [N,K] -> cm (N,K)^T…
  // rows/cols BEFORE op, with ld = the rm row stride:
  //   B rm [K,N] (tB=0): B̄ is (N x K) cm, ld = ldb; op N gives (N x K)?
  // We need op(Aslot) = (N x K).  tB=0: B̄ = (N x K) already -> op N.
  // tB=1: B rm [N,K] -> B̄ = (K x N) -> op T gives (N x K).  Symmetric
  // for the B-slot: op(Bslot) = (K x M) from Ā.
  const int64_t a_rows = k.tB ? k.K : k.N, a_cols = k.tB ? k.N : k.K;
  const int64_t b_rows = k.tA ? k.M : k.K, b_cols = k.tA ? k.K : k.M;
  hipblasLtMatmulDescCreate(&p->desc, HIPBLAS_COMPUTE_32F, HIP_R_32F);
  hipblasLtMatmulDescSetAttribute(p->desc, HIPBLASLT_MATMUL_DESC_TRANSA, &opA,
                                  sizeof(opA));
  hipblasLtMatmulDescSetAttribute(p->desc, HIPBLASLT_MATMUL_DESC_TRANSB, &opB,
                                  sizeof(opB));
  if (k.bias) {
    const hipblasLtEpilogue_t ep = HIPBLASLT_EPILOGUE_BIAS;
    hipblasLtMatmulDescSetAttribute(p->desc, HIPBLASLT_MATMUL_DESC_EPILOGUE,
                                    &ep, sizeof(ep));
    const int32_t bt = HIP_R_32F;
    hipblasLtMatmulDescSetAttribute(
        p->desc, HIPBLASLT_MATMUL_DESC_BIAS_DATA_TYPE, &bt, sizeof(bt));
    hipblasLtMatmulDescSetAttribute(
        p->desc, HIPBLASLT_MATMUL_DESC_BIAS_POINTER, &bias, sizeof(bias));
  }
  const hipDataType abt = k.ab_f32 ? HIP_R_32F : HIP_R_16BF;
  hipblasLtMatrixLayoutCreate(&p->la, abt, a_rows, a_cols, k.ldb);
  hipblasLtMatrixLayoutCreate(&p->lb, abt, b_rows, b_cols, k.lda);
  hipblasLtMatrixLayoutCreate(&p->lc, k.c_f32 ? HIP_R_32F : HIP_R_16BF, k.N,
                              k.M, k.ldc);
  if (batch > 1) {
    const int32_t n = batch;
    const int64_t sa = k.K * k.ldb, sb = k.K * k.lda, sc = k.M * k.N;
    const std::pair<hipblasLtMatrixLayout_t, int64_t> ls[] = {
        {p->la, sa}, {p->lb, sb}, {p->lc, sc}};
    for (const auto& l : ls) {
      hipblasLtMatrixLayoutSetAttribute(
          l.first, HIPBLASLT_MATRIX_LAYOUT_BATCH_COUNT, &n, sizeof(n));
      hipblasLtMatrixLayoutSetAttribute(
          l.first, HIPBLASLT_MATRIX_LAYOUT_STRIDED_BATCH_OFFSET, &l.second,
          sizeof(l.second));
    }
  }
}

void lt_problem_destroy(LtProblem* p) {
  if (p->la) hipblasLtMatrixLayoutDestroy(p->la);
  if (p->lb) hipblasLtMatrixLayoutDestroy(p->lb);
  if (p->lc) hipblasLtMatrixLayoutDestroy(p->lc);
  if (p->desc) hipblasLtMatmulDescDestroy(p->desc);
  *p = LtProblem();
}

// up to n candidates in the heuristic's order, workspace <= kLtWs
int lt_heuristic(hipblasLtHandle_t h, const LtProblem& p, int n,
                 hipblasLtMatmulHeuristicResult_t* res) {
  hipblasLtMatmulPreference_t pref;
  hipblasLtMatmulPreferenceCreate(&pref);
  const uint64_t ws = kLtWs;
  hipblasLtMatmulPreferenceSetAttribute(
      pref, HIPBLASLT_MATMUL_PREF_MAX_WORKSPACE_BYTES, &ws, sizeof(ws));
  int nres = 0;
  const hipblasStatus_t st = hipblasLtMatmulAlgoGetHeuristic(
      h, p.desc, p.la, p.lb, p.lc, p.lc, pref, n, res, &nres);
  hipblasLtMatmulPreferenceDestroy(pref);
  return st == HIPBLAS_STATUS_SUCCESS ? nres : 0;
}

// the table's solution for this handle and problem, if it still fits
bool lt_algo_from_index(hipblasLtHandle_t h, const LtProblem& p,
                        float beta, int index, hipblasLtMatmulAlgo_t* algo) {
  std::vector<int> idx{index};
  std::vector<hipblasLtMatmulHeuristicResult_t> r;
  if (hipblaslt_ext::getAlgosFromIndex(h, idx, r) != HIPBLAS_STATUS_SUCCESS ||
      r.empty())
    return false;
  const float alpha = 1.f;
  size_t need = 0;
  if (hipblaslt_ext::matmulIsAlgoSupported(h, p.desc, &alpha, p.la, p.lb,
                                           &beta, p.lc, p.lc, r[0].algo,
                                           need) != HIPBLAS_STATUS_SUCCESS ||
      need > kLtWs)
    return false;
  *algo = r[0].algo;
  return true;
}

LtPlan lt_plan_build(LtCtx* ctx, const Key& key, const void* bias) {
  LtPlan p;
  lt_problem_create(key.s, bias, &p.p, key.batch);
  int index = -1;
  {
    // the table is keyed by the unsliced shape; a sliced plan takes the
    // table's batched solution when it was measured for this slice count
    std::lock_guard<std::mutex> lk(g_tab_mu);
    auto it = g_tab.find(Key{key.s});
    if (it == g_tab.end()) {
      p.untuned = lt_tune_on() && key.batch == 1;
    } else if (it->second.tuned && lt_tune_on()) {
      if (key.batch == 1)
        index = it->second.index, p.slices = it->second.slices;
      else if (it->second.slices == key.batch)
        index = it->second.slice_index;
    }
  }
  const float beta = key.batch == 1 && key.s.beta1 ? 1.f : 0.f;
  if (index >= 0 && lt_algo_from_index(ctx->h, p.p, beta, index, &p.algo)) {
    p.index = index;
    p.ok = true;
    return p;
  }
  hipblasLtMatmulHeuristicResult_t res[1];
  if (lt_heuristic(ctx->h, p.p, 1, res) > 0 &&
      res[0].state == HIPBLAS_STATUS_SUCCESS) {
    p.algo = res[0].algo;
    p.index = hipblaslt_ext::getIndexFromAlgo(p.algo);
    p.ok = true;
  }
  return p;
}

// ---- sliced weight grads (ob_dw_slices.h) ----------------

// OB_DW_SLICES (read once): 0 / unset the tuner decides, 1 never slice, n
// force n slices wherever the rule admits them (probing)
int dw_slices_env() {
  static const int n = ob_env_int("OB_DW_SLICES", 0);
  return n < 0 ? 0 : n;
}

// CUs of the current device; 0 (nothing is sliced) if it cannot be asked
int lt_cus() {
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

ob_dw_slice_shape dw_slice_shape(const ob_lt_shape& k) {
  return {k.tA, k.tB, k.c_f32, k.beta1, !k.bias && !k.cin && !k.ab_f32,
          k.M,  k.N,  k.K,     k.ldc};
}

// The fold of a sliced weight grad: g[j] += slab[0][j] + ... + slab[S-1][j]
// for j < n, the slabs n floats apart.  The slabs are summed in ascending
// order in fp32 and the total is added to g once; one thread owns its W
// elements, so there are no atomics and the result depends on S alone.  All
// S + 1 loads are issued before the first add.  W = 4 needs g and slab
// 16-byte aligned and n % 4 == 0.  Bound by memory: (S + 2) * 4n bytes.
// (Outside the unnamed namespace so that profiles show it by name.)
}  // namespace

template <int S, int W>
__global__ __launch_bounds__(256) void k_dw_fold(float* __restrict__ g,
                                                 const float* __restrict__ slab,
                                                 int64_t n) {
  using V = typename std::conditional<W == 4, float4, float>::type;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n / W) return;
  V v[S];
#pragma unroll
  for (int k = 0; k < S; k++)
    v[k] = reinterpret_cast<const V*>(slab + (int64_t)k * n)[i];
  V acc = reinterpret_cast<const V*>(g)[i];
  V t = v[0];
#pragma unroll
  for (int k = 1; k < S; k++) t += v[k];
  acc += t;
  reinterpret_cast<V*>(g)[i] = acc;
}

namespace {

template <int W>
int dw_fold_w(float* g, const float* slab, int s, int64_t n, hipStream_t st) {
  const int64_t blocks = (n / W + 255) / 256;
  if (blocks > INT32_MAX) return ob_fail("dw_fold: output too large");
  const dim3 grid((unsigned)blocks);
  switch (s) {
    case 2: k_dw_fold<2, W><<<grid, 256, 0, st>>>(g, slab, n); break;
    case 4: k_dw_fold<4, W><<<grid, 256, 0, st>>>(g, slab, n); break;
    case 8: k_dw_fold<8, W><<<grid, 256, 0, st>>>(g, slab, n); break;
    case 16: k_dw_fold<16, W><<<grid, 256, 0, st>>>(g, slab, n); break;
    default: return ob_fail("dw_fold: %d slices", s);
  }
  OB_LAUNCH_CHECK();
  return 0;
}

int dw_fold(float* g, const float* slab, int s, int64_t n, hipStream_t st) {
  if (n <= 0) return 0;
  const bool vec = n % 4 == 0 && (uintptr_t)g % 16 == 0 &&
                   (uintptr_t)slab % 16 == 0;
  return vec ? dw_fold_w<4>(g, slab, s, n, st) : dw_fold_w<1>(g, slab, s, n, st);
}

// ---- tuner ----------------------------------------------------------------

// values in [-1, 1) from an integer hash of the index
__global__ void k_lt_fill(void* p, int64_t n, int f32, uint32_t seed) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t h = (uint32_t)i * 2654435761u + (uint32_t)(i >> 32) + seed;
    h ^= h >> 16, h *= 0x7feb352du, h ^= h >> 15, h *= 0x846ca68bu;
    h ^= h >> 16;
    const float v = (float)(h >> 16) * (1.f / 32768.f) - 1.f;
    if (f32) ((float*)p)[i] = v;
    else ((__bf16*)p)[i] = (__bf16)v;
  }
}

// acc[0] += sum (x - ref)^2, acc[1] += sum ref^2
__global__ void k_lt_diff(const void* x, const void* ref, int64_t n, int f32,
                          double* acc) {
  double d2 = 0, r2 = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float a = f32 ? ((const float*)x)[i] : (float)((const __bf16*)x)[i];
    const float b =
        f32 ? ((const float*)ref)[i] : (float)((const __bf16*)ref)[i];
    d2 += (double)(a - b) * (a - b);
    r2 += (double)b * b;
  }
  __shared__ double sd[256], sr[256];
  sd[threadIdx.x] = d2, sr[threadIdx.x] = r2;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      sd[threadIdx.x] += sd[threadIdx.x + s];
      sr[threadIdx.x] += sr[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    atomicAdd(&acc[0], sd[0]);
    atomicAdd(&acc[1], sr[0]);
  }
}

double median_of(std::vector<float> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

// scratch of one tuning run; everything is released by the destructor
struct TuneScratch {
  hipStream_t stream = nullptr;
  hipblasLtHandle_t h = nullptr;
  void *ws = nullptr, *A = nullptr, *B = nullptr, *C = nullptr, *Cref = nullptr,
       *Cin = nullptr, *bias = nullptr, *slab = nullptr;
  double* acc = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  LtProblem p;
  std::vector<LtProblem> sp;  // the batched problems, one per slice count
  ~TuneScratch() {
    lt_problem_destroy(&p);
    for (LtProblem& q : sp) lt_problem_destroy(&q);
    for (void* q : {ws, A, B, C, Cref, Cin, bias, slab, (void*)acc})
      if (q) (void)hipFree(q);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (h) hipblasLtDestroy(h);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

struct Cand {
  hipblasLtMatmulAlgo_t algo;
  int pos = 0;  // position in the candidate list
  int slices = 1, prob = -1;  // > 1: a sliced pair on batched problem sp[prob]
  int reps = 1;
  float warm_us = 0.f;
  std::vector<float> us;  // per round, per call
};

// Measures the heuristic's candidates for one shape and fills *out.  Returns
// false when tuning was abandoned (allocation failure or any HIP error):
// the caller keeps top-1.  slab_floats > 0: the caller can run the shape
// sliced with a slab that large, so for every slice count the rule admits
// the first candidates of the batched problem, each followed by the fold,
// are measured in the same rounds.
bool lt_tune_run(const ob_lt_shape& k, int64_t slab_floats, LtChoice* out) {
  const int n_env = ob_env_int("OB_LT_TUNE_N", 8);
  const int n_max = n_env < 1 ? 1 : n_env > 128 ? 128 : n_env;
  constexpr int kRounds = 5;
  TuneScratch t;
#define LT_TRY(x) \
  if ((x) != hipSuccess) return false
  LT_TRY(hipStreamCreateWithFlags(&t.stream, hipStreamNonBlocking));
  if (hipblasLtCreate(&t.h) != HIPBLAS_STATUS_SUCCESS) return false;
  LT_TRY(hipEventCreate(&t.e0));
  LT_TRY(hipEventCreate(&t.e1));
  const size_t es_ab = k.ab_f32 ? 4 : 2, es_c = k.c_f32 ? 4 : 2;
  const int64_t nA = (k.tA ? k.K : k.M) * k.lda;
  const int64_t nB = (k.tB ? k.N : k.K) * k.ldb;
  const int64_t nC = k.M * k.ldc;
  LT_TRY(hipMalloc(&t.ws, kLtWs));
  LT_TRY(hipMalloc(&t.A, nA * es_ab));
  LT_TRY(hipMalloc(&t.B, nB * es_ab));
  LT_TRY(hipMalloc(&t.C, nC * es_c));
  LT_TRY(hipMalloc(&t.Cref, nC * es_c));
  LT_TRY(hipMalloc((void**)&t.acc, 2 * sizeof(double)));
  if (k.cin) LT_TRY(hipMalloc(&t.Cin, nC * es_c));
  if (k.bias) LT_TRY(hipMalloc(&t.bias, k.N * sizeof(float)));
  auto fill = [&](void* p, int64_t n, int f32, uint32_t seed) {
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 4096);
    k_lt_fill<<<(unsigned)blocks, 256, 0, t.stream>>>(p, n, f32, seed);
  };
  fill(t.A, nA, k.ab_f32, 1u);
  fill(t.B, nB, k.ab_f32, 2u);
  if (t.Cin) fill(t.Cin, nC, k.c_f32, 3u);
  if (t.bias) fill(t.bias, k.N, 1, 4u);
  LT_TRY(hipGetLastError());
  lt_problem_create(k, t.bias, &t.p);

  std::vector<hipblasLtMatmulHeuristicResult_t> res(n_max);
  res.resize(std::max(0, lt_heuristic(t.h, t.p, n_max, res.data())));
  if (res.empty() || res[0].state != HIPBLAS_STATUS_SUCCESS) return false;
  out->top1_index = hipblaslt_ext::getIndexFromAlgo(res[0].algo);
  out->top1_name = hipblaslt_ext::getKernelNameFromAlgo(t.h, res[0].algo);

  const float alpha = 1.f, beta = k.beta1 ? 1.f : 0.f;
  // OB_LT_TUNE_ALL=1 (tools): behind the heuristic's list, every solution of
  // the library for these types and transposes that supports the problem
  if (ob_env_flag("OB_LT_TUNE_ALL", false)) {
    std::vector<hipblasLtMatmulHeuristicResult_t> every;
    const hipDataType abt = k.ab_f32 ? HIP_R_32F : HIP_R_16BF;
    const hipDataType ct = k.c_f32 ? HIP_R_32F : HIP_R_16BF;
    if (hipblaslt_ext::getAllAlgos(
            t.h, hipblaslt_ext::GemmType::HIPBLASLT_GEMM,
            k.tB ? HIPBLAS_OP_T : HIPBLAS_OP_N,
            k.tA ? HIPBLAS_OP_T : HIPBLAS_OP_N, abt, abt, ct, ct,
            HIPBLAS_COMPUTE_32F, every) == HIPBLAS_STATUS_SUCCESS) {
      std::set<int> seen;
      for (auto& r : res) seen.insert(hipblaslt_ext::getIndexFromAlgo(r.algo));
      for (auto& r : every) {
        size_t need = 0;
        if (!seen.insert(hipblaslt_ext::getIndexFromAlgo(r.algo)).second)
          continue;
        if (hipblaslt_ext::matmulIsAlgoSupported(
                t.h, t.p.desc, &alpha, t.p.la, t.p.lb, &beta, t.p.lc, t.p.lc,
                r.algo, need) != HIPBLAS_STATUS_SUCCESS ||
            need > kLtWs)
          continue;
        r.state = HIPBLAS_STATUS_SUCCESS;
        res.push_back(r);
      }
    }
  }
  const int nres = (int)res.size();
  std::vector<Cand> listed;
  for (int i = 0; i < nres; i++) {
    if (res[i].state != HIPBLAS_STATUS_SUCCESS) {
      out->dropped++;
      continue;
    }
    Cand c;
    c.algo = res[i].algo;
    c.pos = i;
    listed.push_back(c);
  }
  // candidate 0, the reference of the gate and of the hysteresis, is the
  // heuristic's first unsliced answer; without one the shape is abandoned
  if (listed.empty() || listed[0].pos != 0 || listed[0].slices != 1)
    return false;
  // the sliced pairs: per admissible slice count, the first OB_LT_TUNE_SLICE_N
  // (default 2) candidates of the batched problem.  OB_DW_SLICES=1 lists
  // none, OB_DW_SLICES=n only those of n slices.
  const auto ts0 = std::chrono::steady_clock::now();
  auto since = [](std::chrono::steady_clock::time_point a) {
    return std::chrono::duration<double, std::milli>(
               std::chrono::steady_clock::now() - a)
        .count();
  };
  const int forced = dw_slices_env();
  int slist[4], ns = 0;
  if (slab_floats > 0 && forced != 1)
    ns = ob_dw_slices_list(dw_slice_shape(k), lt_cus(), slab_floats, slist);
  if (ns > 0) {
    const int per_env = ob_env_int("OB_LT_TUNE_SLICE_N", 2);
    const int per = per_env < 1 ? 1 : per_env > 8 ? 8 : per_env;
    int smax = 0;
    for (int j = 0; j < ns; j++) {
      const int s = slist[j];
      if (forced > 1 ? s != forced : s > OB_DW_SLICES_AUTO_MAX) continue;
      t.sp.emplace_back();
      lt_problem_create(k, nullptr, &t.sp.back(), s);
      hipblasLtMatmulHeuristicResult_t sres[8];
      const int got = lt_heuristic(t.h, t.sp.back(), per, sres);
      for (int i = 0; i < got; i++) {
        if (sres[i].state != HIPBLAS_STATUS_SUCCESS) continue;
        Cand c;
        c.algo = sres[i].algo;
        c.pos = i, c.slices = s, c.prob = (int)t.sp.size() - 1;
        listed.push_back(c);
        smax = s;
      }
    }
    if (smax) LT_TRY(hipMalloc(&t.slab, (size_t)smax * k.M * k.N * 4));
  }
  out->slice_ms += since(ts0);
  // one call; into dst for the gate, into C when timing.  A beta=1 call
  // without a separate C-input accumulates into its (zeroed) output.  A
  // sliced pair is the batched beta=0 matmul into the slab and the fold of
  // the slab into dst.
  const float zero = 0.f;
  auto run = [&](Cand& c, void* dst) {
    if (c.slices > 1) {
      const LtProblem& q = t.sp[c.prob];
      const hipblasStatus_t st = hipblasLtMatmul(
          t.h, q.desc, &alpha, t.B, q.la, t.A, q.lb, &zero, t.slab, q.lc,
          t.slab, q.lc, &c.algo, t.ws, kLtWs, t.stream);
      if (st != HIPBLAS_STATUS_SUCCESS) return st;
      return dw_fold((float*)dst, (const float*)t.slab, c.slices, k.M * k.N,
                     t.stream)
                 ? HIPBLAS_STATUS_INTERNAL_ERROR
                 : HIPBLAS_STATUS_SUCCESS;
    }
    return hipblasLtMatmul(t.h, t.p.desc, &alpha, t.B, t.p.la, t.A, t.p.lb,
                           &beta, t.Cin ? t.Cin : dst, t.p.lc, dst, t.p.lc,
                           &c.algo, t.ws, kLtWs, t.stream);
  };
  // correctness gate: every candidate once, against candidate 0's output on
  // the same inputs.  Both are exact bf16 products summed in fp32 in another
  // order: one output ulp for bf16, the project's rtol for fp32 accumulation.
  const double bound = k.c_f32 ? 1e-3 : 1.0 / 256;
  std::vector<Cand> cands;
  for (size_t i = 0; i < listed.size(); i++) {
    const auto tc0 = std::chrono::steady_clock::now();
    const bool sliced = listed[i].slices > 1;
    void* dst = i == 0 ? t.Cref : t.C;
    LT_TRY(hipMemsetAsync(dst, 0, nC * es_c, t.stream));
    const hipblasStatus_t st = run(listed[i], dst);
    if (i == 0 && st != HIPBLAS_STATUS_SUCCESS) return false;
    if (st != HIPBLAS_STATUS_SUCCESS) {
      LT_TRY(hipStreamSynchronize(t.stream));
      out->dropped++;
      continue;
    }
    if (i > 0) {
      LT_TRY(hipMemsetAsync(t.acc, 0, 2 * sizeof(double), t.stream));
      const int64_t blocks = std::min<int64_t>((nC + 255) / 256, 4096);
      k_lt_diff<<<(unsigned)blocks, 256, 0, t.stream>>>(t.C, t.Cref, nC,
                                                        k.c_f32, t.acc);
      double acc[2] = {0, 0};
      LT_TRY(hipMemcpyAsync(acc, t.acc, sizeof(acc), hipMemcpyDeviceToHost,
                            t.stream));
      LT_TRY(hipStreamSynchronize(t.stream));
      if (!(acc[0] <= bound * bound * acc[1])) {
        out->dropped++;
        continue;
      }
    } else {
      LT_TRY(hipStreamSynchronize(t.stream));
    }
    cands.push_back(listed[i]);
    if (sliced) out->slice_ms += since(tc0);
  }
  out->tried = nres;
  // a visit: events around reps back-to-back calls, read only after the
  // closing event completed; it includes whatever else the library enqueues.
  // A library status other than success drops the candidate (V_DROP, after
  // the stream drained); a HIP error abandons the shape (V_HIP).
  enum { V_OK = 0, V_DROP = 1, V_HIP = 2 };
  auto visit = [&](Cand& c, int reps, float* us) {
    if (hipEventRecord(t.e0, t.stream) != hipSuccess) return (int)V_HIP;
    bool lib_ok = true;
    for (int r = 0; r < reps && lib_ok; r++)
      lib_ok = run(c, t.C) == HIPBLAS_STATUS_SUCCESS;
    float ms = 0.f;
    if (hipEventRecord(t.e1, t.stream) != hipSuccess ||
        hipEventSynchronize(t.e1) != hipSuccess ||
        hipEventElapsedTime(&ms, t.e0, t.e1) != hipSuccess)
      return (int)V_HIP;
    if (!lib_ok) return (int)V_DROP;
    *us = ms * 1000.f / reps;
    return (int)V_OK;
  };
  // a dropped candidate leaves the list and is counted; candidate 0 cannot
  // be dropped, the shape is abandoned instead
  auto drop = [&](size_t i) {
    if (i == 0) return false;
    cands.erase(cands.begin() + i);
    out->dropped++;
    return true;
  };
  auto reps_for = [](float us) {
    return std::max(1, std::min(4096, (int)(1250.f / std::max(us, 0.25f)) + 1));
  };
  LT_TRY(hipMemsetAsync(t.C, 0, nC * es_c, t.stream));
  // warm each candidate twice: one call, then a window of 8 calls whose
  // per-call time (launch and event overhead spread over 8) sizes reps for
  // a window of 1.25 ms
  for (size_t i = 0; i < cands.size();) {
    Cand& c = cands[i];
    const auto tc0 = std::chrono::steady_clock::now();
    float us = 0.f;
    int v = visit(c, 1, &us);
    if (v == V_OK) v = visit(c, 8, &us);
    if (c.slices > 1) out->slice_ms += since(tc0);
    if (v == V_HIP || (v == V_DROP && !drop(i))) return false;
    if (v == V_DROP) continue;
    c.warm_us = us;
    c.reps = reps_for(us);
    i++;
  }
  // an unsliced list longer than n_max (OB_LT_TUNE_ALL): the rounds go to
  // candidate 0 and the n_max - 1 fastest of the warm visits (the sliced
  // pairs stand behind the unsliced candidates and all stay)
  const int n_unsl = (int)std::count_if(
      cands.begin(), cands.end(), [](const Cand& c) { return c.slices == 1; });
  if (n_unsl > n_max) {
    std::stable_sort(cands.begin() + 1, cands.begin() + n_unsl,
                     [](const Cand& a, const Cand& b) {
                       return a.warm_us < b.warm_us;
                     });
    cands.erase(cands.begin() + n_max, cands.begin() + n_unsl);
  }
  // rounds visit all candidates round-robin, so clock drift and neighbours
  // hit them alike.  A window that came out under 1 ms is not scored: reps
  // grows and the visit is repeated.
  for (int r = 0; r < kRounds; r++)
    for (size_t i = 0; i < cands.size();) {
      Cand& c = cands[i];
      const auto tc0 = std::chrono::steady_clock::now();
      float us = 0.f;
      int v = V_OK;
      for (int attempt = 0; attempt < 4; attempt++) {
        v = visit(c, c.reps, &us);
        if (v != V_OK || us * c.reps >= 1000.f || c.reps >= 4096) break;
        c.reps = std::max(c.reps + 1, reps_for(us));
      }
      if (c.slices > 1) out->slice_ms += since(tc0);
      if (v == V_HIP || (v == V_DROP && !drop(i))) return false;
      if (v == V_DROP) continue;
      c.us.push_back(us);
      i++;
    }
  LT_TRY(hipStreamSynchronize(t.stream));
#undef LT_TRY
  // keep candidate 0 unless the best median beats its median by more than
  // candidate 0's own spread over the rounds AND the challenger won every
  // round (its slowest round under candidate 0's fastest): the choice is
  // made per process, and two processes should not split over a near tie
  const double med0 = median_of(cands[0].us);
  const double spread0 =
      *std::max_element(cands[0].us.begin(), cands[0].us.end()) -
      *std::min_element(cands[0].us.begin(), cands[0].us.end());
  size_t best = 0;
  double best_med = med0;
  out->timed.push_back(
      {hipblaslt_ext::getIndexFromAlgo(cands[0].algo), 0, med0});
  for (size_t i = 1; i < cands.size() && cands[i].slices == 1; i++) {
    const double m = median_of(cands[i].us);
    out->timed.push_back(
        {hipblaslt_ext::getIndexFromAlgo(cands[i].algo), cands[i].pos, m});
    if (m < best_med) best_med = m, best = i;
  }
  out->spread_top1 = spread0;
  const double min0 =
      *std::min_element(cands[0].us.begin(), cands[0].us.end());
  if (!(best_med < med0 - spread0) ||
      !(*std::max_element(cands[best].us.begin(), cands[best].us.end()) <
        min0))
    best = 0, best_med = med0;
  out->us_top1 = med0;
  out->us_chosen = best_med;
  out->index = hipblaslt_ext::getIndexFromAlgo(cands[best].algo);
  out->chosen_name = hipblaslt_ext::getKernelNameFromAlgo(t.h, cands[best].algo);
  // the sliced pairs, by the same hysteresis: the shape stays unsliced unless
  // the fastest pair's median beats top-1's by more than top-1's spread, won
  // every round against top-1, and is under the chosen unsliced median too.
  // OB_DW_SLICES=n takes the fastest pair of n slices as it is.
  size_t sbest = 0;
  double sbest_med = 0;
  for (size_t i = 1; i < cands.size(); i++) {
    if (cands[i].slices == 1) continue;
    const double m = median_of(cands[i].us);
    out->sliced.push_back({cands[i].slices,
                           hipblaslt_ext::getIndexFromAlgo(cands[i].algo),
                           cands[i].pos, m});
    if (!sbest || m < sbest_med) sbest_med = m, sbest = i;
  }
  if (sbest) {
    out->us_sliced = sbest_med;
    const bool wins =
        sbest_med < med0 - spread0 && sbest_med < best_med &&
        *std::max_element(cands[sbest].us.begin(), cands[sbest].us.end()) <
            min0;
    if (wins || forced > 1) {
      out->slices = cands[sbest].slices;
      out->slice_index = hipblaslt_ext::getIndexFromAlgo(cands[sbest].algo);
    }
  }
  out->tuned = true;
  return true;
}

Key key_from_i64(const int64_t* v) {
  Key key;
  ob_lt_shape& s = key.s;
  s.tA = v[0] != 0, s.tB = v[1] != 0, s.M = v[2], s.N = v[3], s.K = v[4];
  s.lda = v[5], s.ldb = v[6], s.ldc = v[7], s.c_f32 = v[8] != 0;
  s.beta1 = v[9] != 0, s.bias = v[10] != 0, s.cin = v[11] != 0;
  s.ab_f32 = v[12] != 0;
  return key;
}

}  // namespace

int ob_lt_tune_shape(const ob_lt_shape& s, int64_t slab_floats) {
  if (!lt_tune_on()) return 0;
  if (s.M <= 0 || s.N <= 0 || s.K <= 0 || s.ldc < s.N ||
      s.lda < (s.tA ? s.M : s.K) || s.ldb < (s.tB ? s.K : s.N))
    return ob_fail("lt_tune: bad shape");
  const Key key{s};
  {
    std::lock_guard<std::mutex> lk(g_tab_mu);
    if (g_tab.count(key)) return 0;
  }
  // never beside the step streams
  OB_HIP(hipDeviceSynchronize());
  const auto t0 = std::chrono::steady_clock::now();
  LtChoice c;
  if (!lt_tune_run(s, slab_floats, &c)) {
    // abandoned: the entry stays untuned (plans use top-1) and is not retried
    c.tuned = false;
    c.index = c.top1_index;
    (void)hipGetLastError();
  }
  (void)hipDeviceSynchronize();
  c.wall_ms = std::chrono::duration<double, std::milli>(
                  std::chrono::steady_clock::now() - t0)
                  .count();
  {
    std::lock_guard<std::mutex> lk(g_tab_mu);
    g_tab.emplace(key, c);
  }
  // plans built for this shape before it had an entry are rebuilt
  for (auto& sc : g_lt_by_stream)
    for (int batch = 1; batch <= OB_DW_SLICES_MAX; batch *= 2) {
      auto it = sc.second.plans.find(Key{s, batch});
      if (it == sc.second.plans.end()) continue;
      lt_problem_destroy(&it->second.p);
      sc.second.plans.erase(it);
    }
  return 0;
}

// Plain row-major GEMM: C[M,N] = alpha * op(A) op(B) + beta * C.
// A is [M,K] (or [K,M] if tA), B is [K,N] (or [N,K] if tB), bf16,
// fp32 accumulate; C bf16 (c_f32 == 0) or fp32 (c_f32 == 1).
// Returns 0 on success, -1 if no algo (caller falls back), 1 on error.
// bias (optional, fp32, length N) is applied via the BIAS epilogue —
// in the column-major swap D = C-bar (N x M), whose rows are our output
// columns, exactly the broadcast hipBLASLt defines.
// Cin: the C-INPUT operand (D = alpha*op(A)op(B) + beta*Cin, written to
// C) — hipblasLt supports C != D, which folds a residual WITHOUT the
// 12.6 MB copy the round-1 path paid per forward projection GEMM.
static const LtPlan* lt_plan_get(LtCtx* ctx, const Key& key,
                                 const void* bias) {
  auto it = ctx->plans.find(key);
  if (it == ctx->plans.end())
    it = ctx->plans.emplace(key, lt_plan_build(ctx, key, bias)).first;
  return &it->second;
}

static int lt_matmul(int tA, int tB, int64_t M, int64_t N, int64_t K,
                     float alpha, const void* A, int64_t lda, const void* B,
                     int64_t ldb, float beta, void* C, int64_t ldc,
                     int c_f32, const void* bias, int ab_f32, void* stream,
                     const void* Cin = nullptr) {
  if (!Cin) Cin = C;
  LtCtx* ctx = lt_ctx(stream);
  if (!ctx) return ob_fail("hipblasLt per-stream context init failed");
  const Key key{ob_lt_shape_of(tA, tB, M, N, K, lda, ldb, ldc, c_f32, beta,
                               bias != nullptr, Cin != C, ab_f32)};
  const LtPlan& p = *lt_plan_get(ctx, key, bias);
  if (!p.ok) return -1;
  if (p.untuned) g_untuned_uses.fetch_add(1, std::memory_order_relaxed);
  if (bias)
    hipblasLtMatmulDescSetAttribute(
        p.p.desc, HIPBLASLT_MATMUL_DESC_BIAS_POINTER, &bias, sizeof(bias));
  const hipblasStatus_t st = hipblasLtMatmul(
      ctx->h, p.p.desc, &alpha, B, p.p.la, A, p.p.lb, &beta, Cin, p.p.lc, C,
      p.p.lc, &p.algo, ctx->ws, kLtWs, reinterpret_cast<hipStream_t>(stream));
  if (st != HIPBLAS_STATUS_SUCCESS)
    return ob_fail("hipblasLtMatmul failed (%d)", (int)st);
  return 0;
}

// The sliced form of a TN weight grad C[M,N] += A[K,M]^T B[K,N]: one
// strided-batched matmul whose entry i is K-slice i, beta = 0, into slab i of
// slab[n, M, N], then k_dw_fold adds the slabs to C.  The caller has asked
// the rule (ob_dw_slices_ok), so ldc == N and the slab holds n * M * N
// floats.  -1, with nothing enqueued, if the library has no solution.
static int lt_dw_sliced(LtCtx* ctx, const ob_lt_shape& s, int n, const void* A,
                        const void* B, float* C, float* slab, void* stream) {
  const LtPlan& p = *lt_plan_get(ctx, Key{s, n}, nullptr);
  if (!p.ok) return -1;
  const float one = 1.f, zero = 0.f;
  const hipblasStatus_t st = hipblasLtMatmul(
      ctx->h, p.p.desc, &one, B, p.p.la, A, p.p.lb, &zero, slab, p.p.lc, slab,
      p.p.lc, &p.algo, ctx->ws, kLtWs, reinterpret_cast<hipStream_t>(stream));
  if (st != HIPBLAS_STATUS_SUCCESS)
    return ob_fail("hipblasLtMatmul (sliced) failed (%d)", (int)st);
  return dw_fold(C, slab, n, s.M * s.N, reinterpret_cast<hipStream_t>(stream));
}

// The layer's weight grad (dw_bf16_ws): sliced when the choice table says so
// for this shape and the slab still fits, else the plain beta = 1 call.  A
// call either slices or runs unsliced, never both.
int ob_lt_dw_run(const ob_lt_shape& s, const void* act, const void* dY,
                 float* gout, float* slab, int64_t slab_floats, void* stream) {
  LtCtx* ctx = lt_ctx(stream);
  if (!ctx) return ob_fail("hipblasLt per-stream context init failed");
  // the unsliced plan is built (and kept) for a sliced shape too: it carries
  // the table's slice count, and it is what runs if the slab no longer fits
  const int n = lt_plan_get(ctx, Key{s}, nullptr)->slices;
  if (n > 1 && slab &&
      ob_dw_slices_ok(dw_slice_shape(s), n, lt_cus(), slab_floats)) {
    const int r = lt_dw_sliced(ctx, s, n, act, dY, gout, slab, stream);
    if (r >= 0) return r;
  }
  return lt_matmul(s.tA, s.tB, s.M, s.N, s.K, 1.f, act, s.lda, dY, s.ldb, 1.f,
                   gout, s.ldc, s.c_f32, nullptr, 0, stream);
}

// The sliced weight grad with an explicit slice count (tests, probes):
// C[M,N] += A[K,M]^T B[K,N], bf16 operands, fp32 C.  s slices if the rule
// admits them on this device with this slab, else unsliced; *used (optional)
// gets the count that ran.  The choice table and OB_DW_SLICES play no part.
extern "C" int ob_gemm_lt_dw_sliced(int64_t M, int64_t N, int64_t K,
                                    const void* A, int64_t lda, const void* B,
                                    int64_t ldb, void* C, int64_t ldc, int s,
                                    void* slab, int64_t slab_floats,
                                    void* stream, int32_t* used) {
  if (!A || !B || !C) return ob_fail("gemm_lt_dw_sliced: null operand");
  if (M <= 0 || N <= 0 || K <= 0 || lda < M || ldb < N || ldc < N)
    return ob_fail("gemm_lt_dw_sliced: bad shape");
  const ob_lt_shape k = ob_lt_dw(M, N, K, lda);
  ob_lt_shape kk = k;
  kk.ldb = ldb, kk.ldc = ldc;
  if (used) *used = 1;
  LtCtx* ctx = lt_ctx(stream);
  if (!ctx) return ob_fail("hipblasLt per-stream context init failed");
  if (slab && ob_dw_slices_ok(dw_slice_shape(kk), s, lt_cus(), slab_floats)) {
    const int r =
        lt_dw_sliced(ctx, kk, s, A, B, (float*)C, (float*)slab, stream);
    if (r == 0 && used) *used = s;
    if (r >= 0) return r;
  }
  const int r = lt_matmul(1, 0, M, N, K, 1.f, A, lda, B, ldb, 1.f, C, ldc, 1,
                          nullptr, 0, stream);
  return r < 0 ? ob_fail("gemm_lt_dw_sliced: the library has no solution") : r;
}

// host-only: does the rule (ob_dw_slices.h) admit s slices of this shape on a
// device of cus CUs with a slab of slab_floats floats?
extern "C" int ob_dw_slices_admit(const int64_t* shape, int s, int cus,
                                  int64_t slab_floats) {
  if (!shape) return 0;
  return ob_dw_slices_ok(dw_slice_shape(key_from_i64(shape).s), s, cus,
                         slab_floats)
             ? 1
             : 0;
}

extern "C" int ob_gemm_lt(int tA, int tB, int64_t M, int64_t N, int64_t K,
                          float alpha, const void* A, int64_t lda,
                          const void* B, int64_t ldb, float beta, void* C,
                          int64_t ldc, int c_f32, void* stream) {
  return lt_matmul(tA, tB, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc,
                   c_f32, nullptr, 0, stream);
}

extern "C" int ob_gemm_lt_bias(int tA, int tB, int64_t M, int64_t N,
                               int64_t K, float alpha, const void* A,
                               int64_t lda, const void* B, int64_t ldb,
                               float beta, void* C, int64_t ldc, int c_f32,
                               const void* bias, void* stream) {
  return lt_matmul(tA, tB, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc,
                   c_f32, bias, 0, stream);
}

/* bias epilogue + residual folded as the C-input (no copy) */
extern "C" int ob_gemm_lt_bias_res(int tA, int tB, int64_t M, int64_t N,
                                   int64_t K, float alpha, const void* A,
                                   int64_t lda, const void* B, int64_t ldb,
                                   void* C, int64_t ldc, int c_f32,
                                   const void* bias, const void* residual,
                                   void* stream) {
  return lt_matmul(tA, tB, M, N, K, alpha, A, lda, B, ldb, 1.f, C, ldc,
                   c_f32, bias, 0, stream, residual);
}

// fp32 operands, fp32 accumulate/out (the reference-dtype leg)
extern "C" int ob_gemm_lt_f32(int tA, int tB, int64_t M, int64_t N,
                              int64_t K, float alpha, const void* A,
                              int64_t lda, const void* B, int64_t ldb,
                              float beta, void* C, int64_t ldc,
                              void* stream) {
  return lt_matmul(tA, tB, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, 1,
                   nullptr, 1, stream);
}

// ---- host-only queries (shape = OB_LT_SHAPE_FIELDS int64s, the order of
// ob_lt_shape) ---------------------------------------------------------------

extern "C" int ob_gemm_lt_tune(const int64_t* shape) {
  if (!shape) return ob_fail("gemm_lt_tune: null shape");
  return ob_lt_tune_shape(key_from_i64(shape).s);
}

// ob_gemm_lt_tune for a caller that can run the shape sliced with a slab of
// slab_floats floats (what ob_layer_create does for a BLOCK's weight grads)
extern "C" int ob_gemm_lt_tune_slab(const int64_t* shape,
                                    int64_t slab_floats) {
  if (!shape) return ob_fail("gemm_lt_tune_slab: null shape");
  return ob_lt_tune_shape(key_from_i64(shape).s,
                          slab_floats > 0 ? slab_floats : 0);
}

extern "C" int ob_gemm_lt_choice(const int64_t* shape, double* out,
                                 char* top1_name, char* chosen_name,
                                 int name_cap) {
  if (!shape || !out) return ob_fail("gemm_lt_choice: null argument");
  const Key key = key_from_i64(shape);
  std::lock_guard<std::mutex> lk(g_tab_mu);
  auto it = g_tab.find(key);
  for (int i = 0; i < 10; i++) out[i] = 0;
  if (top1_name && name_cap > 0) top1_name[0] = 0;
  if (chosen_name && name_cap > 0) chosen_name[0] = 0;
  if (it == g_tab.end()) return 0;
  const LtChoice& c = it->second;
  out[0] = 1, out[1] = c.index, out[2] = c.tuned, out[3] = c.top1_index;
  out[4] = c.us_top1, out[5] = c.us_chosen, out[6] = c.tried;
  out[7] = c.dropped, out[8] = c.wall_ms, out[9] = c.spread_top1;
  if (top1_name && name_cap > 0)
    snprintf(top1_name, name_cap, "%s", c.top1_name.c_str());
  if (chosen_name && name_cap > 0)
    snprintf(chosen_name, name_cap, "%s", c.chosen_name.c_str());
  return 0;
}

// The sliced side of a shape's table entry.  out[0] = entry found, out[1] =
// the slice count the step runs (1: unsliced), out[2] = the batched problem's
// solution index (-1 unsliced), out[3] = the fastest sliced pair's median
// microseconds (matmul + fold; 0 if none was timed), out[4] = the
// milliseconds the sliced candidates added to the shape's tuning time,
// out[5] = that fastest pair's slice count.  Every sliced pair that was timed
// goes to slices/index/us, fastest first; returns their number.
extern "C" int ob_gemm_lt_slices(const int64_t* shape, double* out,
                                 int32_t* slices, int32_t* index, double* us,
                                 int cap) {
  if (!shape || !out || (cap > 0 && (!slices || !index || !us))) return -1;
  for (int i = 0; i < 6; i++) out[i] = 0;
  std::lock_guard<std::mutex> lk(g_tab_mu);
  auto it = g_tab.find(key_from_i64(shape));
  if (it == g_tab.end()) return 0;
  const LtChoice& c = it->second;
  auto v = c.sliced;
  std::stable_sort(v.begin(), v.end(),
                   [](const LtChoice::Sliced& a, const LtChoice::Sliced& b) {
                     return a.us < b.us;
                   });
  out[0] = 1, out[1] = c.tuned ? c.slices : 1;
  out[2] = c.tuned ? c.slice_index : -1, out[3] = c.us_sliced;
  out[4] = c.slice_ms, out[5] = v.empty() ? 1 : v[0].slices;
  for (int i = 0; i < (int)v.size() && i < cap; i++)
    slices[i] = v[i].slices, index[i] = v[i].index, us[i] = v[i].us;
  return (int)v.size();
}

// the candidates the tuner timed for a shape, fastest first: solution index,
// position in the candidate list, median microseconds; returns their number
extern "C" int ob_gemm_lt_candidates(const int64_t* shape, int32_t* index,
                                     int32_t* pos, double* us, int cap) {
  if (!shape || (cap > 0 && (!index || !pos || !us))) return -1;
  std::lock_guard<std::mutex> lk(g_tab_mu);
  auto it = g_tab.find(key_from_i64(shape));
  if (it == g_tab.end()) return 0;
  auto v = it->second.timed;
  std::stable_sort(v.begin(), v.end(),
                   [](const LtChoice::Timed& a, const LtChoice::Timed& b) {
                     return a.us < b.us;
                   });
  for (int i = 0; i < (int)v.size() && i < cap; i++)
    index[i] = v[i].index, pos[i] = v[i].pos, us[i] = v[i].us;
  return (int)v.size();
}

extern "C" int64_t ob_gemm_lt_table_size(void) {
  std::lock_guard<std::mutex> lk(g_tab_mu);
  return (int64_t)g_tab.size();
}

extern "C" int64_t ob_gemm_lt_untuned_uses(void) {
  return g_untuned_uses.load(std::memory_order_relaxed);
}

// the solution index of this stream's plan for a shape; -1 without a plan
extern "C" int ob_gemm_lt_plan_index(const int64_t* shape, void* stream) {
  if (!shape) return -1;
  auto sc = g_lt_by_stream.find(stream);
  if (sc == g_lt_by_stream.end()) return -1;
  auto it = sc->second.plans.find(key_from_i64(shape));
  return it == sc->second.plans.end() || !it->second.ok ? -1
                                                        : it->second.index;
}
