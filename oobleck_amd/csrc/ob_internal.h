// Internal shared declarations between ob_kernels.hip and ob_layer.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/oobleck_stage.h"

// thread-local last-error buffer (single driving thread per GPU by contract,
// but thread-local keeps the reconfig listener thread safe too).
int ob_fail(const char* fmt, ...);

#define OB_HIP(x)                                                     \
  do {                                                                \
    hipError_t e_ = (x);                                              \
    if (e_ != hipSuccess)                                             \
      return ob_fail("%s:%d: %s", __FILE__, __LINE__,                 \
                     hipGetErrorString(e_));                          \
  } while (0)

#define OB_LAUNCH_CHECK()                                             \
  do {                                                                \
    hipError_t e_ = hipGetLastError();                                \
    if (e_ != hipSuccess)                                             \
      return ob_fail("%s:%d: launch: %s", __FILE__, __LINE__,         \
                     hipGetErrorString(e_));                          \
  } while (0)

// Environment switches.  Call sites keep the result in a function-local
// static const, so each switch is read once per process.  A default-off
// flag is set by '1', a default-on flag is cleared by '0'.
inline bool ob_env_flag(const char* name, bool dflt) {
  const char* e = getenv(name);
  return (e && e[0] == (dflt ? '0' : '1')) ? !dflt : dflt;
}
inline int ob_env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// ---------------------------------------------------------------------------
// In-step profiler (state in ob_layer.hip).  When enabled (ob_profile_enable,
// public ABI), every wrapped launch region is bracketed by HIP events ON THE
// STREAM IT LAUNCHES ON and accumulated per family, so bench.py can report
// the production dispatch's in-step per-launch times (roofline) and a
// per-family step-time split.  Off by default: zero overhead in the timed
// region (one branch per call).
enum {
  OB_PF_FC_FWD = 0,     // the roofline kernel: MLP fc forward GEMM
  OB_PF_GEMM_FWD = 1,   // other forward GEMMs (qkv/attnproj/mlpproj/lm_head)
  OB_PF_GEMM_DX = 2,    // backward activation-grad GEMMs
  OB_PF_GEMM_DW = 3,    // weight-grad GEMMs (side stream)
  OB_PF_FLASH_FWD = 4,  // flash fwd + its V^T staging
  OB_PF_FLASH_BWD = 5,  // flash bwd (transposes + dsum + dkdv/dq)
  OB_PF_ATTN_MAT = 6,   // non-flash attention matmuls + softmax
  OB_PF_LN = 7,
  OB_PF_CE = 8,
  OB_PF_ELEM = 9,       // gelu / colsum / embed / misc elementwise
  OB_PF_ADAMW = 10,
  OB_PF_NFAM = 11
};
bool ob_prof_on();
int ob_prof_beg(int fam, hipStream_t s);
void ob_prof_end(int fam, int slot, hipStream_t s);

#define OB_PROF(fid, strm, call)                                        \
  ({                                                                    \
    int _r;                                                             \
    if (ob_prof_on()) {                                                 \
      hipStream_t _ps = reinterpret_cast<hipStream_t>(strm);            \
      const int _fi = (fid);                                            \
      const int _slot = ob_prof_beg(_fi, _ps);                          \
      _r = (call);                                                      \
      ob_prof_end(_fi, _slot, _ps);                                     \
    } else {                                                            \
      _r = (call);                                                      \
    }                                                                   \
    _r;                                                                 \
  })

// One element of the fused AdamW update, shared by k_adamw (ob_kernels.hip)
// and k_adamw_scaled (ob_optim.hip) so the two cannot drift apart: gi is the
// gradient the update consumes (raw, or raw * clip coefficient).
__device__ __forceinline__ void ob_adamw_update(
    float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
    int64_t i, float gi, float wd_factor, float step_size, float inv_sqrt_bc2,
    float beta1, float beta2, float eps) {
  float mi = beta1 * m[i] + (1.f - beta1) * gi;
  float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
  m[i] = mi;
  v[i] = vi;
  const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
  p[i] = p[i] * wd_factor - step_size * mi / denom;
}

// internal launchers used by the layer orchestration (same semantics as the
// public ob_* wrappers but C++ linkage, no error wrapping duplication).
int ob_embed_fwd_f32(const int64_t* ids, const float* wte, const float* wpe,
                     float* out, int64_t B, int64_t S, int64_t H, void* stream);
int ob_embed_bwd_f32(const int64_t* ids, const float* dout, float* dwte,
                     float* dwpe, int64_t B, int64_t S, int64_t H, void* stream);
int ob_ce_fwd_f32(const float* logits, const int64_t* labels, float* lse,
                  float* loss, int64_t B, int64_t S, int64_t V, void* stream);
int ob_ce_bwd_f32(float* logits_to_dlogits, const int64_t* labels,
                  const float* lse, const float* dloss_or_null, int64_t B,
                  int64_t S, int64_t V, void* stream);

// dropout launchers (ob_dropout.hip), keyed by the site's ob_drop_key
// (ob_philox.h); bf16 != 0 selects the bf16 kernels.  y may alias x / t.
struct ob_drop_key;
int ob_drop_scale(const ob_drop_key& key, int bf16, const void* x, void* y,
                  int64_t n, void* stream);
int ob_drop_add(const ob_drop_key& key, int bf16, const void* t,
                const void* res, void* y, int64_t n, void* stream);
// ws non-null (bf16 only): the column sums go through that slab of
// ob_drop_cs_ws_count floats (deterministic mode)
int ob_drop_scale_colsum(const ob_drop_key& key, int bf16, const void* dy,
                         void* dm, void* db, int64_t M, int64_t N,
                         void* stream, float* ws = nullptr);
int ob_embed_fwd_drop(const ob_drop_key& key, int bf16, const int64_t* ids,
                      const float* wte, const float* wpe, void* out, int64_t B,
                      int64_t Sq, int64_t H, void* stream);
int ob_embed_bwd_drop(const ob_drop_key& key, int bf16, const int64_t* ids,
                      const void* dout, float* dwte, float* dwpe, int64_t B,
                      int64_t Sq, int64_t H, void* stream);
// deterministic mode (bf16 only): the colsum through a slab of
// ob_drop_cs_ws_count floats; the owner-computes embedding backward (key
// null: no dropout)
int64_t ob_drop_cs_ws_count(int64_t M, int64_t N);
int ob_embed_bwd_det(const ob_drop_key* key, const int64_t* ids,
                     const void* dout, float* dwte, float* dwpe, int64_t B,
                     int64_t Sq, int64_t H, void* stream);

// bf16-path launchers (defined in ob_kernels_bf16.hip; the flash family
// and ob_transpose_bf16_b in ob_flash_bf16.hip; the GEMMs, below, in
// ob_gemm_bf16.hip)
extern "C" {
int ob_f32_to_bf16_t_ld(const void* x, void* y, int64_t rows, int64_t cols,
                        int64_t out_ld, void* stream);
int ob_layernorm_fwd_bf16(const void* x, const void* w, const void* b,
                          void* y, void* mean, void* rstd, int64_t rows,
                          int64_t H, float eps, void* stream);
int ob_layernorm_bwd_bf16(const void* x, const void* w, const void* mean,
                          const void* rstd, const void* dy, void* dx,
                          void* dw, void* db, int64_t rows, int64_t H,
                          int dx_accum, void* stream);
// fused tail: ln fwd that also writes the stash copy of x (xcopy null = none)
int ob_layernorm_fwd_copy_bf16(const void* x, const void* w, const void* b,
                               void* y, void* xcopy, void* mean, void* rstd,
                               int64_t rows, int64_t H, float eps,
                               void* stream);
// ln bwd with dx = bf16(res + v) (res null = none, may equal dx) and the
// optional side sums sum_res += colsum(res), sum_dx += colsum(dx)
int ob_layernorm_bwd_res_bf16(const void* x, const void* w, const void* mean,
                              const void* rstd, const void* dy,
                              const void* res, void* dx, void* dw, void* db,
                              void* sum_res, void* sum_dx, int64_t rows,
                              int64_t H, void* stream);
// gelu bwd over [M,N] that also accumulates db[N] += colsum(du)
int ob_gelu_bwd_colsum_bf16(const void* u, const void* dg, void* du,
                            void* db, int64_t M, int64_t N, void* stream);
int ob_softmax_causal_fwd_bf16(void* scores, int64_t batch, int64_t Sq,
                               float scale, void* stream);
int ob_softmax_causal_bwd_bf16(const void* P, void* dP, int64_t batch,
                               int64_t Sq, void* stream);
int ob_gelu_fwd_bf16(const void* u, void* g, int64_t n, void* stream);
int ob_gelu_bwd_bf16(const void* u, const void* dg, void* du, int64_t n,
                     void* stream);
int ob_colsum_bf16(const void* X, void* db, int64_t M, int64_t N,
                   void* stream);
int ob_embed_fwd_bf16(const void* ids, const void* wte, const void* wpe,
                      void* out, int64_t B, int64_t Sq, int64_t H,
                      void* stream);
int ob_embed_bwd_bf16(const void* ids, const void* dout, void* dwte,
                      void* dwpe, int64_t B, int64_t Sq, int64_t H,
                      void* stream);
int ob_ce_fwd_bf16(const void* logits, const void* labels, void* lse,
                   void* loss, int64_t B, int64_t Sq, int64_t V, int64_t ld,
                   void* stream);
int ob_ce_bwd_bf16(void* logits, const void* labels, const void* lse,
                   const void* dloss, int64_t B, int64_t Sq, int64_t V,
                   int64_t ld, void* stream);
int ob_transpose_bf16(const void* in, void* out, int64_t R, int64_t C,
                      void* stream);
int ob_flash_fwd_bf16(const void* qkv, const void* VT, void* O, void* lse,
                      int64_t B, int64_t Sq, int64_t H, int64_t nh,
                      float scale, void* stream);
int ob_transpose_bf16_b(const void* in, void* out, int64_t R, int64_t C,
                        int64_t sIn1, int64_t sIn2, int64_t ldin, int64_t n1,
                        int64_t n2, void* stream);
int ob_flash_dsum_bf16(const void* O, const void* dO, void* D, int64_t B,
                       int64_t Sq, int64_t H, int64_t nh, void* stream);
int ob_flash_bwd_bf16(const void* qkv, const void* QT, const void* KT,
                      const void* dOT, const void* dO, const void* lse,
                      const void* D, void* dqkv, int64_t B, int64_t Sq,
                      int64_t H, int64_t nh, float scale, void* stream);
int ob_flash_fwd_nt_bf16(const void* qkv, void* O, void* lse, int64_t B,
                         int64_t Sq, int64_t H, int64_t nh, float scale,
                         void* stream);
int ob_flash_bwd_nt_bf16(const void* qkv, const void* dO, const void* lse,
                         const void* D, void* dqkv, void* dbias_qkv,
                         int64_t B, int64_t Sq, int64_t H, int64_t nh,
                         float scale, void* stream);
int ob_flash_bwd_nt_d_bf16(const void* qkv, const void* O, const void* dO,
                           const void* lse, void* D_ws, void* dqkv,
                           void* dbias_qkv, int64_t B, int64_t Sq, int64_t H,
                           int64_t nh, float scale, void* stream);
}
// The reductions' common form (ob_kernels_bf16.hip): ws null runs the
// atomic kernels, as the entries above do; ws non-null (deterministic mode)
// runs the DET kernels through that slab of ob_det_ws_count floats, as the
// public _det entries do.  The layer passes its mode's slab or null.
int ob_layernorm_bwd_ws(const void* x, const void* w, const void* mean,
                        const void* rstd, const void* dy, void* dx, void* dw,
                        void* db, int64_t rows, int64_t H, int dx_accum,
                        float* ws, void* stream);
int ob_layernorm_bwd_res_ws(const void* x, const void* w, const void* mean,
                            const void* rstd, const void* dy, const void* res,
                            void* dx, void* dw, void* db, void* sum_res,
                            void* sum_dx, int64_t rows, int64_t H, float* ws,
                            void* stream);
int ob_colsum_ws(const void* X, void* db, int64_t M, int64_t N, float* ws,
                 void* stream);
int ob_gelu_bwd_colsum_ws(const void* u, const void* dg, void* du, void* db,
                          int64_t M, int64_t N, float* ws, void* stream);
int ob_ce_fwd_ws(const void* logits, const void* labels, void* lse,
                 void* loss, int64_t B, int64_t Sq, int64_t V, int64_t ld,
                 float* ws, void* stream);
// hipBLASLt path for plain GEMMs (ob_blaslt.hip); returns -1 when the
// heuristic offers no algo (caller falls back to the hand-written path)
extern "C" int ob_gemm_lt(int tA, int tB, int64_t M, int64_t N, int64_t K,
                          float alpha, const void* A, int64_t lda,
                          const void* B, int64_t ldb, float beta, void* C,
                          int64_t ldc, int c_f32, void* stream);
extern "C" int ob_gemm_lt_bias(int tA, int tB, int64_t M, int64_t N,
                               int64_t K, float alpha, const void* A,
                               int64_t lda, const void* B, int64_t ldb,
                               float beta, void* C, int64_t ldc, int c_f32,
                               const void* bias, void* stream);
extern "C" int ob_gemm_lt_bias_res(int tA, int tB, int64_t M, int64_t N,
                                   int64_t K, float alpha, const void* A,
                                   int64_t lda, const void* B, int64_t ldb,
                                   void* C, int64_t ldc, int c_f32,
                                   const void* bias, const void* residual,
                                   void* stream);
extern "C" int ob_gemm_lt_f32(int tA, int tB, int64_t M, int64_t N,
                              int64_t K, float alpha, const void* A,
                              int64_t lda, const void* B, int64_t ldb,
                              float beta, void* C, int64_t ldc,
                              void* stream);
// ---------------------------------------------------------------------------
// One library GEMM problem, row-major semantics: everything hipBLASLt's
// descriptor and layouts are built from, and so the key of both the
// per-stream plan cache and the process-wide choice table (ob_blaslt.hip).
// ob_lt_shape_of is the ONE place a key is filled: lt_matmul calls it with
// the arguments of the call, the layer's shape list (ob_layer_lt_list,
// ob_layer.hip) through the same two constructors the call sites use.
struct ob_lt_shape {
  int tA = 0, tB = 0;
  int64_t M = 0, N = 0, K = 0, lda = 0, ldb = 0, ldc = 0;
  int c_f32 = 0;   // fp32 output (else bf16)
  int beta1 = 0;   // beta != 0
  int bias = 0;    // fp32 [N] BIAS epilogue
  int cin = 0;     // the C-input operand is a buffer other than C
  int ab_f32 = 0;  // fp32 A/B (the reference-dtype leg)
};
#define OB_LT_SHAPE_FIELDS 13  // int64s per shape in ob_layer_lt_shapes
inline ob_lt_shape ob_lt_shape_of(int tA, int tB, int64_t M, int64_t N,
                                  int64_t K, int64_t lda, int64_t ldb,
                                  int64_t ldc, int c_f32, float beta,
                                  bool bias, bool cin, int ab_f32) {
  ob_lt_shape s;
  s.tA = tA != 0, s.tB = tB != 0, s.M = M, s.N = N, s.K = K;
  s.lda = lda, s.ldb = ldb, s.ldc = ldc, s.c_f32 = c_f32 != 0;
  s.beta1 = beta != 0.f, s.bias = bias, s.cin = cin, s.ab_f32 = ab_f32 != 0;
  return s;
}
// the layer's two library GEMM forms.  linear: out[M,N] = in[M,K] W[N,K]^T
// (+ bias) (+ res), bf16; dw: gout[actw,dyw] += act[BS,actw]^T dY[BS,dyw],
// fp32, act rows lda apart.
inline ob_lt_shape ob_lt_linear(int64_t M, int64_t K, int64_t N, bool bias,
                                bool res) {
  return ob_lt_shape_of(0, 1, M, N, K, K, K, N, 0, res ? 1.f : 0.f, bias, res,
                        0);
}
inline ob_lt_shape ob_lt_dw(int64_t actw, int64_t dyw, int64_t BS,
                            int64_t lda) {
  return ob_lt_shape_of(1, 0, actw, dyw, BS, lda, dyw, dyw, 1, 1.f, false,
                        false, 0);
}
// tunes one shape if the choice table has no entry for it (host code, never
// inside a step; a no-op with OB_LT_TUNE=0).  0, or 1 with ob_fail set.
// slab_floats > 0: the caller can run the shape sliced along K with a slab of
// that many floats (ob_dw_slices.h), so the sliced forms are measured too.
int ob_lt_tune_shape(const ob_lt_shape& s, int64_t slab_floats = 0);
// a listed dw shape's call: gout += act^T dY, as the slice count of the
// choice table says (1 without an entry, with OB_DW_SLICES=1, OB_LT_TUNE=0
// and in deterministic mode); slab is scratch of slab_floats floats on the
// caller's stream.  Returns as ob_gemm_lt.
int ob_lt_dw_run(const ob_lt_shape& s, const void* act, const void* dY,
                 float* gout, float* slab, int64_t slab_floats, void* stream);

// ---------------------------------------------------------------------------
// bf16 GEMM call (ob_gemm_bf16.hip): C = alpha * op(A) op(B) (+ bias)
// (+ residual) (+ beta * C) over an n1 x n2 batch.  Leading dims and batch
// strides are in elements.  The defaults are the layer's unbatched NT linear
// (A [M,K], B [N,K], bf16 out).
struct ob_bf16_gemm {
  const void* A = nullptr;
  const void* B = nullptr;
  void* C = nullptr;
  const void* bias = nullptr;      // fp32 [N]
  const void* residual = nullptr;  // bf16, C's layout
  int64_t M = 0, N = 0, K = 0;
  int64_t lda = 0, ldb = 0, ldc = 0;
  int64_t sA1 = 0, sA2 = 0, sB1 = 0, sB2 = 0, sC1 = 0, sC2 = 0;
  int64_t n1 = 1, n2 = 1;
  float alpha = 1.f, beta = 0.f;
  int transA = 0, transB = 1;
  int out_kind = 0;  // BF_OUT_*: 0 bf16, 1 f32, 2 f32 atomicAdd
  int splitk = 1;    // > 1 needs out_kind 2
  int64_t Mr = 0;    // NT dispatchers only: rows >= Mr are not stored
  void* stream = nullptr;
};
// checks, routes (ob_gemm_route.h) and launches; ignores Mr (stores M rows)
int ob_gemm_bf16_run(const ob_bf16_gemm& g);
// the hand-written NT kernels, unconditionally.  glds: M, N % 128, K % 32;
// nt256: M % 256, N % BN, BN in {128, 256}, K % 64; 8ph: M, N % 256,
// K % 64.  All: 16-byte aligned bases and strides.
int ob_gemm_bf16_nt_dispatch(const ob_bf16_gemm& g);
int ob_gemm_bf16_nt256_dispatch(const ob_bf16_gemm& g, int BN);
int ob_gemm_bf16_nt_8ph_dispatch(const ob_bf16_gemm& g);
