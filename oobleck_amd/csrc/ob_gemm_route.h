// ob_gemm_route.h — which kernel a bf16 GEMM call gets.  The ONE place the
// rule is written: ob_gemm_bf16 (ob_gemm_bf16.hip) launches what it returns
// and the host query ob_gemm_bf16_route (tests/test_gemm_route.py) reports
// it.  Pure arithmetic: no pointers, no environment reads, no GPU.
#pragma once
#include <cstdint>
#include <initializer_list>

// generic-kernel tile (k_gemm_bf16); BF_BN narrows to 64 when N <= 64
#define BF_BM 128
#define BF_BN 128
#define BF_BK 32

// out-kind for the epilogue
enum { BF_OUT_BF16 = 0, BF_OUT_F32 = 1, BF_OUT_F32_ATOMIC = 2 };

enum {
  OB_GEMM_GENERIC = 0,  // k_gemm_bf16: any transposes, edges, alignment
  OB_GEMM_GLDS = 1,     // k_gemm_bf16_nt_glds: 128x128 tile
  OB_GEMM_NT256 = 2,    // k_gemm_bf16_nt_256: 256 x BN tile
  OB_GEMM_P8 = 3        // k_gemm_bf16_nt_8ph: 256x256 8-phase
};

// the process's switches; force is the OB_BF16_FORCE string or null
struct ob_gemm_env {
  bool no_lt, no_glds, no256;
  const char* force;
};

struct ob_gemm_route {
  bool try_lt_first;  // offer the call to hipBLASLt; kernel is the fallback
  int kernel;
  int BN;     // N tile: 64/128 generic, 128 glds, 128/256 nt256, 256 8-phase
  bool edge;  // generic kernel's guarded instantiation
  int splitk;
};

// aligned16: A and B bases are 16-byte aligned and their four batch strides
// are multiples of 8 halfs.
inline ob_gemm_route ob_gemm_bf16_pick(int transA, int transB, int64_t M,
                                       int64_t N, int64_t K, int64_t n1,
                                       int64_t n2, int out_kind, int splitk,
                                       float beta, bool aligned16,
                                       const ob_gemm_env& env) {
  ob_gemm_route r;
  r.splitk = splitk < 1 ? 1 : splitk;
  r.BN = (N <= 64) ? 64 : 128;  // narrow tiles for head_dim GEMMs
  r.edge = (M % BF_BM) || (N % r.BN) || (K % BF_BK);
  r.kernel = OB_GEMM_GENERIC;
  r.try_lt_first = false;
  const bool nt = transA == 0 && transB == 1;
  // probe hook (tools/fc_probe.py): OB_BF16_FORCE picks one NT kernel
  // unconditionally ("glds" | "n128" | "n256" | "8ph")
  if (env.force && nt) {
    const char f = env.force[0];
    if (f == 'g' || f == 'n' || f == '8') {
      r.kernel = f == 'g' ? OB_GEMM_GLDS : f == 'n' ? OB_GEMM_NT256 : OB_GEMM_P8;
      r.BN = f == 'g' ? 128 : (f == 'n' && env.force[1] != '2') ? 128 : 256;
      return r;
    }
  }
  // plain GEMMs (no bias/residual/beta, unbatched, bf16 out) go to
  // hipBLASLt — the dX family, the bias-free lm_head family (measured
  // 815-1166 TF vs 436-692 for the hand-written kernels on those
  // shapes, tools/blas_probe.py).  Fused epilogues stay on ours.
  r.try_lt_first = !env.no_lt && beta == 0.f && n1 == 1 && n2 == 1 &&
                   r.splitk == 1 && out_kind == BF_OUT_BF16 &&
                   M * N >= 512 * 512;
  // fast NT path: async glds staging (interior 128-aligned shapes with
  // 16-byte-aligned bases/strides only)
  if (env.no_glds || !nt || r.edge || !aligned16 || K < 2 * BF_BK) return r;
  const int64_t zb = n1 * n2 * r.splitk;
  // 8-phase 256^2 kernel: wins when its grid fills whole scheduling
  // rounds (measured: lmhead 692 vs 618 TF, 4096^3 1058 vs 995; loses
  // on partial rounds — fc 1.5 rounds: 529 vs 554).  tiles >= 192 and
  // round-efficiency >= 0.9 required.
  // NOTE: an auto-splitk search for atomic outputs was tried here
  // (round-filling sk up to 16) and REGRESSED the step 360k->347k
  // tok/s: split-k multiplies the f32 atomic output traffic by sk,
  // which dominates on the (W1, W2, BS) weight-grad shapes.
  if (M % 256 == 0 && N % 256 == 0 && K % 64 == 0) {
    const int64_t tiles = (M / 256) * (N / 256) * zb;
    const double eff = (double)tiles / (((tiles + 255) / 256) * 256);
    if (tiles >= 192 && eff >= 0.9) {
      r.kernel = OB_GEMM_P8;
      r.BN = 256;
      return r;
    }
  }
  if (!env.no256 && M % 256 == 0 && K % 64 == 0 && K >= 1024) {
    // pick BN by scheduling-round efficiency (blocks / ceil-to-256):
    // e.g. fc (M=8192,N=3072): BN=256 -> 384 blocks = 1.5 rounds (75%),
    // BN=128 -> 768 blocks = 3 full rounds (100%)
    int bn2 = 0;
    double best_eff = 0.0;
    for (int cand : {256, 128}) {
      if (N % cand) continue;
      const int64_t blocks = (M / 256) * (N / cand) * zb;
      const double eff = (double)blocks / (((blocks + 255) / 256) * 256);
      if (eff > best_eff + 1e-9) {
        best_eff = eff;
        bn2 = cand;
      }
    }
    if (bn2 && (M / 256) * (N / bn2) * zb >= 192) {
      r.kernel = OB_GEMM_NT256;
      r.BN = bn2;
      return r;
    }
  }
  r.kernel = OB_GEMM_GLDS;
  r.BN = 128;
  return r;
}
