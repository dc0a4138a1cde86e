// ob_dw_slices.h — which weight-grad GEMMs may be cut along K, and into how
// many slices.  The ONE place the rule is written: the tuner and the sliced
// call of ob_blaslt.hip ask it, and the host query ob_dw_slices_admit
// (tests/test_dw_slices_cpu.py) reports it.  Pure arithmetic: no pointers, no
// environment reads, no GPU.
//
// A sliced call runs the K-slices of a TN weight grad as
// the entries of one strided-batched library matmul, each writing its fp32
// [M, N] product into its own slab, and k_dw_fold then adds the slabs to the
// grads in ascending order.  It pays where the unsliced output has fewer
// 128 x 128 tiles than the device has CUs, so that part of the chip gets no
// workgroup, and K is deep enough to cut.
#pragma once
#include <cstdint>

#define OB_DW_SLICE_TILE 128        // the library's best tile on these shapes
#define OB_DW_SLICE_K_ALIGN 256     // a slice is whole MT..x256 K-steps
#define OB_DW_SLICE_K_MIN 1024      // shorter slices: the fold outweighs them
#define OB_DW_SLICES_MAX 16
// The most slices the tuner picks by itself (OB_DW_SLICES unset).  Its solo
// timing favours 4 slices for three of GPT-2 small's four shapes, but in the
// step 4 slices lost to the parent and 2 won: every
// slice adds a slab the fold reads back beside the main streams' kernels,
// which a solo measurement does not see.  OB_DW_SLICES=n still forces n.
#define OB_DW_SLICES_AUTO_MAX 2

// the shape as ob_lt_shape names it (ob_internal.h); plain: no bias
// epilogue, no separate C-input, bf16 operands
struct ob_dw_slice_shape {
  int tA, tB, c_f32, beta1;
  bool plain;
  int64_t M, N, K, ldc;
};

// may this shape run as s slices on a device of cus CUs, given a slab of
// slab_floats floats?
inline bool ob_dw_slices_ok(const ob_dw_slice_shape& k, int s, int cus,
                            int64_t slab_floats) {
  if (!(k.tA == 1 && k.tB == 0 && k.c_f32 && k.beta1 && k.plain)) return false;
  if (k.M <= 0 || k.N <= 0 || k.K <= 0 || k.ldc != k.N) return false;
  if (s != 2 && s != 4 && s != 8 && s != OB_DW_SLICES_MAX) return false;
  const int64_t tiles = ((k.M + OB_DW_SLICE_TILE - 1) / OB_DW_SLICE_TILE) *
                        ((k.N + OB_DW_SLICE_TILE - 1) / OB_DW_SLICE_TILE);
  if (tiles >= cus) return false;
  if (k.K % s) return false;
  const int64_t ks = k.K / s;
  if (ks % OB_DW_SLICE_K_ALIGN || ks < OB_DW_SLICE_K_MIN) return false;
  return (int64_t)s * k.M * k.N <= slab_floats;
}

// the admissible slice counts in ascending order; returns their number
inline int ob_dw_slices_list(const ob_dw_slice_shape& k, int cus,
                             int64_t slab_floats, int out[4]) {
  int n = 0;
  for (int s = 2; s <= OB_DW_SLICES_MAX; s *= 2)
    if (ob_dw_slices_ok(k, s, cus, slab_floats)) out[n++] = s;
  return n;
}
