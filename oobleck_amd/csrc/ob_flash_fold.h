// ob_flash_fold.h — which rows a flash block owns, and which linear block
// id is which (head, block).  The ONE place this mapping lives: the three
// production flash kernels, their launchers and the host query entries
// (ob_flash_fold_rows / _grid / _id, tests/test_flash_fold_map.py) all call
// these functions.  DESIGN.md §8 item 14.
//
// Fold: causal work grows linearly with the row index, so a block owns one
// light piece and its mirror-image heavy piece and every block of a launch
// costs the same, whatever XCD or CU it lands on.
//   forward / dq (units = 4 waves of 32 q rows, tiles = 64-row kv tiles):
//     block a in [0, S/128): waves 0,1 take the 64-row half a, waves 2,3 the
//     half n64-1-a (n64 = S/64).  A wave computes kv tiles 0..its diagonal;
//     the block loops (stages K/V, barriers) to the heavy half's diagonal.
//   dkdv (units = 2 wave pairs of 32 kv rows, tiles = 32-row q tiles):
//     block x in [0, S/64): pair 0 takes kv tile x, pair 1 kv tile n32-1-x
//     (n32 = S/32).  A pair computes q tiles from its diagonal to the end;
//     the block loops from pair 0's diagonal.
// Id map: the hardware deals linear block ids round-robin over the 8 XCDs,
// so id % 8 picks the XCD; the blocks of one head share K/V (or Q/dO) and
// are given ids of one residue class, i.e. one L2.  Placement is a speed
// matter only — nothing depends on it for correctness.
#pragma once
#include <hip/hip_runtime.h>

#define OB_FOLD_HD __host__ __device__ __forceinline__

enum { OB_FOLD_FWD = 0, OB_FOLD_DQ = 1, OB_FOLD_DKDV = 2 };
constexpr int OB_FOLD_XCDS = 8;

// ---- forward / dq ---------------------------------------------------------
OB_FOLD_HD int ob_fold_q_nblk(int S) { return S / 128; }
// first q row of wave w (0..3) of block a
OB_FOLD_HD int ob_fold_q_row0(int S, int a, int w) {
  const int n64 = S / 64;
  return w < 2 ? 64 * a + 32 * w : 64 * (n64 - 1 - a) + 32 * (w - 2);
}
// kv tiles a wave with first row q0 computes: 0 .. its diagonal
OB_FOLD_HD int ob_fold_q_wave_tiles(int q0) { return (q0 + 31) / 64 + 1; }
// kv tiles block a stages: 0 .. the heavy half's diagonal
OB_FOLD_HD int ob_fold_q_block_tiles(int S, int a) { return S / 64 - a; }

// ---- dkdv -----------------------------------------------------------------
OB_FOLD_HD int ob_fold_kv_nblk(int S) { return S / 64; }
// first kv row of wave pair p (0..1) of block x
OB_FOLD_HD int ob_fold_kv_row0(int S, int x, int p) {
  const int n32 = S / 32;
  return 32 * (p ? n32 - 1 - x : x);
}
// first q tile a pair with first row kv0 computes (its diagonal); it runs
// to tile S/32 - 1
OB_FOLD_HD int ob_fold_kv_pair_first(int kv0) { return kv0 / 32; }
// first q tile block x stages: pair 0's diagonal
OB_FOLD_HD int ob_fold_kv_block_first(int x) { return x; }

// ---- linear block id <-> (head z, block) ----------------------------------
OB_FOLD_HD unsigned ob_fold_grid(int nblk, int Z) {
  return (unsigned)(OB_FOLD_XCDS * ((Z + OB_FOLD_XCDS - 1) / OB_FOLD_XCDS) *
                    nblk);
}
// false for the padding ids of a head count that is no multiple of 8
OB_FOLD_HD bool ob_fold_id(unsigned id, int nblk, int Z, int* blk, int* z) {
  const int g = (int)(id % OB_FOLD_XCDS), j = (int)(id / OB_FOLD_XCDS);
  *blk = j % nblk;
  *z = OB_FOLD_XCDS * (j / nblk) + g;
  return *z < Z;
}
