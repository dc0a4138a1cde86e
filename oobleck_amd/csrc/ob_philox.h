// ob_philox.h — the dropout mask definition (DESIGN.md "Dropout masks").
//
// A keep bit is a pure function of (seed, layer_id, site, tick, element
// index): no RNG state exists, the backward regenerates what the forward
// drew, and a pipeline rebuilt after a failure needs nothing broadcast.
// This definition is frozen: changing it changes every trained-with-dropout
// trajectory.
//
//   Philox4x32-10 (Salmon et al., SC'11), multipliers 0xD2511F53 /
//   0xCD9E8D57, Weyl key increments 0x9E3779B9 / 0xBB67AE85.
//   For element e of a site's tensor (e < 2^34):
//     counter = (low32(e >> 2), low32(tick), high32(tick),
//                layer_id << 8 | site)
//     key     = (low32(seed), high32(seed))
//     word    = output[e & 3]
//   keep iff word >= thr, thr = floor(p * 2^32) computed on the host in
//   double; kept elements are scaled by 1 / (1 - p) in fp32.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define OB_PHILOX_HD __host__ __device__ __forceinline__
#else
#define OB_PHILOX_HD inline
#endif

// Sites (OB_DROP_* in include/oobleck_stage.h) and the tensor e indexes:
//   0 EMBD        [B,S,H] embedding output
//   1 ATTN        [B,nh,S,S] probabilities, full square
//   2 RESID_ATTN  [B,S,H]
//   3 RESID_MLP   [B,S,H]

// everything a kernel needs to regenerate one site's mask, by value
struct ob_drop_key {
  uint32_t k0, k1;      // seed halves
  uint32_t c1, c2, c3;  // tick halves, layer_id << 8 | site
  uint32_t thr;         // keep iff word >= thr
  float scale;          // 1 / (1 - p)
};

struct ob_philox4 {
  uint32_t w[4];
};

OB_PHILOX_HD void ob_mulhilo32(uint32_t a, uint32_t b, uint32_t* hi,
                               uint32_t* lo) {
  const uint64_t p = (uint64_t)a * (uint64_t)b;
  *hi = (uint32_t)(p >> 32);
  *lo = (uint32_t)p;
}

OB_PHILOX_HD ob_philox4 ob_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2,
                                         uint32_t c3, uint32_t k0,
                                         uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint32_t hi0, lo0, hi1, lo1;
    ob_mulhilo32(0xD2511F53u, c0, &hi0, &lo0);
    ob_mulhilo32(0xCD9E8D57u, c2, &hi1, &lo1);
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  ob_philox4 o;
  o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
  return o;
}

// the four words covering elements 4q .. 4q+3 (q = e >> 2)
OB_PHILOX_HD ob_philox4 ob_drop_words(const ob_drop_key& k, uint32_t q) {
  return ob_philox4x32_10(q, k.c1, k.c2, k.c3, k.k0, k.k1);
}

// keep·scale factor of one element (0 when dropped)
OB_PHILOX_HD float ob_drop_factor(const ob_drop_key& k, uint32_t word) {
  return word >= k.thr ? k.scale : 0.f;
}

static inline int ob_drop_p_ok(float p) { return p >= 0.f && p < 1.f; }

static inline ob_drop_key ob_drop_make_key(uint64_t seed, int32_t layer_id,
                                           int32_t site, uint64_t tick,
                                           float p) {
  ob_drop_key k;
  k.k0 = (uint32_t)seed;
  k.k1 = (uint32_t)(seed >> 32);
  k.c1 = (uint32_t)tick;
  k.c2 = (uint32_t)(tick >> 32);
  k.c3 = ((uint32_t)layer_id << 8) | (uint32_t)site;
  k.thr = (uint32_t)((double)p * 4294967296.0);  // floor, p in [0,1)
  k.scale = 1.0f / (1.0f - p);
  return k;
}
