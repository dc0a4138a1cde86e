// ob_flash_seg_bf16.hip — document-masked (block-diagonal) causal flash
// attention for packed sequences, bf16, head_dim 64 and 128 (DESIGN.md §8 item
// 26).  A row of Sq tokens holds several documents; query row i of batch row b
// attends the keys j with lo[b,i] <= j <= i, where lo[b,i] is the first token
// of i's document.  Three kernels per head size, as in the banded set
// (ob_flash_win_bf16.hip): forward (O and the row LSE), dQ (forming D =
// rowsum(dO * O) into D_ws) and dK/dV; one body per kernel, a template on the
// head size.  A fourth, small kernel (k_seg_bounds) turns "starts a document"
// flags into the two bound arrays the others read:
//   lo int32 [B, Sq]: lo[b,i] = first token of i's document   (forward, dQ)
//   hi int32 [B, Sq]: hi[b,j] = last token of j's document    (dK/dV)
// Both are non-decreasing along a row, lo[i] <= i <= hi[i], and constant
// within a document.  Two arrays, not one array of document ids: a q row's
// first key and a kv row's last query are then ONE load each, and a wave's
// tile range is a shift of the value its first or last lane already holds.
//
// The arithmetic is the banded kernels': swapped QK^T so a lane owns one q
// column, bf_dance into the PV / dS A fragment, transposed B operands read
// column-wise from the row-major LDS tile, double-buffered tiles under one
// barrier per tile, `scale` folded in the same places, and that file's rules
// for rows whose running max is still -inf (a wave starts at the first tile
// its FIRST row reaches, so a later row whose document starts further right is
// fully masked in the wave's first tiles).  A band is the special case lo = i
// - W + 1.  What is this file's own is where the ranges come from: device
// memory, per microbatch.
//
// Block map (consecutive rows, as in the banded file; only the linear-id ->
// (head, block) map ob_fold_id / ob_fold_grid is shared with the dense
// kernels):
//   forward / dQ: block a owns q rows 128a .. 128a+127, wave w the 32 rows
//     from q0 = 128a + 32w.  It stages the 64-row kv tiles lo[128a]/64 ..
//     2a+1; wave w computes lo[q0]/64 .. (q0+31)/64 of them.
//   dK/dV: block x owns kv rows 64x .. 64x+63, wave pair p the 32 rows from
//     kv0 = 64x + 32p.  It stages the 32-row q tiles 2x .. hi[64x+63]/32;
//     pair p computes kv0/32 .. hi[kv0+31]/32.
// A block whose documents end early simply loops less: work falls from Sq^2
// to the sum of the squared document lengths, rounded up to tiles.
//
// Tile classes, per wave.  forward: a tile with kv0 + 63 <= q0 and kv0 >=
// lo[q0+31] is inside the document of all 32 rows and takes no mask; any other
// takes `(unsigned)(kv - lo) <= (unsigned)(q - lo)`, the document test (kv >=
// lo) and the causal test (kv <= q) in one compare.  dK/dV: a q tile with q0
// >= kv0 + 31 and q0 + 31 <= hi[kv0] takes no mask; any other takes
// `(unsigned)(q - kv) <= (unsigned)(hi - kv)`.
//
// Bounds.  Each lane loads its own row's bound once, before the loop, with an
// ordinary vector load; the wave-uniform values (first and last lane's, and the
// block's first or last row's) are moved to scalar registers with v_readlane
// (a lane broadcast, no scalar memory access), so the loop control stays
// scalar.  Every
// loaded bound is clamped to the range its definition gives it (lo to [0, i],
// hi to [j, Sq-1]): a tile index derived from it is then inside the buffers
// whatever the arrays hold, and k_seg_bounds produces valid arrays from any
// input, so no data can send a kernel out of bounds.
//
// Compiled without packed fp32 VALU ops, forceinline bodies under attributed
// __global__ wrappers, as the banded kernels.  Resources:
// profiles/flash_seg_resources.txt (no scratch; the banded kernels' LDS).
//
// Out of scope: dropout, a band, bidirectional or grouped-query attention on
// such a layer, head_dim 80/96, the materialized-P and fp32 routes, padding.
#include "ob_flash_common.h"
#include "ob_internal.h"
#include "ob_flash_fold.h"

#include <cmath>

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

#define OB_SEG_KERNEL __attribute__((target("no-packed-fp32-ops")))

// a loaded bound, forced into the range its definition gives it
__device__ __forceinline__ int seg_lo(const int* lop, int row) {
  return min(max(lop[row], 0), row);
}
__device__ __forceinline__ int seg_hi(const int* hip, int row, int Sq) {
  return max(min(hip[row], Sq - 1), row);
}
// lane `lane`'s value as a wave-uniform (scalar) value
__device__ __forceinline__ int seg_uni(int v, int lane) {
  return __builtin_amdgcn_readlane(v, lane);
}

// ---- LDS image per head size (the banded file's) ---------------------------
template <int HD> struct seg_lds;
template <> struct seg_lds<64> {
  static __device__ __forceinline__ int off(int row, int ch) {
    return nt_off(row, ch);
  }
  static __device__ __forceinline__ bf16x8 frag(const __bf16* t, int lane,
                                                int r0, int d) {
    return nt_tr_frag(t, lane, r0, d);
  }
};
template <> struct seg_lds<128> {
  static __device__ __forceinline__ int off(int row, int ch) {
    return hd_off(row, ch);
  }
  static __device__ __forceinline__ bf16x8 frag(const __bf16* t, int lane,
                                                int r0, int d) {
    return hd_tr_frag(t, lane, r0, d);
  }
};

// Stages two [ROWS][HD] tiles (rows lda / ldb elements apart in memory) into
// their LDS images: 256 threads, 16-byte chunks, thread = chunk tid % (HD/8)
// of rows tid / (HD/8) + RP*i.  All the loads are issued before the first
// store.
template <int HD, int ROWS>
__device__ __forceinline__ void seg_stage2(__bf16* da, const __bf16* a,
                                           int64_t lda, __bf16* db,
                                           const __bf16* b, int64_t ldb,
                                           int tid) {
  constexpr int CH = HD / 8, RP = 256 / CH, N = ROWS / RP;
  const int sr = tid / CH, sc = tid % CH;
  const int so = seg_lds<HD>::off(sr, sc);
  bf16x8 ra[N], rb[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    ra[i] = *reinterpret_cast<const bf16x8*>(a + (sr + RP * i) * lda + sc * 8);
    rb[i] = *reinterpret_cast<const bf16x8*>(b + (sr + RP * i) * ldb + sc * 8);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    *reinterpret_cast<bf16x8*>(da + so + RP * HD * i) = ra[i];
    *reinterpret_cast<bf16x8*>(db + so + RP * HD * i) = rb[i];
  }
}

// ===========================================================================
// Bounds from flags.  One block per batch row; thread t owns the contiguous
// chunk [t*C, (t+1)*C) of the row.  Pass 1: the last and the first start of
// the chunk go to LDS.  Pass 2: a forward sweep from the last start before the
// chunk writes lo, a backward sweep from the first start after it writes hi.
// Position 0 is a start whatever it holds; ds null = no other start.  Any
// input gives 0 <= lo[i] <= i <= hi[i] < Sq.
// ===========================================================================
__global__ __launch_bounds__(256) void k_seg_bounds(
    const int* __restrict__ ds, int* __restrict__ lo, int* __restrict__ hi,
    int Sq) {
  __shared__ int last_s[256], first_s[256];
  const int t = threadIdx.x;
  const int C = (Sq + 255) / 256;
  const int i0 = min(t * C, Sq), i1 = min(i0 + C, Sq);
  const int64_t row = (int64_t)blockIdx.x * Sq;
  const int* dsp = ds ? ds + row : nullptr;
  int last = -1, first = Sq;
  for (int i = i0; i < i1; ++i)
    if (i == 0 || (dsp && dsp[i] != 0)) {
      last = i;
      first = min(first, i);
    }
  last_s[t] = last, first_s[t] = first;
  __syncthreads();
  int cur = 0, nxt = Sq;
  for (int u = 0; u < t; ++u) cur = max(cur, last_s[u]);
  for (int u = t + 1; u < 256; ++u) nxt = min(nxt, first_s[u]);
  for (int i = i0; i < i1; ++i) {
    if (i == 0 || (dsp && dsp[i] != 0)) cur = i;
    lo[row + i] = cur;
  }
  for (int i = i1 - 1; i >= i0; --i) {
    hi[row + i] = nxt - 1;
    if (i == 0 || (dsp && dsp[i] != 0)) nxt = i;
  }
}

// ===========================================================================
// Forward.  LDS: 2 x (K + V tile) + bcast = 32.5 KB (hd 64), 64.5 KB (hd 128).
// ===========================================================================
template <int HD>
__device__ __forceinline__ void seg_fwd_body(
    const __bf16* __restrict__ qkv, const int* __restrict__ lo,
    __bf16* __restrict__ Obase, float* __restrict__ lse, int Sq, int H, int nh,
    int Z, float scale) {
  constexpr int NS = HD / 16, ND = HD / 32;
  using L = seg_lds<HD>;
  __shared__ __attribute__((aligned(16))) __bf16 kbuf[2][64 * HD];
  __shared__ __attribute__((aligned(16))) __bf16 vbuf[2][64 * HD];
  __shared__ float bcast[128];
  int blk, z;
  if (!ob_fold_id(blockIdx.x, Sq / 128, Z, &blk, &z))
    return;  // block-uniform: grid padding
  const int b = z / nh, h = z % nh;
  const int64_t ld = 3 * (int64_t)H;
  const __bf16* Qp = qkv + (int64_t)b * Sq * ld + h * HD;
  const __bf16* Kp = Qp + H;
  const __bf16* Vp = Qp + 2 * H;
  __bf16* Op = Obase + (int64_t)b * Sq * H + h * HD;
  float* lsep = lse + (int64_t)z * Sq;
  const int* lop = lo + (int64_t)b * Sq;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int il = lane & 31, kh = lane >> 5;
  const int q0 = 128 * blk + 32 * w;
  const int myq = q0 + il;
  // this row's first key; span = the keys it attends, minus one
  const int mylo = seg_lo(lop, myq);
  const unsigned span = (unsigned)(myq - mylo);
  const int lo_last = seg_uni(mylo, 31);  // of the wave's last row
  // block-uniform staged range, wave-uniform computed range
  const int t_lo = seg_uni(seg_lo(lop, 128 * blk), 0) >> 6, t_hi = 2 * blk + 1;
  const int w_lo = seg_uni(mylo, 0) >> 6, w_hi = (q0 + 31) >> 6;

  bf16x8 qf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s)
    qf[s] = *reinterpret_cast<const bf16x8*>(Qp + myq * ld + s * 16 + kh * 8);

  seg_stage2<HD, 64>(kbuf[0], Kp + t_lo * 64 * ld, ld, vbuf[0],
                     Vp + t_lo * 64 * ld, ld, tid);
  __syncthreads();

  f32x16 o[ND] = {};
  float m = -INFINITY, l = 0.f;
  for (int kvt = t_lo; kvt <= t_hi; ++kvt) {
    const int kv0 = kvt * 64;
    const int buf = (kvt - t_lo) & 1;
    if (kvt < t_hi)
      seg_stage2<HD, 64>(kbuf[buf ^ 1], Kp + (kv0 + 64) * ld, ld,
                         vbuf[buf ^ 1], Vp + (kv0 + 64) * ld, ld, tid);
    if (kvt >= w_lo && kvt <= w_hi) {  // wave-uniform
      const __bf16* kb = kbuf[buf];
      const __bf16* vb = vbuf[buf];
      f32x16 sacc0 = {}, sacc1 = {};
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int ch = s * 2 + kh;
        const bf16x8 ka =
            *reinterpret_cast<const bf16x8*>(&kb[L::off(il, ch)]);
        const bf16x8 kb2 =
            *reinterpret_cast<const bf16x8*>(&kb[L::off(32 + il, ch)]);
        sacc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qf[s], sacc0, 0,
                                                        0, 0);
        sacc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kb2, qf[s], sacc1,
                                                        0, 0, 0);
      }
      float sv[32];
      // interior: every kv of the tile <= every q of the wave, and the tile
      // starts inside the document of the wave's last row (so of every row)
      if (kv0 + 63 <= q0 && kv0 >= lo_last) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          sv[r] = sacc0[r] * scale;
          sv[16 + r] = sacc1[r] * scale;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          // lo <= kv <= q in one compare (kv < lo wraps above span)
          const unsigned off = (unsigned)(kv0 + acc_row(r, kh) - mylo);
          sv[r] = off <= span ? sacc0[r] * scale : -INFINITY;
          sv[16 + r] = off + 32u <= span ? sacc1[r] * scale : -INFINITY;
        }
      }
      float mx[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        mx[j] = fmaxf(fmaxf(sv[j], sv[8 + j]),
                      fmaxf(sv[16 + j], sv[24 + j]));
      float mt = fmaxf(fmaxf(fmaxf(mx[0], mx[1]), fmaxf(mx[2], mx[3])),
                       fmaxf(fmaxf(mx[4], mx[5]), fmaxf(mx[6], mx[7])));
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
      // m may be -inf here (a row fully masked so far): the banded file's
      // rules
      if (__any(mt > m + 8.f)) {
        const float mnew = fmaxf(m, mt);
        const float af = (mnew == m) ? 1.f : __expf(m - mnew);
        m = mnew;
        if (kh == 0) bcast[w * 32 + il] = af;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float a = bcast[w * 32 + acc_row(r, kh)];
#pragma unroll
          for (int d = 0; d < ND; ++d) o[d][r] *= a;
        }
        l *= af;
      }
      float ps[8] = {};
#pragma unroll
      for (int r = 0; r < 32; ++r) {
        sv[r] = (sv[r] == -INFINITY) ? 0.f : __expf(sv[r] - m);
        ps[r & 7] += sv[r];
      }
      float psum = ((ps[0] + ps[1]) + (ps[2] + ps[3])) +
                   ((ps[4] + ps[5]) + (ps[6] + ps[7]));
      psum += __shfl_xor(psum, 32, 64);
      l += psum;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const bf16x8 pa = bf_dance(sv + t * 8);
        // B[k = kv 16t+8kh..+7][n = d]: columns of the row-major V tile
#pragma unroll
        for (int d = 0; d < ND; ++d) {
          const bf16x8 vf = L::frag(vb, lane, t * 16 + kh * 8, d);
          o[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa, vf, o[d], 0, 0,
                                                         0);
        }
      }
    }
    __syncthreads();
  }

  if (kh == 0) {
    bcast[w * 32 + il] = 1.f / l;
    lsep[myq] = m + __logf(l);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = acc_row(r, kh);
    const float inv = bcast[w * 32 + row];
#pragma unroll
    for (int d = 0; d < ND; ++d)
      Op[(int64_t)(q0 + row) * H + 32 * d + il] = (__bf16)(o[d][r] * inv);
  }
}
template <int HD>
__global__ OB_SEG_KERNEL __launch_bounds__(256, HD == 64 ? 3 : 2) void
k_flash_fwd_seg(const __bf16* __restrict__ qkv, const int* __restrict__ lo,
                __bf16* __restrict__ Obase, float* __restrict__ lse, int Sq,
                int H, int nh, int Z, float scale) {
  seg_fwd_body<HD>(qkv, lo, Obase, lse, Sq, H, nh, Z, scale);
}

// ===========================================================================
// dQ: the forward's blocks, ranges and K/V staging.  The two 32-row kv
// sub-tiles of a tile run one after the other; a sub-tile wholly outside the
// wave's rows' documents or wholly above its diagonal is skipped,
// wave-uniformly.  D is formed from the resident dO fragments and O loaded in
// the same layout, used, and written to Dout for the dK/dV launch that
// follows.
// LDS: 2 x (K + V tile) + red = 33 KB (hd 64), 66 KB (hd 128).
// ===========================================================================
template <int HD>
__device__ __forceinline__ void seg_dq_body(
    const __bf16* __restrict__ qkv, const __bf16* __restrict__ dO,
    const float* __restrict__ lse, const __bf16* __restrict__ O,
    const int* __restrict__ lo, float* __restrict__ Dout,
    __bf16* __restrict__ dqkv, float* __restrict__ dbias, int Sq, int H,
    int nh, int Z, float scale) {
  constexpr int NS = HD / 16, ND = HD / 32;
  using L = seg_lds<HD>;
  __shared__ __attribute__((aligned(16))) __bf16 kbuf[2][64 * HD];
  __shared__ __attribute__((aligned(16))) __bf16 vbuf[2][64 * HD];
  __shared__ float red[4 * HD];
  int blk, z;
  if (!ob_fold_id(blockIdx.x, Sq / 128, Z, &blk, &z))
    return;  // block-uniform: grid padding
  const int b = z / nh, h = z % nh;
  const int64_t ld = 3 * (int64_t)H;
  const int64_t base = (int64_t)b * Sq * ld + h * HD;
  const __bf16* Qp = qkv + base;
  const __bf16* Kp = Qp + H;
  const __bf16* Vp = Qp + 2 * H;
  const int64_t obase = (int64_t)b * Sq * H + h * HD;
  const int* lop = lo + (int64_t)b * Sq;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int il = lane & 31, kh = lane >> 5;
  const int q0 = 128 * blk + 32 * w;
  const int myq = q0 + il;
  const int mylo = seg_lo(lop, myq);
  const unsigned span = (unsigned)(myq - mylo);
  // `off < lim` is `off <= span`, except for a row that is a document of its
  // own: its one P is 1 and its dS identically 0, which lim = 0 writes as an
  // exact 0 and not as the rounding residue of dP - D
  const unsigned lim = span + (span != 0u);
  const int lo_first = seg_uni(mylo, 0);  // of the wave's first row
  const int t_lo = seg_uni(seg_lo(lop, 128 * blk), 0) >> 6, t_hi = 2 * blk + 1;
  const float mylse = lse[(int64_t)z * Sq + myq];

  bf16x8 qf[NS], df[NS];
  float part = 0.f;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    qf[s] = *reinterpret_cast<const bf16x8*>(Qp + myq * ld + s * 16 + kh * 8);
    df[s] = *reinterpret_cast<const bf16x8*>(dO + obase + (int64_t)myq * H +
                                             s * 16 + kh * 8);
    const bf16x8 ov = *reinterpret_cast<const bf16x8*>(
        O + obase + (int64_t)myq * H + s * 16 + kh * 8);
    float c = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) c += bf2f(ov[j]) * bf2f(df[s][j]);
    part += c;
  }
  const float myD = part + __shfl_xor(part, 32, 64);
  if (kh == 0) Dout[(int64_t)z * Sq + myq] = myD;

  seg_stage2<HD, 64>(kbuf[0], Kp + t_lo * 64 * ld, ld, vbuf[0],
                     Vp + t_lo * 64 * ld, ld, tid);
  __syncthreads();

  f32x16 dq[ND] = {};
  for (int kvt = t_lo; kvt <= t_hi; ++kvt) {
    const int kv0 = kvt * 64;
    const int buf = (kvt - t_lo) & 1;
    if (kvt < t_hi)
      seg_stage2<HD, 64>(kbuf[buf ^ 1], Kp + (kv0 + 64) * ld, ld,
                         vbuf[buf ^ 1], Vp + (kv0 + 64) * ld, ld, tid);
    const __bf16* kb = kbuf[buf];
    const __bf16* vb = vbuf[buf];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int kvu = kv0 + 32 * u;
      // wave-uniform: the sub-tile starts at or below the wave's last row
      // and ends inside the document of its first row
      if (kvu <= q0 + 31 && kvu + 31 >= lo_first) {
        f32x16 sa = {}, pa = {};
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const int ch = s * 2 + kh;
          const bf16x8 ka = *reinterpret_cast<const bf16x8*>(
              &kb[L::off(32 * u + il, ch)]);
          const bf16x8 va = *reinterpret_cast<const bf16x8*>(
              &vb[L::off(32 * u + il, ch)]);
          sa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qf[s], sa, 0, 0,
                                                       0);
          pa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, df[s], pa, 0, 0,
                                                       0);
        }
        float dsv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const bool ok = (unsigned)(kvu + acc_row(r, kh) - mylo) < lim;
          // dS = P * (dP - D); a masked P is 0 without an exp
          dsv[r] = ok ? __expf(sa[r] * scale - mylse) * (pa[r] - myD) : 0.f;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const bf16x8 da = bf_dance(dsv + t * 8);
          // B[k = kv 32u+16t+8kh..+7][n = d]: columns of the K tile
#pragma unroll
          for (int d = 0; d < ND; ++d) {
            const bf16x8 kt = L::frag(kb, lane, 32 * u + 16 * t + kh * 8, d);
            dq[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da, kt, dq[d], 0,
                                                            0, 0);
          }
        }
      }
    }
    __syncthreads();
  }
  __bf16* dQp = dqkv + base;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int q = q0 + acc_row(r, kh);
#pragma unroll
    for (int d = 0; d < ND; ++d)
      dQp[q * ld + 32 * d + il] = (__bf16)(scale * dq[d][r]);
  }
  if (dbias) {  // kernel-uniform
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      float c = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) c += scale * dq[d][r];
      c += __shfl_xor(c, 32, 64);
      if (kh == 0) red[w * HD + 32 * d + il] = c;
    }
    __syncthreads();
    if (tid < HD)
      atomicAdd(dbias + h * HD + tid,
                (red[tid] + red[HD + tid]) +
                    (red[2 * HD + tid] + red[3 * HD + tid]));
  }
}
template <int HD>
__global__ OB_SEG_KERNEL __launch_bounds__(256, HD == 64 ? 3 : 2) void
k_flash_bwd_dq_seg(const __bf16* __restrict__ qkv,
                   const __bf16* __restrict__ dO,
                   const float* __restrict__ lse, const __bf16* __restrict__ O,
                   const int* __restrict__ lo, float* __restrict__ Dout,
                   __bf16* __restrict__ dqkv, float* __restrict__ dbias, int Sq,
                   int H, int nh, int Z, float scale) {
  seg_dq_body<HD>(qkv, dO, lse, O, lo, Dout, dqkv, dbias, Sq, H, nh, Z, scale);
}

// ===========================================================================
// dK/dV: the banded kernels' split-duty wave pairs (role 0: K resident,
// S -> P -> dV; role 1: V resident, dP -> dS -> dK; only P crosses the pair,
// through xch) over 32-row q tiles.  A pair idles, staging and meeting the
// barrier only, before its diagonal tile and after the last tile its rows'
// documents reach.  The B fragments are read before the iteration's barrier:
// after it a fast wave already stages tile qt+2 into this buffer.
// LDS: xch 16 KB + 2 x (Q + dO tile) + red = 33 KB (hd 64), 50 KB (hd 128).
// ===========================================================================
template <int HD>
__device__ __forceinline__ void seg_dkdv_body(
    const __bf16* __restrict__ qkv, const __bf16* __restrict__ dO,
    const float* __restrict__ lse, const float* __restrict__ D,
    const int* __restrict__ hi, __bf16* __restrict__ dqkv,
    float* __restrict__ dbias, int Sq, int H, int nh, int Z, float scale) {
  constexpr int NS = HD / 16, ND = HD / 32;
  using L = seg_lds<HD>;
  __shared__ float xch[2][2][32 * 32];  // [buffer][pair][P tile]
  __shared__ __attribute__((aligned(16))) __bf16 qbuf[2][32 * HD];
  __shared__ __attribute__((aligned(16))) __bf16 obuf[2][32 * HD];
  __shared__ float red[4 * HD];
  int blk, z;
  if (!ob_fold_id(blockIdx.x, Sq / 64, Z, &blk, &z))
    return;  // block-uniform: grid padding
  const int b = z / nh, h = z % nh;
  const int64_t ld = 3 * (int64_t)H;
  const int64_t base = (int64_t)b * Sq * ld + h * HD;
  const __bf16* Qp = qkv + base;
  const __bf16* dOp = dO + (int64_t)b * Sq * H + h * HD;
  const float* lsep = lse + (int64_t)z * Sq;
  const float* Dp = D + (int64_t)z * Sq;
  const int* hip = hi + (int64_t)b * Sq;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int pair = w >> 1, role = w & 1;
  const int il = lane & 31, kh = lane >> 5;
  const int kv0 = 64 * blk + 32 * pair;
  const int mykv = kv0 + il;
  // the last query that attends this kv row; span = its queries, minus one
  const int myhi = seg_hi(hip, mykv, Sq);
  const unsigned span = (unsigned)(myhi - mykv);
  const int hi_first = seg_uni(myhi, 0);  // of the pair's first row
  // this kv row is a document of its own (it ends here and the previous one
  // ended just before): its dS column is identically 0, written as an exact 0
  // as in the dQ kernel
  const bool solo = myhi == mykv && (mykv == 0 || hip[mykv - 1] < mykv);
  // block-uniform staged range, pair-uniform computed range
  const int qt_lo = 2 * blk,
            qt_hi = seg_uni(seg_hi(hip, 64 * blk + 63, Sq), 0) >> 5;
  const int p_lo = kv0 >> 5, p_hi = seg_uni(myhi, 31) >> 5;

  const __bf16* KV = Qp + (role ? 2 * H : H);
  bf16x8 of[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s)
    of[s] = *reinterpret_cast<const bf16x8*>(KV + mykv * ld + s * 16 + kh * 8);

  seg_stage2<HD, 32>(qbuf[qt_lo & 1], Qp + qt_lo * 32 * ld, ld,
                     obuf[qt_lo & 1], dOp + (int64_t)qt_lo * 32 * H, H, tid);
  __syncthreads();

  f32x16 acc[ND] = {};  // role 0: dV d groups; role 1: dK d groups
  for (int qt = qt_lo; qt <= qt_hi; ++qt) {
    const int q0 = qt * 32;
    if (qt < qt_hi)
      seg_stage2<HD, 32>(qbuf[(qt + 1) & 1], Qp + (q0 + 32) * ld, ld,
                         obuf[(qt + 1) & 1], dOp + (int64_t)(q0 + 32) * H, H,
                         tid);
    // wave-uniform; each wave meets exactly one barrier per iteration on
    // either side of the branch
    if (qt < p_lo || qt > p_hi) {
      __syncthreads();
      continue;
    }
    // own tile's A image, and the B image: role 0 multiplies P^T by dO,
    // role 1 dS^T by Q
    const __bf16* ab = role ? obuf[qt & 1] : qbuf[qt & 1];
    const __bf16* bb = role ? qbuf[qt & 1] : obuf[qt & 1];
    bf16x8 bf[2][ND];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int d = 0; d < ND; ++d)
        bf[t][d] = L::frag(bb, lane, 16 * t + kh * 8, d);
    // own tile: S (role 0, A = Q rows) or dP (role 1, A = dO rows)
    f32x16 own = {};
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const bf16x8 af =
          *reinterpret_cast<const bf16x8*>(&ab[L::off(il, s * 2 + kh)]);
      own = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, of[s], own, 0, 0, 0);
    }
    float pv[16];
    float* ptile = xch[qt & 1][pair];
    if (role == 0) {
      const float lse_t = lsep[q0 + il];
      // interior: the q tile lies wholly above the diagonal and ends inside
      // the document of the pair's first row (so of every row)
      const bool interior = q0 >= kv0 + 31 && q0 + 31 <= hi_first;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qoff = acc_row(r, kh);
        // kv <= q <= hi in one compare (q < kv wraps above span)
        const bool ok = interior || (unsigned)(q0 + qoff - mykv) <= span;
        const float lse_q = __shfl(lse_t, qoff, 64);
        pv[r] = ok ? __expf(own[r] * scale - lse_q) : 0.f;
        ptile[qoff * 32 + il] = pv[r];
      }
    }
    __syncthreads();
    if (role == 1) {
      const float d_t = Dp[q0 + il];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qoff = acc_row(r, kh);
        const float d_q = __shfl(d_t, qoff, 64);
        // dS = P * (dP - D); masked entries have P == 0 already
        pv[r] = solo ? 0.f : ptile[qoff * 32 + il] * (own[r] - d_q);
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const bf16x8 a = bf_dance(pv + t * 8);
#pragma unroll
      for (int d = 0; d < ND; ++d)
        acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bf[t][d], acc[d],
                                                         0, 0, 0);
    }
  }

  __bf16* outp = dqkv + base + (role ? H : 2 * H);  // dK or dV slice
  const float os = role ? scale : 1.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int kv = kv0 + acc_row(r, kh);
#pragma unroll
    for (int d = 0; d < ND; ++d)
      outp[kv * ld + 32 * d + il] = (__bf16)(os * acc[d][r]);
  }
  if (dbias) {  // kernel-uniform
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      float c = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) c += os * acc[d][r];
      c += __shfl_xor(c, 32, 64);
      if (kh == 0) red[w * HD + 32 * d + il] = c;
    }
    __syncthreads();
    if (tid < 2 * HD) {
      // waves 0/2 hold dV (role 0), waves 1/3 dK (role 1)
      const int rl = tid / HD, c = tid % HD;
      atomicAdd(dbias + (rl ? H : 2 * H) + h * HD + c,
                red[rl * HD + c] + red[(2 + rl) * HD + c]);
    }
  }
}
template <int HD>
__global__ OB_SEG_KERNEL __launch_bounds__(256, HD == 64 ? 3 : 2) void
k_flash_bwd_dkdv_seg(const __bf16* __restrict__ qkv,
                     const __bf16* __restrict__ dO,
                     const float* __restrict__ lse,
                     const float* __restrict__ D, const int* __restrict__ hi,
                     __bf16* __restrict__ dqkv, float* __restrict__ dbias,
                     int Sq, int H, int nh, int Z, float scale) {
  seg_dkdv_body<HD>(qkv, dO, lse, D, hi, dqkv, dbias, Sq, H, nh, Z, scale);
}

// ---- entries ----------------------------------------------------------------
// 64 or 128; 0 with ob_fail set.  The rules of the banded entries.
static int seg_head_dim(const char* who, int64_t B, int64_t Sq, int64_t H,
                        int64_t nh) {
  if (nh <= 0 || H % nh || (H / nh != 64 && H / nh != 128)) {
    ob_fail("%s: n_embd must be a multiple of n_head and head_dim 64 or 128",
            who);
    return 0;
  }
  if (B <= 0 || Sq <= 0 || Sq % 128) {
    ob_fail("%s: S must be a multiple of 128", who);
    return 0;
  }
  return (int)(H / nh);
}

extern "C" int ob_flash_seg_bounds_i32(const void* doc_start, void* lo,
                                       void* hi, int64_t B, int64_t Sq,
                                       void* stream) {
  if (!lo || !hi) return ob_fail("flash_seg_bounds: null lo or hi");
  if (B <= 0 || Sq <= 0 || B > INT32_MAX || Sq > INT32_MAX)
    return ob_fail("flash_seg_bounds: B and Sq must be positive");
  k_seg_bounds<<<(unsigned)B, 256, 0, S(stream)>>>(
      (const int*)doc_start, (int*)lo, (int*)hi, (int)Sq);
  OB_LAUNCH_CHECK();
  return 0;
}

template <int HD>
static int seg_fwd(const void* qkv, const void* lo, void* O, void* lse,
                   int64_t B, int64_t Sq, int64_t H, int64_t nh, float scale,
                   void* stream) {
  const int Z = (int)(B * nh);
  k_flash_fwd_seg<HD><<<ob_fold_grid((int)Sq / 128, Z), 256, 0, S(stream)>>>(
      (const __bf16*)qkv, (const int*)lo, (__bf16*)O, (float*)lse, (int)Sq,
      (int)H, (int)nh, Z, scale);
  OB_LAUNCH_CHECK();
  return 0;
}

extern "C" int ob_flash_fwd_seg_bf16(const void* qkv, const void* lo, void* O,
                                     void* lse, int64_t B, int64_t Sq,
                                     int64_t H, int64_t nh, float scale,
                                     void* stream) {
  const int hd = seg_head_dim("flash_fwd_seg", B, Sq, H, nh);
  if (!hd) return 1;
  if (!lo) return ob_fail("flash_fwd_seg: null lo");
  return hd == 64 ? seg_fwd<64>(qkv, lo, O, lse, B, Sq, H, nh, scale, stream)
                  : seg_fwd<128>(qkv, lo, O, lse, B, Sq, H, nh, scale, stream);
}

// dq first (forms D from O and dO into D_ws), then dkdv, which reads it
template <int HD>
static int seg_bwd(const void* qkv, const void* O, const void* dO,
                   const void* lse, const void* lo, const void* hi, void* D_ws,
                   void* dqkv, void* dbias_qkv, int64_t B, int64_t Sq,
                   int64_t H, int64_t nh, float scale, void* stream) {
  const int Z = (int)(B * nh);
  k_flash_bwd_dq_seg<HD>
      <<<ob_fold_grid((int)Sq / 128, Z), 256, 0, S(stream)>>>(
          (const __bf16*)qkv, (const __bf16*)dO, (const float*)lse,
          (const __bf16*)O, (const int*)lo, (float*)D_ws, (__bf16*)dqkv,
          (float*)dbias_qkv, (int)Sq, (int)H, (int)nh, Z, scale);
  OB_LAUNCH_CHECK();
  k_flash_bwd_dkdv_seg<HD>
      <<<ob_fold_grid((int)Sq / 64, Z), 256, 0, S(stream)>>>(
          (const __bf16*)qkv, (const __bf16*)dO, (const float*)lse,
          (const float*)D_ws, (const int*)hi, (__bf16*)dqkv,
          (float*)dbias_qkv, (int)Sq, (int)H, (int)nh, Z, scale);
  OB_LAUNCH_CHECK();
  return 0;
}

extern "C" int ob_flash_bwd_seg_d_bf16(const void* qkv, const void* O,
                                       const void* dO, const void* lse,
                                       const void* lo, const void* hi,
                                       void* D_ws, void* dqkv,
                                       void* dbias_qkv, int64_t B, int64_t Sq,
                                       int64_t H, int64_t nh, float scale,
                                       void* stream) {
  const int hd = seg_head_dim("flash_bwd_seg_d", B, Sq, H, nh);
  if (!hd) return 1;
  if (!lo || !hi) return ob_fail("flash_bwd_seg_d: null lo or hi");
  return hd == 64 ? seg_bwd<64>(qkv, O, dO, lse, lo, hi, D_ws, dqkv,
                                dbias_qkv, B, Sq, H, nh, scale, stream)
                  : seg_bwd<128>(qkv, O, dO, lse, lo, hi, D_ws, dqkv,
                                 dbias_qkv, B, Sq, H, nh, scale, stream);
}
