// ob_dropout.hip — dropout kernels for gfx950 over the stateless Philox mask
// of ob_philox.h.  Every kernel regenerates keep bits from the element index
// alone, so the result is independent of grid size, vector width, dtype
// path, pointer alignment and stash slot.
//
//   dropout_scale         y = keep*scale*x                  (y may alias x)
//   dropout_add           y = res + keep*scale*t            (y may alias t)
//   dropout_scale_colsum  dm = keep*scale*dy, db[n] += colsum(dm)
//   embed fwd/bwd         the embedding kernels with the mask folded in
//   dropout_mask          keep bytes, for tests
//
// bf16 is the hot path: 16-byte loads/stores, 8 elements (two Philox calls)
// per thread-iteration.  fp32 is the parity anchor: one Philox call per
// thread-iteration, scalar accesses, products and sums rounded separately
// (no fma contraction) so it is bit-comparable with a host restatement.
#include "ob_internal.h"
#include "ob_philox.h"

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
static __host__ __device__ inline int64_t dmin64(int64_t a, int64_t b) { return a < b ? a : b; }

#define OB_DROP_MAX_N ((int64_t)1 << 34)

__device__ __forceinline__ float dbf2f(__bf16 h) { return (float)h; }
__device__ __forceinline__ unsigned dbf_bits(__bf16 h) {
  return (unsigned)__builtin_bit_cast(unsigned short, h);
}
__device__ __forceinline__ float dbits2f(unsigned u16) {
  return __builtin_bit_cast(float, u16 << 16);
}
__device__ __forceinline__ float dld(const float* p) { return *p; }
__device__ __forceinline__ float dld(const __bf16* p) { return dbf2f(*p); }
__device__ __forceinline__ void dst(float* p, float v) { *p = v; }
__device__ __forceinline__ void dst(__bf16* p, float v) { *p = (__bf16)v; }

// keep*scale*x with the product rounded on its own
__device__ __forceinline__ float drop_mul(const ob_drop_key& k, uint32_t w,
                                          float x) {
  return w >= k.thr ? __fmul_rn(x, k.scale) : 0.f;
}

__device__ __forceinline__ uint4 dpack8(const float* v) {
  uint4 o;
  o.x = dbf_bits((__bf16)v[0]) | (dbf_bits((__bf16)v[1]) << 16);
  o.y = dbf_bits((__bf16)v[2]) | (dbf_bits((__bf16)v[3]) << 16);
  o.z = dbf_bits((__bf16)v[4]) | (dbf_bits((__bf16)v[5]) << 16);
  o.w = dbf_bits((__bf16)v[6]) | (dbf_bits((__bf16)v[7]) << 16);
  return o;
}
__device__ __forceinline__ void dunpack8(const uint4& v, float* o) {
  o[0] = dbits2f(v.x & 0xffffu); o[1] = dbits2f(v.x >> 16);
  o[2] = dbits2f(v.y & 0xffffu); o[3] = dbits2f(v.y >> 16);
  o[4] = dbits2f(v.z & 0xffffu); o[5] = dbits2f(v.z >> 16);
  o[6] = dbits2f(v.w & 0xffffu); o[7] = dbits2f(v.w >> 16);
}

// ---------------------------------------------------------------------------
// keep bytes
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_drop_mask(ob_drop_key key, int64_t n,
                                                   uint8_t* __restrict__ keep) {
  const int64_t nq = (n + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq;
       q += (int64_t)gridDim.x * 256) {
    const ob_philox4 r = ob_drop_words(key, (uint32_t)q);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t e = q * 4 + j;
      if (e < n) keep[e] = r.w[j] >= key.thr ? 1 : 0;
    }
  }
}

// ---------------------------------------------------------------------------
// elementwise: y = (ADD ? res : 0) + keep*scale*x
// ---------------------------------------------------------------------------

// any dtype, any alignment: one Philox call covers 4 consecutive elements
template <typename T, bool ADD>
__global__ __launch_bounds__(256) void k_drop_ew(ob_drop_key key, const T* x,
                                                 const T* __restrict__ res,
                                                 T* y, int64_t n) {
  const int64_t nq = (n + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq;
       q += (int64_t)gridDim.x * 256) {
    const ob_philox4 r = ob_drop_words(key, (uint32_t)q);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t e = q * 4 + j;
      if (e < n) {
        float v = drop_mul(key, r.w[j], dld(x + e));
        if (ADD) v = __fadd_rn(dld(res + e), v);
        dst(y + e, v);
      }
    }
  }
}

// bf16, 16-byte aligned pointers, n8 = n / 8 whole groups
template <bool ADD>
__global__ __launch_bounds__(256) void k_drop_ew_bf16v(
    ob_drop_key key, const __bf16* x, const __bf16* __restrict__ res,
    __bf16* y, int64_t n8) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8;
       i += (int64_t)gridDim.x * 256) {
    const uint4 xin = *reinterpret_cast<const uint4*>(x + i * 8);
    uint4 rin = {0, 0, 0, 0};
    if (ADD) rin = *reinterpret_cast<const uint4*>(res + i * 8);
    const ob_philox4 r0 = ob_drop_words(key, (uint32_t)(i * 2));
    const ob_philox4 r1 = ob_drop_words(key, (uint32_t)(i * 2 + 1));
    float xv[8], rv[8], out[8];
    dunpack8(xin, xv);
    if (ADD) dunpack8(rin, rv);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t w = j < 4 ? r0.w[j] : r1.w[j - 4];
      float v = drop_mul(key, w, xv[j]);
      if (ADD) v = __fadd_rn(rv[j], v);
      out[j] = v;
    }
    *reinterpret_cast<uint4*>(y + i * 8) = dpack8(out);
  }
}

static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <typename T, bool ADD>
static int launch_ew(const ob_drop_key& key, const void* x, const void* res,
                     void* y, int64_t n, void* stream) {
  if (n <= 0) return 0;
  if (n > OB_DROP_MAX_N) return ob_fail("dropout: n > 2^34 unsupported");
  const int64_t nq = (n + 3) >> 2;
  k_drop_ew<T, ADD><<<(int)dmin64((nq + 255) / 256, 8192), 256, 0,
                      S(stream)>>>(key, (const T*)x, (const T*)res, (T*)y, n);
  OB_LAUNCH_CHECK();
  return 0;
}

// tail groups [q0, ceil(n/4)) of a bf16 tensor (at most two groups)
template <bool ADD>
__global__ void k_drop_tail_bf16(ob_drop_key key, const __bf16* x,
                                 const __bf16* __restrict__ res, __bf16* y,
                                 int64_t q0, int64_t n) {
  const int64_t q = q0 + threadIdx.x;
  if (q * 4 >= n) return;
  const ob_philox4 r = ob_drop_words(key, (uint32_t)q);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t e = q * 4 + j;
    if (e < n) {
      float v = drop_mul(key, r.w[j], dbf2f(x[e]));
      if (ADD) v = __fadd_rn(dbf2f(res[e]), v);
      y[e] = (__bf16)v;
    }
  }
}
template <bool ADD>
static int launch_ew_bf16(const ob_drop_key& key, const void* x,
                          const void* res, void* y, int64_t n, void* stream) {
  if (n <= 0) return 0;
  if (n > OB_DROP_MAX_N) return ob_fail("dropout: n > 2^34 unsupported");
  if (!(al16(x) && al16(y) && (!ADD || al16(res))))
    return launch_ew<__bf16, ADD>(key, x, res, y, n, stream);
  const int64_t n8 = n >> 3;
  if (n8 > 0) {
    k_drop_ew_bf16v<ADD><<<(int)dmin64((n8 + 255) / 256, 8192), 256, 0,
                           S(stream)>>>(key, (const __bf16*)x,
                                        (const __bf16*)res, (__bf16*)y, n8);
    OB_LAUNCH_CHECK();
  }
  if (n8 * 8 < n) {  // < 8 trailing elements: their one or two 4-groups
    k_drop_tail_bf16<ADD><<<1, 64, 0, S(stream)>>>(
        key, (const __bf16*)x, (const __bf16*)res, (__bf16*)y, n8 * 2, n);
    OB_LAUNCH_CHECK();
  }
  return 0;
}

// ---------------------------------------------------------------------------
// dm = keep*scale*dy over [M,N] (element index r*N + c), db[n] += colsum(dm)
// ---------------------------------------------------------------------------

#define DCS_ROWS 128

// any dtype / width / alignment.  Block = 256 columns x DCS_ROWS rows, one
// atomic per column per block; the colsum adds the values as stored (the
// bf16-rounded dm on the bf16 path).  DET (deterministic mode, both kernels):
// db is the partial slab [gridDim.y][N]; row blockIdx.y = rows [128 y,
// 128 y + 128), a function of the shape alone; every (y, c < N) is written.
template <typename T, bool DET = false>
__global__ __launch_bounds__(256) void k_drop_cs(ob_drop_key key, const T* dy,
                                                 T* dm,
                                                 float* __restrict__ db,
                                                 int64_t M, int64_t N) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  const int64_t r0 = (int64_t)blockIdx.y * DCS_ROWS;
  const int64_t r1 = dmin64(M, r0 + DCS_ROWS);
  float acc = 0.f;
  for (int64_t r = r0; r < r1; ++r) {
    const int64_t e = r * N + c;
    const ob_philox4 w = ob_drop_words(key, (uint32_t)(e >> 2));
    const uint32_t wj = (e & 3) == 0 ? w.w[0] : (e & 3) == 1 ? w.w[1]
                        : (e & 3) == 2 ? w.w[2] : w.w[3];
    const float v = drop_mul(key, wj, dld(dy + e));
    dst(dm + e, v);
    acc += dld(dm + e);
  }
  if constexpr (DET) db[(int64_t)blockIdx.y * N + c] = acc;
  else atomicAdd(&db[c], acc);
}

// bf16, N % 8 == 0, 16-byte aligned: the k_gelu_bwd_cs_bf16 tiling.  Block =
// 16 col-threads x 16 row-threads over 128 cols x DCS_ROWS rows; a thread
// owns 8 fixed columns and keeps 4 rows in flight.  Column partials fold
// registers -> wave shfl -> LDS -> one atomic per column per block.
template <bool DET = false>
__global__ __launch_bounds__(256) void k_drop_cs_bf16(
    ob_drop_key key, const __bf16* dy, __bf16* dm, float* __restrict__ db,
    int64_t M, int64_t N) {
  __shared__ float red[4][128];
  const int tid = threadIdx.x;
  const int cg = tid & 15, rt = tid >> 4;
  const int lane = tid & 63, wv = tid >> 6;
  const int64_t c0 = (int64_t)blockIdx.x * 128 + cg * 8;
  const int64_t rbase = (int64_t)blockIdx.y * DCS_ROWS + rt;
  float acc[8] = {0};
  if (c0 < N) {  // N % 8 == 0: the whole 8-column group is in range
    for (int it = 0; it < DCS_ROWS / 64; ++it) {
      uint4 gin[4] = {};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t r = rbase + it * 64 + i * 16;
        if (r < M) gin[i] = *reinterpret_cast<const uint4*>(dy + r * N + c0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t r = rbase + it * 64 + i * 16;
        if (r < M) {
          const int64_t e = r * N + c0;  // multiple of 8
          const ob_philox4 r0 = ob_drop_words(key, (uint32_t)(e >> 2));
          const ob_philox4 r1 = ob_drop_words(key, (uint32_t)((e >> 2) + 1));
          float gv[8], out[8];
          dunpack8(gin[i], gv);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const uint32_t w = j < 4 ? r0.w[j] : r1.w[j - 4];
            out[j] = dbf2f((__bf16)drop_mul(key, w, gv[j]));
            acc[j] += out[j];
          }
          *reinterpret_cast<uint4*>(dm + r * N + c0) = dpack8(out);
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

template <typename T, bool DET = false>
static int launch_cs(const ob_drop_key& key, const void* dy, void* dm,
                     void* db, int64_t M, int64_t N, void* stream) {
  dim3 grid((unsigned)((N + 255) / 256),
            (unsigned)((M + DCS_ROWS - 1) / DCS_ROWS));
  k_drop_cs<T, DET><<<grid, 256, 0, S(stream)>>>(key, (const T*)dy, (T*)dm,
                                                 (float*)db, M, N);
  OB_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// embedding with the mask folded in (e = row*H + c over the [B,S,H] output)
// ---------------------------------------------------------------------------

__device__ __forceinline__ uint32_t drop_word_at(const ob_drop_key& key,
                                                 int64_t e) {
  const ob_philox4 w = ob_drop_words(key, (uint32_t)(e >> 2));
  const int j = (int)(e & 3);
  return j == 0 ? w.w[0] : j == 1 ? w.w[1] : j == 2 ? w.w[2] : w.w[3];
}

template <typename T>
__global__ __launch_bounds__(256) void k_embed_fwd_drop(
    ob_drop_key key, const int64_t* __restrict__ ids,
    const float* __restrict__ wte, const float* __restrict__ wpe,
    T* __restrict__ out, int64_t BS, int Sq, int H) {
  for (int64_t row = blockIdx.x; row < BS; row += gridDim.x) {
    const int64_t id = ids[row];
    const int s = (int)(row % Sq);
    const float* te = wte + id * H;
    const float* pe = wpe + (int64_t)s * H;
    T* o = out + row * H;
    for (int c = threadIdx.x; c < H; c += 256) {
      const uint32_t w = drop_word_at(key, row * H + c);
      dst(o + c, drop_mul(key, w, __fadd_rn(te[c], pe[c])));
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_embed_bwd_drop(
    ob_drop_key key, const int64_t* __restrict__ ids,
    const T* __restrict__ dout, float* __restrict__ dwte,
    float* __restrict__ dwpe, int64_t BS, int Sq, int H) {
  for (int64_t row = blockIdx.x; row < BS; row += gridDim.x) {
    const int64_t id = ids[row];
    const int s = (int)(row % Sq);
    const T* d = dout + row * H;
    for (int c = threadIdx.x; c < H; c += 256) {
      const uint32_t w = drop_word_at(key, row * H + c);
      if (w >= key.thr) {  // a dropped element contributes exactly 0
        const float v = __fmul_rn(dld(d + c), key.scale);
        atomicAdd(&dwte[id * H + c], v);
        atomicAdd(&dwpe[(int64_t)s * H + c], v);
      }
    }
  }
}

// Deterministic embedding backward, owner-computes (no atomics, no slab):
// blocks [0, BS) are token rows, blocks [BS, BS + Sq) positions.
// dwpe[s]: its block adds the B rows of position s in ascending b and does
// one += per column.  dwte: the block of token row t is the LEADER of its id
// if no row < t has the same id; a leader adds the rows with that id in
// ascending row order and does one += per column; other blocks leave.  Every
// dwte / dwpe element has one writer per launch.  The ids are scanned once
// per block, 256 rows at a time: the four waves' ballots of "same id" go to
// LDS and every thread walks their set bits in ascending order for the
// EBD_CPT columns it holds in registers (wider rows take further passes).
// DROP applies the keep*scale of k_embed_bwd_drop (a dropped element is
// skipped).
#define EBD_CPT 8
template <bool DROP>
__global__ __launch_bounds__(256) void k_embed_bwd_det_bf16(
    ob_drop_key key, const int64_t* __restrict__ ids,
    const __bf16* __restrict__ dout, float* __restrict__ dwte,
    float* __restrict__ dwpe, int64_t BS, int Sq, int H) {
  __shared__ int dup;
  __shared__ unsigned long long match[4];
  auto term = [&](int64_t row, int c, float* acc) {
    const float d = dld(dout + row * H + c);
    if (DROP) {
      if (drop_word_at(key, row * H + c) >= key.thr)
        *acc += __fmul_rn(d, key.scale);
    } else {
      *acc += d;
    }
  };
  if ((int64_t)blockIdx.x >= BS) {
    const int64_t s = (int64_t)blockIdx.x - BS;
    for (int c = threadIdx.x; c < H; c += 256) {
      float acc = 0.f;
      for (int64_t row = s; row < BS; row += Sq) term(row, c, &acc);
      dwpe[s * H + c] += acc;
    }
    return;
  }
  const int64_t t = blockIdx.x;
  const int64_t id = ids[t];
  if (threadIdx.x == 0) dup = 0;
  __syncthreads();
  int mine = 0;
  for (int64_t r = threadIdx.x; r < t; r += 256) mine |= ids[r] == id;
  if (mine) dup = 1;  // every writer stores the same value
  __syncthreads();
  if (dup) return;  // block-uniform
  const int wid = threadIdx.x >> 6;
  for (int cb = 0; cb < H; cb += 256 * EBD_CPT) {
    float acc[EBD_CPT] = {0};
    for (int64_t base = t; base < BS; base += 256) {
      const int64_t r = base + threadIdx.x;
      const unsigned long long m = __ballot(r < BS && ids[r] == id);
      if ((threadIdx.x & 63) == 0) match[wid] = m;
      __syncthreads();
#pragma unroll 1
      for (int w = 0; w < 4; ++w) {
        unsigned long long bits = match[w];
        while (bits) {
          const int i = __ffsll((long long)bits) - 1;
          bits &= bits - 1;
          const int64_t row = base + w * 64 + i;
#pragma unroll
          for (int j = 0; j < EBD_CPT; ++j) {
            const int c = cb + threadIdx.x + j * 256;
            if (c < H) term(row, c, &acc[j]);
          }
        }
      }
      __syncthreads();  // match[] is rewritten by the next chunk
    }
#pragma unroll
    for (int j = 0; j < EBD_CPT; ++j) {
      const int c = cb + threadIdx.x + j * 256;
      if (c < H) dwte[id * H + c] += acc[j];
    }
  }
}

// key null: no dropout
int ob_embed_bwd_det(const ob_drop_key* key, const int64_t* ids,
                     const void* dout, float* dwte, float* dwpe, int64_t B,
                     int64_t Sq, int64_t H, void* stream) {
  const int64_t BS = B * Sq;
  if (BS <= 0 || H <= 0) return 0;
  if (BS * H > OB_DROP_MAX_N) return ob_fail("dropout: n > 2^34 unsupported");
  if (BS + Sq > INT32_MAX) return ob_fail("embed_bwd_det: B*S too large");
  const unsigned grid = (unsigned)(BS + Sq);
  if (key)
    k_embed_bwd_det_bf16<true><<<grid, 256, 0, S(stream)>>>(
        *key, ids, (const __bf16*)dout, dwte, dwpe, BS, (int)Sq, (int)H);
  else
    k_embed_bwd_det_bf16<false><<<grid, 256, 0, S(stream)>>>(
        ob_drop_key{}, ids, (const __bf16*)dout, dwte, dwpe, BS, (int)Sq,
        (int)H);
  OB_LAUNCH_CHECK();
  return 0;
}

int ob_embed_fwd_drop(const ob_drop_key& key, int bf16, const int64_t* ids,
                      const float* wte, const float* wpe, void* out, int64_t B,
                      int64_t Sq, int64_t H, void* stream) {
  const int64_t BS = B * Sq;
  if (BS * H > OB_DROP_MAX_N) return ob_fail("dropout: n > 2^34 unsupported");
  const int grid = (int)dmin64(BS, 16384);
  if (bf16)
    k_embed_fwd_drop<__bf16><<<grid, 256, 0, S(stream)>>>(
        key, ids, wte, wpe, (__bf16*)out, BS, (int)Sq, (int)H);
  else
    k_embed_fwd_drop<float><<<grid, 256, 0, S(stream)>>>(
        key, ids, wte, wpe, (float*)out, BS, (int)Sq, (int)H);
  OB_LAUNCH_CHECK();
  return 0;
}

int ob_embed_bwd_drop(const ob_drop_key& key, int bf16, const int64_t* ids,
                      const void* dout, float* dwte, float* dwpe, int64_t B,
                      int64_t Sq, int64_t H, void* stream) {
  const int64_t BS = B * Sq;
  if (BS * H > OB_DROP_MAX_N) return ob_fail("dropout: n > 2^34 unsupported");
  const int grid = (int)dmin64(BS, 16384);
  if (bf16)
    k_embed_bwd_drop<__bf16><<<grid, 256, 0, S(stream)>>>(
        key, ids, (const __bf16*)dout, dwte, dwpe, BS, (int)Sq, (int)H);
  else
    k_embed_bwd_drop<float><<<grid, 256, 0, S(stream)>>>(
        key, ids, (const float*)dout, dwte, dwpe, BS, (int)Sq, (int)H);
  OB_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// keyed launchers used by the layer orchestration (ob_internal.h)
// ---------------------------------------------------------------------------

int ob_drop_scale(const ob_drop_key& key, int bf16, const void* x, void* y,
                  int64_t n, void* stream) {
  return bf16 ? launch_ew_bf16<false>(key, x, nullptr, y, n, stream)
              : launch_ew<float, false>(key, x, nullptr, y, n, stream);
}

int ob_drop_add(const ob_drop_key& key, int bf16, const void* t,
                const void* res, void* y, int64_t n, void* stream) {
  return bf16 ? launch_ew_bf16<true>(key, t, res, y, n, stream)
              : launch_ew<float, true>(key, t, res, y, n, stream);
}

int ob_drop_scale_colsum(const ob_drop_key& key, int bf16, const void* dy,
                         void* dm, void* db, int64_t M, int64_t N,
                         void* stream, float* ws) {
  if (M <= 0 || N <= 0) return 0;
  if (M * N > OB_DROP_MAX_N) return ob_fail("dropout: n > 2^34 unsupported");
  if (ws && !bf16)
    return ob_fail("dropout_scale_colsum: the slab form is bf16 only");
  if (!bf16) return launch_cs<float>(key, dy, dm, db, M, N, stream);
  // ws (deterministic mode): the kernels' db is the slab, folded afterwards
  const int64_t nblk = (M + DCS_ROWS - 1) / DCS_ROWS;
  if (N % 8 == 0 && al16(dy) && al16(dm)) {
    dim3 grid((unsigned)((N + 127) / 128), (unsigned)nblk);
    if (ws)
      k_drop_cs_bf16<true><<<grid, 256, 0, S(stream)>>>(
          key, (const __bf16*)dy, (__bf16*)dm, ws, M, N);
    else
      k_drop_cs_bf16<false><<<grid, 256, 0, S(stream)>>>(
          key, (const __bf16*)dy, (__bf16*)dm, (float*)db, M, N);
    OB_LAUNCH_CHECK();
  } else if (ws ? launch_cs<__bf16, true>(key, dy, dm, ws, M, N, stream)
                : launch_cs<__bf16, false>(key, dy, dm, db, M, N, stream)) {
    return 1;
  }
  return ws ? ob_colpart_finish_f32(ws, nblk, N, N, db, stream) : 0;
}

// slab floats of ob_drop_scale_colsum with ws: one row per DCS_ROWS rows
int64_t ob_drop_cs_ws_count(int64_t M, int64_t N) {
  return (M + DCS_ROWS - 1) / DCS_ROWS * N;
}

// ---------------------------------------------------------------------------
// public standalone entry points (include/oobleck_stage.h)
// ---------------------------------------------------------------------------

static int key_from_args(uint64_t seed, int32_t layer_id, int32_t site,
                         uint64_t tick, float p, ob_drop_key* out) {
  if (!ob_drop_p_ok(p)) return ob_fail("dropout: p must be in [0,1)");
  if (site < 0 || site > 3) return ob_fail("dropout: bad site %d", site);
  if (layer_id < 0 || layer_id >= (1 << 24))
    return ob_fail("dropout: layer_id out of range");
  *out = ob_drop_make_key(seed, layer_id, site, tick, p);
  return 0;
}

#define OB_DROP_KEY()                                                   \
  ob_drop_key key;                                                      \
  if (key_from_args(seed, layer_id, site, tick, p, &key)) return 1

extern "C" int ob_dropout_mask(uint64_t seed, int32_t layer_id, int32_t site,
                               uint64_t tick, float p, int64_t n,
                               void* keep_u8, void* stream) {
  OB_DROP_KEY();
  if (n <= 0) return 0;
  if (n > OB_DROP_MAX_N) return ob_fail("dropout: n > 2^34 unsupported");
  const int64_t nq = (n + 3) >> 2;
  k_drop_mask<<<(int)dmin64((nq + 255) / 256, 8192), 256, 0, S(stream)>>>(
      key, n, (uint8_t*)keep_u8);
  OB_LAUNCH_CHECK();
  return 0;
}

extern "C" int ob_dropout_scale_f32(uint64_t seed, int32_t layer_id,
                                    int32_t site, uint64_t tick, float p,
                                    const void* x, void* y, int64_t n,
                                    void* stream) {
  OB_DROP_KEY();
  return ob_drop_scale(key, 0, x, y, n, stream);
}
extern "C" int ob_dropout_scale_bf16(uint64_t seed, int32_t layer_id,
                                     int32_t site, uint64_t tick, float p,
                                     const void* x, void* y, int64_t n,
                                     void* stream) {
  OB_DROP_KEY();
  return ob_drop_scale(key, 1, x, y, n, stream);
}
extern "C" int ob_dropout_add_f32(uint64_t seed, int32_t layer_id,
                                  int32_t site, uint64_t tick, float p,
                                  const void* t, const void* res, void* y,
                                  int64_t n, void* stream) {
  OB_DROP_KEY();
  return ob_drop_add(key, 0, t, res, y, n, stream);
}
extern "C" int ob_dropout_add_bf16(uint64_t seed, int32_t layer_id,
                                   int32_t site, uint64_t tick, float p,
                                   const void* t, const void* res, void* y,
                                   int64_t n, void* stream) {
  OB_DROP_KEY();
  return ob_drop_add(key, 1, t, res, y, n, stream);
}
extern "C" int ob_dropout_scale_colsum_f32(uint64_t seed, int32_t layer_id,
                                           int32_t site, uint64_t tick,
                                           float p, const void* dy, void* dm,
                                           void* db, int64_t M, int64_t N,
                                           void* stream) {
  OB_DROP_KEY();
  return ob_drop_scale_colsum(key, 0, dy, dm, db, M, N, stream);
}
extern "C" int ob_dropout_scale_colsum_bf16(uint64_t seed, int32_t layer_id,
                                            int32_t site, uint64_t tick,
                                            float p, const void* dy, void* dm,
                                            void* db, int64_t M, int64_t N,
                                            void* stream) {
  OB_DROP_KEY();
  return ob_drop_scale_colsum(key, 1, dy, dm, db, M, N, stream);
}
extern "C" int ob_dropout_scale_colsum_det_bf16(
    uint64_t seed, int32_t layer_id, int32_t site, uint64_t tick, float p,
    const void* dy, void* dm, void* db, int64_t M, int64_t N, void* ws,
    void* stream) {
  OB_DROP_KEY();
  if (!ws) return ob_fail("dropout_scale_colsum_det_bf16: ws required");
  return ob_drop_scale_colsum(key, 1, dy, dm, db, M, N, stream, (float*)ws);
}
extern "C" int ob_embed_bwd_det_bf16(const void* ids, const void* dout,
                                     void* dwte, void* dwpe, int64_t B,
                                     int64_t Sq, int64_t H, void* stream) {
  return ob_embed_bwd_det(nullptr, (const int64_t*)ids, dout, (float*)dwte,
                          (float*)dwpe, B, Sq, H, stream);
}
extern "C" int ob_embed_bwd_drop_det_bf16(uint64_t seed, int32_t layer_id,
                                          int32_t site, uint64_t tick, float p,
                                          const void* ids, const void* dout,
                                          void* dwte, void* dwpe, int64_t B,
                                          int64_t Sq, int64_t H,
                                          void* stream) {
  OB_DROP_KEY();
  return ob_embed_bwd_det(&key, (const int64_t*)ids, dout, (float*)dwte,
                          (float*)dwpe, B, Sq, H, stream);
}
