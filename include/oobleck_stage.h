/* include/oobleck_stage.h — the C-ABI drop-in boundary of the MI355X-native
 * rebuild of Oobleck's pipeline-parallel execution hot path.
 *
 * The reference implements this path in Python-on-torch; its internal seams
 * (the interfaces this ABI replaces) are:
 *
 *   - Layer forward/backward over one fx-sharded GPT-2 layer:
 *       /root/reference/oobleck/execution/layer.py:144-145 (forward),
 *       :250-260 (backward: loss.backward() on the last stage, else
 *       autograd.backward(outputs, received grads)).
 *   - The flat contiguous parameter buffer per layer consumed by the
 *     optimizer and by reconfiguration layer-copy:
 *       /root/reference/oobleck/execution/pipeline.py:117-119
 *       (_param_handle.flat_param), engine.py:283-299 (broadcast source).
 *   - The fused AdamW step over those flat buffers:
 *       /root/reference/oobleck/execution/pipeline.py:117-127, 241-244.
 *   - Per-instruction execution handlers the pipeline dispatches into:
 *       /root/reference/oobleck/execution/pipeline.py:169-244.
 *
 * Ownership: the CALLER (the Python host, via torch CUDA tensors) owns the
 * flat parameter / gradient / Adam-state buffers and all activation I/O
 * buffers — so RCCL collectives (grad all-reduce, reconfig broadcast) can
 * run on them directly through torch.distributed without copies.  The
 * extension owns only its internal activation stash and scratch workspace
 * (HIP memory, sized at bind time).
 *
 * Threading: one driving thread per GPU (matches 1 worker = 1 GPU,
 * /root/reference/oobleck/elastic/agent.py:141-174).  Calls are not
 * thread-safe.  All compute is asynchronous on the hipStream_t passed per
 * call; no call synchronizes the device.
 *
 * Errors: every function returns 0 on success, non-zero on failure; the
 * last failure message is available via ob_last_error().  No exceptions
 * cross the ABI.
 *
 * Python-side binding: ctypes over this header.
 */
#ifndef OOBLECK_STAGE_H
#define OOBLECK_STAGE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- layer kinds: the fx-shard grain of the reference -------------------
 * (/root/reference/oobleck/module/sharding.py:12-47: GPT model splits into
 *  [embedding] [transformer.h.i]*L [ln_f + lm_head + loss])              */
enum {
  OB_KIND_EMBED = 0,  /* wte gather + wpe add            ids[B,S] -> f32[B,S,H] */
  OB_KIND_BLOCK = 1,  /* LN1/QKV/attn/proj/LN2/MLP block f32[B,S,H] -> f32[B,S,H] */
  OB_KIND_FINAL = 2   /* ln_f + lm_head + shifted CE     f32[B,S,H] -> f32 loss  */
};

typedef struct ob_layer* ob_layer_t;

typedef struct {
  int32_t kind;         /* OB_KIND_* */
  int32_t n_embd;       /* H */
  int32_t n_head;
  int32_t n_positions;
  int32_t vocab_size;
  int32_t max_batch;    /* microbatch size the stash is sized for */
  int32_t seq_len;      /* S */
  int32_t n_slots;      /* in-flight microbatches (pipeline buffer slots,
                           deepspeed-compatible num_pipe_buffers) */
  int32_t dtype;        /* 0 = fp32; 1 = bf16 activations/GEMMs with fp32
                           master weights + fp32 grads (§8 f4) */
} ob_layer_desc;

/* Number of fp32 elements in the layer's flat parameter buffer.  Layout is
 * the canonical order shared with oracle/gpt2_oracle.py::layer_param_spec. */
int64_t ob_layer_param_count(const ob_layer_desc* desc);

/* Create a layer; allocates the activation stash + workspace on the current
 * HIP device.  Parameters/grads are NOT allocated here — see ob_layer_bind. */
int ob_layer_create(const ob_layer_desc* desc, ob_layer_t* out);

/* ---- dropout (GPT-2's embd / resid / attn pdrop) --------------------------
 * Masks are stateless: a keep bit is Philox4x32-10 of (seed, layer_id, site,
 * tick, element index) -- see DESIGN.md "Dropout masks" for the frozen
 * definition.  The backward of a slot regenerates the masks of that slot's
 * forward from the tick the forward used; nothing is stashed.
 * Sites: 0 embedding output [B,S,H], 1 attention probabilities [B,nh,S,S],
 * 2 attention-projection output [B,S,H], 3 MLP-projection output [B,S,H]. */
enum {
  OB_DROP_EMBD = 0,
  OB_DROP_ATTN = 1,
  OB_DROP_RESID_ATTN = 2,
  OB_DROP_RESID_MLP = 3
};

typedef struct {
  float embd_pdrop;     /* EMBED layers; each probability in [0,1) */
  float resid_pdrop;    /* BLOCK layers, sites 2 and 3 */
  float attn_pdrop;     /* BLOCK layers, site 1.  A flash-eligible layer draws
                           the masks inside the flash kernels
                           (ob_flash_*_nt_drop_bf16); with OB_FLASH_DROP=0 or
                           OB_FLASH_TR=0 in the environment, > 0 takes the
                           materialized-P attention path instead */
  int32_t layer_id;     /* 0 <= layer_id < 2^24 */
  uint64_t seed;
} ob_dropout_desc;

/* ob_layer_create with dropout.  drop NULL or all probabilities 0 is exactly
 * ob_layer_create: the same kernels are launched and nothing else. */
int ob_layer_create_ex(const ob_layer_desc* desc, const ob_dropout_desc* drop,
                       ob_layer_t* out);

/* 1 when the layer's attention runs the fused flash kernels (bf16 BLOCK,
 * n_embd % n_head == 0, head_dim 64 or 128, seq_len % 128 == 0; at head_dim
 * 64, for attn_pdrop > 0, neither OB_FLASH_DROP=0 nor OB_FLASH_TR=0; at
 * head_dim 128 attn_pdrop == 0 and neither OB_FLASH_TR=0 nor
 * OB_FLASH_HD128=0), 0 otherwise.  Host-only. */
int ob_layer_uses_flash(ob_layer_t l);
/* The same decision for a description, before any layer exists: what
 * ob_layer_create_ex will take for `desc` with this attn_pdrop.  Host-only,
 * no GPU call. */
int ob_flash_eligible(const ob_layer_desc* desc, float attn_pdrop);

/* The device memory ob_layer_create_ex takes for `desc` (drop may be null),
 * from the same table the create allocates by (DESIGN.md "Layer memory").
 * modes: bit 0 deterministic, 1 OB_BF16_FLASH, 2 OB_FLASH_TR, 3
 * OB_FLASH_DROP, 4 OB_FLASH_HD128 (a set bit = that switch on); -1 = this
 * process's.  Writes up to cap int64s and returns the field count (-1 on a
 * null argument).  Fields, in order: flash, side (needs the side stream),
 * v_pad, slot_stride (floats of one stash slot), ids_count (int64s, all
 * slots), shadow_count (bf16 elements); the 15 stash regions' offsets within
 * a slot, then their lengths (floats; x, mean1, rstd1, ln1, qkv, p, attnm,
 * hmid, mean2, rstd2, ln2, u, g, logits, lse; length 0 = not of this kind);
 * the 10 shadows' offsets (bf16 elements; qkv, qkv_t, ap, ap_t, fc, fc_t,
 * mp, mp_t, lm, lm_t); the floats needed of each of the 16 shared workspace
 * buffers (0 = not used; dp, dln, datt, dqkv, dy4, flash_bwd, flash_vt, dw_a,
 * dw_b, pd_fwd, pd_bwd, dm_attn, dm_mlp, det_main, det_side, det_fwd); the
 * layout of flash_bwd under OB_FLASH_TR=0: offsets of Q^T, K^T, dO^T (bf16
 * elements) and of D (floats).  Host-only, no GPU call. */
int ob_layer_plan_query(const ob_layer_desc* desc,
                        const ob_dropout_desc* drop, int modes, int64_t* out,
                        int cap);

/* Training mode (default 1).  0 makes dropout inert (eval): forwards run
 * today's dropout-free path and do not advance the tick. */
int ob_layer_set_training(ob_layer_t l, int on);

/* Tick of the NEXT forward (default 0); each training forward of a layer
 * with dropout then post-increments it.  The tick a forward used is kept per
 * slot, and the backward of slot s uses slot s's tick. */
int ob_layer_set_dropout_tick(ob_layer_t l, uint64_t tick);

/* Bind caller-owned device fp32 buffers of ob_layer_param_count() elements:
 * params (read/write: forward reads, adam writes) and grads (backward
 * ACCUMULATES, caller zeroes between steps).  Mirrors flat_param /
 * flat_param.grad of the reference's FlatParamHandle (layer.py:96-111). */
int ob_layer_bind(ob_layer_t l, void* params, void* grads);

/* Set the actual microbatch size (<= max_batch) for subsequent calls. */
int ob_layer_set_batch(ob_layer_t l, int32_t batch);

/* Forward one microbatch in stash slot `slot` (0 <= slot < n_slots).
 *   EMBED: in = int64 ids[B,S],  out = f32[B,S,H],   labels ignored
 *   BLOCK: in = f32[B,S,H],      out = f32[B,S,H],   labels ignored
 *   FINAL: in = f32[B,S,H],      labels = int64[B,S], out = f32[1] (mean
 *          shifted CE loss, modeling_gpt2 semantics)
 * Asynchronous on `stream` (a hipStream_t). */
int ob_layer_forward(ob_layer_t l, int32_t slot, const void* in, void* out,
                     const int64_t* labels, void* stream);

/* Backward for the microbatch stashed in `slot`.
 *   FINAL: dout = NULL (seed dloss = 1.0, the last-stage semantics of
 *          layer.py:250-253) or f32[1] scale; din = f32[B,S,H]
 *   BLOCK: dout = f32[B,S,H], din = f32[B,S,H]
 *   EMBED: dout = f32[B,S,H], din ignored (int input)
 * Accumulates into the bound grad buffer (autograd += semantics). */
int ob_layer_backward(ob_layer_t l, int32_t slot, const void* dout, void* din,
                      void* stream);

int ob_layer_destroy(ob_layer_t l);

/* bf16 mode only: refresh the extension's bf16 weight shadows (plain +
 * transposed layouts) from the fp32 master params — call after ob_layer_bind
 * and after every optimizer step. */
int ob_layer_refresh_weights(ob_layer_t l, void* stream);

/* Fused AdamW over a flat buffer (replaces torch AdamW(fused=True) of
 * pipeline.py:117-127; decoupled weight decay + bias correction, eps added
 * after sqrt(v)/sqrt(bc2), matching torch.optim.AdamW).  step is 1-based. */
int ob_adamw_step(void* p, const void* g, void* m, void* v, int64_t n,
                  int32_t step, float lr, float beta1, float beta2, float eps,
                  float weight_decay, void* stream);

/* ---- global gradient-norm clipping (the `# amp enable check: gradient
 * clipping` seam the reference left open at pipeline.py:241-244) ----------
 *
 * Three calls per optimizer step, all asynchronous on `stream`, no host
 * synchronisation: per-tensor square norms -> (the host all-reduces the
 * per-layer vector over the pipeline's ranks) -> ob_clip_finish -> one
 * ob_adamw_step_scaled per flat buffer.  The caller owns every buffer.
 *
 * Semantics: the norm is taken over the gradient the optimizer consumes
 * (after the data-parallel all-reduce that is the SUM over replicas; the
 * reference never averages).  It is bit-identical across replicas whose
 * layers have the same shard count, whatever their stage splits.  Where
 * shard counts differ, a layer's fp64 partial sums associate differently:
 * totals agree to fp64 rounding, which can in principle move the fp32
 * coefficient by one ulp. */

/* Workspace size of ob_sqnorm_multi_f32, in doubles, for `n` tensors of
 * counts[i] elements. */
int64_t ob_sqnorm_ws_count(const int64_t* counts, int32_t n);

/* out[out_index[i]] = sum_j g_i[j]^2 in fp64 for n fp32 device buffers.
 * ptrs / counts / out_index are HOST arrays (out_index NULL = identity);
 * ws (ob_sqnorm_ws_count doubles) and out are device fp64.  Output slots not
 * named in out_index are left untouched; a 0-element tensor writes 0.
 * Products and sums are fp64 from the first multiply.  Deterministic: the
 * result for a tensor depends only on its values and element count, never on
 * the run, the pointer's alignment (4-byte alignment is required, 16-byte
 * enables vector loads) or the other tensors in the call.  No atomics. */
int ob_sqnorm_multi_f32(const void* const* ptrs, const int64_t* counts,
                        const int32_t* out_index, int32_t n, void* ws,
                        void* out, void* stream);

/* Adds sq[0..n) (device fp64) in index order and writes the 4-double device
 * record stats = {total_sq, norm, coef, skipped_steps}:
 *   coef = (float)min(1, max_norm / (norm + 1e-6))   -- the semantics of
 *   torch.nn.utils.clip_grad_norm_, exactly 1.0f when norm + 1e-6 <= max_norm.
 * If the total is not finite, coef is the SKIP MARKER -1.0 (any coef < 0)
 * and skipped_steps is incremented; otherwise skipped_steps is left as is
 * (the caller zero-initialises the record once).  max_norm must be > 0. */
int ob_clip_finish(const void* sq, int32_t n, float max_norm, void* stats,
                   void* stream);

/* ob_adamw_step over g[i] * coef, with coef read on the device from the
 * record ob_clip_finish wrote; otherwise the same arithmetic (coef == 1.0f
 * is bit-identical to ob_adamw_step).  Deviation from torch's in-place
 * clip: the scaled gradient is NOT written back to g (it would add 4 B/param
 * of traffic and the caller zeroes g right after the step).  On the skip
 * marker none of p, m, v is touched. */
int ob_adamw_step_scaled(void* p, const void* g, void* m, void* v, int64_t n,
                         int32_t step, float lr, float beta1, float beta2,
                         float eps, float weight_decay, const void* clip_stats,
                         void* stream);

/* ---- standalone kernel entry points (parity tests + roofline probes) ---- */

/* C[M,N] (+)= alpha * op(A)[M,K] @ op(B)[K,N] + bias[n] + R[m,n]
 * op(X) = X stored row-major [M,K]/[K,N]; transX=1 means X is stored
 * transposed ([K,M]/[N,K]).  Two-level strided batch: z = i1*n2 + i2,
 * operand offset = i1*stride?1 + i2*stride?2.  beta 0 or 1.  bias/R NULL to
 * skip.  atomic!=0 stores via atomicAdd (used for split-K weight grads). */
int ob_gemm_f32(int transA, int transB, int64_t M, int64_t N, int64_t K,
                float alpha, const void* A, int64_t lda,
                int64_t strideA1, int64_t strideA2,
                const void* B, int64_t ldb,
                int64_t strideB1, int64_t strideB2,
                float beta, void* C, int64_t ldc,
                int64_t strideC1, int64_t strideC2,
                int64_t n1, int64_t n2,
                const void* bias, const void* residual, int atomic, int splitk,
                void* stream);

/* LayerNorm over the last dim: y = (x-mu)*rstd*w + b, rows x H. */
int ob_layernorm_fwd_f32(const void* x, const void* w, const void* b, void* y,
                         void* mean, void* rstd, int64_t rows, int64_t H,
                         float eps, void* stream);
/* dx (+)= LN backward (accumulate if dx_accum); dw,db accumulated atomically. */
int ob_layernorm_bwd_f32(const void* x, const void* w, const void* mean,
                         const void* rstd, const void* dy, void* dx,
                         void* dw, void* db, int64_t rows, int64_t H,
                         int dx_accum, void* stream);

/* Causal row softmax in place on scores[batch, S, S] (row r keeps cols 0..r),
 * scale applied before the max. */
int ob_softmax_causal_fwd_f32(void* scores, int64_t batch, int64_t S,
                              float scale, void* stream);
/* dS = P * (dP - rowsum(dP*P)), in place on dP. */
int ob_softmax_causal_bwd_f32(const void* P, void* dP, int64_t batch,
                              int64_t S, void* stream);

/* gelu_new (tanh approximation, transformers NewGELUActivation). */
int ob_gelu_fwd_f32(const void* u, void* g, int64_t n, void* stream);
int ob_gelu_bwd_f32(const void* u, const void* dg, void* du, int64_t n,
                    void* stream);

/* db[n] += sum_m X[m,n] (bias gradient). */
int ob_colsum_f32(const void* X, void* db, int64_t M, int64_t N, void* stream);

/* Dropout kernels over the mask of (seed, layer_id, site, tick), element
 * index = flat index into the tensor; p in [0,1); n (or M*N) <= 2^34.
 * keep_u8[e] = 1 if element e is kept. */
int ob_dropout_mask(uint64_t seed, int32_t layer_id, int32_t site,
                    uint64_t tick, float p, int64_t n, void* keep_u8,
                    void* stream);
/* y = keep * x / (1-p); y may alias x. */
int ob_dropout_scale_f32(uint64_t seed, int32_t layer_id, int32_t site,
                         uint64_t tick, float p, const void* x, void* y,
                         int64_t n, void* stream);
int ob_dropout_scale_bf16(uint64_t seed, int32_t layer_id, int32_t site,
                          uint64_t tick, float p, const void* x, void* y,
                          int64_t n, void* stream);
/* y = res + keep * t / (1-p); y may alias t. */
int ob_dropout_add_f32(uint64_t seed, int32_t layer_id, int32_t site,
                       uint64_t tick, float p, const void* t, const void* res,
                       void* y, int64_t n, void* stream);
int ob_dropout_add_bf16(uint64_t seed, int32_t layer_id, int32_t site,
                        uint64_t tick, float p, const void* t,
                        const void* res, void* y, int64_t n, void* stream);
/* dm[M,N] = keep * dy / (1-p) (dm may alias dy); db[n] += sum_m dm[m,n]
 * (fp32, atomically; on bf16 the bf16-rounded dm is what is summed). */
int ob_dropout_scale_colsum_f32(uint64_t seed, int32_t layer_id, int32_t site,
                                uint64_t tick, float p, const void* dy,
                                void* dm, void* db, int64_t M, int64_t N,
                                void* stream);
int ob_dropout_scale_colsum_bf16(uint64_t seed, int32_t layer_id, int32_t site,
                                 uint64_t tick, float p, const void* dy,
                                 void* dm, void* db, int64_t M, int64_t N,
                                 void* stream);

/* ---- bf16 mixed-precision path ------------------------
 * bf16 MFMA GEMM (v_mfma_f32_32x32x16_bf16, fp32 accumulate).  Same
 * call shape as ob_gemm_f32; A/B are bf16; out_kind: 0 = bf16 C,
 * 1 = fp32 C, 2 = fp32 atomicAdd (weight grads / split-K).  lda/ldb must
 * be multiples of 8 (16-byte staging). */
int ob_gemm_bf16(int transA, int transB, int64_t M, int64_t N, int64_t K,
                 float alpha, const void* A, int64_t lda,
                 int64_t strideA1, int64_t strideA2,
                 const void* B, int64_t ldb,
                 int64_t strideB1, int64_t strideB2,
                 float beta, void* C, int64_t ldc,
                 int64_t strideC1, int64_t strideC2,
                 int64_t n1, int64_t n2,
                 const void* bias, const void* residual, int out_kind,
                 int splitk, void* stream);
/* Host-only query (no GPU call): the route ob_gemm_bf16 takes for a call.
 * aligned16: A/B bases 16-byte aligned and their batch strides multiples of
 * 8.  env_mask: bit 0 OB_NO_BLASLT, bit 1 OB_BF16_NOGLDS, bit 2
 * OB_BF16_NO256; force: the OB_BF16_FORCE string or null.
 * out[5] = {hipBLASLt is tried first, kernel (0 generic, 1 glds 128x128,
 * 2 256-row, 3 256x256 8-phase; the fallback when hipBLASLt is tried),
 * N tile, generic kernel's edge guard, split-K}. */
int ob_gemm_bf16_route(int transA, int transB, int64_t M, int64_t N, int64_t K,
                       int64_t n1, int64_t n2, int out_kind, int splitk,
                       float beta, int aligned16, int env_mask,
                       const char* force, int32_t* out);

/* ---- hipBLASLt solution choice -----------------------
 * A library GEMM shape is 13 int64s: {transA, transB, M, N, K, lda, ldb, ldc,
 * fp32 out, beta != 0, bias epilogue, C-input is a buffer other than C,
 * fp32 A/B}, row-major semantics as in ob_gemm_lt*.  All host-only, and all
 * on the layer's driving thread: the per-stream plan caches they read or
 * rebuild are not locked, so none may run while a step is in flight or
 * beside a layer call on another thread.
 *
 * ob_layer_lt_shapes: the library GEMM shapes of a layer description at
 * M = max_batch * seq_len, the ones ob_layer_create tunes; writes up to cap
 * shapes and returns their number (-1 on a null argument).  No GPU call.
 * ob_gemm_lt_tune: measures the heuristic's first OB_LT_TUNE_N (default 8,
 * at most 128) candidates for one shape on scratch operands and records the
 * winner in the process-wide table, unless the table has the shape already.
 * A no-op with OB_LT_TUNE=0.
 * ob_gemm_lt_choice: out[10] = {has an entry, chosen solution index, tuned
 * (0: tuning was abandoned, top-1 runs), top-1's solution index, top-1's
 * microseconds, the chosen solution's microseconds, candidates tried,
 * candidates dropped, tuning wall milliseconds, top-1's max - min over the
 * rounds (the margin a challenger must beat)}; the two kernel names go to
 * top1_name / chosen_name (name_cap bytes each, may be null).
 * ob_gemm_lt_candidates: the candidates the tuner timed, fastest first
 * (solution index, position in the candidate list, median microseconds);
 * writes up to cap and returns their number (-1 on a null argument).
 * ob_gemm_lt_table_size: entries in the table.
 * ob_gemm_lt_untuned_uses: library GEMM calls so far, with tuning on, whose
 * shape had no table entry when its plan was built (0 for a training step
 * at the batch the layers were created for).
 * ob_gemm_lt_plan_index: the solution index of the plan this stream holds
 * for a shape, -1 if it has none. */
int ob_layer_lt_shapes(const ob_layer_desc* desc, int64_t* out, int cap);
int ob_gemm_lt_tune(const int64_t* shape);
int ob_gemm_lt_choice(const int64_t* shape, double* out, char* top1_name,
                      char* chosen_name, int name_cap);
int ob_gemm_lt_candidates(const int64_t* shape, int32_t* index, int32_t* pos,
                          double* us, int cap);
int64_t ob_gemm_lt_table_size(void);
int64_t ob_gemm_lt_untuned_uses(void);
int ob_gemm_lt_plan_index(const int64_t* shape, void* stream);

/* ---- sliced weight grads ------------------------------
 * A TN weight grad C[M,N] += A[K,M]^T B[K,N] (bf16 operands, fp32 C, ldc ==
 * N) whose 128 x 128 output tiles are fewer than the device's CUs may run as
 * s K-slices: one strided-batched library matmul, slice i into slab i of a
 * [s, M, N] fp32 slab with beta = 0, then k_dw_fold adds the slabs to C in
 * ascending order.  ob_layer_create measures the sliced forms of a BLOCK's
 * weight grads beside the unsliced candidates (by itself at most 2 slices)
 * and the step runs the winner;
 * OB_DW_SLICES=1 never slices, OB_DW_SLICES=n forces n where the rule admits
 * it; deterministic mode, OB_LT_TUNE=0 and OB_NO_BLASLT=1 never slice.
 *
 * ob_dw_slices_admit (host-only, no GPU call): 1 if the rule admits s slices
 * of the shape on a device of cus CUs with a slab of slab_floats floats: TN,
 * fp32 out, beta = 1, no bias, no C-input, bf16 operands, ldc == N, fewer
 * tiles than CUs, s in {2, 4, 8, 16}, K % s == 0, K / s a multiple of 256 and
 * at least 1024, s * M * N <= slab_floats.
 * ob_gemm_lt_dw_sliced: the call with an explicit s, on the caller's stream;
 * runs s slices if the rule admits them on this device, else the unsliced
 * library call, and writes the count that ran to *used (may be null).
 * ob_gemm_lt_tune_slab: ob_gemm_lt_tune for a caller that can run the shape
 * sliced with a slab of slab_floats floats: the sliced pairs (the first
 * OB_LT_TUNE_SLICE_N, default 2, candidates of the batched problem per
 * admitted slice count, each with the fold) are timed in the same rounds.
 * ob_gemm_lt_tune itself tunes unsliced.
 * ob_gemm_lt_slices: the sliced side of a shape's table entry.  out[6] =
 * {has an entry, the slice count the step runs (1 unsliced), the batched
 * problem's solution index (-1 unsliced), the fastest sliced pair's median
 * microseconds (matmul + fold, 0 if none was timed), the milliseconds the
 * sliced candidates added to the shape's tuning time, that fastest pair's
 * slice count}; every sliced pair timed goes to slices / index / us, fastest
 * first, up to cap; returns their number (-1 on a null argument). */
int ob_dw_slices_admit(const int64_t* shape, int s, int cus,
                       int64_t slab_floats);
int ob_gemm_lt_dw_sliced(int64_t M, int64_t N, int64_t K, const void* A,
                         int64_t lda, const void* B, int64_t ldb, void* C,
                         int64_t ldc, int s, void* slab, int64_t slab_floats,
                         void* stream, int32_t* used);
int ob_gemm_lt_tune_slab(const int64_t* shape, int64_t slab_floats);
int ob_gemm_lt_slices(const int64_t* shape, double* out, int32_t* slices,
                      int32_t* index, double* us, int cap);

/* Fused causal flash attention on packed bf16 qkv [B, Sq, 3H] (H % nh == 0,
 * head_dim 64 or 128 — the entries dispatch on H / nh —, Sq % 128 == 0)
 * without transposed operand copies: the kernels read the
 * column-major MFMA operands from their row-major LDS tiles.
 * fwd: O bf16 [B, Sq, H], lse fp32 [B*nh, Sq].
 * bwd: D fp32 [B*nh, Sq] = rowsum(dO * O); dqkv bf16 [B, Sq, 3H];
 * dbias_qkv: fp32 [3H] or null; when given, the column sums of dqkv (from
 * the fp32 accumulators, before bf16 rounding) are atomically added. */
int ob_flash_fwd_nt_bf16(const void* qkv, void* O, void* lse, int64_t B,
                         int64_t Sq, int64_t H, int64_t nh, float scale,
                         void* stream);
int ob_flash_bwd_nt_bf16(const void* qkv, const void* dO, const void* lse,
                         const void* D, void* dqkv, void* dbias_qkv,
                         int64_t B, int64_t Sq, int64_t H, int64_t nh,
                         float scale, void* stream);
/* The same backward without a D input: the dq kernel forms D from O and dO
 * (at head_dim 64 bit-identical to ob_flash_dsum_bf16's), writes it to D_ws
 * (fp32 [B*nh, Sq]) and the dkdv kernel, launched after it, reads it there. */
int ob_flash_bwd_nt_d_bf16(const void* qkv, const void* O, const void* dO,
                           const void* lse, void* D_ws, void* dqkv,
                           void* dbias_qkv, int64_t B, int64_t Sq, int64_t H,
                           int64_t nh, float scale, void* stream);
/* ob_flash_fwd_nt_bf16 / ob_flash_bwd_nt_d_bf16 with attention dropout drawn
 * inside the kernels: site OB_DROP_ATTN of (seed, layer_id, tick, p), element
 * index into the full [B*nh, Sq, Sq] square as the dropout section above
 * defines it; no mask or P is stored.  The forward's LSE is that of the
 * undropped P and O = (P * factor) V; the backward must be given the
 * forward's key.  head_dim 64 only; otherwise the shape rules of the plain
 * entries; also p in [0,1) and B*nh*Sq*Sq <= 2^34.  p == 0 launches the
 * plain kernels. */
int ob_flash_fwd_nt_drop_bf16(const void* qkv, void* O, void* lse, int64_t B,
                              int64_t Sq, int64_t H, int64_t nh, float scale,
                              uint64_t seed, int32_t layer_id, uint64_t tick,
                              float p, void* stream);
int ob_flash_bwd_nt_d_drop_bf16(const void* qkv, const void* O, const void* dO,
                                const void* lse, void* D_ws, void* dqkv,
                                void* dbias_qkv, int64_t B, int64_t Sq,
                                int64_t H, int64_t nh, float scale,
                                uint64_t seed, int32_t layer_id, uint64_t tick,
                                float p, void* stream);
/* Host-only queries of the block -> work mapping of the three kernels above
 * (no GPU call).  kind: 0 forward, 1 dq, 2 dkdv.
 * rows: unit = wave 0..3 (forward, dq) or wave pair 0..1 (dkdv) of `block`
 *   -> the first of its 32 rows and the tile range it computes; unit = -1 ->
 *   the tile range the block stages (row0 = -1).  Tiles: 64 kv rows for
 *   forward and dq, 32 q rows for dkdv.
 * grid: blocks launched for Z = B*nh heads, padding included.
 * id: linear block id -> (z, block); returns 1, or 0 for a padding id. */
int ob_flash_fold_rows(int64_t kind, int64_t Sq, int64_t block, int64_t unit,
                       int64_t* row0, int64_t* first_tile, int64_t* n_tiles);
int64_t ob_flash_fold_grid(int64_t kind, int64_t Sq, int64_t Z);
int ob_flash_fold_id(int64_t kind, int64_t Sq, int64_t Z, int64_t id,
                     int64_t* z, int64_t* block);

/* ---- deterministic mode -------------------------------
 * Off by default; with it off every launch is what it was.  With it on, every
 * array a bf16 training step produces (loss, activations, din, flat grads,
 * params and AdamW moments) is bit-identical between two fresh processes of
 * the same build on the same machine, given the same inputs, seeds, batch,
 * slot sequence and stream usage.  Shown: layer stacks
 * of all three kinds on every attention / LayerNorm / dropout route, and the
 * GPT-2 small benchmark step with forward and backward on ONE stream.  NOT
 * covered: a forward that runs beside a backward on another stream (the
 * Python pipeline's pp1 overlap, which it therefore leaves off in the mode),
 * and OB_NO_BLASLT=1.  The sums that otherwise go through
 * atomicAdd (bias grads, LayerNorm dw/db, embedding grads, the loss) are
 * formed in a fixed order instead: each block stores its per-column partial
 * to its own row of a slab and ob_colpart_finish_f32 folds the rows; the
 * embedding backward is owner-computes.  In the mode the b_qkv grad of a
 * flash layer is the column sum of the bf16-ROUNDED dqkv (ob_colsum_det_bf16
 * on the side stream; the flash kernels get dbias_qkv = NULL), the
 * hand-written dW fallback runs with split-K 1 and the library GEMMs run
 * their top-1 solution (no tuning, as with OB_LT_TUNE=0).
 *
 * The switch is process-wide.  Its default is the environment's
 * OB_DETERMINISTIC=1, read once.  ob_set_deterministic fails once a layer has
 * been created in the process; creating an fp32 layer (dtype 0) fails while
 * the mode is on.  ob_deterministic returns the current value. */
int ob_set_deterministic(int on);
int ob_deterministic(void);

/* The _det entries: their atomic siblings with the column sums run-to-run
 * bit-stable.  ws is a caller-owned fp32 device slab of ob_det_ws_count(which,
 * M, N) floats (rows, H for LayerNorm; B*Sq, 1 for the loss), written before
 * it is read in every call and not shared with a call on another stream.
 * Everything else (dx, du, dm, lse) is bit-identical to the sibling's. */
enum {
  OB_DET_WS_COLSUM = 0,
  OB_DET_WS_GELU = 1,
  OB_DET_WS_LN = 2,
  OB_DET_WS_DROP_CS = 3,
  OB_DET_WS_CE = 4
};
int64_t ob_det_ws_count(int which, int64_t M, int64_t N); /* host-only */
int ob_colsum_det_bf16(const void* X, void* db, int64_t M, int64_t N,
                       void* ws, void* stream);
int ob_gelu_bwd_colsum_det_bf16(const void* u, const void* dg, void* du,
                                void* db, int64_t M, int64_t N, void* ws,
                                void* stream);
int ob_layernorm_bwd_res_det_bf16(const void* x, const void* w,
                                  const void* mean, const void* rstd,
                                  const void* dy, const void* res, void* dx,
                                  void* dw, void* db, void* sum_res,
                                  void* sum_dx, int64_t rows, int64_t H,
                                  void* ws, void* stream);
int ob_dropout_scale_colsum_det_bf16(uint64_t seed, int32_t layer_id,
                                     int32_t site, uint64_t tick, float p,
                                     const void* dy, void* dm, void* db,
                                     int64_t M, int64_t N, void* ws,
                                     void* stream);
int ob_ce_fwd_det_bf16(const void* logits, const void* labels, void* lse,
                       void* loss, int64_t B, int64_t Sq, int64_t V,
                       int64_t ld, void* ws, void* stream);
/* dwte[ids[r]] += dout[r], dwpe[r % Sq] += dout[r] over bf16 dout [B,Sq,H],
 * owner-computes: each position and each distinct id has one block, which
 * adds its rows in ascending row order and does one += per element.  The
 * _drop form scales by the keep mask of (seed, layer_id, site, tick, p). */
int ob_embed_bwd_det_bf16(const void* ids, const void* dout, void* dwte,
                          void* dwpe, int64_t B, int64_t Sq, int64_t H,
                          void* stream);
int ob_embed_bwd_drop_det_bf16(uint64_t seed, int32_t layer_id, int32_t site,
                               uint64_t tick, float p, const void* ids,
                               const void* dout, void* dwte, void* dwpe,
                               int64_t B, int64_t Sq, int64_t H, void* stream);
/* dst[c] += fold(part[0..nblk)[c]) for c < N over a slab with row stride ld.
 * The association depends on nblk only: group g (0..7) adds rows g, g + 8,
 * ... in ascending order, the group sums are then added in ascending g, and
 * the total is added to dst[c]. */
int ob_colpart_finish_f32(const void* part, int64_t nblk, int64_t N,
                          int64_t ld, void* dst, void* stream);

/* dtype casts (weight shadows / activation conversion). */
int ob_f32_to_bf16(const void* x, void* y, int64_t n, void* stream);
int ob_f32_to_bf16_t(const void* x, void* y, int64_t rows, int64_t cols,
                     void* stream);  /* y[c][r] = x[r][c] */
int ob_bf16_to_f32(const void* x, void* y, int64_t n, void* stream);

/* ---- in-step profiling (measurement only; off by default) ---------------
 * When enabled, each wrapped launch region inside ob_layer_forward/backward
 * and ob_adamw_step (and the clipping calls, family 10) is bracketed by HIP events on its launch stream and
 * accumulated per family, so the bench can report the production dispatch's
 * in-step per-launch time (roofline) and a per-family step-time split.
 * Families (ob_profile_read's `fam`): 0 fc_fwd_gemm (the roofline kernel),
 * 1 gemm_fwd_other, 2 gemm_dx, 3 gemm_dw(side stream), 4 flash_fwd,
 * 5 flash_bwd, 6 attn_matmuls(non-flash), 7 layernorm, 8 cross_entropy,
 * 9 elementwise(gelu/colsum/embed/dropout), 10 adamw. */
void ob_profile_enable(int on);
void ob_profile_reset(void);
int ob_profile_read(int fam, double* total_ms, long long* count);

const char* ob_last_error(void);

/* Build stamp: returns the gfx arch this library was compiled for. */
const char* ob_build_arch(void);

#ifdef __cplusplus
}
#endif
#endif /* OOBLECK_STAGE_H */
