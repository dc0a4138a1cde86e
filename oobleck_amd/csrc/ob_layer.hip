// ob_layer.hip — C-ABI layer objects for the Oobleck hot path on MI355X.
//
// One ob_layer = one fx-shard of the reference's model
// (/root/reference/oobleck/module/sharding.py:12-47): embedding, one
// transformer block, or ln_f+lm_head+loss.  Forward/backward orchestrate the
// hand-written kernels of ob_kernels.hip on the caller's hipStream_t,
// mirroring the semantics of /root/reference/oobleck/execution/layer.py
// (forward :144-145, backward :250-260 — grads ACCUMULATE into the bound
// flat grad buffer) and pipeline.py:169-244 (loss on the last layer).
//
// The activation stash is slot-indexed so several microbatches can be in
// flight, matching deepspeed-style pipe buffers (pipeline.py:556-562).
#include "ob_gemm_route.h"
#include "ob_internal.h"
#include "ob_layer_plan.h"
#include "ob_philox.h"

#include <atomic>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <vector>

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

// ---------------------------------------------------------------------------
// shared workspace (single driving thread per GPU by ABI contract)
// ---------------------------------------------------------------------------

// buffers and sizes (floats) by WS_* of ob_layer_plan.h, which says what each
// one holds and which stream owns it; grown at create, never shrunk
static struct {
  float* buf[WS_N];
  int64_t size[WS_N];
} g_ws;
// the one place a workspace buffer gets its element type
template <class T>
static T* ws(int i) { return reinterpret_cast<T*>(g_ws.buf[i]); }

// side stream + events for overlapping the weight-grad family (dW
// transposes + atomic GEMMs + bias colsums: HBM-heavy, independent of
// the dX chain) under the main stream's dX/attention work.  All
// enqueued host-side in order, so event reuse across calls is safe.
struct SideSync {
  hipStream_t stream = nullptr;
  // FRESH event per record (ring): re-recording an event that still has
  // queued waiters serializes those waiters against the future record,
  // which compounds with queue depth (the pp1-overlap stall); a 128-deep
  // ring keeps every in-flight record a distinct object.
  hipEvent_t ring[128] = {};
  int ri = 0;
  bool ready = false;
};
static SideSync g_side;

static hipEvent_t side_evt() {
  hipEvent_t e = g_side.ring[g_side.ri & 127];
  g_side.ri++;
  return e;
}

static int side_init() {
  if (g_side.ready) return 0;
  OB_HIP(hipStreamCreateWithFlags(&g_side.stream, hipStreamNonBlocking));
  for (int i = 0; i < 128; i++)
    OB_HIP(hipEventCreateWithFlags(&g_side.ring[i], hipEventDisableTiming));
  g_side.ready = true;
  return 0;
}

// record a fresh event on `from` and make `to` wait it
#define OB_SIDE_FENCE(from, to)                      \
  do {                                               \
    hipEvent_t ev_ = side_evt();                     \
    OB_HIP(hipEventRecord(ev_, (from)));             \
    OB_HIP(hipStreamWaitEvent((to), ev_, 0));        \
  } while (0)

// ---------------------------------------------------------------------------
// in-step profiler (ob_internal.h declares the family ids + OB_PROF macro).
// Ring of reusable event pairs per family: a slot being reused is first
// drained (sync + accumulate), so memory stays bounded while totals cover
// every region.  Enabled only outside bench.py's timed region.
// ---------------------------------------------------------------------------

struct ProfFam {
  static constexpr int RING = 64;
  hipEvent_t beg[RING] = {}, end[RING] = {};
  bool pending[RING] = {};
  int head = 0;
  double total_ms = 0.0;
  long long count = 0;
};
static struct {
  bool on = false;
  ProfFam fam[OB_PF_NFAM];
} g_prof;

static void prof_drain_slot(ProfFam& f, int i) {
  if (!f.pending[i]) return;
  hipEventSynchronize(f.end[i]);
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, f.beg[i], f.end[i]) == hipSuccess)
    f.total_ms += ms;
  f.pending[i] = false;
}

bool ob_prof_on() { return g_prof.on; }

int ob_prof_beg(int fam, hipStream_t s) {
  ProfFam& f = g_prof.fam[fam];
  const int i = f.head;
  if (!f.beg[i]) {
    hipEventCreate(&f.beg[i]);
    hipEventCreate(&f.end[i]);
  }
  prof_drain_slot(f, i);
  hipEventRecord(f.beg[i], s);
  return i;
}

void ob_prof_end(int fam, int slot, hipStream_t s) {
  ProfFam& f = g_prof.fam[fam];
  hipEventRecord(f.end[slot], s);
  f.pending[slot] = true;
  f.count++;
  f.head = (slot + 1) % ProfFam::RING;
}

extern "C" void ob_profile_enable(int on) { g_prof.on = on != 0; }

extern "C" void ob_profile_reset(void) {
  for (auto& f : g_prof.fam) {
    for (int i = 0; i < ProfFam::RING; i++)
      if (f.pending[i]) {
        hipEventSynchronize(f.end[i]);
        f.pending[i] = false;
      }
    f.total_ms = 0.0;
    f.count = 0;
    f.head = 0;
  }
}

extern "C" int ob_profile_read(int fam, double* total_ms, long long* count) {
  if (fam < 0 || fam >= OB_PF_NFAM) return ob_fail("profile_read: bad fam");
  ProfFam& f = g_prof.fam[fam];
  for (int i = 0; i < ProfFam::RING; i++) prof_drain_slot(f, i);
  *total_ms = f.total_ms;
  *count = f.count;
  return 0;
}

// ---------------------------------------------------------------------------
// deterministic mode (include/oobleck_stage.h): process-wide, default from
// OB_DETERMINISTIC (read once), frozen by the first layer created
// ---------------------------------------------------------------------------
// -1: not set by ob_set_deterministic, the environment's default holds
static std::atomic<int> g_det{-1};
static int64_t g_layers_created = 0;

extern "C" int ob_deterministic(void) {
  static const bool env_on = ob_env_flag("OB_DETERMINISTIC", false);
  const int v = g_det.load(std::memory_order_relaxed);
  return v < 0 ? (env_on ? 1 : 0) : v;
}

extern "C" int ob_set_deterministic(int on) {
  if (g_layers_created > 0)
    return ob_fail(
        "set_deterministic: a layer has already been created in this "
        "process; set the mode before the first layer");
  g_det.store(on != 0 ? 1 : 0, std::memory_order_relaxed);
  return 0;
}

static int ws_ensure(float** buf, int64_t* cur, int64_t need) {
  if (need <= *cur) return 0;
  if (*buf) OB_HIP(hipFree(*buf));
  *buf = nullptr;
  *cur = 0;
  OB_HIP(hipMalloc(buf, need * sizeof(float)));
  *cur = need;
  return 0;
}

// ---------------------------------------------------------------------------
// layer object
// ---------------------------------------------------------------------------

struct ob_layer {
  ob_layer_desc d;
  int B;                    // current microbatch size (<= max_batch)
  float* params = nullptr;  // caller-owned flat fp32
  float* grads = nullptr;
  // what this layer owns and shares, and where (ob_layer_plan.h)
  ob_layer_plan plan;
  // stash (extension-owned), one contiguous allocation, slot-strided.  A
  // bf16 layer keeps the fp32-sized regions and its data occupies the first
  // half of each (2x overcommit, traded for zero layout churn; memory is
  // plentiful at 288 GB).
  float* stash = nullptr;
  int64_t* ids = nullptr;   // EMBED: [n_slots, B*S]; FINAL: labels
  // bf16 mode (d.dtype == 1): weight shadows in plain + transposed layouts
  // so every GEMM operand has k contiguous in memory (see
  // ob_gemm_bf16.hip header)
  __bf16* shadows = nullptr;
  // dropout (ob_layer_create_ex); all probabilities 0 = none.  Only the
  // probabilities that apply to this layer's kind are kept.
  float p_embd = 0.f, p_resid = 0.f, p_attn = 0.f;
  int32_t layer_id = 0;
  uint64_t seed = 0;
  bool training = true;
  uint64_t next_tick = 0;
  // host-side, per slot: whether that slot's forward drew masks, and the
  // tick it used (calls are enqueued in host order, so the backward of slot
  // s reads what the forward of slot s wrote)
  std::vector<uint8_t> slot_drop;
  std::vector<uint64_t> slot_tick;
};

static bool has_dropout(const ob_layer* l) {
  return l->p_embd > 0.f || l->p_resid > 0.f || l->p_attn > 0.f;
}
static ob_drop_key drop_key(const ob_layer* l, int slot, int site, float p) {
  return ob_drop_make_key(l->seed, l->layer_id, site, l->slot_tick[slot], p);
}

// The views: the one place a stash region, a shadow or this slot's ids get
// their address and element type (T: float, or __bf16 for a bf16 layer).
template <class T>
static T* st_at(const ob_layer* l, int slot, int region) {
  return reinterpret_cast<T*>(l->stash + (int64_t)slot * l->plan.slot_stride +
                              l->plan.st_off[region]);
}
static __bf16* shadow(const ob_layer* l, int which) {
  return l->shadows + l->plan.sh_off[which];
}
static int64_t* slot_ids(const ob_layer* l, int slot) {
  return l->ids + (int64_t)slot * l->d.max_batch * l->d.seq_len;
}
template <class T>
struct BlockStash {
  T *x, *ln1, *qkv, *P, *am, *hmid, *ln2, *u, *gact;
  float *mean1, *rstd1, *mean2, *rstd2;
  float* lseP;  // a flash layer's row LSE, kept where P would be
  BlockStash(const ob_layer* l, int s)
      : x(st_at<T>(l, s, ST_X)), ln1(st_at<T>(l, s, ST_LN1)),
        qkv(st_at<T>(l, s, ST_QKV)), P(st_at<T>(l, s, ST_P)),
        am(st_at<T>(l, s, ST_ATTNM)), hmid(st_at<T>(l, s, ST_HMID)),
        ln2(st_at<T>(l, s, ST_LN2)), u(st_at<T>(l, s, ST_U)),
        gact(st_at<T>(l, s, ST_G)), mean1(st_at<float>(l, s, ST_MEAN1)),
        rstd1(st_at<float>(l, s, ST_RSTD1)),
        mean2(st_at<float>(l, s, ST_MEAN2)),
        rstd2(st_at<float>(l, s, ST_RSTD2)), lseP(st_at<float>(l, s, ST_P)) {}
};
template <class T>
struct FinalStash {
  T *x, *lnf, *logits;  // the backward turns logits into dlogits in place
  float *mean, *rstd, *lse;
  int64_t* labs;
  FinalStash(const ob_layer* l, int s)
      : x(st_at<T>(l, s, ST_X)), lnf(st_at<T>(l, s, ST_LN1)),
        logits(st_at<T>(l, s, ST_LOGITS)), mean(st_at<float>(l, s, ST_MEAN1)),
        rstd(st_at<float>(l, s, ST_RSTD1)), lse(st_at<float>(l, s, ST_LSE)),
        labs(slot_ids(l, s)) {}
};
// the backward's workspace (WS_* of ob_layer_plan.h)
template <class T>
struct BwdWs {
  T *DY4, *DLN, *DATT, *DQKV, *DP, *pd, *dm1, *dm2;
  T *QT, *KT, *dOT;  // OB_FLASH_TR=0 only
  float* D;          // flash backward's rowsum(dO * O)
  explicit BwdWs(const ob_layer* l)
      : DY4(ws<T>(WS_DY4)), DLN(ws<T>(WS_DLN)), DATT(ws<T>(WS_DATT)),
        DQKV(ws<T>(WS_DQKV)), DP(ws<T>(WS_DP)), pd(ws<T>(WS_PD_BWD)),
        dm1(ws<T>(WS_DM_ATTN)), dm2(ws<T>(WS_DM_MLP)),
        QT(ws<T>(WS_FLASH_BWD) + l->plan.pk_qt),
        KT(ws<T>(WS_FLASH_BWD) + l->plan.pk_kt),
        dOT(ws<T>(WS_FLASH_BWD) + l->plan.pk_dot),
        D(ws<float>(WS_FLASH_BWD) + l->plan.pk_d) {}
};

// The flash path reads its column-major MFMA operands from the row-major LDS
// tiles (ob_flash_*_nt_bf16): no V^T / Q^T / K^T / dO^T copies, and the
// b_qkv bias grad comes from the backward kernels' accumulators.
// OB_FLASH_TR=0 (read once) keeps the transposes + old kernels + colsum.
static bool flash_tr() {
  static const bool on = ob_env_flag("OB_FLASH_TR", true);
  return on;
}
// OB_NO_BLASLT=1 (read once) keeps every GEMM on the hand-written kernels
static bool no_blaslt() {
  static const bool on = ob_env_flag("OB_NO_BLASLT", false);
  return on;
}

// This process's modes.  OB_BF16_FLASH=0 keeps every layer on the
// materialized-P path; OB_FLASH_DROP=0 sends attn_pdrop > 0 there, and
// OB_FLASH_HD128=0 head_dim 128, as before those kernels existed
// (ob_flash_*_nt_drop_bf16, ob_flash_hd128_bf16.hip).  All read once.
static ob_layer_modes process_modes() {
  static const bool fl = ob_env_flag("OB_BF16_FLASH", true),
                    drop = ob_env_flag("OB_FLASH_DROP", true),
                    hd128 = ob_env_flag("OB_FLASH_HD128", true);
  return {ob_deterministic() != 0, fl, flash_tr(), drop, hd128};
}
static ob_layer_modes modes_of_bits(int bits) {
  if (bits < 0) return process_modes();
  return {(bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0,
          (bits & 16) != 0};
}

// the decision ob_layer_create_ex takes for `d` with this attn_pdrop; host
// only, no GPU call
extern "C" int ob_flash_eligible(const ob_layer_desc* d, float attn_pdrop) {
  return d && ob_layer_plan_of(*d, 0.f, attn_pdrop, process_modes()).flash;
}

extern "C" int ob_layer_plan_query(const ob_layer_desc* d,
                                   const ob_dropout_desc* drop, int modes,
                                   int64_t* out, int cap) {
  if (!d || (!out && cap > 0)) return -1;
  const ob_layer_plan p =
      ob_layer_plan_of(*d, drop ? drop->resid_pdrop : 0.f,
                       drop ? drop->attn_pdrop : 0.f, modes_of_bits(modes));
  if (p.error) return ob_fail("plan_query: %s", p.error), -1;
  int64_t f[OB_LAYER_PLAN_FIELDS];
  ob_layer_plan_fields(p, f);
  for (int i = 0; i < OB_LAYER_PLAN_FIELDS && i < cap; i++) out[i] = f[i];
  return OB_LAYER_PLAN_FIELDS;
}

// parameter offsets (canonical layout, oracle/gpt2_oracle.py::layer_param_spec)
struct BlockParams {
  int64_t ln1_w, ln1_b, w_qkv, b_qkv, w_attnproj, b_attnproj, ln2_w, ln2_b,
      w_fc, b_fc, w_mlpproj, b_mlpproj, total;
};
static BlockParams block_params(int64_t H) {
  BlockParams p;
  int64_t o = 0;
  p.ln1_w = o; o += H;
  p.ln1_b = o; o += H;
  p.w_qkv = o; o += H * 3 * H;
  p.b_qkv = o; o += 3 * H;
  p.w_attnproj = o; o += H * H;
  p.b_attnproj = o; o += H;
  p.ln2_w = o; o += H;
  p.ln2_b = o; o += H;
  p.w_fc = o; o += H * 4 * H;
  p.b_fc = o; o += 4 * H;
  p.w_mlpproj = o; o += 4 * H * H;
  p.b_mlpproj = o; o += H;
  p.total = o;
  return p;
}

extern "C" int64_t ob_layer_param_count(const ob_layer_desc* d) {
  const int64_t H = d->n_embd, V = d->vocab_size, P = d->n_positions;
  switch (d->kind) {
    case OB_KIND_EMBED: return V * H + P * H;
    case OB_KIND_BLOCK: return block_params(H).total;
    case OB_KIND_FINAL: return 2 * H + V * H;
  }
  return -1;
}

static void ob_layer_lt_list(const ob_layer_desc* d, bool resid_drop,
                             std::vector<ob_lt_shape>* out);

struct layer_deleter {
  void operator()(ob_layer* l) const { ob_layer_destroy(l); }
};

static int layer_create(const ob_layer_desc* d, const ob_dropout_desc* drop,
                        ob_layer_t* out) {
  if (!d || !out) return ob_fail("create: null arg");
  if (d->kind < 0 || d->kind > 2) return ob_fail("create: bad kind");
  if (d->seq_len > 2048)
    return ob_fail("create: seq_len > 2048 unsupported in round 1");
  if (d->n_slots < 1) return ob_fail("create: n_slots < 1");
  const bool det = ob_deterministic() != 0;
  if (det && d->dtype != 1)
    return ob_fail(
        "create: fp32 layers (dtype 0) are not supported in deterministic "
        "mode (OB_DETERMINISTIC=1 / ob_set_deterministic): their kernels "
        "still sum with atomics");
  if (drop) {
    if (!ob_drop_p_ok(drop->embd_pdrop) || !ob_drop_p_ok(drop->resid_pdrop) ||
        !ob_drop_p_ok(drop->attn_pdrop))
      return ob_fail("create_ex: dropout probabilities must be in [0,1)");
    if (drop->layer_id < 0 || drop->layer_id >= (1 << 24))
      return ob_fail("create_ex: layer_id out of range");
  }
  // every failure from here on frees what the layer took so far
  std::unique_ptr<ob_layer, layer_deleter> guard(new ob_layer());
  ob_layer* const l = guard.get();
  l->d = *d;
  l->B = d->max_batch;
  l->slot_drop.assign(d->n_slots, 0);
  l->slot_tick.assign(d->n_slots, 0);
  if (drop) {
    if (d->kind == OB_KIND_EMBED) l->p_embd = drop->embd_pdrop;
    if (d->kind == OB_KIND_BLOCK) {
      l->p_resid = drop->resid_pdrop;
      l->p_attn = drop->attn_pdrop;
    }
    l->layer_id = drop->layer_id;
    l->seed = drop->seed;
  }
  const ob_layer_plan& pl = l->plan =
      ob_layer_plan_of(*d, l->p_resid, l->p_attn, process_modes());
  if (pl.error) return ob_fail("create: %s", pl.error);
  if (pl.slot_stride > 0 &&
      hipMalloc(&l->stash, (size_t)pl.slot_stride * d->n_slots *
                               sizeof(float)) != hipSuccess)
    return ob_fail("create: stash hipMalloc of %lld floats failed",
                   (long long)(pl.slot_stride * d->n_slots));
  if (pl.ids_count > 0 &&
      hipMalloc(&l->ids, (size_t)pl.ids_count * sizeof(int64_t)) !=
          hipSuccess)
    return ob_fail("create: ids hipMalloc failed");
  if (pl.shadow_count > 0) {
    if (hipMalloc(&l->shadows, (size_t)pl.shadow_count * sizeof(__bf16)) !=
        hipSuccess)
      return ob_fail("create: shadow hipMalloc failed");
    OB_HIP(hipMemset(l->shadows, 0, (size_t)pl.shadow_count * sizeof(__bf16)));
  }
  // grow the shared workspace to this layer's needs
  for (int i = 0; i < WS_N; i++)
    if (ws_ensure(&g_ws.buf[i], &g_ws.size[i], pl.ws[i])) return 1;
  if (pl.side && side_init()) return 1;
  // pick the library GEMMs' solutions by measurement, once per shape and
  // process (ob_blaslt.hip; a no-op with OB_LT_TUNE=0 and in deterministic
  // mode, where every plan is the heuristic's top-1)
  if (!no_blaslt()) {
    std::vector<ob_lt_shape> shapes;
    ob_layer_lt_list(d, l->p_resid > 0.f, &shapes);
    // a BLOCK's weight grads may run sliced along K with WS_DW_A as the slab
    const int64_t slab = d->kind == OB_KIND_BLOCK ? pl.ws[WS_DW_A] : 0;
    for (const ob_lt_shape& s : shapes)
      if (ob_lt_tune_shape(s, s.tA ? slab : 0)) return 1;
  }
  g_layers_created++;
  *out = guard.release();
  return 0;
}

extern "C" int ob_layer_create(const ob_layer_desc* d, ob_layer_t* out) {
  return layer_create(d, nullptr, out);
}

extern "C" int ob_layer_create_ex(const ob_layer_desc* d,
                                  const ob_dropout_desc* drop,
                                  ob_layer_t* out) {
  return layer_create(d, drop, out);
}

extern "C" int ob_layer_uses_flash(ob_layer_t l) {
  return l && l->plan.flash ? 1 : 0;
}

extern "C" int ob_layer_set_training(ob_layer_t l, int on) {
  if (!l) return ob_fail("set_training: null layer");
  l->training = on != 0;
  return 0;
}

extern "C" int ob_layer_set_dropout_tick(ob_layer_t l, uint64_t tick) {
  if (!l) return ob_fail("set_dropout_tick: null layer");
  l->next_tick = tick;
  return 0;
}

extern "C" int ob_layer_bind(ob_layer_t l, void* params, void* grads) {
  if (!l) return ob_fail("bind: null layer");
  l->params = (float*)params;
  l->grads = (float*)grads;
  return 0;
}

extern "C" int ob_layer_set_batch(ob_layer_t l, int32_t batch) {
  if (!l) return ob_fail("set_batch: null layer");
  if (batch < 1 || batch > l->d.max_batch)
    return ob_fail("set_batch: %d out of range (max %d)", batch,
                   l->d.max_batch);
  l->B = batch;
  return 0;
}

extern "C" int ob_layer_destroy(ob_layer_t l) {
  if (!l) return 0;
  if (l->stash) hipFree(l->stash);
  if (l->ids) hipFree(l->ids);
  if (l->shadows) hipFree(l->shadows);
  delete l;
  return 0;
}

extern "C" int ob_layer_refresh_weights(ob_layer_t l, void* stream) {
  if (!l) return ob_fail("refresh: null layer");
  if (l->d.dtype != 1) return 0;  // fp32 mode: nothing to do
  if (!l->params) return ob_fail("refresh: params not bound");
  const int64_t H = l->d.n_embd, V = l->d.vocab_size;
  const float* p = l->params;
  switch (l->d.kind) {
    case OB_KIND_EMBED:
      return 0;  // embedding reads the fp32 master directly
    case OB_KIND_BLOCK: {
      const BlockParams bp = block_params(H);
      if (ob_f32_to_bf16(p + bp.w_qkv, shadow(l, SH_QKV), 3 * H * H, stream) ||
          ob_f32_to_bf16_t_ld(p + bp.w_qkv, shadow(l, SH_QKV_T), H, 3 * H, H,
                              stream) ||
          ob_f32_to_bf16(p + bp.w_attnproj, shadow(l, SH_AP), H * H, stream) ||
          ob_f32_to_bf16_t_ld(p + bp.w_attnproj, shadow(l, SH_AP_T), H, H, H,
                              stream) ||
          ob_f32_to_bf16(p + bp.w_fc, shadow(l, SH_FC), 4 * H * H, stream) ||
          ob_f32_to_bf16_t_ld(p + bp.w_fc, shadow(l, SH_FC_T), H, 4 * H, H,
                              stream) ||
          ob_f32_to_bf16(p + bp.w_mlpproj, shadow(l, SH_MP), 4 * H * H,
                         stream) ||
          ob_f32_to_bf16_t_ld(p + bp.w_mlpproj, shadow(l, SH_MP_T), 4 * H, H,
                              4 * H, stream))
        return 1;
      return 0;
    }
    case OB_KIND_FINAL:
      if (ob_f32_to_bf16(p + 2 * H, shadow(l, SH_LM), V * H, stream) ||
          ob_f32_to_bf16_t_ld(p + 2 * H, shadow(l, SH_LM_T), V, H,
                              l->plan.v_pad, stream))
        return 1;
      return 0;
  }
  return ob_fail("refresh: bad kind");
}

// helper: plain strided-batch GEMM call (n1=batch, n2=1) or 2-level.
static int gemm(int tA, int tB, int64_t M, int64_t N, int64_t K, float alpha,
                const float* A, int64_t lda, int64_t sA1, int64_t sA2,
                const float* B, int64_t ldb, int64_t sB1, int64_t sB2,
                float beta, float* C, int64_t ldc, int64_t sC1, int64_t sC2,
                int64_t n1, int64_t n2, const float* bias, const float* R,
                int atomic, int splitk, void* stream) {
  // plain (unbatched, no fused epilogue) fp32 GEMMs to hipBLASLt —
  // covers the dW family too (it accumulates through beta=1)
  if (!no_blaslt() && !bias && !R && !atomic && splitk <= 1 && n1 == 1 &&
      n2 == 1 && M * N >= 512 * 512) {
    const int r = ob_gemm_lt_f32(tA, tB, M, N, K, alpha, A, lda, B, ldb,
                                 beta, C, ldc, stream);
    if (r >= 0) return r;
  }
  return ob_gemm_f32(tA, tB, M, N, K, alpha, A, lda, sA1, sA2, B, ldb, sB1,
                     sB2, beta, C, ldc, sC1, sC2, n1, n2, bias, R, atomic,
                     splitk, stream);
}

// pick a split-K factor for weight-grad GEMMs so the grid fills the chip
// (256 CUs want >= ~512 blocks of 128x128).
static int pick_splitk(int64_t M, int64_t N, int64_t K) {
  const int64_t tiles = ((M + 127) / 128) * ((N + 127) / 128);
  int sk = 1;
  while (sk < 16 && tiles * sk < 512 && (K / (sk * 2)) >= 256) sk *= 2;
  return sk;
}

// narrow-N activation-grad GEMMs (dX = dY @ W^T with N = H): only
// M/128 x H/128 tiles -> the chip is underfilled and the long-K loop is
// latency-bound (measured 57 TF at K=50257 vs 105+ on wide shapes).
// Zero the output and split K across atomicAdd slices instead.
static int gemm_dx_splitk(int tB, int64_t M, int64_t N, int64_t K,
                          float alpha, const float* A, int64_t lda,
                          const float* B, int64_t ldb, float* C, int64_t ldc,
                          void* stream) {
  if (!no_blaslt()) {
    const int r = ob_gemm_lt_f32(0, tB, M, N, K, alpha, A, lda, B, ldb, 0.f,
                                 C, ldc, stream);
    if (r >= 0) return r;
  }
  const int64_t tiles = ((M + 127) / 128) * ((N + 127) / 128);
  int sk = 1;
  while (sk < 16 && tiles * sk < 1024 && (K / (sk * 2)) >= 512) sk *= 2;
  if (sk == 1)
    return ob_gemm_f32(0, tB, M, N, K, alpha, A, lda, 0, 0, B, ldb, 0, 0,
                       0.f, C, ldc, 0, 0, 1, 1, nullptr, nullptr, 0, 1,
                       stream);
  OB_HIP(hipMemsetAsync(C, 0, (size_t)M * ldc * sizeof(float), S(stream)));
  return ob_gemm_f32(0, tB, M, N, K, alpha, A, lda, 0, 0, B, ldb, 0, 0, 0.f,
                     C, ldc, 0, 0, 1, 1, nullptr, nullptr, 1, sk, stream);
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------

static int block_forward(ob_layer* l, int slot, const float* in, float* out,
                         void* stream) {
  const int64_t Sq = l->d.seq_len, H = l->d.n_embd, nh = l->d.n_head;
  const int64_t B = l->B, BS = B * Sq;
  const int64_t hd = H / nh;
  const float* p = l->params;
  const BlockStash<float> s(l, slot);
  const BlockParams bp = block_params(H);
  const bool dA = l->slot_drop[slot] && l->p_attn > 0.f;
  const bool dR = l->slot_drop[slot] && l->p_resid > 0.f;

  OB_HIP(hipMemcpyAsync(s.x, in, BS * H * sizeof(float),
                        hipMemcpyDeviceToDevice, S(stream)));
  if (ob_layernorm_fwd_f32(s.x, p + bp.ln1_w, p + bp.ln1_b, s.ln1, s.mean1,
                           s.rstd1, BS, H, 1e-5f, stream))
    return 1;
  if (gemm(0, 0, BS, 3 * H, H, 1.f, s.ln1, H, 0, 0, p + bp.w_qkv, 3 * H, 0, 0,
           0.f, s.qkv, 3 * H, 0, 0, 1, 1, p + bp.b_qkv, nullptr, 0, 1, stream))
    return 1;
  // scores: P[b,h] = Q @ K^T ; Q/K are strided slices of qkv
  if (gemm(0, 1, Sq, Sq, hd, 1.f,
           s.qkv, 3 * H, Sq * 3 * H, hd,            // Q slice
           s.qkv + H, 3 * H, Sq * 3 * H, hd,        // K slice (stored [S,hd])
           0.f, s.P, Sq, nh * Sq * Sq, Sq * Sq, B, nh, nullptr, nullptr, 0, 1,
           stream))
    return 1;
  if (ob_softmax_causal_fwd_f32(s.P, B * nh, Sq, 1.f / sqrtf((float)hd),
                                stream))
    return 1;
  // attention dropout: the stash keeps the undropped P (softmax backward
  // needs it at dropped positions); the PV GEMM reads Pd = drop(P) from the
  // forward-only workspace
  const float* Pv = s.P;
  if (dA) {
    if (ob_drop_scale(drop_key(l, slot, OB_DROP_ATTN, l->p_attn), 0, s.P,
                      ws<float>(WS_PD_FWD), B * nh * Sq * Sq, stream))
      return 1;
    Pv = ws<float>(WS_PD_FWD);
  }
  // attn_merged[b,:,h*hd:(h+1)*hd] = Pd[b,h] @ V[b,h]
  if (gemm(0, 0, Sq, hd, Sq, 1.f, Pv, Sq, nh * Sq * Sq, Sq * Sq, s.qkv + 2 * H,
           3 * H, Sq * 3 * H, hd, 0.f, s.am, H, Sq * H, hd, B, nh, nullptr,
           nullptr, 0, 1, stream))
    return 1;
  // h_mid = attn_merged @ w_attnproj + b + x (residual)
  if (gemm(0, 0, BS, H, H, 1.f, s.am, H, 0, 0, p + bp.w_attnproj, H, 0, 0, 0.f,
           s.hmid, H, 0, 0, 1, 1, p + bp.b_attnproj, dR ? nullptr : s.x, 0, 1,
           stream))
    return 1;
  // residual dropout: the GEMM wrote the biased projection only
  if (dR && ob_drop_add(drop_key(l, slot, OB_DROP_RESID_ATTN, l->p_resid), 0,
                        s.hmid, s.x, s.hmid, BS * H, stream))
    return 1;
  if (ob_layernorm_fwd_f32(s.hmid, p + bp.ln2_w, p + bp.ln2_b, s.ln2, s.mean2,
                           s.rstd2, BS, H, 1e-5f, stream))
    return 1;
  if (gemm(0, 0, BS, 4 * H, H, 1.f, s.ln2, H, 0, 0, p + bp.w_fc, 4 * H, 0, 0,
           0.f, s.u, 4 * H, 0, 0, 1, 1, p + bp.b_fc, nullptr, 0, 1, stream))
    return 1;
  if (ob_gelu_fwd_f32(s.u, s.gact, BS * 4 * H, stream)) return 1;
  if (gemm(0, 0, BS, H, 4 * H, 1.f, s.gact, 4 * H, 0, 0, p + bp.w_mlpproj, H, 0,
           0, 0.f, out, H, 0, 0, 1, 1, p + bp.b_mlpproj, dR ? nullptr : s.hmid,
           0, 1, stream))
    return 1;
  if (dR && ob_drop_add(drop_key(l, slot, OB_DROP_RESID_MLP, l->p_resid), 0,
                        out, s.hmid, out, BS * H, stream))
    return 1;
  return 0;
}

static int final_forward(ob_layer* l, int slot, const float* in, float* out,
                         const int64_t* labels, void* stream) {
  const int64_t Sq = l->d.seq_len, H = l->d.n_embd, V = l->d.vocab_size;
  const int64_t B = l->B, BS = B * Sq;
  const float* p = l->params;
  const FinalStash<float> s(l, slot);
  if (!labels) return ob_fail("final_forward: labels required");

  OB_HIP(hipMemcpyAsync(s.x, in, BS * H * sizeof(float),
                        hipMemcpyDeviceToDevice, S(stream)));
  OB_HIP(hipMemcpyAsync(s.labs, labels, BS * sizeof(int64_t),
                        hipMemcpyDeviceToDevice, S(stream)));
  if (ob_layernorm_fwd_f32(s.x, p + 0, p + H, s.lnf, s.mean, s.rstd, BS, H,
                           1e-5f, stream))
    return 1;
  // logits = ln_out @ w_lm^T   (w_lm stored [V,H])
  if (gemm(0, 1, BS, V, H, 1.f, s.lnf, H, 0, 0, p + 2 * H, H, 0, 0, 0.f,
           s.logits, V, 0, 0, 1, 1, nullptr, nullptr, 0, 1, stream))
    return 1;
  OB_HIP(hipMemsetAsync(out, 0, sizeof(float), S(stream)));
  return ob_ce_fwd_f32(s.logits, s.labs, s.lse, out, B, Sq, V, stream);
}

// ---------------------------------------------------------------------------
// bf16 mixed-precision path (d.dtype == 1): bf16 activations + bf16 MFMA
// GEMMs with fp32 accumulate, fp32 master weights/biases/LN params, fp32
// grads.  Weight operands come from the plain/transposed shadows so every
// GEMM stages its operands with k contiguous (see ob_gemm_bf16.hip).
// ---------------------------------------------------------------------------

// ---------------------------------------------------------------------------
// The layer's unbatched GEMMs, the SOLE list of them: the forward and
// backward below take every such call's dimensions from here, and
// ob_layer_lt_list hands the same shapes to the hipBLASLt tuner at create
// time, so the tuned keys and the keys the step uses cannot drift apart.
enum {
  LG_QKV = 0, LG_AP, LG_FC, LG_MP,              // forward, bias (+ residual)
  LG_DX_MP, LG_DX_FC, LG_DX_AP, LG_DX_QKV,      // activation grads
  LG_DW_MP, LG_DW_FC, LG_DW_AP, LG_DW_QKV,      // weight grads, TN beta=1
  LG_BLOCK_N
};
enum { LG_LM = 0, LG_DLNOUT, LG_DW_LM, LG_FINAL_N };

// res: the two projections fold their residual (false under residual dropout)
static void block_gemms(int64_t H, int64_t BS, bool res, ob_lt_shape* g) {
  g[LG_QKV] = ob_lt_linear(BS, H, 3 * H, true, false);
  g[LG_AP] = ob_lt_linear(BS, H, H, true, res);
  g[LG_FC] = ob_lt_linear(BS, H, 4 * H, true, false);
  g[LG_MP] = ob_lt_linear(BS, 4 * H, H, true, res);
  g[LG_DX_MP] = ob_lt_linear(BS, H, 4 * H, false, false);
  g[LG_DX_FC] = ob_lt_linear(BS, 4 * H, H, false, false);
  g[LG_DX_AP] = ob_lt_linear(BS, H, H, false, false);
  g[LG_DX_QKV] = ob_lt_linear(BS, 3 * H, H, false, false);
  g[LG_DW_MP] = ob_lt_dw(4 * H, H, BS, 4 * H);
  g[LG_DW_FC] = ob_lt_dw(H, 4 * H, BS, H);
  g[LG_DW_AP] = ob_lt_dw(H, H, BS, H);
  g[LG_DW_QKV] = ob_lt_dw(H, 3 * H, BS, H);
}

// lm_head N = v_pad, d_lnout K = v_pad, dW_lm M = V over v_pad-wide rows
static void final_gemms(int64_t H, int64_t V, int64_t v_pad, int64_t BS,
                        ob_lt_shape* g) {
  g[LG_LM] = ob_lt_linear(BS, H, v_pad, false, false);
  g[LG_DLNOUT] = ob_lt_linear(BS, v_pad, H, false, false);
  g[LG_DW_LM] = ob_lt_dw(V, H, BS, v_pad);
}

// does the step offer this shape to hipBLASLt?  A linear goes by the bf16
// route rule; a weight grad always does.
static bool lt_routed(const ob_lt_shape& s) {
  if (s.tA) return true;
  const ob_gemm_env env = {false, false, false, nullptr};
  return ob_gemm_bf16_pick(0, 1, s.M, s.N, s.K, 1, 1, BF_OUT_BF16, 1, 0.f,
                           true, env)
      .try_lt_first;
}

// host-only: the library GEMM shapes of a layer at M = max_batch * seq_len.
// resid_drop adds the projections' residual-free form (training forwards
// under residual dropout) beside the folded one (eval forwards).
static void ob_layer_lt_list(const ob_layer_desc* d, bool resid_drop,
                             std::vector<ob_lt_shape>* out) {
  if (d->dtype != 1) return;
  const int64_t H = d->n_embd, V = d->vocab_size;
  const int64_t BS = (int64_t)d->max_batch * d->seq_len;
  ob_lt_shape g[LG_BLOCK_N];
  int n = 0;
  if (d->kind == OB_KIND_BLOCK) {
    block_gemms(H, BS, true, g);
    n = LG_BLOCK_N;
  } else if (d->kind == OB_KIND_FINAL) {
    final_gemms(H, V, ob_v_pad(V), BS, g);
    n = LG_FINAL_N;
  }
  for (int i = 0; i < n; i++)
    if (lt_routed(g[i])) out->push_back(g[i]);
  if (d->kind == OB_KIND_BLOCK && resid_drop) {
    block_gemms(H, BS, false, g);
    for (int i : {LG_AP, LG_MP})
      if (lt_routed(g[i])) out->push_back(g[i]);
  }
}

extern "C" int ob_layer_lt_shapes(const ob_layer_desc* d, int64_t* out,
                                  int cap) {
  if (!d || (!out && cap > 0)) return -1;
  std::vector<ob_lt_shape> v;
  ob_layer_lt_list(d, false, &v);
  for (int i = 0; i < (int)v.size() && i < cap; i++) {
    const ob_lt_shape& s = v[i];
    int64_t* o = out + (int64_t)i * OB_LT_SHAPE_FIELDS;
    o[0] = s.tA, o[1] = s.tB, o[2] = s.M, o[3] = s.N, o[4] = s.K;
    o[5] = s.lda, o[6] = s.ldb, o[7] = s.ldc, o[8] = s.c_f32, o[9] = s.beta1;
    o[10] = s.bias, o[11] = s.cin, o[12] = s.ab_f32;
  }
  return (int)v.size();
}

// unbatched NT linear, bf16 out: out[M,N] = in[M,K] @ W[N,K]^T (+ bias)
// (+ res).  The forward projections, the dX GEMMs, lm_head and d_lnout.
static int linear_bf(const ob_lt_shape& s, const void* in, const void* W,
                     const float* bias, const void* res, void* out,
                     void* stream) {
  if ((bias != nullptr) != (s.bias != 0) || (res != nullptr) != (s.cin != 0))
    return ob_fail("linear_bf: operands do not match the listed shape");
  ob_bf16_gemm g;
  g.A = in, g.B = W, g.C = out, g.bias = bias, g.residual = res;
  g.M = s.M, g.N = s.N, g.K = s.K, g.lda = s.lda, g.ldb = s.ldb;
  g.ldc = s.ldc, g.stream = stream;
  return ob_gemm_bf16_run(g);
}

// the non-flash attention matmuls: one [M,K] x [K,N] product per (batch,
// head); the caller names the three operands' leading dims and strides
static ob_bf16_gemm attn_gemm(int tA, int tB, int64_t M, int64_t N, int64_t K,
                              float alpha, int64_t B, int64_t nh,
                              void* stream) {
  ob_bf16_gemm g;
  g.transA = tA, g.transB = tB, g.M = M, g.N = N, g.K = K, g.alpha = alpha;
  g.n1 = B, g.n2 = nh, g.stream = stream;
  return g;
}

// weight-grad GEMM for bf16: materialize X^T / dY^T (cheap HBM transpose)
// so the GEMM runs on the fast NT glds path instead of the
// transpose-staged TN case (~150 TF measured there).
static int dw_bf16_ws(const ob_lt_shape& s, const __bf16* act,
                      const __bf16* dY, float* gout, void* stream) {
  const int64_t actw = s.M, dyw = s.N, BS = s.K, ldc = s.ldc;
  // direct TN via hipBLASLt with beta=1 accumulation into the fp32 flat
  // grads: no transpose materialization, no atomics (measured 694 TF on
  // the fc dW shape vs 436 for transpose + atomic NT)
  // the 128x128 tiles of a block's dW outputs cover 36 to 144 of 256 CUs, so
  // where the tuner measured it faster the call runs as K-slices into
  // WS_DW_A (idle on this path) and a fold (ob_dw_slices.h)
  if (!no_blaslt()) {
    const int r = ob_lt_dw_run(s, act, dY, gout, ws<float>(WS_DW_A),
                               g_ws.size[WS_DW_A], stream);
    if (r >= 0) return r;
  }
  // gout[actw,dyw] += act^T dY, atomically, K = BS split to fill the chip
  ob_bf16_gemm g;
  g.C = gout, g.M = actw, g.N = dyw, g.K = BS, g.ldc = ldc;
  // deterministic mode: one adder per element per launch (split-K 1)
  g.out_kind = 2, g.stream = stream;
  g.splitk = ob_deterministic() ? 1 : pick_splitk(actw, dyw, BS);
  if ((actw % 128) || (dyw % 128) || (BS % 128)) {
    g.transA = 1, g.transB = 0;
    g.A = act, g.lda = actw, g.B = dY, g.ldb = dyw;
    return ob_gemm_bf16_run(g);
  }
  __bf16* XT = ws<__bf16>(WS_DW_A);
  __bf16* DYT = ws<__bf16>(WS_DW_B);
  if (ob_transpose_bf16(act, XT, BS, actw, stream)) return 1;
  if (ob_transpose_bf16(dY, DYT, BS, dyw, stream)) return 1;
  g.A = XT, g.lda = BS, g.B = DYT, g.ldb = BS;
  return ob_gemm_bf16_run(g);
}

static int block_forward_bf16(ob_layer* l, int slot, const __bf16* in,
                              __bf16* out, void* stream) {
  const int64_t Sq = l->d.seq_len, H = l->d.n_embd, nh = l->d.n_head;
  const int64_t B = l->B, BS = B * Sq;
  const int64_t hd = H / nh;
  const float* p = l->params;
  const BlockStash<__bf16> s(l, slot);
  const BlockParams bp = block_params(H);
  const bool dA = l->slot_drop[slot] && l->p_attn > 0.f;
  const bool dR = l->slot_drop[slot] && l->p_resid > 0.f;
  ob_lt_shape lg[LG_BLOCK_N];
  block_gemms(H, BS, !dR, lg);

  // ln1 reads the input once and also writes its stash copy x
  if (OB_PROF(OB_PF_LN, stream,
              ob_layernorm_fwd_copy_bf16(in, p + bp.ln1_w, p + bp.ln1_b, s.ln1,
                                         s.x, s.mean1, s.rstd1, BS, H, 1e-5f,
                                         stream)))
    return 1;
  if (OB_PROF(OB_PF_GEMM_FWD, stream,
              linear_bf(lg[LG_QKV], s.ln1, shadow(l, SH_QKV_T), p + bp.b_qkv,
                        nullptr, s.qkv, stream)))
    return 1;
  if (l->plan.flash && flash_tr()) {
    // the fused kernel writes O and the per-row LSE (stored where the
    // materialized-P path keeps P)
    if (dA) {
      // attention dropout inside the kernel: masks of this slot's tick
      if (OB_PROF(OB_PF_FLASH_FWD, stream,
                  ob_flash_fwd_nt_drop_bf16(s.qkv, s.am, s.lseP, B, Sq, H, nh,
                                            1.f / sqrtf((float)hd), l->seed,
                                            l->layer_id, l->slot_tick[slot],
                                            l->p_attn, stream)))
        return 1;
    } else if (OB_PROF(OB_PF_FLASH_FWD, stream,
                       ob_flash_fwd_nt_bf16(s.qkv, s.am, s.lseP, B, Sq, H, nh,
                                            1.f / sqrtf((float)hd), stream)))
      return 1;
  } else if (l->plan.flash) {
    // OB_FLASH_TR=0: V^T materialization (workspace, transient within this
    // call) feeding the kernel that takes a transposed V
    __bf16* VTw = ws<__bf16>(WS_FLASH_VT);
    if (OB_PROF(OB_PF_FLASH_FWD, stream,
                ob_transpose_bf16_b(s.qkv + 2 * H, VTw, Sq, 64, Sq * 3 * H, 64,
                                    3 * H, B, nh, stream)))
      return 1;
    if (OB_PROF(OB_PF_FLASH_FWD, stream,
                ob_flash_fwd_bf16(s.qkv, VTw, s.am, s.lseP, B, Sq, H, nh,
                                  1.f / sqrtf((float)hd), stream)))
      return 1;
  } else {
    ob_bf16_gemm qk = attn_gemm(0, 1, Sq, Sq, hd, 1.f, B, nh, stream);
    qk.A = s.qkv, qk.lda = 3 * H, qk.sA1 = Sq * 3 * H, qk.sA2 = hd;
    qk.B = s.qkv + H, qk.ldb = 3 * H, qk.sB1 = Sq * 3 * H, qk.sB2 = hd;
    qk.C = s.P, qk.ldc = Sq, qk.sC1 = nh * Sq * Sq, qk.sC2 = Sq * Sq;
    if (OB_PROF(OB_PF_ATTN_MAT, stream, ob_gemm_bf16_run(qk))) return 1;
    if (OB_PROF(OB_PF_ATTN_MAT, stream,
                ob_softmax_causal_fwd_bf16(s.P, B * nh, Sq,
                                           1.f / sqrtf((float)hd), stream)))
      return 1;
    // attention dropout: stash keeps P, the PV GEMM reads Pd = drop(P) from
    // the forward-only workspace (only a non-flash layer gets here with dA)
    const __bf16* Pv = s.P;
    if (dA) {
      if (OB_PROF(OB_PF_ELEM, stream,
                  ob_drop_scale(drop_key(l, slot, OB_DROP_ATTN, l->p_attn), 1,
                                s.P, ws<__bf16>(WS_PD_FWD), B * nh * Sq * Sq,
                                stream)))
        return 1;
      Pv = ws<__bf16>(WS_PD_FWD);
    }
    ob_bf16_gemm pv = attn_gemm(0, 0, Sq, hd, Sq, 1.f, B, nh, stream);
    pv.A = Pv, pv.lda = Sq, pv.sA1 = nh * Sq * Sq, pv.sA2 = Sq * Sq;
    pv.B = s.qkv + 2 * H, pv.ldb = 3 * H, pv.sB1 = Sq * 3 * H, pv.sB2 = hd;
    pv.C = s.am, pv.ldc = H, pv.sC1 = Sq * H, pv.sC2 = hd;
    if (OB_PROF(OB_PF_ATTN_MAT, stream, ob_gemm_bf16_run(pv))) return 1;
  }
  if (OB_PROF(OB_PF_GEMM_FWD, stream,
              linear_bf(lg[LG_AP], s.am, shadow(l, SH_AP_T), p + bp.b_attnproj,
                        dR ? nullptr : s.x, s.hmid, stream)))
    return 1;
  // residual dropout: the GEMM wrote the biased projection only
  if (dR &&
      OB_PROF(OB_PF_ELEM, stream,
              ob_drop_add(drop_key(l, slot, OB_DROP_RESID_ATTN, l->p_resid), 1,
                          s.hmid, s.x, s.hmid, BS * H, stream)))
    return 1;
  if (OB_PROF(OB_PF_LN, stream,
              ob_layernorm_fwd_bf16(s.hmid, p + bp.ln2_w, p + bp.ln2_b, s.ln2,
                                    s.mean2, s.rstd2, BS, H, 1e-5f, stream)))
    return 1;
  if (OB_PROF(OB_PF_FC_FWD, stream,
              linear_bf(lg[LG_FC], s.ln2, shadow(l, SH_FC_T), p + bp.b_fc,
                        nullptr, s.u, stream)))
    return 1;
  if (OB_PROF(OB_PF_ELEM, stream,
              ob_gelu_fwd_bf16(s.u, s.gact, BS * 4 * H, stream)))
    return 1;
  if (OB_PROF(OB_PF_GEMM_FWD, stream,
              linear_bf(lg[LG_MP], s.gact, shadow(l, SH_MP_T),
                        p + bp.b_mlpproj, dR ? nullptr : s.hmid, out, stream)))
    return 1;
  if (dR &&
      OB_PROF(OB_PF_ELEM, stream,
              ob_drop_add(drop_key(l, slot, OB_DROP_RESID_MLP, l->p_resid), 1,
                          out, s.hmid, out, BS * H, stream)))
    return 1;
  return 0;
}

static int final_forward_bf16(ob_layer* l, int slot, const __bf16* in,
                              float* out, const int64_t* labels,
                              void* stream) {
  const int64_t Sq = l->d.seq_len, H = l->d.n_embd, V = l->d.vocab_size;
  const int64_t B = l->B, BS = B * Sq;
  const float* p = l->params;
  const FinalStash<__bf16> s(l, slot);
  if (!labels) return ob_fail("final_forward_bf16: labels required");
  ob_lt_shape lg[LG_FINAL_N];
  final_gemms(H, V, l->plan.v_pad, BS, lg);

  OB_HIP(hipMemcpyAsync(s.labs, labels, BS * sizeof(int64_t),
                        hipMemcpyDeviceToDevice, S(stream)));
  if (OB_PROF(OB_PF_LN, stream,
              ob_layernorm_fwd_copy_bf16(in, p + 0, p + H, s.lnf, s.x, s.mean,
                                         s.rstd, BS, H, 1e-5f, stream)))
    return 1;
  // N = v_pad (zero-padded shadow rows -> padded logits are exactly 0)
  if (OB_PROF(OB_PF_GEMM_FWD, stream,
              linear_bf(lg[LG_LM], s.lnf, shadow(l, SH_LM), nullptr, nullptr,
                        s.logits, stream)))
    return 1;
  OB_HIP(hipMemsetAsync(out, 0, sizeof(float), S(stream)));
  // deterministic mode: the loss through the forward stream's slab
  float* const wsf = ob_deterministic() ? ws<float>(WS_DET_FWD) : nullptr;
  return OB_PROF(OB_PF_CE, stream,
                 ob_ce_fwd_ws(s.logits, s.labs, s.lse, out, B, Sq, V,
                              l->plan.v_pad, wsf, stream));
}

static int block_backward_bf16(ob_layer* l, int slot, const __bf16* dout,
                               __bf16* din, void* stream) {
  const int64_t Sq = l->d.seq_len, H = l->d.n_embd, nh = l->d.n_head;
  const int64_t B = l->B, BS = B * Sq;
  const int64_t hd = H / nh;
  const float scale = 1.f / sqrtf((float)hd);
  const float* p = l->params;
  const BlockStash<__bf16> s(l, slot);
  const BwdWs<__bf16> w(l);
  float* g = l->grads;
  const BlockParams bp = block_params(H);
  // the masks this slot's forward drew, regenerated from its tick
  const bool dA = l->slot_drop[slot] && l->p_attn > 0.f;
  const bool dR = l->slot_drop[slot] && l->p_resid > 0.f;
  ob_lt_shape lg[LG_BLOCK_N];
  block_gemms(H, BS, !dR, lg);
  // deterministic mode: the same calls, same places, same streams, with
  // the stream's slab (null: the atomic kernels)
  const bool det = ob_deterministic() != 0;
  float* const wsm = det ? ws<float>(WS_DET_MAIN) : nullptr;

  // The dW family (transposes + atomic GEMMs + the qkv bias colsum) has
  // no consumer inside this call and no effect on the dX chain (the other
  // three bias grads are side sums of the main-stream gelu / ln2 backward
  // kernels): it runs on
  // g_side, overlapped under the dX/attention work, fenced by events at
  // the producer edges and JOINED at the end of the call (the g_ws
  // buffers it reads are reused by the next microbatch's backward).
  void* const side = (void*)g_side.stream;
  OB_SIDE_FENCE(S(stream), g_side.stream);  // entry state (dout ready)

  // ---- MLP ----
  // residual dropout: the projection saw mask*dout; that kernel also takes
  // the b_mlpproj grad.  The residual branch (ln2 backward) keeps dout.
  const __bf16* dmlp = dout;
  if (dR) {
    if (OB_PROF(OB_PF_ELEM, stream,
                ob_drop_scale_colsum(
                    drop_key(l, slot, OB_DROP_RESID_MLP, l->p_resid), 1, dout,
                    w.dm2, g + bp.b_mlpproj, BS, H, stream, wsm)))
      return 1;
    dmlp = w.dm2;
    OB_SIDE_FENCE(S(stream), g_side.stream);  // dm2 ready
  }
  if (OB_PROF(OB_PF_GEMM_DX, stream,
              linear_bf(lg[LG_DX_MP], dmlp, shadow(l, SH_MP), nullptr, nullptr,
                        w.DY4, stream)))
    return 1;
  if (OB_PROF(OB_PF_GEMM_DW, side,
              dw_bf16_ws(lg[LG_DW_MP], s.gact, dmlp, g + bp.w_mlpproj, side)))
    return 1;
  // gelu backward also sums its output columns into the b_fc grad
  if (OB_PROF(OB_PF_ELEM, stream,
              ob_gelu_bwd_colsum_ws(s.u, w.DY4, w.DY4, g + bp.b_fc, BS, 4 * H,
                                    wsm, stream)))
    return 1;
  OB_SIDE_FENCE(S(stream), g_side.stream);  // DY4 post-gelu
  if (OB_PROF(OB_PF_GEMM_DW, side,
              dw_bf16_ws(lg[LG_DW_FC], s.ln2, w.DY4, g + bp.w_fc, side)))
    return 1;
  if (OB_PROF(OB_PF_GEMM_DX, stream,
              linear_bf(lg[LG_DX_FC], w.DY4, shadow(l, SH_FC), nullptr,
                        nullptr, w.DLN, stream)))
    return 1;
  // ln2 backward takes the residual straight from dout (din = dout + v,
  // no entry copy) and sums both streams it holds in registers: dout
  // columns -> b_mlpproj grad, din columns -> b_attnproj grad
  if (OB_PROF(OB_PF_LN, stream,
              ob_layernorm_bwd_res_ws(s.hmid, p + bp.ln2_w, s.mean2, s.rstd2,
                                      w.DLN, dout, din, g + bp.ln2_w,
                                      g + bp.ln2_b,
                                      dR ? nullptr : g + bp.b_mlpproj,
                                      dR ? nullptr : g + bp.b_attnproj,
                                      BS, H, wsm, stream)))
    return 1;
  // ---- attention projection ----
  const __bf16* dap = din;
  if (dR) {
    if (OB_PROF(OB_PF_ELEM, stream,
                ob_drop_scale_colsum(
                    drop_key(l, slot, OB_DROP_RESID_ATTN, l->p_resid), 1, din,
                    w.dm1, g + bp.b_attnproj, BS, H, stream, wsm)))
      return 1;
    dap = w.dm1;
  }
  OB_SIDE_FENCE(S(stream), g_side.stream);  // din post-ln2-bwd (dm1 ready)
  if (OB_PROF(OB_PF_GEMM_DX, stream,
              linear_bf(lg[LG_DX_AP], dap, shadow(l, SH_AP), nullptr, nullptr,
                        w.DATT, stream)))
    return 1;
  if (OB_PROF(OB_PF_GEMM_DW, side,
              dw_bf16_ws(lg[LG_DW_AP], s.am, dap, g + bp.w_attnproj, side)))
    return 1;
  // din is re-updated by the final ln1 backward: the main stream must
  // not reach it before the side finished reading din
  hipEvent_t ev_din_done = side_evt();
  OB_HIP(hipEventRecord(ev_din_done, g_side.stream));
  // ---- attention core ----
  const bool flash_nt = l->plan.flash && flash_tr();
  if (flash_nt) {
    // the dq kernel forms D = rowsum(dO * O) into w.D for the dkdv kernel;
    // also adds the b_qkv grad (column sums of DQKV) from its accumulators
    // (deterministic mode: not asked for; the side-stream colsum below)
    float* const dbq = det ? nullptr : g + bp.b_qkv;
    if (dA) {
      // regenerates the masks the forward of this slot drew
      if (OB_PROF(OB_PF_FLASH_BWD, stream,
                  ob_flash_bwd_nt_d_drop_bf16(s.qkv, s.am, w.DATT, s.lseP, w.D,
                                              w.DQKV, dbq, B, Sq, H, nh, scale,
                                              l->seed, l->layer_id,
                                              l->slot_tick[slot], l->p_attn,
                                              stream)))
        return 1;
    } else if (OB_PROF(OB_PF_FLASH_BWD, stream,
                       ob_flash_bwd_nt_d_bf16(s.qkv, s.am, w.DATT, s.lseP, w.D,
                                              w.DQKV, dbq, B, Sq, H, nh, scale,
                                              stream)))
      return 1;
  } else if (l->plan.flash) {
    if (OB_PROF(OB_PF_FLASH_BWD, stream,
                ob_transpose_bf16_b(s.qkv, w.QT, Sq, 64, Sq * 3 * H, 64, 3 * H,
                                    B, nh, stream)))
      return 1;
    if (OB_PROF(OB_PF_FLASH_BWD, stream,
                ob_transpose_bf16_b(s.qkv + H, w.KT, Sq, 64, Sq * 3 * H, 64,
                                    3 * H, B, nh, stream)))
      return 1;
    if (OB_PROF(OB_PF_FLASH_BWD, stream,
                ob_transpose_bf16_b(w.DATT, w.dOT, Sq, 64, Sq * H, 64, H, B,
                                    nh, stream)))
      return 1;
    if (OB_PROF(OB_PF_FLASH_BWD, stream,
                ob_flash_dsum_bf16(s.am, w.DATT, w.D, B, Sq, H, nh, stream)))
      return 1;
    if (OB_PROF(OB_PF_FLASH_BWD, stream,
                ob_flash_bwd_bf16(s.qkv, w.QT, w.KT, w.dOT, w.DATT, s.lseP,
                                  w.D, w.DQKV, B, Sq, H, nh, scale, stream)))
      return 1;
  } else {
    // dPd = dO V^T
    ob_bf16_gemm dp = attn_gemm(0, 1, Sq, Sq, hd, 1.f, B, nh, stream);
    dp.A = w.DATT, dp.lda = H, dp.sA1 = Sq * H, dp.sA2 = hd;
    dp.B = s.qkv + 2 * H, dp.ldb = 3 * H, dp.sB1 = Sq * 3 * H, dp.sB2 = hd;
    dp.C = w.DP, dp.ldc = Sq, dp.sC1 = nh * Sq * Sq, dp.sC2 = Sq * Sq;
    if (OB_PROF(OB_PF_ATTN_MAT, stream, ob_gemm_bf16_run(dp))) return 1;
    // attention dropout: DP holds dPd.  Regenerate Pd for dV, mask dPd into
    // dP in place, then the softmax backward runs on the stored P.
    const __bf16* Pv = s.P;
    if (dA) {
      const ob_drop_key ka = drop_key(l, slot, OB_DROP_ATTN, l->p_attn);
      if (OB_PROF(OB_PF_ELEM, stream,
                  ob_drop_scale(ka, 1, s.P, w.pd, B * nh * Sq * Sq, stream)))
        return 1;
      if (OB_PROF(OB_PF_ELEM, stream,
                  ob_drop_scale(ka, 1, w.DP, w.DP, B * nh * Sq * Sq, stream)))
        return 1;
      Pv = w.pd;
    }
    if (OB_PROF(OB_PF_ATTN_MAT, stream,
                ob_softmax_causal_bwd_bf16(s.P, w.DP, B * nh, Sq, stream)))
      return 1;
    // dQ = scale dS K, dK = scale dS^T Q, dV = Pd^T dO into DQKV's thirds
    ob_bf16_gemm dq = attn_gemm(0, 0, Sq, hd, Sq, scale, B, nh, stream);
    dq.A = w.DP, dq.lda = Sq, dq.sA1 = nh * Sq * Sq, dq.sA2 = Sq * Sq;
    dq.B = s.qkv + H, dq.ldb = 3 * H, dq.sB1 = Sq * 3 * H, dq.sB2 = hd;
    dq.C = w.DQKV, dq.ldc = 3 * H, dq.sC1 = Sq * 3 * H, dq.sC2 = hd;
    if (OB_PROF(OB_PF_ATTN_MAT, stream, ob_gemm_bf16_run(dq))) return 1;
    ob_bf16_gemm dk = dq;
    dk.transA = 1, dk.B = s.qkv, dk.C = w.DQKV + H;
    if (OB_PROF(OB_PF_ATTN_MAT, stream, ob_gemm_bf16_run(dk))) return 1;
    ob_bf16_gemm dv = dk;
    dv.alpha = 1.f, dv.A = Pv, dv.C = w.DQKV + 2 * H;
    dv.B = w.DATT, dv.ldb = H, dv.sB1 = Sq * H, dv.sB2 = hd;
    if (OB_PROF(OB_PF_ATTN_MAT, stream, ob_gemm_bf16_run(dv))) return 1;
  }
  // ---- QKV projection ----
  OB_SIDE_FENCE(S(stream), g_side.stream);  // DQKV ready
  if ((!flash_nt || det) &&
      OB_PROF(OB_PF_ELEM, side,
              ob_colsum_ws(w.DQKV, g + bp.b_qkv, BS, 3 * H,
                           det ? ws<float>(WS_DET_SIDE) : nullptr, side)))
    return 1;
  if (OB_PROF(OB_PF_GEMM_DW, side,
              dw_bf16_ws(lg[LG_DW_QKV], s.ln1, w.DQKV, g + bp.w_qkv, side)))
    return 1;
  if (OB_PROF(OB_PF_GEMM_DX, stream,
              linear_bf(lg[LG_DX_QKV], w.DQKV, shadow(l, SH_QKV), nullptr,
                        nullptr, w.DLN, stream)))
    return 1;
  // ln1 backward accumulates into din: wait for the side's din readers
  OB_HIP(hipStreamWaitEvent(S(stream), ev_din_done, 0));
  if (OB_PROF(OB_PF_LN, stream,
              ob_layernorm_bwd_ws(s.x, p + bp.ln1_w, s.mean1, s.rstd1, w.DLN,
                                  din, g + bp.ln1_w, g + bp.ln1_b, BS, H, 1,
                                  wsm, stream)))
    return 1;
  // join: the next call reuses DY4/DQKV/din workspaces on the main stream
  OB_SIDE_FENCE(g_side.stream, S(stream));  // join
  return 0;
}

static int final_backward_bf16(ob_layer* l, int slot, const float* dout,
                               __bf16* din, void* stream) {
  const int64_t Sq = l->d.seq_len, H = l->d.n_embd, V = l->d.vocab_size;
  const int64_t B = l->B, BS = B * Sq;
  const float* p = l->params;
  const FinalStash<__bf16> s(l, slot);
  const BwdWs<__bf16> w(l);
  float* g = l->grads;
  ob_lt_shape lg[LG_FINAL_N];
  final_gemms(H, V, l->plan.v_pad, BS, lg);
  const ob_lt_shape& dwlm = lg[LG_DW_LM];

  if (OB_PROF(OB_PF_CE, stream,
              ob_ce_bwd_bf16(s.logits, s.labs, s.lse, dout, B, Sq, V,
                             l->plan.v_pad, stream)))
    return 1;
  // dW_lm on the side stream (overlaps d_lnout + ln backward below):
  // transpose dlogits and lnf so the GEMM runs on the glds path; tile
  // over v_pad rows, store-guard at V (pad rows of dlogits are 0 anyway,
  // but they have no grad slot).
  {
    OB_SIDE_FENCE(S(stream), g_side.stream);  // dlogits ready
    void* const side = (void*)g_side.stream;
    // direct TN via hipBLASLt: M = V with lda = v_pad skips the pad
    // rows entirely (no store guard, no 826 MB logits transpose)
    int r = -1;
    if (!no_blaslt())
      r = OB_PROF(OB_PF_GEMM_DW, side,
                  ob_gemm_lt(dwlm.tA, dwlm.tB, dwlm.M, dwlm.N, dwlm.K, 1.f,
                             s.logits, dwlm.lda, s.lnf, dwlm.ldb, 1.f,
                             g + 2 * H, dwlm.ldc, dwlm.c_f32, side));
    if (r > 0) return 1;
    if (r < 0) {
      __bf16* DLT = ws<__bf16>(WS_DW_A);
      __bf16* LNT = ws<__bf16>(WS_DW_B);
      if (ob_transpose_bf16(s.logits, DLT, BS, l->plan.v_pad, side)) return 1;
      if (ob_transpose_bf16(s.lnf, LNT, BS, H, side)) return 1;
      ob_bf16_gemm dw;
      dw.A = DLT, dw.lda = BS, dw.B = LNT, dw.ldb = BS;
      dw.C = g + 2 * H, dw.ldc = H, dw.M = l->plan.v_pad, dw.N = H, dw.K = BS;
      dw.out_kind = 2, dw.splitk = ob_deterministic() ? 1 : 2, dw.Mr = V;
      dw.stream = side;
      if (OB_PROF(OB_PF_GEMM_DW, side, ob_gemm_bf16_nt_dispatch(dw)))
        return 1;
    }
  }
  // d_lnout: K = v_pad (padded dlogits cols and shadow^T cols are zero)
  if (OB_PROF(OB_PF_GEMM_DX, stream,
              linear_bf(lg[LG_DLNOUT], s.logits, shadow(l, SH_LM_T),
                        nullptr, nullptr, w.DLN, stream)))
    return 1;
  float* const wsm = ob_deterministic() ? ws<float>(WS_DET_MAIN) : nullptr;
  if (OB_PROF(OB_PF_LN, stream,
              ob_layernorm_bwd_ws(s.x, p + 0, s.mean, s.rstd, w.DLN, din,
                                  g + 0, g + H, BS, H, 0, wsm, stream)))
    return 1;
  // join: the next backward reuses the dW buffers and reads g on the main
  // stream
  OB_SIDE_FENCE(g_side.stream, S(stream));  // join
  return 0;
}

extern "C" int ob_layer_forward(ob_layer_t l, int32_t slot, const void* in,
                                void* out, const int64_t* labels,
                                void* stream) {
  if (!l) return ob_fail("forward: null layer");
  if (!l->params) return ob_fail("forward: params not bound");
  if (slot < 0 || slot >= l->d.n_slots) return ob_fail("forward: bad slot");
  // dropout bookkeeping: this slot's backward regenerates the masks from
  // the tick recorded here, never from "the latest"
  const bool drop = l->training && has_dropout(l);
  l->slot_drop[slot] = drop ? 1 : 0;
  l->slot_tick[slot] = l->next_tick;
  if (drop) l->next_tick++;
  switch (l->d.kind) {
    case OB_KIND_EMBED: {
      const int64_t Sq = l->d.seq_len, H = l->d.n_embd, V = l->d.vocab_size;
      const int64_t BS = (int64_t)l->B * Sq;
      int64_t* ids = slot_ids(l, slot);
      OB_HIP(hipMemcpyAsync(ids, in, BS * sizeof(int64_t),
                            hipMemcpyDeviceToDevice, S(stream)));
      if (drop)
        return OB_PROF(OB_PF_ELEM, stream,
                       ob_embed_fwd_drop(
                           drop_key(l, slot, OB_DROP_EMBD, l->p_embd),
                           l->d.dtype == 1, ids, l->params, l->params + V * H,
                           out, l->B, Sq, H, stream));
      if (l->d.dtype == 1)
        return OB_PROF(OB_PF_ELEM, stream,
                       ob_embed_fwd_bf16(ids, l->params, l->params + V * H,
                                         out, l->B, Sq, H, stream));
      return OB_PROF(OB_PF_ELEM, stream,
                     ob_embed_fwd_f32(ids, l->params, l->params + V * H,
                                      (float*)out, l->B, Sq, H, stream));
    }
    case OB_KIND_BLOCK:
      if (l->d.dtype == 1)
        return block_forward_bf16(l, slot, (const __bf16*)in, (__bf16*)out,
                                  stream);
      return block_forward(l, slot, (const float*)in, (float*)out, stream);
    case OB_KIND_FINAL:
      if (l->d.dtype == 1)
        return final_forward_bf16(l, slot, (const __bf16*)in, (float*)out,
                                  labels, stream);
      return final_forward(l, slot, (const float*)in, (float*)out, labels,
                           stream);
  }
  return ob_fail("forward: bad kind");
}

// ---------------------------------------------------------------------------
// backward (accumulates into the bound grad buffer)
// ---------------------------------------------------------------------------

static int block_backward(ob_layer* l, int slot, const float* dout, float* din,
                          void* stream) {
  const int64_t Sq = l->d.seq_len, H = l->d.n_embd, nh = l->d.n_head;
  const int64_t B = l->B, BS = B * Sq;
  const int64_t hd = H / nh;
  const float scale = 1.f / sqrtf((float)hd);
  const float* p = l->params;
  const BlockStash<float> s(l, slot);
  const BwdWs<float> w(l);
  float* g = l->grads;
  const BlockParams bp = block_params(H);
  // the masks this slot's forward drew, regenerated from its tick
  const bool dA = l->slot_drop[slot] && l->p_attn > 0.f;
  const bool dR = l->slot_drop[slot] && l->p_resid > 0.f;

  // din starts as d(h_mid) accumulator = dout (residual skip)
  OB_HIP(hipMemcpyAsync(din, dout, BS * H * sizeof(float),
                        hipMemcpyDeviceToDevice, S(stream)));
  // ---- MLP backward ----
  // residual dropout: the projection saw dm = mask*dout (the kernel also
  // takes db = colsum(dm)); the residual skip above keeps dout itself
  const float* dmlp = dout;
  if (dR) {
    if (ob_drop_scale_colsum(drop_key(l, slot, OB_DROP_RESID_MLP, l->p_resid),
                             0, dout, w.dm2, g + bp.b_mlpproj, BS, H, stream))
      return 1;
    dmlp = w.dm2;
  }
  // dg = dout @ w_mlpproj^T
  if (gemm(0, 1, BS, 4 * H, H, 1.f, dmlp, H, 0, 0, p + bp.w_mlpproj, H, 0, 0,
           0.f, w.DY4, 4 * H, 0, 0, 1, 1, nullptr, nullptr, 0, 1, stream))
    return 1;
  // dW_mlpproj += g^T @ dout ; db += colsum(dout)
  if (gemm(1, 0, 4 * H, H, BS, 1.f, s.gact, 4 * H, 0, 0, dmlp, H, 0, 0, 1.f,
           g + bp.w_mlpproj, H, 0, 0, 1, 1, nullptr, nullptr, 1,
           pick_splitk(4 * H, H, BS), stream))
    return 1;
  if (!dR && ob_colsum_f32(dout, g + bp.b_mlpproj, BS, H, stream)) return 1;
  // du = dg * gelu'(u)   (in place on DY4)
  if (ob_gelu_bwd_f32(s.u, w.DY4, w.DY4, BS * 4 * H, stream)) return 1;
  // dW_fc += ln2^T @ du ; db_fc += colsum(du)
  if (gemm(1, 0, H, 4 * H, BS, 1.f, s.ln2, H, 0, 0, w.DY4, 4 * H, 0, 0, 1.f,
           g + bp.w_fc, 4 * H, 0, 0, 1, 1, nullptr, nullptr, 1,
           pick_splitk(H, 4 * H, BS), stream))
    return 1;
  if (ob_colsum_f32(w.DY4, g + bp.b_fc, BS, 4 * H, stream)) return 1;
  // d_ln2out = du @ w_fc^T  (narrow-N: auto split-K)
  if (gemm_dx_splitk(1, BS, H, 4 * H, 1.f, w.DY4, 4 * H, p + bp.w_fc, 4 * H,
                     w.DLN, H, stream))
    return 1;
  // ln2 backward: din += dx ; dw/db accumulate
  if (ob_layernorm_bwd_f32(s.hmid, p + bp.ln2_w, s.mean2, s.rstd2, w.DLN, din,
                           g + bp.ln2_w, g + bp.ln2_b, BS, H, 1, stream))
    return 1;
  // ---- attention projection backward (din now = d_hmid) ----
  const float* dap = din;
  if (dR) {
    if (ob_drop_scale_colsum(drop_key(l, slot, OB_DROP_RESID_ATTN, l->p_resid),
                             0, din, w.dm1, g + bp.b_attnproj, BS, H, stream))
      return 1;
    dap = w.dm1;
  }
  if (gemm_dx_splitk(1, BS, H, H, 1.f, dap, H, p + bp.w_attnproj, H, w.DATT,
                     H, stream))
    return 1;
  if (gemm(1, 0, H, H, BS, 1.f, s.am, H, 0, 0, dap, H, 0, 0, 1.f,
           g + bp.w_attnproj, H, 0, 0, 1, 1, nullptr, nullptr, 1,
           pick_splitk(H, H, BS), stream))
    return 1;
  if (!dR && ob_colsum_f32(din, g + bp.b_attnproj, BS, H, stream)) return 1;
  // ---- attention core backward ----
  // dP = dO @ V^T
  if (gemm(0, 1, Sq, Sq, hd, 1.f, w.DATT, H, Sq * H, hd, s.qkv + 2 * H, 3 * H,
           Sq * 3 * H, hd, 0.f, w.DP, Sq, nh * Sq * Sq, Sq * Sq, B, nh, nullptr,
           nullptr, 0, 1, stream))
    return 1;
  // attention dropout: DP holds dPd.  Regenerate Pd for dV, mask dPd into
  // dP in place; the softmax backward then runs on the stored P.
  const float* Pv = s.P;
  if (dA) {
    const ob_drop_key ka = drop_key(l, slot, OB_DROP_ATTN, l->p_attn);
    if (ob_drop_scale(ka, 0, s.P, w.pd, B * nh * Sq * Sq, stream)) return 1;
    if (ob_drop_scale(ka, 0, w.DP, w.DP, B * nh * Sq * Sq, stream)) return 1;
    Pv = w.pd;
  }
  // dS = softmax_bwd(P, dP)  in place on DP
  if (ob_softmax_causal_bwd_f32(s.P, w.DP, B * nh, Sq, stream)) return 1;
  // dQ = scale * dS @ K
  if (gemm(0, 0, Sq, hd, Sq, scale, w.DP, Sq, nh * Sq * Sq, Sq * Sq, s.qkv + H,
           3 * H, Sq * 3 * H, hd, 0.f, w.DQKV, 3 * H, Sq * 3 * H, hd, B, nh,
           nullptr, nullptr, 0, 1, stream))
    return 1;
  // dK = scale * dS^T @ Q
  if (gemm(1, 0, Sq, hd, Sq, scale, w.DP, Sq, nh * Sq * Sq, Sq * Sq, s.qkv,
           3 * H, Sq * 3 * H, hd, 0.f, w.DQKV + H, 3 * H, Sq * 3 * H, hd, B, nh,
           nullptr, nullptr, 0, 1, stream))
    return 1;
  // dV = Pd^T @ dO
  if (gemm(1, 0, Sq, hd, Sq, 1.f, Pv, Sq, nh * Sq * Sq, Sq * Sq, w.DATT, H,
           Sq * H, hd, 0.f, w.DQKV + 2 * H, 3 * H, Sq * 3 * H, hd, B, nh,
           nullptr, nullptr, 0, 1, stream))
    return 1;
  // ---- QKV projection backward ----
  if (ob_colsum_f32(w.DQKV, g + bp.b_qkv, BS, 3 * H, stream)) return 1;
  if (gemm(1, 0, H, 3 * H, BS, 1.f, s.ln1, H, 0, 0, w.DQKV, 3 * H, 0, 0, 1.f,
           g + bp.w_qkv, 3 * H, 0, 0, 1, 1, nullptr, nullptr, 1,
           pick_splitk(H, 3 * H, BS), stream))
    return 1;
  if (gemm_dx_splitk(1, BS, H, 3 * H, 1.f, w.DQKV, 3 * H, p + bp.w_qkv, 3 * H,
                     w.DLN, H, stream))
    return 1;
  // ln1 backward: din += dx
  return ob_layernorm_bwd_f32(s.x, p + bp.ln1_w, s.mean1, s.rstd1, w.DLN, din,
                              g + bp.ln1_w, g + bp.ln1_b, BS, H, 1, stream);
}

static int final_backward(ob_layer* l, int slot, const float* dout, float* din,
                          void* stream) {
  const int64_t Sq = l->d.seq_len, H = l->d.n_embd, V = l->d.vocab_size;
  const int64_t B = l->B, BS = B * Sq;
  const float* p = l->params;
  const FinalStash<float> s(l, slot);
  const BwdWs<float> w(l);
  float* g = l->grads;

  if (ob_ce_bwd_f32(s.logits, s.labs, s.lse, (const float*)dout, B, Sq, V,
                    stream))
    return 1;
  // dW_lm += dlogits^T @ ln_out
  if (gemm(1, 0, V, H, BS, 1.f, s.logits, V, 0, 0, s.lnf, H, 0, 0, 1.f,
           g + 2 * H, H, 0, 0, 1, 1, nullptr, nullptr, 1, 1, stream))
    return 1;
  // d_lnout = dlogits @ w_lm  (N=H, K=V: auto split-K)
  if (gemm_dx_splitk(0, BS, H, V, 1.f, s.logits, V, p + 2 * H, H, w.DLN, H,
                     stream))
    return 1;
  return ob_layernorm_bwd_f32(s.x, p + 0, s.mean, s.rstd, w.DLN, din, g + 0,
                              g + H, BS, H, 0, stream);
}

extern "C" int ob_layer_backward(ob_layer_t l, int32_t slot, const void* dout,
                                 void* din, void* stream) {
  if (!l) return ob_fail("backward: null layer");
  if (!l->params || !l->grads) return ob_fail("backward: buffers not bound");
  if (slot < 0 || slot >= l->d.n_slots) return ob_fail("backward: bad slot");
  switch (l->d.kind) {
    case OB_KIND_EMBED: {
      const int64_t Sq = l->d.seq_len, H = l->d.n_embd, V = l->d.vocab_size;
      int64_t* ids = slot_ids(l, slot);
      if (ob_deterministic()) {  // bf16 only: create refuses fp32
        const ob_drop_key ke = drop_key(l, slot, OB_DROP_EMBD, l->p_embd);
        return OB_PROF(OB_PF_ELEM, stream,
                       ob_embed_bwd_det(l->slot_drop[slot] ? &ke : nullptr,
                                        ids, dout, l->grads, l->grads + V * H,
                                        l->B, Sq, H, stream));
      }
      if (l->slot_drop[slot])
        return OB_PROF(OB_PF_ELEM, stream,
                       ob_embed_bwd_drop(
                           drop_key(l, slot, OB_DROP_EMBD, l->p_embd),
                           l->d.dtype == 1, ids, dout, l->grads,
                           l->grads + V * H, l->B, Sq, H, stream));
      if (l->d.dtype == 1)
        return OB_PROF(OB_PF_ELEM, stream,
                       ob_embed_bwd_bf16(ids, dout, l->grads,
                                         l->grads + V * H, l->B, Sq, H,
                                         stream));
      return OB_PROF(OB_PF_ELEM, stream,
                     ob_embed_bwd_f32(ids, (const float*)dout, l->grads,
                                      l->grads + V * H, l->B, Sq, H,
                                      stream));
    }
    case OB_KIND_BLOCK:
      if (!dout || !din) return ob_fail("block backward: dout/din required");
      if (l->d.dtype == 1)
        return block_backward_bf16(l, slot, (const __bf16*)dout, (__bf16*)din,
                                   stream);
      return block_backward(l, slot, (const float*)dout, (float*)din, stream);
    case OB_KIND_FINAL:
      if (!din) return ob_fail("final backward: din required");
      if (l->d.dtype == 1)
        return final_backward_bf16(l, slot, (const float*)dout, (__bf16*)din,
                                   stream);
      return final_backward(l, slot, (const float*)dout, (float*)din, stream);
  }
  return ob_fail("backward: bad kind");
}
