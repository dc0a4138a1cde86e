// ob_layer_plan.h — the device memory of one layer, as one host-only table:
// the slot-strided stash it owns, its bf16 weight shadows, and what it needs
// of the process-wide workspace.  ob_layer_plan_of is a pure function of its
// arguments (no GPU call, no process state): ob_layer_create allocates from
// it, the views of ob_layer.hip index by it, and ob_layer_plan_query reports
// it.  DESIGN.md "Layer memory" is this file in prose.
#pragma once
#include <cstdint>

#include "../../include/oobleck_stage.h"

// stash regions, in slot order (offsets and lengths in floats; a bf16 layer
// keeps bf16 data in the first half of an fp32-sized region)
enum {
  ST_X = 0, ST_MEAN1, ST_RSTD1, ST_LN1, ST_QKV,
  ST_P,  // P [B*nh, S, S]; a flash layer keeps only the row LSE [B*nh, S]
  ST_ATTNM, ST_HMID, ST_MEAN2, ST_RSTD2, ST_LN2, ST_U, ST_G,
  ST_LOGITS,  // FINAL; bf16: [BS, v_pad] bf16
  ST_LSE,
  ST_N
};

// bf16 weight shadows, plain and transposed (offsets in bf16 elements)
enum {
  SH_QKV = 0, SH_QKV_T, SH_AP, SH_AP_T, SH_FC, SH_FC_T, SH_MP, SH_MP_T,
  SH_LM, SH_LM_T,  // [v_pad, H] and [H, v_pad], pad rows zero
  SH_N
};

// workspace buffers, shared by every layer of the process (one driving
// thread per GPU).  main / side / fwd: the backward's stream, the dW side
// stream, the forward's stream (which under pp1 overlap runs beside a
// backward, so forward buffers are shared with no backward buffer).
enum {
  WS_DP = 0,     // main: dP -> dS [B*nh, S, S], materialized-P backward
  WS_DLN,        // main: grad of a LayerNorm's output [BS, H]
  WS_DATT,       // main: grad of the attention output [BS, H]
  WS_DQKV,       // main, read by side until the join: grad of qkv [BS, 3H]
  WS_DY4,        // main, read by side until the join: MLP grads [BS, 4H]
  WS_FLASH_BWD,  // main: flash D [B*nh, S]; OB_FLASH_TR=0: Q^T|K^T|dO^T|D
  WS_FLASH_VT,   // fwd: V^T, OB_FLASH_TR=0 only
  WS_DW_A,       // side: BLOCK: the fp32 slab [s, M, N] of a sliced dW call
                 // (ob_dw_slices.h), or, when the library takes no part, the
                 // dW fallback's A^T (act^T; FINAL: dlogits^T), bf16; a call
                 // runs one of the two, so the buffer has one user at a time
  WS_DW_B,       // side: dW fallback's B^T (dY^T; FINAL: ln_f out^T), bf16
  WS_PD_FWD,     // fwd: Pd = drop(P), attention dropout without flash
  WS_PD_BWD,     // main: Pd regenerated, attention dropout without flash
  WS_DM_ATTN,    // main, read by side until the join: masked d(hmid) [BS, H]
  WS_DM_MLP,     // main, read by side until the join: masked dout [BS, H]
  WS_DET_MAIN,   // main: deterministic slab (dropout colsum, gelu, LN bwd)
  WS_DET_SIDE,   // side: deterministic slab (b_qkv colsum)
  WS_DET_FWD,    // fwd: deterministic slab (CE loss)
  WS_N
};

// the process switches a plan depends on
struct ob_layer_modes {
  bool det, bf16_flash, flash_tr, flash_drop, flash_hd128;
};

struct ob_layer_plan {
  bool flash = false;  // fused flash attention (decided here: sizes ST_P)
  bool side = false;   // needs the side stream
  int64_t v_pad = 0;   // vocab rows of the lm_head shadows, logits and GEMMs
  int64_t st_off[ST_N] = {}, st_len[ST_N] = {}, slot_stride = 0;  // floats
  int64_t ids_count = 0;  // int64 ids (EMBED) / labels (FINAL), all slots
  int64_t sh_off[SH_N] = {}, shadow_count = 0;  // bf16 elements
  int64_t ws[WS_N] = {};  // floats needed of each buffer, 0 = not used
  // WS_FLASH_BWD's layout: Q^T, K^T, dO^T (bf16 elements; OB_FLASH_TR=0
  // only) and D (floats; 0 on the production path, which holds D alone)
  int64_t pk_qt = 0, pk_kt = 0, pk_dot = 0, pk_d = 0;
  const char* error = nullptr;  // non-null: no layer can be created from it
};

// Vocab rows of the lm_head shadows, logits and their GEMMs: padded to a 256
// multiple, which makes the lm_head GEMM family (logits fwd, d_lnout, dW_lm
// via transposes) interior shapes for the glds path AND the 256^2 8-phase
// kernel (gpt2's 50257 at 128 padding lands on 50304 % 256 != 0); shadow pad
// rows stay zero, so padded logits and grads are exactly zero.
inline int64_t ob_v_pad(int64_t V) { return (V + 255) / 256 * 256; }

// flash applies to bf16 BLOCK layers with n_embd % n_head == 0, head_dim 64
// (GPT-2 small and XL) or 128 (the GPT-3 sizes from 1.3B up) and S % 128 ==
// 0.  head_dim 128 has production kernels only: no OB_FLASH_TR=0 twins and
// no dropout variant; at head_dim 64 only the production kernels have one.
inline bool ob_plan_flash(const ob_layer_desc& d, float p_attn,
                          const ob_layer_modes& m) {
  if (p_attn > 0.f && !(m.flash_tr && m.flash_drop)) return false;
  if (!m.bf16_flash || d.kind != OB_KIND_BLOCK || d.dtype != 1 ||
      d.n_head <= 0 || d.n_embd % d.n_head || d.seq_len <= 0 ||
      d.seq_len % 128)
    return false;
  const int64_t hd = d.n_embd / d.n_head;
  if (hd == 128) return p_attn == 0.f && m.flash_tr && m.flash_hd128;
  return hd == 64;
}

inline ob_layer_plan ob_layer_plan_of(const ob_layer_desc& d, float p_resid,
                                      float p_attn, const ob_layer_modes& m) {
  ob_layer_plan p;
  const int64_t Bm = d.max_batch, Sq = d.seq_len, H = d.n_embd, nh = d.n_head,
                V = d.vocab_size;
  const int64_t BS = Bm * Sq, BSH = BS * H, PSS = Bm * nh * Sq * Sq;
  const int64_t half4 = (4 * H * BS + 1) / 2;  // [BS, 4H] bf16, in floats
  const bool bf16 = d.dtype == 1;
  p.v_pad = ob_v_pad(V);
  p.flash = ob_plan_flash(d, p_attn, m);
  int64_t o = 0, o2 = 0;
  auto st = [&](int r, int64_t n) { p.st_off[r] = o, p.st_len[r] = n, o += n; };
  auto sh = [&](int r, int64_t n) { p.sh_off[r] = o2, o2 += n; };
  auto det = [&](int which, int64_t N) {
    return m.det && bf16 ? ob_det_ws_count(which, BS, N) : 0;
  };
  auto max2 = [](int64_t a, int64_t b) { return a > b ? a : b; };
  switch (d.kind) {
    case OB_KIND_EMBED:
      p.ids_count = BS * d.n_slots;
      break;
    case OB_KIND_BLOCK:
      st(ST_X, BSH), st(ST_MEAN1, BS), st(ST_RSTD1, BS), st(ST_LN1, BSH);
      st(ST_QKV, 3 * BSH), st(ST_P, p.flash ? Bm * nh * Sq : PSS);
      st(ST_ATTNM, BSH), st(ST_HMID, BSH), st(ST_MEAN2, BS), st(ST_RSTD2, BS);
      st(ST_LN2, BSH), st(ST_U, 4 * BSH), st(ST_G, 4 * BSH);
      p.ws[WS_DP] = p.flash ? 0 : PSS;
      p.ws[WS_DLN] = p.ws[WS_DATT] = BSH;
      p.ws[WS_DQKV] = 3 * BSH, p.ws[WS_DY4] = 4 * BSH;
      if (p_attn > 0.f && !p.flash) p.ws[WS_PD_FWD] = p.ws[WS_PD_BWD] = PSS;
      if (p_resid > 0.f) p.ws[WS_DM_ATTN] = p.ws[WS_DM_MLP] = BSH;
      if (!bf16) break;
      sh(SH_QKV, 3 * H * H), sh(SH_QKV_T, 3 * H * H), sh(SH_AP, H * H);
      sh(SH_AP_T, H * H), sh(SH_FC, 4 * H * H), sh(SH_FC_T, 4 * H * H);
      sh(SH_MP, 4 * H * H), sh(SH_MP_T, 4 * H * H);
      p.side = true;
      p.ws[WS_DW_A] = p.ws[WS_DW_B] = half4;
      if (p.flash && m.flash_tr) {
        p.ws[WS_FLASH_BWD] = Bm * nh * Sq;
      } else if (p.flash) {
        p.ws[WS_FLASH_BWD] = p.ws[WS_FLASH_VT] = half4;
        p.pk_kt = BSH, p.pk_dot = 2 * BSH, p.pk_d = (3 * BSH + 1) / 2;
        if (p.pk_d + Bm * nh * Sq > p.ws[WS_FLASH_BWD] ||
            BSH > 2 * p.ws[WS_FLASH_VT])
          p.error = "OB_FLASH_TR=0 transposes do not fit their workspace";
      }
      p.ws[WS_DET_MAIN] =
          max2(max2(det(OB_DET_WS_GELU, 4 * H), det(OB_DET_WS_LN, H)),
               p_resid > 0.f ? det(OB_DET_WS_DROP_CS, H) : 0);
      p.ws[WS_DET_SIDE] = det(OB_DET_WS_COLSUM, 3 * H);
      break;
    case OB_KIND_FINAL:
      st(ST_X, BSH), st(ST_MEAN1, BS), st(ST_RSTD1, BS), st(ST_LN1, BSH);
      // the bf16 logits are [BS, v_pad] bf16, more than BS * V floats when
      // V < 128
      st(ST_LOGITS, bf16 ? max2(BS * V, (BS * p.v_pad + 1) / 2) : BS * V);
      st(ST_LSE, BS);
      p.ids_count = BS * d.n_slots;
      p.ws[WS_DLN] = BSH;
      if (!bf16) break;
      sh(SH_LM, p.v_pad * H), sh(SH_LM_T, H * p.v_pad);
      p.side = true;
      p.ws[WS_DW_A] = (p.v_pad * BS + 1) / 2, p.ws[WS_DW_B] = half4;
      p.ws[WS_DET_MAIN] = det(OB_DET_WS_LN, H);
      p.ws[WS_DET_FWD] = det(OB_DET_WS_CE, 1);
      break;
  }
  p.slot_stride = o, p.shadow_count = o2;
  return p;
}

// ob_layer_plan_query's field order (include/oobleck_stage.h)
#define OB_LAYER_PLAN_FIELDS (6 + 2 * ST_N + SH_N + WS_N + 4)
inline void ob_layer_plan_fields(const ob_layer_plan& p, int64_t* f) {
  *f++ = p.flash, *f++ = p.side, *f++ = p.v_pad, *f++ = p.slot_stride;
  *f++ = p.ids_count, *f++ = p.shadow_count;
  for (int i = 0; i < ST_N; i++) *f++ = p.st_off[i];
  for (int i = 0; i < ST_N; i++) *f++ = p.st_len[i];
  for (int i = 0; i < SH_N; i++) *f++ = p.sh_off[i];
  for (int i = 0; i < WS_N; i++) *f++ = p.ws[i];
  *f++ = p.pk_qt, *f++ = p.pk_kt, *f++ = p.pk_dot, *f++ = p.pk_d;
}
