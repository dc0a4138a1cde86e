# ctypes binding of the C-ABI (include/oobleck_stage.h).
#
# The product compute path runs ONLY through this extension.  If the .so is
# missing on a machine with a GPU, get_ext() raises — there is no eager /
# PyTorch fallback for the hot path (tier contract: a silent fallback would
# void every parity and perf claim).
from __future__ import annotations

import ctypes
import pathlib

_LIB = None
SO_PATH = pathlib.Path(__file__).resolve().parent / "libob_stage.so"


class ObLayerDesc(ctypes.Structure):
    _fields_ = [
        ("kind", ctypes.c_int32),
        ("n_embd", ctypes.c_int32),
        ("n_head", ctypes.c_int32),
        ("n_positions", ctypes.c_int32),
        ("vocab_size", ctypes.c_int32),
        ("max_batch", ctypes.c_int32),
        ("seq_len", ctypes.c_int32),
        ("n_slots", ctypes.c_int32),
        ("dtype", ctypes.c_int32),
    ]


class ObDropoutDesc(ctypes.Structure):
    _fields_ = [
        ("embd_pdrop", ctypes.c_float),
        ("resid_pdrop", ctypes.c_float),
        ("attn_pdrop", ctypes.c_float),
        ("layer_id", ctypes.c_int32),
        ("seed", ctypes.c_uint64),
    ]


# dropout sites (OB_DROP_* of include/oobleck_stage.h)
DROP_EMBD, DROP_ATTN, DROP_RESID_ATTN, DROP_RESID_MLP = 0, 1, 2, 3


def _configure(lib: ctypes.CDLL) -> ctypes.CDLL:
    i64, i32, f32, vp = ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_void_p
    lib.ob_last_error.restype = ctypes.c_char_p
    lib.ob_build_arch.restype = ctypes.c_char_p
    lib.ob_layer_param_count.restype = i64
    lib.ob_layer_param_count.argtypes = [ctypes.POINTER(ObLayerDesc)]
    lib.ob_layer_create.argtypes = [ctypes.POINTER(ObLayerDesc),
                                    ctypes.POINTER(vp)]
    u64 = ctypes.c_uint64
    lib.ob_layer_create_ex.argtypes = [ctypes.POINTER(ObLayerDesc),
                                       ctypes.POINTER(ObDropoutDesc),
                                       ctypes.POINTER(vp)]
    lib.ob_layer_set_training.argtypes = [vp, i32]
    lib.ob_layer_uses_flash.argtypes = [vp]
    lib.ob_flash_eligible.argtypes = [ctypes.POINTER(ObLayerDesc), f32]
    lib.ob_layer_plan_query.argtypes = [ctypes.POINTER(ObLayerDesc),
                                        ctypes.POINTER(ObDropoutDesc), i32,
                                        ctypes.POINTER(i64), i32]
    lib.ob_layer_set_dropout_tick.argtypes = [vp, u64]
    # (seed, layer_id, site, tick, p) select the mask of every dropout entry
    key = [u64, i32, i32, u64, f32]
    lib.ob_dropout_mask.argtypes = key + [i64, vp, vp]
    lib.ob_dropout_scale_f32.argtypes = key + [vp, vp, i64, vp]
    lib.ob_dropout_scale_bf16.argtypes = key + [vp, vp, i64, vp]
    lib.ob_dropout_add_f32.argtypes = key + [vp, vp, vp, i64, vp]
    lib.ob_dropout_add_bf16.argtypes = key + [vp, vp, vp, i64, vp]
    lib.ob_dropout_scale_colsum_f32.argtypes = key + [vp, vp, vp, i64, i64, vp]
    lib.ob_dropout_scale_colsum_bf16.argtypes = key + [vp, vp, vp, i64, i64,
                                                       vp]
    lib.ob_layer_bind.argtypes = [vp, vp, vp]
    lib.ob_layer_set_batch.argtypes = [vp, i32]
    lib.ob_layer_forward.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.ob_layer_backward.argtypes = [vp, i32, vp, vp, vp]
    lib.ob_layer_destroy.argtypes = [vp]
    lib.ob_layer_refresh_weights.argtypes = [vp, vp]
    lib.ob_adamw_step.argtypes = [vp, vp, vp, vp, i64, i32, f32, f32, f32,
                                  f32, f32, vp]
    lib.ob_sqnorm_ws_count.restype = i64
    lib.ob_sqnorm_ws_count.argtypes = [ctypes.POINTER(i64), i32]
    lib.ob_sqnorm_multi_f32.argtypes = [ctypes.POINTER(vp),
                                        ctypes.POINTER(i64),
                                        ctypes.POINTER(i32), i32, vp, vp, vp]
    lib.ob_clip_finish.argtypes = [vp, i32, f32, vp, vp]
    lib.ob_adamw_step_scaled.argtypes = [vp, vp, vp, vp, i64, i32, f32, f32,
                                         f32, f32, f32, vp, vp]
    lib.ob_gemm_f32.argtypes = [i32, i32, i64, i64, i64, f32, vp, i64, i64,
                                i64, vp, i64, i64, i64, f32, vp, i64, i64,
                                i64, i64, i64, vp, vp, i32, i32, vp]
    lib.ob_layernorm_fwd_f32.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64,
                                         f32, vp]
    lib.ob_layernorm_bwd_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i64,
                                         i64, i32, vp]
    lib.ob_softmax_causal_fwd_f32.argtypes = [vp, i64, i64, f32, vp]
    lib.ob_softmax_causal_bwd_f32.argtypes = [vp, vp, i64, i64, vp]
    lib.ob_gelu_fwd_f32.argtypes = [vp, vp, i64, vp]
    lib.ob_gelu_bwd_f32.argtypes = [vp, vp, vp, i64, vp]
    lib.ob_colsum_f32.argtypes = [vp, vp, i64, i64, vp]
    lib.ob_gemm_bf16.argtypes = [i32, i32, i64, i64, i64, f32, vp, i64, i64,
                                 i64, vp, i64, i64, i64, f32, vp, i64, i64,
                                 i64, i64, i64, vp, vp, i32, i32, vp]
    lib.ob_f32_to_bf16.argtypes = [vp, vp, i64, vp]
    lib.ob_f32_to_bf16_t.argtypes = [vp, vp, i64, i64, vp]
    lib.ob_f32_to_bf16_t_ld.argtypes = [vp, vp, i64, i64, i64, vp]
    lib.ob_bf16_to_f32.argtypes = [vp, vp, i64, vp]
    # every remaining kernel entry point: ctypes without argtypes passes
    # Python ints as 32-bit c_int, leaving int64 params with undefined
    # upper halves (the elem_probe/ce_probe GPU faults) — declare them all
    lib.ob_gelu_fwd_bf16.argtypes = [vp, vp, i64, vp]
    lib.ob_gelu_bwd_bf16.argtypes = [vp, vp, vp, i64, vp]
    lib.ob_ce_fwd_bf16.argtypes = [vp, vp, vp, vp, i64, i64, i64, i64, vp]
    lib.ob_ce_bwd_bf16.argtypes = [vp, vp, vp, vp, i64, i64, i64, i64, vp]
    lib.ob_embed_fwd_bf16.argtypes = [vp, vp, vp, vp, i64, i64, i64, vp]
    lib.ob_embed_bwd_bf16.argtypes = [vp, vp, vp, vp, i64, i64, i64, vp]
    lib.ob_softmax_causal_fwd_bf16.argtypes = [vp, i64, i64, f32, vp]
    lib.ob_softmax_causal_bwd_bf16.argtypes = [vp, vp, i64, i64, vp]
    lib.ob_transpose_bf16.argtypes = [vp, vp, i64, i64, vp]
    lib.ob_gemm_lt_bias.argtypes = [i32, i32, i64, i64, i64, f32, vp, i64,
                                    vp, i64, f32, vp, i64, i32, vp, vp]
    lib.ob_gemm_lt_f32.argtypes = [i32, i32, i64, i64, i64, f32, vp, i64,
                                   vp, i64, f32, vp, i64, vp]
    lib.ob_flash_fwd_bf16.argtypes = [vp, vp, vp, vp, i64, i64, i64, i64,
                                      f32, vp]
    lib.ob_transpose_bf16_b.argtypes = [vp, vp, i64, i64, i64, i64, i64,
                                        i64, i64, vp]
    lib.ob_layernorm_fwd_bf16.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64,
                                          f32, vp]
    lib.ob_layernorm_bwd_bf16.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp,
                                          i64, i64, i32, vp]
    lib.ob_colsum_bf16.argtypes = [vp, vp, i64, i64, vp]
    lib.ob_layernorm_fwd_copy_bf16.argtypes = [vp, vp, vp, vp, vp, vp, vp,
                                               i64, i64, f32, vp]
    lib.ob_layernorm_bwd_res_bf16.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp,
                                              vp, vp, vp, i64, i64, vp]
    lib.ob_gelu_bwd_colsum_bf16.argtypes = [vp, vp, vp, vp, i64, i64, vp]
    lib.ob_gemm_lt.argtypes = [i32, i32, i64, i64, i64, f32, vp, i64, vp,
                               i64, f32, vp, i64, i32, vp]
    lib.ob_gemm_bf16_nt_8ph.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64,
                                        i64, i64, i64, i64, i64, i64, i64,
                                        i64, i64, i64, i64, f32, f32, i32,
                                        i32, vp, i64]
    lib.ob_gemm_bf16_route.argtypes = [i32, i32, i64, i64, i64, i64, i64, i32,
                                       i32, f32, i32, i32, ctypes.c_char_p,
                                       ctypes.POINTER(ctypes.c_int32)]
    lib.ob_gemm_lt_bias_res.argtypes = [i32, i32, i64, i64, i64, f32, vp, i64,
                                        vp, i64, vp, i64, i32, vp, vp, vp]
    # hipBLASLt solution choice; a shape is LT_SHAPE_FIELDS int64s
    shape = ctypes.POINTER(i64)
    lib.ob_layer_lt_shapes.argtypes = [ctypes.POINTER(ObLayerDesc), shape, i32]
    lib.ob_gemm_lt_tune.argtypes = [shape]
    lib.ob_gemm_lt_choice.argtypes = [shape, ctypes.POINTER(ctypes.c_double),
                                      ctypes.c_char_p, ctypes.c_char_p, i32]
    lib.ob_gemm_lt_candidates.argtypes = [shape, ctypes.POINTER(i32),
                                          ctypes.POINTER(i32),
                                          ctypes.POINTER(ctypes.c_double), i32]
    lib.ob_gemm_lt_table_size.argtypes = []
    lib.ob_gemm_lt_table_size.restype = i64
    lib.ob_gemm_lt_untuned_uses.argtypes = []
    lib.ob_gemm_lt_untuned_uses.restype = i64
    lib.ob_gemm_lt_plan_index.argtypes = [shape, vp]
    # sliced weight grads
    lib.ob_dw_slices_admit.argtypes = [shape, i32, i32, i64]
    lib.ob_gemm_lt_dw_sliced.argtypes = [i64, i64, i64, vp, i64, vp, i64, vp,
                                         i64, i32, vp, i64, vp,
                                         ctypes.POINTER(i32)]
    lib.ob_gemm_lt_tune_slab.argtypes = [shape, i64]
    lib.ob_gemm_lt_slices.argtypes = [shape, ctypes.POINTER(ctypes.c_double),
                                      ctypes.POINTER(i32), ctypes.POINTER(i32),
                                      ctypes.POINTER(ctypes.c_double), i32]
    lib.ob_profile_enable.argtypes = [i32]
    lib.ob_profile_enable.restype = None
    lib.ob_profile_reset.argtypes = []
    lib.ob_profile_reset.restype = None
    lib.ob_profile_read.argtypes = [i32, ctypes.POINTER(ctypes.c_double),
                                    ctypes.POINTER(ctypes.c_longlong)]
    lib.ob_flash_dsum_bf16.argtypes = [vp, vp, vp, i64, i64, i64, i64, vp]
    lib.ob_flash_bwd_bf16.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i64,
                                      i64, i64, i64, f32, vp]
    lib.ob_flash_fwd_nt_bf16.argtypes = [vp, vp, vp, i64, i64, i64, i64,
                                         f32, vp]
    lib.ob_flash_bwd_nt_bf16.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64,
                                         i64, i64, f32, vp]
    lib.ob_flash_bwd_nt_d_bf16.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64,
                                           i64, i64, i64, f32, vp]
    # (seed, layer_id, tick, p): the site is always DROP_ATTN
    lib.ob_flash_fwd_nt_drop_bf16.argtypes = [vp, vp, vp, i64, i64, i64, i64,
                                              f32, u64, i32, u64, f32, vp]
    lib.ob_flash_bwd_nt_d_drop_bf16.argtypes = [vp, vp, vp, vp, vp, vp, vp,
                                                i64, i64, i64, i64, f32, u64,
                                                i32, u64, f32, vp]
    # deterministic mode (include/oobleck_stage.h)
    lib.ob_set_deterministic.argtypes = [i32]
    lib.ob_deterministic.argtypes = []
    lib.ob_det_ws_count.argtypes = [i32, i64, i64]
    lib.ob_det_ws_count.restype = i64
    lib.ob_colsum_det_bf16.argtypes = [vp, vp, i64, i64, vp, vp]
    lib.ob_gelu_bwd_colsum_det_bf16.argtypes = [vp, vp, vp, vp, i64, i64, vp,
                                                vp]
    lib.ob_layernorm_bwd_res_det_bf16.argtypes = [vp, vp, vp, vp, vp, vp, vp,
                                                  vp, vp, vp, vp, i64, i64,
                                                  vp, vp]
    lib.ob_dropout_scale_colsum_det_bf16.argtypes = key + [vp, vp, vp, i64,
                                                           i64, vp, vp]
    lib.ob_ce_fwd_det_bf16.argtypes = [vp, vp, vp, vp, i64, i64, i64, i64,
                                       vp, vp]
    lib.ob_embed_bwd_det_bf16.argtypes = [vp, vp, vp, vp, i64, i64, i64, vp]
    lib.ob_embed_bwd_drop_det_bf16.argtypes = key + [vp, vp, vp, vp, i64,
                                                     i64, i64, vp]
    lib.ob_colpart_finish_f32.argtypes = [vp, i64, i64, i64, vp, vp]
    p64 = ctypes.POINTER(ctypes.c_int64)
    lib.ob_flash_fold_rows.argtypes = [i64, i64, i64, i64, p64, p64, p64]
    lib.ob_flash_fold_grid.argtypes = [i64, i64, i64]
    lib.ob_flash_fold_grid.restype = ctypes.c_int64
    lib.ob_flash_fold_id.argtypes = [i64, i64, i64, i64, p64, p64]
    return lib


def get_ext(build_if_missing: bool = True) -> ctypes.CDLL:
    """Load (building in-tree if necessary) the HIP extension.  Raises
    RuntimeError — loudly, no fallback — when unavailable."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not SO_PATH.exists():
        if build_if_missing:
            from .build import build
            try:
                build()
            except Exception as e:  # noqa: BLE001
                raise RuntimeError(
                    f"oobleck_amd: HIP extension missing and build failed: {e}. "
                    "The hot path has no fallback — run __graft_entry__.build().") from e
        else:
            raise RuntimeError(
                "oobleck_amd: HIP extension libob_stage.so is missing. "
                "The hot path has no fallback — run __graft_entry__.build().")
    _LIB = _configure(ctypes.CDLL(str(SO_PATH)))
    return _LIB


LT_SHAPE_FIELDS = 13
LT_SHAPE_NAMES = ("tA", "tB", "M", "N", "K", "lda", "ldb", "ldc", "c_f32",
                  "beta1", "bias", "cin", "ab_f32")


def lt_shape(tA, tB, M, N, K, lda, ldb, ldc, c_f32=0, beta1=0, bias=0, cin=0,
             ab_f32=0):
    """One library GEMM shape as the int64 array the ob_gemm_lt_* queries
    take (include/oobleck_stage.h)."""
    return (ctypes.c_int64 * LT_SHAPE_FIELDS)(tA, tB, M, N, K, lda, ldb, ldc,
                                              c_f32, beta1, bias, cin, ab_f32)


def layer_lt_shapes(desc: ObLayerDesc) -> list[tuple]:
    """The library GEMM shapes ob_layer_create tunes for a description."""
    lib = get_ext()
    n = lib.ob_layer_lt_shapes(ctypes.byref(desc), None, 0)
    if n < 0:
        raise RuntimeError("ob_layer_lt_shapes failed")
    buf = (ctypes.c_int64 * (LT_SHAPE_FIELDS * max(n, 1)))()
    lib.ob_layer_lt_shapes(ctypes.byref(desc), buf, n)
    return [tuple(buf[i * LT_SHAPE_FIELDS:(i + 1) * LT_SHAPE_FIELDS])
            for i in range(n)]


def lt_choice(shape) -> dict | None:
    """The choice table's entry for a shape, or None."""
    out = (ctypes.c_double * 10)()
    top1 = ctypes.create_string_buffer(512)
    chosen = ctypes.create_string_buffer(512)
    check(get_ext().ob_gemm_lt_choice(lt_shape(*shape), out, top1, chosen, 512),
          "gemm_lt_choice")
    if not out[0]:
        return None
    return {"index": int(out[1]), "tuned": bool(out[2]),
            "top1_index": int(out[3]), "us_top1": out[4], "us_chosen": out[5],
            "tried": int(out[6]), "dropped": int(out[7]), "wall_ms": out[8],
            "spread_top1": out[9],
            "top1_kernel": top1.value.decode(),
            "chosen_kernel": chosen.value.decode()}


def lt_candidates(shape, cap: int = 128) -> list[dict]:
    """The candidates the tuner timed for a shape, fastest first."""
    idx, pos = (ctypes.c_int32 * cap)(), (ctypes.c_int32 * cap)()
    us = (ctypes.c_double * cap)()
    n = get_ext().ob_gemm_lt_candidates(lt_shape(*shape), idx, pos, us, cap)
    return [{"index": idx[i], "pos": pos[i], "us": us[i]}
            for i in range(max(0, min(n, cap)))]


def dw_slices_admit(shape, s: int, cus: int, slab_floats: int) -> bool:
    """The rule of ob_dw_slices.h: may this shape run as s K-slices on a
    device of cus CUs with a slab of slab_floats floats?  No GPU call."""
    return bool(get_ext().ob_dw_slices_admit(lt_shape(*shape), s, cus,
                                             slab_floats))


def lt_slices(shape, cap: int = 32) -> dict | None:
    """The sliced side of a shape's table entry (ob_gemm_lt_slices), or
    None."""
    out = (ctypes.c_double * 6)()
    sl, idx = (ctypes.c_int32 * cap)(), (ctypes.c_int32 * cap)()
    us = (ctypes.c_double * cap)()
    n = get_ext().ob_gemm_lt_slices(lt_shape(*shape), out, sl, idx, us, cap)
    if n < 0 or not out[0]:
        return None
    return {"slices": int(out[1]), "slice_index": int(out[2]),
            "us_sliced": out[3], "added_ms": out[4],
            "fastest_slices": int(out[5]),
            "pairs": [{"slices": sl[i], "index": idx[i], "us": us[i]}
                      for i in range(min(n, cap))]}


# ob_layer_plan_query's fields, in order (include/oobleck_stage.h)
PLAN_STASH = ("x", "mean1", "rstd1", "ln1", "qkv", "p", "attnm", "hmid",
              "mean2", "rstd2", "ln2", "u", "g", "logits", "lse")
PLAN_SHADOWS = ("qkv", "qkv_t", "ap", "ap_t", "fc", "fc_t", "mp", "mp_t",
                "lm", "lm_t")
PLAN_WS = ("dp", "dln", "datt", "dqkv", "dy4", "flash_bwd", "flash_vt",
           "dw_a", "dw_b", "pd_fwd", "pd_bwd", "dm_attn", "dm_mlp",
           "det_main", "det_side", "det_fwd")
LAYER_PLAN_NAMES = (
    ("flash", "side", "v_pad", "slot_stride", "ids_count", "shadow_count")
    + tuple(f"st_off_{n}" for n in PLAN_STASH)
    + tuple(f"st_len_{n}" for n in PLAN_STASH)
    + tuple(f"sh_off_{n}" for n in PLAN_SHADOWS)
    + tuple(f"ws_{n}" for n in PLAN_WS)
    + ("pk_qt", "pk_kt", "pk_dot", "pk_d"))
# bits of ob_layer_plan_query's modes
PLAN_DET, PLAN_BF16_FLASH, PLAN_FLASH_TR, PLAN_FLASH_DROP, PLAN_FLASH_HD128 = (
    1, 2, 4, 8, 16)


def layer_plan(desc: ObLayerDesc, drop: ObDropoutDesc | None = None,
               modes: int = -1) -> dict:
    """The device memory ob_layer_create_ex takes for a description: stash
    layout, shadows and the share of the workspace (DESIGN.md "Layer
    memory").  No GPU call."""
    n = len(LAYER_PLAN_NAMES)
    buf = (ctypes.c_int64 * n)()
    got = get_ext().ob_layer_plan_query(
        ctypes.byref(desc), ctypes.byref(drop) if drop else None, modes, buf,
        n)
    if got != n:
        raise RuntimeError(f"ob_layer_plan_query returned {got}, not {n}")
    return dict(zip(LAYER_PLAN_NAMES, buf))


# which-codes of ob_det_ws_count (OB_DET_WS_* of include/oobleck_stage.h)
DET_WS_COLSUM, DET_WS_GELU, DET_WS_LN, DET_WS_DROP_CS, DET_WS_CE = range(5)


def set_deterministic(on: bool) -> None:
    """Turn the process-wide deterministic mode on or off (default: the
    environment's OB_DETERMINISTIC=1).  Raises once a layer has been created
    in this process."""
    check(get_ext().ob_set_deterministic(1 if on else 0), "set_deterministic")


def deterministic() -> bool:
    return bool(get_ext().ob_deterministic())


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        err = get_ext().ob_last_error().decode()
        raise RuntimeError(f"oobleck_amd extension error in {what}: {err}")
