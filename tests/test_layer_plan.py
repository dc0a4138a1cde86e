# CPU: ob_layer_plan_query — the device memory ob_layer_create_ex takes for a
# description (stash layout, shadows, share of the process-wide workspace),
# from the table the create itself allocates by
# (oobleck_amd/csrc/ob_layer_plan.h, DESIGN.md "Layer memory").  Host calls
# only.  The expected numbers are written out here from the size rules; the
# modes are passed as bits, so the environment's switches play no part.
import ctypes

import pytest

from oobleck_amd import _ext
from oobleck_amd._ext import (PLAN_BF16_FLASH, PLAN_DET, PLAN_FLASH_DROP,
                              PLAN_FLASH_HD128, PLAN_FLASH_TR, PLAN_SHADOWS,
                              PLAN_STASH, PLAN_WS, ObDropoutDesc, ObLayerDesc)

EMBED, BLOCK, FINAL = 0, 1, 2
F32, BF16 = 0, 1
B, SLOTS = 2, 2
DEFAULT = PLAN_BF16_FLASH | PLAN_FLASH_TR | PLAN_FLASH_DROP | PLAN_FLASH_HD128
DET_SLABS = ("det_main", "det_side", "det_fwd")


def _lib():
    try:
        return _ext.get_ext()
    except RuntimeError as e:
        pytest.fail(f"extension must build on CPU via hipcc: {e}")


def _desc(kind, H, nh, S, dtype, V=304):
    return ObLayerDesc(kind=kind, n_embd=H, n_head=nh, n_positions=max(S, 128),
                       vocab_size=V, max_batch=B, seq_len=S, n_slots=SLOTS,
                       dtype=dtype)


def _plan(kind, H, nh, S, dtype, V=304, resid=0.0, attn=0.0, modes=DEFAULT):
    _lib()
    drop = None
    if resid or attn:
        drop = ObDropoutDesc(embd_pdrop=0.0, resid_pdrop=resid,
                             attn_pdrop=attn, layer_id=1, seed=3)
    return _ext.layer_plan(_desc(kind, H, nh, S, dtype, V), drop, modes)


def _ws(plan):
    """The workspace buffers the plan asks for, by name."""
    return {n: plan[f"ws_{n}"] for n in PLAN_WS if plan[f"ws_{n}"]}


def _stash(plan):
    """(name, offset, length) of the regions the layer has, in slot order."""
    return [(n, plan[f"st_off_{n}"], plan[f"st_len_{n}"]) for n in PLAN_STASH
            if plan[f"st_len_{n}"]]


def _block_lengths(H, nh, S, flash):
    BS = B * S
    BSH = BS * H
    return [("x", BSH), ("mean1", BS), ("rstd1", BS), ("ln1", BSH),
            ("qkv", 3 * BSH), ("p", B * nh * S if flash else B * nh * S * S),
            ("attnm", BSH), ("hmid", BSH), ("mean2", BS), ("rstd2", BS),
            ("ln2", BSH), ("u", 4 * BSH), ("g", 4 * BSH)]


def _check_layout(plan, lengths):
    """Regions in the documented order, back to back from 0, and the slot
    stride at the last one's end."""
    o = 0
    got = _stash(plan)
    assert [n for n, _, _ in got] == [n for n, _ in lengths]
    for (name, off, length), (_, want) in zip(got, lengths):
        assert (off, length) == (o, want), name
        o += want
    assert plan["slot_stride"] == o


def _half(n_bf16):
    return (n_bf16 + 1) // 2


# every case of this file, for the invariants at the bottom
CASES = {
    "f32_block": dict(kind=BLOCK, H=48, nh=2, S=48, dtype=F32),
    "matp": dict(kind=BLOCK, H=128, nh=2, S=96, dtype=BF16),
    "hd64": dict(kind=BLOCK, H=128, nh=2, S=128, dtype=BF16),
    "hd128": dict(kind=BLOCK, H=256, nh=2, S=128, dtype=BF16),
    "hd64_tr0": dict(kind=BLOCK, H=128, nh=2, S=128, dtype=BF16,
                     modes=DEFAULT & ~PLAN_FLASH_TR),
    "hd128_off": dict(kind=BLOCK, H=256, nh=2, S=128, dtype=BF16,
                      modes=DEFAULT & ~PLAN_FLASH_HD128),
    "hd128_tr0": dict(kind=BLOCK, H=256, nh=2, S=128, dtype=BF16,
                      modes=DEFAULT & ~PLAN_FLASH_TR),
    "hd128_attn": dict(kind=BLOCK, H=256, nh=2, S=128, dtype=BF16, attn=0.1),
    "matp_resid": dict(kind=BLOCK, H=128, nh=2, S=96, dtype=BF16, resid=0.1),
    "matp_attn": dict(kind=BLOCK, H=128, nh=2, S=96, dtype=BF16, attn=0.1),
    "hd64_attn": dict(kind=BLOCK, H=128, nh=2, S=128, dtype=BF16, attn=0.1),
    "hd64_det": dict(kind=BLOCK, H=128, nh=2, S=128, dtype=BF16,
                     modes=DEFAULT | PLAN_DET),
    "hd64_det_resid": dict(kind=BLOCK, H=128, nh=2, S=128, dtype=BF16,
                           resid=0.1, modes=DEFAULT | PLAN_DET),
    "final_det": dict(kind=FINAL, H=128, nh=2, S=128, dtype=BF16,
                      modes=DEFAULT | PLAN_DET),
    "final_v304": dict(kind=FINAL, H=128, nh=2, S=128, dtype=BF16, V=304),
    "final_v100": dict(kind=FINAL, H=128, nh=2, S=128, dtype=BF16, V=100),
    "final_f32_v100": dict(kind=FINAL, H=128, nh=2, S=128, dtype=F32, V=100),
    "embed": dict(kind=EMBED, H=128, nh=2, S=128, dtype=BF16),
}


def test_fp32_block():
    H, nh, S = 48, 2, 48
    BS, BSH = B * S, B * S * H
    p = _plan(**CASES["f32_block"])
    _check_layout(p, _block_lengths(H, nh, S, flash=False))
    assert p["shadow_count"] == 0
    assert _ws(p) == {"dp": B * nh * S * S, "dqkv": 3 * BSH, "dy4": 4 * BSH,
                      "dln": BSH, "datt": BSH}
    assert (p["flash"], p["side"], p["ids_count"]) == (0, 0, 0)


def test_bf16_block_materialized_p():
    H, nh, S = 128, 2, 96
    BS, BSH = B * S, B * S * H
    p = _plan(**CASES["matp"])
    _check_layout(p, _block_lengths(H, nh, S, flash=False))
    assert p["st_len_p"] == B * nh * S * S
    # nothing of this layer touches the flash buffers
    assert p["ws_flash_bwd"] == 0 and p["ws_flash_vt"] == 0
    assert _ws(p) == {"dp": B * nh * S * S, "dqkv": 3 * BSH, "dy4": 4 * BSH,
                      "dln": BSH, "datt": BSH,
                      "dw_a": _half(4 * H * BS), "dw_b": _half(4 * H * BS)}
    assert (p["flash"], p["side"]) == (0, 1)
    # shadows: plain and transposed, back to back
    sizes = [3 * H * H] * 2 + [H * H] * 2 + [4 * H * H] * 4
    o = 0
    for name, n in zip(PLAN_SHADOWS, sizes):
        assert p[f"sh_off_{name}"] == o, name
        o += n
    assert p["shadow_count"] == o == 24 * H * H


@pytest.mark.parametrize("case,H", [("hd64", 128), ("hd128", 256)])
def test_bf16_block_flash(case, H):
    nh, S = 2, 128
    BS, BSH = B * S, B * S * H
    p = _plan(**CASES[case])
    assert p["flash"] == 1
    _check_layout(p, _block_lengths(H, nh, S, flash=True))
    assert p["st_len_p"] == B * nh * S
    # only D of the flash backward; no dp, no V^T
    assert _ws(p) == {"dqkv": 3 * BSH, "dy4": 4 * BSH, "dln": BSH,
                      "datt": BSH, "flash_bwd": B * nh * S,
                      "dw_a": _half(4 * H * BS), "dw_b": _half(4 * H * BS)}
    assert (p["pk_qt"], p["pk_kt"], p["pk_dot"], p["pk_d"]) == (0, 0, 0, 0)


def test_flash_tr_off_packs_the_transposes():
    H, nh, S = 128, 2, 128
    BS, BSH = B * S, B * S * H
    p = _plan(**CASES["hd64_tr0"])
    assert p["flash"] == 1 and p["ws_dp"] == 0
    assert p["ws_flash_bwd"] == _half(4 * H * BS)
    assert p["ws_flash_vt"] == _half(4 * H * BS)
    # Q^T | K^T | dO^T (bf16) then D (floats), inside flash_bwd
    assert (p["pk_qt"], p["pk_kt"], p["pk_dot"]) == (0, BSH, 2 * BSH)
    assert 2 * p["pk_d"] >= 3 * BSH
    assert p["pk_d"] + B * nh * S <= p["ws_flash_bwd"]
    # V^T fits the forward's buffer
    assert BSH <= 2 * p["ws_flash_vt"]


@pytest.mark.parametrize("case", ["hd128_off", "hd128_tr0", "hd128_attn"])
def test_head_dim_128_off_flash(case):
    nh, S = 2, 128
    p = _plan(**CASES[case])
    assert p["flash"] == 0
    assert p["st_len_p"] == B * nh * S * S == p["ws_dp"]
    assert p["ws_flash_bwd"] == 0 and p["ws_flash_vt"] == 0


def test_dropout_buffers():
    H, nh, S = 128, 2, 96
    BSH = B * S * H
    none = _ws(_plan(**CASES["matp"]))
    resid = _ws(_plan(**CASES["matp_resid"]))
    assert resid == {**none, "dm_attn": BSH, "dm_mlp": BSH}
    attn = _ws(_plan(**CASES["matp_attn"]))
    assert attn == {**none, "pd_fwd": B * nh * S * S, "pd_bwd": B * nh * S * S}
    # a flash layer draws its attention masks in the flash kernels
    fl = _plan(**CASES["hd64_attn"])
    assert fl["flash"] == 1
    assert _ws(fl) == _ws(_plan(**CASES["hd64"]))


def test_deterministic_slabs():
    lib = _lib()
    H, S = 128, 128
    BS = B * S

    def count(which, N):
        return lib.ob_det_ws_count(which, BS, N)

    base = _ws(_plan(**CASES["hd64"]))
    main = max(count(_ext.DET_WS_GELU, 4 * H), count(_ext.DET_WS_LN, H))
    side = count(_ext.DET_WS_COLSUM, 3 * H)
    assert main > 0 and side > 0
    assert _ws(_plan(**CASES["hd64_det"])) == {
        **base, "det_main": main, "det_side": side}
    main_r = max(main, count(_ext.DET_WS_DROP_CS, H))
    got = _ws(_plan(**CASES["hd64_det_resid"]))
    assert (got["det_main"], got["det_side"]) == (main_r, side)
    assert "det_fwd" not in got
    fin = _ws(_plan(**CASES["final_det"]))
    assert fin == {**_ws(_plan(**CASES["final_v304"])),
                   "det_main": count(_ext.DET_WS_LN, H),
                   "det_fwd": count(_ext.DET_WS_CE, 1)}


def test_bf16_final():
    H, S, V, v_pad = 128, 128, 304, 512
    BS, BSH = B * S, B * S * H
    p = _plan(**CASES["final_v304"])
    assert p["v_pad"] == v_pad
    _check_layout(p, [("x", BSH), ("mean1", BS), ("rstd1", BS), ("ln1", BSH),
                      ("logits", BS * V), ("lse", BS)])
    # no flash buffers, no attention grad; the dW_lm fallback's transposes
    assert _ws(p) == {"dln": BSH, "dw_a": _half(v_pad * BS),
                      "dw_b": _half(4 * H * BS)}
    assert (p["side"], p["ids_count"]) == (1, BS * SLOTS)
    assert (p["sh_off_lm"], p["sh_off_lm_t"]) == (0, v_pad * H)
    assert p["shadow_count"] == 2 * v_pad * H


def test_bf16_final_small_vocab_holds_its_padded_logits():
    S, V, v_pad = 128, 100, 256
    BS = B * S
    p = _plan(**CASES["final_v100"])
    assert p["v_pad"] == v_pad
    # the bf16 logits are [BS, v_pad] bf16: more than BS * V floats here
    assert p["st_len_logits"] >= _half(BS * v_pad) > BS * V
    assert p["st_off_lse"] >= p["st_off_logits"] + _half(BS * v_pad)
    assert p["st_len_logits"] == max(BS * V, _half(BS * v_pad))
    # fp32 logits are [BS, V] floats
    f = _plan(**CASES["final_f32_v100"])
    assert f["st_len_logits"] == BS * V
    assert _ws(f) == {"dln": BS * 128}
    assert (f["side"], f["shadow_count"]) == (0, 0)


def test_embed():
    p = _plan(**CASES["embed"])
    assert p["slot_stride"] == 0 and _stash(p) == []
    assert p["ids_count"] == B * 128 * SLOTS
    assert _ws(p) == {} and p["shadow_count"] == 0 and p["side"] == 0


@pytest.mark.parametrize("case", sorted(CASES))
def test_regions_do_not_overlap(case):
    p = _plan(**CASES[case])
    end = 0
    for name, off, length in _stash(p):
        assert off >= end, name       # non-decreasing, no overlap
        end = off + length
    assert p["slot_stride"] == end
    if not CASES[case].get("modes", 0) & PLAN_DET:
        assert all(p[f"ws_{n}"] == 0 for n in DET_SLABS)


def test_null_description():
    out = (ctypes.c_int64 * len(_ext.LAYER_PLAN_NAMES))()
    assert _lib().ob_layer_plan_query(None, None, -1, out, len(out)) == -1
