# CPU: document-masked attention in the layer plan
# (ob_layer_desc.attn_segments, oobleck_amd/csrc/ob_layer_plan.h).  Host calls
# only; the query takes the modes as bits, ob_flash_eligible this process's.
import ctypes

import pytest

from oobleck_amd import _ext
from oobleck_amd._ext import ObDropoutDesc, ObLayerDesc

BLOCK, F32, BF16 = 1, 0, 1
B, S, SLOTS = 2, 256, 3
DEFAULT = (_ext.PLAN_BF16_FLASH | _ext.PLAN_FLASH_TR | _ext.PLAN_FLASH_DROP
           | _ext.PLAN_FLASH_HD128)


def _desc(H=128, nh=2, S=S, dtype=BF16, seg=1, **kw):
    return ObLayerDesc(kind=BLOCK, n_embd=H, n_head=nh, n_positions=S,
                       vocab_size=304, max_batch=B, seq_len=S, n_slots=SLOTS,
                       dtype=dtype, attn_segments=seg, **kw)


def _plan(attn=0.0, **kw):
    drop = ObDropoutDesc(attn_pdrop=attn, layer_id=1, seed=3) if attn else None
    return _ext.layer_plan(_desc(**kw), drop, DEFAULT)


def _eligible(attn=0.0, **kw):
    return _ext.get_ext().ob_flash_eligible(ctypes.byref(_desc(**kw)), attn)


@pytest.mark.parametrize("H,nh", [(128, 2), (256, 2)], ids=["hd64", "hd128"])
def test_seg_plan_is_the_flash_plan_plus_bounds(H, nh):
    p, plain = _plan(H=H, nh=nh), _plan(H=H, nh=nh, seg=0)
    assert p["flash"] == 1 and plain["flash"] == 1
    assert p["ids_count"] == B * S * SLOTS and plain["ids_count"] == 0
    assert {**p, "ids_count": 0} == plain
    assert _eligible(H=H, nh=nh) == 1


@pytest.mark.parametrize("kw", [
    dict(dtype=F32), dict(H=192, nh=2), dict(S=96), dict(attn=0.1),
    dict(attn_window=64), dict(attn_bidir=1), dict(n_kv_head=1),
], ids=["f32", "hd96", "s96", "attn_pdrop", "window", "bidir", "mqa"])
def test_seg_plan_refused(kw):
    with pytest.raises(RuntimeError, match="returned -1"):
        _plan(**kw)
    assert b"attn_segments" in _ext.get_ext().ob_last_error()
    assert _eligible(**kw) == 0
