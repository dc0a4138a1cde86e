# CPU: locally banded attention in the config and the layer plan
# (ModelConfig.layer_attn_window, ob_layer_desc.attn_window,
# oobleck_amd/csrc/ob_layer_plan.h).  Host calls only; modes are passed as
# bits, so the environment's switches play no part.
import pytest

from oobleck_amd import _ext
from oobleck_amd._ext import (PLAN_BF16_FLASH, PLAN_FLASH_DROP,
                              PLAN_FLASH_HD128, PLAN_FLASH_TR, ObDropoutDesc,
                              ObLayerDesc)
from oobleck_amd.config import ModelConfig

BLOCK, F32, BF16 = 1, 0, 1
B, S = 2, 256
DEFAULT = PLAN_BF16_FLASH | PLAN_FLASH_TR | PLAN_FLASH_DROP | PLAN_FLASH_HD128


def _plan(H, nh, window, S=S, dtype=BF16, attn=0.0, modes=DEFAULT):
    desc = ObLayerDesc(kind=BLOCK, n_embd=H, n_head=nh, n_positions=S,
                       vocab_size=304, max_batch=B, seq_len=S, n_slots=2,
                       dtype=dtype, attn_window=window)
    drop = ObDropoutDesc(attn_pdrop=attn, layer_id=1, seed=3) if attn else None
    return _ext.layer_plan(desc, drop, modes)


@pytest.mark.parametrize("every,banded", [(1, [1, 2, 3, 4, 5, 6]),
                                          (2, [2, 4, 6]), (3, [3, 6])])
def test_layer_attn_window(every, banded):
    """6 blocks are layers 1..6; layer 0 is EMBED, layer 7 FINAL."""
    cfg = ModelConfig(n_layer=6, attn_window=256, attn_window_every=every)
    got = [cfg.layer_attn_window(lid) for lid in range(cfg.n_layers_total)]
    assert got == [256 if lid in banded else 0 for lid in range(8)]
    dense = ModelConfig(n_layer=6, attn_window_every=every)
    assert not any(dense.layer_attn_window(lid) for lid in range(8))


@pytest.mark.parametrize("H,nh", [(128, 2), (256, 2)])
def test_windowed_plan_is_the_dense_flash_plan(H, nh):
    dense = _plan(H, nh, 0)
    p = _plan(H, nh, 64)
    assert p["flash"] == 1
    assert p["st_len_p"] == B * nh * S
    assert p["ws_dp"] == 0
    assert p == dense
    # window >= S is the dense layer, whatever else the description says
    assert _plan(H, nh, S) == dense and _plan(H, nh, 10 * S) == dense
    assert _plan(H, nh, S, attn=0.1) == _plan(H, nh, 0, attn=0.1)


@pytest.mark.parametrize("kw", [
    dict(H=128, nh=2, dtype=F32),
    dict(H=192, nh=2),                      # head_dim 96
    dict(H=128, nh=2, S=192),               # S % 128 != 0
    dict(H=128, nh=2, modes=DEFAULT & ~PLAN_FLASH_TR),
    dict(H=256, nh=2, modes=DEFAULT & ~PLAN_FLASH_HD128),
    dict(H=128, nh=2, attn=0.1),
    dict(H=128, nh=2, window=-1),
], ids=["f32", "hd96", "s192", "tr0", "hd128_off", "attn_pdrop", "negative"])
def test_windowed_plan_refused(kw):
    kw.setdefault("window", 64)
    with pytest.raises(RuntimeError, match="returned -1"):
        _plan(**kw)
    assert b"attn_window" in _ext.get_ext().ob_last_error()
    # the same description without a window has a plan
    _plan(**dict(kw, window=0))
