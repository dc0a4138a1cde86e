# CPU: bidirectional attention in the layer plan (ob_layer_desc.attn_bidir,
# oobleck_amd/csrc/ob_layer_plan.h).  Host calls only; the query takes the
# modes as bits, ob_flash_eligible this process's.
import ctypes

import pytest

from oobleck_amd import _ext
from oobleck_amd._ext import PLAN_FLASH_TR, ObDropoutDesc, ObLayerDesc

BLOCK, F32, BF16 = 1, 0, 1
B, S = 2, 256
DEFAULT = (_ext.PLAN_BF16_FLASH | PLAN_FLASH_TR | _ext.PLAN_FLASH_DROP
           | _ext.PLAN_FLASH_HD128)


def _desc(H=128, nh=2, S=S, dtype=BF16, window=0, bidir=1):
    return ObLayerDesc(kind=BLOCK, n_embd=H, n_head=nh, n_positions=S,
                       vocab_size=304, max_batch=B, seq_len=S, n_slots=2,
                       dtype=dtype, attn_window=window, attn_bidir=bidir)


def _plan(attn=0.0, modes=DEFAULT, **kw):
    drop = ObDropoutDesc(attn_pdrop=attn, layer_id=1, seed=3) if attn else None
    return _ext.layer_plan(_desc(**kw), drop, modes)


def _eligible(attn=0.0, **kw):
    return _ext.get_ext().ob_flash_eligible(ctypes.byref(_desc(**kw)), attn)


def test_bidir_plan_is_the_causal_flash_plan():
    p = _plan()
    assert p["flash"] == 1 and p["st_len_p"] == B * 2 * S and p["ws_dp"] == 0
    assert p == _plan(bidir=0)
    assert _plan(window=S) == p  # a window >= S is no window
    assert _eligible() == 1


# each with the `flash` the causal layer of the same description has had
@pytest.mark.parametrize("kw,causal_flash", [
    (dict(H=256, nh=2), 1),          # head_dim 128
    (dict(S=192), 0),
    (dict(attn=0.1), 1),
    (dict(window=64), 1),
    (dict(dtype=F32), 0),
    (dict(modes=DEFAULT & ~PLAN_FLASH_TR), 1),
], ids=["hd128", "s192", "attn_pdrop", "window", "f32", "tr0"])
def test_bidir_plan_refused(kw, causal_flash):
    with pytest.raises(RuntimeError, match="returned -1"):
        _plan(**kw)
    assert b"attn_bidir" in _ext.get_ext().ob_last_error()
    # attn_bidir = 0 answers as before
    assert _plan(bidir=0, **kw)["flash"] == causal_flash
    # ob_flash_eligible reads this process's modes, not the bits
    if "modes" not in kw:
        assert _eligible(**kw) == 0
        assert _eligible(bidir=0, **kw) == causal_flash
