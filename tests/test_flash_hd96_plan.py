# CPU: the plan of a head_dim 80 / 96 layer under the PLAN_FLASH_HD96 mode
# bit (OB_FLASH_HD96, off by default; oobleck_amd/csrc/ob_layer_plan.h), dense
# and banded, and the GPT-3 760M / 2.7B presets.  Host calls only; modes are
# passed as bits, so the environment's switches play no part.
import os

import pytest

from oobleck_amd import _ext
from oobleck_amd._ext import PLAN_FLASH_HD96, PLAN_FLASH_TR
from tests.test_flash_eligible import _eligible
from tests.test_flash_window_plan import DEFAULT, B, S, _plan

ON = DEFAULT | PLAN_FLASH_HD96
DIMS = pytest.mark.parametrize("H,nh", [(160, 2), (192, 2)])


def _refused(**kw):
    with pytest.raises(RuntimeError, match="returned -1"):
        _plan(**kw)
    assert b"attn_window" in _ext.get_ext().ob_last_error()


@DIMS
def test_with_the_bit_it_is_the_dense_flash_plan(H, nh):
    assert PLAN_FLASH_HD96 == 64 and not DEFAULT & PLAN_FLASH_HD96
    dense = _plan(H, nh, 0, modes=ON)
    assert dense["flash"] == 1
    assert dense["st_len_p"] == B * nh * S
    assert dense["ws_dp"] == 0
    assert _plan(H, nh, 64, modes=ON) == dense
    assert _plan(H, nh, S, modes=ON) == dense
    assert _plan(H, nh, 10 * S, modes=ON) == dense


@DIMS
def test_attention_dropout_stays_off_the_route(H, nh):
    assert _plan(H, nh, 0, attn=0.1, modes=ON)["flash"] == 0
    _refused(H=H, nh=nh, window=64, attn=0.1, modes=ON)


@DIMS
def test_without_the_bit_nothing_changes(H, nh):
    p = _plan(H, nh, 0)
    assert p["flash"] == 0 and p["st_len_p"] == B * nh * S * S
    _refused(H=H, nh=nh, window=64)
    # the bit needs the production path
    assert _plan(H, nh, 0, modes=ON & ~PLAN_FLASH_TR)["flash"] == 0
    # this process's switch is unset
    assert "OB_FLASH_HD96" not in os.environ
    assert _eligible(H, nh, S) == 0


def test_gpt3_presets_have_head_dim_96_and_80():
    from oobleck_amd.config import GPT3_2_7B, GPT3_760M
    for cfg, dims, hd in ((GPT3_760M, (1536, 16, 24), 96),
                          (GPT3_2_7B, (2560, 32, 32), 80)):
        assert (cfg.n_embd, cfg.n_head, cfg.n_layer) == dims
        assert cfg.n_embd // cfg.n_head == hd and cfg.n_embd % cfg.n_head == 0
        assert cfg.n_positions == 2048
