# CPU: the plan of a head_dim 128 layer with attention dropout under the
# PLAN_FLASH_HD128_DROP mode bit (OB_FLASH_HD128_DROP, off by default;
# oobleck_amd/csrc/ob_layer_plan.h).  Host calls only; modes are passed as
# bits, so the environment's switches play no part.
import pytest

from oobleck_amd._ext import (PLAN_FLASH_DROP, PLAN_FLASH_HD128,
                              PLAN_FLASH_HD128_DROP, PLAN_FLASH_TR, PLAN_WS)
from tests.test_layer_plan import BF16, BLOCK, DEFAULT, _plan

ON = DEFAULT | PLAN_FLASH_HD128_DROP


def _hd128(attn, modes):
    return _plan(BLOCK, 256, 2, 128, BF16, attn=attn, modes=modes)


def test_bit_is_appended():
    assert PLAN_FLASH_HD128_DROP == 32 and not DEFAULT & PLAN_FLASH_HD128_DROP


def test_hd128_attn_drop_is_the_p0_flash_plan():
    got, plain = _hd128(0.1, ON), _hd128(0.0, DEFAULT)
    assert got["flash"] == 1 and plain["flash"] == 1
    # the LSE [B*nh, S] where a materialized layer keeps P [B*nh, S, S]
    assert got["st_len_p"] == 2 * 2 * 128
    assert got["ws_pd_fwd"] == 0 and got["ws_pd_bwd"] == 0
    assert got["ws_dp"] == 0
    for n in PLAN_WS:
        assert got[f"ws_{n}"] == plain[f"ws_{n}"], n
    assert got["slot_stride"] == plain["slot_stride"]


@pytest.mark.parametrize("cleared", [PLAN_FLASH_TR, PLAN_FLASH_DROP,
                                     PLAN_FLASH_HD128, PLAN_FLASH_HD128_DROP])
def test_hd128_attn_drop_needs_every_switch(cleared):
    got = _hd128(0.1, ON & ~cleared)
    assert got["flash"] == 0
    assert got["st_len_p"] == 2 * 2 * 128 * 128
    assert got["ws_pd_fwd"] == got["ws_pd_bwd"] == 2 * 2 * 128 * 128
