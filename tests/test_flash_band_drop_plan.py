# CPU: the plan of a layer with attention dropout that is banded or has
# head_dim 80 / 96, under the PLAN_FLASH_BAND_DROP mode bit (OB_FLASH_BAND_DROP,
# off by default; oobleck_amd/csrc/ob_layer_plan.h).  Host calls only; modes
# are passed as bits, so the environment's switches play no part.
import pytest

from oobleck_amd._ext import (PLAN_FLASH_BAND_DROP, PLAN_FLASH_DROP,
                              PLAN_FLASH_HD96, PLAN_FLASH_TR)
from tests.test_flash_hd96_plan import _refused
from tests.test_flash_window_plan import DEFAULT, F32, _plan

ON = DEFAULT | PLAN_FLASH_BAND_DROP
# (H, nh, window, further bits): hd 64, 128 banded; 80, 96 dense and banded
CELLS = pytest.mark.parametrize("H,nh,window,more", [
    (128, 2, 64, 0), (256, 2, 64, 0),
    (160, 2, 0, PLAN_FLASH_HD96), (160, 2, 64, PLAN_FLASH_HD96),
    (192, 2, 0, PLAN_FLASH_HD96), (192, 2, 64, PLAN_FLASH_HD96)])


@CELLS
def test_with_the_bit_it_is_the_p0_dense_flash_plan(H, nh, window, more):
    assert PLAN_FLASH_BAND_DROP == 128 and not DEFAULT & PLAN_FLASH_BAND_DROP
    p = _plan(H, nh, window, attn=0.1, modes=ON | more)
    assert p["flash"] == 1 and p["ws_pd_fwd"] == 0 and p["ws_pd_bwd"] == 0
    assert p == _plan(H, nh, 0, modes=ON | more)


@CELLS
def test_without_the_bit_nothing_changes(H, nh, window, more):
    if window:
        _refused(H=H, nh=nh, window=window, attn=0.1, modes=DEFAULT | more)
    else:
        assert _plan(H, nh, 0, attn=0.1, modes=DEFAULT | more)["flash"] == 0


@pytest.mark.parametrize("kw", [
    dict(dtype=F32), dict(S=192), dict(modes=ON & ~PLAN_FLASH_TR),
    dict(modes=ON & ~PLAN_FLASH_DROP)], ids=["f32", "s192", "tr0", "drop0"])
def test_still_refused_with_the_bit(kw):
    _refused(**{**dict(H=128, nh=2, window=64, attn=0.1, modes=ON), **kw})
