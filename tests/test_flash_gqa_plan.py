# CPU: grouped-query attention in the layer plan (ob_layer_desc.n_kv_head,
# oobleck_amd/csrc/ob_layer_plan.h), the parameter count and the dK/dV split
# rule.  Host calls only.
import ctypes
import dataclasses

import pytest

from oobleck_amd import _ext
from oobleck_amd._ext import ObLayerDesc
from oobleck_amd.config import SANTACODER
from oobleck_amd.params import KIND_BLOCK, layer_param_numel

BLOCK, BF16 = 1, 1
B, S, H, NH = 2, 2048, 2048, 16


def _desc(n_kv, H=H, nh=NH):
    return ObLayerDesc(kind=BLOCK, n_embd=H, n_head=nh, n_positions=S,
                       vocab_size=304, max_batch=B, seq_len=S, n_slots=2,
                       dtype=BF16, n_kv_head=n_kv)


@pytest.mark.parametrize("n_kv", [0, 1, 4, NH])
def test_param_count_is_the_python_spec(n_kv):
    cfg = dataclasses.replace(SANTACODER, n_kv_head=n_kv)
    n = _ext.get_ext().ob_layer_param_count(ctypes.byref(_desc(n_kv)))
    assert n == layer_param_numel(cfg, KIND_BLOCK)
    W = H + 2 * 128 * n_kv if 0 < n_kv < NH else 3 * H
    assert n == 9 * H * H + H * W + W + 10 * H


def test_plan_widths():
    base = _ext.layer_plan(_desc(0))
    assert _ext.layer_plan(_desc(NH)) == base
    assert base["st_len_qkv"] == base["ws_dqkv"] == B * S * 3 * H
    p = _ext.layer_plan(_desc(1))
    W = H + 2 * 128
    assert p["flash"] == 1
    assert p["st_len_qkv"] == p["ws_dqkv"] == B * S * W
    assert p["sh_off_qkv_t"] - p["sh_off_qkv"] == H * W
    assert p["sh_off_ap"] - p["sh_off_qkv_t"] == H * W
    assert p["ws_flash_bwd"] >= B * NH * S
    shapes = _ext.layer_lt_shapes(_desc(1))
    names = _ext.LT_SHAPE_NAMES
    n_of = {dict(zip(names, s))["N"] for s in shapes}
    assert W in n_of and 3 * H not in n_of


def test_eligibility():
    lib = _ext.get_ext()
    assert lib.ob_flash_eligible(ctypes.byref(_desc(1)), 0.0) == 1
    assert lib.ob_flash_eligible(ctypes.byref(_desc(1, H=1024)), 0.0) == 0
    with pytest.raises(RuntimeError, match="returned -1"):
        _ext.layer_plan(_desc(1, H=1024))  # head_dim 64
    assert b"n_kv_head" in lib.ob_last_error()
    with pytest.raises(RuntimeError, match="returned -1"):
        _ext.layer_plan(_desc(3))  # 16 % 3
    assert b"n_kv_head" in lib.ob_last_error()


@pytest.mark.parametrize("B,S,nh,n_kv", [(2, 2048, 16, 1), (2, 2048, 32, 8),
                                         (1, 128, 6, 2), (8, 2048, 16, 2)])
@pytest.mark.parametrize("cus", [64, 256, 304])
def test_split_rule(B, S, nh, n_kv, cus):
    s = _ext.get_ext().ob_flash_gqa_split(B, S, nh, n_kv, cus)
    assert s >= 1 and (nh // n_kv) % s == 0
    if B * n_kv * (S // 64) >= cus:
        assert s == 1
