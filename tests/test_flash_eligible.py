# CPU: ob_flash_eligible — the decision ob_layer_create_ex takes about the
# fused flash attention path, for a description and an attn_pdrop, with no
# GPU call (oobleck_amd/csrc/ob_layer.hip) — and the GPT-3 presets it is
# there for.  Runs with the default switches (OB_FLASH_TR, OB_FLASH_DROP,
# OB_FLASH_HD128, OB_BF16_FLASH unset).
import ctypes

import pytest

BLOCK = 1
BF16, F32 = 1, 0


def _ext():
    from oobleck_amd._ext import get_ext
    try:
        return get_ext()
    except RuntimeError as e:
        pytest.fail(f"extension must build on CPU via hipcc: {e}")


def _eligible(n_embd, n_head, seq_len, dtype=BF16, attn_pdrop=0.0):
    from oobleck_amd._ext import ObLayerDesc
    d = ObLayerDesc(kind=BLOCK, n_embd=n_embd, n_head=n_head,
                    n_positions=max(seq_len, 128), vocab_size=304,
                    max_batch=1, seq_len=seq_len, n_slots=1, dtype=dtype)
    return _ext().ob_flash_eligible(ctypes.byref(d), attn_pdrop)


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for name in ("OB_FLASH_TR", "OB_FLASH_DROP", "OB_FLASH_HD128",
                 "OB_BF16_FLASH"):
        monkeypatch.delenv(name, raising=False)


def test_head_dim_64_and_128_are_eligible():
    assert _eligible(128, 2, 128) == 1      # head_dim 64
    assert _eligible(256, 2, 128) == 1      # head_dim 128
    assert _eligible(2176, 17, 128) == 1    # 128, an odd head count


@pytest.mark.parametrize("kw", [
    dict(n_embd=160, n_head=2, seq_len=128),              # head_dim 80
    dict(n_embd=200, n_head=3, seq_len=128),              # 200 % 3 != 0
    dict(n_embd=193, n_head=3, seq_len=128),              # 193 // 3 == 64
    dict(n_embd=256, n_head=2, seq_len=128, dtype=F32),   # fp32, hd 128
    dict(n_embd=128, n_head=2, seq_len=128, dtype=F32),   # fp32, hd 64
    dict(n_embd=256, n_head=2, seq_len=192),              # S % 128 != 0
    dict(n_embd=128, n_head=2, seq_len=192),
    dict(n_embd=256, n_head=2, seq_len=128, attn_pdrop=0.1),  # drop at 128
])
def test_not_eligible(kw):
    assert _eligible(**kw) == 0


def test_head_dim_64_keeps_its_dropout_kernels():
    assert _eligible(128, 2, 128, attn_pdrop=0.1) == 1


def test_null_description():
    assert _ext().ob_flash_eligible(None, 0.0) == 0


def test_gpt3_presets_have_head_dim_128():
    from oobleck_amd.config import GPT3_1_3B, GPT3_6_7B
    for cfg, width, heads, layers in ((GPT3_1_3B, 2048, 16, 24),
                                      (GPT3_6_7B, 4096, 32, 32)):
        assert (cfg.n_embd, cfg.n_head, cfg.n_layer) == (width, heads, layers)
        assert cfg.n_embd % cfg.n_head == 0
        assert cfg.n_embd // cfg.n_head == 128
        assert cfg.n_positions == 2048
        assert _eligible(cfg.n_embd, cfg.n_head, 1024) == 1
