# Model/training configuration for the hot path.
#
# Mirrors the reference's configs: examples/gpt2.yaml (GPT-2 small,
# microbatch 8, global microbatch 128) and examples/gpt3.yaml (GPT-2 XL dims:
# n_embd=1600, 48 layers, 25 heads, microbatch 2) —
# /root/reference/examples/*.yaml, elastic/training_util.py:7-39.
from __future__ import annotations

from dataclasses import dataclass


@dataclass
class ModelConfig:
    n_embd: int = 768
    n_head: int = 12
    n_layer: int = 12            # transformer blocks
    n_positions: int = 1024
    vocab_size: int = 50257
    # GPT-2's dropout probabilities (HF GPT2Config defaults are 0.1 each; the
    # reference trains with them).  0 = off: the dropout-free kernels run.
    embd_pdrop: float = 0.0
    resid_pdrop: float = 0.0
    attn_pdrop: float = 0.0
    # Locally banded attention (GPT-3's and GPT-Neo's "local" layers): a
    # banded block's query i sees the keys i - attn_window < j <= i.  0 = every
    # block dense.  Block b is banded when b % attn_window_every ==
    # attn_window_every - 1: every=2 alternates dense, banded, ... (GPT-Neo's
    # order), every=1 bands every block.
    attn_window: int = 0
    attn_window_every: int = 2
    # False: every block's attention is bidirectional (no causal mask), the
    # attention of an encoder (Megatron-BERT, ViT).  bf16 flash layers at
    # head_dim 64 with attn_pdrop == 0 and no window only.
    attn_causal: bool = True
    # K/V heads of every block.  0 (or n_head): one per query head.  0 <
    # n_kv_head < n_head: grouped-query attention (1: multi-query, GPT-BigCode),
    # n_head / n_kv_head query heads share a K/V head and the packed qkv width
    # is qkv_width.  bf16 flash layers at head_dim 128 with attn_pdrop == 0,
    # dense and causal, only.
    n_kv_head: int = 0
    # Packed sequences: >= 0 is the id of the token that ends a document.  The
    # token AFTER a separator starts a new document, every block is created
    # with attn_segments and a query attends the keys of its own document only
    # (block-diagonal causal attention).  -1: a row is one document.  bf16
    # flash layers at head_dim 64 or 128 with attn_pdrop == 0, dense and causal,
    # one K/V head per query head, only.
    doc_sep_token: int = -1

    @property
    def qkv_width(self) -> int:
        """Columns of w_qkv / b_qkv: [Q (n_embd) | K heads | V heads]."""
        if self.n_kv_head in (0, self.n_head):
            return 3 * self.n_embd
        return self.n_embd + 2 * 128 * self.n_kv_head

    @property
    def n_layers_total(self) -> int:
        # fx-shard grain: embedding + blocks + (ln_f + lm_head + loss)
        # (/root/reference/oobleck/module/sharding.py:12-47)
        return self.n_layer + 2

    def layer_kind(self, layer_id: int) -> int:
        from .params import KIND_BLOCK, KIND_EMBED, KIND_FINAL
        if layer_id == 0:
            return KIND_EMBED
        if layer_id == self.n_layers_total - 1:
            return KIND_FINAL
        return KIND_BLOCK

    def layer_attn_window(self, layer_id: int) -> int:
        """The attention window of layer `layer_id` (0 = dense; EMBED and
        FINAL layers always 0)."""
        from .params import KIND_BLOCK
        if self.attn_window <= 0 or self.layer_kind(layer_id) != KIND_BLOCK:
            return 0
        every = self.attn_window_every
        return self.attn_window if (layer_id - 1) % every == every - 1 else 0


GPT2_SMALL = ModelConfig()
# examples/gpt3.yaml model_args (the yaml's actual dims; BASELINE.json calls
# this "GPT-3 2.7B", SURVEY.md §5 notes it is 1600x48 ≈ GPT-2 XL 1.56B)
GPT2_XL = ModelConfig(n_embd=1600, n_head=25, n_layer=48, n_positions=1024)
# GPT-3 sizes (Brown et al. 2020, table 2.1); both have head_dim 128
GPT3_1_3B = ModelConfig(n_embd=2048, n_head=16, n_layer=24, n_positions=2048)
GPT3_6_7B = ModelConfig(n_embd=4096, n_head=32, n_layer=32, n_positions=2048)
# head_dim 96 and 80: flash layers only with OB_FLASH_HD96=1
GPT3_760M = ModelConfig(n_embd=1536, n_head=16, n_layer=24, n_positions=2048)
GPT3_2_7B = ModelConfig(n_embd=2560, n_head=32, n_layer=32, n_positions=2048)
# GPT-BigCode's SantaCoder (Allal et al. 2023): the GPT-2 block with
# multi-query attention, 16 query heads on one K/V head of 128 columns
SANTACODER = ModelConfig(n_embd=2048, n_head=16, n_layer=24, n_positions=2048,
                         vocab_size=49280, n_kv_head=1)
# a grouped-query example: the 6.7B block with 8 K/V heads (groups of 4)
GPT3_6_7B_GQA8 = ModelConfig(n_embd=4096, n_head=32, n_layer=32,
                             n_positions=2048, n_kv_head=8)


@dataclass
class TrainingConfig:
    microbatch_size: int = 8          # gpt2.yaml:5
    global_microbatch_size: int = 128  # gpt2.yaml:6
    seq_len: int = 1024
    lr: float = 5e-5                  # HF TrainingArguments default
    adam_beta1: float = 0.9
    adam_beta2: float = 0.999
    adam_eps: float = 1e-8
    weight_decay: float = 0.0
    warmup_steps: int = 0
    # global gradient-norm clipping (HF TrainingArguments.max_grad_norm; the
    # reference leaves the seam open at pipeline.py:241-244).  0 = off.
    max_grad_norm: float = 0.0
    # dropout masks are a pure function of (dropout_seed, pipeline id, layer,
    # site, optimizer step, microbatch, element): no RNG state to carry
    dropout_seed: int = 0
    # deterministic mode: bit-reproducible bf16 steps.
    # Process-wide; the pipeline applies it before it creates its first layer.
    deterministic: bool = False

    @property
    def num_microbatches(self) -> int:
        assert self.global_microbatch_size % self.microbatch_size == 0
        return self.global_microbatch_size // self.microbatch_size


def synthetic_batch(cfg: ModelConfig, batch: int, seq: int, seed: int):
    """Synthetic token batch (no network: dataset.py:150-208's tokenized
    wikitext is replaced by seeded random ids; labels = input_ids copies the
    reference's dataset.py:201)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, cfg.vocab_size, (batch, seq), generator=g)
    return ids, ids.clone()
