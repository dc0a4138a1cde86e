# Host restatement of the dropout mask (numpy Philox4x32-10, the definition
# frozen in oobleck_amd/csrc/ob_philox.h / DESIGN.md) and a torch fp32
# autograd restatement of embed / block / final that takes explicit keep
# masks.  Shared by tests/test_dropout_cpu.py and tests/test_gpu_dropout.py.
from __future__ import annotations

import math

import numpy as np
import torch

from oracle.gpt2_oracle import (KIND_BLOCK, KIND_EMBED, KIND_FINAL,
                                OracleConfig, layer_param_spec)

SITE_EMBD, SITE_ATTN, SITE_RESID_ATTN, SITE_RESID_MLP = 0, 1, 2, 3

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr: 4 uint32 arrays (or scalars), key: 2 ints -> 4 uint32 arrays."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & _LO for v in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _LO,
             (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _LO]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def threshold(p: float) -> int:
    """floor(p * 2^32) with p taken as the fp32 the C-ABI receives."""
    return int(math.floor(float(np.float32(p)) * 4294967296.0))


def scale(p: float) -> float:
    """1/(1-p) in fp32."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_mask(seed: int, layer_id: int, site: int, tick: int, p: float,
              n: int) -> np.ndarray:
    """uint8[n]: 1 where element e is kept."""
    assert n <= 1 << 34
    nq = (n + 3) // 4
    q = np.arange(nq, dtype=np.uint64)
    words = philox4x32_10(
        (q, tick & 0xFFFFFFFF, (tick >> 32) & 0xFFFFFFFF,
         ((layer_id << 8) | site) & 0xFFFFFFFF),
        (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    w = np.stack([np.broadcast_to(v, (nq,)) for v in words], axis=1)
    return (w.reshape(-1)[:n] >= np.uint32(threshold(p))).astype(np.uint8)


def factor(keep, p: float, shape) -> torch.Tensor:
    """keep bytes -> the fp32 multiplier keep * 1/(1-p), shaped."""
    k = torch.as_tensor(np.asarray(keep), dtype=torch.float32)
    return (k * scale(p)).reshape(shape)


def layer_masks(seed: int, layer_id: int, kind: int, tick: int, pdrop: dict,
                B: int, S: int, H: int, nh: int) -> dict:
    """The multipliers one layer's forward at `tick` draws, from the numpy
    reference.  pdrop: {"embd","resid","attn"} -> p."""
    m = {}
    if kind == KIND_EMBED and pdrop.get("embd", 0) > 0:
        p = pdrop["embd"]
        m["embd"] = factor(keep_mask(seed, layer_id, SITE_EMBD, tick, p,
                                     B * S * H), p, (B, S, H))
    if kind == KIND_BLOCK:
        if pdrop.get("attn", 0) > 0:
            p = pdrop["attn"]
            m["attn"] = factor(keep_mask(seed, layer_id, SITE_ATTN, tick, p,
                                         B * nh * S * S), p, (B, nh, S, S))
        if pdrop.get("resid", 0) > 0:
            p = pdrop["resid"]
            for name, site in (("resid_attn", SITE_RESID_ATTN),
                               ("resid_mlp", SITE_RESID_MLP)):
                m[name] = factor(keep_mask(seed, layer_id, site, tick, p,
                                           B * S * H), p, (B, S, H))
    return m


# ---------------------------------------------------------------------------
# torch fp32 restatement with explicit masks (missing mask = no dropout)
# ---------------------------------------------------------------------------

def _unpack(cfg: OracleConfig, kind: int, flat: torch.Tensor) -> dict:
    out, off = {}, 0
    for name, shape in layer_param_spec(cfg, kind):
        n = math.prod(shape)
        out[name] = flat[off:off + n].view(shape)
        off += n
    assert off == flat.numel()
    return out


def _ln(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = x.var(-1, keepdim=True, unbiased=False)
    return (x - mu) * torch.rsqrt(var + eps) * w + b


def _gelu(x):
    return 0.5 * x * (1.0 + torch.tanh(
        math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def _drop(x, m):
    return x if m is None else x * m


def layer_forward(cfg: OracleConfig, kind: int, flat, x, masks: dict,
                  labels=None):
    p = _unpack(cfg, kind, flat)
    eps = cfg.layer_norm_eps
    if kind == KIND_EMBED:
        return _drop(p["wte"][x] + p["wpe"][:x.shape[1]], masks.get("embd"))
    if kind == KIND_BLOCK:
        B, S, H = x.shape
        nh = cfg.n_head
        a = _ln(x, p["ln1_w"], p["ln1_b"], eps)
        qkv = a @ p["w_qkv"] + p["b_qkv"]
        q, k, v = (t.view(B, S, nh, H // nh).permute(0, 2, 1, 3)
                   for t in qkv.split(H, dim=-1))
        w = q @ k.transpose(-1, -2) / math.sqrt(H // nh)
        causal = torch.tril(torch.ones(S, S, dtype=torch.bool))
        w = torch.softmax(w.masked_fill(~causal, torch.finfo(w.dtype).min), -1)
        o = (_drop(w, masks.get("attn")) @ v).permute(0, 2, 1, 3)
        o = o.reshape(B, S, H) @ p["w_attnproj"] + p["b_attnproj"]
        h = x + _drop(o, masks.get("resid_attn"))
        m = _ln(h, p["ln2_w"], p["ln2_b"], eps)
        m = _gelu(m @ p["w_fc"] + p["b_fc"]) @ p["w_mlpproj"] + p["b_mlpproj"]
        return h + _drop(m, masks.get("resid_mlp"))
    if kind == KIND_FINAL:
        logits = _ln(x, p["lnf_w"], p["lnf_b"], eps) @ p["w_lm"].t()
        return torch.nn.functional.cross_entropy(
            logits[:, :-1].reshape(-1, cfg.vocab_size),
            labels[:, 1:].reshape(-1))
    raise ValueError(kind)


def stage_forward_backward(cfg: OracleConfig, flats, layer_ids, x_in,
                           masks: list[dict], labels=None, dout=None):
    """oracle.gpt2_oracle.stage_forward_backward with masks[i] applied in
    layer layer_ids[i].  Returns (out, dx_in, grad_flats)."""
    flats = [f.detach().clone().requires_grad_(True) for f in flats]
    x0 = x_in.detach().clone()
    if x0.is_floating_point():
        x0.requires_grad_(True)
    x = x0
    for i, lid in enumerate(layer_ids):
        kind = cfg.layer_kind(lid)
        x = layer_forward(cfg, kind, flats[i], x, masks[i],
                          labels if kind == KIND_FINAL else None)
    if dout is None:
        x.backward()
    else:
        torch.autograd.backward(x, dout)
    dx = x0.grad if x0.is_floating_point() else None
    return x.detach(), dx, [f.grad for f in flats]
