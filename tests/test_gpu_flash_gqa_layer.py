# @gpu test of a multi-query bf16 BLOCK layer (n_kv_head = 1) against an fp32
# torch block built from params.layer_param_spec (the W-wide w_qkv and b_qkv),
# with the per-layer bf16 bounds (1.5e-2 forward, 3e-2 grads).
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
DEV = "cuda:0"
B, S, H, NH, NKV = 2, 256, 256, 2, 1
HD = H // NH


def rel_l2(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _cfg(**kw):
    from oobleck_amd.config import ModelConfig
    return ModelConfig(n_embd=H, n_head=NH, n_layer=2, n_positions=S,
                       vocab_size=304, n_kv_head=NKV, **kw)


def _block_ref(cfg, flat, x):
    """GPT-2 block (pre-LN, gelu_new), fp32, causal, NKV shared K/V heads."""
    from oobleck_amd.params import KIND_BLOCK, layer_param_spec
    p, o = {}, 0
    for name, shape in layer_param_spec(cfg, KIND_BLOCK):
        n = math.prod(shape)
        p[name] = flat[o:o + n].view(shape)
        o += n
    assert o == flat.numel() and p["w_qkv"].shape == (H, H + 2 * HD * NKV)
    ln = torch.nn.functional.layer_norm
    qkv = ln(x, (H,), p["ln1_w"], p["ln1_b"], 1e-5) @ p["w_qkv"] + p["b_qkv"]
    q, k, v = qkv.split((H, HD * NKV, HD * NKV), dim=-1)
    q = q.view(B, S, NH, HD).permute(0, 2, 1, 3)
    k, v = (t.view(B, S, NKV, HD).permute(0, 2, 1, 3)
            .repeat_interleave(NH // NKV, dim=1) for t in (k, v))
    s = q @ k.transpose(-1, -2) / math.sqrt(HD)
    s = s.masked_fill(~torch.tril(torch.ones(S, S, dtype=torch.bool)),
                      float("-inf"))
    a = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B, S, H)
    h = x + a @ p["w_attnproj"] + p["b_attnproj"]
    u = ln(h, (H,), p["ln2_w"], p["ln2_b"], 1e-5) @ p["w_fc"] + p["b_fc"]
    return h + torch.nn.functional.gelu(u, approximate="tanh") \
        @ p["w_mlpproj"] + p["b_mlpproj"]


@requires_gpu
def test_gqa_block_layer():
    from oobleck_amd.layer import Layer
    from oobleck_amd.params import init_layer_params
    cfg = _cfg()
    layer = Layer(1, cfg, B, S, 1, torch.device(DEV), dtype="bf16")
    assert layer.uses_flash and layer.n_kv_head == 1
    flat = init_layer_params(cfg, 1, 77, "gpt2")
    layer.flat_param.copy_(flat.to(DEV))
    layer.refresh_weights()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, S, H, generator=g) * 0.5
    dout = torch.randn(B, S, H, generator=g) * 0.1
    xg = x.to(DEV).bfloat16()
    out, din = torch.empty_like(xg), torch.empty_like(xg)
    layer.forward_slot(0, xg, out)
    layer.backward_slot(0, dout.to(DEV).bfloat16(), din)
    torch.cuda.synchronize()

    fr = flat.clone().requires_grad_(True)
    xr = xg.float().cpu().requires_grad_(True)
    ref = _block_ref(cfg, fr, xr)
    ref.backward(dout.bfloat16().float())
    e = (rel_l2(out.float().cpu(), ref.detach()),
         rel_l2(din.float().cpu(), xr.grad),
         rel_l2(layer.flat_grad.cpu(), fr.grad))
    print(f"gqa block: out {e[0]:.3e} din {e[1]:.3e} grad {e[2]:.3e}")
    assert e[0] < 1.5e-2 and e[1] < 3e-2 and e[2] < 3e-2, e


@requires_gpu
@pytest.mark.parametrize("kw", [dict(dtype="f32"),
                                dict(dtype="bf16", attn_pdrop=0.1)],
                         ids=["f32", "attn_pdrop"])
def test_gqa_layer_refused(kw):
    from oobleck_amd.layer import Layer
    with pytest.raises(RuntimeError, match="n_kv_head"):
        Layer(1, _cfg(), B, S, 1, torch.device(DEV), **kw)
