# @gpu test of a bidirectional bf16 BLOCK layer (attn_causal = False) against
# the fp32 torch block of tests/test_gpu_flash_window_layer.py without the
# mask, with the per-layer bf16 bounds (1.5e-2 forward, 3e-2 grads).
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
DEV = "cuda:0"
B, S, H, NH = 2, 256, 128, 2


def rel_l2(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _cfg(**kw):
    from oobleck_amd.config import ModelConfig
    return ModelConfig(n_embd=H, n_head=NH, n_layer=2, n_positions=S,
                       vocab_size=304, **kw)


def _block_ref(cfg, flat, x):
    """GPT-2 block (pre-LN, gelu_new), fp32, every query sees every key."""
    from oobleck_amd.params import KIND_BLOCK, layer_param_spec
    p, o = {}, 0
    for name, shape in layer_param_spec(cfg, KIND_BLOCK):
        n = math.prod(shape)
        p[name] = flat[o:o + n].view(shape)
        o += n
    ln = torch.nn.functional.layer_norm
    qkv = ln(x, (H,), p["ln1_w"], p["ln1_b"], 1e-5) @ p["w_qkv"] + p["b_qkv"]
    q, k, v = (t.view(B, S, NH, H // NH).permute(0, 2, 1, 3)
               for t in qkv.split(H, dim=-1))
    s = q @ k.transpose(-1, -2) / math.sqrt(H // NH)
    a = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B, S, H)
    h = x + a @ p["w_attnproj"] + p["b_attnproj"]
    u = ln(h, (H,), p["ln2_w"], p["ln2_b"], 1e-5) @ p["w_fc"] + p["b_fc"]
    return h + torch.nn.functional.gelu(u, approximate="tanh") \
        @ p["w_mlpproj"] + p["b_mlpproj"]


@requires_gpu
def test_bidir_block_layer():
    from oobleck_amd.layer import Layer
    from oobleck_amd.params import init_layer_params
    cfg = _cfg(attn_causal=False)
    layer = Layer(1, cfg, B, S, 1, torch.device(DEV), dtype="bf16")
    assert layer.uses_flash and not layer.attn_causal
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
    print(f"bidir block: out {e[0]:.3e} din {e[1]:.3e} grad {e[2]:.3e}")
    assert e[0] < 1.5e-2 and e[1] < 3e-2 and e[2] < 3e-2, e


@requires_gpu
def test_bidir_fp32_layer_refused():
    from oobleck_amd.layer import Layer
    with pytest.raises(RuntimeError, match="attn_bidir"):
        Layer(1, _cfg(), B, S, 1, torch.device(DEV), dtype="f32",
              attn_causal=False)
