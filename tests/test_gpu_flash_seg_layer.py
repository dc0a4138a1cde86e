# @gpu test of a document-masked bf16 BLOCK layer (attn_segments) at head_dim
# 64 and 128: forward and backward through Layer with doc_start given, against
# the fp32 torch restatement of the GPT-2 block of
# tests/test_gpu_flash_window_layer.py with the document mask, with that file's
# bounds (1.5e-2 forward, 3e-2 grads); then the same slot with doc_start=None
# against the plain causal block.
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
DEV = "cuda:0"
B, S = 2, 256
STARTS = [[64, 131], [200]]


def rel_l2(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _block_ref(cfg, flat, x, doc):
    """GPT-2 block (pre-LN, gelu_new), fp32; query i sees the keys j <= i with
    doc[b, j] == doc[b, i]."""
    from oobleck_amd.params import KIND_BLOCK, layer_param_spec
    H, nh = cfg.n_embd, cfg.n_head
    p, o = {}, 0
    for name, shape in layer_param_spec(cfg, KIND_BLOCK):
        n = math.prod(shape)
        p[name] = flat[o:o + n].view(shape)
        o += n
    ln = torch.nn.functional.layer_norm
    qkv = ln(x, (H,), p["ln1_w"], p["ln1_b"], 1e-5) @ p["w_qkv"] + p["b_qkv"]
    q, k, v = (t.view(B, S, nh, H // nh).permute(0, 2, 1, 3)
               for t in qkv.split(H, dim=-1))
    s = q @ k.transpose(-1, -2) / math.sqrt(H // nh)
    i = torch.arange(S)
    keep = (doc[:, :, None] == doc[:, None, :]) & (i[:, None] >= i[None, :])
    s = s.masked_fill(~keep[:, None], float("-inf"))
    a = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B, S, H)
    h = x + a @ p["w_attnproj"] + p["b_attnproj"]
    u = ln(h, (H,), p["ln2_w"], p["ln2_b"], 1e-5) @ p["w_fc"] + p["b_fc"]
    return h + torch.nn.functional.gelu(u, approximate="tanh") \
        @ p["w_mlpproj"] + p["b_mlpproj"]


@requires_gpu
@pytest.mark.parametrize("H,nh", [(128, 2), (256, 2)])
def test_segmented_block_layer(H, nh):
    from oobleck_amd.config import ModelConfig
    from oobleck_amd.layer import Layer
    from oobleck_amd.params import init_layer_params
    cfg = ModelConfig(n_embd=H, n_head=nh, n_layer=2, n_positions=S,
                      vocab_size=304, doc_sep_token=7)
    layer = Layer(1, cfg, B, S, 1, torch.device(DEV), dtype="bf16")
    assert layer.uses_flash and layer.attn_segments
    flat = init_layer_params(cfg, 1, 77, "gpt2")
    layer.flat_param.copy_(flat.to(DEV))
    layer.refresh_weights()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, S, H, generator=g) * 0.5
    dout = torch.randn(B, S, H, generator=g) * 0.1
    xg = x.to(DEV).bfloat16()
    ds = torch.zeros(B, S, dtype=torch.int32)
    for b, st in enumerate(STARTS):
        ds[b, st] = 1
    # documents given, then the same slot reset to one document per row
    for doc_start, doc in ((ds.to(DEV), ds.cumsum(1)),
                           (None, torch.zeros(B, S))):
        out, din = torch.empty_like(xg), torch.empty_like(xg)
        layer.zero_grads()
        layer.forward_slot(0, xg, out, doc_start=doc_start)
        layer.backward_slot(0, dout.to(DEV).bfloat16(), din)
        torch.cuda.synchronize()
        fr = flat.clone().requires_grad_(True)
        xr = xg.float().cpu().requires_grad_(True)
        ref = _block_ref(cfg, fr, xr, doc)
        ref.backward(dout.bfloat16().float())
        e = (rel_l2(out.float().cpu(), ref.detach()),
             rel_l2(din.float().cpu(), xr.grad),
             rel_l2(layer.flat_grad.cpu(), fr.grad))
        print(f"segmented block H={H} nh={nh} "
              f"{'docs' if doc_start is not None else 'reset'}: out "
              f"{e[0]:.3e} din {e[1]:.3e} grad {e[2]:.3e}")
        assert e[0] < 1.5e-2 and e[1] < 3e-2 and e[2] < 3e-2, e


@requires_gpu
def test_segmented_layer_refusals():
    from oobleck_amd.config import ModelConfig
    from oobleck_amd.layer import Layer
    cfg = ModelConfig(n_embd=128, n_head=2, n_layer=2, n_positions=S,
                      vocab_size=304)
    with pytest.raises(RuntimeError, match="attn_segments"):
        Layer(1, cfg, B, S, 1, torch.device(DEV), dtype="f32",
              attn_segments=True)
    plain = Layer(1, cfg, B, S, 1, torch.device(DEV), dtype="bf16")
    assert not plain.attn_segments
    x = torch.zeros(B, S, 128, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="attn_segments"):
        plain.forward_slot(0, x, torch.empty_like(x),
                           doc_start=torch.zeros(B, S, dtype=torch.int32,
                                                 device=DEV))
