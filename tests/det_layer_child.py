# Child process of test_gpu_det_layers.py: for each configuration named in
# argv[3:], builds EMBED -> BLOCK -> BLOCK -> FINAL (bf16) and runs 2
# optimizer steps of 3 microbatches over 2 slots with AdamW, fixed seeds.
# Saves to the .npz in argv[1] the loss of every microbatch, din of the first
# block, every flat grad before each step, and params and moments after it.
# argv[2] is "det" (deterministic mode, set through the Python switch before
# the first layer) or "default".  A det child also records what
# ob_set_deterministic returns once layers exist and whether an fp32 layer
# can be created.  The extension reads its switches once per process, hence
# the child.
import pathlib
import sys

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

import oobleck_amd  # noqa: E402
from oobleck_amd._ext import check, get_ext  # noqa: E402
from oobleck_amd.config import ModelConfig  # noqa: E402
from oobleck_amd.layer import Layer  # noqa: E402
from tests.gpu_helpers import ptr, stream  # noqa: E402

# name -> (H, n_head, S, pdrop)
CONFIGS = {
    "hd64_cpt": (128, 2, 128, 0.0),    # head_dim 64 flash, CPT LayerNorm
    "hd64_wave": (512, 8, 256, 0.0),   # wave LayerNorm
    "hd128": (256, 2, 128, 0.0),       # head_dim 128 flash
    "matp": (128, 2, 192, 0.0),        # S % 128 != 0: materialized P
    "drop": (512, 8, 128, 0.1),        # all three dropouts
}
B, V, STEPS, MBS, SLOTS = 2, 304, 2, 3, 2
DEV = torch.device("cuda:0")


def bits(t):
    t = t.detach().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy()
    return t.float().cpu().numpy()


def run_config(name, out):
    H, nh, S, pd = CONFIGS[name]
    mc = ModelConfig(n_embd=H, n_head=nh, n_layer=2, n_positions=256,
                     vocab_size=V, embd_pdrop=pd, resid_pdrop=pd,
                     attn_pdrop=pd)
    L = mc.n_layers_total
    layers = [Layer(lid, mc, B, S, SLOTS, DEV, dtype="bf16", seed=7 + lid,
                    dropout_seed=11) for lid in range(L)]
    out[f"{name}__flash"] = np.array([int(layers[1].uses_flash)])
    out[f"{name}__det"] = np.array([int(l.deterministic) for l in layers])
    moments = [(torch.zeros_like(l.flat_param), torch.zeros_like(l.flat_param))
               for l in layers]
    ext = get_ext()
    g = torch.Generator().manual_seed(5)
    for step in range(STEPS):
        for mb in range(MBS):
            slot = mb % SLOTS
            tick = step * MBS + mb
            ids = torch.randint(0, V, (B, S), generator=g).to(DEV)
            x = ids
            for lid, layer in enumerate(layers):
                if lid == L - 1:
                    y = torch.zeros(1, device=DEV)
                    layer.forward_slot(slot, x, y, ids, tick=tick)
                else:
                    y = torch.empty(B, S, H, device=DEV, dtype=torch.bfloat16)
                    layer.forward_slot(slot, x, y, tick=tick)
                x = y
            out[f"{name}__loss__{step}_{mb}"] = bits(x)
            dout = None
            for lid in range(L - 1, -1, -1):
                din = None if lid == 0 else torch.empty(
                    B, S, H, device=DEV, dtype=torch.bfloat16)
                layers[lid].backward_slot(slot, dout, din)
                if lid == 1:
                    torch.cuda.synchronize()
                    out[f"{name}__din__{step}_{mb}"] = bits(din)
                dout = din
        torch.cuda.synchronize()
        for lid, layer in enumerate(layers):
            out[f"{name}__grad__{step}_{lid}"] = bits(layer.flat_grad)
            m, v = moments[lid]
            check(ext.ob_adamw_step(ptr(layer.flat_param), ptr(layer.flat_grad),
                                    ptr(m), ptr(v), layer.flat_param.numel(),
                                    step + 1, 1e-3, 0.9, 0.999, 1e-8, 0.01,
                                    stream()), "adamw")
            layer.refresh_weights()
            layer.zero_grads()
        torch.cuda.synchronize()
        for lid, layer in enumerate(layers):
            out[f"{name}__param__{step}_{lid}"] = bits(layer.flat_param)
            out[f"{name}__m__{step}_{lid}"] = bits(moments[lid][0])
            out[f"{name}__v__{step}_{lid}"] = bits(moments[lid][1])
    return mc, layers


def main():
    path, mode, names = sys.argv[1], sys.argv[2], sys.argv[3:]
    if mode == "det":
        oobleck_amd.set_deterministic(True)
    out = {}
    mc = layers = None
    for name in names:
        mc, layers = run_config(name, out)
    if mode == "det":
        ext = get_ext()
        # the switch is frozen once a layer exists
        out["set_after_create_rc"] = np.array(
            [ext.ob_set_deterministic(0), ext.ob_deterministic()])
        try:
            Layer(1, mc, B, 128, 1, DEV, dtype="f32")
            msg = ""
        except RuntimeError as e:
            msg = str(e)
        out["fp32_create_error"] = np.array([msg])
    np.savez(path, **out)


if __name__ == "__main__":
    main()
