# @gpu test of the head_dim 80 / 96 layer route behind OB_FLASH_HD96, in the
# pattern of test_gpu_flash_hd128_dropout.py::test_layer_route_behind_the_
# switch: the switch is read once per process, so a fresh child with it set
# (tests/flash_hd96_layer_child.py) runs bf16 BLOCK layers, dense and with
# attn_window = 64, forward and backward; they must be flash layers and meet
# the bounds of tests/test_gpu_flash_window_layer.py (out 1.5e-2, din 3e-2,
# grad 3e-2) against that file's fp32 restatement of the block.  This process
# (unset) keeps the dense layer off the route and refuses the banded one.
import os
import pathlib
import subprocess
import sys

import pytest
import torch

from tests.test_gpu_flash_window_layer import (DEV, B, S, W, _block_ref,
                                               rel_l2)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
LAYERS = [(H, nh, win) for H, nh in ((160, 2), (192, 2)) for win in (0, W)]


def make_cfg(H, nh, window):
    from oobleck_amd.config import ModelConfig
    return ModelConfig(n_embd=H, n_head=nh, n_layer=2, n_positions=S,
                       vocab_size=304, attn_window=window, attn_window_every=1)


def make_layer(cfg):
    from oobleck_amd.layer import Layer
    return Layer(1, cfg, B, S, 1, torch.device(DEV), dtype="bf16")


def layer_inputs(cfg):
    """flat parameters (fp32), x and dout (bf16), all on the CPU"""
    from oobleck_amd.params import init_layer_params
    g = torch.Generator().manual_seed(8)
    x = (torch.randn(B, S, cfg.n_embd, generator=g) * 0.5).bfloat16()
    dout = (torch.randn(B, S, cfg.n_embd, generator=g) * 0.1).bfloat16()
    return init_layer_params(cfg, 1, 77, "gpt2"), x, dout


@requires_gpu
def test_layer_route_behind_the_switch(tmp_path):
    assert "OB_FLASH_HD96" not in os.environ
    for H, nh, _ in LAYERS[::2]:
        assert make_layer(make_cfg(H, nh, 0)).uses_flash is False
        with pytest.raises(RuntimeError, match="attn_window"):
            make_layer(make_cfg(H, nh, W))
    out_path = tmp_path / "hd96.pt"
    child = pathlib.Path(__file__).with_name("flash_hd96_layer_child.py")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + \
          [str(child), str(out_path)]
    subprocess.run(cmd, check=True, timeout=300,
                   env=dict(os.environ, OB_FLASH_HD96="1"))
    for (H, nh, win), got in zip(LAYERS, torch.load(out_path)):
        assert got["uses_flash"] is True and got["attn_window"] == win
        cfg = make_cfg(H, nh, win)
        flat, x, dout = layer_inputs(cfg)
        fr = flat.clone().requires_grad_(True)
        xr = x.float().requires_grad_(True)
        ref = _block_ref(cfg, fr, xr, win or S)
        ref.backward(dout.float())
        e = [rel_l2(got[k].float(), r) for k, r in zip(
            ("out", "din", "grad"), (ref.detach(), xr.grad, fr.grad))]
        print(f"hd96 layer H={H} nh={nh} window={win}: out, din, grad", e)
        assert e[0] < 1.5e-2 and e[1] < 3e-2 and e[2] < 3e-2, (H, win, e)
