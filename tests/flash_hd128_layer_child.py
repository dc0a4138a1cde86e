# Child process of test_gpu_wide_layers.py::test_hd128_layer_ab: one bf16
# BLOCK layer with head_dim 128 (H = 256, 2 heads), forward + backward,
# fixed seed; saves the output, din, the flat grad and uses_flash to the
# path in argv[1].  The parent sets OB_FLASH_HD128 and OB_LT_TUNE, which the
# extension reads once per process.
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from oracle.gpt2_oracle import OracleConfig, init_layer_params  # noqa: E402
from oobleck_amd.config import ModelConfig  # noqa: E402
from oobleck_amd.layer import Layer  # noqa: E402

DEV = "cuda:0"
H = 256
dims = dict(n_embd=H, n_head=2, n_layer=2, n_positions=128, vocab_size=304)
mc, oc = ModelConfig(**dims), OracleConfig(**dims)
B, S = 2, 128
flat = init_layer_params(oc, 1, 77)
layer = Layer(1, mc, B, S, 2, torch.device(DEV), dtype="bf16")
layer.flat_param.copy_(flat.to(DEV))
layer.refresh_weights()
g = torch.Generator().manual_seed(8)
x = (torch.randn(B, S, H, generator=g) * 0.5).to(DEV).bfloat16()
dout = (torch.randn(B, S, H, generator=g) * 0.1).to(DEV).bfloat16()
out = torch.empty_like(x)
layer.forward_slot(0, x, out)
din = torch.empty_like(x)
layer.backward_slot(0, dout, din)
torch.cuda.synchronize()
torch.save({"out": out.cpu(), "din": din.cpu(),
            "grad": layer.flat_grad.float().cpu(),
            "uses_flash": layer.uses_flash}, sys.argv[1])
