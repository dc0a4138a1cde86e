# Child process of test_gpu_dw_slices.py::test_whole_layer_ab: one bf16 BLOCK
# layer (H = 128, 2 heads, S = 1024, B = 2), forward + backward, fixed seed;
# saves the output, din, the flat grad and the slice count the choice table
# holds for each of its four weight-grad shapes to the path in argv[1].  The
# backward then runs a second time from zeroed grads in the same process
# ("din2", "grad2"): the same-arm control that shows which grads are
# bit-stable from run to run at all.  The parent sets OB_DW_SLICES, which the
# extension reads once per process.
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from oracle.gpt2_oracle import OracleConfig, init_layer_params  # noqa: E402
from oobleck_amd._ext import layer_lt_shapes, lt_slices  # noqa: E402
from oobleck_amd.config import ModelConfig  # noqa: E402
from oobleck_amd.layer import Layer  # noqa: E402

DEV = "cuda:0"
H, B, S = 128, 2, 1024
dims = dict(n_embd=H, n_head=2, n_layer=2, n_positions=S, vocab_size=304)
mc, oc = ModelConfig(**dims), OracleConfig(**dims)
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
grad = layer.flat_grad.float().cpu()
layer.flat_grad.zero_()
layer.forward_slot(0, x, torch.empty_like(x))  # refill the slot's stash
din2 = torch.empty_like(x)
layer.backward_slot(0, dout, din2)
torch.cuda.synchronize()
slices = {}
for shape in layer_lt_shapes(layer._desc):
    if shape[0]:  # transposed A: a weight grad
        e = lt_slices(shape)
        slices[(shape[2], shape[3])] = e["slices"] if e else None
torch.save({"out": out.cpu(), "din": din.cpu(),
            "grad": grad, "din2": din2.cpu(),
            "grad2": layer.flat_grad.float().cpu(), "slices": slices},
           sys.argv[1])
