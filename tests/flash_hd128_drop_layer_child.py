# Child process of test_gpu_flash_hd128_dropout.py::
# test_layer_route_behind_the_switch: that file's bf16 BLOCK layer (head_dim
# 128, attention + residual dropout), forward + backward at a fixed tick;
# saves uses_flash, the output, din and the flat grad to the path in argv[1].
# The parent sets OB_FLASH_HD128_DROP, which the extension reads once per
# process.
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from tests import test_gpu_flash_hd128_dropout as t  # noqa: E402

layer = t.make_layer()
x, dout = t.layer_inputs()
H = t.LAYER_DIMS["n_embd"]
out = torch.empty(t.LAYER_B, t.LAYER_S, H, device=t.DEV, dtype=torch.bfloat16)
din = torch.empty_like(out)
layer.forward_slot(0, x.to(t.DEV), out, tick=t.LAYER_TICK)
layer.backward_slot(0, dout.to(t.DEV), din)
torch.cuda.synchronize()
torch.save({"uses_flash": layer.uses_flash, "out": out.cpu(),
            "din": din.cpu(), "grad": layer.flat_grad.float().cpu()},
           sys.argv[1])
