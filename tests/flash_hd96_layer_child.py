# Child process of test_gpu_flash_hd96_layer.py::
# test_layer_route_behind_the_switch: that file's bf16 BLOCK layers (head_dim
# 80 and 96, dense and banded), forward + backward; saves a list of
# uses_flash, attn_window, the output, din and the flat grad per layer to the
# path in argv[1].  The parent sets OB_FLASH_HD96, which the extension reads
# once per process.
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from tests import test_gpu_flash_hd96_layer as t  # noqa: E402

results = []
for H, nh, window in t.LAYERS:
    cfg = t.make_cfg(H, nh, window)
    layer = t.make_layer(cfg)
    flat, x, dout = t.layer_inputs(cfg)
    layer.flat_param.copy_(flat.to(t.DEV))
    layer.refresh_weights()
    out = torch.empty(t.B, t.S, H, device=t.DEV, dtype=torch.bfloat16)
    din = torch.empty_like(out)
    layer.forward_slot(0, x.to(t.DEV), out)
    layer.backward_slot(0, dout.to(t.DEV), din)
    torch.cuda.synchronize()
    results.append({"uses_flash": layer.uses_flash,
                    "attn_window": layer.attn_window, "out": out.cpu(),
                    "din": din.cpu(), "grad": layer.flat_grad.float().cpu()})
torch.save(results, sys.argv[1])
