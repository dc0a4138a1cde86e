# Child of test_gpu_flash_band_dropout.py::test_layer_route_behind_the_switch,
# started with OB_FLASH_BAND_DROP and OB_FLASH_HD96 set (read once per process):
# that file's banded dropout layer at each head size, forward + backward at a
# fixed tick; saves {head_dim: route, output, din, flat grad} to argv[1].
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from tests import test_gpu_flash_band_dropout as t  # noqa: E402

res = {}
for hd in t.HDS:
    layer = t.make_layer(hd)
    x, dout = t.layer_inputs(hd)
    out = torch.empty(t.LAYER_B, t.LAYER_S, 2 * hd, device=t.DEV,
                      dtype=torch.bfloat16)
    din = torch.empty_like(out)
    layer.forward_slot(0, x.to(t.DEV), out, tick=t.LAYER_TICK)
    layer.backward_slot(0, dout.to(t.DEV), din)
    torch.cuda.synchronize()
    res[hd] = {"uses_flash": layer.uses_flash,
               "attn_window": layer.attn_window, "out": out.cpu(),
               "din": din.cpu(), "grad": layer.flat_grad.float().cpu()}
torch.save(res, sys.argv[1])
