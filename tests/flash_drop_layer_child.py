# Child process of test_gpu_flash_dropout.py::test_layer_flash_drop_off: the
# bf16 BLOCK layer of that file's layer tests (attention + residual dropout),
# forward + backward at a fixed tick; saves uses_flash, the output, din and
# the flat grad to the path in argv[1].  The parent sets OB_FLASH_DROP, which
# the extension reads once per process.
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from tests import test_gpu_flash_dropout as t  # noqa: E402

layer = t.make_layer(n_slots=1)
x, dout = t.layer_inputs(0)
out, din = t.run_layer(layer, 0, x, dout, t.LAYER_TICK)
torch.save({"uses_flash": layer.uses_flash, "out": out.cpu(),
            "din": din.cpu(), "grad": layer.flat_grad.float().cpu()},
           sys.argv[1])
