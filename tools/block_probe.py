# Times forward + backward of ONE bf16 BLOCK layer for given dimensions and
# prints one JSON line: the route the layer took (uses_flash), milliseconds
# per forward+backward (median, min, max over the windows), and what the
# layer holds on the device.  Device events around each window; the inputs
# rotate over --rotate buffers so a window does not re-read what the last
# call left in the caches.  The environment switches (OB_FLASH_HD128, ...)
# are read once per process, so an A/B is two processes.
#
#   python tools/block_probe.py --n-embd 4096 --n-head 32 --batch 2 --seq 1024
import argparse
import json
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from oobleck_amd.config import ModelConfig  # noqa: E402
from oobleck_amd.layer import Layer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n-embd", type=int, default=4096)
ap.add_argument("--n-head", type=int, default=32)
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--seq", type=int, default=1024)
ap.add_argument("--slots", type=int, default=1)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=10, help="calls per window")
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--rotate", type=int, default=4, help="input buffer sets")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("block_probe: needs a GPU")
DEV = torch.device("cuda:0")
H, nh, B, S = args.n_embd, args.n_head, args.batch, args.seq
cfg = ModelConfig(n_embd=H, n_head=nh, n_layer=1, n_positions=max(S, 128),
                  vocab_size=304)
torch.cuda.synchronize()
free0 = torch.cuda.mem_get_info()[0]
layer = Layer(1, cfg, B, S, args.slots, DEV, dtype="bf16")
torch.cuda.synchronize()
held = free0 - torch.cuda.mem_get_info()[0]

# per-slot stash of a BLOCK layer in floats (layer_create, ob_layer.hip):
# everything but the attention slot, then P [B, nh, S, S] or the LSE
BS = B * S
common = 16 * BS * H + 4 * BS
attn = B * nh * S * (1 if layer.uses_flash else S)
stash_bytes = 4 * args.slots * (common + attn)

g = torch.Generator().manual_seed(1)
xs = [(torch.randn(B, S, H, generator=g) * 0.5).to(DEV).bfloat16()
      for _ in range(args.rotate)]
douts = [(torch.randn(B, S, H, generator=g) * 0.1).to(DEV).bfloat16()
         for _ in range(args.rotate)]
out = torch.empty_like(xs[0])
din = torch.empty_like(xs[0])


def call(i):
    k = i % args.rotate
    layer.forward_slot(0, xs[k], out)
    layer.backward_slot(0, douts[k], din)


for i in range(args.warmup):
    call(i)
torch.cuda.synchronize()
ms = []
st, en = torch.cuda.Event(True), torch.cuda.Event(True)
for _ in range(args.windows):
    st.record()
    for i in range(args.reps):
        call(i)
    en.record()
    torch.cuda.synchronize()
    ms.append(st.elapsed_time(en) / args.reps)
print(json.dumps({
    "n_embd": H, "n_head": nh, "batch": B, "seq": S, "slots": args.slots,
    "uses_flash": layer.uses_flash,
    "ms_fwd_bwd_median": round(statistics.median(ms), 4),
    "ms_fwd_bwd_min": round(min(ms), 4), "ms_fwd_bwd_max": round(max(ms), 4),
    "stash_bytes": stash_bytes, "attn_stash_bytes": 4 * args.slots * attn,
    "device_bytes_held_after_create": held}))
