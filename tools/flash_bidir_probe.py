# Solo timing of the bidirectional flash entries (ob_flash_fwd_bidir_bf16 /
# ob_flash_bwd_bidir_d_bf16, head_dim 64) next to the causal ones
# (ob_flash_fwd_nt_bf16 / ob_flash_bwd_nt_d_bf16) at --shape B,nh,S.
#
# The two arms alternate, --repeats times after a warm-up of both; a repeat is
# the mean of --calls back-to-back calls between device events, each call on
# the next of --sets buffer sets (qkv, O, lse, dO, D, dqkv of its own: at the
# step shape four sets are about 400 MB, more than the last-level cache), so no
# call finds its operands where the previous one left them.  It prints every
# repeat, min / median / max per arm and the TF/s of the medians: a
# bidirectional forward is 4*B*nh*S*S*64 FLOP (two GEMMs over the whole
# square), a causal one half of that; a backward 2.5x its forward (five GEMMs).
# The backward rows are dq + dkdv together with the bias sum; each arm's
# backward reads the O and lse of its own forward.
import argparse
import ctypes
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from oobleck_amd._ext import check, get_ext  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="8,12,1024", metavar="B,nh,S")
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--sets", type=int, default=4)
args = ap.parse_args()

B, nh, S = (int(v) for v in args.shape.split(","))
HD = 64
H = nh * HD
DEV = "cuda"
ext = get_ext()
scale = ctypes.c_float(1.0 / HD ** 0.5)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


g = torch.Generator().manual_seed(3)
sets = []
for _ in range(args.sets):
    qkv = (torch.randn(B, S, 3 * H, generator=g) * 0.3).to(DEV).bfloat16()
    dO = (torch.randn(B, S, H, generator=g) * 0.3).to(DEV).bfloat16()
    sets.append(dict(
        qkv=qkv, dO=dO, O=torch.empty_like(dO),
        lse=torch.empty(B * nh * S, device=DEV),
        D=torch.empty(B * nh * S, device=DEV), dqkv=torch.empty_like(qkv)))
dbias = torch.zeros(3 * H, device=DEV)
turn = [0]


def next_set():
    turn[0] = (turn[0] + 1) % len(sets)
    return sets[turn[0]]


def fwd(entry):
    def call(s=None):
        s = s or next_set()
        check(entry(ptr(s["qkv"]), ptr(s["O"]), ptr(s["lse"]), B, S, H, nh,
                    scale, stream()))
    return call


def bwd(entry):
    def call():
        s = next_set()
        check(entry(ptr(s["qkv"]), ptr(s["O"]), ptr(s["dO"]), ptr(s["lse"]),
                    ptr(s["D"]), ptr(s["dqkv"]), ptr(dbias), B, S, H, nh,
                    scale, stream()))
    return call


def timed(fn):
    st, en = torch.cuda.Event(True), torch.cuda.Event(True)
    st.record()
    for _ in range(args.calls):
        fn()
    en.record()
    torch.cuda.synchronize()
    return st.elapsed_time(en) / args.calls * 1e3


fwd_c, fwd_b = fwd(ext.ob_flash_fwd_nt_bf16), fwd(ext.ob_flash_fwd_bidir_bf16)
bwd_c = bwd(ext.ob_flash_bwd_nt_d_bf16)
bwd_b = bwd(ext.ob_flash_bwd_bidir_d_bf16)
mflop = 4 * B * nh * S * S * HD * 1e-6  # bidirectional forward

print(f"head_dim {HD}, (B, nh, S) = ({B}, {nh}, {S}), {args.sets} buffer "
      f"sets, {args.calls} calls per repeat")
for name, causal, bidir, pre, gemms in (
        ("fwd", fwd_c, fwd_b, (None, None), 1.0),
        ("bwd (dq + dkdv, D in-kernel, + bias)", bwd_c, bwd_b, (fwd_c, fwd_b),
         2.5)):
    us = ([], [])
    for rep in range(-1, args.repeats):  # rep -1 warms both arms up
        for arm, fn in enumerate((causal, bidir)):
            if pre[arm]:  # every set gets this arm's O and lse
                for s in sets:
                    pre[arm](s)
            t = timed(fn)
            if rep >= 0:
                us[arm].append(t)
    print(name)
    for arm, label, work in ((0, "causal", 0.5), (1, "bidir ", 1.0)):
        v = us[arm]
        med = statistics.median(v)
        print(f"  {label} us: " + " ".join(f"{x:7.1f}" for x in v))
        print(f"  {label} min {min(v):.1f} median {med:.1f} max {max(v):.1f}"
              f"; {gemms * work * mflop / med:.1f} TF/s")
    print(f"  bidir / causal time = "
          f"{statistics.median(us[1]) / statistics.median(us[0]):.2f}")
