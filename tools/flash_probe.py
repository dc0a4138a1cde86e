# Within-box A/B of the two flash-attention paths at the step shape
# (B=8, nh=12, S=1024, head_dim 64): transposed copies + the
# transposed-operand kernels (what ob_layer.hip runs per block-microbatch
# under OB_FLASH_TR=0) vs the production `_nt` entry points.  Prints whether
# the outputs are bit-identical, then one timing row per path.
# Per-kernel times: run this file under a kernel trace (tools/kstats.py).
#
# --attn-pdrop P (0 < P < 1) adds the attention-dropout entries
# (ob_flash_fwd_nt_drop_bf16 / ob_flash_bwd_nt_d_drop_bf16) next to the plain
# ones.
#
# --head-dim 128 times the head_dim 128 kernels behind the same `_nt` entries
# instead (there are no transposed-operand twins at 128), at --shape B,nh,S,
# and prints TF next to the microseconds: causal FLOPs, 2*B*nh*S*S*hd for
# the forward (2 GEMMs over half the square) and 5*B*nh*S*S*hd for the
# backward (5 GEMMs).  The default, --head-dim 64, prints what it always did.
import argparse
import ctypes
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from oobleck_amd._ext import check, get_ext  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--attn-pdrop", type=float, default=0.0, metavar="P",
                help="also time the dropout variants of the three kernels")
ap.add_argument("--head-dim", type=int, default=64, choices=(64, 128))
ap.add_argument("--shape", default="8,12,1024", metavar="B,nh,S")
args = ap.parse_args()

B, nh, S = (int(v) for v in args.shape.split(","))
hd = args.head_dim
H = nh * hd
DEV = "cuda"


def ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def timeit(fn, reps=30):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    st, en = torch.cuda.Event(True), torch.cuda.Event(True)
    best = float("inf")
    for _ in range(3):
        st.record()
        for _ in range(reps):
            fn()
        en.record()
        torch.cuda.synchronize()
        best = min(best, st.elapsed_time(en) / reps)
    return best


ext = get_ext()
g = torch.Generator().manual_seed(3)
qkv = (torch.randn(B, S, 3 * H, generator=g) * 0.3).to(DEV).bfloat16()
dO = (torch.randn(B, S, H, generator=g) * 0.3).to(DEV).bfloat16()
O = torch.empty(B, S, H, device=DEV, dtype=torch.bfloat16)
lse = torch.empty(B * nh * S, device=DEV)
D = torch.empty(B * nh * S, device=DEV)
dqkv = torch.zeros_like(qkv)
VT = torch.empty(B * nh, hd, S, device=DEV, dtype=torch.bfloat16)
QT = torch.empty_like(VT)
KT = torch.empty_like(VT)
dOT = torch.empty_like(VT)
scale = ctypes.c_float(1.0 / hd ** 0.5)

V_ptr = ctypes.c_void_p(qkv.data_ptr() + 2 * H * 2)
K_ptr = ctypes.c_void_p(qkv.data_ptr() + H * 2)
dbias = torch.zeros(3 * H, device=DEV)


def tr(src, dst, sb, ld):
    check(ext.ob_transpose_bf16_b(src, ptr(dst), S, hd, sb, hd, ld, B, nh,
                                  stream()))


def fwd_old():
    tr(V_ptr, VT, S * 3 * H, 3 * H)
    check(ext.ob_flash_fwd_bf16(ptr(qkv), ptr(VT), ptr(O), ptr(lse), B, S, H,
                                nh, scale, stream()))


def fwd_new():
    check(ext.ob_flash_fwd_nt_bf16(ptr(qkv), ptr(O), ptr(lse), B, S, H, nh,
                                   scale, stream()))


def bwd_old(colsum=False):
    tr(ptr(qkv), QT, S * 3 * H, 3 * H)
    tr(K_ptr, KT, S * 3 * H, 3 * H)
    tr(ptr(dO), dOT, S * H, H)
    check(ext.ob_flash_bwd_bf16(
        ptr(qkv), ptr(QT), ptr(KT), ptr(dOT), ptr(dO), ptr(lse), ptr(D),
        ptr(dqkv), B, S, H, nh, scale, stream()))
    if colsum:
        check(ext.ob_colsum_bf16(ptr(dqkv), ptr(dbias), B * S, 3 * H,
                                 stream()))


def bwd_new(bias=None):
    check(ext.ob_flash_bwd_nt_bf16(
        ptr(qkv), ptr(dO), ptr(lse), ptr(D), ptr(dqkv), ptr(bias), B, S, H,
        nh, scale, stream()))


def dsum():
    check(ext.ob_flash_dsum_bf16(ptr(O), ptr(dO), ptr(D), B, S, H, nh,
                                 stream()))


def dsum_bwd_new(bias=None):
    dsum()
    bwd_new(bias)


D_ws = torch.empty_like(D)


def bwd_new_d(bias=None):
    # dq forms D from O and dO itself and hands it to dkdv through D_ws
    check(ext.ob_flash_bwd_nt_d_bf16(
        ptr(qkv), ptr(O), ptr(dO), ptr(lse), ptr(D_ws), ptr(dqkv), ptr(bias),
        B, S, H, nh, scale, stream()))


# dropout key: any seed / layer / tick; the cost does not depend on them
DROP_KEY = ((0xDEADBEEF << 32) | 0x1234567, 5, (1 << 32) + 3)


def fwd_drop():
    check(ext.ob_flash_fwd_nt_drop_bf16(
        ptr(qkv), ptr(O), ptr(lse), B, S, H, nh, scale, DROP_KEY[0],
        DROP_KEY[1], DROP_KEY[2], args.attn_pdrop, stream()))


def bwd_drop(bias=None):
    check(ext.ob_flash_bwd_nt_d_drop_bf16(
        ptr(qkv), ptr(O), ptr(dO), ptr(lse), ptr(D_ws), ptr(dqkv), ptr(bias),
        B, S, H, nh, scale, DROP_KEY[0], DROP_KEY[1], DROP_KEY[2],
        args.attn_pdrop, stream()))


if hd == 128:
    fwd_new()
    dsum()
    torch.cuda.synchronize()
    unit = B * nh * S * S * hd * 1e-12  # TFLOP per causal GEMM pair / 2
    print(f"head_dim 128, (B, nh, S) = ({B}, {nh}, {S})")
    rows = [("fwd  nt                      ", fwd_new, 2),
            ("bwd  nt (dq + dkdv)          ", bwd_new, 5),
            ("bwd  nt + bias in-kernel     ", lambda: bwd_new(dbias), 5),
            ("dsum alone                   ", dsum, 0),
            ("bwd  nt, D in-kernel, + bias ", lambda: bwd_new_d(dbias), 5)]
    for name, fn, gemms in rows:
        us = timeit(fn) * 1e3
        tf = f" {gemms * unit / (us * 1e-6):7.1f} TF" if gemms else ""
        print(f"{name} {us:8.1f} us{tf}")
    sys.exit(0)

O_old = torch.empty_like(O)
fwd_old()
O_old.copy_(O)
fwd_new()
check(ext.ob_flash_dsum_bf16(ptr(O), ptr(dO), ptr(D), B, S, H, nh, stream()))
dq_old = torch.empty_like(dqkv)
bwd_old()
dq_old.copy_(dqkv)
bwd_new()
torch.cuda.synchronize()
print(f"nt outputs bit-identical: fwd {torch.equal(O, O_old)} "
      f"bwd {torch.equal(dqkv, dq_old)}")
dqkv.zero_()
bwd_new_d()
torch.cuda.synchronize()
print(f"D in-kernel bit-identical: D {torch.equal(D_ws, D)} "
      f"bwd {torch.equal(dqkv, dq_old)}")
rows = [("fwd  transpose + v4          ", fwd_old),
        ("fwd  nt                      ", fwd_new),
        ("bwd  3 transposes + dkdv + dq", bwd_old),
        ("bwd  nt (dkdv + dq)          ", bwd_new),
        ("bwd  old + colsum(dqkv)      ", lambda: bwd_old(True)),
        ("bwd  nt + bias in-kernel     ", lambda: bwd_new(dbias)),
        ("dsum alone                   ", dsum),
        ("dsum + bwd nt + bias         ", lambda: dsum_bwd_new(dbias)),
        ("bwd  nt, D in-kernel, + bias ", lambda: bwd_new_d(dbias))]
for name, fn in rows:
    print(f"{name} {timeit(fn)*1e3:8.1f} us")
if args.attn_pdrop > 0.0:
    fwd_drop()   # the dropout backward reads the dropout forward's O and lse
    torch.cuda.synchronize()
    rows = [(f"fwd  nt, dropout p={args.attn_pdrop}      ", fwd_drop),
            ("bwd  nt, D in-kernel, + bias, dropout", lambda: bwd_drop(dbias))]
    for name, fn in rows:
        print(f"{name} {timeit(fn)*1e3:8.1f} us")
