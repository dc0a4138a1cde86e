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
# backward (5 GEMMs).  With --attn-pdrop P it adds the head_dim 128 dropout
# entries (ob_flash_fwd_drop_hd128_bf16 / ob_flash_bwd_d_drop_hd128_bf16)
# and their ratio to the plain rows.  The default, --head-dim 64, prints what
# it always did.
#
# --window W (0 < W < S) times the locally banded entries
# (ob_flash_fwd_win_bf16 / ob_flash_bwd_win_d_bf16) against the dense ones at
# --head-dim / --shape: the two arms alternate, --repeats times, each repeat
# the mean of 30 back-to-back calls between device events; it prints every
# repeat, min / max per arm and dense / window of the minima, with the dense
# arm's own max - min next to the margin.  The backward rows are dq + dkdv
# together; the three kernels on their own come from a kernel trace of this
# same command (tools/kstats.py), where the two arms' kernels have different
# names.
#
# --head-dim 80 / 96 go through ob_flash_fwd_hd96_bf16 /
# ob_flash_bwd_hd96_d_bf16, whose dense and banded arms are one kernel set:
# without --window it prints --repeats repeats of the dense forward and
# backward with min / max and TF; with --window the A/B above (plus the TF of
# both arms' minima: causal FLOPs times band / triangle for the window arm).
#
# --attn-pdrop P together with --window W, or with --head-dim 80 / 96 (then
# also without a window: the dense arm), times the dropout entries of those
# kernels (ob_flash_*_win_drop_bf16 / ob_flash_*_hd96_drop_bf16) against the
# plain ones at the same window: the A/B above with the arms "plain" and
# "drop", and drop / plain of the minima.
#
# --n-kv N (with --head-dim 128, N a proper divisor of nh) times the
# grouped-query entries (ob_flash_fwd_gqa_bf16 / ob_flash_bwd_gqa_d_bf16, N
# K/V heads) against the dense head_dim 128 ones at the same --shape: the
# forward, and the backward at every split that divides nh / N.  The arms
# alternate in one process, --repeats rounds of 30 back-to-back calls between
# device events; it prints every round, each arm's median and max - min, and
# the TF of the median.  The backward rows differ only in their dkdv (and
# fold) launches: the dq kernel is the same in every gqa row.
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
ap.add_argument("--head-dim", type=int, default=64, choices=(64, 80, 96, 128))
ap.add_argument("--shape", default="8,12,1024", metavar="B,nh,S")
ap.add_argument("--window", type=int, default=0, metavar="W",
                help="time the banded entries against the dense ones")
ap.add_argument("--n-kv", type=int, default=0, metavar="N",
                help="time the grouped-query entries against the dense ones")
ap.add_argument("--repeats", type=int, default=7)
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


if hd in (80, 96):  # one entry pair, dense = window 0
    def fwd_new():
        check(ext.ob_flash_fwd_hd96_bf16(ptr(qkv), ptr(O), ptr(lse), B, S, H,
                                         nh, 0, scale, stream()))

    def bwd_new_d(bias=None):
        check(ext.ob_flash_bwd_hd96_d_bf16(
            ptr(qkv), ptr(O), ptr(dO), ptr(lse), ptr(D_ws), ptr(dqkv),
            ptr(bias), B, S, H, nh, 0, scale, stream()))


# dropout key: any seed / layer / tick; the cost does not depend on them
DROP_KEY = ((0xDEADBEEF << 32) | 0x1234567, 5, (1 << 32) + 3)


fwd_drop_entry, bwd_drop_entry = (
    (ext.ob_flash_fwd_drop_hd128_bf16, ext.ob_flash_bwd_d_drop_hd128_bf16)
    if hd == 128 else
    (ext.ob_flash_fwd_nt_drop_bf16, ext.ob_flash_bwd_nt_d_drop_bf16))


def fwd_drop():
    check(fwd_drop_entry(
        ptr(qkv), ptr(O), ptr(lse), B, S, H, nh, scale, DROP_KEY[0],
        DROP_KEY[1], DROP_KEY[2], args.attn_pdrop, stream()))


def bwd_drop(bias=None):
    check(bwd_drop_entry(
        ptr(qkv), ptr(O), ptr(dO), ptr(lse), ptr(D_ws), ptr(dqkv), ptr(bias),
        B, S, H, nh, scale, DROP_KEY[0], DROP_KEY[1], DROP_KEY[2],
        args.attn_pdrop, stream()))


def timeit_once(fn, reps=30):
    st, en = torch.cuda.Event(True), torch.cuda.Event(True)
    st.record()
    for _ in range(reps):
        fn()
    en.record()
    torch.cuda.synchronize()
    return st.elapsed_time(en) / reps * 1e3


if args.n_kv:
    n_kv = args.n_kv
    assert hd == 128 and 0 < n_kv < nh and nh % n_kv == 0, \
        "--n-kv needs --head-dim 128 and a proper divisor of nh"
    G, Hkv = nh // n_kv, 128 * n_kv
    qkv_g = (torch.randn(B, S, H + 2 * Hkv, generator=g) * 0.3) \
        .to(DEV).bfloat16()
    dqkv_g = torch.zeros_like(qkv_g)
    dbias_g = torch.zeros(H + 2 * Hkv, device=DEV)
    O_g, lse_g, D_g = torch.empty_like(O), torch.empty_like(lse), \
        torch.empty_like(D)
    slab = torch.empty(G * B * S * 2 * Hkv, device=DEV)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rule = ext.ob_flash_gqa_split(B, S, nh, n_kv, cus)

    def fwd_gqa():
        check(ext.ob_flash_fwd_gqa_bf16(ptr(qkv_g), ptr(O_g), ptr(lse_g), B,
                                        S, H, nh, n_kv, scale, stream()))

    def bwd_gqa(split):
        return lambda: check(ext.ob_flash_bwd_gqa_d_bf16(
            ptr(qkv_g), ptr(O_g), ptr(dO), ptr(lse_g), ptr(D_g), ptr(dqkv_g),
            ptr(dbias_g), B, S, H, nh, n_kv, split, ptr(slab), slab.numel(),
            scale, stream()))

    splits = [s for s in range(1, G + 1) if G % s == 0]
    print(f"head_dim 128, (B, nh, n_kv, S) = ({B}, {nh}, {n_kv}, {S}), "
          f"{cus} CUs: dkdv blocks at split 1 = {B * n_kv * (S // 64)}, "
          f"ob_flash_gqa_split = {rule}")
    fwd_new()
    fwd_gqa()  # each backward reads the O and lse of its own arm's forward
    unit = B * nh * S * S * hd * 1e-6  # MFLOP per causal GEMM pair / 2
    for title, gemms, arms in (
            ("fwd", 2, [("mha", fwd_new), ("gqa", fwd_gqa)]),
            ("bwd (dq + dkdv [+ fold], D in-kernel, + bias)", 5,
             [("mha", lambda: bwd_new_d(dbias))] +
             [(f"gqa split {s}", bwd_gqa(s)) for s in splits])):
        for _, fn in arms:
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        us = [[] for _ in arms]
        for _ in range(args.repeats):  # the arms alternate
            for a, (_, fn) in enumerate(arms):
                us[a].append(timeit_once(fn))
        print(title)
        for (name, _), v in zip(arms, us):
            med = sorted(v)[len(v) // 2]
            print(f"  {name:12s} us: " + " ".join(f"{x:7.1f}" for x in v) +
                  f" | median {med:.1f} spread {max(v) - min(v):.1f}; "
                  f"{gemms * unit / med:.1f} TF")
    sys.exit(0)

if args.attn_pdrop > 0.0 and (args.window or hd in (80, 96)):
    W = args.window
    assert 0 <= W < S, "--window must be in (0, S)"
    fam = "hd96" if hd in (80, 96) else "win"
    key = (*DROP_KEY, args.attn_pdrop)

    def arm(drop):
        f = getattr(ext, f"ob_flash_fwd_{fam}{'_drop' * drop}_bf16")
        b = getattr(ext, f"ob_flash_bwd_{fam}_d{'_drop' * drop}_bf16")
        tail = (W, scale) + (key if drop else ()) + (stream(),)
        return (lambda: check(f(ptr(qkv), ptr(O), ptr(lse), B, S, H, nh,
                                *tail)),
                lambda: check(b(ptr(qkv), ptr(O), ptr(dO), ptr(lse),
                                ptr(D_ws), ptr(dqkv), ptr(dbias), B, S, H, nh,
                                *tail)))

    (fwd_p, bwd_p), (fwd_d, bwd_d) = arm(0), arm(1)
    print(f"head_dim {hd}, (B, nh, S) = ({B}, {nh}, {S}), window {W or 'none'}"
          f", attn_pdrop {args.attn_pdrop}")
    # each backward reads the O and lse of its own arm's forward
    for name, plain, drop, pre in (
            ("fwd", fwd_p, fwd_d, (None, None)),
            ("bwd (dq + dkdv, D in-kernel, + bias)", bwd_p, bwd_d,
             (fwd_p, fwd_d))):
        for fn in (plain, drop):
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        us = ([], [])
        for _ in range(args.repeats):
            for a, fn in enumerate((plain, drop)):
                if pre[a]:
                    pre[a]()
                us[a].append(timeit_once(fn))
        p_, d_ = us
        print(f"{name}")
        print("  plain us: " + " ".join(f"{v:7.1f}" for v in p_))
        print("  drop  us: " + " ".join(f"{v:7.1f}" for v in d_))
        print(f"  plain min {min(p_):.1f} max {max(p_):.1f}; drop min "
              f"{min(d_):.1f} max {max(d_):.1f}; drop / plain = "
              f"{min(d_) / min(p_):.2f}")
    sys.exit(0)

if args.window:
    W = args.window
    assert 0 < W < S, "--window must be in (0, S)"

    fwd_win_entry, bwd_win_entry = (
        (ext.ob_flash_fwd_hd96_bf16, ext.ob_flash_bwd_hd96_d_bf16)
        if hd in (80, 96) else
        (ext.ob_flash_fwd_win_bf16, ext.ob_flash_bwd_win_d_bf16))

    def fwd_win():
        check(fwd_win_entry(ptr(qkv), ptr(O), ptr(lse), B, S, H,
                                        nh, W, scale, stream()))

    def bwd_win():
        check(bwd_win_entry(
            ptr(qkv), ptr(O), ptr(dO), ptr(lse), ptr(D_ws), ptr(dqkv),
            ptr(dbias), B, S, H, nh, W, scale, stream()))

    work = (S * W - W * W / 2) / (S * S / 2)
    print(f"head_dim {hd}, (B, nh, S) = ({B}, {nh}, {S}), window {W}: "
          f"band / triangle = {work:.3f} of the MFMA work")
    # each backward reads the O and lse of its own arm's forward
    unit = B * nh * S * S * hd * 1e-6  # MFLOP per causal GEMM pair / 2
    for name, dense, win, pre, gemms in (
            ("fwd", fwd_new, fwd_win, (None, None), 2),
            ("bwd (dq + dkdv, D in-kernel, + bias)",
             lambda: bwd_new_d(dbias), bwd_win, (fwd_new, fwd_win), 5)):
        for fn in (dense, win):
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        us = ([], [])
        for _ in range(args.repeats):
            for arm, fn in enumerate((dense, win)):
                if pre[arm]:
                    pre[arm]()
                us[arm].append(timeit_once(fn))
        d, w_ = us
        print(f"{name}")
        print("  dense  us: " + " ".join(f"{v:7.1f}" for v in d))
        print("  window us: " + " ".join(f"{v:7.1f}" for v in w_))
        print(f"  dense min {min(d):.1f} max {max(d):.1f} (spread "
              f"{max(d) - min(d):.1f}); window min {min(w_):.1f} max "
              f"{max(w_):.1f}; dense / window = {min(d) / min(w_):.2f}; "
              f"margin {min(d) - max(w_):.1f} us")
        print(f"  dense {gemms * unit / min(d):.1f} TF; window "
              f"{gemms * unit * work / min(w_):.1f} TF")
    sys.exit(0)

if hd in (80, 96):
    unit = B * nh * S * S * hd * 1e-6  # MFLOP per causal GEMM pair / 2
    print(f"head_dim {hd}, (B, nh, S) = ({B}, {nh}, {S})")
    fwd_new()  # the backward reads this forward's O and lse
    for name, fn, gemms in (
            ("fwd", fwd_new, 2),
            ("bwd (dq + dkdv, D in-kernel, + bias)",
             lambda: bwd_new_d(dbias), 5)):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        us = [timeit_once(fn) for _ in range(args.repeats)]
        print(f"{name}")
        print("  us: " + " ".join(f"{v:7.1f}" for v in us))
        print(f"  min {min(us):.1f} max {max(us):.1f}; "
              f"{gemms * unit / min(us):.1f} TF")
    sys.exit(0)

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
    took = {}
    for name, fn, gemms in rows:
        us = took[name] = timeit(fn) * 1e3
        tf = f" {gemms * unit / (us * 1e-6):7.1f} TF" if gemms else ""
        print(f"{name} {us:8.1f} us{tf}")
    if args.attn_pdrop > 0.0:
        fwd_drop()  # the dropout backward reads this forward's O and lse
        torch.cuda.synchronize()
        for name, fn, gemms, plain in (
                (f"fwd  dropout p={args.attn_pdrop}           ", fwd_drop, 2,
                 rows[0][0]),
                (f"bwd  dropout p={args.attn_pdrop}, D, + bias", lambda:
                 bwd_drop(dbias), 5, rows[4][0])):
            us = timeit(fn) * 1e3
            print(f"{name} {us:8.1f} us {gemms * unit / (us * 1e-6):7.1f} TF"
                  f"  x{us / took[plain]:.2f} of the plain row")
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
