# The computations of tests/test_gpu_lt_tune.py, importable so the test runs
# them in its own process (tuning on) and, as a script, in a child whose
# OB_LT_TUNE the parent sets (the switch is read once per process): the four
# library GEMM variants on seeded inputs, and one forward + backward of a
# small bf16 BLOCK and FINAL layer.  As a script it saves every result to the
# path in argv[1].
import ctypes
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from oobleck_amd._ext import check, get_ext, lt_shape  # noqa: E402

DEV = "cuda:0"
# the smallest shapes at which layout, ld and epilogue mistakes show: an
# interior one, a ragged one, one narrower than a tile
SHAPES = [(256, 384, 128), (200, 136, 72), (128, 64, 128)]
VARIANTS = ["nt_bias", "nt_bias_res", "nn", "tn_beta1"]
f32 = ctypes.c_float


def ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def rb(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV).bfloat16()


def key(variant, M, N, K, lda=None):
    """(tA, tB, M, N, K, lda, ldb, ldc, c_f32, beta1, bias, cin, ab_f32)"""
    if variant == "nt_bias":
        return (0, 1, M, N, K, lda or K, K, N, 0, 0, 1, 0, 0)
    if variant == "nt_bias_res":
        return (0, 1, M, N, K, lda or K, K, N, 0, 1, 1, 1, 0)
    if variant == "nn":
        return (0, 0, M, N, K, lda or K, N, N, 0, 0, 0, 0, 0)
    return (1, 0, M, N, K, lda or M, N, N, 1, 1, 0, 0, 0)


def operands(variant, M, N, K, lda=None):
    """Seeded operands; a padded A (lda > its row length) keeps garbage in
    the pad columns, which no correct layout reads."""
    rows, cols = (K, M) if variant == "tn_beta1" else (M, K)
    A = rb(rows, lda or cols, seed=31)
    B = rb(N, K, seed=32) if variant.startswith("nt") else rb(K, N, seed=32)
    g = torch.Generator().manual_seed(33)
    bias = torch.randn(N, generator=g).to(DEV)
    res = rb(M, N, seed=34)
    C0 = torch.randn(M, N, generator=g).to(DEV)
    return A, B, bias, res, C0


def reference(variant, M, N, K, ops):
    A, B, bias, res, C0 = ops
    if variant == "tn_beta1":
        return C0 + 2 * (A[:, :M].float().T @ B.float())
    Bop = B.float().T if variant.startswith("nt") else B.float()
    ref = A[:, :K].float() @ Bop
    if variant != "nn":
        ref = ref + bias
    if variant == "nt_bias_res":
        ref = ref + res.float()
    return ref


def run_gemm(variant, M, N, K, ops, lda=None, strm=None):
    """One variant through its ob_gemm_lt* entry; returns the output."""
    A, B, bias, res, C0 = ops
    ext, s = get_ext(), strm or stream()
    if variant == "tn_beta1":
        C = C0.clone()
        for _ in range(2):  # accumulates twice into a non-zero C
            rc = ext.ob_gemm_lt(1, 0, M, N, K, f32(1), ptr(A), lda or M,
                                ptr(B), N, f32(1), ptr(C), N, 1, s)
            assert rc == 0, (rc, ext.ob_last_error())
        return C
    C = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    if variant == "nt_bias":
        rc = ext.ob_gemm_lt_bias(0, 1, M, N, K, f32(1), ptr(A), lda or K,
                                 ptr(B), K, f32(0), ptr(C), N, 0, ptr(bias), s)
    elif variant == "nt_bias_res":
        rc = ext.ob_gemm_lt_bias_res(0, 1, M, N, K, f32(1), ptr(A), lda or K,
                                     ptr(B), K, ptr(C), N, 0, ptr(bias),
                                     ptr(res), s)
    else:
        rc = ext.ob_gemm_lt(0, 0, M, N, K, f32(1), ptr(A), lda or K, ptr(B),
                            N, f32(0), ptr(C), N, 0, s)
    assert rc == 0, (rc, ext.ob_last_error())
    return C


def tune(shape_key):
    check(get_ext().ob_gemm_lt_tune(lt_shape(*shape_key)), "gemm_lt_tune")


def run_gemms():
    """{(variant, M, N, K): output} after tuning each key (a no-op under
    OB_LT_TUNE=0)."""
    out = {}
    for M, N, K in SHAPES:
        for v in VARIANTS:
            tune(key(v, M, N, K))
            out[(v, M, N, K)] = run_gemm(v, M, N, K, operands(v, M, N, K))
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in out.items()}


LAYER_DIMS = dict(n_embd=128, n_head=2, n_layer=2, n_positions=128,
                  vocab_size=1000)
LAYER_B, LAYER_S = 2, 128


def run_layers():
    """One forward + backward of a flash-eligible bf16 BLOCK layer and of a
    FINAL layer (V = 1000), created here (which tunes their shapes)."""
    from oobleck_amd.config import ModelConfig
    from oobleck_amd.layer import Layer
    mc = ModelConfig(**LAYER_DIMS)
    B, S, H = LAYER_B, LAYER_S, LAYER_DIMS["n_embd"]
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(8)
    x = (torch.randn(B, S, H, generator=g) * 0.5).to(DEV).bfloat16()
    dout = (torch.randn(B, S, H, generator=g) * 0.1).to(DEV).bfloat16()
    ids = torch.randint(0, LAYER_DIMS["vocab_size"], (B, S), generator=g)
    res = {}
    block = Layer(1, mc, B, S, 2, dev, dtype="bf16")
    out, din = torch.empty_like(x), torch.empty_like(x)
    block.forward_slot(0, x, out)
    block.backward_slot(0, dout, din)
    final = Layer(LAYER_DIMS["n_layer"] + 1, mc, B, S, 1, dev, dtype="bf16")
    loss, fdin = torch.zeros(1, device=DEV), torch.empty_like(x)
    final.forward_slot(0, x, loss, ids.to(DEV))
    final.backward_slot(0, None, fdin)
    torch.cuda.synchronize()
    res = {"block_out": out, "block_din": din, "block_grad": block.flat_grad,
           "final_loss": loss, "final_din": fdin,
           "final_grad": final.flat_grad}
    return {k: t.float().cpu() for k, t in res.items()}, (block, final)


if __name__ == "__main__":
    layers, _keep = run_layers()
    torch.save({"gemms": run_gemms(), "layers": layers}, sys.argv[1])
