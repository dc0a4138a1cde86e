# @gpu parity for the bf16 MFMA path (§8 f4): the bf16 GEMM against a
# torch fp32 reference computed from the SAME bf16-rounded inputs (our
# kernel accumulates in fp32, so the comparison tolerance covers only the
# bf16 input rounding + fp32 sum-order effects).
import ctypes

import pytest
import torch

from tests.gpu_helpers import ptr, stream

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
DEV = "cuda:0"


def gemm_bf16(A, Bm, C, *, transA=0, transB=0, M, N, K, alpha=1.0, beta=0.0,
              lda, ldb, ldc, sA=(0, 0), sB=(0, 0), sC=(0, 0), n1=1, n2=1,
              bias=None, residual=None, out_kind=0, splitk=1):
    from oobleck_amd._ext import check, get_ext
    check(get_ext().ob_gemm_bf16(
        transA, transB, M, N, K, alpha, ptr(A), lda, sA[0], sA[1], ptr(Bm),
        ldb, sB[0], sB[1], beta, ptr(C), ldc, sC[0], sC[1], n1, n2, ptr(bias),
        ptr(residual), out_kind, splitk, stream()), "gemm_bf16")


def rb(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).bfloat16()


@requires_gpu
@pytest.mark.parametrize("tA,tB", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(128, 128, 32), (256, 384, 128),
                                   (200, 136, 72), (96, 64, 1024)])
def test_gemm_bf16_parity(tA, tB, M, N, K):
    # asymmetric operands (transpose-detecting, guide G9)
    A = rb(*(K, M) if tA else (M, K), seed=1)
    B = rb(*(N, K) if tB else (K, N), seed=2)
    lda, ldb = A.shape[1], B.shape[1]
    if lda % 8 or ldb % 8:
        pytest.skip("unaligned ld")
    C = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    gemm_bf16(A, B, C, transA=tA, transB=tB, M=M, N=N, K=K,
              lda=lda, ldb=ldb, ldc=N)
    Aop = (A.t() if tA else A).float()
    Bop = (B.t() if tB else B).float()
    ref = Aop @ Bop
    torch.cuda.synchronize()
    torch.testing.assert_close(C.float(), ref, rtol=2e-2, atol=2e-2)
    # tighter check in fp32-out mode (removes the output rounding)
    C32 = torch.empty(M, N, device=DEV, dtype=torch.float32)
    gemm_bf16(A, B, C32, transA=tA, transB=tB, M=M, N=N, K=K,
              lda=lda, ldb=ldb, ldc=N, out_kind=1)
    torch.cuda.synchronize()
    torch.testing.assert_close(C32, ref, rtol=1e-3, atol=1e-3)


@requires_gpu
def test_gemm_bf16_bias_residual_beta():
    M, N, K = 256, 256, 128
    A, B = rb(M, K, seed=3), rb(K, N, seed=4)
    bias = torch.randn(N, device=DEV)
    R = rb(M, N, seed=5)
    C = rb(M, N, seed=6)
    C0 = C.clone()
    gemm_bf16(A, B, C, M=M, N=N, K=K, lda=K, ldb=N, ldc=N, alpha=0.5,
              beta=1.0, bias=bias, residual=R)
    ref = 0.5 * (A.float() @ B.float()) + bias + R.float() + C0.float()
    torch.cuda.synchronize()
    torch.testing.assert_close(C.float(), ref, rtol=2e-2, atol=2e-2)


@requires_gpu
def test_gemm_bf16_atomic_splitk_f32out():
    M, N, K = 128, 384, 4096
    A = rb(K, M, seed=7)  # TA (the dW pattern)
    B = rb(K, N, seed=8)
    C = torch.zeros(M, N, device=DEV, dtype=torch.float32)
    gemm_bf16(A, B, C, transA=1, M=M, N=N, K=K, lda=M, ldb=N, ldc=N,
              out_kind=2, splitk=4)
    ref = A.t().float() @ B.float()
    torch.cuda.synchronize()
    torch.testing.assert_close(C, ref, rtol=2e-3, atol=2e-2)


@requires_gpu
def test_casts_roundtrip():
    from oobleck_amd._ext import check, get_ext
    x = torch.randn(1000, device=DEV)
    y = torch.empty(1000, device=DEV, dtype=torch.bfloat16)
    check(get_ext().ob_f32_to_bf16(ptr(x), ptr(y), 1000, stream()), "cast")
    torch.cuda.synchronize()
    torch.testing.assert_close(y, x.bfloat16())
    z = torch.empty(1000, device=DEV)
    check(get_ext().ob_bf16_to_f32(ptr(y), ptr(z), 1000, stream()), "cast2")
    torch.cuda.synchronize()
    torch.testing.assert_close(z, y.float())
    # transposed cast
    w = torch.randn(96, 288, device=DEV)
    wt = torch.empty(288, 96, device=DEV, dtype=torch.bfloat16)
    check(get_ext().ob_f32_to_bf16_t(ptr(w), ptr(wt), 96, 288, stream()),
          "cast_t")
    torch.cuda.synchronize()
    torch.testing.assert_close(wt, w.t().contiguous().bfloat16())


@requires_gpu
def test_gemm_bf16_batched_strided():
    Bn, S, hd = 4, 128, 64
    q = rb(Bn, S, hd, seed=9)
    k = rb(Bn, S, hd, seed=10)
    out = torch.empty(Bn, S, S, device=DEV, dtype=torch.bfloat16)
    gemm_bf16(q, k, out, transB=1, M=S, N=S, K=hd, lda=hd, ldb=hd, ldc=S,
              sA=(S * hd, 0), sB=(S * hd, 0), sC=(S * S, 0), n1=Bn, n2=1)
    ref = torch.matmul(q.float(), k.float().transpose(-1, -2))
    torch.cuda.synchronize()
    torch.testing.assert_close(out.float(), ref, rtol=2e-2, atol=2e-2)


# ---------------------------------------------------------------------------
# The two NT families the small ob_gemm_bf16 shapes above never route to, at
# the smallest shapes inside what the production dispatch sends them
# (M % 256, K % 64; K >= 1024 for the 256-row kernel).  Same tolerances as
# above: fp32 out 1e-3, bf16 out 2e-2, against torch fp32 on the bf16 inputs.
# ---------------------------------------------------------------------------

def _nt_case(M, N, K):
    A, B = rb(M, K, seed=11), rb(N, K, seed=12)  # asymmetric operands
    return A, B, A.float() @ B.float().t()


def _nt_out(M, N, out_kind):
    if out_kind == 0:
        return torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    return torch.zeros(M, N, device=DEV, dtype=torch.float32)


def _tol(out_kind):
    return dict(rtol=2e-2, atol=2e-2) if out_kind == 0 else \
        dict(rtol=1e-3, atol=1e-3)


def gemm_nt_8ph(A, B, C, M, N, K, *, out_kind, splitk=1, bias=None,
                residual=None):
    from oobleck_amd._ext import check, get_ext
    check(get_ext().ob_gemm_bf16_nt_8ph(
        ptr(A), ptr(B), ptr(C), ptr(bias), ptr(residual), M, N, K, K, K, N,
        0, 0, 0, 0, 0, 0, 1, 1, 1.0, 0.0, out_kind, splitk, stream(), M),
        "gemm_bf16_nt_8ph")


@requires_gpu
@pytest.mark.parametrize("out_kind,splitk", [(0, 1), (1, 1), (2, 2)])
@pytest.mark.parametrize("M,N,K", [(256, 256, 768), (512, 256, 1024)])
def test_gemm_bf16_nt_8ph_parity(M, N, K, out_kind, splitk):
    A, B, ref = _nt_case(M, N, K)
    C = _nt_out(M, N, out_kind)  # zeroed for the atomic split-K sum
    gemm_nt_8ph(A, B, C, M, N, K, out_kind=out_kind, splitk=splitk)
    torch.cuda.synchronize()
    torch.testing.assert_close(C.float(), ref, **_tol(out_kind))


@requires_gpu
def test_gemm_bf16_nt_8ph_bias_residual():
    M, N, K = 256, 256, 768
    A, B, ref = _nt_case(M, N, K)
    bias = torch.randn(N, device=DEV)
    R = rb(M, N, seed=13)
    C = _nt_out(M, N, 0)
    gemm_nt_8ph(A, B, C, M, N, K, out_kind=0, bias=bias, residual=R)
    torch.cuda.synchronize()
    torch.testing.assert_close(C.float(), ref + bias + R.float(), **_tol(0))


@requires_gpu
@pytest.mark.parametrize("out_kind", [0, 1])
@pytest.mark.parametrize("force,BN,M,N,K", [("n2", 256, 256, 256, 1024),
                                            ("n1", 128, 256, 128, 1024)])
def test_gemm_bf16_nt256_parity(monkeypatch, force, BN, M, N, K, out_kind):
    from oobleck_amd._ext import get_ext
    r = (ctypes.c_int32 * 5)()
    assert get_ext().ob_gemm_bf16_route(0, 1, M, N, K, 1, 1, out_kind, 1, 0.0,
                                        1, 0, force.encode(), r) == 0
    assert (r[1], r[2]) == (2, BN)  # the 256-row kernel at this N tile
    A, B, ref = _nt_case(M, N, K)
    C = _nt_out(M, N, out_kind)
    # OB_BF16_FORCE is read on every call
    monkeypatch.setenv("OB_BF16_FORCE", force)
    gemm_bf16(A, B, C, transB=1, M=M, N=N, K=K, lda=K, ldb=K, ldc=N,
              out_kind=out_kind)
    monkeypatch.delenv("OB_BF16_FORCE")
    torch.cuda.synchronize()
    torch.testing.assert_close(C.float(), ref, **_tol(out_kind))


# ---------------------------------------------------------------------------
# bf16 layer-path parity vs the fp32 oracle.  bf16 has an 8-bit mantissa:
# tolerances are the documented bf16 bound (BASELINE.md "separate documented
# tolerance for the bf16 path"): loss rel 2e-2; activation outputs rel/abs
# 5e-2; per-layer grads compared by relative L2 error < 5e-2 (elementwise
# bounds are meaningless for near-zero entries under bf16 rounding).
# ---------------------------------------------------------------------------

def rel_l2(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


@requires_gpu
def test_bf16_block_layer_parity():
    from oracle.gpt2_oracle import OracleConfig, stage_forward_backward
    from oracle.gpt2_oracle import init_layer_params
    from oobleck_amd.config import ModelConfig
    from oobleck_amd.layer import Layer
    dims = dict(n_embd=128, n_head=2, n_layer=2, n_positions=96,
                vocab_size=304)
    mc, oc = ModelConfig(**dims), OracleConfig(**dims)
    B, S = 2, 96
    flat = init_layer_params(oc, 1, 77)
    layer = Layer(1, mc, B, S, 2, torch.device(DEV), dtype="bf16")
    layer.flat_param.copy_(flat.to(DEV))
    layer.refresh_weights()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, S, 128, generator=g) * 0.5
    dout = torch.randn(B, S, 128, generator=g) * 0.1
    xg = x.to(DEV).bfloat16()
    out = torch.empty_like(xg)
    layer.forward_slot(0, xg, out)
    din = torch.empty_like(xg)
    layer.backward_slot(0, dout.to(DEV).bfloat16(), din)
    torch.cuda.synchronize()
    ref_out, ref_dx, (ref_grad,) = stage_forward_backward(
        oc, [flat], [1], x, dout=dout)
    assert rel_l2(out.float().cpu(), ref_out) < 5e-2
    assert rel_l2(din.float().cpu(), ref_dx) < 5e-2
    assert rel_l2(layer.flat_grad.cpu(), ref_grad) < 5e-2


@requires_gpu
def test_bf16_full_model_parity():
    from oracle.gpt2_oracle import OracleConfig, stage_forward_backward
    from oracle.gpt2_oracle import init_layer_params
    from oobleck_amd.config import ModelConfig
    from oobleck_amd.layer import Layer
    dims = dict(n_embd=128, n_head=2, n_layer=2, n_positions=96,
                vocab_size=304)
    mc, oc = ModelConfig(**dims), OracleConfig(**dims)
    B, S = 2, 96
    L = oc.n_layers_total
    flats = [init_layer_params(oc, oc.layer_kind(i), 300 + i)
             for i in range(L)]
    layers = []
    for lid in range(L):
        layer = Layer(lid, mc, B, S, 1, torch.device(DEV), dtype="bf16")
        layer.flat_param.copy_(flats[lid].to(DEV))
        layer.refresh_weights()
        layers.append(layer)
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, oc.vocab_size, (B, S), generator=g)
    x = ids.to(DEV)
    for lid, layer in enumerate(layers):
        if lid == L - 1:
            out = torch.zeros(1, device=DEV)
            layer.forward_slot(0, x, out, ids.to(DEV))
        else:
            out = torch.empty(B, S, 128, device=DEV, dtype=torch.bfloat16)
            layer.forward_slot(0, x, out)
        x = out
    dout = None
    for lid in range(L - 1, -1, -1):
        din = None if lid == 0 else torch.empty(B, S, 128, device=DEV,
                                                dtype=torch.bfloat16)
        layers[lid].backward_slot(0, dout, din)
        dout = din
    torch.cuda.synchronize()
    gpu_loss = x.item()
    ref_loss, _, ref_grads = stage_forward_backward(
        oc, flats, list(range(L)), ids, labels=ids.clone())
    assert abs(gpu_loss - ref_loss.item()) / abs(ref_loss.item()) < 2e-2, \
        (gpu_loss, ref_loss.item())
    for lid, layer in enumerate(layers):
        assert rel_l2(layer.flat_grad.cpu(), ref_grads[lid]) < 8e-2, lid


@requires_gpu
def test_bf16_per_layer_parity():
    """Per-layer bf16 bounds: every layer of the chain is
    compared against the oracle evaluated on THAT layer's own inputs (the
    bf16 activations the HIP layer actually consumed, upcast to fp32), so
    a single-block regression cannot hide inside a loose end-to-end bound.
    The residual error is one layer's bf16 rounding (operands + weight
    shadows) under fp32 accumulation: bounded at 1.5e-2 fwd / 3e-2 grads
    rel-L2, ~5x tighter than the whole-model smoke (8e-2)."""
    from oracle.gpt2_oracle import OracleConfig, stage_forward_backward
    from oracle.gpt2_oracle import init_layer_params
    from oobleck_amd.config import ModelConfig
    from oobleck_amd.layer import Layer
    # head_dim 64 + S % 128 == 0 -> the flash path is the one under test
    dims = dict(n_embd=128, n_head=2, n_layer=3, n_positions=128,
                vocab_size=304)
    mc, oc = ModelConfig(**dims), OracleConfig(**dims)
    B, S = 2, 128
    L = oc.n_layers_total
    flats = [init_layer_params(oc, oc.layer_kind(i), 600 + i)
             for i in range(L)]
    layers = []
    for lid in range(L):
        layer = Layer(lid, mc, B, S, 1, torch.device(DEV), dtype="bf16")
        layer.flat_param.copy_(flats[lid].to(DEV))
        layer.refresh_weights()
        layers.append(layer)
    g = torch.Generator().manual_seed(19)
    ids = torch.randint(0, oc.vocab_size, (B, S), generator=g)

    # forward chain: per-layer check on the layer's own input
    x = ids.to(DEV)
    fwd_inputs = []  # what each layer consumed (cpu fp32 / int64)
    for lid, layer in enumerate(layers):
        xin = x.float().cpu() if x.is_floating_point() else x.cpu()
        fwd_inputs.append(xin)
        if lid == L - 1:
            out = torch.zeros(1, device=DEV)
            layer.forward_slot(0, x, out, ids.to(DEV))
        else:
            out = torch.empty(B, S, dims["n_embd"], device=DEV,
                              dtype=torch.bfloat16)
            layer.forward_slot(0, x, out)
        torch.cuda.synchronize()
        if lid == L - 1:
            ref_loss, _, _ = stage_forward_backward(
                oc, [flats[lid]], [lid], xin, labels=ids.clone())
            assert abs(out.item() - ref_loss.item()) \
                < 1.5e-2 * abs(ref_loss.item()), (lid, out.item(),
                                                  ref_loss.item())
        else:
            ref_out, _, _ = stage_forward_backward(
                oc, [flats[lid]], [lid], xin, dout=torch.zeros_like(
                    xin if xin.is_floating_point()
                    else torch.zeros(B, S, dims["n_embd"])))
            assert rel_l2(out.float().cpu(), ref_out) < 1.5e-2, lid
        x = out

    # backward chain: per-layer check on the layer's own dout
    dout = None
    for lid in range(L - 1, -1, -1):
        layer = layers[lid]
        din = None if lid == 0 else torch.empty(B, S, dims["n_embd"],
                                                device=DEV,
                                                dtype=torch.bfloat16)
        dout_cpu = dout.float().cpu() if dout is not None else None
        layer.backward_slot(0, dout, din)
        torch.cuda.synchronize()
        if lid == L - 1:
            _, ref_dx, (ref_grad,) = stage_forward_backward(
                oc, [flats[lid]], [lid], fwd_inputs[lid], labels=ids.clone())
        else:
            _, ref_dx, (ref_grad,) = stage_forward_backward(
                oc, [flats[lid]], [lid], fwd_inputs[lid], dout=dout_cpu)
        assert rel_l2(layer.flat_grad.cpu(), ref_grad) < 3e-2, lid
        if din is not None and ref_dx is not None:
            assert rel_l2(din.float().cpu(), ref_dx) < 3e-2, lid
        dout = din


@requires_gpu
@pytest.mark.parametrize("B,nh,S", [(2, 2, 128), (1, 3, 256), (2, 2, 1024)])
def test_flash_fwd_bf16(B, nh, S):
    """Flash forward vs a torch fp32 reference of causal attention on the
    same bf16-rounded inputs."""
    import math
    from oobleck_amd._ext import check, get_ext
    H = nh * 64
    g = torch.Generator().manual_seed(31)
    qkv = (torch.randn(B, S, 3 * H, generator=g) * 0.5).to(DEV).bfloat16()
    VT = torch.empty(B * nh, 64, S, device=DEV, dtype=torch.bfloat16)
    # V slices: qkv[..., 2H + h*64 : ...] viewed [S, 64] at ld 3H
    check(get_ext().ob_transpose_bf16_b(
        ptr(qkv.flatten()[2 * H:]), ptr(VT), S, 64, S * 3 * H, 64, 3 * H,
        B, nh, stream()), "vt")
    O = torch.empty(B, S, H, device=DEV, dtype=torch.bfloat16)
    lse = torch.empty(B * nh, S, device=DEV, dtype=torch.float32)
    check(get_ext().ob_flash_fwd_bf16(
        ptr(qkv), ptr(VT), ptr(O), ptr(lse), B, S, H, nh,
        1.0 / math.sqrt(64.0), stream()), "flash")
    torch.cuda.synchronize()

    qf = qkv.float()
    q = qf[..., :H].view(B, S, nh, 64).permute(0, 2, 1, 3)
    k = qf[..., H:2 * H].view(B, S, nh, 64).permute(0, 2, 1, 3)
    v = qf[..., 2 * H:].view(B, S, nh, 64).permute(0, 2, 1, 3)
    w = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(64.0)
    mask = torch.tril(torch.ones(S, S, dtype=torch.bool, device=DEV))
    w = torch.where(mask, w, torch.tensor(float("-inf"), device=DEV))
    lse_ref = torch.logsumexp(w, dim=-1)            # [B, nh, S]
    P = torch.softmax(w, dim=-1)
    O_ref = torch.matmul(P, v).permute(0, 2, 1, 3).reshape(B, S, H)
    err = (O.float() - O_ref).norm() / O_ref.norm()
    assert err < 2e-2, err.item()
    torch.testing.assert_close(lse.view(B, nh, S), lse_ref,
                               rtol=1e-3, atol=1e-3)


@requires_gpu
@pytest.mark.parametrize("B,nh,S", [(2, 2, 128), (1, 3, 256), (2, 2, 512)])
def test_flash_bwd_bf16(B, nh, S):
    """Flash backward (recompute dQ/dK/dV) vs torch fp32 autograd of causal
    attention on the same bf16-rounded inputs."""
    import math
    from oobleck_amd._ext import check, get_ext
    H = nh * 64
    scale = 1.0 / math.sqrt(64.0)
    g = torch.Generator().manual_seed(41)
    qkv = (torch.randn(B, S, 3 * H, generator=g) * 0.5).to(DEV).bfloat16()
    dO = (torch.randn(B, S, H, generator=g) * 0.3).to(DEV).bfloat16()
    ext = get_ext()
    # forward to obtain O and lse
    VT = torch.empty(B * nh, 64, S, device=DEV, dtype=torch.bfloat16)
    check(ext.ob_transpose_bf16_b(
        ptr(qkv.flatten()[2 * H:]), ptr(VT), S, 64, S * 3 * H, 64, 3 * H,
        B, nh, stream()), "vt")
    O = torch.empty(B, S, H, device=DEV, dtype=torch.bfloat16)
    lse = torch.empty(B * nh, S, device=DEV, dtype=torch.float32)
    check(ext.ob_flash_fwd_bf16(ptr(qkv), ptr(VT), ptr(O), ptr(lse), B, S, H,
                                nh, scale, stream()), "ffwd")
    # transposes + D + backward
    QT = torch.empty(B * nh, 64, S, device=DEV, dtype=torch.bfloat16)
    KT = torch.empty_like(QT)
    dOT = torch.empty_like(QT)
    check(ext.ob_transpose_bf16_b(ptr(qkv), ptr(QT), S, 64, S * 3 * H, 64,
                                  3 * H, B, nh, stream()), "qt")
    check(ext.ob_transpose_bf16_b(ptr(qkv.flatten()[H:]), ptr(KT), S, 64,
                                  S * 3 * H, 64, 3 * H, B, nh, stream()),
          "kt")
    check(ext.ob_transpose_bf16_b(ptr(dO), ptr(dOT), S, 64, S * H, 64, H, B,
                                  nh, stream()), "dot")
    D = torch.empty(B * nh, S, device=DEV, dtype=torch.float32)
    check(ext.ob_flash_dsum_bf16(ptr(O), ptr(dO), ptr(D), B, S, H, nh,
                                 stream()), "dsum")
    dqkv = torch.empty_like(qkv)
    check(ext.ob_flash_bwd_bf16(ptr(qkv), ptr(QT), ptr(KT), ptr(dOT),
                                ptr(dO), ptr(lse), ptr(D), ptr(dqkv), B, S,
                                H, nh, scale, stream()), "fbwd")
    torch.cuda.synchronize()

    # fp32 autograd reference on the bf16-rounded inputs
    qf = qkv.float().requires_grad_(True)
    q = qf[..., :H].view(B, S, nh, 64).permute(0, 2, 1, 3)
    k = qf[..., H:2 * H].view(B, S, nh, 64).permute(0, 2, 1, 3)
    v = qf[..., 2 * H:].view(B, S, nh, 64).permute(0, 2, 1, 3)
    w = torch.matmul(q, k.transpose(-1, -2)) * scale
    mask = torch.tril(torch.ones(S, S, dtype=torch.bool, device=DEV))
    w = torch.where(mask, w, torch.tensor(float("-inf"), device=DEV))
    P = torch.softmax(w, dim=-1)
    O_ref = torch.matmul(P, v).permute(0, 2, 1, 3).reshape(B, S, H)
    O_ref.backward(dO.float())
    ref = qf.grad
    # D parity as a unit check too
    D_ref = (O.float() * dO.float()).view(B, S, nh, 64).sum(-1)
    torch.testing.assert_close(D.view(B, nh, S),
                               D_ref.permute(0, 2, 1).contiguous(),
                               rtol=1e-2, atol=1e-2)
    for name, sl in (("dQ", slice(0, H)), ("dK", slice(H, 2 * H)),
                     ("dV", slice(2 * H, 3 * H))):
        e = rel_l2(dqkv[..., sl].float(), ref[..., sl])
        assert e < 3e-2, (name, e)


@requires_gpu
def test_bf16_block_layer_parity_flash():
    """Same as test_bf16_block_layer_parity but at S=128 / head_dim=64 so
    the fused flash path is auto-selected (use_flash, ob_layer.hip)."""
    from oracle.gpt2_oracle import OracleConfig, stage_forward_backward
    from oracle.gpt2_oracle import init_layer_params
    from oobleck_amd.config import ModelConfig
    from oobleck_amd.layer import Layer
    dims = dict(n_embd=128, n_head=2, n_layer=2, n_positions=128,
                vocab_size=304)
    mc, oc = ModelConfig(**dims), OracleConfig(**dims)
    B, S = 2, 128
    flat = init_layer_params(oc, 1, 77)
    layer = Layer(1, mc, B, S, 2, torch.device(DEV), dtype="bf16")
    layer.flat_param.copy_(flat.to(DEV))
    layer.refresh_weights()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, S, 128, generator=g) * 0.5
    dout = torch.randn(B, S, 128, generator=g) * 0.1
    xg = x.to(DEV).bfloat16()
    out = torch.empty_like(xg)
    layer.forward_slot(0, xg, out)
    din = torch.empty_like(xg)
    layer.backward_slot(0, dout.to(DEV).bfloat16(), din)
    torch.cuda.synchronize()
    ref_out, ref_dx, (ref_grad,) = stage_forward_backward(
        oc, [flat], [1], x, dout=dout)
    assert rel_l2(out.float().cpu(), ref_out) < 5e-2
    assert rel_l2(din.float().cpu(), ref_dx) < 5e-2
    assert rel_l2(layer.flat_grad.cpu(), ref_grad) < 5e-2


@requires_gpu
@pytest.mark.parametrize("R,H", [(512, 768), (300, 1024), (1000, 512)])
def test_ln_bwd_bf16_wave(R, H):
    """Wave-per-row ln backward (H>=512 path) vs torch fp32 on the same
    bf16-rounded inputs."""
    from oobleck_amd._ext import check, get_ext
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(R, H, generator=g)).cuda().bfloat16()
    dy = (torch.randn(R, H, generator=g) * 0.5).cuda().bfloat16()
    w = torch.randn(H, generator=g).cuda().float()
    b = torch.randn(H, generator=g).cuda().float()
    xf = x.float().requires_grad_(True)
    mu = xf.mean(-1, keepdim=True)
    var = xf.var(-1, unbiased=False, keepdim=True)
    y = (xf - mu) / torch.sqrt(var + 0.0) * w + b
    y.backward(dy.float())
    mean = x.float().mean(-1).contiguous()
    rstd = (1.0 / x.float().var(-1, unbiased=False).sqrt()).contiguous()
    dx = torch.empty_like(x)
    dw = torch.zeros(H, device=DEV, dtype=torch.float32)
    db = torch.zeros(H, device=DEV, dtype=torch.float32)
    check(get_ext().ob_layernorm_bwd_bf16(
        ptr(x), ptr(w), ptr(mean), ptr(rstd), ptr(dy), ptr(dx), ptr(dw),
        ptr(db), R, H, 0, stream()), "lnbwd")
    torch.cuda.synchronize()
    assert rel_l2(dx.float(), xf.grad) < 3e-2
    assert rel_l2(dw, (dy.float() * (x.float() - mu) *
                       (var + 0.0).rsqrt()).sum(0)) < 2e-2
    assert rel_l2(db, dy.float().sum(0)) < 2e-2


@requires_gpu
@pytest.mark.parametrize("M,N", [(8192, 768), (1000, 3072), (129, 520),
                                 (64, 40)])
def test_colsum_bf16_v9(M, N):
    from oobleck_amd._ext import check, get_ext
    g = torch.Generator().manual_seed(6)
    x = (torch.randn(M, N, generator=g)).cuda().bfloat16()
    db = torch.zeros(N, device=DEV, dtype=torch.float32)
    check(get_ext().ob_colsum_bf16(ptr(x), ptr(db), M, N, stream()), "cs")
    torch.cuda.synchronize()
    assert rel_l2(db, x.float().sum(0)) < 2e-2


@requires_gpu
@pytest.mark.parametrize("R,H", [(512, 768), (301, 1024), (77, 520)])
def test_ln_fwd_bf16_wave(R, H):
    from oobleck_amd._ext import check, get_ext
    g = torch.Generator().manual_seed(15)
    x = (torch.randn(R, H, generator=g)).cuda().bfloat16()
    w = torch.randn(H, generator=g).cuda().float()
    b = torch.randn(H, generator=g).cuda().float()
    y = torch.empty_like(x)
    mean = torch.empty(R, device=DEV, dtype=torch.float32)
    rstd = torch.empty(R, device=DEV, dtype=torch.float32)
    check(get_ext().ob_layernorm_fwd_bf16(
        ptr(x), ptr(w), ptr(b), ptr(y), ptr(mean), ptr(rstd), R, H, 1e-5,
        stream()), "lnfwd")
    torch.cuda.synchronize()
    xf = x.float()
    mu = xf.mean(-1, keepdim=True)
    var = xf.var(-1, unbiased=False, keepdim=True)
    ref = (xf - mu) * (var + 1e-5).rsqrt() * w + b
    assert rel_l2(y.float(), ref) < 2e-2
    torch.testing.assert_close(mean, mu.squeeze(-1), rtol=1e-3, atol=1e-3)


@requires_gpu
def test_lt_plain_nt_parity():
    """The hipBLASLt plain-GEMM route (M*N >= 512^2, no epilogue) vs
    torch fp32 on bf16-rounded inputs (ob_blaslt.hip column-major swap)."""
    M, N, K = 1024, 768, 320
    A = rb(M, K, seed=21)
    B = rb(N, K, seed=22)
    C = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    gemm_bf16(A, B, C, transB=1, M=M, N=N, K=K, lda=K, ldb=K, ldc=N)
    torch.cuda.synchronize()
    ref = A.float() @ B.float().T
    assert rel_l2(C.float(), ref) < 2e-2


@requires_gpu
def test_lt_bias_epilogue_parity():
    from oobleck_amd._ext import check, get_ext
    M, N, K = 1024, 1024, 256
    A = rb(M, K, seed=23)
    B = rb(N, K, seed=24)
    bias = torch.randn(N, device=DEV, dtype=torch.float32)
    C = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    gemm_bf16(A, B, C, transB=1, M=M, N=N, K=K, lda=K, ldb=K, ldc=N,
              bias=bias)
    torch.cuda.synchronize()
    ref = A.float() @ B.float().T + bias
    assert rel_l2(C.float(), ref) < 2e-2


@requires_gpu
def test_lt_tn_beta1_accumulate():
    """Direct-TN dW route: C_f32 += A^T B with beta=1 (the weight-grad
    accumulation path, ob_gemm_lt c_f32=1)."""
    import ctypes
    from oobleck_amd._ext import check, get_ext
    BS, W1, W2 = 768, 512, 640
    A = rb(BS, W1, seed=25)
    B = rb(BS, W2, seed=26)
    C = torch.randn(W1, W2, device=DEV, dtype=torch.float32)
    C0 = C.clone()
    r = get_ext().ob_gemm_lt(1, 0, W1, W2, BS, ctypes.c_float(1.0), ptr(A),
                             W1, ptr(B), W2, ctypes.c_float(1.0), ptr(C),
                             W2, 1, stream())
    torch.cuda.synchronize()
    if r == -1:
        pytest.skip("hipBLASLt offered no algo for this shape")
    assert r == 0
    ref = C0 + A.float().T @ B.float()
    assert rel_l2(C, ref) < 2e-2
