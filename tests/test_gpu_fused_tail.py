# @gpu parity for the fused HBM-bound tail of the bf16 transformer block:
# ln forward that also writes the stash copy, ln backward with a separate
# residual source and two bias-grad side sums, gelu backward that also
# produces the b_fc bias grad.  References are torch fp32 on the SAME
# bf16-rounded inputs, never the extension's own output; the bounds are
# those of the unfused kernels' tests in test_gpu_bf16.py.
import pytest
import torch

from tests.gpu_helpers import ptr, stream

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
DEV = "cuda:0"


def rel_l2(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _ext():
    from oobleck_amd._ext import check, get_ext
    return get_ext(), check


# ---------------------------------------------------------------------------
# ln forward + stash copy
# ---------------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("with_copy", [True, False])
@pytest.mark.parametrize("R,H", [(512, 768), (301, 1024), (77, 520),
                                 (40, 1600)])
def test_ln_fwd_copy(R, H, with_copy):
    """(301,1024): odd trailing row; (77,520): one lane in the second
    half-row and a partial block; (40,1600): composed (non-wave) path."""
    ext, check = _ext()
    g = torch.Generator().manual_seed(15)
    x = (torch.randn(R, H, generator=g)).cuda().bfloat16()
    w = torch.randn(H, generator=g).cuda().float()
    b = torch.randn(H, generator=g).cuda().float()
    y = torch.empty_like(x)
    sentinel = torch.full_like(x, 7.0)
    xcopy = sentinel.clone() if with_copy else None
    mean = torch.empty(R, device=DEV, dtype=torch.float32)
    rstd = torch.empty(R, device=DEV, dtype=torch.float32)
    check(ext.ob_layernorm_fwd_copy_bf16(
        ptr(x), ptr(w), ptr(b), ptr(y), ptr(xcopy), ptr(mean), ptr(rstd), R,
        H, 1e-5, stream()), "lnfwd_copy")
    torch.cuda.synchronize()
    xf = x.float()
    mu = xf.mean(-1, keepdim=True)
    var = xf.var(-1, unbiased=False, keepdim=True)
    ref = (xf - mu) * (var + 1e-5).rsqrt() * w + b
    assert rel_l2(y.float(), ref) < 3e-2
    torch.testing.assert_close(mean, mu.squeeze(-1), rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(rstd, (var + 1e-5).rsqrt().squeeze(-1),
                               rtol=1e-3, atol=1e-3)
    if with_copy:
        assert torch.equal(xcopy.view(torch.int16), x.view(torch.int16))
    else:
        # null xcopy behaves as the plain entry point: same y bit for bit
        y2 = torch.empty_like(x)
        check(ext.ob_layernorm_fwd_bf16(
            ptr(x), ptr(w), ptr(b), ptr(y2), ptr(mean), ptr(rstd), R, H,
            1e-5, stream()), "lnfwd")
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int16), y2.view(torch.int16))


# ---------------------------------------------------------------------------
# ln backward + residual source + side sums
# ---------------------------------------------------------------------------

def _ln_bwd_case(R, H, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(R, H, generator=g)).cuda().bfloat16()
    dy = (torch.randn(R, H, generator=g) * 0.5).cuda().bfloat16()
    res = (torch.randn(R, H, generator=g) * 0.5).cuda().bfloat16()
    w = torch.randn(H, generator=g).cuda().float()
    b = torch.randn(H, generator=g).cuda().float()
    pre = [torch.randn(H, generator=g).cuda().float() for _ in range(4)]
    xf = x.float().requires_grad_(True)
    mu = xf.mean(-1, keepdim=True)
    var = xf.var(-1, unbiased=False, keepdim=True)
    yy = (xf - mu) / torch.sqrt(var + 0.0) * w + b
    yy.backward(dy.float())
    mean = x.float().mean(-1).contiguous()
    rstd = (1.0 / x.float().var(-1, unbiased=False).sqrt()).contiguous()
    ref = dict(
        v=xf.grad.detach(),
        dx=(res.float() + xf.grad).bfloat16(),
        dw=(dy.float() * (x.float() - mu.detach()) *
            (var.detach() + 0.0).rsqrt()).sum(0),
        db=dy.float().sum(0),
        sres=res.float().sum(0))
    ref["sdx"] = ref["dx"].float().sum(0)
    return x, dy, res, w, mean, rstd, pre, ref


_LN_BWD_CASES = {}


def _ln_bwd_shared(R, H):
    # one reference per shape, shared (read-only) by the parametrised cases
    if (R, H) not in _LN_BWD_CASES:
        _LN_BWD_CASES[(R, H)] = _ln_bwd_case(R, H)
    return _LN_BWD_CASES[(R, H)]


@requires_gpu
@pytest.mark.parametrize("sums", [True, False])
@pytest.mark.parametrize("aliased", [False, True])
@pytest.mark.parametrize("R,H", [(512, 768), (300, 1024), (1000, 512),
                                 (77, 520), (40, 1600)])
def test_ln_bwd_res_sums(R, H, aliased, sums):
    """(300,1024) / (77,520): odd trailing row pair and a partial last
    block; (77,520): a single lane in the second half-row; (40,1600): the
    composed path.  All four fp32 vectors are pre-filled: the entry point
    accumulates.  The 2e-2 bound on sum_dx checks the column sum of dx; it
    is too wide to tell a sum over the bf16-rounded dx from one over the
    unrounded values."""
    ext, check = _ext()
    x, dy, res, w, mean, rstd, pre, ref = _ln_bwd_shared(R, H)
    dw, db, sres, sdx = (p.clone() for p in pre)
    if aliased:
        dx = res.clone()
        resbuf = dx
    else:
        dx = torch.full_like(x, 3.0)
        resbuf = res.clone()
    check(ext.ob_layernorm_bwd_res_bf16(
        ptr(x), ptr(w), ptr(mean), ptr(rstd), ptr(dy), ptr(resbuf), ptr(dx),
        ptr(dw), ptr(db), ptr(sres) if sums else ptr(None),
        ptr(sdx) if sums else ptr(None), R, H, stream()), "lnbwd_res")
    torch.cuda.synchronize()
    assert rel_l2(dx.float(), ref["dx"].float()) < 3e-2
    assert rel_l2(dw - pre[0], ref["dw"]) < 2e-2
    assert rel_l2(db - pre[1], ref["db"]) < 2e-2
    if sums:
        assert rel_l2(sres - pre[2], ref["sres"]) < 2e-2
        assert rel_l2(sdx - pre[3], ref["sdx"]) < 2e-2
    else:
        assert torch.equal(sres, pre[2]) and torch.equal(sdx, pre[3])
    if not aliased:
        assert torch.equal(resbuf.view(torch.int16), res.view(torch.int16))


@requires_gpu
@pytest.mark.parametrize("R,H", [(512, 768), (77, 520)])
def test_ln_bwd_no_residual_and_one_sum(R, H):
    """res null (dx = v) with only sum_dx requested, and the unchanged
    ob_layernorm_bwd_bf16 entry point in both dx_accum modes."""
    ext, check = _ext()
    x, dy, res, w, mean, rstd, pre, ref = _ln_bwd_shared(R, H)
    dw, db, _, sdx = (p.clone() for p in pre)
    dx = torch.full_like(x, 3.0)
    check(ext.ob_layernorm_bwd_res_bf16(
        ptr(x), ptr(w), ptr(mean), ptr(rstd), ptr(dy), ptr(None), ptr(dx),
        ptr(dw), ptr(db), ptr(None), ptr(sdx), R, H, stream()), "lnbwd_nores")
    torch.cuda.synchronize()
    assert rel_l2(dx.float(), ref["v"]) < 3e-2
    assert rel_l2(dw - pre[0], ref["dw"]) < 2e-2
    assert rel_l2(db - pre[1], ref["db"]) < 2e-2
    assert rel_l2(sdx - pre[3], ref["v"].bfloat16().float().sum(0)) < 2e-2
    for accum in (0, 1):
        dw, db = pre[0].clone(), pre[1].clone()
        dx = res.clone()
        check(ext.ob_layernorm_bwd_bf16(
            ptr(x), ptr(w), ptr(mean), ptr(rstd), ptr(dy), ptr(dx), ptr(dw),
            ptr(db), R, H, accum, stream()), "lnbwd")
        torch.cuda.synchronize()
        want = ref["dx"].float() if accum else ref["v"]
        assert rel_l2(dx.float(), want) < 3e-2
        assert rel_l2(dw - pre[0], ref["dw"]) < 2e-2
        assert rel_l2(db - pre[1], ref["db"]) < 2e-2


@requires_gpu
def test_ln_bwd_res_sums_grid_cap():
    """More 32-row chunks (1026) than the 1024-block grid cap: the first
    blocks walk a second chunk before they add their column sums."""
    ext, check = _ext()
    R, H = 32 * 1025 + 9, 512
    x, dy, res, w, mean, rstd, pre, ref = _ln_bwd_case(R, H, seed=9)
    dw, db, sres, sdx = (p.clone() for p in pre)
    dx = torch.empty_like(x)
    check(ext.ob_layernorm_bwd_res_bf16(
        ptr(x), ptr(w), ptr(mean), ptr(rstd), ptr(dy), ptr(res), ptr(dx),
        ptr(dw), ptr(db), ptr(sres), ptr(sdx), R, H, stream()), "lnbwd_cap")
    torch.cuda.synchronize()
    assert rel_l2(dx.float(), ref["dx"].float()) < 3e-2
    assert rel_l2(dw - pre[0], ref["dw"]) < 2e-2
    assert rel_l2(db - pre[1], ref["db"]) < 2e-2
    assert rel_l2(sres - pre[2], ref["sres"]) < 2e-2
    assert rel_l2(sdx - pre[3], ref["sdx"]) < 2e-2


# ---------------------------------------------------------------------------
# gelu backward + column sum
# ---------------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("M,N", [(1000, 3072), (129, 520), (33, 6400),
                                 (64, 40), (16, 36)])
def test_gelu_bwd_colsum(M, N, inplace):
    """(1000,3072): several row tiles with a partial last one; (129,520)
    and (64,40): partial column tiles; (33,6400): one partial row tile;
    (16,36): N not a multiple of 8, the composed path."""
    ext, check = _ext()
    g = torch.Generator().manual_seed(6)
    u = (torch.randn(M, N, generator=g) * 1.5).cuda().bfloat16()
    dg = (torch.randn(M, N, generator=g)).cuda().bfloat16()
    pre = torch.randn(N, generator=g).cuda().float()
    uf = u.float().requires_grad_(True)
    torch.nn.functional.gelu(uf, approximate="tanh").backward(dg.float())
    ref_du = uf.grad.bfloat16()
    db = pre.clone()
    du = dg.clone() if inplace else torch.empty_like(u)
    src = du if inplace else dg
    check(ext.ob_gelu_bwd_colsum_bf16(ptr(u), ptr(src), ptr(du), ptr(db), M,
                                      N, stream()), "gelu_bwd_cs")
    torch.cuda.synchronize()
    assert rel_l2(du.float(), uf.grad) < 3e-2
    assert rel_l2(db - pre, ref_du.float().sum(0)) < 2e-2


# ---------------------------------------------------------------------------
# one block layer through the fused tail
# ---------------------------------------------------------------------------

@requires_gpu
def test_bf16_block_layer_fused_tail():
    """GPT-2-small block (H=768, 12 heads) at B=2, S=128 vs the oracle at
    the bounds of test_bf16_block_layer_parity_flash.  Forward + backward
    run twice into the same grad buffer (grads accumulate: 2x the oracle's),
    and the input buffer is overwritten between forward and backward, so
    the backward can only be right if ln1 really took the stash copy."""
    from oracle.gpt2_oracle import OracleConfig, stage_forward_backward
    from oracle.gpt2_oracle import init_layer_params
    from oobleck_amd.config import ModelConfig
    from oobleck_amd.layer import Layer
    dims = dict(n_embd=768, n_head=12, n_layer=2, n_positions=128,
                vocab_size=304)
    mc, oc = ModelConfig(**dims), OracleConfig(**dims)
    B, S, H = 2, 128, 768
    flat = init_layer_params(oc, 1, 77)
    layer = Layer(1, mc, B, S, 2, torch.device(DEV), dtype="bf16")
    layer.flat_param.copy_(flat.to(DEV))
    layer.refresh_weights()
    layer.zero_grads()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, S, H, generator=g) * 0.5
    dout = torch.randn(B, S, H, generator=g) * 0.1
    x_dev = x.to(DEV).bfloat16()
    dout_dev = dout.to(DEV).bfloat16()
    for _ in range(2):
        xg = x_dev.clone()
        out = torch.empty_like(xg)
        layer.forward_slot(0, xg, out)
        xg.fill_(float("nan"))
        din = torch.empty_like(xg)
        layer.backward_slot(0, dout_dev, din)
    torch.cuda.synchronize()
    ref_out, ref_dx, (ref_grad,) = stage_forward_backward(
        oc, [flat], [1], x, dout=dout)
    assert rel_l2(out.float().cpu(), ref_out) < 5e-2
    assert rel_l2(din.float().cpu(), ref_dx) < 5e-2
    assert rel_l2(layer.flat_grad.cpu(), 2.0 * ref_grad) < 5e-2
    assert torch.equal(dout_dev.cpu(), dout.bfloat16())  # dout is read-only
