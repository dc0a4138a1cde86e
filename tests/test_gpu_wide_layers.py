# @gpu tests past the two width walls of the head_dim 64 / n_embd <= 2048
# code: LayerNorm backward beyond 2048 columns (the block-per-row kernels'
# columns-per-thread count, ob_kernels.hip / ob_kernels_bf16.hip) and whole
# layers whose attention has head_dim 128 (ob_flash_hd128_bf16.hip behind
# the layer's flash route, ob_layer.hip).
import os
import pathlib
import subprocess
import sys

import pytest
import torch

from tests import gpu_helpers as gh
from tests.gpu_helpers import ptr, stream

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
DEV = "cuda:0"
# (64, 2176): the first width past the old wall, 16 columns per thread with
# a partly filled ninth column slot; (40, 4096): 16 exactly full; (33,
# 12288): 48, the new limit, and a partial last row chunk
LN_SHAPES = [(64, 2176), (40, 4096), (33, 12288)]


def rel_l2(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _ext():
    from oobleck_amd._ext import check, get_ext
    return get_ext(), check


_LN_CASES = {}


def _ln_case(R, H):
    """bf16 inputs and the torch fp32 reference on them (eps = 0, as
    test_ln_bwd_bf16_wave); one per shape, shared read-only."""
    if (R, H) in _LN_CASES:
        return _LN_CASES[(R, H)]
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(R, H, generator=g)).cuda().bfloat16()
    dy = (torch.randn(R, H, generator=g) * 0.5).cuda().bfloat16()
    res = (torch.randn(R, H, generator=g) * 0.5).cuda().bfloat16()
    w = torch.randn(H, generator=g).cuda().float()
    b = torch.randn(H, generator=g).cuda().float()
    pre = [torch.randn(H, generator=g).cuda().float() for _ in range(4)]
    xf = x.float().requires_grad_(True)
    mu = xf.mean(-1, keepdim=True)
    var = xf.var(-1, unbiased=False, keepdim=True)
    y = (xf - mu) / torch.sqrt(var + 0.0) * w + b
    y.backward(dy.float())
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
    _LN_CASES[(R, H)] = (x, dy, res, w, mean, rstd, pre, ref)
    return _LN_CASES[(R, H)]


@requires_gpu
@pytest.mark.parametrize("dx_accum", [0, 1])
@pytest.mark.parametrize("R,H", LN_SHAPES)
def test_ln_bwd_bf16_wide(R, H, dx_accum):
    ext, check = _ext()
    x, dy, res, w, mean, rstd, pre, ref = _ln_case(R, H)
    dx = res.clone() if dx_accum else torch.full_like(x, float("nan"))
    dw, db = pre[0].clone(), pre[1].clone()
    check(ext.ob_layernorm_bwd_bf16(
        ptr(x), ptr(w), ptr(mean), ptr(rstd), ptr(dy), ptr(dx), ptr(dw),
        ptr(db), R, H, dx_accum, stream()), "lnbwd")
    torch.cuda.synchronize()
    want = ref["dx"].float() if dx_accum else ref["v"]
    e = (rel_l2(dx.float(), want), rel_l2(dw - pre[0], ref["dw"]),
         rel_l2(db - pre[1], ref["db"]))
    print(f"ln bwd bf16 ({R},{H}) accum={dx_accum}: dx {e[0]:.3e} "
          f"dw {e[1]:.3e} db {e[2]:.3e}")
    assert not torch.isnan(dx.float()).any()
    assert e[0] < 3e-2 and e[1] < 2e-2 and e[2] < 2e-2, e


@requires_gpu
@pytest.mark.parametrize("R,H", LN_SHAPES)
def test_ln_bwd_res_bf16_wide(R, H):
    """The fused-tail entry with both side sums (its composed path at these
    widths); all four fp32 vectors are pre-filled: the entry accumulates."""
    ext, check = _ext()
    x, dy, res, w, mean, rstd, pre, ref = _ln_case(R, H)
    dw, db, sres, sdx = (p.clone() for p in pre)
    dx = torch.full_like(x, float("nan"))
    resbuf = res.clone()
    check(ext.ob_layernorm_bwd_res_bf16(
        ptr(x), ptr(w), ptr(mean), ptr(rstd), ptr(dy), ptr(resbuf), ptr(dx),
        ptr(dw), ptr(db), ptr(sres), ptr(sdx), R, H, stream()), "lnbwd_res")
    torch.cuda.synchronize()
    e = (rel_l2(dx.float(), ref["dx"].float()),
         rel_l2(dw - pre[0], ref["dw"]), rel_l2(db - pre[1], ref["db"]),
         rel_l2(sres - pre[2], ref["sres"]), rel_l2(sdx - pre[3], ref["sdx"]))
    print(f"ln bwd res bf16 ({R},{H}): dx {e[0]:.3e} dw {e[1]:.3e} "
          f"db {e[2]:.3e} sum_res {e[3]:.3e} sum_dx {e[4]:.3e}")
    assert not torch.isnan(dx.float()).any()
    assert e[0] < 3e-2
    assert all(v < 2e-2 for v in e[1:]), e
    assert torch.equal(resbuf.view(torch.int16), res.view(torch.int16))


@requires_gpu
@pytest.mark.parametrize("R,H", LN_SHAPES)
def test_ln_bwd_f32_wide(R, H):
    """fp32 entry, with the bounds of test_gpu_kernels.py's
    test_layernorm_fwd_bwd, accumulate flag included."""
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(R, H, generator=g) * 2.0).to(DEV)
    w = torch.randn(H, generator=g).to(DEV) + 1.0
    b = torch.randn(H, generator=g).to(DEV)
    dy = torch.randn(R, H, generator=g).to(DEV)
    y, mean, rstd = gh.layernorm_fwd(x, w, b)
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(xr, (H,), wr, br, eps=1e-5)
    torch.cuda.synchronize()
    torch.testing.assert_close(y, yr, rtol=1e-5, atol=1e-5)
    yr.backward(dy)
    dx = torch.full_like(x, float("nan"))
    dw = torch.zeros(H, device=DEV)
    db = torch.zeros(H, device=DEV)
    gh.layernorm_bwd(x, w, mean, rstd, dy, dx, dw, db)
    torch.cuda.synchronize()
    torch.testing.assert_close(dx, xr.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(dw, wr.grad, rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(db, br.grad, rtol=1e-4, atol=1e-3)
    dx2 = torch.ones_like(x)
    gh.layernorm_bwd(x, w, mean, rstd, dy, dx2, dw, db, dx_accum=1)
    torch.cuda.synchronize()
    torch.testing.assert_close(dx2, xr.grad + 1.0, rtol=1e-4, atol=1e-5)


@requires_gpu
def test_ln_bwd_refuses_past_12288():
    ext, check = _ext()
    R, H = 2, 12296
    x = torch.zeros(R, H, device=DEV, dtype=torch.bfloat16)
    xf = torch.zeros(R, H, device=DEV)
    w = torch.ones(H, device=DEV)
    mean = torch.zeros(R, device=DEV)
    rstd = torch.ones(R, device=DEV)
    dw = torch.zeros(H, device=DEV)
    db = torch.zeros(H, device=DEV)
    dx = torch.zeros_like(x)
    rc = ext.ob_layernorm_bwd_bf16(ptr(x), ptr(w), ptr(mean), ptr(rstd),
                                   ptr(x), ptr(dx), ptr(dw), ptr(db), R, H, 0,
                                   stream())
    assert rc != 0 and b"12288" in ext.ob_last_error()
    rc = ext.ob_layernorm_bwd_res_bf16(
        ptr(x), ptr(w), ptr(mean), ptr(rstd), ptr(x), ptr(None), ptr(dx),
        ptr(dw), ptr(db), ptr(None), ptr(None), R, H, stream())
    assert rc != 0 and b"12288" in ext.ob_last_error()
    dxf = torch.zeros_like(xf)
    rc = ext.ob_layernorm_bwd_f32(ptr(xf), ptr(w), ptr(mean), ptr(rstd),
                                  ptr(xf), ptr(dxf), ptr(dw), ptr(db), R, H,
                                  0, stream())
    assert rc != 0 and b"12288" in ext.ob_last_error()
    torch.cuda.synchronize()


@requires_gpu
def test_wide_block_layer_parity_hd128():
    """One BLOCK layer at n_embd = 2176, 17 heads: the smallest width past
    the old LayerNorm wall with head_dim 128, and 17 heads pad the flash
    grid.  Bounds of test_bf16_block_layer_parity_flash."""
    from oracle.gpt2_oracle import OracleConfig, stage_forward_backward
    from oracle.gpt2_oracle import init_layer_params
    from oobleck_amd.config import ModelConfig
    from oobleck_amd.layer import Layer
    H = 2176
    dims = dict(n_embd=H, n_head=17, n_layer=2, n_positions=128,
                vocab_size=304)
    mc, oc = ModelConfig(**dims), OracleConfig(**dims)
    B, S = 1, 128
    flat = init_layer_params(oc, 1, 77)
    layer = Layer(1, mc, B, S, 2, torch.device(DEV), dtype="bf16")
    assert layer.uses_flash
    layer.flat_param.copy_(flat.to(DEV))
    layer.refresh_weights()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, S, H, generator=g) * 0.5
    dout = torch.randn(B, S, H, generator=g) * 0.1
    xg = x.to(DEV).bfloat16()
    out = torch.empty_like(xg)
    layer.forward_slot(0, xg, out)
    din = torch.empty_like(xg)
    layer.backward_slot(0, dout.to(DEV).bfloat16(), din)
    torch.cuda.synchronize()
    ref_out, ref_dx, (ref_grad,) = stage_forward_backward(
        oc, [flat], [1], x, dout=dout)
    e = (rel_l2(out.float().cpu(), ref_out), rel_l2(din.float().cpu(), ref_dx),
         rel_l2(layer.flat_grad.cpu(), ref_grad))
    print(f"wide block H=2176 nh=17: out {e[0]:.3e} din {e[1]:.3e} "
          f"grad {e[2]:.3e}")
    assert e[0] < 5e-2 and e[1] < 5e-2 and e[2] < 5e-2, e


@requires_gpu
def test_bf16_per_layer_parity_hd128():
    """test_bf16_per_layer_parity's chain (EMBED -> 2 BLOCKs -> FINAL, each
    layer against the oracle on its own inputs, 1.5e-2 fwd / 3e-2 grads) at
    n_embd = 256, n_head = 2: head_dim 128."""
    from oracle.gpt2_oracle import OracleConfig, stage_forward_backward
    from oracle.gpt2_oracle import init_layer_params
    from oobleck_amd.config import ModelConfig
    from oobleck_amd.layer import Layer
    from oobleck_amd.params import KIND_BLOCK
    dims = dict(n_embd=256, n_head=2, n_layer=2, n_positions=128,
                vocab_size=304)
    mc, oc = ModelConfig(**dims), OracleConfig(**dims)
    B, S, H = 2, 128, dims["n_embd"]
    L = oc.n_layers_total
    flats = [init_layer_params(oc, oc.layer_kind(i), 600 + i)
             for i in range(L)]
    layers = []
    for lid in range(L):
        layer = Layer(lid, mc, B, S, 1, torch.device(DEV), dtype="bf16")
        layer.flat_param.copy_(flats[lid].to(DEV))
        layer.refresh_weights()
        layers.append(layer)
        assert layer.uses_flash == (layer.kind == KIND_BLOCK), lid
    g = torch.Generator().manual_seed(19)
    ids = torch.randint(0, oc.vocab_size, (B, S), generator=g)

    x = ids.to(DEV)
    fwd_inputs = []
    for lid, layer in enumerate(layers):
        xin = x.float().cpu() if x.is_floating_point() else x.cpu()
        fwd_inputs.append(xin)
        if lid == L - 1:
            out = torch.zeros(1, device=DEV)
            layer.forward_slot(0, x, out, ids.to(DEV))
        else:
            out = torch.empty(B, S, H, device=DEV, dtype=torch.bfloat16)
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
                oc, [flats[lid]], [lid], xin, dout=torch.zeros(B, S, H))
            e = rel_l2(out.float().cpu(), ref_out)
            print(f"per-layer hd128 fwd layer {lid}: {e:.3e}")
            assert e < 1.5e-2, lid
        x = out

    dout = None
    for lid in range(L - 1, -1, -1):
        layer = layers[lid]
        din = None if lid == 0 else torch.empty(B, S, H, device=DEV,
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
        e = rel_l2(layer.flat_grad.cpu(), ref_grad)
        print(f"per-layer hd128 bwd layer {lid}: grad {e:.3e}")
        assert e < 3e-2, lid
        if din is not None and ref_dx is not None:
            assert rel_l2(din.float().cpu(), ref_dx) < 3e-2, lid
        dout = din


def _run_layer_child(tmp_path, flag):
    out = tmp_path / f"hd128_{flag}.pt"
    env = dict(os.environ, OB_LT_TUNE="0")
    env.pop("OB_FLASH_HD128", None)
    if flag is not None:
        env["OB_FLASH_HD128"] = flag
    child = pathlib.Path(__file__).resolve().parent / \
        "flash_hd128_layer_child.py"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + \
          [str(child), str(out)]
    subprocess.run(cmd, check=True, env=env, timeout=300)
    return torch.load(out)


@requires_gpu
def test_hd128_layer_ab(tmp_path):
    """One BLOCK layer with head_dim 128 (H = 256) in fresh processes with
    OB_FLASH_HD128=0 and with the default (the switch is read once per
    process), both with OB_LT_TUNE=0 so the library GEMMs cannot differ:
    the materialized route / the flash route, each within the 5e-2 bounds
    of the oracle.  The distance between the arms is printed, not bounded."""
    from oracle.gpt2_oracle import OracleConfig, stage_forward_backward
    from oracle.gpt2_oracle import init_layer_params
    H, B, S = 256, 2, 128
    oc = OracleConfig(n_embd=H, n_head=2, n_layer=2, n_positions=128,
                      vocab_size=304)
    flat = init_layer_params(oc, 1, 77)
    g = torch.Generator().manual_seed(8)
    # the child rounds its inputs to bf16; give the oracle the same values
    x = (torch.randn(B, S, H, generator=g) * 0.5).bfloat16().float()
    dout = (torch.randn(B, S, H, generator=g) * 0.1).bfloat16().float()
    ref_out, ref_dx, (ref_grad,) = stage_forward_backward(
        oc, [flat], [1], x, dout=dout)
    arms = {}
    for name, flag, want in (("materialized", "0", False),
                             ("flash", None, True)):
        r = _run_layer_child(tmp_path, flag)
        assert r["uses_flash"] is want, name
        e = (rel_l2(r["out"].float(), ref_out),
             rel_l2(r["din"].float(), ref_dx), rel_l2(r["grad"], ref_grad))
        print(f"hd128 layer {name}: out {e[0]:.3e} din {e[1]:.3e} "
              f"grad {e[2]:.3e}")
        assert e[0] < 5e-2 and e[1] < 5e-2 and e[2] < 5e-2, (name, e)
        arms[name] = r
    a, b = arms["flash"], arms["materialized"]
    print("hd128 layer flash vs materialized: out "
          f"{rel_l2(a['out'].float(), b['out'].float()):.3e} din "
          f"{rel_l2(a['din'].float(), b['din'].float()):.3e} grad "
          f"{rel_l2(a['grad'], b['grad']):.3e}")
