# @gpu tests for the head_dim 128 flash kernels
# (oobleck_amd/csrc/ob_flash_hd128_bf16.hip) behind the production entries
# ob_flash_fwd_nt_bf16 / ob_flash_bwd_nt_bf16 / ob_flash_bwd_nt_d_bf16, which
# dispatch on H / nh.  There are no transposed-operand twins at 128: the
# reference is fp32 torch causal attention and autograd on the same
# bf16-rounded inputs, with the bounds the project uses for the hd-64
# kernels (tests/test_gpu_bf16.py) — the new kernels add no rounding step,
# only longer fp32 sums.  Outputs are pre-filled with NaN: a row or column
# no block owns stays NaN and fails.
import functools
import math

import pytest
import torch

from tests.gpu_helpers import ptr, stream

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
DEV = "cuda:0"
HD = 128
SCALE = 1.0 / math.sqrt(float(HD))
# (2,2,128): one block, the fold is the identity; (1,3,256): the fold
# differs, Z = 3 pads the grid; (2,2,384): an odd block count; (2,4,256):
# Z = 8; (1,1,1024): the long loops over both LDS buffers, a dkdv pair idle
# for 31 iterations
SHAPES = [(2, 2, 128), (1, 3, 256), (2, 2, 384), (2, 4, 256), (1, 1, 1024)]


def rel_l2(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _ext():
    from oobleck_amd._ext import get_ext
    return get_ext()


def _check(rc, what):
    from oobleck_amd._ext import check
    check(rc, what)


def _nan_like(t):
    return torch.full_like(t, float("nan"))


def _inputs(B, nh, S, hd, seed=47):
    H = nh * hd
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B, S, 3 * H, generator=g) * 0.5).to(DEV).bfloat16()
    dO = (torch.randn(B, S, H, generator=g) * 0.3).to(DEV).bfloat16()
    return H, qkv, dO


@functools.lru_cache(maxsize=None)
def _case(B, nh, S):
    """Inputs, the fp32 torch reference (O, lse, dqkv) and the kernels'
    forward outputs; computed once per shape, never modified."""
    H, qkv, dO = _inputs(B, nh, S, HD)
    qf = qkv.float().requires_grad_(True)
    q = qf[..., :H].view(B, S, nh, HD).permute(0, 2, 1, 3)
    k = qf[..., H:2 * H].view(B, S, nh, HD).permute(0, 2, 1, 3)
    v = qf[..., 2 * H:].view(B, S, nh, HD).permute(0, 2, 1, 3)
    w = torch.matmul(q, k.transpose(-1, -2)) * SCALE
    mask = torch.tril(torch.ones(S, S, dtype=torch.bool, device=DEV))
    w = torch.where(mask, w, torch.tensor(float("-inf"), device=DEV))
    lse_ref = torch.logsumexp(w, dim=-1).detach().reshape(B * nh, S)
    P = torch.softmax(w, dim=-1)
    O_ref = torch.matmul(P, v).permute(0, 2, 1, 3).reshape(B, S, H)
    O_ref.backward(dO.float())

    O = _nan_like(dO)
    lse = torch.full((B * nh, S), float("nan"), device=DEV)
    _check(_ext().ob_flash_fwd_nt_bf16(ptr(qkv), ptr(O), ptr(lse), B, S, H,
                                       nh, SCALE, stream()), "flash_fwd_nt")
    torch.cuda.synchronize()
    # D of the kernels' own O, as the backward defines it
    D_ref = (O.float() * dO.float()).view(B, S, nh, HD).sum(-1) \
        .permute(0, 2, 1).reshape(B * nh, S).contiguous()
    return dict(H=H, qkv=qkv, dO=dO, O=O, lse=lse, O_ref=O_ref.detach(),
                lse_ref=lse_ref, D_ref=D_ref, dqkv_ref=qf.grad)


def _bwd(c, B, nh, S, dbias, form_d):
    """-> (dqkv, D_ws or None), outputs pre-filled with NaN"""
    dqkv = _nan_like(c["qkv"])
    if form_d:
        D_ws = _nan_like(c["D_ref"])
        _check(_ext().ob_flash_bwd_nt_d_bf16(
            ptr(c["qkv"]), ptr(c["O"]), ptr(c["dO"]), ptr(c["lse"]),
            ptr(D_ws), ptr(dqkv), ptr(dbias), B, S, c["H"], nh, SCALE,
            stream()), "flash_bwd_nt_d")
    else:
        D_ws = None
        D = _nan_like(c["D_ref"])
        _check(_ext().ob_flash_dsum_bf16(ptr(c["O"]), ptr(c["dO"]), ptr(D), B,
                                         S, c["H"], nh, stream()), "dsum")
        torch.cuda.synchronize()
        torch.testing.assert_close(D, c["D_ref"], rtol=1e-2, atol=1e-2)
        _check(_ext().ob_flash_bwd_nt_bf16(
            ptr(c["qkv"]), ptr(c["dO"]), ptr(c["lse"]), ptr(D), ptr(dqkv),
            ptr(dbias), B, S, c["H"], nh, SCALE, stream()), "flash_bwd_nt")
    torch.cuda.synchronize()
    return dqkv, D_ws


def _check_dqkv(c, dqkv, tag):
    H = c["H"]
    assert not torch.isnan(dqkv.float()).any(), tag
    for name, sl in (("dQ", slice(0, H)), ("dK", slice(H, 2 * H)),
                     ("dV", slice(2 * H, 3 * H))):
        e = rel_l2(dqkv[..., sl].float(), c["dqkv_ref"][..., sl])
        print(f"hd128 {tag} {name}: rel-L2 {e:.3e}")
        assert e < 3e-2, (name, e)


@requires_gpu
@pytest.mark.parametrize("B,nh,S", SHAPES)
def test_hd128_fwd(B, nh, S):
    c = _case(B, nh, S)
    assert not torch.isnan(c["O"].float()).any()
    assert not torch.isnan(c["lse"]).any()
    e = rel_l2(c["O"].float(), c["O_ref"])
    print(f"hd128 fwd ({B},{nh},{S}): O rel-L2 {e:.3e}, lse max abs err "
          f"{(c['lse'] - c['lse_ref']).abs().max().item():.3e}")
    assert e < 2e-2, e
    torch.testing.assert_close(c["lse"], c["lse_ref"], rtol=1e-3, atol=1e-3)


@requires_gpu
@pytest.mark.parametrize("form_d", [False, True])
@pytest.mark.parametrize("B,nh,S", SHAPES)
def test_hd128_bwd(B, nh, S, form_d):
    """Both backward entries: D given (from ob_flash_dsum_bf16, checked) and
    D formed by the dq kernel."""
    c = _case(B, nh, S)
    dqkv, D_ws = _bwd(c, B, nh, S, None, form_d)
    if form_d:
        assert not torch.isnan(D_ws).any()
        print(f"hd128 D ({B},{nh},{S}): max abs err "
              f"{(D_ws - c['D_ref']).abs().max().item():.3e}")
        torch.testing.assert_close(D_ws, c["D_ref"], rtol=1e-2, atol=1e-2)
    _check_dqkv(c, dqkv, f"bwd ({B},{nh},{S}) form_d={form_d}")


@requires_gpu
@pytest.mark.parametrize("form_d", [False, True])
@pytest.mark.parametrize("B,nh,S", SHAPES)
def test_hd128_bwd_bias(B, nh, S, form_d):
    """dbias_qkv accumulates, from a known non-zero start, the column sums
    of the fp32 accumulators; a block covered twice would double a column
    against ob_colsum_bf16(dqkv)."""
    c = _case(B, nh, S)
    H = c["H"]
    start = torch.linspace(-1.0, 1.0, 3 * H, device=DEV)
    acc = start.clone()
    dqkv, _ = _bwd(c, B, nh, S, acc, form_d)
    _check_dqkv(c, dqkv, f"bwd+bias ({B},{nh},{S}) form_d={form_d}")
    added = acc - start
    assert not torch.isnan(added).any()
    ref = c["dqkv_ref"].reshape(B * S, 3 * H).sum(0)
    cs = torch.zeros(3 * H, device=DEV)
    _check(_ext().ob_colsum_bf16(ptr(dqkv), ptr(cs), B * S, 3 * H, stream()),
           "colsum")
    torch.cuda.synchronize()
    e_ref, e_cs = rel_l2(added, ref), rel_l2(added, cs)
    print(f"hd128 bwd bias ({B},{nh},{S}) form_d={form_d}: rel-L2 vs fp32 "
          f"autograd {e_ref:.3e}, vs ob_colsum_bf16(dqkv) {e_cs:.3e}")
    assert e_ref < 3e-2, e_ref
    assert e_cs < 3e-2, e_cs


@requires_gpu
def test_hd64_dispatch_unchanged():
    """Dispatch sanity check, not a yardstick: head_dim 64 through the same
    entries gives the same bits in two identical calls (and no NaN)."""
    B, nh, S = 1, 3, 256
    H, qkv, dO = _inputs(B, nh, S, 64)
    scale = 1.0 / math.sqrt(64.0)
    runs = []
    for _ in range(2):
        O = _nan_like(dO)
        lse = torch.full((B * nh, S), float("nan"), device=DEV)
        _check(_ext().ob_flash_fwd_nt_bf16(ptr(qkv), ptr(O), ptr(lse), B, S,
                                           H, nh, scale, stream()), "fwd64")
        D_ws = _nan_like(lse)
        dqkv = _nan_like(qkv)
        _check(_ext().ob_flash_bwd_nt_d_bf16(
            ptr(qkv), ptr(O), ptr(dO), ptr(lse), ptr(D_ws), ptr(dqkv),
            ptr(None), B, S, H, nh, scale, stream()), "bwd64")
        torch.cuda.synchronize()
        runs.append((O, lse, D_ws, dqkv))
    for a, b in zip(*runs):
        assert not torch.isnan(a.float()).any()
        assert torch.equal(a, b)


@requires_gpu
def test_hd128_dropout_entries_refuse():
    """Attention dropout at head_dim 128 is out of scope: the dropout
    entries fail, naming head_dim, and launch nothing."""
    B, nh, S = 1, 1, 128
    H, qkv, dO = _inputs(B, nh, S, HD)
    O = _nan_like(dO)
    lse = torch.full((B * nh, S), float("nan"), device=DEV)
    ext = _ext()
    rc = ext.ob_flash_fwd_nt_drop_bf16(ptr(qkv), ptr(O), ptr(lse), B, S, H,
                                       nh, SCALE, 1, 0, 0, 0.1, stream())
    assert rc != 0
    assert b"head_dim" in ext.ob_last_error()
    dqkv = _nan_like(qkv)
    D_ws = _nan_like(lse)
    rc = ext.ob_flash_bwd_nt_d_drop_bf16(
        ptr(qkv), ptr(O), ptr(dO), ptr(lse), ptr(D_ws), ptr(dqkv), ptr(None),
        B, S, H, nh, SCALE, 1, 0, 0, 0.1, stream())
    assert rc != 0
    assert b"head_dim" in ext.ob_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(O.float()).all() and torch.isnan(dqkv.float()).all()
