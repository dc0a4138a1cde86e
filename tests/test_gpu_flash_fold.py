# @gpu tests for the folded block -> work mapping of the production flash
# kernels (oobleck_amd/csrc/ob_flash_fold.h): a block owns a light and a
# heavy piece of the causal triangle, the blocks of one head get linear ids
# of one XCD, and the dq kernel can form D itself
# (ob_flash_bwd_nt_d_bf16).  None of that changes a wave's arithmetic, so
# O, lse, D and dqkv are compared bit for bit with the transposed-operand
# twins, whose mapping is the plain one.  Outputs are pre-filled with NaN:
# a row no block owns stays NaN and fails the comparison.
import functools
import math

import pytest
import torch

from tests.gpu_helpers import ptr, stream

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
DEV = "cuda:0"
SCALE = 1.0 / math.sqrt(64.0)
# (2,2,128): one block, the fold is the identity; (1,3,256): smallest S
# where the fold differs, Z = 3 pads the grid; (2,2,384): odd number of
# 128-row blocks, the middle block's halves are adjacent; (2,4,256): Z = 8,
# no padding; (1,1,1024): the step's tile counts, a dkdv pair idle for up
# to 31 iterations across both LDS buffers
SHAPES = [(2, 2, 128), (1, 3, 256), (2, 2, 384), (2, 4, 256), (1, 1, 1024)]


def rel_l2(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _ext():
    from oobleck_amd._ext import get_ext
    return get_ext()


def _check(rc, what):
    from oobleck_amd._ext import check
    check(rc, what)


@functools.lru_cache(maxsize=None)
def _case(B, nh, S):
    """Inputs, the twins' outputs (transposes + plain-mapped kernels) and
    the fp32 autograd dqkv; computed once per shape, never modified."""
    ext = _ext()
    H = nh * 64
    g = torch.Generator().manual_seed(47)
    qkv = (torch.randn(B, S, 3 * H, generator=g) * 0.5).to(DEV).bfloat16()
    dO = (torch.randn(B, S, H, generator=g) * 0.3).to(DEV).bfloat16()

    def tr(src_off, src, ld, sb):
        out = torch.empty(B * nh, 64, S, device=DEV, dtype=torch.bfloat16)
        _check(ext.ob_transpose_bf16_b(
            ptr(src.flatten()[src_off:]), ptr(out), S, 64, sb, 64, ld, B, nh,
            stream()), "transpose")
        return out

    QT = tr(0, qkv, 3 * H, S * 3 * H)
    KT = tr(H, qkv, 3 * H, S * 3 * H)
    VT = tr(2 * H, qkv, 3 * H, S * 3 * H)
    dOT = tr(0, dO, H, S * H)
    O = torch.empty(B, S, H, device=DEV, dtype=torch.bfloat16)
    lse = torch.empty(B * nh, S, device=DEV, dtype=torch.float32)
    _check(ext.ob_flash_fwd_bf16(ptr(qkv), ptr(VT), ptr(O), ptr(lse), B, S,
                                 H, nh, SCALE, stream()), "flash_fwd")
    D = torch.empty(B * nh, S, device=DEV, dtype=torch.float32)
    _check(ext.ob_flash_dsum_bf16(ptr(O), ptr(dO), ptr(D), B, S, H, nh,
                                  stream()), "dsum")
    dqkv = torch.empty_like(qkv)
    _check(ext.ob_flash_bwd_bf16(ptr(qkv), ptr(QT), ptr(KT), ptr(dOT),
                                 ptr(dO), ptr(lse), ptr(D), ptr(dqkv), B, S,
                                 H, nh, SCALE, stream()), "flash_bwd")
    torch.cuda.synchronize()
    assert not torch.isnan(O.float()).any()
    assert not torch.isnan(dqkv.float()).any()

    qf = qkv.float().requires_grad_(True)
    q = qf[..., :H].view(B, S, nh, 64).permute(0, 2, 1, 3)
    k = qf[..., H:2 * H].view(B, S, nh, 64).permute(0, 2, 1, 3)
    v = qf[..., 2 * H:].view(B, S, nh, 64).permute(0, 2, 1, 3)
    w = torch.matmul(q, k.transpose(-1, -2)) * SCALE
    mask = torch.tril(torch.ones(S, S, dtype=torch.bool, device=DEV))
    w = torch.where(mask, w, torch.tensor(float("-inf"), device=DEV))
    P = torch.softmax(w, dim=-1)
    O_ref = torch.matmul(P, v).permute(0, 2, 1, 3).reshape(B, S, H)
    O_ref.backward(dO.float())
    return dict(H=H, qkv=qkv, dO=dO, O=O, lse=lse, D=D, dqkv=dqkv,
                dqkv_ref=qf.grad)


def _nan_like(t):
    return torch.full_like(t, float("nan"))


def _bwd(c, B, nh, S, dbias, form_d):
    """-> (dqkv, D_ws or None) of the production backward, outputs
    pre-filled with NaN"""
    dqkv = _nan_like(c["qkv"])
    if form_d:
        D_ws = _nan_like(c["D"])
        _check(_ext().ob_flash_bwd_nt_d_bf16(
            ptr(c["qkv"]), ptr(c["O"]), ptr(c["dO"]), ptr(c["lse"]),
            ptr(D_ws), ptr(dqkv), ptr(dbias), B, S, c["H"], nh, SCALE,
            stream()), "flash_bwd_nt_d")
    else:
        D_ws = None
        _check(_ext().ob_flash_bwd_nt_bf16(
            ptr(c["qkv"]), ptr(c["dO"]), ptr(c["lse"]), ptr(c["D"]),
            ptr(dqkv), ptr(dbias), B, S, c["H"], nh, SCALE, stream()),
            "flash_bwd_nt")
    torch.cuda.synchronize()
    return dqkv, D_ws


@requires_gpu
@pytest.mark.parametrize("B,nh,S", SHAPES)
def test_fold_fwd(B, nh, S):
    c = _case(B, nh, S)
    O = _nan_like(c["O"])
    lse = _nan_like(c["lse"])
    _check(_ext().ob_flash_fwd_nt_bf16(ptr(c["qkv"]), ptr(O), ptr(lse), B, S,
                                       c["H"], nh, SCALE, stream()),
           "flash_fwd_nt")
    torch.cuda.synchronize()
    assert torch.equal(O, c["O"])
    assert torch.equal(lse, c["lse"])


@requires_gpu
@pytest.mark.parametrize("B,nh,S", SHAPES)
def test_fold_bwd(B, nh, S):
    c = _case(B, nh, S)
    dqkv, _ = _bwd(c, B, nh, S, None, form_d=False)
    assert torch.equal(dqkv, c["dqkv"])


@requires_gpu
@pytest.mark.parametrize("B,nh,S", SHAPES)
def test_fold_bwd_d_in_kernel(B, nh, S):
    c = _case(B, nh, S)
    dqkv, D_ws = _bwd(c, B, nh, S, None, form_d=True)
    assert torch.equal(D_ws, c["D"])
    assert torch.equal(dqkv, c["dqkv"])


@requires_gpu
@pytest.mark.parametrize("form_d", [False, True])
@pytest.mark.parametrize("B,nh,S", SHAPES)
def test_fold_bwd_bias(B, nh, S, form_d):
    """dbias_qkv accumulates, from a known non-zero start, the column sums
    of the fp32 accumulators; a block covered twice would double a column
    against ob_colsum_bf16(dqkv)."""
    c = _case(B, nh, S)
    H = c["H"]
    start = torch.linspace(-1.0, 1.0, 3 * H, device=DEV)
    acc = start.clone()
    dqkv, _ = _bwd(c, B, nh, S, acc, form_d)
    assert torch.equal(dqkv, c["dqkv"])
    added = acc - start
    ref = c["dqkv_ref"].reshape(B * S, 3 * H).sum(0)
    cs = torch.zeros(3 * H, device=DEV)
    _check(_ext().ob_colsum_bf16(ptr(dqkv), ptr(cs), B * S, 3 * H, stream()),
           "colsum")
    torch.cuda.synchronize()
    e_ref, e_cs = rel_l2(added, ref), rel_l2(added, cs)
    print(f"fold bwd bias ({B},{nh},{S}) form_d={form_d}: rel-L2 vs fp32 "
          f"autograd {e_ref:.3e}, vs ob_colsum_bf16(dqkv) {e_cs:.3e}")
    assert e_ref < 3e-2, e_ref
    assert e_cs < 3e-2, e_cs
