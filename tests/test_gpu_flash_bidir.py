# @gpu tests for the bidirectional flash kernels (ob_flash_bidir_bf16.hip)
# against fp32 torch attention without a mask and autograd on the same
# bf16-rounded inputs, with the project's bounds for the dense kernels
# (tests/test_gpu_flash_window.py): no rounding step is added.  Outputs are
# pre-filled with NaN: a row or column no block owns stays NaN and fails.
import functools
import math

import pytest
import torch

from tests.gpu_helpers import ptr, stream

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
DEV = "cuda:0"
HD = 64
# (1,1,128): one forward/dq block and two dkdv blocks, the smallest launch;
# (2,2,256): batch and head offsets, two blocks; (1,3,384): an odd block
# count, Z = 3 pads the grid; (1,1,1024): many trips over both LDS buffers
CASES = [(1, 1, 128), (2, 2, 256), (1, 3, 384), (1, 1, 1024)]


def rel_l2(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _run(B, nh, S, qkv, dO, dbias=None, H=None):
    """The two entries -> their rcs and O, lse, D_ws, dqkv (NaN pre-filled)"""
    from oobleck_amd._ext import get_ext
    H, scale = H or nh * HD, 1.0 / math.sqrt(HD)
    O = torch.full_like(dO, float("nan"))
    lse = torch.full((B * nh, S), float("nan"), device=DEV)
    rc_f = get_ext().ob_flash_fwd_bidir_bf16(ptr(qkv), ptr(O), ptr(lse), B, S,
                                             H, nh, scale, stream())
    D_ws = torch.full_like(lse, float("nan"))
    dqkv = torch.full_like(qkv, float("nan"))
    rc_b = get_ext().ob_flash_bwd_bidir_d_bf16(
        ptr(qkv), ptr(O), ptr(dO), ptr(lse), ptr(D_ws), ptr(dqkv), ptr(dbias),
        B, S, H, nh, scale, stream())
    torch.cuda.synchronize()
    return (rc_f, rc_b), (O, lse, D_ws, dqkv)


@functools.lru_cache(maxsize=None)
def _case(B, nh, S):
    """Inputs, fp32 reference and kernel outputs; computed once, read-only."""
    H = nh * HD
    g = torch.Generator().manual_seed(53)
    qkv = (torch.randn(B, S, 3 * H, generator=g) * 0.5).to(DEV).bfloat16()
    dO = (torch.randn(B, S, H, generator=g) * 0.3).to(DEV).bfloat16()
    qf = qkv.float().requires_grad_(True)
    q, k, v = (qf[..., i * H:(i + 1) * H].view(B, S, nh, HD)
               .permute(0, 2, 1, 3) for i in range(3))
    w = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(HD)
    lse_ref = torch.logsumexp(w, dim=-1).detach().reshape(B * nh, S)
    O_ref = torch.matmul(torch.softmax(w, dim=-1), v).permute(0, 2, 1, 3) \
        .reshape(B, S, H)
    O_ref.backward(dO.float())
    dbias = torch.zeros(3 * H, device=DEV)
    rcs, (O, lse, D_ws, dqkv) = _run(B, nh, S, qkv, dO, dbias)
    assert rcs == (0, 0), rcs
    return dict(H=H, qkv=qkv, dO=dO, O=O, lse=lse, D_ws=D_ws, dqkv=dqkv,
                dbias=dbias, O_ref=O_ref.detach(), lse_ref=lse_ref,
                dqkv_ref=qf.grad)


@requires_gpu
@pytest.mark.parametrize("B,nh,S", CASES)
def test_bidir_fwd(B, nh, S):
    c = _case(B, nh, S)
    assert not torch.isnan(c["O"].float()).any()
    assert not torch.isnan(c["lse"]).any()
    e = rel_l2(c["O"].float(), c["O_ref"])
    print(f"bidir fwd ({B},{nh},{S}): O rel-L2 {e:.3e}, lse max abs err "
          f"{(c['lse'] - c['lse_ref']).abs().max().item():.3e}")
    assert e < 2e-2, e
    torch.testing.assert_close(c["lse"], c["lse_ref"], rtol=1e-3, atol=1e-3)


@requires_gpu
@pytest.mark.parametrize("B,nh,S", CASES)
def test_bidir_bwd(B, nh, S):
    c = _case(B, nh, S)
    H, dqkv = c["H"], c["dqkv"]
    assert not torch.isnan(dqkv.float()).any()
    assert not torch.isnan(c["D_ws"]).any()
    D_ref = (c["O"].float() * c["dO"].float()).view(B, S, nh, HD).sum(-1) \
        .permute(0, 2, 1).reshape(B * nh, S)
    print(f"bidir bwd ({B},{nh},{S}) D: max abs err "
          f"{(c['D_ws'] - D_ref).abs().max().item():.3e}")
    torch.testing.assert_close(c["D_ws"], D_ref, rtol=1e-2, atol=1e-2)
    for name, sl in (("dQ", slice(0, H)), ("dK", slice(H, 2 * H)),
                     ("dV", slice(2 * H, 3 * H))):
        e = rel_l2(dqkv[..., sl].float(), c["dqkv_ref"][..., sl])
        print(f"bidir bwd ({B},{nh},{S}) {name}: rel-L2 {e:.3e}")
        assert e < 3e-2, (name, e)
    # dbias_qkv from a zeroed buffer: the column sums of the returned dqkv
    e = rel_l2(c["dbias"], dqkv.float().reshape(B * S, 3 * H).sum(0))
    print(f"bidir bwd ({B},{nh},{S}) dbias vs colsum: {e:.3e}")
    assert e < 3e-2, e


@requires_gpu
def test_bidir_constant_v_rows():
    """V = one row vector everywhere: softmax rows sum to 1, so every row of
    O is that vector to bf16 rounding.  The bound: PV sums P rounded to bf16
    (each within 2^-9 relative) over the fp32 sum of the unrounded P, then O
    is rounded to bf16 once more: (1 + 2^-9)^2 - 1, plus 2^-15 for two fp32
    accumulations of 256 terms."""
    B, nh, S = 1, 2, 256
    c = _case(B, nh, S)  # its q and k only
    H = c["H"]
    g = torch.Generator().manual_seed(59)
    vrow = torch.randn(H, generator=g).to(DEV).bfloat16()
    qkv = c["qkv"].clone()
    qkv[..., 2 * H:] = vrow
    rcs, (O, _, _, _) = _run(B, nh, S, qkv, c["dO"])
    assert rcs == (0, 0), rcs
    want = vrow.float().expand(B, S, H)
    err = ((O.float() - want).abs() / want.abs()).max().item()
    print(f"bidir constant V: max rel err {err:.3e}")
    assert err <= (1 + 2.0 ** -9) ** 2 - 1 + 2.0 ** -15, err


@requires_gpu
@pytest.mark.parametrize("nh,S,H", [(2, 256, 256), (2, 192, 128)],
                         ids=["hd128", "s192"])
def test_bidir_refused(nh, S, H):
    g = torch.Generator().manual_seed(61)
    qkv = torch.randn(1, S, 3 * H, generator=g).to(DEV).bfloat16()
    dO = torch.randn(1, S, H, generator=g).to(DEV).bfloat16()
    rcs, outs = _run(1, nh, S, qkv, dO, H=H)
    assert rcs[0] != 0 and rcs[1] != 0, rcs
    for t in outs:
        assert torch.isnan(t.float()).all()
