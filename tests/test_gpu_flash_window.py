# @gpu tests for the locally banded flash kernels
# (oobleck_amd/csrc/ob_flash_win_bf16.hip) behind ob_flash_fwd_win_bf16 /
# ob_flash_bwd_win_d_bf16: query i attends keys i - W < j <= i.  The
# reference is fp32 torch attention with the band mask and autograd on the
# same bf16-rounded inputs, with the project's bounds for the dense kernels
# (tests/test_gpu_flash_hd128.py): the banded kernels add no rounding step
# and sum fewer terms.  Outputs are pre-filled with NaN: a row or column no
# block owns stays NaN and fails.
import functools
import math

import pytest
import torch

from tests.gpu_helpers import ptr, stream

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
DEV = "cuda:0"
# (2,2,256,64): band edges on tile boundaries; (1,3,256,96): the lower edge
# inside a tile, Z = 3 pads the grid; (1,2,256,1): self-attention only, fully
# masked rows in nearly every tile; (2,2,384,200): an odd block count, W no
# multiple of 8; (1,1,1024,256): long loops over both LDS buffers, blocks
# whose range starts past tile 0; (1,2,256,255): only the corner removed
CASES = [(2, 2, 256, 64), (1, 3, 256, 96), (1, 2, 256, 1), (2, 2, 384, 200),
         (1, 1, 1024, 256), (1, 2, 256, 255)]
HDS = [64, 128]


def rel_l2(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _ext():
    from oobleck_amd._ext import get_ext
    return get_ext()


def _check(rc, what):
    from oobleck_amd._ext import check
    check(rc, what)


def _run(hd, B, nh, S, W, qkv, dO, dbias=None):
    """The two banded entries -> O, lse, D_ws, dqkv (pre-filled with NaN)"""
    H, scale = nh * hd, 1.0 / math.sqrt(hd)
    O = torch.full_like(dO, float("nan"))
    lse = torch.full((B * nh, S), float("nan"), device=DEV)
    _check(_ext().ob_flash_fwd_win_bf16(ptr(qkv), ptr(O), ptr(lse), B, S, H,
                                        nh, W, scale, stream()), "fwd_win")
    D_ws = torch.full_like(lse, float("nan"))
    dqkv = torch.full_like(qkv, float("nan"))
    _check(_ext().ob_flash_bwd_win_d_bf16(
        ptr(qkv), ptr(O), ptr(dO), ptr(lse), ptr(D_ws), ptr(dqkv), ptr(dbias),
        B, S, H, nh, W, scale, stream()), "bwd_win_d")
    torch.cuda.synchronize()
    return O, lse, D_ws, dqkv


@functools.lru_cache(maxsize=None)
def _case(hd, B, nh, S, W):
    """Inputs, the fp32 torch reference and the kernels' outputs (dbias into
    a zeroed buffer); computed once per case, never modified."""
    H = nh * hd
    g = torch.Generator().manual_seed(47)
    qkv = (torch.randn(B, S, 3 * H, generator=g) * 0.5).to(DEV).bfloat16()
    dO = (torch.randn(B, S, H, generator=g) * 0.3).to(DEV).bfloat16()
    qf = qkv.float().requires_grad_(True)
    q, k, v = (qf[..., i * H:(i + 1) * H].view(B, S, nh, hd)
               .permute(0, 2, 1, 3) for i in range(3))
    w = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(hd)
    i = torch.arange(S, device=DEV)
    dist = i[:, None] - i[None, :]
    w = w.masked_fill(~((dist >= 0) & (dist < W)), float("-inf"))
    lse_ref = torch.logsumexp(w, dim=-1).detach().reshape(B * nh, S)
    P = torch.softmax(w, dim=-1)
    O_ref = torch.matmul(P, v).permute(0, 2, 1, 3).reshape(B, S, H)
    O_ref.backward(dO.float())
    # dS = P * (dP - D).  At W = 1, P is the identity and dP = D, so dQ and dK
    # are exactly 0 and a rel-L2 against them means nothing; the kernels'
    # rounding error there is relative to the two halves that cancel.  Their
    # scale: the norms of the D half alone, scale * (P * D) K and its
    # transpose times Q.
    with torch.no_grad():
        PD = P * (O_ref * dO.float()).view(B, S, nh, hd).sum(-1) \
            .permute(0, 2, 1)[..., None] / math.sqrt(hd)
        cancel = dict(dQ=torch.matmul(PD, k).norm().item(),
                      dK=torch.matmul(PD.transpose(-1, -2), q).norm().item())
    dbias = torch.zeros(3 * H, device=DEV)
    O, lse, D_ws, dqkv = _run(hd, B, nh, S, W, qkv, dO, dbias)
    return dict(H=H, qkv=qkv, dO=dO, O=O, lse=lse, D_ws=D_ws, dqkv=dqkv,
                dbias=dbias, O_ref=O_ref.detach(), lse_ref=lse_ref,
                dqkv_ref=qf.grad, cancel=cancel)


@requires_gpu
@pytest.mark.parametrize("B,nh,S,W", CASES)
@pytest.mark.parametrize("hd", HDS)
def test_window_fwd(hd, B, nh, S, W):
    c = _case(hd, B, nh, S, W)
    assert not torch.isnan(c["O"].float()).any()
    assert not torch.isnan(c["lse"]).any()
    e = rel_l2(c["O"].float(), c["O_ref"])
    print(f"win fwd hd{hd} ({B},{nh},{S},{W}): O rel-L2 {e:.3e}, lse max abs "
          f"err {(c['lse'] - c['lse_ref']).abs().max().item():.3e}")
    assert e < 2e-2, e
    torch.testing.assert_close(c["lse"], c["lse_ref"], rtol=1e-3, atol=1e-3)
    if W == 1:  # self-attention only: O is V, the LSE the diagonal score
        H = c["H"]
        assert torch.equal(c["O"], c["qkv"][..., 2 * H:])
        diag = (c["qkv"][..., :H].float() * c["qkv"][..., H:2 * H].float()) \
            .view(B, S, nh, hd).sum(-1).permute(0, 2, 1).reshape(B * nh, S)
        torch.testing.assert_close(c["lse"], diag / math.sqrt(hd), rtol=1e-3,
                                   atol=1e-3)


@requires_gpu
@pytest.mark.parametrize("B,nh,S,W", CASES)
@pytest.mark.parametrize("hd", HDS)
def test_window_bwd(hd, B, nh, S, W):
    c = _case(hd, B, nh, S, W)
    H, dqkv = c["H"], c["dqkv"]
    assert not torch.isnan(dqkv.float()).any()
    assert not torch.isnan(c["D_ws"]).any()
    D_ref = (c["O"].float() * c["dO"].float()).view(B, S, nh, hd).sum(-1) \
        .permute(0, 2, 1).reshape(B * nh, S)
    torch.testing.assert_close(c["D_ws"], D_ref, rtol=1e-2, atol=1e-2)
    for name, sl in (("dQ", slice(0, H)), ("dK", slice(H, 2 * H)),
                     ("dV", slice(2 * H, 3 * H))):
        got, ref = dqkv[..., sl].float(), c["dqkv_ref"][..., sl]
        if W == 1 and name != "dV":  # zero reference: see _case
            e = (got - ref).norm().item() / c["cancel"][name]
        else:
            e = rel_l2(got, ref)
        print(f"win bwd hd{hd} ({B},{nh},{S},{W}) {name}: rel-L2 {e:.3e}")
        assert e < 3e-2, (name, e)
    # dbias_qkv from a zeroed buffer: the column sums of the returned dqkv
    cs = dqkv.float().reshape(B * S, 3 * H).sum(0)
    e = rel_l2(c["dbias"], cs)
    print(f"win bwd hd{hd} ({B},{nh},{S},{W}) dbias vs colsum: {e:.3e}")
    assert e < 3e-2, e


@requires_gpu
@pytest.mark.parametrize("hd", HDS)
def test_window_0_and_S_are_the_dense_entries(hd):
    B, nh, S = 1, 2, 256
    c = _case(hd, B, nh, S, 64)  # its inputs only
    H, scale = c["H"], 1.0 / math.sqrt(hd)
    O = torch.full_like(c["dO"], float("nan"))
    lse = torch.full((B * nh, S), float("nan"), device=DEV)
    _check(_ext().ob_flash_fwd_nt_bf16(ptr(c["qkv"]), ptr(O), ptr(lse), B, S,
                                       H, nh, scale, stream()), "fwd_nt")
    D_ws = torch.full_like(lse, float("nan"))
    dqkv = torch.full_like(c["qkv"], float("nan"))
    _check(_ext().ob_flash_bwd_nt_d_bf16(
        ptr(c["qkv"]), ptr(O), ptr(c["dO"]), ptr(lse), ptr(D_ws), ptr(dqkv),
        ptr(None), B, S, H, nh, scale, stream()), "bwd_nt_d")
    torch.cuda.synchronize()
    for W in (0, S):
        got = _run(hd, B, nh, S, W, c["qkv"], c["dO"])
        for a, b in zip(got, (O, lse, D_ws, dqkv)):
            assert not torch.isnan(a.float()).any()
            assert torch.equal(a, b), W
