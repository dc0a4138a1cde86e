# @gpu tests for the head_dim 80 / 96 flash kernels
# (oobleck_amd/csrc/ob_flash_hd96_bf16.hip) behind ob_flash_fwd_hd96_bf16 /
# ob_flash_bwd_hd96_d_bf16, dense (W = 0) and banded (query i attends keys
# i - W < j <= i), in the manner of tests/test_gpu_flash_window.py and with its
# reference and bounds: fp32 torch attention with the band mask and autograd
# on the same bf16-rounded inputs; the bounds hold for the head sizes on
# either side (64, 128) and these kernels add no rounding step.  Outputs are
# pre-filled with NaN, and O and dqkv are the leading part of a buffer with one
# more NaN row: a head_dim 80 padding column that escapes lands there or in
# the next head, where the comparison catches it.
import functools
import math

import pytest
import torch

from tests.gpu_helpers import ptr, stream
from tests.test_gpu_flash_window import DEV, _check, _ext, rel_l2

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
# (1,3,128,0): one forward block, two dK/dV blocks, Z = 3 pads the grid;
# (2,2,384,0): an odd block count in the fold; (1,2,256,1): the masked-row
# rule in nearly every tile; (2,2,384,200): the band edge inside a tile;
# (1,1,1024,256): both LDS buffers, ranges starting past tile 0;
# (1,2,256,255): only the corner removed
CASES = [(1, 3, 128, 0), (2, 2, 384, 0), (1, 2, 256, 1), (2, 2, 384, 200),
         (1, 1, 1024, 256), (1, 2, 256, 255)]
HDS = [80, 96]


def _run(B, nh, S, H, W, qkv, dO, dbias=None):
    """The two entries -> rc, O, lse, D_ws, dqkv, the two guard rows; every
    output pre-filled with NaN"""
    scale = 1.0 / math.sqrt(H / nh)
    nan = float("nan")
    Obuf = torch.full((B * S + 1, H), nan, device=DEV, dtype=torch.bfloat16)
    dbuf = torch.full((B * S + 1, 3 * H), nan, device=DEV,
                      dtype=torch.bfloat16)
    O, dqkv = Obuf[:B * S].view(B, S, H), dbuf[:B * S].view(B, S, 3 * H)
    lse = torch.full((B * nh, S), nan, device=DEV)
    D_ws = torch.full_like(lse, nan)
    rc = (_ext().ob_flash_fwd_hd96_bf16(ptr(qkv), ptr(O), ptr(lse), B, S, H,
                                        nh, W, scale, stream()),
          _ext().ob_flash_bwd_hd96_d_bf16(
              ptr(qkv), ptr(O), ptr(dO), ptr(lse), ptr(D_ws), ptr(dqkv),
              ptr(dbias), B, S, H, nh, W, scale, stream()))
    torch.cuda.synchronize()
    return rc, O, lse, D_ws, dqkv, (Obuf[B * S], dbuf[B * S])


def _inputs(B, S, H):
    g = torch.Generator().manual_seed(47)
    qkv = (torch.randn(B, S, 3 * H, generator=g) * 0.5).to(DEV).bfloat16()
    dO = (torch.randn(B, S, H, generator=g) * 0.3).to(DEV).bfloat16()
    return qkv, dO


@functools.lru_cache(maxsize=None)
def _case(hd, B, nh, S, W):
    """Inputs, the fp32 torch reference and the kernels' outputs (dbias into
    a zeroed buffer); computed once per case, never modified."""
    H, Wm = nh * hd, W or S
    qkv, dO = _inputs(B, S, H)
    qf = qkv.float().requires_grad_(True)
    q, k, v = (qf[..., i * H:(i + 1) * H].view(B, S, nh, hd)
               .permute(0, 2, 1, 3) for i in range(3))
    w = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(hd)
    i = torch.arange(S, device=DEV)
    dist = i[:, None] - i[None, :]
    w = w.masked_fill(~((dist >= 0) & (dist < Wm)), float("-inf"))
    lse_ref = torch.logsumexp(w, dim=-1).detach().reshape(B * nh, S)
    P = torch.softmax(w, dim=-1)
    O_ref = torch.matmul(P, v).permute(0, 2, 1, 3).reshape(B, S, H)
    O_ref.backward(dO.float())
    # W = 1: dQ and dK are exactly 0 (P is the identity and dP = D); the
    # kernels' rounding error is relative to the halves that cancel, scale *
    # (P * D) K and its transpose times Q (tests/test_gpu_flash_window.py)
    with torch.no_grad():
        PD = P * (O_ref * dO.float()).view(B, S, nh, hd).sum(-1) \
            .permute(0, 2, 1)[..., None] / math.sqrt(hd)
        cancel = dict(dQ=torch.matmul(PD, k).norm().item(),
                      dK=torch.matmul(PD.transpose(-1, -2), q).norm().item())
    dbias = torch.zeros(3 * H, device=DEV)
    rc, O, lse, D_ws, dqkv, guard = _run(B, nh, S, H, W, qkv, dO, dbias)
    _check(rc[0], "fwd_hd96"), _check(rc[1], "bwd_hd96_d")
    return dict(H=H, qkv=qkv, dO=dO, O=O, lse=lse, D_ws=D_ws, dqkv=dqkv,
                guard=guard, dbias=dbias, O_ref=O_ref.detach(),
                lse_ref=lse_ref, dqkv_ref=qf.grad, cancel=cancel)


@requires_gpu
@pytest.mark.parametrize("B,nh,S,W", CASES)
@pytest.mark.parametrize("hd", HDS)
def test_hd96_fwd(hd, B, nh, S, W):
    c = _case(hd, B, nh, S, W)
    assert not torch.isnan(c["O"].float()).any()
    assert not torch.isnan(c["lse"]).any()
    assert torch.isnan(c["guard"][0].float()).all()
    e = rel_l2(c["O"].float(), c["O_ref"])
    print(f"hd96 fwd hd{hd} ({B},{nh},{S},{W}): O rel-L2 {e:.3e}, lse max abs "
          f"err {(c['lse'] - c['lse_ref']).abs().max().item():.3e}")
    assert e < 2e-2, e
    torch.testing.assert_close(c["lse"], c["lse_ref"], rtol=1e-3, atol=1e-3)


@requires_gpu
@pytest.mark.parametrize("B,nh,S,W", CASES)
@pytest.mark.parametrize("hd", HDS)
def test_hd96_bwd(hd, B, nh, S, W):
    c = _case(hd, B, nh, S, W)
    H, dqkv = c["H"], c["dqkv"]
    assert not torch.isnan(dqkv.float()).any()
    assert not torch.isnan(c["D_ws"]).any()
    assert torch.isnan(c["guard"][1].float()).all()
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
        print(f"hd96 bwd hd{hd} ({B},{nh},{S},{W}) {name}: rel-L2 {e:.3e}")
        assert e < 3e-2, (name, e)
    # dbias_qkv from a zeroed buffer: the column sums of the returned dqkv
    cs = dqkv.float().reshape(B * S, 3 * H).sum(0)
    e = rel_l2(c["dbias"], cs)
    print(f"hd96 bwd hd{hd} ({B},{nh},{S},{W}) dbias vs colsum: {e:.3e}")
    assert e < 3e-2, e


@requires_gpu
@pytest.mark.parametrize("hd", HDS)
def test_window_0_and_S_are_bit_equal(hd):
    B, nh, S, _ = CASES[0]
    c = _case(hd, *CASES[0])
    rc, *got = _run(B, nh, S, c["H"], S, c["qkv"], c["dO"])
    assert rc == (0, 0)
    for a, b in zip(got[:4], (c["O"], c["lse"], c["D_ws"], c["dqkv"])):
        assert torch.equal(a, b)


@requires_gpu
@pytest.mark.parametrize("hd,S,W", [(64, 128, 0), (72, 128, 0), (96, 192, 0),
                                    (96, 128, -1)],
                         ids=["hd64", "hd72", "s192", "w-1"])
def test_bad_arguments_launch_nothing(hd, S, W):
    B, nh = 1, 2
    qkv, dO = _inputs(B, S, nh * hd)
    rc, *outs, guard = _run(B, nh, S, nh * hd, W, qkv, dO)
    assert rc[0] != 0 and rc[1] != 0
    for t in outs:
        assert torch.isnan(t.float()).all()
