# @gpu tests for the document-masked flash kernels
# (oobleck_amd/csrc/ob_flash_seg_bf16.hip) behind ob_flash_seg_bounds_i32,
# ob_flash_fwd_seg_bf16 and ob_flash_bwd_seg_d_bf16: query i attends the keys
# of its own document up to i.  The reference is fp32 torch attention with the
# block-diagonal causal mask built from the same doc_start and autograd on the
# same bf16-rounded inputs, with the project's bounds for the banded kernels
# (tests/test_gpu_flash_window.py): the arithmetic is theirs.  Outputs are
# pre-filled with NaN: a row or column no block owns stays NaN and fails.
import math

import pytest
import torch

from tests.gpu_helpers import ptr, stream

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
DEV = "cuda:0"
# (B, nh, S, document starts per batch row beside the implicit 0)
# one document: the dense kernels' result; boundaries on tile edges, different
# per batch row; one-token documents, boundaries inside a tile and inside a
# wave's 32 rows, Z = 3 pads the grid; an odd block count and a last document
# of one token; long loops over both LDS buffers and blocks whose range starts
# past tile 0
CASES = [(1, 2, 256, [[]]), (2, 2, 256, [[64, 128], [192]]),
         (1, 3, 256, [[1, 2, 3, 100, 131]]), (2, 2, 384, [[37, 300], [383]]),
         (1, 1, 1024, [[520]])]
HDS = [64, 128]


def rel_l2(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _ext():
    from oobleck_amd._ext import get_ext
    return get_ext()


def _check(rc, what):
    from oobleck_amd._ext import check
    check(rc, what)


def _doc_start(B, S, starts):
    ds = torch.zeros(B, S, dtype=torch.int32)
    for b, st in enumerate(starts):
        ds[b, st] = 1
    return ds.to(DEV)


def _bounds(ds):
    lo = torch.full_like(ds, -7)
    hi = torch.full_like(ds, -7)
    _check(_ext().ob_flash_seg_bounds_i32(ptr(ds), ptr(lo), ptr(hi),
                                          ds.shape[0], ds.shape[1], stream()),
           "seg_bounds")
    return lo, hi


def _run(hd, B, nh, S, ds, qkv, dO, dbias=None):
    """bounds, then the two entries -> O, lse, D_ws, dqkv (pre-filled NaN)"""
    H, scale = nh * hd, 1.0 / math.sqrt(hd)
    lo, hi = _bounds(ds)
    O = torch.full_like(dO, float("nan"))
    lse = torch.full((B * nh, S), float("nan"), device=DEV)
    _check(_ext().ob_flash_fwd_seg_bf16(ptr(qkv), ptr(lo), ptr(O), ptr(lse), B,
                                        S, H, nh, scale, stream()), "fwd_seg")
    D_ws = torch.full_like(lse, float("nan"))
    dqkv = torch.full_like(qkv, float("nan"))
    _check(_ext().ob_flash_bwd_seg_d_bf16(
        ptr(qkv), ptr(O), ptr(dO), ptr(lse), ptr(lo), ptr(hi), ptr(D_ws),
        ptr(dqkv), ptr(dbias), B, S, H, nh, scale, stream()), "bwd_seg_d")
    torch.cuda.synchronize()
    return O, lse, D_ws, dqkv


def _ref(hd, B, nh, S, ds, qkv, dO):
    """fp32 torch: O, lse [B*nh, S], dqkv"""
    H = nh * hd
    qf = qkv.float().requires_grad_(True)
    q, k, v = (qf[..., i * H:(i + 1) * H].view(B, S, nh, hd)
               .permute(0, 2, 1, 3) for i in range(3))
    w = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(hd)
    doc = ds.clone()
    doc[:, 0] = 1
    doc = doc.cumsum(1)
    i = torch.arange(S, device=DEV)
    keep = (doc[:, :, None] == doc[:, None, :]) & (i[:, None] >= i[None, :])
    w = w.masked_fill(~keep[:, None], float("-inf"))
    lse = torch.logsumexp(w, dim=-1).detach().reshape(B * nh, S)
    O = torch.matmul(torch.softmax(w, dim=-1), v).permute(0, 2, 1, 3) \
        .reshape(B, S, H)
    O.backward(dO.float())
    return O.detach(), lse, qf.grad


@requires_gpu
@pytest.mark.parametrize("B,nh,S,starts", CASES)
@pytest.mark.parametrize("hd", HDS)
def test_seg_attention(hd, B, nh, S, starts):
    H = nh * hd
    g = torch.Generator().manual_seed(53)
    qkv = (torch.randn(B, S, 3 * H, generator=g) * 0.5).to(DEV).bfloat16()
    dO = (torch.randn(B, S, H, generator=g) * 0.3).to(DEV).bfloat16()
    ds = _doc_start(B, S, starts)
    dbias = torch.zeros(3 * H, device=DEV)
    O, lse, D_ws, dqkv = _run(hd, B, nh, S, ds, qkv, dO, dbias)
    refs = [("torch", _ref(hd, B, nh, S, ds, qkv, dO))]
    if not any(starts):  # one document: also the dense kernels' result
        On = torch.full_like(O, float("nan"))
        ln, dn = torch.full_like(lse, float("nan")), torch.full_like(lse, 0.)
        gn = torch.full_like(dqkv, float("nan"))
        sc = 1.0 / math.sqrt(hd)
        _check(_ext().ob_flash_fwd_nt_bf16(ptr(qkv), ptr(On), ptr(ln), B, S, H,
                                           nh, sc, stream()), "fwd_nt")
        _check(_ext().ob_flash_bwd_nt_d_bf16(
            ptr(qkv), ptr(On), ptr(dO), ptr(ln), ptr(dn), ptr(gn), ptr(None),
            B, S, H, nh, sc, stream()), "bwd_nt_d")
        torch.cuda.synchronize()
        refs.append(("nt", (On.float(), ln, gn.float())))
    for t in (O, lse, D_ws, dqkv):
        assert not torch.isnan(t.float()).any()
    for who, (O_ref, lse_ref, dqkv_ref) in refs:
        e = rel_l2(O.float(), O_ref)
        print(f"seg hd{hd} ({B},{nh},{S}) vs {who}: O rel-L2 {e:.3e}, lse max "
              f"abs err {(lse - lse_ref).abs().max().item():.3e}")
        assert e < 2e-2, e
        torch.testing.assert_close(lse, lse_ref, rtol=1e-3, atol=1e-3)
        for name, sl in (("dQ", slice(0, H)), ("dK", slice(H, 2 * H)),
                         ("dV", slice(2 * H, 3 * H))):
            e = rel_l2(dqkv[..., sl].float(), dqkv_ref[..., sl])
            print(f"seg hd{hd} ({B},{nh},{S}) vs {who} {name}: {e:.3e}")
            assert e < 3e-2, (who, name, e)
    D_ref = (O.float() * dO.float()).view(B, S, nh, hd).sum(-1) \
        .permute(0, 2, 1).reshape(B * nh, S)
    torch.testing.assert_close(D_ws, D_ref, rtol=1e-2, atol=1e-2)
    # dbias_qkv from a zeroed buffer: the column sums of the returned dqkv
    e = rel_l2(dbias, dqkv.float().reshape(B * S, 3 * H).sum(0))
    print(f"seg hd{hd} ({B},{nh},{S}) dbias vs colsum: {e:.3e}")
    assert e < 3e-2, e
    # one-token documents: P is the identity there, so O is V and dS is 0
    st = ds.bool()
    st[:, 0] = True
    one = st & torch.cat([st[:, 1:], torch.ones_like(st[:, :1])], 1)
    assert torch.equal(O[one], qkv[..., 2 * H:][one])
    assert (dqkv[..., :2 * H][one] == 0).all()


@requires_gpu
def test_seg_bounds():
    rows = [_doc_start(B, S, starts) for B, _, S, starts in CASES]
    rows.append(torch.ones(2, 256, dtype=torch.int32, device=DEV))
    garbage = _doc_start(2, 384, [[5, 200], [383]]) * -3
    garbage[:, 0] = torch.tensor([0, -12345])
    rows.append(garbage)
    for ds in rows:
        S = ds.shape[1]
        lo, hi = _bounds(ds)
        torch.cuda.synchronize()
        i = torch.arange(S, device=DEV).expand_as(ds)
        st = ds != 0
        st[:, 0] = True
        lo_ref = torch.where(st, i, 0).cummax(1).values
        # first start at or after i, then shifted: the first start after i
        nxt = torch.where(st, i, S).flip(1).cummin(1).values.flip(1)
        hi_ref = torch.cat([nxt[:, 1:], torch.full_like(nxt[:, :1], S)], 1) - 1
        assert torch.equal(lo, lo_ref.int()) and torch.equal(hi, hi_ref.int())
