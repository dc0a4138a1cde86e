# @gpu tests for the grouped-query / multi-query flash kernels
# (oobleck_amd/csrc/ob_flash_gqa_bf16.hip) behind ob_flash_fwd_gqa_bf16 and
# ob_flash_bwd_gqa_d_bf16.  The reference is fp32 torch causal attention and
# autograd on the same bf16-rounded inputs, K and V expanded with
# repeat_interleave(G) over the head axis, so autograd itself sums a group's
# gradients.  Bounds are the head_dim 128 kernels' (tests/test_gpu_flash_hd128
# .py): the kernels add no rounding step, only longer fp32 sums.  Outputs are
# pre-filled with NaN: a row or column no block owns stays NaN and fails.
import functools
import math

import pytest
import torch

from oobleck_amd._ext import check as _check, get_ext as _ext
from tests.gpu_helpers import ptr, stream

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
DEV = "cuda:0"
HD = 128
SCALE = 1.0 / math.sqrt(float(HD))
# (B, nh, n_kv, S).  (1,2,1,128): one block, MQA; (2,4,2,256): two groups of
# two, the fold differs from the identity; (1,3,1,384): an odd group, an odd
# block count, grid padding; (1,8,1,256): G = 8, heads change many times
# inside one dK/dV block; (1,4,1,1024): long loops over both LDS buffers;
# (3,4,2,128): 12 heads, more than one per XCD in the forward / dq placement
SHAPES = [(1, 2, 1, 128), (2, 4, 2, 256), (1, 3, 1, 384), (1, 8, 1, 256),
          (1, 4, 1, 1024), (3, 4, 2, 128)]
SPLIT_CASES = [(*s, sp) for s in SHAPES
               for sp in sorted({0, 1, 2, s[1] // s[2]})
               if sp == 0 or (s[1] // s[2]) % sp == 0]


def rel_l2(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _nan_like(t):
    return torch.full_like(t, float("nan"))


def _inputs(B, nh, n_kv, S, hd=HD, seed=53):
    H, Hkv = nh * hd, n_kv * hd
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B, S, H + 2 * Hkv, generator=g) * 0.5) \
        .to(DEV).bfloat16()
    dO = (torch.randn(B, S, H, generator=g) * 0.3).to(DEV).bfloat16()
    return H, Hkv, qkv, dO


@functools.lru_cache(maxsize=None)
def _case(B, nh, n_kv, S):
    """Inputs, the fp32 torch reference (O, lse, dqkv) and the kernels'
    forward outputs; computed once per shape, never modified."""
    H, Hkv, qkv, dO = _inputs(B, nh, n_kv, S)
    G = nh // n_kv
    qf = qkv.float().requires_grad_(True)
    q = qf[..., :H].view(B, S, nh, HD).permute(0, 2, 1, 3)
    k = qf[..., H:H + Hkv].view(B, S, n_kv, HD).permute(0, 2, 1, 3) \
        .repeat_interleave(G, dim=1)
    v = qf[..., H + Hkv:].view(B, S, n_kv, HD).permute(0, 2, 1, 3) \
        .repeat_interleave(G, dim=1)
    w = torch.matmul(q, k.transpose(-1, -2)) * SCALE
    mask = torch.tril(torch.ones(S, S, dtype=torch.bool, device=DEV))
    w = torch.where(mask, w, torch.tensor(float("-inf"), device=DEV))
    lse_ref = torch.logsumexp(w, dim=-1).detach().reshape(B * nh, S)
    O_ref = torch.matmul(torch.softmax(w, dim=-1), v) \
        .permute(0, 2, 1, 3).reshape(B, S, H)
    O_ref.backward(dO.float())

    O = _nan_like(dO)
    lse = torch.full((B * nh, S), float("nan"), device=DEV)
    _check(_ext().ob_flash_fwd_gqa_bf16(ptr(qkv), ptr(O), ptr(lse), B, S, H,
                                        nh, n_kv, SCALE, stream()),
           "flash_fwd_gqa")
    torch.cuda.synchronize()
    # D of the kernels' own O, as the backward defines it
    D_ref = (O.float() * dO.float()).view(B, S, nh, HD).sum(-1) \
        .permute(0, 2, 1).reshape(B * nh, S).contiguous()
    return dict(H=H, Hkv=Hkv, W=H + 2 * Hkv, qkv=qkv, dO=dO, O=O, lse=lse,
                O_ref=O_ref.detach(), lse_ref=lse_ref, D_ref=D_ref,
                dqkv_ref=qf.grad)


def _bwd(c, B, nh, n_kv, S, split, dbias=None):
    """-> (dqkv, D_ws), outputs pre-filled with NaN; the slab holds `split`
    parts exactly (split 0: room for G)"""
    dqkv, D_ws = _nan_like(c["qkv"]), _nan_like(c["D_ref"])
    parts = split if split else nh // n_kv
    slab = torch.full((parts * B * S * 2 * c["Hkv"],), float("nan"),
                      device=DEV)
    _check(_ext().ob_flash_bwd_gqa_d_bf16(
        ptr(c["qkv"]), ptr(c["O"]), ptr(c["dO"]), ptr(c["lse"]), ptr(D_ws),
        ptr(dqkv), ptr(dbias), B, S, c["H"], nh, n_kv, split, ptr(slab),
        slab.numel(), SCALE, stream()), "flash_bwd_gqa_d")
    torch.cuda.synchronize()
    return dqkv, D_ws


def _check_dqkv(c, dqkv, tag):
    H, Hkv, W = c["H"], c["Hkv"], c["W"]
    assert not torch.isnan(dqkv.float()).any(), tag
    for name, sl in (("dQ", slice(0, H)), ("dK", slice(H, H + Hkv)),
                     ("dV", slice(H + Hkv, W))):
        e = rel_l2(dqkv[..., sl].float(), c["dqkv_ref"][..., sl])
        print(f"gqa {tag} {name}: rel-L2 {e:.3e}")
        assert e < 3e-2, (name, e)


@requires_gpu
@pytest.mark.parametrize("B,nh,n_kv,S", SHAPES)
def test_gqa_fwd(B, nh, n_kv, S):
    c = _case(B, nh, n_kv, S)
    assert not torch.isnan(c["O"].float()).any()
    assert not torch.isnan(c["lse"]).any()
    e = rel_l2(c["O"].float(), c["O_ref"])
    print(f"gqa fwd ({B},{nh},{n_kv},{S}): O rel-L2 {e:.3e}, lse max abs err "
          f"{(c['lse'] - c['lse_ref']).abs().max().item():.3e}")
    assert e < 2e-2, e
    torch.testing.assert_close(c["lse"], c["lse_ref"], rtol=1e-3, atol=1e-3)


@requires_gpu
@pytest.mark.parametrize("B,nh,n_kv,S,split", SPLIT_CASES)
def test_gqa_bwd(B, nh, n_kv, S, split):
    """dqkv, D_ws and dbias_qkv (accumulated from a known non-zero start: a
    block covered twice would double a column against ob_colsum_bf16(dqkv));
    a second call with the same split gives the same dqkv bits."""
    c = _case(B, nh, n_kv, S)
    W = c["W"]
    tag = f"bwd ({B},{nh},{n_kv},{S}) split={split}"
    start = torch.linspace(-1.0, 1.0, W, device=DEV)
    acc = start.clone()
    dqkv, D_ws = _bwd(c, B, nh, n_kv, S, split, acc)
    assert not torch.isnan(D_ws).any()
    print(f"gqa D {tag}: max abs err "
          f"{(D_ws - c['D_ref']).abs().max().item():.3e}")
    torch.testing.assert_close(D_ws, c["D_ref"], rtol=1e-2, atol=1e-2)
    _check_dqkv(c, dqkv, tag)
    added = acc - start
    assert not torch.isnan(added).any()
    ref = c["dqkv_ref"].reshape(B * S, W).sum(0)
    cs = torch.zeros(W, device=DEV)
    _check(_ext().ob_colsum_bf16(ptr(dqkv), ptr(cs), B * S, W, stream()),
           "colsum")
    torch.cuda.synchronize()
    e_ref, e_cs = rel_l2(added, ref), rel_l2(added, cs)
    print(f"gqa bias {tag}: rel-L2 vs fp32 autograd {e_ref:.3e}, vs "
          f"ob_colsum_bf16(dqkv) {e_cs:.3e}")
    assert e_ref < 3e-2, e_ref
    assert e_cs < 3e-2, e_cs
    if split:
        again, _ = _bwd(c, B, nh, n_kv, S, split)
        assert torch.equal(again, dqkv)


@requires_gpu
def test_gqa_all_kv_heads_is_the_dense_entry():
    """n_kv == nh: the layouts coincide and the dense entries run."""
    B, nh, S = 1, 3, 256
    H, _, qkv, dO = _inputs(B, nh, nh, S)
    ext, runs = _ext(), []
    for gqa in (False, True):
        O, dqkv = _nan_like(dO), _nan_like(qkv)
        lse = torch.full((B * nh, S), float("nan"), device=DEV)
        D_ws = _nan_like(lse)
        if gqa:
            _check(ext.ob_flash_fwd_gqa_bf16(ptr(qkv), ptr(O), ptr(lse), B, S,
                                             H, nh, nh, SCALE, stream()),
                   "fwd_gqa")
            _check(ext.ob_flash_bwd_gqa_d_bf16(
                ptr(qkv), ptr(O), ptr(dO), ptr(lse), ptr(D_ws), ptr(dqkv),
                ptr(None), B, S, H, nh, nh, 0, ptr(None), 0, SCALE, stream()),
                "bwd_gqa")
        else:
            _check(ext.ob_flash_fwd_nt_bf16(ptr(qkv), ptr(O), ptr(lse), B, S,
                                            H, nh, SCALE, stream()), "fwd_nt")
            _check(ext.ob_flash_bwd_nt_d_bf16(
                ptr(qkv), ptr(O), ptr(dO), ptr(lse), ptr(D_ws), ptr(dqkv),
                ptr(None), B, S, H, nh, SCALE, stream()), "bwd_nt_d")
        torch.cuda.synchronize()
        runs.append((O, lse, D_ws, dqkv))
    for a, b in zip(*runs):
        assert not torch.isnan(a.float()).any()
        assert torch.equal(a, b)


@requires_gpu
@pytest.mark.parametrize("nh,n_kv,hd,split,slab_parts,cause", [
    (2, 1, 64, 0, 2, b"head_dim"),
    (3, 2, HD, 0, 2, b"n_kv"),
    (2, 1, HD, 2, 1, b"slab"),
], ids=["hd64", "nh_mod_n_kv", "slab"])
def test_gqa_entries_refuse(nh, n_kv, hd, split, slab_parts, cause):
    """Returns non-zero, names the cause and launches nothing."""
    B, S = 1, 128
    H, Hkv, qkv, dO = _inputs(B, nh, n_kv, S, hd)
    O, dqkv = _nan_like(dO), _nan_like(qkv)
    lse = torch.full((B * nh, S), float("nan"), device=DEV)
    D_ws = _nan_like(lse)
    slab = torch.full((slab_parts * B * S * 2 * Hkv,), float("nan"),
                      device=DEV)
    ext = _ext()
    if cause != b"slab":  # the forward takes no slab
        rc = ext.ob_flash_fwd_gqa_bf16(ptr(qkv), ptr(O), ptr(lse), B, S, H,
                                       nh, n_kv, SCALE, stream())
        assert rc != 0 and cause in ext.ob_last_error()
    rc = ext.ob_flash_bwd_gqa_d_bf16(
        ptr(qkv), ptr(O), ptr(dO), ptr(lse), ptr(D_ws), ptr(dqkv), ptr(None),
        B, S, H, nh, n_kv, split, ptr(slab), slab.numel(), SCALE, stream())
    assert rc != 0 and cause in ext.ob_last_error()
    torch.cuda.synchronize()
    for t in (O, lse, D_ws, dqkv, slab):
        assert torch.isnan(t.float()).all()
