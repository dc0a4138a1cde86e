# @gpu tests for attention dropout inside the banded flash kernels (head_dim
# 64 / 128, ob_flash_*_win_drop_bf16), the head_dim 80 / 96 ones, dense and
# banded (ob_flash_*_hd96_drop_bf16), and the layer route behind
# OB_FLASH_BAND_DROP.  Mask helpers, keys and read-back tolerance are those of
# tests/test_gpu_flash_dropout.py; O and dqkv are followed by one more NaN row,
# as in tests/test_gpu_flash_hd96.py.  Query i attends keys i - W < j <= i.
import math
import os
import pathlib
import subprocess
import sys

import pytest
import torch

from oracle.gpt2_oracle import KIND_BLOCK, OracleConfig, init_layer_params
from tests import dropout_ref as dr
from tests.gpu_helpers import ptr, stream
from tests.test_gpu_flash_dropout import (DEV, KEY, SEED, _assert_bits, _ext,
                                          _nan, keep_bits, rel_l2)

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs MI355X")]
HDS, P = [64, 80, 96, 128], 0.1
# (1,3,256,40): masked rows in most tiles, Z = 3 grid padding, z >= 1 offsets;
# (2,2,384,200): the band edge inside a tile, odd block count, batch stride;
# (1,1,1024,256): both LDS buffers, ranges that start past tile 0 (kv0 moves
# the Philox counter), idle dK/dV pairs.  W = 0: dense, head_dim 80 / 96 only
BANDED = [(1, 3, 256, 40), (2, 2, 384, 200), (1, 1, 1024, 256)]
DENSE = [(1, 3, 128, 0), (2, 2, 384, 0)]
PARITY = [(hd, *c) for hd in HDS for c in BANDED] + \
         [(hd, *c) for hd in (80, 96) for c in DENSE]


def _names(hd, d="_drop"):
    fam = "hd96" if hd in (80, 96) else "win"
    return f"ob_flash_fwd_{fam}{d}_bf16", f"ob_flash_bwd_{fam}_d{d}_bf16"


def _run(hd, B, nh, S, W, qkv, dO, p, key=KEY, dbias=None, names=None):
    """The two entries (p None: the plain ones; names: two dense dropout
    entries, which take no window) -> rc, O, lse, D_ws, dqkv, the two guard
    rows; every output pre-filled with NaN"""
    H, scale = nh * hd, 1.0 / math.sqrt(hd)
    Obuf, dbuf = _nan(B * S + 1, H), _nan(B * S + 1, 3 * H)
    O, dqkv = Obuf[:B * S].view(B, S, H), dbuf[:B * S].view(B, S, 3 * H)
    lse = _nan(B * nh, S, dtype=torch.float32)
    D_ws = torch.full_like(lse, float("nan"))
    fwd, bwd = (getattr(_ext(), n)
                for n in names or _names(hd, "" if p is None else "_drop"))
    tail = ([] if names else [W]) + [scale] + \
        ([] if p is None else [*key, p]) + [stream()]
    rc = (fwd(ptr(qkv), ptr(O), ptr(lse), B, S, H, nh, *tail),
          bwd(ptr(qkv), ptr(O), ptr(dO), ptr(lse), ptr(D_ws), ptr(dqkv),
              ptr(dbias), B, S, H, nh, *tail))
    torch.cuda.synchronize()
    return rc, O, lse, D_ws, dqkv, (Obuf[B * S], dbuf[B * S])


def heads(t, B, nh, S):  # [B, S, nh*hd] -> [B, nh, S, hd]
    return t.view(B, S, nh, -1).permute(0, 2, 1, 3)


def _band(S, W):
    dist = torch.arange(S, device=DEV)[:, None] - torch.arange(S, device=DEV)
    return (dist >= 0) & (dist < (W or S))


def _inputs(B, S, H):
    g = torch.Generator().manual_seed(59)
    return ((torch.randn(B, S, 3 * H, generator=g) * 0.5).to(DEV).bfloat16(),
            (torch.randn(B, S, H, generator=g) * 0.3).to(DEV).bfloat16())


@pytest.mark.parametrize("hd,B,nh,S,W", PARITY)
def test_parity_fp32_autograd(hd, B, nh, S, W):
    """Bounds of these kernels' p = 0 tests: rel-L2 2e-2 for O, LSE rtol =
    atol = 1e-3, 3e-2 per dQ/dK/dV and for dbias_qkv (from a non-zero start,
    against the reference's column sums); D_ws as those tests hold it, against
    rowsum(dO * O) of the kernel's own dropped O."""
    H = nh * hd
    qkv, dO = _inputs(B, S, H)
    qf = qkv.float().requires_grad_(True)
    q, k, v = (heads(qf[..., i * H:(i + 1) * H], B, nh, S) for i in range(3))
    w = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(hd)
    w = w.masked_fill(~_band(S, W), float("-inf"))
    lse_ref = torch.logsumexp(w, dim=-1).detach().reshape(B * nh, S)
    Pd = torch.softmax(w, dim=-1) * keep_bits(B, nh, S, P) * dr.scale(P)
    O_ref = torch.matmul(Pd, v).permute(0, 2, 1, 3).reshape(B, S, H)
    O_ref.backward(dO.float())
    start = torch.linspace(-1.0, 1.0, 3 * H, device=DEV)
    acc = start.clone()
    rc, O, lse, D_ws, dqkv, guard = _run(hd, B, nh, S, W, qkv, dO, P, dbias=acc)
    assert rc == (0, 0), _ext().ob_last_error()
    for t in (O, lse, D_ws, dqkv):
        assert not torch.isnan(t.float()).any()
    assert all(torch.isnan(g.float()).all() for g in guard)
    errs = {"O": rel_l2(O.float(), O_ref.detach())}
    for i, name in enumerate(("dQ", "dK", "dV")):
        sl = slice(i * H, (i + 1) * H)
        errs[name] = rel_l2(dqkv[..., sl].float(), qf.grad[..., sl])
    errs["dbias"] = rel_l2(acc - start, qf.grad.reshape(B * S, 3 * H).sum(0))
    print(f"band dropout parity hd{hd} ({B},{nh},{S},{W}) p={P}: rel-L2 {errs}"
          f", LSE max abs {(lse - lse_ref).abs().max().item():.3e}")
    torch.testing.assert_close(lse, lse_ref, rtol=1e-3, atol=1e-3)
    D_ref = heads(O.float() * dO.float(), B, nh, S).sum(-1).reshape(B * nh, S)
    torch.testing.assert_close(D_ws, D_ref, rtol=1e-2, atol=1e-2)
    for name, e in errs.items():
        assert e < (2e-2 if name == "O" else 3e-2), (name, e)


# mask read-back: the constructions of tests/test_gpu_flash_dropout.py with
# the uniform P = 1/min(q+1, W); 64-row one-hot bands, columns >= 64 zero

MB, MNH, MS, MW = 1, 3, 256, 96
READBACK = pytest.mark.parametrize("hd,p", [(hd, p) for hd in HDS
                                            for p in (0.1, 0.5)])


def one_hot_band(hd, band):
    """[MB, MS, MNH*hd] bf16: row r of the 64-row band has a 1 in column
    r % 64 of every head, everything else is zero"""
    t = torch.zeros(MB, MS, MNH, hd, device=DEV)
    r = torch.arange(band * 64, band * 64 + 64, device=DEV)
    t[:, r, :, r % 64] = 1.0
    return t.view(MB, MS, MNH * hd).bfloat16()


def _cnt():  # keys in the band of row q
    return torch.arange(1, MS + 1, device=DEV).clamp(max=MW).float()


@READBACK
def test_mask_readback_forward(hd, p):
    """Q = K = 0; V one-hot over the kv band makes O[q, d] = Pd[q, 64*band +
    d]: every in-band element against ob_dropout_mask, everything else 0."""
    H, cnt = MNH * hd, _cnt()
    keep, inband = keep_bits(MB, MNH, MS, p), _band(MS, MW)
    for band in range(MS // 64):
        qkv = torch.zeros(MB, MS, 3 * H, device=DEV, dtype=torch.bfloat16)
        qkv[..., 2 * H:] = one_hot_band(hd, band)
        rc, O, lse, *_ = _run(hd, MB, MNH, MS, MW, qkv, qkv[..., :H].clone(),
                              p)
        assert rc == (0, 0)
        torch.testing.assert_close(lse, cnt.log().expand(MB * MNH, MS),
                                   rtol=1e-3, atol=1e-3)
        raw = heads(O.float(), MB, MNH, MS)
        kv = band * 64 + torch.arange(64, device=DEV)
        where = inband[:, kv].expand(MB, MNH, MS, 64)
        assert (raw[..., :64][~where] == 0).all() and (raw[..., 64:] == 0).all()
        _assert_bits(raw[..., :64] * cnt[:, None] / dr.scale(p), keep[..., kv],
                     where, f"fwd hd{hd} p={p} band {band}")


@READBACK
def test_mask_readback_backward(hd, p):
    """Scores stay 0, V = 1, dO one-hot over the q band b1: dP = 1, D[q] =
    O[q, q % 64].  Q one-hot over b1 reads role 0's mask through dV and role
    1's sign bit through dK; K one-hot over the kv band b2 the dq kernel's mask
    through dQ.  dS = P * (factor - D), P = 1/min(q+1, W)."""
    H, cnt, sc, SCALE = MNH * hd, _cnt(), dr.scale(p), 1.0 / math.sqrt(hd)
    keep, inband = keep_bits(MB, MNH, MS, p), _band(MS, MW)
    qkv0 = torch.zeros(MB, MS, 3 * H, device=DEV, dtype=torch.bfloat16)
    qkv0[..., 2 * H:] = 1.0
    O = _run(hd, MB, MNH, MS, MW, qkv0, qkv0[..., :H].clone(), p)[1]

    def bwd(qkv, dO):  # its forward has the same scores and V: the same O
        rc, *_, dqkv, _ = _run(hd, MB, MNH, MS, MW, qkv, dO, p)
        assert rc == (0, 0)
        return dqkv

    for b1 in range(MS // 64):
        q = b1 * 64 + torch.arange(64, device=DEV)       # q of column d
        dO = one_hot_band(hd, b1)
        D = heads(O.float() * dO.float(), MB, MNH, MS).sum(-1)[:, :, q]
        qkv = qkv0.clone()
        qkv[..., :H] = one_hot_band(hd, b1)
        dqkv = bwd(qkv, dO)
        where = inband[q, :].t().expand(MB, MNH, MS, 64)  # [kv, d]
        want = keep[:, :, q, :].transpose(-1, -2)
        dV = heads(dqkv[..., 2 * H:].float(), MB, MNH, MS)[..., :64]
        assert (dV[~where] == 0).all()
        _assert_bits(dV * cnt[q][None, :] / sc, want, where,
                     f"dkdv role 0 hd{hd} p={p} q band {b1}")
        dK = heads(dqkv[..., H:2 * H].float(), MB, MNH, MS)[..., :64]
        fac = dK / SCALE * cnt[q][None, :] + D[:, :, None, :]
        _assert_bits(fac / sc, want, where,
                     f"dkdv role 1 hd{hd} p={p} q band {b1}")
        for b2 in range(b1 + 1):
            kv = b2 * 64 + torch.arange(64, device=DEV)
            qkv = qkv0.clone()
            qkv[..., H:2 * H] = one_hot_band(hd, b2)
            dQ = heads(bwd(qkv, dO)[..., :H].float(), MB, MNH, MS)
            fac = dQ[:, :, q, :64] / SCALE * cnt[q][:, None] + D[..., None]
            _assert_bits(fac / sc, keep[:, :, q, :][..., kv],
                         inband[q][:, kv].expand(MB, MNH, 64, 64),
                         f"dq hd{hd} p={p} q band {b1} kv band {b2}")


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[1:5], b[1:5]))


@pytest.mark.parametrize("hd", HDS)
def test_identities(hd):
    B, nh, S, W = 1, 3, 256, 40
    qkv, dO = _inputs(B, S, nh * hd)
    a = _run(hd, B, nh, S, W, qkv, dO, P)
    assert a[0] == (0, 0)
    # p = 0 is the plain entry; the same key gives the same bits
    assert _same(_run(hd, B, nh, S, W, qkv, dO, 0.0),
                 _run(hd, B, nh, S, W, qkv, dO, None))
    assert _same(_run(hd, B, nh, S, W, qkv, dO, P), a)
    # another tick: another mask, the LSE of the undropped P
    t = _run(hd, B, nh, S, W, qkv, dO, P, key=(KEY[0], KEY[1], KEY[2] + 1))
    assert not torch.equal(t[1], a[1]) and torch.equal(t[2], a[2])
    # W = 0 and W = S: one dense launch (hd96), the dense dropout entry (win)
    w0, ws = (_run(hd, B, nh, S, Wd, qkv, dO, P) for Wd in (0, S))
    assert w0[0] == (0, 0) and _same(w0, ws) and not _same(w0, a)
    if hd in (64, 128):
        dense = {64: ("ob_flash_fwd_nt_drop_bf16",
                      "ob_flash_bwd_nt_d_drop_bf16"),
                 128: ("ob_flash_fwd_drop_hd128_bf16",
                       "ob_flash_bwd_d_drop_hd128_bf16")}[hd]
        assert _same(w0, _run(hd, B, nh, S, 0, qkv, dO, P, names=dense))


@pytest.mark.parametrize("hd", [64, 96])
@pytest.mark.parametrize("B,S,nh,W,p,cause", [
    (1, 128, 2, 64, 0.1, b"head_dim"),          # H = 288: head_dim 144
    (1, 96, 2, 64, 0.1, b"multiple of 128"),
    (1, 128, 2, 64, 1.0, b"[0,1)"),
    (1, 128, 2, -1, 0.1, b"window"),
    (1025, 1024, 16, 64, 0.1, b"2^34"),         # 2^34 + 2^24 mask elements
], ids=["head_dim", "s96", "p1", "w-1", "2^34"])
def test_argument_checks(hd, B, S, nh, W, p, cause):
    """Both entries return non-zero before any launch (the buffers would be
    far too small for the last case) and name the cause."""
    H = 288 if cause == b"head_dim" else nh * hd
    qkv, dO = _inputs(1, 128, 16 * 96)
    Obuf, dbuf = _nan(129, 16 * 96), _nan(129, 3 * 16 * 96)
    lse, D_ws = (_nan(16, 128, dtype=torch.float32) for _ in range(2))
    fwd, bwd = (getattr(_ext(), n) for n in _names(hd))
    tail = (B, S, H, nh, W, 0.125, *KEY, p, stream())
    assert fwd(ptr(qkv), ptr(Obuf), ptr(lse), *tail) != 0
    assert cause in _ext().ob_last_error()
    assert bwd(ptr(qkv), ptr(Obuf), ptr(dO), ptr(lse), ptr(D_ws), ptr(dbuf),
               ptr(None), *tail) != 0
    assert cause in _ext().ob_last_error()
    torch.cuda.synchronize()
    for t in (Obuf, lse, D_ws, dbuf):
        assert torch.isnan(t.float()).all()


# the layer route: bf16 BLOCK, n_head 2, banded, attn_pdrop 0.1
LAYER_B, LAYER_S, LAYER_W, LAYER_LID, LAYER_TICK = 2, 256, 64, 1, 4


def layer_dims(hd):
    return dict(n_embd=2 * hd, n_head=2, n_layer=2, n_positions=LAYER_S,
                vocab_size=307)


def layer_flat(hd):
    return init_layer_params(OracleConfig(**layer_dims(hd)), KIND_BLOCK,
                             42 * 100 + LAYER_LID)


def make_layer(hd):
    from oobleck_amd.config import ModelConfig
    from oobleck_amd.layer import Layer
    layer = Layer(LAYER_LID, ModelConfig(**layer_dims(hd)), LAYER_B, LAYER_S,
                  1, torch.device(DEV), dtype="bf16", embd_pdrop=0.0,
                  resid_pdrop=0.0, attn_pdrop=P, dropout_seed=SEED,
                  attn_window=LAYER_W)
    layer.flat_param.copy_(layer_flat(hd).to(DEV))
    layer.refresh_weights()
    return layer


def layer_inputs(hd):
    g = torch.Generator().manual_seed(8)
    shape = (LAYER_B, LAYER_S, 2 * hd)
    return ((torch.randn(*shape, generator=g) * 0.5).bfloat16(),
            (torch.randn(*shape, generator=g) * 0.1).bfloat16())


def _layer_ref(hd):
    """fp32 restatement of the block at LAYER_TICK: dropout_ref's block with
    the band in the softmax and the ob_dropout_mask factor on P"""
    oc = OracleConfig(**layer_dims(hd))
    B, S, H, nh = LAYER_B, LAYER_S, 2 * hd, 2
    factor = (keep_bits(B, nh, S, P, key=(SEED, LAYER_LID, LAYER_TICK))
              * dr.scale(P)).cpu()
    flat = layer_flat(hd).clone().requires_grad_(True)
    x, dout = (t.float() for t in layer_inputs(hd))
    x.requires_grad_(True)
    p = dr._unpack(oc, KIND_BLOCK, flat)
    eps = oc.layer_norm_eps
    qkv = dr._ln(x, p["ln1_w"], p["ln1_b"], eps) @ p["w_qkv"] + p["b_qkv"]
    q, k, v = (heads(t, B, nh, S) for t in qkv.split(H, dim=-1))
    w = (q @ k.transpose(-1, -2) / math.sqrt(hd)).masked_fill(
        ~_band(S, LAYER_W).cpu(), float("-inf"))
    o = ((torch.softmax(w, -1) * factor) @ v).permute(0, 2, 1, 3)
    h = x + o.reshape(B, S, H) @ p["w_attnproj"] + p["b_attnproj"]
    m = dr._gelu(dr._ln(h, p["ln2_w"], p["ln2_b"], eps) @ p["w_fc"] + p["b_fc"])
    out = h + m @ p["w_mlpproj"] + p["b_mlpproj"]
    out.backward(dout)
    return out.detach(), x.grad, flat.grad


def test_layer_route_behind_the_switch(tmp_path):
    """The switch is read once per process: a fresh child with it (and
    OB_FLASH_HD96) set runs the four banded layers on the flash route within
    test_gpu_flash_hd128_dropout's layer bounds; this process refuses them."""
    assert "OB_FLASH_BAND_DROP" not in os.environ
    for hd in HDS:
        with pytest.raises(RuntimeError, match="attn_window"):
            make_layer(hd)
    out_path = tmp_path / "band_drop.pt"
    child = pathlib.Path(__file__).with_name("flash_band_drop_layer_child.py")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + \
          [str(child), str(out_path)]
    subprocess.run(cmd, check=True, timeout=300,
                   env=dict(os.environ, OB_FLASH_BAND_DROP="1",
                            OB_FLASH_HD96="1"))
    for hd, got in torch.load(out_path).items():
        assert got["uses_flash"] is True and got["attn_window"] == LAYER_W
        errs = [rel_l2(got[k].float(), r)
                for k, r in zip(("out", "din", "grad"), _layer_ref(hd))]
        print(f"band dropout layer hd{hd}: rel-L2 out, din, grad", errs)
        assert errs[0] < 1.5e-2 and errs[1] < 3e-2 and errs[2] < 3e-2, errs
