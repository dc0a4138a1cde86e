# @gpu tests for attention dropout inside the head_dim 128 flash kernels
# (ob_flash_fwd_drop_hd128_bf16 / ob_flash_bwd_d_drop_hd128_bf16) and the
# layer route behind OB_FLASH_HD128_DROP=1.  The mask definition, the
# read-back construction (derived there) and its tolerance are those of
# tests/test_gpu_flash_dropout.py; bands are 128 rows here.
import functools
import math
import os
import pathlib
import subprocess
import sys

import pytest
import torch

from oracle.gpt2_oracle import OracleConfig, init_layer_params
from tests import dropout_ref as dr
from tests.gpu_helpers import ptr, stream
from tests.test_gpu_flash_dropout import (DEV, KEY, _assert_bits, _check,
                                          _ext, _nan, keep_bits, rel_l2)

pytestmark = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
HD = 128
SCALE = 1.0 / math.sqrt(float(HD))
SEED, LAYER_ID, TICK = KEY
# (2,2,128): one folded block; (1,3,256): two blocks, Z = 3 grid padding,
# z >= 1 offsets; (2,2,384): odd block count; (1,1,1024): both LDS buffers,
# kv0 advancing through the counter, a dK/dV pair idle for 31 iterations
MASK_SHAPES = [(2, 2, 128), (1, 3, 256)]
PARITY_SHAPES = MASK_SHAPES + [(2, 2, 384), (1, 1, 1024)]
P_PARITY = 0.1


def fwd_drop(qkv, B, nh, S, p, key=KEY):
    """-> (O, lse), outputs pre-filled with NaN"""
    O, lse = _nan(B, S, nh * HD), _nan(B * nh, S, dtype=torch.float32)
    _check(_ext().ob_flash_fwd_drop_hd128_bf16(
        ptr(qkv), ptr(O), ptr(lse), B, S, nh * HD, nh, SCALE, *key, p,
        stream()), "flash_fwd_drop_hd128")
    torch.cuda.synchronize()
    return O, lse


def bwd_drop(qkv, O, dO, lse, B, nh, S, p, dbias=None):
    """-> (dqkv, D_ws), outputs pre-filled with NaN"""
    dqkv, D_ws = _nan(B, S, 3 * nh * HD), _nan(B * nh, S, dtype=torch.float32)
    _check(_ext().ob_flash_bwd_d_drop_hd128_bf16(
        ptr(qkv), ptr(O), ptr(dO), ptr(lse), ptr(D_ws), ptr(dqkv),
        ptr(dbias), B, S, nh * HD, nh, SCALE, *KEY, p, stream()),
        "flash_bwd_d_drop_hd128")
    torch.cuda.synchronize()
    return dqkv, D_ws


def heads(t, B, nh, S):
    """[B, S, nh*128] -> [B, nh, S, 128]"""
    return t.view(B, S, nh, HD).permute(0, 2, 1, 3)


def one_hot_band(B, nh, S, band):
    """[B, S, nh*128] bf16: row r of the 128-row band has a 1 in column
    r % 128 of every head, every other row is zero"""
    t = torch.zeros(B, S, nh, HD, device=DEV)
    r = torch.arange(band * HD, band * HD + HD, device=DEV)
    t[:, r, :, r % HD] = 1.0
    return t.view(B, S, nh * HD).bfloat16()


def _readback(raw, scaled, want, causal, what):
    assert (raw[~causal] == 0).all(), what
    _assert_bits(scaled, want, causal, "hd128 " + what)


@requires_gpu
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,nh,S", MASK_SHAPES)
def test_mask_readback_forward(B, nh, S, p):
    """Q = K = 0: P[q, kv] = 1/(q+1); V one-hot over a 128-row kv band makes
    O[q, d] = Pd[q, 128*band + d]."""
    H = nh * HD
    keep = keep_bits(B, nh, S, p)
    q1 = torch.arange(1, S + 1, device=DEV, dtype=torch.float32)
    for band in range(S // HD):
        qkv = torch.zeros(B, S, 3 * H, device=DEV, dtype=torch.bfloat16)
        qkv[..., 2 * H:] = one_hot_band(B, nh, S, band)
        O, lse = fwd_drop(qkv, B, nh, S, p)
        torch.testing.assert_close(lse, q1.log().expand(B * nh, S),
                                   rtol=1e-3, atol=1e-3)
        raw = heads(O.float(), B, nh, S)                  # [B, nh, q, d]
        kv = band * HD + torch.arange(HD, device=DEV)
        causal = (kv[None, :] < q1[:, None]).expand(B, nh, S, HD)
        _readback(raw, raw * q1[:, None] / dr.scale(p), keep[..., kv], causal,
                  f"fwd ({B},{nh},{S}) p={p} band {band}")


@requires_gpu
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,nh,S", MASK_SHAPES)
def test_mask_readback_backward(B, nh, S, p):
    """Scores stay 0, V = 1, dO one-hot over the q band b1: dP = 1 and
    D[q] = O[q, q % 128] on the band.  Q one-hot over b1 reads role 0's mask
    back through dV and the bit role 1 takes from the exchange through dK;
    K one-hot over the kv band b2 <= b1 reads the dq kernel's mask back,
    with factor = dS * (q+1) + D."""
    H = nh * HD
    keep = keep_bits(B, nh, S, p)
    qkv0 = torch.zeros(B, S, 3 * H, device=DEV, dtype=torch.bfloat16)
    qkv0[..., 2 * H:] = 1.0
    O, lse = fwd_drop(qkv0, B, nh, S, p)
    q1 = torch.arange(1, S + 1, device=DEV, dtype=torch.float32)
    idx = torch.arange(S, device=DEV)
    sc = dr.scale(p)
    for b1 in range(S // HD):
        tag = f"({B},{nh},{S}) p={p} q band {b1}"
        q = b1 * HD + torch.arange(HD, device=DEV)       # q of column d
        dO = one_hot_band(B, nh, S, b1)
        D = heads(O.float() * dO.float(), B, nh, S).sum(-1)  # [B, nh, S]
        qkv = qkv0.clone()
        qkv[..., :H] = dO
        dqkv, D_ws = bwd_drop(qkv, O, dO, lse, B, nh, S, p)
        torch.testing.assert_close(D_ws, D.view(B * nh, S), rtol=1e-6,
                                   atol=1e-6)
        causal = (idx[:, None] <= q[None, :]).expand(B, nh, S, HD)  # [kv, d]
        want = keep[:, :, q, :].transpose(-1, -2)        # [B, nh, kv, d]
        dV = heads(dqkv[..., 2 * H:].float(), B, nh, S)
        _readback(dV, dV * q1[q][None, :] / sc, want, causal,
                  "dkdv role 0 " + tag)
        dK = heads(dqkv[..., H:2 * H].float(), B, nh, S)
        fac = dK / SCALE * q1[q][None, :] + D[:, :, q][:, :, None, :]
        _readback(dK, fac / sc, want, causal, "dkdv role 1 " + tag)
        for b2 in range(b1 + 1):
            kv = b2 * HD + torch.arange(HD, device=DEV)
            qkv = qkv0.clone()
            qkv[..., H:2 * H] = one_hot_band(B, nh, S, b2)
            dqkv, _ = bwd_drop(qkv, O, dO, lse, B, nh, S, p)
            dQ = heads(dqkv[..., :H].float(), B, nh, S)[:, :, q, :]
            causal = (kv[None, :] <= q[:, None]).expand(B, nh, HD, HD)
            fac = dQ / SCALE * q1[q][:, None] + D[:, :, q][..., None]
            _readback(dQ, fac / sc, keep[:, :, q, :][..., kv], causal,
                      f"dq {tag} kv band {b2}")


@functools.lru_cache(maxsize=None)
def _case(B, nh, S):
    """Random inputs and the torch fp32 restatement (softmax, times factor,
    then PV); computed once per shape, never modified."""
    H = nh * HD
    g = torch.Generator().manual_seed(59)
    qkv = (torch.randn(B, S, 3 * H, generator=g) * 0.5).to(DEV).bfloat16()
    dO = (torch.randn(B, S, H, generator=g) * 0.3).to(DEV).bfloat16()
    factor = keep_bits(B, nh, S, P_PARITY) * dr.scale(P_PARITY)
    qf = qkv.float().requires_grad_(True)
    q, k, v = (heads(qf[..., i * H:(i + 1) * H], B, nh, S) for i in range(3))
    w = torch.matmul(q, k.transpose(-1, -2)) * SCALE
    mask = torch.tril(torch.ones(S, S, dtype=torch.bool, device=DEV))
    w = torch.where(mask, w, torch.tensor(float("-inf"), device=DEV))
    lse_ref = torch.logsumexp(w, dim=-1).detach().reshape(B * nh, S)
    O_ref = torch.matmul(torch.softmax(w, dim=-1) * factor, v) \
        .permute(0, 2, 1, 3).reshape(B, S, H)
    O_ref.backward(dO.float())
    return dict(H=H, qkv=qkv, dO=dO, O_ref=O_ref.detach(), lse_ref=lse_ref,
                dqkv_ref=qf.grad)


@requires_gpu
@pytest.mark.parametrize("B,nh,S", PARITY_SHAPES)
def test_parity_fp32_autograd(B, nh, S):
    """Bounds of tests/test_gpu_flash_hd128.py at p = 0: rel-L2 2e-2 for O,
    LSE rtol = atol = 1e-3, 3e-2 per dQ/dK/dV and for dbias_qkv (from a
    non-zero start, against the reference's column sums); D_ws bit-identical
    to ob_flash_dsum_bf16 of the same O and dO."""
    c = _case(B, nh, S)
    H = c["H"]
    O, lse = fwd_drop(c["qkv"], B, nh, S, P_PARITY)
    start = torch.linspace(-1.0, 1.0, 3 * H, device=DEV)
    acc = start.clone()
    dqkv, D_ws = bwd_drop(c["qkv"], O, c["dO"], lse, B, nh, S, P_PARITY,
                          dbias=acc)
    D = _nan(B * nh, S, dtype=torch.float32)
    _check(_ext().ob_flash_dsum_bf16(ptr(O), ptr(c["dO"]), ptr(D), B, S, H,
                                     nh, stream()), "dsum")
    torch.cuda.synchronize()
    errs = {"O": rel_l2(O.float(), c["O_ref"]),
            "dbias": rel_l2(acc - start,
                            c["dqkv_ref"].reshape(B * S, 3 * H).sum(0))}
    for i, name in enumerate(("dQ", "dK", "dV")):
        sl = slice(i * H, (i + 1) * H)
        errs[name] = rel_l2(dqkv[..., sl].float(), c["dqkv_ref"][..., sl])
    print(f"hd128 flash dropout parity ({B},{nh},{S}) rel-L2:", errs)
    assert not torch.isnan(O.float()).any()
    assert not torch.isnan(dqkv.float()).any()
    torch.testing.assert_close(lse, c["lse_ref"], rtol=1e-3, atol=1e-3)
    assert torch.equal(D_ws, D)
    for name, e in errs.items():
        assert e < (2e-2 if name == "O" else 3e-2), (name, e)


@requires_gpu
def test_p_zero_determinism_and_tick():
    B, nh, S = 1, 3, 256
    c = _case(B, nh, S)
    H = c["H"]
    O, lse = _nan(B, S, H), _nan(B * nh, S, dtype=torch.float32)
    _check(_ext().ob_flash_fwd_nt_bf16(ptr(c["qkv"]), ptr(O), ptr(lse), B, S,
                                       H, nh, SCALE, stream()),
           "flash_fwd_nt")
    dqkv, D_ws = _nan(B, S, 3 * H), _nan(B * nh, S, dtype=torch.float32)
    _check(_ext().ob_flash_bwd_nt_d_bf16(
        ptr(c["qkv"]), ptr(O), ptr(c["dO"]), ptr(lse), ptr(D_ws), ptr(dqkv),
        ptr(None), B, S, H, nh, SCALE, stream()), "flash_bwd_nt_d")
    torch.cuda.synchronize()
    O0, lse0 = fwd_drop(c["qkv"], B, nh, S, 0.0)
    dqkv0, D0 = bwd_drop(c["qkv"], O0, c["dO"], lse0, B, nh, S, 0.0)
    assert torch.equal(O0, O) and torch.equal(lse0, lse)
    assert torch.equal(dqkv0, dqkv) and torch.equal(D0, D_ws)

    Oa, lsea = fwd_drop(c["qkv"], B, nh, S, P_PARITY)
    Ob, lseb = fwd_drop(c["qkv"], B, nh, S, P_PARITY)
    assert torch.equal(Oa, Ob) and torch.equal(lsea, lseb)
    da, Da = bwd_drop(c["qkv"], Oa, c["dO"], lsea, B, nh, S, P_PARITY)
    db, Db = bwd_drop(c["qkv"], Oa, c["dO"], lsea, B, nh, S, P_PARITY)
    assert torch.equal(da, db) and torch.equal(Da, Db)
    Ot, lset = fwd_drop(c["qkv"], B, nh, S, P_PARITY,
                        key=(SEED, LAYER_ID, TICK + 1))
    assert not torch.equal(Ot, Oa)
    assert torch.equal(lset, lsea), "the LSE is that of the undropped P"


@requires_gpu
@pytest.mark.parametrize("B,S,H,nh,p,cause", [
    (1, 128, 256, 4, 0.1, b"head_dim"),       # head_dim 64
    (1, 96, 256, 2, 0.1, b"multiple of 128"),
    (1, 128, 256, 2, 1.0, b"[0,1)"),
    (1025, 1024, 2048, 16, 0.1, b"2^34"),     # 2^34 + 2^24 mask elements
])
def test_argument_checks(B, S, H, nh, p, cause):
    """Both entries return non-zero before any launch (the buffers would be
    far too small for the last case) and name the cause."""
    qkv, dqkv = _nan(1, 128, 3 * 256), _nan(1, 128, 3 * 256)
    O, lse = _nan(1, 128, 256), _nan(2, 128, dtype=torch.float32)
    D_ws = _nan(2, 128, dtype=torch.float32)
    ext = _ext()
    assert ext.ob_flash_fwd_drop_hd128_bf16(
        ptr(qkv), ptr(O), ptr(lse), B, S, H, nh, SCALE, *KEY, p,
        stream()) != 0
    assert cause in ext.ob_last_error()
    assert ext.ob_flash_bwd_d_drop_hd128_bf16(
        ptr(qkv), ptr(O), ptr(O), ptr(lse), ptr(D_ws), ptr(dqkv), ptr(None),
        B, S, H, nh, SCALE, *KEY, p, stream()) != 0
    assert cause in ext.ob_last_error()
    torch.cuda.synchronize()
    for t in (O, lse, dqkv, D_ws):
        assert torch.isnan(t.float()).all()


# layer level: bf16 BLOCK, n_embd 256, n_head 2, resid = attn = 0.1
LAYER_DIMS = dict(n_embd=256, n_head=2, n_layer=2, n_positions=128,
                  vocab_size=307)
LAYER_B, LAYER_S, LAYER_LID, LAYER_TICK, LAYER_P = 2, 128, 1, 4, 0.1


def _layer_flat():
    oc = OracleConfig(**LAYER_DIMS)
    return init_layer_params(oc, oc.layer_kind(LAYER_LID),
                             42 * 100 + LAYER_LID)


def make_layer():
    from oobleck_amd.config import ModelConfig
    from oobleck_amd.layer import Layer
    layer = Layer(LAYER_LID, ModelConfig(**LAYER_DIMS), LAYER_B, LAYER_S, 1,
                  torch.device(DEV), dtype="bf16", embd_pdrop=0.0,
                  resid_pdrop=LAYER_P, attn_pdrop=LAYER_P, dropout_seed=SEED)
    layer.flat_param.copy_(_layer_flat().to(DEV))
    layer.refresh_weights()
    return layer


def layer_inputs():
    g = torch.Generator().manual_seed(8)
    shape = (LAYER_B, LAYER_S, LAYER_DIMS["n_embd"])
    return ((torch.randn(*shape, generator=g) * 0.5).bfloat16(),
            (torch.randn(*shape, generator=g) * 0.1).bfloat16())


def _layer_ref():
    """fp32 restatement at LAYER_TICK, masks from ob_dropout_mask"""
    oc = OracleConfig(**LAYER_DIMS)
    B, S, H, nh = LAYER_B, LAYER_S, oc.n_embd, oc.n_head
    masks = {}
    for name, site, shape in (("attn", dr.SITE_ATTN, (B, nh, S, S)),
                              ("resid_attn", dr.SITE_RESID_ATTN, (B, S, H)),
                              ("resid_mlp", dr.SITE_RESID_MLP, (B, S, H))):
        n = math.prod(shape)
        keep = torch.empty(n, dtype=torch.uint8, device=DEV)
        _check(_ext().ob_dropout_mask(SEED, LAYER_LID, site, LAYER_TICK,
                                      LAYER_P, n, ptr(keep), stream()),
               "dropout_mask")
        torch.cuda.synchronize()
        masks[name] = dr.factor(keep.cpu().numpy(), LAYER_P, shape)
    x, dout = layer_inputs()
    out, dx, (grad,) = dr.stage_forward_backward(
        oc, [_layer_flat()], [LAYER_LID], x.float(), [masks],
        dout=dout.float())
    return out, dx, grad


@requires_gpu
def test_layer_route_behind_the_switch(tmp_path):
    """OB_FLASH_HD128_DROP is read once per process: a fresh child with it
    set takes the flash route and meets the bounds of
    test_layer_flash_dropout_parity; this process (unset) does not."""
    assert "OB_FLASH_HD128_DROP" not in os.environ
    assert make_layer().uses_flash is False
    out_path = tmp_path / "hd128_drop.pt"
    child = pathlib.Path(__file__).with_name("flash_hd128_drop_layer_child.py")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + \
          [str(child), str(out_path)]
    subprocess.run(cmd, check=True, timeout=300,
                   env=dict(os.environ, OB_FLASH_HD128_DROP="1"))
    got = torch.load(out_path)
    assert got["uses_flash"] is True
    errs = [rel_l2(got[k].float(), r)
            for k, r in zip(("out", "din", "grad"), _layer_ref())]
    print("hd128 flash dropout layer: rel-L2 out, din, grad", errs)
    assert errs[0] < 1.5e-2 and errs[1] < 3e-2 and errs[2] < 3e-2, errs
