# @gpu tests for attention dropout inside the flash kernels
# (ob_flash_fwd_nt_drop_bf16 / ob_flash_bwd_nt_d_drop_bf16) and the layer
# route that uses them.
#
# 1. the mask each of the three kernels applies, read back element for
#    element through one-hot operands and compared with ob_dropout_mask
#    (tests/test_gpu_dropout.py pins that export against the numpy Philox);
# 2. parity against fp32 autograd with the same masks made explicit;
# 3. p = 0 is the plain kernel, bit for bit;
# 4. determinism and keying;
# 5. a BLOCK layer with attention dropout stays on the flash path;
# 6. argument checks.
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

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
DEV = "cuda:0"
SCALE = 1.0 / math.sqrt(64.0)
# a seed with a non-zero high half, a tick above 2^32
SEED = (0xDEADBEEF << 32) | 0x1234567
TICK = (1 << 32) + 3
LAYER_ID = 5
KEY = (SEED, LAYER_ID, TICK)
# (2,2,128): one folded block; (1,3,256): two folded blocks, Z = 3 grid
# padding, z >= 1 index offsets; (2,2,384): odd block count, batch stride
MASK_SHAPES = [(2, 2, 128), (1, 3, 256)]
PARITY_SHAPES = MASK_SHAPES + [(2, 2, 384)]
# Read-back tolerance.  Every read-back value is one product of the exact
# fp32 P = 1/(q+1) with a factor, rounded to bf16 once when it becomes an
# MFMA operand and once when the result is stored: two relative errors of
# 2^-9, on values the test scales to at most 1 in magnitude (dq/dk: the
# rounded value is factor - D with |factor - D| <= 1/(1-p), divided by
# 1/(1-p) again), plus fp32 exp/log noise orders below.  2^-8 in all; the
# bound is 2^-7.  A wrong bit is off by 1.
BIT_TOL = 2.0 ** -7


def rel_l2(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _ext():
    from oobleck_amd._ext import get_ext
    return get_ext()


def _check(rc, what):
    from oobleck_amd._ext import check
    check(rc, what)


def _nan(*shape, dtype=torch.bfloat16):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def fwd_drop(qkv, B, nh, S, p, key=KEY):
    """-> (O, lse), outputs pre-filled with NaN"""
    H = nh * 64
    O, lse = _nan(B, S, H), _nan(B * nh, S, dtype=torch.float32)
    seed, lid, tick = key
    _check(_ext().ob_flash_fwd_nt_drop_bf16(
        ptr(qkv), ptr(O), ptr(lse), B, S, H, nh, SCALE, seed, lid, tick, p,
        stream()), "flash_fwd_nt_drop")
    torch.cuda.synchronize()
    return O, lse


def bwd_drop(qkv, O, dO, lse, B, nh, S, p, key=KEY, dbias=None):
    """-> (dqkv, D_ws), outputs pre-filled with NaN"""
    H = nh * 64
    dqkv, D_ws = _nan(B, S, 3 * H), _nan(B * nh, S, dtype=torch.float32)
    seed, lid, tick = key
    _check(_ext().ob_flash_bwd_nt_d_drop_bf16(
        ptr(qkv), ptr(O), ptr(dO), ptr(lse), ptr(D_ws), ptr(dqkv),
        ptr(dbias), B, S, H, nh, SCALE, seed, lid, tick, p, stream()),
        "flash_bwd_nt_d_drop")
    torch.cuda.synchronize()
    return dqkv, D_ws


@functools.lru_cache(maxsize=None)
def keep_bits(B, nh, S, p, key=KEY):
    """float [B, nh, S, S] on the GPU: 1 where OB_DROP_ATTN keeps (q, kv)"""
    seed, lid, tick = key
    n = B * nh * S * S
    keep = torch.empty(n, dtype=torch.uint8, device=DEV)
    _check(_ext().ob_dropout_mask(seed, lid, dr.SITE_ATTN, tick, p, n,
                                  ptr(keep), stream()), "dropout_mask")
    torch.cuda.synchronize()
    return keep.view(B, nh, S, S).float()


def heads(t, B, nh, S):
    """[B, S, nh*64] -> [B, nh, S, 64]"""
    return t.view(B, S, nh, 64).permute(0, 2, 1, 3)


def one_hot_band(B, nh, S, band):
    """[B, S, nh*64] bf16: row r of the 64-row band has a 1 in column r % 64
    of every head, every other row is zero"""
    t = torch.zeros(B, S, nh, 64, device=DEV)
    r = torch.arange(band * 64, band * 64 + 64, device=DEV)
    t[:, r, :, r % 64] = 1.0
    return t.view(B, S, nh * 64).bfloat16()


def _assert_bits(val, want, where, what):
    """val ~ want (0 or 1) on the elements `where` selects"""
    err = ((val - want).abs() * where).max().item()
    nbad = (((val - want).abs() > BIT_TOL) & where).sum().item()
    print(f"{what}: {int(where.sum().item())} elements, max |value - keep| "
          f"{err:.3e}, {nbad} beyond {BIT_TOL:.3e}")
    assert nbad == 0, (what, nbad, err)


# ---------------------------------------------------------------------------
# 1. mask read-back
# ---------------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,nh,S", MASK_SHAPES)
def test_mask_readback_forward(B, nh, S, p):
    """Q = K = 0 makes P[q, kv] = 1/(q+1) on the triangle; V one-hot over one
    64-row kv band makes O[q, d] = Pd[q, 64*band + d].  Every causal element
    of every (z, q, kv) is compared with ob_dropout_mask; everything above
    the diagonal must come out exactly zero."""
    H = nh * 64
    keep = keep_bits(B, nh, S, p)
    q1 = torch.arange(1, S + 1, device=DEV, dtype=torch.float32)
    qi = torch.arange(S, device=DEV)
    for band in range(S // 64):
        qkv = torch.zeros(B, S, 3 * H, device=DEV, dtype=torch.bfloat16)
        qkv[..., 2 * H:] = one_hot_band(B, nh, S, band)
        O, lse = fwd_drop(qkv, B, nh, S, p)
        torch.testing.assert_close(lse, q1.log().expand(B * nh, S),
                                   rtol=1e-3, atol=1e-3)
        raw = heads(O.float(), B, nh, S)                  # [B, nh, q, d]
        val = raw * q1[:, None] / dr.scale(p)
        kv = band * 64 + torch.arange(64, device=DEV)
        causal = (kv[None, :] <= qi[:, None]).expand(B, nh, S, 64)
        assert (raw[~causal] == 0).all()
        _assert_bits(val, keep[..., kv], causal,
                     f"fwd ({B},{nh},{S}) p={p} band {band}")


@functools.lru_cache(maxsize=None)
def _uniform_forward(B, nh, S, p):
    """Q = K = 0, V = 1: the forward whose stash every read-back backward
    uses.  O[q, :] = sum_kv Pd[q, kv], lse[q] = log(q + 1)."""
    H = nh * 64
    qkv = torch.zeros(B, S, 3 * H, device=DEV, dtype=torch.bfloat16)
    qkv[..., 2 * H:] = 1.0
    O, lse = fwd_drop(qkv, B, nh, S, p)
    return qkv, O, lse


@requires_gpu
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,nh,S", MASK_SHAPES)
def test_mask_readback_backward(B, nh, S, p):
    """Scores stay 0 (Q or K is 0), V = 1 and dO one-hot over the q band b1,
    so dP = 1 and D[q] = O[q, q % 64] on the band's rows and 0 elsewhere.
      * Q one-hot over b1, K = 0:
          dV[kv, d] = Pd[q, kv], dK[kv, d] = SCALE * dS[q, kv], q = 64*b1 + d
        dV reads back role 0's mask of the dkdv kernel, dK the bit role 1
        takes from the exchange;
      * Q = 0, K one-hot over the kv band b2 <= b1:
          dQ[q, d] = SCALE * dS[q, 64*b2 + d]
        reads back the dq kernel's mask,
    with dS = P * (factor - D), P = 1/(q+1): factor = dS * (q+1) + D."""
    H = nh * 64
    keep = keep_bits(B, nh, S, p)
    qkv0, O, lse = _uniform_forward(B, nh, S, p)
    q1 = torch.arange(1, S + 1, device=DEV, dtype=torch.float32)
    idx = torch.arange(S, device=DEV)
    sc = dr.scale(p)
    for b1 in range(S // 64):
        q = b1 * 64 + torch.arange(64, device=DEV)       # q of column d
        dO = one_hot_band(B, nh, S, b1)
        D = heads(O.float() * dO.float(), B, nh, S).sum(-1)  # [B, nh, S]
        # -- dkdv: both roles ------------------------------------------------
        qkv = qkv0.clone()
        qkv[..., :H] = one_hot_band(B, nh, S, b1)
        dqkv, D_ws = bwd_drop(qkv, O, dO, lse, B, nh, S, p)
        torch.testing.assert_close(D_ws, D.view(B * nh, S), rtol=1e-6,
                                   atol=1e-6)
        causal = (idx[:, None] <= q[None, :]).expand(B, nh, S, 64)  # [kv, d]
        want = keep[:, :, q, :].transpose(-1, -2)        # [B, nh, kv, d]
        dV = heads(dqkv[..., 2 * H:].float(), B, nh, S)
        assert (dV[~causal] == 0).all()
        _assert_bits(dV * q1[q][None, :] / sc, want, causal,
                     f"dkdv role 0 ({B},{nh},{S}) p={p} q band {b1}")
        dK = heads(dqkv[..., H:2 * H].float(), B, nh, S)
        fac = dK / SCALE * q1[q][None, :] + D[:, :, q][:, :, None, :]
        _assert_bits(fac / sc, want, causal,
                     f"dkdv role 1 ({B},{nh},{S}) p={p} q band {b1}")
        # -- dq --------------------------------------------------------------
        for b2 in range(b1 + 1):
            kv = b2 * 64 + torch.arange(64, device=DEV)
            qkv = qkv0.clone()
            qkv[..., H:2 * H] = one_hot_band(B, nh, S, b2)
            dqkv, _ = bwd_drop(qkv, O, dO, lse, B, nh, S, p)
            dQ = heads(dqkv[..., :H].float(), B, nh, S)[:, :, q, :]
            fac = dQ / SCALE * q1[q][:, None] + D[:, :, q][..., None]
            causal = (kv[None, :] <= q[:, None]).expand(B, nh, 64, 64)
            _assert_bits(fac / sc, keep[:, :, q, :][..., kv], causal,
                         f"dq ({B},{nh},{S}) p={p} q band {b1} kv band {b2}")


# ---------------------------------------------------------------------------
# 2. parity against fp32 autograd with explicit masks
# ---------------------------------------------------------------------------

P_PARITY = 0.1


@functools.lru_cache(maxsize=None)
def _case(B, nh, S):
    """Random inputs and the torch fp32 restatement (softmax, times factor,
    then PV); computed once per shape, never modified."""
    H = nh * 64
    g = torch.Generator().manual_seed(53)
    qkv = (torch.randn(B, S, 3 * H, generator=g) * 0.5).to(DEV).bfloat16()
    dO = (torch.randn(B, S, H, generator=g) * 0.3).to(DEV).bfloat16()
    factor = keep_bits(B, nh, S, P_PARITY) * dr.scale(P_PARITY)
    qf = qkv.float().requires_grad_(True)
    q, k, v = (heads(qf[..., i * H:(i + 1) * H], B, nh, S) for i in range(3))
    w = torch.matmul(q, k.transpose(-1, -2)) * SCALE
    mask = torch.tril(torch.ones(S, S, dtype=torch.bool, device=DEV))
    w = torch.where(mask, w, torch.tensor(float("-inf"), device=DEV))
    lse_ref = torch.logsumexp(w, dim=-1).detach()
    Pd = torch.softmax(w, dim=-1) * factor
    O_ref = torch.matmul(Pd, v).permute(0, 2, 1, 3).reshape(B, S, H)
    O_ref.backward(dO.float())
    O_ref = O_ref.detach()
    D_ref = heads(O_ref * dO.float(), B, nh, S).sum(-1)
    return dict(H=H, qkv=qkv, dO=dO, O_ref=O_ref, lse_ref=lse_ref,
                dqkv_ref=qf.grad, D_ref=D_ref)


@requires_gpu
@pytest.mark.parametrize("B,nh,S", PARITY_SHAPES)
def test_parity_fp32_autograd(B, nh, S):
    """Bounds of tests/test_gpu_flash_nt.py: rel-L2 2e-2 forward, 3e-2 per
    dQ/dK/dV, LSE rtol = atol = 1e-3; D_ws as tests/test_gpu_flash_fold.py
    holds it: bit-identical to ob_flash_dsum_bf16 of the same O and dO.
    dbias_qkv as test_fold_bwd_bias: from a non-zero start, against the
    reference's column sums and against ob_colsum_bf16(dqkv)."""
    c = _case(B, nh, S)
    H = c["H"]
    O, lse = fwd_drop(c["qkv"], B, nh, S, P_PARITY)
    e_o = rel_l2(O.float(), c["O_ref"])
    e_lse = (lse.view(B, nh, S) - c["lse_ref"]).abs().max().item()
    start = torch.linspace(-1.0, 1.0, 3 * H, device=DEV)
    acc = start.clone()
    dqkv, D_ws = bwd_drop(c["qkv"], O, c["dO"], lse, B, nh, S, P_PARITY,
                          dbias=acc)
    errs = {name: rel_l2(dqkv[..., sl].float(), c["dqkv_ref"][..., sl])
            for name, sl in (("dQ", slice(0, H)), ("dK", slice(H, 2 * H)),
                             ("dV", slice(2 * H, 3 * H)))}
    D = torch.empty(B * nh, S, device=DEV, dtype=torch.float32)
    _check(_ext().ob_flash_dsum_bf16(ptr(O), ptr(c["dO"]), ptr(D), B, S, H,
                                     nh, stream()), "dsum")
    cs = torch.zeros(3 * H, device=DEV)
    _check(_ext().ob_colsum_bf16(ptr(dqkv), ptr(cs), B * S, 3 * H, stream()),
           "colsum")
    torch.cuda.synchronize()
    added = acc - start
    e_bref = rel_l2(added, c["dqkv_ref"].reshape(B * S, 3 * H).sum(0))
    e_bcs = rel_l2(added, cs)
    e_d = rel_l2(D_ws.view(B, nh, S), c["D_ref"])
    print(f"flash dropout parity ({B},{nh},{S}) p={P_PARITY}: rel-L2 O "
          f"{e_o:.3e}, LSE max abs {e_lse:.3e}, dQ {errs['dQ']:.3e} dK "
          f"{errs['dK']:.3e} dV {errs['dV']:.3e}, D vs fp32 {e_d:.3e}, dbias "
          f"vs fp32 autograd {e_bref:.3e} vs ob_colsum_bf16(dqkv) "
          f"{e_bcs:.3e}")
    assert not torch.isnan(O.float()).any()
    assert not torch.isnan(dqkv.float()).any()
    assert e_o < 2e-2, e_o
    torch.testing.assert_close(lse.view(B, nh, S), c["lse_ref"], rtol=1e-3,
                               atol=1e-3)
    for name, e in errs.items():
        assert e < 3e-2, (name, e)
    assert torch.equal(D_ws, D)
    assert e_bref < 3e-2, e_bref
    assert e_bcs < 3e-2, e_bcs


# ---------------------------------------------------------------------------
# 3. p = 0 is the plain kernel
# ---------------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("B,nh,S", MASK_SHAPES)
def test_p_zero_is_the_plain_kernel(B, nh, S):
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
    assert torch.equal(O0, O)
    assert torch.equal(lse0, lse)
    assert torch.equal(dqkv0, dqkv)
    assert torch.equal(D0, D_ws)


# ---------------------------------------------------------------------------
# 4. determinism and keying
# ---------------------------------------------------------------------------

@requires_gpu
def test_determinism_and_keying():
    B, nh, S = 2, 2, 128
    c = _case(B, nh, S)
    O, lse = fwd_drop(c["qkv"], B, nh, S, P_PARITY)
    O2, lse2 = fwd_drop(c["qkv"], B, nh, S, P_PARITY)
    assert torch.equal(O, O2) and torch.equal(lse, lse2)
    for other in ((SEED, LAYER_ID, TICK + 1), (SEED, LAYER_ID + 1, TICK),
                  (SEED + 1, LAYER_ID, TICK), (SEED + (1 << 32), LAYER_ID, TICK),
                  (SEED, LAYER_ID, TICK + (1 << 32))):
        Oo, lseo = fwd_drop(c["qkv"], B, nh, S, P_PARITY, key=other)
        assert not torch.equal(Oo, O), other
        assert torch.equal(lseo, lse), "the LSE is that of the undropped P"
    d1, D1 = bwd_drop(c["qkv"], O, c["dO"], lse, B, nh, S, P_PARITY)
    d2, D2 = bwd_drop(c["qkv"], O, c["dO"], lse, B, nh, S, P_PARITY)
    assert torch.equal(d1, d2) and torch.equal(D1, D2)


# ---------------------------------------------------------------------------
# 5. layer level
# ---------------------------------------------------------------------------

LAYER_DIMS = dict(n_embd=128, n_head=2, n_layer=2, n_positions=128,
                  vocab_size=307)   # test_gpu_dropout's TINY64, 128 positions
LAYER_B, LAYER_S, LAYER_LID = 2, 128, 1
LAYER_PDROP = dict(resid=0.1, attn=0.1)
LAYER_TICK = 4


def _layer_flat():
    oc = OracleConfig(**LAYER_DIMS)
    return init_layer_params(oc, oc.layer_kind(LAYER_LID),
                             42 * 100 + LAYER_LID)


def make_layer(n_slots=2, pdrop=LAYER_PDROP):
    from oobleck_amd.config import ModelConfig
    from oobleck_amd.layer import Layer
    mc = ModelConfig(**LAYER_DIMS)
    if pdrop is None:
        layer = Layer(LAYER_LID, mc, LAYER_B, LAYER_S, n_slots,
                      torch.device(DEV), dtype="bf16")
    else:
        layer = Layer(LAYER_LID, mc, LAYER_B, LAYER_S, n_slots,
                      torch.device(DEV), dtype="bf16", embd_pdrop=0.0,
                      resid_pdrop=pdrop["resid"], attn_pdrop=pdrop["attn"],
                      dropout_seed=SEED)
    layer.flat_param.copy_(_layer_flat().to(DEV))
    layer.refresh_weights()
    return layer


def layer_inputs(i):
    """(x, dout) number i, bf16 on the CPU"""
    g = torch.Generator().manual_seed(8 + i)
    H = LAYER_DIMS["n_embd"]
    x = (torch.randn(LAYER_B, LAYER_S, H, generator=g) * 0.5).bfloat16()
    dout = (torch.randn(LAYER_B, LAYER_S, H, generator=g) * 0.1).bfloat16()
    return x, dout


def run_layer(layer, slot, x, dout, tick):
    out = torch.empty(LAYER_B, LAYER_S, LAYER_DIMS["n_embd"], device=DEV,
                      dtype=torch.bfloat16)
    din = torch.empty_like(out)
    layer.forward_slot(slot, x.to(DEV), out, tick=tick)
    layer.backward_slot(slot, dout.to(DEV), din)
    torch.cuda.synchronize()
    return out, din


@functools.lru_cache(maxsize=None)
def _layer_ref(i, tick):
    """fp32 restatement of inputs i at `tick`, masks from ob_dropout_mask"""
    oc = OracleConfig(**LAYER_DIMS)
    B, S, H, nh = LAYER_B, LAYER_S, oc.n_embd, oc.n_head
    masks = {}
    for name, site, p, shape in (
            ("attn", dr.SITE_ATTN, LAYER_PDROP["attn"], (B, nh, S, S)),
            ("resid_attn", dr.SITE_RESID_ATTN, LAYER_PDROP["resid"], (B, S, H)),
            ("resid_mlp", dr.SITE_RESID_MLP, LAYER_PDROP["resid"], (B, S, H))):
        n = math.prod(shape)
        keep = torch.empty(n, dtype=torch.uint8, device=DEV)
        _check(_ext().ob_dropout_mask(SEED, LAYER_LID, site, tick, p, n,
                                      ptr(keep), stream()), "dropout_mask")
        torch.cuda.synchronize()
        masks[name] = dr.factor(keep.cpu().numpy(), p, shape)
    x, dout = layer_inputs(i)
    out, dx, (grad,) = dr.stage_forward_backward(
        oc, [_layer_flat()], [LAYER_LID], x.float(), [masks],
        dout=dout.float())
    return out, dx, grad


def _assert_layer_bounds(out, din, grad, ref, what):
    """per-layer bounds of test_bf16_block_parity_dropout"""
    e_out = rel_l2(out.float().cpu(), ref[0])
    e_dx = rel_l2(din.float().cpu(), ref[1])
    e_g = rel_l2(grad.float().cpu(), ref[2])
    print(f"{what}: rel-L2 out {e_out:.3e} din {e_dx:.3e} grad {e_g:.3e}")
    assert e_out < 1.5e-2, e_out
    assert e_dx < 3e-2, e_dx
    assert e_g < 3e-2, e_g


@requires_gpu
def test_layer_flash_dropout_parity():
    layer = make_layer()
    assert layer.uses_flash
    x, dout = layer_inputs(0)
    out, din = run_layer(layer, 0, x, dout, LAYER_TICK)
    _assert_layer_bounds(out, din, layer.flat_grad, _layer_ref(0, LAYER_TICK),
                         "flash dropout layer")


@requires_gpu
def test_layer_eval_is_the_legacy_forward():
    x, _ = layer_inputs(0)

    def fwd(layer):
        out = torch.empty(LAYER_B, LAYER_S, LAYER_DIMS["n_embd"], device=DEV,
                          dtype=torch.bfloat16)
        layer.forward_slot(0, x.to(DEV), out)
        torch.cuda.synchronize()
        return out

    legacy = make_layer(pdrop=None)
    assert not legacy.has_dropout and legacy.uses_flash
    want = fwd(legacy)
    dropped = make_layer()
    assert dropped.uses_flash
    assert not torch.equal(fwd(dropped), want)
    dropped.eval()
    assert torch.equal(fwd(dropped), want)
    dropped.train()
    assert not torch.equal(fwd(dropped), want)


@requires_gpu
def test_layer_slots_keep_their_ticks():
    """Inputs 0 in slot 0 at tick 5, inputs 1 in slot 1 at tick 6, then
    backward slot 1, then slot 0: each backward regenerates ITS forward's
    masks (pattern of test_slot_tick_bookkeeping)."""
    layer = make_layer(n_slots=2)
    assert layer.uses_flash
    H = LAYER_DIMS["n_embd"]
    plan = ((0, 5), (1, 6))
    outs, dins = {}, {}
    for slot, tick in plan:
        x, _ = layer_inputs(slot)
        outs[slot] = torch.empty(LAYER_B, LAYER_S, H, device=DEV,
                                 dtype=torch.bfloat16)
        layer.forward_slot(slot, x.to(DEV), outs[slot], tick=tick)
    for slot in (1, 0):
        _, dout = layer_inputs(slot)
        dins[slot] = torch.empty_like(outs[slot])
        layer.backward_slot(slot, dout.to(DEV), dins[slot])
    torch.cuda.synchronize()
    refs = {slot: _layer_ref(slot, tick) for slot, tick in plan}
    grad_sum = refs[0][2] + refs[1][2]
    for slot, tick in plan:
        e_out = rel_l2(outs[slot].float().cpu(), refs[slot][0])
        e_dx = rel_l2(dins[slot].float().cpu(), refs[slot][1])
        print(f"slot {slot} tick {tick}: rel-L2 out {e_out:.3e} din "
              f"{e_dx:.3e}")
        assert e_out < 1.5e-2, (slot, e_out)
        assert e_dx < 3e-2, (slot, e_dx)
    e_g = rel_l2(layer.flat_grad.float().cpu(), grad_sum)
    print(f"both slots: rel-L2 grad {e_g:.3e}")
    assert e_g < 3e-2, e_g


@requires_gpu
def test_layer_flash_drop_off(tmp_path):
    """OB_FLASH_DROP=0 (read once per process, so a fresh child) restores
    the materialized-P route: uses_flash is false, the same bounds hold."""
    out_path = tmp_path / "drop0.pt"
    env = dict(os.environ, OB_FLASH_DROP="0")
    child = pathlib.Path(__file__).resolve().parent / "flash_drop_layer_child.py"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + \
          [str(child), str(out_path)]
    subprocess.run(cmd, check=True, env=env, timeout=300)
    got = torch.load(out_path)
    assert got["uses_flash"] is False
    _assert_layer_bounds(got["out"], got["din"], got["grad"],
                         _layer_ref(0, LAYER_TICK), "OB_FLASH_DROP=0 layer")


# ---------------------------------------------------------------------------
# 6. argument checks
# ---------------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("B,S,H,nh,p", [
    (1, 128, 128, 2, 1.0),       # p outside [0,1)
    (1, 128, 128, 2, -0.1),
    (1, 128, 128, 4, 0.1),       # head_dim 32
    (1, 96, 128, 2, 0.1),        # S not a multiple of 128
    (1025, 1024, 1024, 16, 0.1),  # B*nh*S*S = 2^34 + 2^24 mask elements
])
def test_argument_checks(B, S, H, nh, p):
    """Both entries return non-zero before any launch (the buffers would be
    far too small for the last case)."""
    qkv = torch.zeros(1, 128, 3 * 128, device=DEV, dtype=torch.bfloat16)
    O = torch.zeros(1, 128, 128, device=DEV, dtype=torch.bfloat16)
    lse = torch.zeros(4, 128, device=DEV, dtype=torch.float32)
    dqkv, D_ws = torch.zeros_like(qkv), torch.zeros_like(lse)
    ext = _ext()
    assert ext.ob_flash_fwd_nt_drop_bf16(
        ptr(qkv), ptr(O), ptr(lse), B, S, H, nh, SCALE, SEED, LAYER_ID, TICK,
        p, stream()) != 0
    assert ext.ob_flash_bwd_nt_d_drop_bf16(
        ptr(qkv), ptr(O), ptr(O), ptr(lse), ptr(D_ws), ptr(dqkv),
        ptr(None), B, S, H, nh, SCALE, SEED, LAYER_ID, TICK, p, stream()) != 0
    torch.cuda.synchronize()
    assert torch.equal(O, torch.zeros_like(O))
    assert torch.equal(dqkv, torch.zeros_like(dqkv))
