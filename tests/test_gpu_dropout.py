# @gpu dropout: the stateless Philox mask, the standalone dropout kernels
# (f32 + bf16), layer / model parity with masks against the torch
# restatement in tests/dropout_ref.py, slot/tick bookkeeping, eval and
# determinism, and the pp1 pipeline with and without the fwd/bwd overlap.
from __future__ import annotations

import ctypes
import json
import os
import pathlib
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle.gpt2_oracle import OracleConfig, init_layer_params
from tests import dropout_ref as dr
from tests.gpu_helpers import ptr, stream

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
DEV = torch.device("cuda:0")
REPO_ROOT = pathlib.Path(__file__).resolve().parent.parent

TINY24 = dict(n_embd=96, n_head=4, n_layer=3, n_positions=64, vocab_size=211)
TINY64 = dict(n_embd=128, n_head=2, n_layer=2, n_positions=96, vocab_size=307)

SEEDS = [(1 << 32) + 12345, (0xDEADBEEF << 32) | 0x1234567]
P_ALL = dict(embd=0.1, resid=0.1, attn=0.1)


def ext():
    from oobleck_amd._ext import get_ext
    return get_ext()


def check(rc, what):
    from oobleck_amd._ext import check as _check
    _check(rc, what)


def gpu_mask(seed, layer_id, site, tick, p, n) -> torch.Tensor:
    keep = torch.empty(n, dtype=torch.uint8, device=DEV)
    check(ext().ob_dropout_mask(seed, layer_id, site, tick, p, n, ptr(keep),
                                stream()), "dropout_mask")
    return keep


def gpu_layer_masks(seed, layer_id, kind, tick, pdrop, B, S, H, nh) -> dict:
    """dropout_ref.layer_masks with the keep bytes exported by the extension
    (test_mask_matches_numpy_reference ties the export to the numpy one)."""
    def f(site, p, shape):
        keep = gpu_mask(seed, layer_id, site, tick, p, int(np.prod(shape)))
        return dr.factor(keep.cpu().numpy(), p, shape)
    m = {}
    if kind == 0 and pdrop.get("embd", 0) > 0:
        m["embd"] = f(dr.SITE_EMBD, pdrop["embd"], (B, S, H))
    if kind == 1:
        if pdrop.get("attn", 0) > 0:
            m["attn"] = f(dr.SITE_ATTN, pdrop["attn"], (B, nh, S, S))
        if pdrop.get("resid", 0) > 0:
            m["resid_attn"] = f(dr.SITE_RESID_ATTN, pdrop["resid"], (B, S, H))
            m["resid_mlp"] = f(dr.SITE_RESID_MLP, pdrop["resid"], (B, S, H))
    return m


def cfgs(d):
    from oobleck_amd.config import ModelConfig
    return ModelConfig(**d), OracleConfig(**d)


def flats_for(oc, seed=42):
    return [init_layer_params(oc, oc.layer_kind(i), seed * 100 + i)
            for i in range(oc.n_layers_total)]


def make_layer(mc, lid, flat, B, S, n_slots=2, dtype="f32", seed=SEEDS[0],
               pdrop=P_ALL):
    from oobleck_amd.layer import Layer
    layer = Layer(lid, mc, B, S, n_slots, DEV, dtype=dtype,
                  embd_pdrop=pdrop.get("embd", 0.0),
                  resid_pdrop=pdrop.get("resid", 0.0),
                  attn_pdrop=pdrop.get("attn", 0.0), dropout_seed=seed)
    layer.flat_param.copy_(flat.to(DEV))
    layer.refresh_weights()
    return layer


# ---------------------------------------------------------------------------
# 1. the mask
# ---------------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_matches_numpy_reference(p):
    n = 4099  # not a multiple of 4 or 8
    for seed in SEEDS:
        for tick in (0, (1 << 32) + 3):
            for site in range(4):
                got = gpu_mask(seed, 5, site, tick, p, n).cpu().numpy()
                want = dr.keep_mask(seed, 5, site, tick, p, n)
                assert np.array_equal(got, want), (seed, tick, site)


@requires_gpu
def test_mask_keep_fraction():
    n, p = 1 << 20, 0.1
    sigma = (0.09 / n) ** 0.5
    for seed in SEEDS:
        mean = gpu_mask(seed, 2, dr.SITE_RESID_ATTN, 0, p,
                        n).float().mean().item()
        print(f"keep fraction seed={seed:#x}: {mean:.6f} (6 sigma = "
              f"{6 * sigma:.2e})")
        assert abs(mean - 0.9) < 6 * sigma, (seed, mean)


# ---------------------------------------------------------------------------
# 2. standalone kernels
# ---------------------------------------------------------------------------

KEY = (SEEDS[1], 7, dr.SITE_RESID_MLP, (1 << 32) + 3)
SHAPES = [(131, 768), (37, 1600)]


def _factor(p, rows, cols):
    keep = gpu_mask(*KEY, p, rows * cols)
    return (keep.float() * dr.scale(p)).view(rows, cols)


def _bf16_ulp(ref: torch.Tensor) -> torch.Tensor:
    """One bf16 ulp at the magnitude of ref (fp32), floor at the smallest
    normal's ulp."""
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 7)


@requires_gpu
@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_scale_and_add_f32(rows, cols, p):
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, cols, generator=g).to(DEV)
    res = torch.randn(rows, cols, generator=g).to(DEV)
    f = _factor(p, rows, cols)
    n = rows * cols
    y = torch.empty_like(x)
    check(ext().ob_dropout_scale_f32(*KEY, p, ptr(x), ptr(y), n, stream()),
          "scale")
    torch.testing.assert_close(y, x * f, rtol=1e-6, atol=0)
    xa = x.clone()  # y == x
    check(ext().ob_dropout_scale_f32(*KEY, p, ptr(xa), ptr(xa), n, stream()),
          "scale alias")
    assert torch.equal(xa, y)
    want = res + x * f
    ya = torch.empty_like(x)
    check(ext().ob_dropout_add_f32(*KEY, p, ptr(x), ptr(res), ptr(ya), n,
                                   stream()), "add")
    torch.testing.assert_close(ya, want, rtol=1e-6, atol=0)
    ta = x.clone()  # y == t
    check(ext().ob_dropout_add_f32(*KEY, p, ptr(ta), ptr(res), ptr(ta), n,
                                   stream()), "add alias")
    assert torch.equal(ta, ya)


@requires_gpu
@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_scale_and_add_bf16(rows, cols, p):
    g = torch.Generator().manual_seed(rows + 1)
    x = torch.randn(rows, cols, generator=g).to(DEV).bfloat16()
    res = torch.randn(rows, cols, generator=g).to(DEV).bfloat16()
    f = _factor(p, rows, cols)
    n = rows * cols

    def close(got, ref32):
        want = ref32.bfloat16().float()
        err = (got.float() - want).abs()
        assert (err <= _bf16_ulp(ref32)).all(), err.max().item()
        # dropped elements are exactly what the reference says
        return want

    y = torch.empty_like(x)
    check(ext().ob_dropout_scale_bf16(*KEY, p, ptr(x), ptr(y), n, stream()),
          "scale")
    close(y, x.float() * f)
    assert (y[f == 0] == 0).all()
    xa = x.clone()
    check(ext().ob_dropout_scale_bf16(*KEY, p, ptr(xa), ptr(xa), n, stream()),
          "scale alias")
    assert torch.equal(xa, y)
    # a misaligned view and an odd length take the scalar path: same mask
    # semantics are per element index of the tensor handed in
    xo = x.flatten()[1:4098].contiguous()
    buf = torch.empty(4098, dtype=torch.bfloat16, device=DEV)
    yo = buf[1:]  # 2-byte aligned only
    check(ext().ob_dropout_scale_bf16(*KEY, p, ptr(xo), ptr(yo), 4097,
                                      stream()), "scale odd")
    fo = (gpu_mask(*KEY, p, 4097).float() * dr.scale(p))
    close(yo, xo.float() * fo)

    ya = torch.empty_like(x)
    check(ext().ob_dropout_add_bf16(*KEY, p, ptr(x), ptr(res), ptr(ya), n,
                                    stream()), "add")
    close(ya, res.float() + x.float() * f)
    ta = x.clone()
    check(ext().ob_dropout_add_bf16(*KEY, p, ptr(ta), ptr(res), ptr(ta), n,
                                    stream()), "add alias")
    assert torch.equal(ta, ya)
    # vector path + tail: n = 8k + 5 on aligned pointers
    nt = 8 * 300 + 5
    xt, rt = x.flatten()[:nt].contiguous(), res.flatten()[:nt].contiguous()
    yt = torch.empty_like(xt)
    check(ext().ob_dropout_add_bf16(*KEY, p, ptr(xt), ptr(rt), ptr(yt), nt,
                                    stream()), "add tail")
    assert torch.equal(yt, ya.flatten()[:nt])


@requires_gpu
@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_dropout_scale_colsum(rows, cols, dtype):
    p = 0.1
    g = torch.Generator().manual_seed(rows + 2)
    dy = (torch.randn(rows, cols, generator=g) * 0.1).to(DEV)
    db0 = torch.randn(cols, generator=g).to(DEV)
    f = _factor(p, rows, cols)
    if dtype == "bf16":
        dy = dy.bfloat16()
        fn = ext().ob_dropout_scale_colsum_bf16
    else:
        fn = ext().ob_dropout_scale_colsum_f32
    dm = torch.empty_like(dy)
    db = db0.clone()
    check(fn(*KEY, p, ptr(dy), ptr(dm), ptr(db), rows, cols, stream()), "cs")
    ref32 = dy.float() * f
    if dtype == "f32":
        torch.testing.assert_close(dm, ref32, rtol=1e-6, atol=0)
        want_dm = ref32
    else:
        want_dm = ref32.bfloat16().float()
        assert ((dm.float() - want_dm).abs() <= _bf16_ulp(ref32)).all()
    ref_sum = dm.double().sum(0)
    bound = 1e-5 * dm.double().abs().sum(0)
    err = (db.double() - db0.double() - ref_sum).abs()
    print(f"colsum {dtype} {rows}x{cols}: max err {err.max().item():.3e}, "
          f"min bound {bound.min().item():.3e}")
    assert (err <= bound).all(), (err.max().item(), bound.min().item())
    # in place: dm == dy
    dya = dy.clone()
    dba = db0.clone()
    check(fn(*KEY, p, ptr(dya), ptr(dya), ptr(dba), rows, cols, stream()),
          "cs alias")
    assert torch.equal(dya, dm)


# ---------------------------------------------------------------------------
# 3. layer parity, f32
# ---------------------------------------------------------------------------

@requires_gpu
def test_embed_layer_parity_dropout():
    mc, oc = cfgs(TINY24)
    flat = flats_for(oc)[0]
    B, S, H = 2, 48, oc.n_embd
    tick = (1 << 32) + 9
    g = torch.Generator().manual_seed(6)
    ids = torch.randint(0, oc.vocab_size, (B, S), generator=g)
    dout = torch.randn(B, S, H, generator=g) * 0.1
    emb = make_layer(mc, 0, flat, B, S)
    out = torch.empty(B, S, H, device=DEV)
    emb.forward_slot(0, ids.to(DEV), out, tick=tick)
    emb.backward_slot(0, dout.to(DEV), None)
    torch.cuda.synchronize()
    masks = gpu_layer_masks(SEEDS[0], 0, 0, tick, P_ALL, B, S, H, oc.n_head)
    ref_out, _, (ref_grad,) = dr.stage_forward_backward(
        oc, [flat], [0], ids, [masks], dout=dout)
    assert (ref_out == 0).any(), "precondition: some elements dropped"
    torch.testing.assert_close(out.cpu(), ref_out, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(emb.flat_grad.cpu(), ref_grad, rtol=1e-3,
                               atol=1e-3)


@requires_gpu
@pytest.mark.parametrize("dims,B,S", [(TINY24, 2, 48), (TINY64, 2, 96)])
def test_block_layer_parity_dropout(dims, B, S):
    mc, oc = cfgs(dims)
    flat = flats_for(oc)[1]
    H = oc.n_embd
    layer = make_layer(mc, 1, flat, B, S)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, S, H, generator=g) * 0.5
    dout = torch.randn(B, S, H, generator=g) * 0.1
    out = torch.empty(B, S, H, device=DEV)
    din = torch.empty_like(out)
    layer.forward_slot(0, x.to(DEV), out, tick=3)
    layer.backward_slot(0, dout.to(DEV), din)
    torch.cuda.synchronize()
    masks = gpu_layer_masks(SEEDS[0], 1, 1, 3, P_ALL, B, S, H, oc.n_head)
    ref_out, ref_dx, (ref_grad,) = dr.stage_forward_backward(
        oc, [flat], [1], x, [masks], dout=dout)
    torch.testing.assert_close(out.cpu(), ref_out, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(din.cpu(), ref_dx, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(layer.flat_grad.cpu(), ref_grad, rtol=1e-3,
                               atol=1e-3)


def _run_model(layers, ids, labels, slot, tick, B, S, H, act=torch.float32):
    L = len(layers)
    x = ids
    for lid, layer in enumerate(layers):
        if lid == L - 1:
            out = torch.zeros(1, device=DEV)
            layer.forward_slot(slot, x, out, labels, tick=tick)
        else:
            out = torch.empty(B, S, H, device=DEV, dtype=act)
            layer.forward_slot(slot, x, out, tick=tick)
        x = out
    return x


def _backward_model(layers, slot, B, S, H, act=torch.float32):
    dout = None
    for lid in range(len(layers) - 1, -1, -1):
        din = None if lid == 0 else torch.empty(B, S, H, device=DEV,
                                                dtype=act)
        layers[lid].backward_slot(slot, dout, din)
        dout = din


def _model_masks(oc, tick, B, S):
    return [gpu_layer_masks(SEEDS[0], lid, oc.layer_kind(lid), tick, P_ALL,
                            B, S, oc.n_embd, oc.n_head)
            for lid in range(oc.n_layers_total)]


@requires_gpu
def test_full_model_parity_dropout():
    mc, oc = cfgs(TINY24)
    flats = flats_for(oc)
    B, S, H, L = 2, 48, oc.n_embd, oc.n_layers_total
    layers = [make_layer(mc, lid, flats[lid], B, S) for lid in range(L)]
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(0, oc.vocab_size, (B, S), generator=g)
    loss = _run_model(layers, ids.to(DEV), ids.to(DEV), 0, 11, B, S, H)
    _backward_model(layers, 0, B, S, H)
    torch.cuda.synchronize()
    ref_loss, _, ref_grads = dr.stage_forward_backward(
        oc, flats, list(range(L)), ids, _model_masks(oc, 11, B, S),
        labels=ids)
    torch.testing.assert_close(loss.cpu()[0], ref_loss, rtol=1e-4, atol=1e-5)
    for lid, layer in enumerate(layers):
        torch.testing.assert_close(layer.flat_grad.cpu(), ref_grads[lid],
                                   rtol=1e-3, atol=1e-3)


# ---------------------------------------------------------------------------
# 4. bf16 block (head_dim 64)
# ---------------------------------------------------------------------------

def rel_l2(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


@requires_gpu
@pytest.mark.parametrize("attn_p", [0.0, 0.1])
def test_bf16_block_parity_dropout(attn_p):
    """Per-layer bounds of test_bf16_per_layer_parity (1.5e-2 forward, 3e-2
    grads and din, rel-L2, reference evaluated on the bf16 inputs the layer
    consumed).  attn_p = 0 at S = 128 stays on the flash path."""
    dims = dict(TINY64, n_positions=128)
    mc, oc = cfgs(dims)
    B, S, H = 2, 128, oc.n_embd
    pdrop = dict(resid=0.1, attn=attn_p)
    flat = flats_for(oc)[1]
    layer = make_layer(mc, 1, flat, B, S, dtype="bf16", pdrop=pdrop)
    g = torch.Generator().manual_seed(8)
    x = (torch.randn(B, S, H, generator=g) * 0.5).bfloat16()
    dout = (torch.randn(B, S, H, generator=g) * 0.1).bfloat16()
    out = torch.empty(B, S, H, device=DEV, dtype=torch.bfloat16)
    din = torch.empty_like(out)
    layer.forward_slot(0, x.to(DEV), out, tick=4)
    layer.backward_slot(0, dout.to(DEV), din)
    torch.cuda.synchronize()
    masks = gpu_layer_masks(SEEDS[0], 1, 1, 4, pdrop, B, S, H, oc.n_head)
    assert ("attn" in masks) == (attn_p > 0)
    ref_out, ref_dx, (ref_grad,) = dr.stage_forward_backward(
        oc, [flat], [1], x.float(), [masks], dout=dout.float())
    e_out = rel_l2(out.float().cpu(), ref_out)
    e_dx = rel_l2(din.float().cpu(), ref_dx)
    e_g = rel_l2(layer.flat_grad.cpu(), ref_grad)
    print(f"bf16 block attn_p={attn_p}: rel-L2 out {e_out:.3e} "
          f"din {e_dx:.3e} grad {e_g:.3e}")
    assert e_out < 1.5e-2
    assert e_dx < 3e-2
    assert e_g < 3e-2


# ---------------------------------------------------------------------------
# 5. slot and tick bookkeeping
# ---------------------------------------------------------------------------

@requires_gpu
def test_slot_tick_bookkeeping():
    """A in slot 0 at tick 5, B in slot 1 at tick 6, then backward slot 1,
    then slot 0: each backward regenerates ITS forward's masks."""
    mc, oc = cfgs(TINY24)
    flats = flats_for(oc)
    B, S, H, L = 2, 48, oc.n_embd, oc.n_layers_total
    layers = [make_layer(mc, lid, flats[lid], B, S, n_slots=2)
              for lid in range(L)]
    g = torch.Generator().manual_seed(21)
    batches = [torch.randint(0, oc.vocab_size, (B, S), generator=g)
               for _ in range(2)]
    losses = []
    for slot, tick in ((0, 5), (1, 6)):
        ids = batches[slot].to(DEV)
        losses.append(_run_model(layers, ids, ids, slot, tick, B, S, H))
    _backward_model(layers, 1, B, S, H)
    _backward_model(layers, 0, B, S, H)
    torch.cuda.synchronize()
    ref_sum = [torch.zeros_like(f) for f in flats]
    for slot, tick in ((0, 5), (1, 6)):
        ref_loss, _, gs = dr.stage_forward_backward(
            oc, flats, list(range(L)), batches[slot],
            _model_masks(oc, tick, B, S), labels=batches[slot])
        torch.testing.assert_close(losses[slot].cpu()[0], ref_loss,
                                   rtol=1e-4, atol=1e-5)
        for acc, gi in zip(ref_sum, gs):
            acc += gi
    for lid, layer in enumerate(layers):
        torch.testing.assert_close(layer.flat_grad.cpu(), ref_sum[lid],
                                   rtol=1e-3, atol=1e-3)


# ---------------------------------------------------------------------------
# 6./7. eval, zero, determinism
# ---------------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_eval_and_zero_are_the_legacy_layer(dtype):
    """set_training(0), and create_ex with all-zero probabilities, give a
    forward bit-identical to a legacy-created layer."""
    from oobleck_amd._ext import ObDropoutDesc
    from oobleck_amd.layer import Layer
    mc, oc = cfgs(TINY64)
    B, S, H = 2, 96, oc.n_embd
    flats = flats_for(oc)
    act = torch.float32 if dtype == "f32" else torch.bfloat16
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, oc.vocab_size, (B, S), generator=g).to(DEV)
    x = (torch.randn(B, S, H, generator=g) * 0.5).to(DEV).to(act)

    def fwd(layer, inp):
        out = torch.empty(B, S, H, device=DEV, dtype=act)
        layer.forward_slot(0, inp, out)
        torch.cuda.synchronize()
        return out

    for lid, inp in ((0, ids), (1, x)):
        legacy = Layer(lid, mc, B, S, 1, DEV, dtype=dtype)
        legacy.flat_param.copy_(flats[lid].to(DEV))
        legacy.refresh_weights()
        assert not legacy.has_dropout
        want = fwd(legacy, inp)
        assert torch.equal(fwd(legacy, inp), want), \
            "precondition: the legacy forward is run-to-run bit-stable"

        dropped = make_layer(mc, lid, flats[lid], B, S, 1, dtype=dtype)
        assert not torch.equal(fwd(dropped, inp), want)
        dropped.eval()
        assert torch.equal(fwd(dropped, inp), want)
        dropped.train()
        assert not torch.equal(fwd(dropped, inp), want)

        # create_ex with all-zero probabilities, straight through the C-ABI
        zero = Layer(lid, mc, B, S, 1, DEV, dtype=dtype)
        check(ext().ob_layer_destroy(zero._h), "destroy")
        h = ctypes.c_void_p()
        desc = ObDropoutDesc(0.0, 0.0, 0.0, lid, SEEDS[0])
        check(ext().ob_layer_create_ex(ctypes.byref(zero._desc),
                                       ctypes.byref(desc), ctypes.byref(h)),
              "create_ex")
        zero._h = h
        check(ext().ob_layer_bind(h, ptr(zero.flat_param),
                                  ptr(zero.flat_grad)), "bind")
        zero.flat_param.copy_(flats[lid].to(DEV))
        zero.refresh_weights()
        assert torch.equal(fwd(zero, inp), want)


@requires_gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_determinism_same_tick_same_output(dtype):
    mc, oc = cfgs(TINY64)
    B, S, H = 2, 96, oc.n_embd
    act = torch.float32 if dtype == "f32" else torch.bfloat16
    layer = make_layer(mc, 1, flats_for(oc)[1], B, S, dtype=dtype)
    x = (torch.randn(B, S, H, generator=torch.Generator().manual_seed(10))
         * 0.5).to(DEV).to(act)
    outs = []
    for slot, tick in ((0, 7), (1, 7), (0, 8)):
        out = torch.empty(B, S, H, device=DEV, dtype=act)
        layer.forward_slot(slot, x, out, tick=tick)
        outs.append(out)
    # no tick given: continues from the last one (8 -> 9)
    out = torch.empty(B, S, H, device=DEV, dtype=act)
    layer.forward_slot(0, x, out)
    out9 = torch.empty(B, S, H, device=DEV, dtype=act)
    layer.forward_slot(1, x, out9, tick=9)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])      # same tick, another slot
    assert not torch.equal(outs[0], outs[2])  # another tick
    assert torch.equal(out, out9)             # post-increment


# ---------------------------------------------------------------------------
# 8. pp1 pipeline, overlap on / off
# ---------------------------------------------------------------------------

PP_DIMS = dict(n_embd=128, n_head=2, n_layer=2, n_positions=128,
               vocab_size=307)
PP_B, PP_S, PP_MB = 2, 128, 4


def _run_pp1_dropout(rank: int, tmp: str, overlap: str, dtype: str):
    if str(REPO_ROOT) not in sys.path:
        sys.path.insert(0, str(REPO_ROOT))
    os.environ["OB_PP1_OVERLAP"] = overlap
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{tmp}/rdzv{overlap}",
                            rank=0, world_size=1)
    torch.cuda.set_device(0)
    from oobleck_amd.config import ModelConfig, TrainingConfig
    from oobleck_amd.engine import DataParallelEngine, make_rank_grid
    from oobleck_amd.layer import Layer
    from oobleck_amd.optimizer import FusedAdamW, WarmupLR
    from oobleck_amd.pipeline import OobleckPipeline

    dev = torch.device("cuda", 0)
    mc = ModelConfig(**PP_DIMS, embd_pdrop=0.1, resid_pdrop=0.1,
                     attn_pdrop=0.1)
    oc = OracleConfig(**PP_DIMS)
    tc = TrainingConfig(microbatch_size=PP_B,
                        global_microbatch_size=PP_B * PP_MB, seq_len=PP_S,
                        lr=1e-3, dropout_seed=SEEDS[0])
    L = oc.n_layers_total
    flats = flats_for(oc)
    grid = make_rank_grid(L, [list(range(L))], [[0]])

    class Loader:
        def __iter__(self):
            g = torch.Generator().manual_seed(31)
            while True:
                ids = torch.randint(0, oc.vocab_size, (PP_B, PP_S),
                                    generator=g)
                yield {"input_ids": ids, "labels": ids.clone()}

    pipe = OobleckPipeline(0, grid, mc, tc, Loader(), PP_MB, dev)
    pipe.initialize_distributed_fsdp()
    pipe.initialize_distributed_pipeline()

    def layer_factory(lid, pg, n_slots):
        layer = Layer(lid, mc, PP_B, PP_S, n_slots, dev, dtype=dtype,
                      dropout_seed=pipe.dropout_seed)
        layer.flat_param.copy_(flats[lid].to(dev))
        layer.refresh_weights()
        return layer

    def optimizer_factory(layers):
        opt = FusedAdamW(layers, lr=tc.lr)
        return opt, WarmupLR(opt, 0)

    pipe.initialize_execution(layer_factory, optimizer_factory)
    assert pipe.execution._overlap == (overlap == "1")
    assert all(l.has_dropout for l in pipe.execution._layers[:-1])
    dp = DataParallelEngine([pipe])
    totals = []
    for _ in range(2):
        pipe.train()
        dp.do_allreduce(pipe)
        pipe.execution.optimizer_step()
        for layer in pipe.execution._layers:
            layer.zero_grads()
        torch.cuda.synchronize()
        totals.append(pipe.execution.total_loss.item())
    with open(f"{tmp}/loss{overlap}.json", "w") as f:
        json.dump([totals[0], totals[1] - totals[0]], f)
    dist.destroy_process_group()


@requires_gpu
@pytest.mark.parametrize("dtype", ["bf16"])
def test_pp1_pipeline_dropout_overlap_on_off(dtype, tmp_path):
    """Two training steps with all p = 0.1 through OobleckPipeline.train(),
    with and without the forward/backward stream overlap: the masks are a
    function of (step, microbatch) and the forward's dropout scratch is its
    own, so both runs compute the same losses."""
    losses = {}
    for overlap in ("1", "0"):
        mp.spawn(_run_pp1_dropout, args=(str(tmp_path), overlap, dtype),
                 nprocs=1, join=True)
        losses[overlap] = json.loads(
            (tmp_path / f"loss{overlap}.json").read_text())
    print("pp1 dropout losses (step1, step2):", losses)
    a, b = losses["1"], losses["0"]
    assert abs(a[0] - b[0]) <= 1e-6 * abs(b[0]), (a, b)
    ltol = 1e-4 if dtype == "f32" else 2e-2
    assert abs(a[1] - b[1]) < ltol * abs(b[1]), (a, b)
    # dropout is on: the summed loss differs from the dropout-free model's
    assert a[0] > 0 and a[1] > 0
