# @gpu tests for the flash entry points that take no transposed copies
# (ob_flash_fwd_nt_bf16 / ob_flash_bwd_nt_bf16): the kernels read their
# column-major MFMA operands from the row-major LDS tiles with the gfx950
# transposed LDS read.  The MFMA order and operand values equal the older
# entry points', so outputs are compared bit for bit against them (every
# element: a swapped chunk or row of the LDS image cannot pass), and
# against torch fp32 references with the bounds of test_gpu_bf16.py.
import functools
import math
import os
import pathlib
import subprocess
import sys

import pytest
import torch

from tests.gpu_helpers import ptr, stream

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
DEV = "cuda:0"
SCALE = 1.0 / math.sqrt(64.0)
# (2,2,128): one q-block, diagonal tiles only; (1,3,256): odd head count
# (z -> (b,h) map) and both LDS buffers; (2,2,384): odd number of 128-row
# blocks, batch stride
SHAPES = [(2, 2, 128), (1, 3, 256), (2, 2, 384)]


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
    """Inputs, the old path's outputs (transposes + old kernels) and the
    torch fp32 references; computed once per shape, never modified."""
    ext = _ext()
    H = nh * 64
    g = torch.Generator().manual_seed(31)
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

    qf = qkv.float().requires_grad_(True)
    q = qf[..., :H].view(B, S, nh, 64).permute(0, 2, 1, 3)
    k = qf[..., H:2 * H].view(B, S, nh, 64).permute(0, 2, 1, 3)
    v = qf[..., 2 * H:].view(B, S, nh, 64).permute(0, 2, 1, 3)
    w = torch.matmul(q, k.transpose(-1, -2)) * SCALE
    mask = torch.tril(torch.ones(S, S, dtype=torch.bool, device=DEV))
    w = torch.where(mask, w, torch.tensor(float("-inf"), device=DEV))
    lse_ref = torch.logsumexp(w, dim=-1).detach()
    P = torch.softmax(w, dim=-1)
    O_ref = torch.matmul(P, v).permute(0, 2, 1, 3).reshape(B, S, H)
    O_ref.backward(dO.float())
    return dict(H=H, qkv=qkv, dO=dO, O=O, lse=lse, D=D, dqkv=dqkv,
                O_ref=O_ref.detach(), lse_ref=lse_ref, dqkv_ref=qf.grad)


def _bwd_nt(c, B, nh, S, dbias):
    dqkv = torch.empty_like(c["qkv"])
    _check(_ext().ob_flash_bwd_nt_bf16(
        ptr(c["qkv"]), ptr(c["dO"]), ptr(c["lse"]), ptr(c["D"]), ptr(dqkv),
        ptr(dbias), B, S, c["H"], nh, SCALE, stream()), "flash_bwd_nt")
    torch.cuda.synchronize()
    return dqkv


@requires_gpu
@pytest.mark.parametrize("B,nh,S", SHAPES)
def test_flash_fwd_nt(B, nh, S):
    c = _case(B, nh, S)
    H = c["H"]
    O = torch.empty(B, S, H, device=DEV, dtype=torch.bfloat16)
    lse = torch.empty(B * nh, S, device=DEV, dtype=torch.float32)
    _check(_ext().ob_flash_fwd_nt_bf16(ptr(c["qkv"]), ptr(O), ptr(lse), B, S,
                                       H, nh, SCALE, stream()),
           "flash_fwd_nt")
    torch.cuda.synchronize()
    assert torch.equal(O, c["O"])
    assert torch.equal(lse, c["lse"])
    err = rel_l2(O.float(), c["O_ref"])
    assert err < 2e-2, err
    torch.testing.assert_close(lse.view(B, nh, S), c["lse_ref"], rtol=1e-3,
                               atol=1e-3)


@requires_gpu
@pytest.mark.parametrize("B,nh,S", SHAPES)
def test_flash_bwd_nt(B, nh, S):
    c = _case(B, nh, S)
    H = c["H"]
    dqkv = _bwd_nt(c, B, nh, S, None)
    assert torch.equal(dqkv, c["dqkv"])
    for name, sl in (("dQ", slice(0, H)), ("dK", slice(H, 2 * H)),
                     ("dV", slice(2 * H, 3 * H))):
        e = rel_l2(dqkv[..., sl].float(), c["dqkv_ref"][..., sl])
        assert e < 3e-2, (name, e)


@requires_gpu
@pytest.mark.parametrize("B,nh,S", SHAPES)
def test_flash_bwd_nt_bias(B, nh, S):
    """dbias_qkv accumulates (known non-zero start) the column sums of the
    fp32 accumulators; dqkv itself is unchanged by it."""
    c = _case(B, nh, S)
    H = c["H"]
    start = torch.linspace(-1.0, 1.0, 3 * H, device=DEV)
    acc = start.clone()
    dqkv = _bwd_nt(c, B, nh, S, acc)
    assert torch.equal(dqkv, c["dqkv"])
    added = acc - start
    ref = c["dqkv_ref"].reshape(B * S, 3 * H).sum(0)
    e = rel_l2(added, ref)
    cs = torch.zeros(3 * H, device=DEV)
    _check(_ext().ob_colsum_bf16(ptr(dqkv), ptr(cs), B * S, 3 * H, stream()),
           "colsum")
    torch.cuda.synchronize()
    print(f"flash_bwd_nt bias ({B},{nh},{S}): rel-L2 vs fp32 autograd "
          f"{e:.3e}, vs ob_colsum_bf16(dqkv) {rel_l2(added, cs):.3e}")
    assert e < 3e-2, e


def _run_layer_child(tmp_path, flag):
    out = tmp_path / f"tr{flag}.pt"
    env = dict(os.environ, OB_FLASH_TR=flag)
    child = pathlib.Path(__file__).resolve().parent / "flash_nt_layer_child.py"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + \
          [str(child), str(out)]
    subprocess.run(cmd, check=True, env=env, timeout=300)
    return torch.load(out)


@requires_gpu
def test_flash_nt_layer_ab(tmp_path):
    """One BLOCK layer (S=128, H=128, nh=2), forward + backward in fresh
    processes with OB_FLASH_TR=1 and =0 (the switch is read once per
    process): output, din and every grad but b_qkv are equal; the b_qkv
    grad comes from fp32 accumulators instead of bf16-rounded DQKV.

    The four LayerNorm grads are the exception to "equal": their kernels
    add per-block partial sums with fp32 atomics in arrival order, so two
    runs of ONE build already differ in the last bits.  They get the
    reordering bound of an fp32 sum over the B*S = 256 rows, 256 * 2^-24,
    as rel-L2; every other segment must match bit for bit."""
    new = _run_layer_child(tmp_path, "1")
    old = _run_layer_child(tmp_path, "0")
    assert torch.equal(new["out"], old["out"])
    assert torch.equal(new["din"], old["din"])
    H = 128
    segs = [("ln1_w", H), ("ln1_b", H), ("w_qkv", 3 * H * H),
            ("b_qkv", 3 * H), ("w_attnproj", H * H), ("b_attnproj", H),
            ("ln2_w", H), ("ln2_b", H), ("w_fc", 4 * H * H), ("b_fc", 4 * H),
            ("w_mlpproj", 4 * H * H), ("b_mlpproj", H)]
    gn, go = new["grad"], old["grad"]
    assert gn.numel() == go.numel() == sum(n for _, n in segs)
    o = 0
    for name, n in segs:
        a, b = gn[o:o + n], go[o:o + n]
        o += n
        if name == "b_qkv":
            e = rel_l2(a, b)
            print(f"b_qkv grad rel-L2 OB_FLASH_TR=1 vs 0: {e:.3e}")
            assert e < 3e-2, e
        elif name.startswith("ln"):
            assert rel_l2(a, b) < 256 * 2.0 ** -24, (name, rel_l2(a, b))
        else:
            assert torch.equal(a, b), name
