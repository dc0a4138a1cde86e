# @gpu: the hipBLASLt solution choice (ob_blaslt.hip).
# Every case calls the ob_gemm_lt* entries directly: shapes this small do not
# route to the library through ob_gemm_bf16.  The computations live in
# tests/lt_tune_child.py, which also runs them in a child process under
# OB_LT_TUNE=0 (the switch is read once per process).
#
# Bounds.  Against the fp32 torch.matmul reference on the same bf16 inputs:
# the ones test_gpu_bf16.py uses for the same operations, rel-L2 2e-2 for a
# bf16 output and rtol = atol = 1e-3 for an fp32 one.  Tuned against
# untuned: both sum exact bf16 products in fp32 in another order, so one
# output ulp (2^-8) for bf16 and the project's fp32 reordering rtol 1e-3.
# Layers: the per-layer bf16 bounds, 1.5e-2 forward and 3e-2 grads.
import ctypes
import os
import pathlib
import subprocess
import sys

import pytest
import torch

from tests import lt_tune_child as lc

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
CASES = [(v, *s) for s in lc.SHAPES for v in lc.VARIANTS]


def rel_l2(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _ext():
    from oobleck_amd._ext import get_ext
    return get_ext()


def _choice(key):
    from oobleck_amd._ext import lt_choice
    return lt_choice(key)


def _tuning_on():
    return os.environ.get("OB_LT_TUNE", "1")[:1] != "0"


@pytest.fixture(scope="module")
def tuned():
    """The four variants on the three shapes in this process, each key tuned
    first."""
    return lc.run_gemms()


@pytest.fixture(scope="module")
def untuned(tmp_path_factory):
    """The same computations in a fresh process with OB_LT_TUNE=0."""
    out = tmp_path_factory.mktemp("lt") / "untuned.pt"
    child = pathlib.Path(lc.__file__).resolve()
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + \
          [str(child), str(out)]
    subprocess.run(cmd, check=True, env=dict(os.environ, OB_LT_TUNE="0"),
                   timeout=300)
    return torch.load(out)


@requires_gpu
@pytest.mark.parametrize("variant,M,N,K", CASES)
def test_variant_matches_reference(tuned, variant, M, N, K):
    ops = lc.operands(variant, M, N, K)
    res_before = ops[3].clone()
    got = tuned[(variant, M, N, K)]
    ref = lc.reference(variant, M, N, K, ops).cpu()
    if _tuning_on():
        c = _choice(lc.key(variant, M, N, K))
        assert c is not None and c["tried"] >= 1
    if variant == "tn_beta1":
        torch.testing.assert_close(got, ref, rtol=1e-3, atol=1e-3)
    else:
        assert rel_l2(got.float(), ref) < 2e-2
    if variant == "nt_bias_res":
        # C != C-input: the residual buffer comes back unchanged
        C = lc.run_gemm(variant, M, N, K, ops)
        torch.cuda.synchronize()
        assert torch.equal(ops[3], res_before)
        assert rel_l2(C.float().cpu(), ref) < 2e-2


@requires_gpu
@pytest.mark.parametrize("variant,M,N,K", CASES)
def test_tuned_against_untuned(tuned, untuned, variant, M, N, K):
    a = tuned[(variant, M, N, K)].float()
    b = untuned["gemms"][(variant, M, N, K)].float()
    e = rel_l2(a, b)
    print(f"{variant} ({M},{N},{K}): tuned vs OB_LT_TUNE=0 rel-L2 {e:.3e}")
    assert e <= (1e-3 if variant == "tn_beta1" else 2.0 ** -8)


@requires_gpu
def test_tuning_is_cached(tuned):
    k = lc.key("nt_bias", 256, 384, 128)
    first = _choice(k)
    if not _tuning_on():
        assert first is None  # OB_LT_TUNE=0: no table, top-1 plans
        return
    lc.tune(k)
    again = _choice(k)
    assert again == first  # same index, tried count and measured times
    assert first["tuned"] and first["index"] >= 0
    assert 1 <= first["tried"] <= 128
    assert first["us_chosen"] <= first["us_top1"]


@requires_gpu
def test_two_streams_run_the_same_solution(tuned):
    from oobleck_amd._ext import lt_shape
    v, M, N, K = "nt_bias_res", 256, 384, 128
    k = lc.key(v, M, N, K)
    ops = lc.operands(v, M, N, K)
    ref = lc.reference(v, M, N, K, ops).cpu()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    outs, idx = [], []
    for s in streams:
        sp = ctypes.c_void_p(s.cuda_stream)
        outs.append(lc.run_gemm(v, M, N, K, ops, strm=sp))
        idx.append(_ext().ob_gemm_lt_plan_index(lt_shape(*k), sp))
    torch.cuda.synchronize()
    assert idx[0] == idx[1] and idx[0] >= 0
    if _tuning_on():
        assert idx[0] == _choice(k)["index"]
    for C in outs:
        assert rel_l2(C.float().cpu(), ref) < 2e-2


@requires_gpu
@pytest.mark.parametrize("variant,pad", [("nt_bias", 64), ("tn_beta1", 8)])
def test_leading_dimension_is_part_of_the_key(tuned, variant, pad):
    """Equal M, N, K, another lda: each call gets the layout of its own lda
    (the plan cache once keyed on M, N, K and ldc alone)."""
    M, N, K = 256, 384, 128
    dense = lc.key(variant, M, N, K)[5]
    for lda in (dense, dense + pad):
        ops = lc.operands(variant, M, N, K, lda=lda)
        got = lc.run_gemm(variant, M, N, K, ops, lda=lda)
        torch.cuda.synchronize()
        ref = lc.reference(variant, M, N, K, ops)
        if variant == "tn_beta1":
            torch.testing.assert_close(got, ref, rtol=1e-3, atol=1e-3)
        else:
            assert rel_l2(got.float(), ref) < 2e-2, lda


@requires_gpu
def test_layers_tune_their_shapes(untuned):
    from oobleck_amd._ext import layer_lt_shapes
    ext = _ext()
    uses0 = ext.ob_gemm_lt_untuned_uses()
    got, (block, final) = lc.run_layers()
    listed = layer_lt_shapes(block._desc) + layer_lt_shapes(final._desc)
    assert len(listed) == 4 + 2
    if _tuning_on():
        # as many tuned keys as listed shapes (a layer of the same
        # dimensions may have tuned some of them earlier in this process)
        assert len(set(listed)) == len(listed)
        assert sum(_choice(s) is not None for s in listed) == len(listed)
        assert ext.ob_gemm_lt_table_size() >= len(listed)
    else:
        assert ext.ob_gemm_lt_table_size() == 0
    # every library GEMM of the forward + backward found its shape tuned
    assert ext.ob_gemm_lt_untuned_uses() - uses0 == 0
    want = untuned["layers"]
    e = {k: rel_l2(got[k], want[k]) for k in got}
    print("layers, tuned vs OB_LT_TUNE=0 rel-L2:", e)
    assert e["block_out"] < 1.5e-2 and e["final_loss"] < 1.5e-2
    for k in ("block_din", "block_grad", "final_din", "final_grad"):
        assert e[k] < 3e-2, (k, e[k])
