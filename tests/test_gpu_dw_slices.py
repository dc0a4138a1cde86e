# @gpu: the sliced weight-grad call (ob_blaslt.hip)
# through ob_gemm_lt_dw_sliced, which takes the slice count explicitly:
# C[M,N] += A[K,M]^T B[K,N] as s K-slices of one strided-batched library
# matmul into a slab, folded into C by k_dw_fold.
#
# Bounds.  (a): the reference is the float64 product of the same bf16
# operands plus the prefill; the sliced call's rel-L2 error may be at most
# twice that of the unsliced library call on the same inputs (both sum the
# same exact products in fp32, in another order).  Set OB_DW_SLICES_ERRORS to
# a path and (a) appends both errors there as JSON lines
# (profiles/dw_slices_table.json holds a recorded set).
import ctypes
import json
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
f32 = ctypes.c_float
# (M, N, K, s, lda): ragged tiles with a padded A; one tile; attnproj's shape
CASES = [(192, 320, 2048, 2, 256), (128, 128, 4096, 4, 128),
         (768, 768, 8192, 8, 768)]


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() /
            b.double().norm().clamp_min(1e-300)).item()


def _ext():
    from oobleck_amd._ext import get_ext
    return get_ext()


def operands(M, N, K, lda, seed=0):
    """bf16 A [K, lda] (pad columns hold values no correct layout reads),
    bf16 B [K, N] and a random fp32 prefill."""
    g = torch.Generator().manual_seed(100 + seed)
    A = torch.randn(K, lda, generator=g).to(DEV).bfloat16()
    B = torch.randn(K, N, generator=g).to(DEV).bfloat16()
    C0 = torch.randn(M, N, generator=g).to(DEV)
    return A, B, C0


def product64(A, B, M):
    return A[:, :M].double().T @ B.double()


def sliced(A, B, C, s, slab, lda=None):
    """One ob_gemm_lt_dw_sliced call into C; returns the slice count that
    ran."""
    K, N = B.shape
    M = C.shape[0]
    used = ctypes.c_int32(-1)
    rc = _ext().ob_gemm_lt_dw_sliced(M, N, K, ptr(A), lda or A.shape[1],
                                     ptr(B), N, ptr(C), N, s, ptr(slab),
                                     slab.numel() if slab is not None else 0,
                                     stream(), ctypes.byref(used))
    assert rc == 0, (rc, _ext().ob_last_error())
    return used.value


def unsliced(A, B, C, lda=None):
    K, N = B.shape
    M = C.shape[0]
    rc = _ext().ob_gemm_lt(1, 0, M, N, K, f32(1), ptr(A), lda or A.shape[1],
                           ptr(B), N, f32(1), ptr(C), N, 1, stream())
    assert rc == 0, (rc, _ext().ob_last_error())


def nan_slab(n):
    return torch.full((n,), float("nan"), device=DEV)


@requires_gpu
@pytest.mark.parametrize("M,N,K,s,lda", CASES)
def test_accuracy_against_the_unsliced_call(M, N, K, s, lda):
    A, B, C0 = operands(M, N, K, lda)
    ref = C0.double() + product64(A, B, M)
    Cs, Cu = C0.clone(), C0.clone()
    assert sliced(A, B, Cs, s, nan_slab(s * M * N), lda) == s
    unsliced(A, B, Cu, lda)
    torch.cuda.synchronize()
    es, eu = rel_l2(Cs, ref), rel_l2(Cu, ref)
    print(f"dW ({M},{N},{K}) lda {lda}: rel-L2 vs float64, {s} slices "
          f"{es:.3e}, unsliced {eu:.3e}")
    path = os.environ.get("OB_DW_SLICES_ERRORS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"M": M, "N": N, "K": K, "slices": s,
                                "lda": lda, "rel_l2_sliced": es,
                                "rel_l2_unsliced": eu}) + "\n")
    assert es <= 2 * eu, (es, eu)


@requires_gpu
def test_two_calls_accumulate_twice():
    M, N, K, s, lda = CASES[0]
    A, B, C0 = operands(M, N, K, lda)
    ref = C0.double() + 2 * product64(A, B, M)
    Cs, Cu = C0.clone(), C0.clone()
    slab = nan_slab(s * M * N)
    for _ in range(2):
        assert sliced(A, B, Cs, s, slab, lda) == s
        unsliced(A, B, Cu, lda)
    torch.cuda.synchronize()
    es, eu = rel_l2(Cs, ref), rel_l2(Cu, ref)
    print(f"two calls: rel-L2 sliced {es:.3e}, unsliced {eu:.3e}")
    assert es <= 2 * eu, (es, eu)


@requires_gpu
def test_slab_reuse_leaks_nothing():
    """Shape A (4 slices), a smaller shape B (2 slices), A again, one slab,
    one stream: each result is correct, so nothing a former call left in the
    slab (NaN at first) reaches the grads."""
    Ma, Na, Ka, sa = 128, 128, 4096, 4
    Mb, Nb, Kb, sb = 64, 96, 2048, 2
    slab = nan_slab(sa * Ma * Na)
    Aa, Ba, Ca0 = operands(Ma, Na, Ka, Ma, seed=1)
    Ab, Bb, Cb0 = operands(Mb, Nb, Kb, Mb, seed=2)
    refa = Ca0.double() + product64(Aa, Ba, Ma)
    refb = Cb0.double() + product64(Ab, Bb, Mb)
    Ca1, Cb, Ca2, Cua, Cub = (Ca0.clone(), Cb0.clone(), Ca0.clone(),
                              Ca0.clone(), Cb0.clone())
    assert sliced(Aa, Ba, Ca1, sa, slab) == sa
    assert sliced(Ab, Bb, Cb, sb, slab) == sb
    assert sliced(Aa, Ba, Ca2, sa, slab) == sa
    unsliced(Aa, Ba, Cua)
    unsliced(Ab, Bb, Cub)
    torch.cuda.synchronize()
    assert rel_l2(Ca1, refa) <= 2 * rel_l2(Cua, refa)
    assert rel_l2(Cb, refb) <= 2 * rel_l2(Cub, refb)
    assert torch.equal(Ca1, Ca2)


@requires_gpu
def test_repeatable_bit_for_bit():
    M, N, K, s, lda = CASES[1]
    A, B, C0 = operands(M, N, K, lda)
    slab = nan_slab(s * M * N)
    C1, C2 = C0.clone(), C0.clone()
    assert sliced(A, B, C1, s, slab) == s
    assert sliced(A, B, C2, s, slab) == s
    torch.cuda.synchronize()
    assert torch.equal(C1, C2)


@requires_gpu
@pytest.mark.parametrize("s,slab_floats", [
    (8, 8 * 128 * 128),    # slices of 512 rows: shorter than the rule's 1024
    (3, 4 * 128 * 128),    # not a slice count
    (4, 4 * 128 * 128 - 1),  # the slab is one float short
    (4, None),             # no slab
])
def test_inadmissible_slice_count_runs_unsliced(s, slab_floats):
    M, N, K, _, lda = CASES[1]
    A, B, C0 = operands(M, N, K, lda)
    ref = C0.double() + product64(A, B, M)
    slab = None if slab_floats is None else nan_slab(slab_floats)
    C, Cu = C0.clone(), C0.clone()
    assert sliced(A, B, C, s, slab) == 1
    unsliced(A, B, Cu)
    torch.cuda.synchronize()
    assert torch.equal(C, Cu)  # the same library call
    assert rel_l2(C, ref) < 1e-3
    if slab is not None:
        assert torch.isnan(slab).all()  # untouched


def _run_layer_child(tmp_path, flag):
    out = tmp_path / f"slices{flag}.pt"
    env = dict(os.environ, OB_DW_SLICES=flag)
    for k in ("OB_DETERMINISTIC", "OB_LT_TUNE", "OB_NO_BLASLT"):
        env.pop(k, None)  # each of them keeps every call unsliced
    child = pathlib.Path(__file__).resolve().parent / \
        "dw_slices_layer_child.py"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + \
          [str(child), str(out)]
    subprocess.run(cmd, check=True, env=env, timeout=300)
    return torch.load(out)


def _unsliced_error(M, N, K):
    """(a)'s yardstick at one shape: the unsliced library call's rel-L2 error
    against the float64 product of its bf16 operands plus the prefill."""
    A, B, C0 = operands(M, N, K, M, seed=3)
    ref = C0.double() + product64(A, B, M)
    C = C0.clone()
    unsliced(A, B, C)
    torch.cuda.synchronize()
    return rel_l2(C, ref)


@requires_gpu
def test_whole_layer_ab(tmp_path):
    """One BLOCK layer (H = 128, 2 heads, S = 1024, B = 2), backward in fresh
    processes with OB_DW_SLICES=2 and =1.  The layer's output and din are
    equal bit for bit.  The four weight grads ran as two slices in one
    process and unsliced in the other.

    Weight grads, the bound of (a).  (a) allows the sliced call twice the
    unsliced call's error e against the true product.  The layer does not
    expose the operands of its dW GEMMs, so the two processes' grads are
    compared with each other: one within e and the other within 2e of the
    same product lie within 3e of each other.  e is measured here as in (a),
    the unsliced library call against float64 at the grad's own M, N and
    K = B * S = 2048 (a few 1e-7), and the result is capped by the fp32
    reordering bound 2048 * 2^-24.

    DEPARTURE FROM THE ISSUE, which asks that all other outputs be bit-equal:
    the bias and LayerNorm grads are not asked to be.  They do not pass
    through the sliced call, but their kernels (the LayerNorm backward, the
    gelu / residual column sums, the flash backward's b_qkv sum) add the
    partial sums of the 16 row blocks of B * S = 2048 with fp32 atomics in
    arrival order, so two runs of ONE build already differ in the last bits.
    They get the reordering bound of an fp32 sum over 2048 rows, 2048 * 2^-24
    as rel-L2 (as the LayerNorm grads do in test_flash_nt_layer_ab, whose
    B * S = 256 leaves the bias sums two addends).  The control: each child
    runs its backward twice in one process; between those two runs din and
    the weight grads must be bit-equal in both arms, and the test prints
    which bias and LayerNorm segments differed (it does not assert that they
    differ: arrival order may also coincide)."""
    two = _run_layer_child(tmp_path, "2")
    one = _run_layer_child(tmp_path, "1")
    assert sorted(two["slices"].values()) == [2, 2, 2, 2], two["slices"]
    assert sorted(one["slices"].values()) == [1, 1, 1, 1], one["slices"]
    assert torch.equal(two["out"], one["out"])
    assert torch.equal(two["din"], one["din"])
    H, K = 128, 2048
    reorder = K * 2.0 ** -24
    segs = [("ln1_w", H), ("ln1_b", H), ("w_qkv", 3 * H * H),
            ("b_qkv", 3 * H), ("w_attnproj", H * H), ("b_attnproj", H),
            ("ln2_w", H), ("ln2_b", H), ("w_fc", 4 * H * H), ("b_fc", 4 * H),
            ("w_mlpproj", 4 * H * H), ("b_mlpproj", H)]
    dims = {"w_qkv": (H, 3 * H), "w_attnproj": (H, H), "w_fc": (H, 4 * H),
            "w_mlpproj": (4 * H, H)}
    g2, g1 = two["grad"], one["grad"]
    assert g2.numel() == g1.numel() == sum(n for _, n in segs)
    unstable = []
    for arm in (two, one):  # the same-arm control
        assert torch.equal(arm["din"], arm["din2"])
    o = 0
    for name, n in segs:
        a, b = g2[o:o + n], g1[o:o + n]
        e = rel_l2(a, b)
        same = [torch.equal(arm["grad"][o:o + n], arm["grad2"][o:o + n])
                for arm in (two, one)]
        o += n
        if name.startswith("w_"):
            assert all(same), (name, same)
            eu = _unsliced_error(*dims[name], K)
            bound = min(3 * eu, reorder)
            print(f"{name}: OB_DW_SLICES=2 vs 1 rel-L2 {e:.3e}, unsliced "
                  f"call vs float64 {eu:.3e}, bound {bound:.3e}")
            assert e <= bound, (name, e, bound)
        else:
            if not all(same):
                unstable.append(name)
            print(f"{name}: OB_DW_SLICES=2 vs 1 rel-L2 {e:.3e}")
            assert e <= reorder, (name, e)
    print("not bit-equal between two backward runs of one process:", unstable)
