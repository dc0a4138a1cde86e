# @gpu parity tests of the gradient-clipping C-ABI: ob_sqnorm_multi_f32,
# ob_clip_finish and ob_adamw_step_scaled, called directly through ctypes.
from __future__ import annotations

import ctypes
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

SQ_CHUNK = 16384  # elements per workgroup in ob_optim.hip
SIZES = [1, 3, 7, 4099, SQ_CHUNK - 1, SQ_CHUNK, SQ_CHUNK + 1, 2 ** 20 + 3]
EPS52 = 2.0 ** -52


def _ext():
    from oobleck_amd._ext import get_ext
    return get_ext()


def _check(rc, what):
    from oobleck_amd._ext import check
    check(rc, what)


def _vp(t: torch.Tensor) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr())


def _stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def sqnorm_multi(tensors, out, index=None):
    """ob_sqnorm_multi_f32 over `tensors` into the fp64 device vector `out`."""
    n = len(tensors)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors])
    counts = (ctypes.c_int64 * n)(*[t.numel() for t in tensors])
    idx = None if index is None else (ctypes.c_int32 * n)(*index)
    need = _ext().ob_sqnorm_ws_count(counts, n)
    assert need == sum(-(-t.numel() // SQ_CHUNK) for t in tensors)
    ws = torch.empty(max(1, need), dtype=torch.float64, device="cuda")
    _check(_ext().ob_sqnorm_multi_f32(ptrs, counts, idx, n, _vp(ws), _vp(out),
                                      _stream()), "sqnorm_multi")


def sqnorm_one(t: torch.Tensor) -> float:
    out = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
    sqnorm_multi([t], out)
    return out.item()


def clip_finish(sq, max_norm, stats):
    _check(_ext().ob_clip_finish(_vp(sq), sq.numel(), max_norm, _vp(stats),
                                 _stream()), "clip_finish")


def adamw_scaled(p, g, m, v, step, lr, wd, stats, b1=0.9, b2=0.999, eps=1e-8):
    _check(_ext().ob_adamw_step_scaled(_vp(p), _vp(g), _vp(m), _vp(v),
                                       p.numel(), step, lr, b1, b2, eps, wd,
                                       _vp(stats), _stream()), "adamw_scaled")


@functools.lru_cache(maxsize=None)
def _data(n: int, seed: int = 0):
    """(cpu tensor, fp64 CPU reference) — computed once, never modified."""
    g = torch.Generator().manual_seed(1000 + 7 * seed + n)
    x = torch.randn(n, generator=g) * 3e-2
    return x, (x.double() ** 2).sum().item()


@functools.lru_cache(maxsize=None)
def _gpu_sq(n: int, seed: int = 0) -> float:
    return sqnorm_one(_data(n, seed)[0].cuda())


@requires_gpu
@pytest.mark.parametrize("n", SIZES)
def test_sqnorm_parity(n):
    ref = _data(n)[1]
    got = _gpu_sq(n)
    rel = abs(got - ref) / ref
    print(f"n={n} got={got!r} ref={ref!r} rel={rel:.3e} bound={n * EPS52:.3e}")
    assert rel <= n * EPS52


@requires_gpu
@pytest.mark.parametrize("n", [7, 4099, SQ_CHUNK + 1, 2 ** 20 + 3])
def test_sqnorm_deterministic_and_alignment_independent(n):
    x = _data(n)[0]
    aligned = x.cuda()
    assert aligned.data_ptr() % 16 == 0
    buf = torch.zeros(n + 8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    shifted = buf[1:n + 1]
    shifted.copy_(x)
    assert shifted.data_ptr() % 16 == 4
    a1, a2 = sqnorm_one(aligned), sqnorm_one(aligned)
    s = sqnorm_one(shifted)
    assert a1.hex() == a2.hex()
    assert s.hex() == a1.hex()
    assert a1.hex() == _gpu_sq(n).hex()


@requires_gpu
def test_sqnorm_multi_tensor_permuted_slots():
    # 70 tensors > one 64-entry launch table; mixed sizes, one empty, every
    # third one a float past a 16-byte boundary
    pool = SIZES[:-1] + [5, 1000, 40000, 3 * SQ_CHUNK + 1]
    sizes = [pool[i % len(pool)] for i in range(70)]
    sizes[13] = 0
    sizes[66] = 2 ** 20 + 3  # a many-chunk tensor in the second table
    tensors = []
    for i, n in enumerate(sizes):
        x = _data(n, seed=i)[0] if n else torch.empty(0)
        if i % 3 == 1 and n:
            buf = torch.zeros(n + 8, device="cuda")
            t = buf[1:n + 1]
            t.copy_(x)
        else:
            t = x.cuda()
        tensors.append(t)
    single = [_gpu_sq(n, seed=i) if n else 0.0 for i, n in enumerate(sizes)]
    for i, n in enumerate(sizes):
        if n:
            assert abs(single[i] - _data(n, seed=i)[1]) <= \
                n * EPS52 * _data(n, seed=i)[1]

    SENT = -7.5
    perm = torch.randperm(100, generator=torch.Generator().manual_seed(5))
    index = perm[:70].tolist()
    out = torch.full((100,), SENT, dtype=torch.float64, device="cuda")
    sqnorm_multi(tensors, out, index)
    got = out.cpu().tolist()
    for i, slot in enumerate(index):
        assert got[slot].hex() == single[i].hex(), (i, sizes[i])
    for slot in perm[70:].tolist():
        assert got[slot] == SENT

    # NULL out_index = identity
    out2 = torch.full((70,), SENT, dtype=torch.float64, device="cuda")
    sqnorm_multi(tensors, out2)
    assert [v.hex() for v in out2.cpu().tolist()] == [v.hex() for v in single]


def _expected_coef(sq_values, max_norm):
    tot = 0.0
    for s in sq_values:
        tot += s
    norm = math.sqrt(tot)
    mn = float(np.float32(max_norm))  # the ABI takes max_norm as fp32
    return tot, norm, float(np.float32(min(1.0, mn / (norm + 1e-6))))


@requires_gpu
def test_clip_finish_coef_and_skip_counter():
    vals = [0.25, 1.5, 2.0, 0.0, 3.25, 1e-9, 0.1]
    sq = torch.tensor(vals, dtype=torch.float64, device="cuda")
    stats = torch.zeros(4, dtype=torch.float64, device="cuda")
    for max_norm in (1.0, 0.05, 2.5):
        clip_finish(sq, max_norm, stats)
        tot, norm, coef = _expected_coef(vals, max_norm)
        got = stats.cpu().tolist()
        assert got[0] == tot and got[1] == norm
        assert got[2] == coef and 0.0 < got[2] < 1.0
        assert got[3] == 0.0
    # under the threshold (and exactly at norm + 1e-6 <= max_norm): exactly 1
    for max_norm in (3.0, 1e4):
        clip_finish(sq, max_norm, stats)
        assert stats.cpu().tolist()[2:] == [1.0, 0.0]
    # non-finite anywhere in sq: skip marker, counter 0 -> 1 -> 2
    for k, bad in enumerate((float("inf"), float("nan")), start=1):
        sq_bad = sq.clone()
        sq_bad[2 + k] = bad
        clip_finish(sq_bad, 1.0, stats)
        got = stats.cpu().tolist()
        assert got[2] < 0.0, "skip marker is a negative coef"
        assert got[3] == float(k)
    # a finite step afterwards clears the marker and keeps the count
    clip_finish(sq, 1.0, stats)
    got = stats.cpu().tolist()
    assert got[2] == _expected_coef(vals, 1.0)[2] and got[3] == 2.0


ADAM_SIZES = (4099, 70001, 513)


@requires_gpu
@pytest.mark.parametrize("max_norm", [1.0, 0.05])
def test_scaled_adamw_matches_torch_clip_plus_adamw(max_norm):
    lr, wd = 1e-3, 0.01
    gen = torch.Generator().manual_seed(77)
    p0 = [torch.randn(n, generator=gen) * 0.1 for n in ADAM_SIZES]
    grads = [[torch.randn(n, generator=gen) * (1e-4 if step == 2 else 0.5)
              for n in ADAM_SIZES] for step in (1, 2, 3)]

    ref_p = [torch.nn.Parameter(p.clone()) for p in p0]
    opt = torch.optim.AdamW(ref_p, lr=lr, weight_decay=wd)

    p = [x.cuda() for x in p0]
    m = [torch.zeros_like(x) for x in p]
    v = [torch.zeros_like(x) for x in p]
    sq = torch.zeros(len(p), dtype=torch.float64, device="cuda")
    stats = torch.zeros(4, dtype=torch.float64, device="cuda")
    for step in (1, 2, 3):
        gs = grads[step - 1]
        for rp, g in zip(ref_p, gs):
            rp.grad = g.clone()
        ref_norm = torch.nn.utils.clip_grad_norm_(ref_p, max_norm).item()
        opt.step()

        gd = [g.cuda() for g in gs]
        sqnorm_multi(gd, sq)
        clip_finish(sq, max_norm, stats)
        for i in range(len(p)):
            adamw_scaled(p[i], gd[i], m[i], v[i], step, lr, wd, stats)
        st = stats.cpu().tolist()
        assert abs(st[1] - ref_norm) <= 1e-6 * ref_norm  # torch's is fp32
        if step == 2:
            assert st[2] == 1.0  # under the threshold: no clipping
        else:
            assert st[2] < 1.0
        for i in range(len(p)):
            # documented deviation: the clipped grad is not written back
            assert torch.equal(gd[i].cpu(), gs[i])
            torch.testing.assert_close(p[i].cpu(), ref_p[i].detach(),
                                       rtol=1e-5, atol=1e-6)
            state = opt.state[ref_p[i]]
            torch.testing.assert_close(m[i].cpu(), state["exp_avg"],
                                       rtol=1e-5, atol=1e-6)
            torch.testing.assert_close(v[i].cpu(), state["exp_avg_sq"],
                                       rtol=1e-5, atol=1e-6)


def _adam_state(n, seed):
    gen = torch.Generator().manual_seed(seed)
    p = (torch.randn(n, generator=gen) * 0.1).cuda()
    g = (torch.randn(n, generator=gen) * 0.5).cuda()
    m = (torch.randn(n, generator=gen) * 0.01).cuda()
    v = (torch.rand(n, generator=gen) * 1e-3).cuda()
    return p, g, m, v


@requires_gpu
def test_scaled_adamw_coef_one_is_bitwise_plain_adamw():
    from tests import gpu_helpers as gh
    p, g, m, v = _adam_state(70001, seed=3)
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    stats = torch.tensor([4.0, 2.0, 1.0, 0.0], dtype=torch.float64,
                         device="cuda")
    for step in (1, 2):
        gh.adamw(p, g, m, v, step, 1e-3, wd=0.01)
        adamw_scaled(p2, g, m2, v2, step, 1e-3, 0.01, stats)
    assert torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2)
    assert not torch.equal(p, _adam_state(70001, seed=3)[0])  # it did step


@requires_gpu
def test_scaled_adamw_skips_on_nonfinite_gradient():
    p, g, m, v = _adam_state(4099, seed=9)
    g[1234] = float("inf")  # ordinary data, not a fault
    p0, m0, v0 = p.clone(), m.clone(), v.clone()
    sq = torch.zeros(1, dtype=torch.float64, device="cuda")
    stats = torch.zeros(4, dtype=torch.float64, device="cuda")
    sqnorm_multi([g], sq)
    assert sq.item() == float("inf")
    clip_finish(sq, 1.0, stats)
    adamw_scaled(p, g, m, v, 1, 1e-3, 0.01, stats)
    st = stats.cpu().tolist()
    assert st[2] < 0.0 and st[3] == 1.0
    assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0)
