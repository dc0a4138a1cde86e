# @gpu tests of the deterministic-mode kernels: the
# fixed-order fold ob_colpart_finish_f32 (order pinned bit for bit against a
# numpy float32 restatement), and every _det producer entry: exact on integer
# data, within the worst-case summation bound of an fp64 reference on random
# data, bit-identical to its atomic sibling in everything but the sums, and
# repeatable.

import numpy as np
import pytest
import torch

from tests.gpu_helpers import ptr, stream

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
DEV = "cuda:0"
U = 2.0 ** -24  # fp32 unit roundoff


def _ext():
    from oobleck_amd._ext import check, get_ext
    return get_ext(), check


def _ws(which, M, N):
    """A slab of the size the entry asks for, NaN-filled: a finish that read
    an element its producer did not write in the same call would show."""
    n = _ext()[0].ob_det_ws_count(which, M, N)
    assert n > 0
    return torch.full((n,), float("nan"), device=DEV, dtype=torch.float32)


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _prefill(n):
    # non-zero integers: the entries ADD to dst
    return ((torch.arange(n) % 5) + 1).float().to(DEV)


# ---------------------------------------------------------------------------
# the fold's association, pinned
# ---------------------------------------------------------------------------

def fold_np(part):
    """The documented association of ob_colpart_finish_f32 in float32: group
    g (0..7) adds rows g, g + 8, ... in ascending order starting from row g;
    the group sums are added in ascending g starting from group 0's."""
    nblk = part.shape[0]
    groups = []
    for g in range(min(8, nblk)):
        s = part[g].copy()
        for b in range(g + 8, nblk, 8):
            s = (s + part[b]).astype(np.float32)
        groups.append(s)
    t = groups[0]
    for s in groups[1:]:
        t = (t + s).astype(np.float32)
    return t


@requires_gpu
@pytest.mark.parametrize("N", [8, 768, 3080])
@pytest.mark.parametrize("nblk", [1, 2, 7, 64, 512])
def test_colpart_finish_order(nblk, N):
    ext, check = _ext()
    rng = np.random.default_rng(1000 * nblk + N)
    ld = N + 8
    m = (1.0 + rng.random((nblk, N))).astype(np.float32)
    e = rng.integers(-10, 21, (nblk, N))
    sign = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), (nblk, N))
    vals = (sign * np.ldexp(m, e)).astype(np.float32)  # +-m * 2^e, exact
    dst0 = rng.standard_normal(N).astype(np.float32) + np.float32(3.0)
    want = (dst0 + fold_np(vals)).astype(np.float32)
    if nblk >= 7:
        # the data can tell block orders apart
        rev = (dst0 + fold_np(vals[::-1])).astype(np.float32)
        assert not np.array_equal(rev, want)
    slab = np.full((nblk, ld), np.nan, dtype=np.float32)  # pad never read
    slab[:, :N] = vals
    part = torch.from_numpy(slab).to(DEV)
    dst = torch.from_numpy(dst0.copy()).to(DEV)
    check(ext.ob_colpart_finish_f32(ptr(part), nblk, N, ld, ptr(dst),
                                    stream()), "colpart_finish")
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------
# thin callers
# ---------------------------------------------------------------------------

def colsum_det(X, db):
    ext, check = _ext()
    M, N = X.shape
    from oobleck_amd._ext import DET_WS_COLSUM
    check(ext.ob_colsum_det_bf16(ptr(X), ptr(db), M, N,
                                 ptr(_ws(DET_WS_COLSUM, M, N)), stream()),
          "colsum_det")


def gelu_det(u, dg, du, db):
    ext, check = _ext()
    M, N = u.shape
    from oobleck_amd._ext import DET_WS_GELU
    check(ext.ob_gelu_bwd_colsum_det_bf16(ptr(u), ptr(dg), ptr(du), ptr(db), M,
                                          N, ptr(_ws(DET_WS_GELU, M, N)),
                                          stream()), "gelu_det")


KEY = (1234, 3, 3, 7)  # seed, layer_id, site, tick


def drop_det(p, dy, dm, db):
    ext, check = _ext()
    M, N = dy.shape
    from oobleck_amd._ext import DET_WS_DROP_CS
    check(ext.ob_dropout_scale_colsum_det_bf16(
        *KEY, p, ptr(dy), ptr(dm), ptr(db), M, N,
        ptr(_ws(DET_WS_DROP_CS, M, N)), stream()), "drop_det")


def keep_mask(key, p, n):
    ext, check = _ext()
    keep = torch.empty(n, device=DEV, dtype=torch.uint8)
    check(ext.ob_dropout_mask(*key, p, n, ptr(keep), stream()), "mask")
    return keep


def ln_det(x, w, mean, rstd, dy, res, dx, dw, db, sres, sdx):
    ext, check = _ext()
    R, H = x.shape
    from oobleck_amd._ext import DET_WS_LN
    check(ext.ob_layernorm_bwd_res_det_bf16(
        ptr(x), ptr(w), ptr(mean), ptr(rstd), ptr(dy), ptr(res), ptr(dx),
        ptr(dw), ptr(db), ptr(sres), ptr(sdx), R, H,
        ptr(_ws(DET_WS_LN, R, H)), stream()), "ln_det")


# ---------------------------------------------------------------------------
# coverage on integer data: every order is exact, so the sums are known
# ---------------------------------------------------------------------------

MS = [1, 130, 257]  # straddle the 128-row tiles


@requires_gpu
@pytest.mark.parametrize("N", [128, 768, 3080, 1001])
@pytest.mark.parametrize("M", MS)
def test_colsum_det_exact(M, N):
    """1001: the scalar kernel (N % 8 != 0), 256-row tiles."""
    g = torch.Generator().manual_seed(M * 7 + N)
    X = _ints(g, (M, N), -8, 8).to(DEV).bfloat16()
    db = _prefill(N)
    want = db + X.float().sum(0)
    colsum_det(X, db)
    torch.cuda.synchronize()
    assert torch.equal(db, want)


@requires_gpu
@pytest.mark.parametrize("N", [128, 768, 3080])
@pytest.mark.parametrize("M", MS)
def test_gelu_det_exact(M, N):
    """u = 32: gelu'(u) is exactly 1, so du = dg and db = colsum(dg)."""
    g = torch.Generator().manual_seed(M * 11 + N)
    u = torch.full((M, N), 32.0, device=DEV).bfloat16()
    dg = _ints(g, (M, N), -8, 8).to(DEV).bfloat16()
    du = torch.empty_like(dg)
    db = _prefill(N)
    want = db + dg.float().sum(0)
    gelu_det(u, dg, du, db)
    torch.cuda.synchronize()
    assert torch.equal(du, dg)
    assert torch.equal(db, want)


@requires_gpu
@pytest.mark.parametrize("N", [128, 768, 3080, 1001])
@pytest.mark.parametrize("M", MS)
def test_drop_cs_det_exact(M, N):
    """p = 0.5: the factor is exactly 2.  1001: the any-width kernel."""
    g = torch.Generator().manual_seed(M * 13 + N)
    dy = _ints(g, (M, N), -8, 8).to(DEV).bfloat16()
    dm = torch.empty_like(dy)
    db = _prefill(N)
    keep = keep_mask(KEY, 0.5, M * N).view(M, N).float()
    want_dm = dy.float() * keep * 2.0
    want = db + want_dm.sum(0)
    drop_det(0.5, dy, dm, db)
    torch.cuda.synchronize()
    assert torch.equal(dm.float(), want_dm)
    assert torch.equal(db, want)


@requires_gpu
@pytest.mark.parametrize("sums", [True, False])
@pytest.mark.parametrize("H", [128, 768, 1600, 2176])
@pytest.mark.parametrize("rows", [33, 100, 530])
def test_ln_det_exact(rows, H, sums):
    """mean 0, rstd 1 and integer x, dy: dw = colsum(dy x), db = colsum(dy);
    w = 0 makes dx = res, so both side sums are colsum(res).  768: the wave
    kernel; 128 / 1600: 8 columns per thread, composed; 2176: 16 per thread.
    rows straddle the 16-row and 32-row blocks."""
    g = torch.Generator().manual_seed(rows * 17 + H)
    x = _ints(g, (rows, H), -4, 4).to(DEV).bfloat16()
    dy = _ints(g, (rows, H), -4, 4).to(DEV).bfloat16()
    res = _ints(g, (rows, H), -8, 8).to(DEV).bfloat16()
    w = torch.zeros(H, device=DEV)
    mean = torch.zeros(rows, device=DEV)
    rstd = torch.ones(rows, device=DEV)
    dx = torch.empty_like(x)
    dw, db, sres, sdx = (_prefill(H) for _ in range(4))
    pre = dw.clone()
    ln_det(x, w, mean, rstd, dy, res, dx, dw, db, sres if sums else None,
           sdx if sums else None)
    torch.cuda.synchronize()
    assert torch.equal(dx, res)
    assert torch.equal(dw, pre + (dy.float() * x.float()).sum(0))
    assert torch.equal(db, pre + dy.float().sum(0))
    if sums:
        assert torch.equal(sres, pre + res.float().sum(0))
        assert torch.equal(sdx, pre + res.float().sum(0))


EB, ES, EV = 2, 128, 304


def _embed_ids(case):
    g = torch.Generator().manual_seed(31)
    if case == "equal":
        return torch.full((EB, ES), 77, dtype=torch.int64)
    vals = torch.tensor([0, 5, 77, 150, EV - 1])  # leaders own long runs
    return vals[torch.randint(0, 5, (EB, ES), generator=g)]


@requires_gpu
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("H", [128, 768])
@pytest.mark.parametrize("case", ["five", "equal"])
def test_embed_bwd_det_exact(case, H, drop):
    ext, check = _ext()
    ids = _embed_ids(case).to(DEV)
    g = torch.Generator().manual_seed(H)
    dout = _ints(g, (EB, ES, H), -8, 8).to(DEV).bfloat16()
    dwte = _prefill(EV * H).view(EV, H).contiguous()
    dwpe = _prefill(ES * H).view(ES, H).contiguous()
    v = dout.float()
    if drop:
        key = (99, 0, 0, 5)
        v = v * keep_mask(key, 0.5, v.numel()).view_as(v).float() * 2.0
    want_te = dwte.clone().index_add_(0, ids.view(-1), v.view(-1, H))
    want_pe = dwpe + v.sum(0)
    if drop:
        check(ext.ob_embed_bwd_drop_det_bf16(*key, 0.5, ptr(ids), ptr(dout),
                                             ptr(dwte), ptr(dwpe), EB, ES, H,
                                             stream()), "embed_drop_det")
    else:
        check(ext.ob_embed_bwd_det_bf16(ptr(ids), ptr(dout), ptr(dwte),
                                        ptr(dwpe), EB, ES, H, stream()),
              "embed_det")
    torch.cuda.synchronize()
    assert torch.equal(dwte, want_te)
    assert torch.equal(dwpe, want_pe)


def _embed_call(drop_p, ids, dout, dwte, dwpe, H, key=(99, 0, 0, 5)):
    ext, check = _ext()
    if drop_p:
        check(ext.ob_embed_bwd_drop_det_bf16(*key, drop_p, ptr(ids), ptr(dout),
                                             ptr(dwte), ptr(dwpe), EB, ES, H,
                                             stream()), "embed_drop_det")
    else:
        check(ext.ob_embed_bwd_det_bf16(ptr(ids), ptr(dout), ptr(dwte),
                                        ptr(dwpe), EB, ES, H, stream()),
              "embed_det")


@requires_gpu
@pytest.mark.parametrize("drop_p", [0.0, 0.1])
@pytest.mark.parametrize("H", [128, 2176])
@pytest.mark.parametrize("case", ["five", "equal"])
def test_embed_bwd_det_random(case, H, drop_p):
    """Random dout against fp64 sums of the terms (dout, or fl32(dout *
    fl32(1 / (1 - p))) where kept: one fp32 multiply, the same in torch, so
    the terms are exact inputs of the summation).  A dwte row sums at most
    B*S terms, a dwpe row B: bound n * 2^-24 * sum|terms|.  p = 0.1: a
    factor that is no power of two.  2176 columns: a second column pass.
    Three launches bit-equal."""
    key = (99, 0, 0, 5)
    ids = _embed_ids(case).to(DEV)
    g = torch.Generator().manual_seed(H + 1)
    dout = torch.randn(EB, ES, H, generator=g).to(DEV).bfloat16()
    v = dout.float()
    if drop_p:
        one = torch.tensor(1.0, device=DEV)
        scale = one / (one - torch.tensor(drop_p, device=DEV))  # fp32
        keep = keep_mask(key, drop_p, v.numel()).view_as(v).float()
        v = (v * scale) * keep
    v = v.double()

    def run():
        dwte = torch.zeros(EV, H, device=DEV)
        dwpe = torch.zeros(ES, H, device=DEV)
        _embed_call(drop_p, ids, dout, dwte, dwpe, H, key)
        return dwte, dwpe
    dwte, dwpe = _three(run)
    flat = ids.view(-1)
    ref_te = torch.zeros(EV, H, device=DEV, dtype=torch.float64).index_add_(
        0, flat, v.view(-1, H))
    abs_te = torch.zeros(EV, H, device=DEV, dtype=torch.float64).index_add_(
        0, flat, v.view(-1, H).abs())
    assert bool(((dwte.double() - ref_te).abs() <= EB * ES * U * abs_te).all())
    assert bool(((dwpe.double() - v.sum(0)).abs()
                 <= EB * U * v.abs().sum(0)).all())
    assert bool((dwte[0] == 0).all()) if case == "equal" else True


# ---------------------------------------------------------------------------
# random data: an fp64 reference, the worst-case bound of ANY summation order
# (rows * 2^-24 * colsum|terms| per column: derived, not tuned), the atomic
# sibling's other outputs bit for bit, and three launches bit-equal
# ---------------------------------------------------------------------------

def _within(got, terms, extra=0):
    """got [N] against the fp64 column sums of terms [rows, N]; the terms
    are exact inputs of the summation unless `extra` roundings went into
    forming each of them (the bound is then (rows + extra) * 2^-24 *
    colsum|terms|)."""
    t = terms.double()
    bound = (t.shape[0] + extra) * U * t.abs().sum(0)
    err = (got.double() - t.sum(0)).abs()
    assert bool((err <= bound).all()), (err - bound).max().item()


def _three(run):
    outs = []
    for _ in range(3):
        outs.append(run())
    torch.cuda.synchronize()
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)
    return outs[0]


RAND_MN = [(257, 768), (130, 3080)]


@requires_gpu
@pytest.mark.parametrize("M,N", RAND_MN + [(300, 1001)])
def test_colsum_det_random(M, N):
    g = torch.Generator().manual_seed(M + N)
    X = torch.randn(M, N, generator=g).to(DEV).bfloat16()

    def run():
        db = torch.zeros(N, device=DEV)
        colsum_det(X, db)
        return (db,)
    (db,) = _three(run)
    _within(db, X)


@requires_gpu
@pytest.mark.parametrize("M,N", RAND_MN)
def test_gelu_det_random(M, N):
    ext, check = _ext()
    g = torch.Generator().manual_seed(M + N + 1)
    u = torch.randn(M, N, generator=g).to(DEV).bfloat16()
    dg = torch.randn(M, N, generator=g).to(DEV).bfloat16()

    def run():
        du = torch.empty_like(dg)
        db = torch.zeros(N, device=DEV)
        gelu_det(u, dg, du, db)
        return du, db
    du, db = _three(run)
    du_a = torch.empty_like(dg)
    db_a = torch.zeros(N, device=DEV)
    check(ext.ob_gelu_bwd_colsum_bf16(ptr(u), ptr(dg), ptr(du_a), ptr(db_a), M,
                                      N, stream()), "gelu")
    torch.cuda.synchronize()
    assert torch.equal(du, du_a)
    _within(db, du)  # the bf16-rounded du is what is summed


@requires_gpu
@pytest.mark.parametrize("M,N", RAND_MN + [(300, 1001)])
def test_drop_cs_det_random(M, N):
    ext, check = _ext()
    g = torch.Generator().manual_seed(M + N + 2)
    dy = torch.randn(M, N, generator=g).to(DEV).bfloat16()

    def run():
        dm = torch.empty_like(dy)
        db = torch.zeros(N, device=DEV)
        drop_det(0.1, dy, dm, db)
        return dm, db
    dm, db = _three(run)
    dm_a = torch.empty_like(dy)
    db_a = torch.zeros(N, device=DEV)
    check(ext.ob_dropout_scale_colsum_bf16(*KEY, 0.1, ptr(dy), ptr(dm_a),
                                           ptr(db_a), M, N, stream()), "drop")
    torch.cuda.synchronize()
    assert torch.equal(dm, dm_a)
    _within(db, dm)


@requires_gpu
@pytest.mark.parametrize("aliased", [False, True])
@pytest.mark.parametrize("R,H", [(100, 768), (530, 1600), (33, 2176)])
def test_ln_det_random(R, H, aliased):
    ext, check = _ext()
    g = torch.Generator().manual_seed(R + H)
    x = torch.randn(R, H, generator=g).to(DEV).bfloat16()
    dy = (torch.randn(R, H, generator=g) * 0.5).to(DEV).bfloat16()
    res = (torch.randn(R, H, generator=g) * 0.5).to(DEV).bfloat16()
    w = torch.randn(H, generator=g).to(DEV)
    xf = x.float()
    mean = xf.mean(-1).contiguous()
    rstd = (xf.var(-1, unbiased=False) + 1e-5).rsqrt().contiguous()

    def run():
        dx = res.clone() if aliased else torch.empty_like(x)
        outs = [torch.zeros(H, device=DEV) for _ in range(4)]
        ln_det(x, w, mean, rstd, dy, dx if aliased else res, dx, *outs)
        return [dx] + outs
    dx, dw, db, sres, sdx = _three(run)
    dx_a = res.clone() if aliased else torch.empty_like(x)
    outs_a = [torch.zeros(H, device=DEV) for _ in range(4)]
    check(ext.ob_layernorm_bwd_res_bf16(
        ptr(x), ptr(w), ptr(mean), ptr(rstd), ptr(dy),
        ptr(dx_a if aliased else res), ptr(dx_a), *(ptr(o) for o in outs_a),
        R, H, stream()), "ln")
    torch.cuda.synchronize()
    assert torch.equal(dx, dx_a)
    # the dw terms as the kernel forms them: xhat = (x - mean) * rstd in fp32
    # (two IEEE roundings, the same in torch), then dy * xhat, exact in fp64.
    # The kernel either fuses that product into the add (no further rounding)
    # or rounds it once first, which the one extra unit covers.
    xhat = (x.float() - mean[:, None]) * rstd[:, None]
    _within(dw, dy.double() * xhat.double(), extra=1)
    _within(db, dy)
    _within(sres, res)
    _within(sdx, dx)  # the bf16-rounded dx is what is summed


@requires_gpu
@pytest.mark.parametrize("B,S,V", [(2, 128, 304), (3, 65, 1001)])
def test_ce_fwd_det(B, S, V):
    """The loss is the fixed-order sum of the per-row terms the kernel left in
    the slab (0 for the last position of a sequence); lse is the sibling's."""
    ext, check = _ext()
    from oobleck_amd._ext import DET_WS_CE
    g = torch.Generator().manual_seed(V)
    ld = (V + 255) // 256 * 256
    logits = torch.zeros(B * S, ld)
    logits[:, :V] = torch.randn(B * S, V, generator=g) * 2
    logits = logits.to(DEV).bfloat16()
    labels = torch.randint(0, V, (B, S), generator=g).to(DEV)
    slabs = []

    def run():
        lse = torch.empty(B * S, device=DEV)
        loss = torch.zeros(1, device=DEV)
        ws = _ws(DET_WS_CE, B * S, 1)
        check(ext.ob_ce_fwd_det_bf16(ptr(logits), ptr(labels), ptr(lse),
                                     ptr(loss), B, S, V, ld, ptr(ws),
                                     stream()), "ce_det")
        slabs.append(ws)
        return lse, loss
    lse, loss = _three(run)
    lse_a = torch.empty(B * S, device=DEV)
    loss_a = torch.zeros(1, device=DEV)
    check(ext.ob_ce_fwd_bf16(ptr(logits), ptr(labels), ptr(lse_a), ptr(loss_a),
                             B, S, V, ld, stream()), "ce")
    torch.cuda.synchronize()
    assert torch.equal(lse, lse_a)
    terms = slabs[0].view(B, S)
    assert bool(torch.isfinite(terms).all())
    assert bool((terms[:, -1] == 0).all())
    _within(loss, terms.reshape(-1, 1))
    # and the terms are the shifted cross entropy
    lp = torch.log_softmax(logits[:, :V].double(), -1).view(B, S, V)
    ref = -lp[:, :-1].gather(-1, labels[:, 1:, None]).mean()
    # independent reference: the bf16 logits are exact inputs; the kernel's
    # hardware exp / log are good to a few fp32 ulps (~1e-6 relative on a
    # term), so 1e-4 leaves two orders of magnitude
    assert abs(loss.item() - ref.item()) < 1e-4 * abs(ref.item())
    assert abs(loss.item() - loss_a.item()) <= 2 * B * S * U * float(
        terms.abs().sum())
