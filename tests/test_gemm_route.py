# CPU: which kernel a bf16 GEMM call gets (oobleck_amd/csrc/ob_gemm_route.h),
# queried through the host-only entry that calls the very function
# ob_gemm_bf16 launches from.  The table pins the rule as it stood when the
# route became a function: every row was confirmed against the previous
# inline rule with its launches replaced by prints.
import ctypes

import pytest

GENERIC, GLDS, NT256, P8 = 0, 1, 2, 3
NO_LT, NO_GLDS, NO256 = 1, 2, 4


def _ext():
    from oobleck_amd._ext import get_ext
    try:
        return get_ext()
    except RuntimeError as e:
        pytest.fail(f"extension must build on CPU via hipcc: {e}")


def route(M, N, K, *, tA=0, tB=1, n1=1, n2=1, out_kind=0, splitk=1, beta=0.0,
          aligned=1, env=0, force=None):
    """-> dict(lt, kernel, BN, edge, splitk)"""
    out = (ctypes.c_int32 * 5)(*([-7] * 5))
    rc = _ext().ob_gemm_bf16_route(tA, tB, M, N, K, n1, n2, out_kind, splitk,
                                   beta, aligned, env, force, out)
    assert rc == 0, _ext().ob_last_error()
    return dict(lt=bool(out[0]), kernel=out[1], BN=out[2], edge=bool(out[3]),
                splitk=out[4])


# (M, N, K), call keywords, lt_first, kernel, extra expectations.  NT,
# aligned, beta 0, splitk 1, bf16 out, unbatched unless said otherwise; where
# lt_first is set, kernel is the hand-written fallback.
TABLE = [
    ((8192, 2304, 768), {}, True, GLDS, {}),                 # qkv
    ((8192, 3072, 768), {}, True, GLDS, {}),                 # fc: 384 tiles, eff 0.75
    ((8192, 768, 768), {}, True, GLDS, {}),                  # attnproj
    ((8192, 768, 3072), {}, True, NT256, {"BN": 128}),       # mlpproj: 192 blocks vs 96
    ((8192, 50432, 768), {}, True, P8, {}),                  # lm_head: 6304 tiles, eff 0.985
    ((8192, 768, 50432), {}, True, NT256, {"BN": 128}),      # d_lnout
    ((4096, 4096, 4096), {}, True, P8, {}),                  # 256 tiles
    ((1024, 1024, 64), {"n1": 8, "n2": 12}, False, P8, {}),  # QK^T: 1536 tiles
    ((256, 384, 128), {}, False, GLDS, {}),
    ((128, 128, 32), {}, False, GENERIC, {"edge": False}),   # K < 64
    ((200, 136, 72), {}, False, GENERIC, {"edge": True}),
    ((128, 64, 128), {"tB": 0}, False, GENERIC, {"BN": 64, "edge": False}),
    # one input varied from 256 x 384 x 128
    ((256, 384, 128), {"tA": 1}, False, GENERIC, {}),
    ((256, 384, 128), {"aligned": 0}, False, GENERIC, {}),
    ((256, 384, 128), {"out_kind": 2, "splitk": 4}, False, GLDS, {"splitk": 4}),
]
FAST = [row for row in TABLE if row[3] != GENERIC]


def _pick_splitk(M, N, K):
    # ob_layer.hip's split-K choice for the weight-grad GEMMs
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    sk = 1
    while sk < 16 and tiles * sk < 512 and K // (sk * 2) >= 256:
        sk *= 2
    return sk


@pytest.mark.parametrize("shape,kw,lt,kernel,extra", TABLE)
def test_route_table(shape, kw, lt, kernel, extra):
    r = route(*shape, **kw)
    assert r["lt"] == lt and r["kernel"] == kernel, r
    for k, v in extra.items():
        assert r[k] == v, (k, r)


@pytest.mark.parametrize("shape,kw,lt,kernel,extra", FAST)
def test_no_glds_sends_fast_rows_to_generic(shape, kw, lt, kernel, extra):
    r = route(*shape, env=NO_GLDS, **kw)
    assert r["kernel"] == GENERIC and r["lt"] == lt, r


def test_no256_sends_nt256_rows_to_glds():
    for shape in [(8192, 768, 3072), (8192, 768, 50432)]:
        assert route(*shape)["kernel"] == NT256
        r = route(*shape, env=NO256)
        assert r["kernel"] == GLDS and r["lt"], r
    # the 8-phase rows do not depend on it
    assert route(8192, 50432, 768, env=NO256)["kernel"] == P8


@pytest.mark.parametrize("shape,kw,lt,kernel,extra", TABLE)
def test_no_lt_clears_lt_first_only(shape, kw, lt, kernel, extra):
    r = route(*shape, env=NO_LT, **kw)
    assert not r["lt"] and r["kernel"] == kernel, r


def test_lt_first_needs_a_plain_call():
    base = dict(M=8192, N=768, K=768)
    assert route(**base)["lt"]
    assert not route(**base, beta=1.0)["lt"]
    assert not route(**base, out_kind=1)["lt"]
    assert not route(**base, out_kind=2, splitk=2)["lt"]
    assert not route(1024, 1024, 768, n2=2)["lt"]
    assert not route(512, 511, 768)["lt"]     # M * N < 512 * 512
    assert route(512, 512, 768)["lt"]
    assert route(8192, 768, 768, tA=1, tB=0)["lt"]  # any transposes


@pytest.mark.parametrize("force,kernel,BN", [
    (b"glds", GLDS, 128), (b"n128", NT256, 128), (b"n256", NT256, 256),
    (b"8ph", P8, 256)])
def test_force_applies_to_nt_only(force, kernel, BN):
    r = route(256, 256, 1024, force=force)
    assert (r["kernel"], r["BN"], r["lt"]) == (kernel, BN, False), r
    # forced before hipBLASLt is considered
    assert not route(8192, 768, 768, force=force)["lt"]
    for tA, tB in [(0, 0), (1, 0), (1, 1)]:
        assert route(256, 384, 128, tA=tA, tB=tB, force=force) == \
            route(256, 384, 128, tA=tA, tB=tB)
    assert route(8192, 768, 768, tA=1, tB=0, force=force)["lt"]


def test_unknown_force_is_ignored():
    assert route(8192, 768, 3072, force=b"x") == route(8192, 768, 3072)


# dw_bf16_ws's fallback for GPT-2 small (H = 768) at BS = 8192: NT on the
# transposed operands, M = act width, N = dY width, K = BS, atomic fp32 out
@pytest.mark.parametrize("M,N,sk,kernel,BN", [
    (3072, 768, 4, GLDS, 128),    # w_mlpproj: 144 256-tiles < 192
    (768, 3072, 4, GLDS, 128),    # w_fc
    (768, 768, 16, GLDS, 128),    # w_attnproj: 144 tiles even at sk 16
    (768, 2304, 8, NT256, 256),   # w_qkv: 216 blocks; BN=256 wins the tie
])
def test_dw_fallback_routes(M, N, sk, kernel, BN):
    assert _pick_splitk(M, N, 8192) == sk
    r = route(M, N, 8192, out_kind=2, splitk=sk)
    assert r == dict(lt=False, kernel=kernel, BN=BN, edge=False, splitk=sk), r


def test_nt256_bn_tie_goes_to_256():
    # 768 x 2304, sk 8: 216 vs 432 blocks, both eff 0.84375 -> 256
    assert route(768, 2304, 8192, out_kind=2, splitk=8)["BN"] == 256
    # 2048 x 512, 4 batches: BN=128 is the better fill (128 blocks, eff 0.5,
    # against 64, eff 0.25) but sits below the 192 floor -> glds
    assert route(2048, 512, 1024, n1=4)["kernel"] == GLDS


def test_thresholds():
    # 8-phase: tiles >= 192 and round efficiency >= 0.9
    assert route(256 * 16, 256 * 16, 768)["kernel"] == P8        # 256 tiles
    assert route(256 * 16, 256 * 15, 768)["kernel"] == P8        # 240: 0.9375
    assert route(256 * 16, 256 * 14, 768)["kernel"] == GLDS      # 224: 0.875
    assert route(256 * 16, 256 * 11, 768)["kernel"] == GLDS      # 176 < 192
    # fast path needs K >= 64; nt256 needs K >= 1024
    assert route(256, 384, 64)["kernel"] == GLDS
    assert route(256, 384, 32)["kernel"] == GENERIC
    assert route(8192, 768, 960)["kernel"] == GLDS
    assert route(8192, 768, 1024)["kernel"] == NT256
    # splitk < 1 is clamped
    assert route(256, 384, 128, splitk=0)["splitk"] == 1


def test_bad_arguments():
    out = (ctypes.c_int32 * 5)()
    ext = _ext()
    assert ext.ob_gemm_bf16_route(0, 1, 0, 128, 128, 1, 1, 0, 1, 0.0, 1, 0,
                                  None, out) != 0
    assert ext.ob_gemm_bf16_route(0, 1, 128, 128, 128, 1, 1, 0, 1, 0.0, 1, 0,
                                  None, None) != 0
