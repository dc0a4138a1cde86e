# CPU: the library GEMM shapes of a layer (ob_layer_lt_shapes), the list
# ob_layer_create hands to the hipBLASLt tuner.  The forward and backward
# take their GEMM dimensions from the same list (ob_layer.hip block_gemms /
# final_gemms), so pinning it here pins the keys the step uses.
import pytest

EMBED, BLOCK, FINAL = 0, 1, 2
H, NH, S, B, V = 768, 12, 1024, 8, 50257
V_PAD = 50432  # V rounded up to 256
BS = B * S


def _desc(kind, *, dtype=1, n_embd=H, n_head=NH, seq=S, batch=B, vocab=V):
    from oobleck_amd._ext import ObLayerDesc
    return ObLayerDesc(kind=kind, n_embd=n_embd, n_head=n_head,
                       n_positions=seq, vocab_size=vocab, max_batch=batch,
                       seq_len=seq, n_slots=2, dtype=dtype)


def shapes(desc):
    from oobleck_amd._ext import LT_SHAPE_NAMES, layer_lt_shapes
    try:
        return [dict(zip(LT_SHAPE_NAMES, s)) for s in layer_lt_shapes(desc)]
    except RuntimeError as e:
        pytest.fail(f"extension must build on CPU via hipcc: {e}")


def nt(M, N, K, *, bias=0, res=0):
    """out[M,N] = in[M,K] W[N,K]^T (+ bias) (+ residual as the C-input)"""
    return dict(tA=0, tB=1, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, c_f32=0,
                beta1=res, bias=bias, cin=res, ab_f32=0)


def tn(M, N, K, *, lda=None):
    """gout[M,N] += act[K,M]^T dY[K,N], fp32, beta = 1"""
    return dict(tA=1, tB=0, M=M, N=N, K=K, lda=lda or M, ldb=N, ldc=N,
                c_f32=1, beta1=1, bias=0, cin=0, ab_f32=0)


def test_block_shapes():
    want = [
        nt(BS, 2304, 768, bias=1), nt(BS, 768, 768, bias=1, res=1),
        nt(BS, 3072, 768, bias=1), nt(BS, 768, 3072, bias=1, res=1),
        nt(BS, 3072, 768), nt(BS, 768, 3072), nt(BS, 768, 768),
        nt(BS, 768, 2304),
        tn(3072, 768, BS), tn(768, 3072, BS), tn(768, 768, BS),
        tn(768, 2304, BS),
    ]
    assert shapes(_desc(BLOCK)) == want


def test_final_shapes():
    want = [nt(BS, V_PAD, 768),          # lm_head, N = v_pad
            nt(BS, 768, V_PAD),          # d_lnout, K = v_pad
            tn(V, 768, BS, lda=V_PAD)]   # dW_lm, M = V over v_pad-wide rows
    assert shapes(_desc(FINAL)) == want


def test_no_shapes_for_embed_or_fp32():
    assert shapes(_desc(EMBED)) == []
    assert shapes(_desc(BLOCK, dtype=0)) == []
    assert shapes(_desc(FINAL, dtype=0)) == []


def test_small_layer_lists_only_library_routed_gemms():
    """The bf16 route rule offers a linear to the library from 512 x 512
    outputs up; a weight grad always goes there.  H = 128, B * S = 256: no
    linear qualifies in the block, the lm_head (256 x 1024) does."""
    blk = shapes(_desc(BLOCK, n_embd=128, n_head=2, seq=128, batch=2))
    assert blk == [tn(512, 128, 256), tn(128, 512, 256), tn(128, 128, 256),
                   tn(128, 384, 256)]
    fin = shapes(_desc(FINAL, n_embd=128, n_head=2, seq=128, batch=2,
                       vocab=1000))
    assert fin == [nt(256, 1024, 128), tn(1000, 128, 256, lda=1024)]


def test_cap_limits_what_is_written():
    import ctypes
    from oobleck_amd._ext import LT_SHAPE_FIELDS, get_ext
    d = _desc(BLOCK)
    buf = (ctypes.c_int64 * (LT_SHAPE_FIELDS * 3))(*([-7] * LT_SHAPE_FIELDS * 3))
    assert get_ext().ob_layer_lt_shapes(ctypes.byref(d), buf, 2) == 12
    assert buf[2 * LT_SHAPE_FIELDS] == -7
    assert list(buf[2:5]) == [BS, 2304, 768]
