# CPU: the rule that says which weight-grad GEMMs may be cut along K and into
# how many slices (oobleck_amd/csrc/ob_dw_slices.h),
# through the host query ob_dw_slices_admit.  No GPU call.
import pytest

from oobleck_amd._ext import dw_slices_admit

CUS = 256                      # MI355X
H, BS, V_PAD = 768, 8192, 50432
SLAB = 2 * H * BS              # WS_DW_A of a GPT-2 small BLOCK, in floats
ALL_S = (2, 4, 8, 16)


def dw(M, N, K, lda=None, ldc=None):
    """The layer's weight-grad shape (ob_lt_dw): TN, fp32 out, beta = 1."""
    return (1, 0, M, N, K, lda or M, N, ldc or N, 1, 1, 0, 0, 0)


def admitted(shape, cus=CUS, slab=SLAB):
    return [s for s in ALL_S if dw_slices_admit(shape, s, cus, slab)]


@pytest.mark.parametrize("name,M,N,want", [
    ("dW_fc", H, 4 * H, [2, 4]),        # 144 tiles; 8 slabs do not fit
    ("dW_mlpproj", 4 * H, H, [2, 4]),
    ("dW_qkv", H, 3 * H, [2, 4]),       # 108 tiles; 8 slabs do not fit
    ("dW_attnproj", H, H, [2, 4, 8]),   # 36 tiles; 16 slices are 512 deep
])
def test_block_shapes(name, M, N, want):
    assert admitted(dw(M, N, BS)) == want, name


def test_dw_lm_stays_out():
    # 393 x 6 = 2358 tiles fill the device many times over
    assert admitted(dw(50257, H, BS, lda=V_PAD), slab=1 << 40) == []


@pytest.mark.parametrize("B_S", [256, 512])
def test_small_test_layers_stay_unsliced(B_S):
    # the H = 128 layers of the existing tests (B * S = 256: the flash A/B
    # layers, which compare weight grads bit for bit between processes)
    for N in (128, 384, 512):
        assert admitted(dw(128, N, B_S), slab=1 << 40) == []
    assert admitted(dw(512, 128, B_S), slab=1 << 40) == []


def test_whole_layer_case_of_the_gpu_test():
    # H = 128, B * S = 2048: two slices of 1024 rows, nothing finer
    assert admitted(dw(128, 512, 2048), slab=2 * 128 * 2048) == [2]


def test_k_must_divide_into_whole_256_steps():
    assert admitted(dw(H, H, 8200)) == []            # 8200 / 2 = 4100
    assert admitted(dw(H, H, 9216)) == [2, 4]        # / 8 = 1152 = 4.5 * 256
    assert admitted(dw(H, H, 8192 + 8)) == []


def test_short_slices():
    assert admitted(dw(H, H, 2048)) == [2]           # / 4 = 512 < 1024
    assert admitted(dw(H, H, 1024)) == []
    assert admitted(dw(H, H, 16384)) == [2, 4, 8, 16]


def test_small_slab():
    n = H * H
    assert admitted(dw(H, H, BS), slab=2 * n - 1) == []
    assert admitted(dw(H, H, BS), slab=2 * n) == [2]
    assert admitted(dw(H, H, BS), slab=4 * n) == [2, 4]
    assert admitted(dw(H, H, BS), slab=0) == []


def test_ldc_must_be_dense():
    assert admitted(dw(H, H, BS, ldc=H + 8)) == []
    assert admitted(dw(H, H, BS, lda=H + 8)) == [2, 4, 8]   # lda is free


def test_tiles_against_cus():
    # 16 x 16 tiles = 256: not fewer than the CUs; 15 x 16 = 240 is
    assert admitted(dw(2048, 2048, BS), slab=1 << 40) == []
    assert admitted(dw(1920, 2048, BS), slab=1 << 40) == [2, 4, 8]
    assert admitted(dw(H, H, BS), cus=36) == []
    assert admitted(dw(H, H, BS), cus=37) == [2, 4, 8]
    assert admitted(dw(H, H, BS), cus=0) == []       # device not asked
    # edge tiles count: 129 x 129 is 4 tiles
    assert admitted(dw(129, 129, BS), cus=4, slab=1 << 40) == []
    assert admitted(dw(129, 129, BS), cus=5, slab=1 << 40) == [2, 4, 8]


@pytest.mark.parametrize("field,value", [
    (0, 0),    # not transposed A
    (1, 1),    # transposed B
    (8, 0),    # bf16 out
    (9, 0),    # beta = 0
    (10, 1),   # bias epilogue
    (11, 1),   # separate C-input
    (12, 1),   # fp32 operands
])
def test_only_the_plain_tn_beta1_form(field, value):
    s = list(dw(H, H, BS))
    s[field] = value
    assert admitted(tuple(s)) == []


def test_other_slice_counts():
    for s in (-2, 0, 1, 3, 6, 32):
        assert not dw_slices_admit(dw(H, H, 1 << 16), s, CUS, 1 << 40)
