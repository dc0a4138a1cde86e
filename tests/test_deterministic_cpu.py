# Deterministic mode, host side (no GPU): the exported symbols, the config
# default, the slab-size query against the grid arithmetic of the kernels it
# sizes, and the environment default of the process-wide switch.
import os
import pathlib
import re
import subprocess
import sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent

DET_SYMBOLS = [
    "ob_set_deterministic", "ob_deterministic", "ob_det_ws_count",
    "ob_colsum_det_bf16", "ob_gelu_bwd_colsum_det_bf16",
    "ob_layernorm_bwd_res_det_bf16", "ob_dropout_scale_colsum_det_bf16",
    "ob_ce_fwd_det_bf16", "ob_embed_bwd_det_bf16",
    "ob_embed_bwd_drop_det_bf16", "ob_colpart_finish_f32",
]


def _lib():
    from oobleck_amd._ext import get_ext
    return get_ext()


def test_header_symbols_exported():
    header = (ROOT / "include" / "oobleck_stage.h").read_text()
    lib = _lib()
    for name in DET_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), f"{name} not in header"
        assert hasattr(lib, name), f"{name} not exported"
        assert getattr(lib, name).argtypes is not None, f"{name}: no argtypes"


def test_training_config_default():
    from oobleck_amd import TrainingConfig, set_deterministic
    assert TrainingConfig().deterministic is False
    assert TrainingConfig(deterministic=True).deterministic is True
    assert callable(set_deterministic)


def _cdiv(a, b):
    return (a + b - 1) // b


@pytest.mark.parametrize("M,N", [(1, 8), (130, 768), (257, 3080), (8192, 768),
                                 (8192, 3072), (16384, 4096), (300, 1001)])
def test_ws_count_is_grid_arithmetic(M, N):
    """One slab row per block row of the producer's grid: 128-row tiles for
    the vector colsum, gelu and dropout kernels, 256 for the scalar colsum
    (N % 8 != 0); the wave LayerNorm (512..1024 columns) has min(ceil(M / 32),
    1024) blocks and four vectors, the block-per-16-rows kernel two."""
    from oobleck_amd import _ext
    lib = _lib()
    cs = _cdiv(M, 128) * N if N % 8 == 0 else _cdiv(M, 256) * N
    assert lib.ob_det_ws_count(_ext.DET_WS_COLSUM, M, N) == cs
    assert lib.ob_det_ws_count(_ext.DET_WS_GELU, M, N) == cs
    assert lib.ob_det_ws_count(_ext.DET_WS_DROP_CS, M, N) == _cdiv(M, 128) * N
    if N % 8 == 0:
        if 512 <= N <= 1024:
            ln = 4 * min(_cdiv(M, 32), 1024) * N
        else:
            ln = max(2 * _cdiv(M, 16) * N, cs)
        assert lib.ob_det_ws_count(_ext.DET_WS_LN, M, N) == ln
    assert lib.ob_det_ws_count(_ext.DET_WS_CE, M, 1) == M
    assert lib.ob_det_ws_count(99, M, N) == -1


def test_ws_count_empty():
    lib = _lib()
    assert lib.ob_det_ws_count(0, 0, 768) == 0


_CHILD = ("from oobleck_amd._ext import get_ext, set_deterministic, "
          "deterministic\n"
          "lib = get_ext()\n"
          "a = lib.ob_deterministic()\n"
          "set_deterministic(not a)\n"
          "print(a, lib.ob_deterministic(), int(deterministic()))\n")


@pytest.mark.parametrize("value,expect", [(None, 0), ("0", 0), ("1", 1)])
def test_env_default_in_child(value, expect):
    """OB_DETERMINISTIC is the default of a fresh process; with no layer
    created the switch can still be flipped."""
    env = dict(os.environ)
    env.pop("OB_DETERMINISTIC", None)
    if value is not None:
        env["OB_DETERMINISTIC"] = value
    r = subprocess.run([sys.executable, "-c", _CHILD], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    a, b, c = (int(t) for t in r.stdout.split())
    assert a == expect and b == 1 - expect and c == 1 - expect
