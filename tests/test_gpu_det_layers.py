# @gpu: deterministic mode at layer level.  The child
# (tests/det_layer_child.py) trains EMBED -> BLOCK -> BLOCK -> FINAL for two
# optimizer steps; two fresh deterministic processes must agree bit for bit
# on every array they save, for every attention / LayerNorm / dropout route.
# The three children (two deterministic, one default) run once per module
# and cover all configurations each.
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")
ROOT = pathlib.Path(__file__).resolve().parent.parent
CHILD = ROOT / "tests" / "det_layer_child.py"
CONFIGS = ["hd64_cpt", "hd64_wave", "hd128", "matp", "drop"]
AB_CONFIG = "hd64_wave"


def _child(path, mode, names, extra_env=None):
    env = dict(os.environ)
    env.pop("OB_DETERMINISTIC", None)
    env.update(extra_env or {})
    r = subprocess.run([sys.executable, str(CHILD), str(path), mode] + names,
                       cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def det_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("det")
    return (_child(d / "a.npz", "det", CONFIGS),
            _child(d / "b.npz", "det", CONFIGS))


@pytest.fixture(scope="module")
def default_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("det_default")
    # top-1 library GEMMs, as in the mode: what is left to differ is the
    # reductions and the b_qkv definition
    return _child(d / "c.npz", "default", [AB_CONFIG], {"OB_LT_TUNE": "0"})


@requires_gpu
@pytest.mark.parametrize("name", CONFIGS)
def test_two_processes_bit_equal(det_runs, name):
    a, b = det_runs
    keys = sorted(k for k in a if k.startswith(name + "__"))
    # loss x6, din x6, and per step 4 layers x (grad, param, m, v), + 2 flags
    assert len(keys) == 6 + 6 + 2 * 4 * 4 + 2
    assert sorted(k for k in b if k.startswith(name + "__")) == keys
    assert a[name + "__det"].tolist() == [1, 1, 1, 1]
    assert a[name + "__flash"].item() == (0 if name == "matp" else 1)
    differ = [k for k in keys if not np.array_equal(a[k], b[k])]
    assert not differ, differ
    for k in keys:
        if a[k].dtype.kind == "f":
            assert np.isfinite(a[k]).all(), k
    # the run did something: grads are non-zero and params moved
    assert np.abs(a[name + "__grad__0_1"]).max() > 0
    assert not np.array_equal(a[name + "__param__0_1"],
                              a[name + "__param__1_1"])


def _rel_l2(x, ref):
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    return np.linalg.norm(x - ref) / max(np.linalg.norm(ref), 1e-30)


def _bf16(a):
    return (a.astype(np.uint16).astype(np.uint32) << 16).view(np.float32)


@requires_gpu
def test_det_agrees_with_default(det_runs, default_run):
    """First optimizer step (same params on both sides): loss and din within
    the forward bound of test_gpu_bf16.py (1.5e-2), every flat grad within
    its grad bound (3e-2 rel-L2)."""
    a, c = det_runs[0], default_run
    n = AB_CONFIG
    assert c[n + "__det"].tolist() == [0, 0, 0, 0]
    for mb in range(3):
        la, lc = a[f"{n}__loss__0_{mb}"], c[f"{n}__loss__0_{mb}"]
        print("loss", mb, la, lc)
        assert abs(la - lc).max() <= 1.5e-2 * abs(lc).max()
        r = _rel_l2(_bf16(a[f"{n}__din__0_{mb}"]),
                    _bf16(c[f"{n}__din__0_{mb}"]))
        print("din", mb, r)
        assert r < 3e-2
    for lid in range(4):
        r = _rel_l2(a[f"{n}__grad__0_{lid}"], c[f"{n}__grad__0_{lid}"])
        print("grad", lid, r)
        assert r < 3e-2


@requires_gpu
def test_switch_frozen_and_fp32_refused(det_runs):
    a = det_runs[0]
    rc, still = a["set_after_create_rc"].tolist()
    assert rc != 0 and still == 1
    msg = str(a["fp32_create_error"][0])
    assert "deterministic" in msg and "fp32" in msg
