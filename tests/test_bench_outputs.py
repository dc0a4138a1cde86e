# Pins bench.py's --dump-outputs sampling and the --full switch (CPU only):
# the sample of a large array is fixed (same indices every run, so two
# builds dump comparable arrays), float32, and within the byte budget.
import numpy as np
import torch


def test_dump_sample_small_is_whole_array():
    from bench import _dump_sample
    t = torch.arange(10, dtype=torch.float64).reshape(2, 5)
    out = _dump_sample(t, 16)
    assert out.dtype == np.float32
    np.testing.assert_array_equal(out, np.arange(10, dtype=np.float32))


def test_dump_sample_large_is_fixed_and_sorted():
    from bench import _dump_sample
    t = torch.arange(100_000, dtype=torch.float32)
    a = _dump_sample(t, 1000)
    b = _dump_sample(t.clone(), 1000)
    assert a.dtype == np.float32 and a.shape == (1000,)
    np.testing.assert_array_equal(a, b)
    assert (np.diff(a) >= 0).all()          # values == indices here
    assert a.max() > 90_000 and a.min() < 10_000   # spread over the array


def test_dump_budget_under_cap():
    from bench import DUMP_BUDGET_BYTES
    assert DUMP_BUDGET_BYTES <= 64 * 10**6
