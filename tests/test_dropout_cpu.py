# CPU: the dropout mask reference (numpy Philox4x32-10) against known-answer
# vectors, the torch masked restatement against the oracle, and the Python
# surface's defaults.  No GPU.
import inspect

import numpy as np
import torch

from oracle.gpt2_oracle import OracleConfig, init_layer_params
from oracle.gpt2_oracle import stage_forward_backward as oracle_sfb
from tests import dropout_ref as dr

TINY24 = dict(n_embd=96, n_head=4, n_layer=3, n_positions=64, vocab_size=211)

KAT = [
    ((0, 0, 0, 0), (0, 0),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2,
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
     (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for ctr, key, want in KAT:
        got = tuple(int(v[0]) for v in dr.philox4x32_10(ctr, key))
        assert got == want, ([hex(g) for g in got], [hex(w) for w in want])


def test_philox_vectorised_equals_scalar():
    q = np.array([0, 1, 7, 2 ** 32 - 1], dtype=np.uint64)
    vec = dr.philox4x32_10((q, 5, 6, 7), (8, 9))
    for i, qi in enumerate(q):
        one = dr.philox4x32_10((int(qi), 5, 6, 7), (8, 9))
        assert [int(v[i]) for v in vec] == [int(v[0]) for v in one]


def test_keep_mask_is_prefix_stable_and_keyed():
    """Element e's bit depends on (seed, layer, site, tick, e) only: a longer
    tensor extends a shorter one, and every key field changes the mask."""
    seed = (7 << 32) | 11
    base = dr.keep_mask(seed, 3, dr.SITE_RESID_MLP, 5, 0.5, 4099)
    assert np.array_equal(
        base, dr.keep_mask(seed, 3, dr.SITE_RESID_MLP, 5, 0.5, 8192)[:4099])
    for other in (dr.keep_mask(seed + 1, 3, dr.SITE_RESID_MLP, 5, 0.5, 4099),
                  dr.keep_mask(seed + (1 << 32), 3, 3, 5, 0.5, 4099),
                  dr.keep_mask(seed, 4, dr.SITE_RESID_MLP, 5, 0.5, 4099),
                  dr.keep_mask(seed, 3, dr.SITE_RESID_ATTN, 5, 0.5, 4099),
                  dr.keep_mask(seed, 3, dr.SITE_RESID_MLP, 6, 0.5, 4099),
                  dr.keep_mask(seed, 3, 3, 5 + (1 << 32), 0.5, 4099)):
        assert not np.array_equal(base, other)
    assert dr.keep_mask(seed, 3, 3, 5, 0.0, 4099).all()  # thr 0 keeps all


def test_keep_fraction_six_sigma():
    n, p = 1 << 20, 0.1
    sigma = (0.09 / n) ** 0.5
    for seed in ((1 << 32) + 12345, (9 << 32) + 7):
        mean = dr.keep_mask(seed, 2, dr.SITE_RESID_ATTN, 0, p, n).mean()
        assert abs(mean - 0.9) < 6 * sigma, (seed, mean)


def test_threshold_and_scale():
    assert dr.threshold(0.0) == 0
    assert dr.threshold(0.5) == 1 << 31
    # p is the fp32 the C-ABI receives, not the Python double
    assert dr.threshold(0.1) == int(float(np.float32(0.1)) * 2 ** 32)
    assert dr.scale(0.5) == 2.0


def test_masked_reference_with_ones_equals_oracle():
    """All-ones masks: the torch restatement IS the oracle (1e-5)."""
    oc = OracleConfig(**TINY24)
    L = oc.n_layers_total
    flats = [init_layer_params(oc, oc.layer_kind(i), 4200 + i)
             for i in range(L)]
    B, S, H, nh = 2, 48, oc.n_embd, oc.n_head
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, oc.vocab_size, (B, S), generator=g)
    ones = [dict(embd=torch.ones(B, S, H))] + \
        [dict(attn=torch.ones(B, nh, S, S), resid_attn=torch.ones(B, S, H),
              resid_mlp=torch.ones(B, S, H)) for _ in range(oc.n_layer)] + [{}]
    lids = list(range(L))
    loss, _, grads = dr.stage_forward_backward(oc, flats, lids, ids, ones,
                                               labels=ids)
    rloss, _, rgrads = oracle_sfb(oc, flats, lids, ids, labels=ids)
    torch.testing.assert_close(loss, rloss, rtol=1e-5, atol=1e-5)
    for a, b in zip(grads, rgrads):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)
    # one block alone, with an upstream grad
    x = torch.randn(B, S, H, generator=g) * 0.5
    dout = torch.randn(B, S, H, generator=g) * 0.1
    out, dx, (gr,) = dr.stage_forward_backward(oc, [flats[1]], [1], x,
                                               [ones[1]], dout=dout)
    rout, rdx, (rgr,) = oracle_sfb(oc, [flats[1]], [1], x, dout=dout)
    torch.testing.assert_close(out, rout, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(dx, rdx, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(gr, rgr, rtol=1e-5, atol=1e-5)


def test_masks_change_the_reference():
    oc = OracleConfig(**TINY24)
    flat = init_layer_params(oc, 1, 4201)
    B, S, H, nh = 2, 48, oc.n_embd, oc.n_head
    x = torch.randn(B, S, H, generator=torch.Generator().manual_seed(4))
    masks = dr.layer_masks(5, 1, 1, 0, dict(resid=0.1, attn=0.1), B, S, H, nh)
    assert set(masks) == {"attn", "resid_attn", "resid_mlp"}
    a = dr.layer_forward(oc, 1, flat, x, masks)
    b = dr.layer_forward(oc, 1, flat, x, {})
    assert not torch.equal(a, b)


def test_config_defaults_are_zero():
    from oobleck_amd.config import ModelConfig, TrainingConfig
    mc = ModelConfig()
    assert (mc.embd_pdrop, mc.resid_pdrop, mc.attn_pdrop) == (0.0, 0.0, 0.0)
    assert TrainingConfig().dropout_seed == 0


def test_default_layer_uses_legacy_create(monkeypatch):
    """_ext exposes ob_layer_create_ex, but a Layer built with defaults goes
    through ob_layer_create and never through create_ex."""
    import oobleck_amd.layer as layer_mod
    from oobleck_amd._ext import get_ext
    from oobleck_amd.config import ModelConfig
    lib = get_ext()
    for sym in ("ob_layer_create_ex", "ob_layer_set_training",
                "ob_layer_set_dropout_tick", "ob_dropout_mask"):
        assert hasattr(lib, sym), sym
    sig = inspect.signature(layer_mod.Layer.__init__)
    for name in ("embd_pdrop", "resid_pdrop", "attn_pdrop", "dropout_seed"):
        assert name in sig.parameters
    assert "tick" in inspect.signature(layer_mod.Layer.forward_slot).parameters
    assert hasattr(layer_mod.Layer, "train") and hasattr(layer_mod.Layer,
                                                         "eval")

    calls = []

    class Stop(Exception):
        pass

    class FakeExt:
        def ob_layer_param_count(self, desc):
            return 8

        def ob_layer_create(self, *a):
            calls.append("create")
            raise Stop

        def ob_layer_create_ex(self, *a):
            calls.append("create_ex")
            raise Stop

    monkeypatch.setattr(layer_mod, "get_ext", lambda: FakeExt())
    monkeypatch.setattr(layer_mod, "init_layer_params",
                        lambda *a, **k: torch.zeros(8))
    mc = ModelConfig(**TINY24)
    for kwargs, want in (({}, "create"),
                         (dict(resid_pdrop=0.0, attn_pdrop=0.0), "create"),
                         (dict(resid_pdrop=0.1), "create_ex")):
        try:
            layer_mod.Layer(1, mc, 2, 48, 2, torch.device("cpu"), **kwargs)
        except Stop:
            pass
        assert calls[-1] == want, (kwargs, calls)
    mcd = ModelConfig(**TINY24, attn_pdrop=0.1)
    try:
        layer_mod.Layer(1, mcd, 2, 48, 2, torch.device("cpu"))
    except Stop:
        pass
    assert calls[-1] == "create_ex"


def test_pipeline_tick_and_seed_are_stateless():
    """tick = step * microbatches + index; the seed folds the pipeline id."""
    from oobleck_amd.pipeline import OobleckPipeline, PipelineExecution

    class Opt:
        step_count = 3

    class Pipe:
        num_microbatches = 4

    ex = PipelineExecution.__new__(PipelineExecution)
    ex._optimizer, ex._pipeline_ref = Opt(), Pipe()
    assert [ex.dropout_tick(i) for i in range(4)] == [12, 13, 14, 15]

    from oobleck_amd.config import TrainingConfig
    seeds = []
    for pid in (0, 1, 2):
        p = OobleckPipeline.__new__(OobleckPipeline)
        p._pipeline_id, p.training_cfg = pid, TrainingConfig(dropout_seed=99)
        seeds.append(p.dropout_seed)
    assert seeds[0] == 99 and len(set(seeds)) == 3
    assert all(0 <= s < 1 << 64 for s in seeds)
