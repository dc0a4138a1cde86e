# @gpu: global gradient-norm clipping through OobleckPipeline at pp2 — the
# norm spans both stages, so each rank's AdamW must consume the coefficient
# of the WHOLE model's norm.  Same harness as test_gpu_pipeline.py: two
# processes share cuda:0, rendezvous and p2p over gloo.
from __future__ import annotations

import math
import os
import pathlib
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

REPO_ROOT = pathlib.Path(__file__).resolve().parent.parent

DIMS = dict(n_embd=128, n_head=2, n_layer=2, n_positions=128, vocab_size=307)
B, S, MB = 2, 128, 4
MAX_NORM = 1e-2


def _setup(rank: int, world: int, tmp: str):
    if str(REPO_ROOT) not in sys.path:
        sys.path.insert(0, str(REPO_ROOT))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group(
        "gloo", init_method=f"file://{tmp}/rdzv", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    torch.set_num_threads(2)


def _batches(vocab, n, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        ids = torch.randint(0, vocab, (B, S), generator=g)
        out.append((ids, ids.clone()))
    return out


def _run_pp2_clip(rank: int, world: int, tmp: str):
    _setup(rank, world, tmp)
    from oracle.gpt2_oracle import OracleConfig, adamw_step, init_layer_params

    from oobleck_amd.config import ModelConfig, TrainingConfig
    from oobleck_amd.engine import DataParallelEngine, make_rank_grid
    from oobleck_amd.layer import Layer
    from oobleck_amd.optimizer import FusedAdamW, WarmupLR
    from oobleck_amd.pipeline import OobleckPipeline

    dev = torch.device("cuda", 0)
    mc = ModelConfig(**DIMS)
    oc = OracleConfig(**DIMS)
    tc = TrainingConfig(microbatch_size=B, global_microbatch_size=B * MB,
                        seq_len=S, lr=1e-3, max_grad_norm=MAX_NORM)
    L = oc.n_layers_total
    flats = [init_layer_params(oc, oc.layer_kind(i), 42 * 100 + i)
             for i in range(L)]
    grid = make_rank_grid(L, [[0, 1], [2, 3]], [[0], [1]])

    class Loader:
        def __iter__(self):
            return iter({"input_ids": i, "labels": l}
                        for i, l in _batches(oc.vocab_size, MB, seed=7))

    def layer_factory(lid, pg, n_slots):
        layer = Layer(lid, mc, B, S, n_slots, dev, dtype="bf16")
        layer.flat_param.copy_(flats[lid].to(dev))
        layer.refresh_weights()
        return layer

    def optimizer_factory(layers):
        opt = FusedAdamW(layers, lr=tc.lr, max_grad_norm=tc.max_grad_norm)
        return opt, WarmupLR(opt, 0)

    pipe = OobleckPipeline(0, grid, mc, tc, Loader(), MB, dev)
    pipe.initialize_distributed_fsdp()
    pipe.initialize_distributed_pipeline()
    pipe.initialize_execution(layer_factory, optimizer_factory)
    opt = pipe.execution._optimizer
    assert opt.clip_group is not None
    dp = DataParallelEngine([pipe])

    pipe.train()
    dp.do_allreduce(pipe)
    torch.cuda.synchronize()

    # expected norm / coefficient from the grads the optimizer will consume:
    # per-layer double square sums, exchanged over gloo, added in layer order
    layers = pipe.execution._layers
    grads = {l.layer_id: l.flat_grad.cpu() for l in layers}
    sq = torch.zeros(L + 1, dtype=torch.float64)
    for lid, g in grads.items():
        sq[lid] = (g.double() ** 2).sum()
        sq[L] += g.numel()
    dist.all_reduce(sq)
    n_total = int(sq[L].item())
    total = 0.0
    for lid in range(L):
        total += sq[lid].item()
    exp_norm = math.sqrt(total)
    exp_coef = float(np.float32(
        min(1.0, float(np.float32(MAX_NORM)) / (exp_norm + 1e-6))))
    print(f"rank {rank}: expected norm {exp_norm!r} coef {exp_coef!r}")
    assert exp_coef < 1.0, "precondition: clipping must engage"

    pipe.execution.optimizer_step()
    torch.cuda.synchronize()

    norm = opt.grad_norm()
    both = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(both, torch.tensor([norm], dtype=torch.float64))
    assert both[0].item().hex() == both[1].item().hex(), \
        "grad_norm must be bitwise equal on both ranks"
    assert abs(norm - exp_norm) <= n_total * 2.0 ** -52 * exp_norm, \
        (norm, exp_norm)
    assert opt.skipped_steps() == 0
    # norms within fp64 rounding of each other round to the same fp32
    # coefficient or to neighbours
    assert abs(opt._gradnorm.last_coef() - exp_coef) <= \
        float(np.spacing(np.float32(exp_coef)))

    coef32 = torch.tensor(exp_coef, dtype=torch.float32)
    for layer in layers:
        lid = layer.layer_id
        # documented deviation: the clipped grad is not written back
        assert torch.equal(layer.flat_grad.cpu(), grads[lid])
        p = flats[lid].clone()
        m = torch.zeros_like(p)
        v = torch.zeros_like(p)
        adamw_step(p, grads[lid] * coef32, m, v, step=1, lr=tc.lr,
                   beta1=tc.adam_beta1, beta2=tc.adam_beta2,
                   eps=tc.adam_eps, weight_decay=tc.weight_decay)
        torch.testing.assert_close(layer.flat_param.cpu(), p, rtol=1e-5,
                                   atol=1e-6)

    # a clipping optimizer in a two-rank pipeline that created no group for
    # it (max_grad_norm == 0 in the pipeline's config) must refuse, not clip
    # by the stage-local norm
    tc0 = TrainingConfig(microbatch_size=B, global_microbatch_size=B * MB,
                         seq_len=S, lr=1e-3)
    pipe0 = OobleckPipeline(1, grid, mc, tc0, Loader(), MB, dev)
    pipe0.initialize_distributed_fsdp()
    pipe0.initialize_distributed_pipeline()
    assert pipe0._clip_pg is None
    with pytest.raises(RuntimeError, match="global gradient norm"):
        pipe0.initialize_execution(layer_factory, optimizer_factory)

    dist.barrier()
    dist.destroy_process_group()


@requires_gpu
def test_pp2_global_clip_end_to_end(tmp_path):
    mp.spawn(_run_pp2_clip, args=(2, str(tmp_path)), nprocs=2, join=True)
