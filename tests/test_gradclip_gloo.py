# CPU (gloo) tests of GlobalGradNorm.combine(): the per-layer fp64 square
# norms of pipelines with DIFFERENT stage splits must combine to bit-identical
# vectors (heterogeneous data-parallel replicas must clip by the same
# coefficient), and FULL_SHARD shards of one layer must add up to the layer.
# The per-layer values are filled here with torch; the device kernels that
# fill them in production are covered by tests/test_gpu_gradclip.py.
from __future__ import annotations

import os
import pathlib
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

REPO_ROOT = pathlib.Path(__file__).resolve().parent.parent

L = 4
SIZES = [5003, 777, 12345, 4096]


def _setup(rank: int, world: int, tmp: str):
    if str(REPO_ROOT) not in sys.path:
        sys.path.insert(0, str(REPO_ROOT))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group(
        "gloo", init_method=f"file://{tmp}/rdzv", rank=rank, world_size=world)
    torch.set_num_threads(1)


def _layer_grads():
    g = torch.Generator().manual_seed(11)
    return [torch.randn(n, generator=g) * 3e-2 for n in SIZES]


def _sq(t: torch.Tensor) -> torch.Tensor:
    return (t.double() ** 2).sum()


def _run_hetero_splits(rank: int, world: int, tmp: str):
    _setup(rank, world, tmp)
    from oobleck_amd.gradnorm import GlobalGradNorm

    grads = _layer_grads()  # after the DP all-reduce both replicas hold these
    reference = torch.stack([_sq(g) for g in grads])

    # pipeline A = ranks 0,1 split [0,1] | [2,3]; B = ranks 2,3 split
    # [0] | [1,2,3].  Every rank co-calls every new_group.
    splits = {0: [0, 1], 1: [2, 3], 2: [0], 3: [1, 2, 3]}
    group_a = dist.new_group([0, 1])
    group_b = dist.new_group([2, 3])
    group = group_a if rank < 2 else group_b

    gn = GlobalGradNorm(L, torch.device("cpu"), group)
    assert gn.vec.dtype == torch.float64 and gn.vec.shape == (L,)
    gn.vec.zero_()
    for lid in splits[rank]:
        gn.vec[lid] = _sq(grads[lid])
    gn.combine()

    assert gn.vec.tolist() == reference.tolist(), \
        "combined vector must equal the single-process reference bit for bit"
    everyone = [torch.zeros(L, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(everyone, gn.vec)
    for other in everyone[1:]:
        assert [x.hex() for x in other.tolist()] == \
            [x.hex() for x in everyone[0].tolist()]

    # no group / a one-rank group: combine() is a no-op
    solo = GlobalGradNorm(L, torch.device("cpu"), None)
    solo.vec.copy_(reference)
    solo.combine()
    assert solo.vec.tolist() == reference.tolist()

    dist.barrier()
    dist.destroy_process_group()


def test_combine_is_bitwise_independent_of_stage_split(tmp_path):
    mp.spawn(_run_hetero_splits, args=(4, str(tmp_path)), nprocs=4, join=True)


def _run_full_shard(rank: int, world: int, tmp: str):
    _setup(rank, world, tmp)
    from oobleck_amd.gradnorm import GlobalGradNorm

    grads = _layer_grads()
    group = dist.new_group([0, 1])
    gn = GlobalGradNorm(L, torch.device("cpu"), group)
    gn.vec.zero_()
    shards = []
    for lid, g in enumerate(grads):
        # FSDP layout: world-size-padded, rank-ordered chunks; padding is 0
        shard_size = (g.numel() + world - 1) // world
        padded = torch.zeros(shard_size * world)
        padded[:g.numel()] = g
        shard = padded[rank * shard_size:(rank + 1) * shard_size]
        shards.append(shard)
        gn.vec[lid] = _sq(shard)
    mine = gn.vec.clone()
    gn.combine()

    # exactly the two shard sums added once ...
    both = [torch.zeros(L, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(both, mine)
    assert gn.vec.tolist() == (both[0] + both[1]).tolist()
    # ... which is the full-buffer sum to fp64 rounding (n * 2^-52 bounds
    # either summation order against the exact sum)
    for lid, g in enumerate(grads):
        full = _sq(g).item()
        assert abs(gn.vec[lid].item() - full) <= \
            2 * g.numel() * 2.0 ** -52 * full

    dist.barrier()
    dist.destroy_process_group()


def test_combine_full_shard_adds_up_to_the_layer(tmp_path):
    mp.spawn(_run_full_shard, args=(2, str(tmp_path)), nprocs=2, join=True)
