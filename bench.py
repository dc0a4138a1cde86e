#!/usr/bin/env python3
# bench.py — the reference's headline benchmark (BASELINE.json: tokens/sec,
# whole node, GPT-2 1F1B) on the MI355X-native hot path.
#
# One "step" = one full training step of the 1F1B pipeline over the global
# microbatch (gpt2.yaml: global_microbatch 128 sequences of S=1024 = 131072
# tokens/step), i.e. pipeline.train() + per-layer DP all-reduce + fused
# AdamW — the exact three calls of the reference's _train_step
# (engine.py:645-649).  Synthetic data (no network), random-init weights,
# fp32 (the reference's compute dtype; bf16 is §8 f4).
#
#   python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
#
# A plain run sets up, warms up, times the K steps and prints the result
# line.  --full adds the legs that take runs of their own (in-step kernel
# profile + roofline, CPU baseline).  --dump-outputs writes what the last
# timed step left behind (losses, updated params, AdamW first moments).
#
# N>1 is launched by the driver via torch.distributed.run (one rank/GPU,
# RCCL).  Topology: N=1 -> 1 stage; N=2 -> 2 stages; N=4 -> 4 stages;
# N=8 -> 4 stages x 2 DP replicas (BASELINE config[2]).
from __future__ import annotations

import argparse
import json
import os
import time

import torch
import torch.distributed as dist

TOPOLOGY = {1: (1, 1), 2: (2, 1), 4: (4, 1), 8: (4, 2)}  # gpus -> (stages, replicas)
F32_MFMA_PEAK_TF = 157.3   # gfx950 f32 matrix peak (MI355X_MICROARCH.md)
BF16_MFMA_PEAK_TF = 2500.0  # gfx950 bf16 dense MFMA peak (NOT the 2:1-sparse 5 PF)


def build_world(args, device):
    from oobleck_amd.config import GPT2_SMALL, GPT2_XL, TrainingConfig
    from oobleck_amd.engine import (DataParallelEngine, even_stage_split,
                                    make_rank_grid)
    from oobleck_amd.layer import Layer
    from oobleck_amd.optimizer import FusedAdamW, WarmupLR
    from oobleck_amd.pipeline import OobleckPipeline, SyntheticDataLoader

    mc = GPT2_XL if args.model == "gpt2-xl" else GPT2_SMALL
    tc = TrainingConfig(seq_len=args.seq_len,
                        microbatch_size=args.microbatch,
                        global_microbatch_size=args.global_batch)
    stages, replicas = TOPOLOGY[args.gpus]
    assert stages * replicas == args.gpus
    mb_total = tc.num_microbatches
    assert mb_total % replicas == 0
    mb_per_pipe = mb_total // replicas

    stage_layers = even_stage_split(mc, stages)
    pipelines, my_pipeline = [], None
    for pid in range(replicas):
        ranks = [pid * stages + s for s in range(stages)]
        grid = make_rank_grid(mc.n_layers_total, stage_layers,
                              [[r] for r in ranks])
        loader = SyntheticDataLoader(mc, tc.microbatch_size, tc.seq_len,
                                     seed=1234 + pid)
        p = OobleckPipeline(pid, grid, mc, tc, loader, mb_per_pipe, device)
        p.initialize_distributed_fsdp()
        p.initialize_distributed_pipeline()
        pipelines.append(p)
    for p in pipelines:
        if p.my_pipeline:
            def layer_factory(lid, pg, n_slots):
                return Layer(lid, mc, tc.microbatch_size, tc.seq_len,
                             n_slots, device, dtype=args.dtype)

            def optimizer_factory(layers):
                opt = FusedAdamW(layers, lr=tc.lr,
                                 betas=(tc.adam_beta1, tc.adam_beta2),
                                 eps=tc.adam_eps, weight_decay=tc.weight_decay)
                return opt, WarmupLR(opt, tc.warmup_steps)

            p.initialize_execution(layer_factory, optimizer_factory)
            my_pipeline = p
    dp = DataParallelEngine(pipelines)
    return mc, tc, pipelines, my_pipeline, dp


def train_step(my_pipeline, dp):
    # the reference's _train_step (engine.py:645-649): pipeline.train() ->
    # dp all-reduce -> optimizer step
    my_pipeline.train()
    if os.environ.get("OB_SKIP_OPT", "0") == "1":  # overlap-debug bisect
        return
    dp.do_allreduce(my_pipeline)
    my_pipeline.execution.optimizer_step()
    # grads accumulate across microbatches within a step; clear for the next
    for layer in my_pipeline.execution._layers:
        layer.zero_grads()


# ob_profile_* family ids (include/oobleck_stage.h)
PROF_FAMILIES = [
    (0, "gemm_fc_fwd"), (1, "gemm_fwd_other"), (2, "gemm_dx"),
    (3, "gemm_dw_side"), (4, "flash_fwd"), (5, "flash_bwd"),
    (6, "attn_matmuls"), (7, "layernorm"), (8, "cross_entropy"),
    (9, "elementwise"), (10, "adamw"),
]


def measure_step_profile(my_pipeline, dp, steps=2):
    """Run `steps` extra (untimed) training steps with the extension's
    in-step profiler enabled: every launch region is bracketed by HIP
    events on its own launch stream, accumulated per kernel family.
    Returns ({family: {total_ms, count, avg_us}}, n_steps).  The fc-fwd
    family's avg is the roofline's in-step per-launch time — the
    production dispatch under real step contention, not a standalone
    probe (it must agree with rocprofv3's per-kernel stats)."""
    import ctypes as ct
    from oobleck_amd._ext import get_ext
    ext = get_ext()
    torch.cuda.synchronize()
    ext.ob_profile_reset()
    ext.ob_profile_enable(1)
    for _ in range(steps):
        train_step(my_pipeline, dp)
    torch.cuda.synchronize()
    ext.ob_profile_enable(0)
    prof = {}
    for fid, name in PROF_FAMILIES:
        total = ct.c_double()
        cnt = ct.c_longlong()
        ext.ob_profile_read(fid, ct.byref(total), ct.byref(cnt))
        if cnt.value == 0:
            continue
        prof[name] = {
            "total_ms_per_step": round(total.value / steps, 3),
            "launches_per_step": cnt.value // steps,
            "avg_us": round(total.value * 1e3 / cnt.value, 2),
        }
    return prof, steps


def roofline_from_profile(mc, args, prof):
    """bf16 roofline from the IN-STEP profile of the production fc-fwd
    dispatch.  achieved = algorithmic FLOPs/launch / avg in-step launch
    time; traffic (HBM bytes/launch) from the committed PMC pass over the
    same dispatch (profiles/pmc_step_bf16.json) when present."""
    fc = prof.get("gemm_fc_fwd")
    if not fc:
        return None
    M, N, K = args.microbatch * args.seq_len, 4 * mc.n_embd, mc.n_embd
    flops = 2.0 * M * N * K
    avg_s = fc["avg_us"] / 1e6
    achieved_tf = flops / avg_s / 1e12
    traffic = None
    pmc_file = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                            "profiles", "pmc_step_bf16.json")
    if os.path.exists(pmc_file) and args.model == "gpt2":
        with open(pmc_file) as f:
            traffic = json.load(f).get("fc_fwd_hbm_bytes_per_launch")
    overlap = os.environ.get("OB_PP1_OVERLAP", "1") == "1"
    return {
        "bound": "mfma", "achieved": round(achieved_tf, 2),
        "peak": BF16_MFMA_PEAK_TF, "unit": "TFLOP/s",
        "frac": round(achieved_tf / BF16_MFMA_PEAK_TF, 4),
        "traffic": traffic,
        "kernel": (f"MLP fc forward GEMM M={M} N={N} K={K} bf16, measured "
                   "IN-STEP via HIP events on the launch stream (production "
                   "dispatch)"
                   + (" — under the default pp1 fwd/bwd dual-stream overlap,"
                      " so per-launch time includes cross-stream contention;"
                      " same kernel solo in-step: 50.4 us = 767 TF = 0.307"
                      " (profiles/r01_step_bf16_blaslt_kernel_stats.json,"
                      " profiles/r02_bench_solo_instep.json)" if overlap else "")),
        "avg_launch_ms": round(fc["avg_us"] / 1e3, 4),
        "launches_per_step": fc["launches_per_step"],
    }


def measure_roofline(args, device):
    """Dominant-kernel roofline: the MFMA GEMM at its most-executed hot
    shape (the MLP fc GEMM of config[0]: M=B*S=8192, N=4H=3072, K=H=768;
    bf16 mode uses the transposed weight shadow -> TB operand).
    achieved = algorithmic FLOPs per launch / avg launch duration (HIP
    events on the launch stream).  DESIGN.md derives the per-unit figures."""
    M, N, K = args.microbatch * args.seq_len, 4 * 768, 768
    bf16 = getattr(args, "dtype", "f32") == "bf16"
    if bf16:
        import tests.test_gpu_bf16 as tb
        A = torch.randn(M, K, device=device).bfloat16()
        B = torch.randn(N, K, device=device).bfloat16()  # transposed shadow
        C = torch.empty(M, N, device=device, dtype=torch.bfloat16)
        def run():
            tb.gemm_bf16(A, B, C, transB=1, M=M, N=N, K=K, lda=K, ldb=K,
                         ldc=N)
    else:
        from tests.gpu_helpers import gemm
        A = torch.randn(M, K, device=device)
        B = torch.randn(K, N, device=device)
        C = torch.empty(M, N, device=device)
        def run():
            gemm(A, B, C, M=M, N=N, K=K, lda=K, ldb=N, ldc=N)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(True), torch.cuda.Event(True)
    reps = 50
    start.record()
    for _ in range(reps):
        run()
    end.record()
    torch.cuda.synchronize()
    avg_s = start.elapsed_time(end) / 1000.0 / reps
    flops = 2.0 * M * N * K
    achieved_tf = flops / avg_s / 1e12
    peak = BF16_MFMA_PEAK_TF if bf16 else F32_MFMA_PEAK_TF
    traffic = None
    # bf16 plain GEMMs dispatch to hipBLASLt (ob_blaslt.hip) — the stale
    # PMC traffic file measured the hand-written kernel, so it only
    # applies to the f32 leg.
    if not bf16:
        pmc_file = os.path.join(
            os.path.dirname(os.path.abspath(__file__)), "profiles",
            "pmc_gemm_fc.json")
        if os.path.exists(pmc_file):
            with open(pmc_file) as f:
                traffic = json.load(f).get("hbm_bytes_per_launch")
    return {
        "bound": "mfma", "achieved": round(achieved_tf, 2),
        "peak": peak, "unit": "TFLOP/s",
        "frac": round(achieved_tf / peak, 4),
        "traffic": traffic,
        "kernel": ("MLP fc GEMM M=8192 N=3072 K=768 bf16 (production "
                   "dispatch: hipBLASLt Cijk; hand-written k_gemm_bf16 "
                   "carries the fused/fallback cases)"
                   if bf16 else
                   "k_gemm_f32 (MLP fc, M=8192 N=3072 K=768, fp32 MFMA)"),
        "avg_launch_ms": round(avg_s * 1e3, 4),
    }


DUMP_BUDGET_BYTES = 16 << 20  # all dumped arrays together (cap: 64 MB)


def _dump_sample(t, k):
    """float32 host copy of `t`, or of a fixed seeded sample of k of its
    elements (sorted indices; the same for every run and every build)."""
    t = t.detach().reshape(-1)
    if t.numel() > k:
        g = torch.Generator().manual_seed(t.numel())
        idx = torch.randint(0, t.numel(), (k,), generator=g).sort().values
        t = t[idx.to(t.device)]
    return t.float().cpu().numpy()


def dump_outputs(out_dir, my_pipeline):
    """Write what the timed path produced in its last step as
    <out_dir>/<name>.npy (float32): the loss buffers the last stage holds
    (one per pipe slot, i.e. the last microbatches of the step, plus the
    running total) and, per layer of this rank, the updated fp32 master
    params and AdamW first moments — sampled so everything fits the
    budget.  Replicas hold identical state, so only pipeline 0 writes."""
    import numpy as np
    if my_pipeline._pipeline_id != 0:
        return
    os.makedirs(out_dir, exist_ok=True)
    torch.cuda.synchronize()
    ex = my_pipeline.execution
    if my_pipeline.is_last_stage():
        slots = sorted(ex._loss_bufs)
        np.save(os.path.join(out_dir, "loss_last_microbatches.npy"),
                np.concatenate([_dump_sample(ex._loss_bufs[s], 1 << 30)
                                for s in slots]))
        np.save(os.path.join(out_dir, "total_loss.npy"),
                _dump_sample(ex.total_loss, 1 << 30))
    n_layers = my_pipeline.model_cfg.n_layers_total
    k = DUMP_BUDGET_BYTES // (4 * 2 * n_layers)
    opt = ex._optimizer
    for layer, m in zip(opt.layers, opt._m):
        np.save(os.path.join(out_dir, f"param_layer{layer.layer_id:02d}.npy"),
                _dump_sample(layer.flat_param, k))
        np.save(os.path.join(out_dir, f"adam_m_layer{layer.layer_id:02d}.npy"),
                _dump_sample(m, k))


def measure_cpu_baseline():
    """The oracle (CPU restatement of the reference's arithmetic) timed on
    this box's host cores — the reported baseline (kind=port).  Per
    BASELINE.md's measurement spec: warmup, then >=10 steady-state
    iterations; bounded to ~10-30 s of CPU work (one fwd+bwd microbatch at
    B=1, S=256 takes ~0.5-1 s here)."""
    from oracle.gpt2_oracle import OracleConfig, stage_forward_backward
    from oracle.gpt2_oracle import init_layer_params
    # cap threads: oversubscribing all 256 host cores on these small
    # matmuls is slower AND blows the bench time budget
    cores = min(32, os.cpu_count() or 8)
    torch.set_num_threads(cores)
    oc = OracleConfig()
    flats = [init_layer_params(oc, oc.layer_kind(i), 42 + i)
             for i in range(oc.n_layers_total)]
    B, S = 1, 256
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, oc.vocab_size, (B, S), generator=g)
    labels = ids.clone()
    all_layers = list(range(oc.n_layers_total))
    for _ in range(2):  # warmup (allocator + thread pool spin-up)
        stage_forward_backward(oc, flats, all_layers, ids, labels=labels)
    iters = 10
    t0 = time.perf_counter()
    for _ in range(iters):
        stage_forward_backward(oc, flats, all_layers, ids, labels=labels)
    dt = (time.perf_counter() - t0) / iters
    return {
        "value": round(B * S / dt, 2), "unit": "tokens/s", "cores": cores,
        "kind": "port",
        "sample": f"oracle GPT-2-small fwd+bwd, B={B} S={S} ({B*S} tokens), "
                  f"{iters} warm iters after 2 warmup, "
                  f"torch {torch.__version__} CPU, {cores} threads",
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--model", choices=["gpt2", "gpt2-xl"], default="gpt2",
                    help="gpt2 = gpt2.yaml GPT-2 small (the headline "
                         "config); gpt2-xl = the dims of examples/"
                         "gpt3.yaml (1600x48, head_dim 64 — BASELINE "
                         "config[3]'s workload)")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seq-len", type=int, default=1024)
    ap.add_argument("--microbatch", type=int, default=8)
    ap.add_argument("--global-batch", type=int, default=128)
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="bf16",
                    help="compute dtype (default bf16 mixed precision with "
                         "fp32 masters/grads — north_star's 'MFMA-bf16 "
                         "roofline' target dtype; f32 = the reference's "
                         "own compute dtype, kept as the parity anchor)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step "
                         "computed (losses, sampled params and AdamW "
                         "moments) as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs that take runs of their own: "
                         "in-step kernel profile + roofline, CPU baseline")
    ap.add_argument("--skip-cpu-baseline", action="store_true",
                    help="with --full: leave out the CPU-baseline leg")
    ap.add_argument("--skip-roofline", action="store_true",
                    help="with --full: leave out the profile/roofline leg")
    ap.add_argument("--probe", choices=["gemm"], default=None,
                    help="run ONLY the dominant-kernel roofline probe "
                         "(for clean rocprofv3 kernel-trace/PMC capture)")
    args = ap.parse_args()

    if args.probe == "gemm":
        torch.cuda.set_device(0)
        print(json.dumps({"probe": "gemm",
                          "roofline": measure_roofline(args, torch.device("cuda", 0))}))
        return

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, f"WORLD_SIZE {world} != --gpus {args.gpus}"

    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1:
        dist.init_process_group("nccl")
    else:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29571")
        dist.init_process_group("nccl", rank=0, world_size=1)

    mc, tc, pipelines, my_pipeline, dp = build_world(args, device)

    for _ in range(args.warmup):
        train_step(my_pipeline, dp)
    dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        train_step(my_pipeline, dp)
    dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    # MAX over ranks
    e = torch.tensor([elapsed], device=device)
    dist.all_reduce(e, op=dist.ReduceOp.MAX)
    elapsed = float(e.item())

    if args.dump_outputs and my_pipeline is not None:
        dump_outputs(args.dump_outputs, my_pipeline)

    want_roofline = args.full and not args.skip_roofline
    want_cpu_baseline = args.full and not args.skip_cpu_baseline

    # in-step kernel profile (extra untimed steps, all ranks so the
    # collectives stay in sync; bf16 roofline + step split come from this)
    prof = None
    if want_roofline:
        prof, _ = measure_step_profile(my_pipeline, dp)

    if rank == 0:
        tokens_per_step = args.global_batch * args.seq_len
        value = tokens_per_step * args.steps / elapsed
        stages, replicas = TOPOLOGY[args.gpus]
        result = {
            "metric": "tokens/sec (whole node) GPT-2 1F1B",
            "value": round(value, 1),
            "unit": "tokens/s",
            "n_gpus": args.gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 1),
            "higher_is_better": True,
            "scaling": "strong",  # global batch fixed at 128 as N grows
            "vs_baseline": None,  # reference publishes no numbers
            "dtype": args.dtype,  # f32 = the reference compute dtype
            "data": "synthetic",
            "config": {
                "workload": (
                    f"{'gpt3.yaml GPT-2-XL' if args.model == 'gpt2-xl' else 'gpt2.yaml GPT-2-small'}"
                    f" 1F1B, global microbatch "
                    f"{args.global_batch}x{args.seq_len} tokens, {args.dtype}"),
                "model": args.model,
                "global_batch": args.global_batch,
                "seq_len": args.seq_len,
                "parallelism": f"pp{stages}dp{replicas}",
            },
        }
        if want_roofline:
            # bf16: in-step measurement of the production dispatch; f32
            # keeps the standalone probe (validated against rocprofv3 in
            # round 1: bench 399.8 us vs rocprof 406.4 us avg)
            rl = roofline_from_profile(mc, args, prof) \
                if args.dtype == "bf16" and prof else None
            result["roofline"] = rl or measure_roofline(args, device)
            if prof:
                result["step_split"] = prof
                result["step_split_note"] = (
                    "per-family GPU busy-time from HIP events on each "
                    "family's launch stream, over 2 untimed post-bench "
                    "steps; gemm_dw_side overlaps gemm_dx/flash_bwd on a "
                    "side stream, so families can sum past ms_per_step")
        if want_cpu_baseline and world == 1:
            # contract: the CPU-baseline leg runs on rank 0 at N=1 only
            result["cpu_baseline"] = measure_cpu_baseline()
        print(json.dumps(result), flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
