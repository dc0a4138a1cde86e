# Fused AdamW over per-layer flat parameter buffers + WarmupLR.
#
# Replaces the reference's torch.optim.AdamW(fused=True) over
# _param_handle.flat_param (/root/reference/oobleck/execution/pipeline.py:
# 117-127) and deepspeed's WarmupLR (pipeline.py:125-127).  One HIP kernel
# launch per layer; 7 words/param of HBM traffic (read p,g,m,v; write p,m,v).
from __future__ import annotations

import torch

from ._ext import check, get_ext


class WarmupLR:
    """deepspeed.runtime.lr_schedules.WarmupLR semantics: lr rises
    log-or-linearly from warmup_min_lr to the optimizer lr over
    warmup_num_steps, then stays flat.  We implement the default linear
    ramp from 0 (deepspeed default warmup_min_lr=0)."""

    def __init__(self, optimizer: "FusedAdamW", warmup_num_steps: int):
        self.optimizer = optimizer
        self.warmup_num_steps = max(0, warmup_num_steps)
        self.base_lr = optimizer.lr
        self._step = 0
        self.step()  # deepspeed schedulers initialize lr at construction

    def step(self) -> None:
        self._step += 1
        if self.warmup_num_steps > 0 and self._step <= self.warmup_num_steps:
            self.optimizer.lr = self.base_lr * self._step / self.warmup_num_steps
        else:
            self.optimizer.lr = self.base_lr


class FusedAdamW:
    """max_grad_norm > 0 turns on global gradient-norm clipping
    (torch.nn.utils.clip_grad_norm_ semantics over the whole model, norm
    type 2): step() then runs GlobalGradNorm local -> combine -> finish and
    the scaled AdamW kernel, all on the device with no host sync.  The norm
    is global over the pipeline, so a rank of a multi-rank pipeline needs
    `clip_group` (the process group over the pipeline's ranks;
    PipelineExecution hands it over via set_clip_group()).

    Deviations from torch's clip + step: the scaled gradient is not written
    back into flat_grad, and a non-finite norm skips the update on the
    device (p, m, v untouched) while the host `step_count` still advances —
    the host never learns of the skip without a sync, so the bias
    correction of later steps counts the skipped one.  With
    max_grad_norm == 0 (default) step() is exactly the unclipped path."""

    def __init__(self, layers, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, max_grad_norm: float = 0.0,
                 clip_group=None, n_layers_total: int | None = None):
        self.layers = list(layers)
        self.lr = lr
        self.betas = betas
        self.eps = eps
        self.weight_decay = weight_decay
        self.step_count = 0
        self._m = [torch.zeros_like(l.flat_param) for l in self.layers]
        self._v = [torch.zeros_like(l.flat_param) for l in self.layers]
        if max_grad_norm < 0:
            raise ValueError("max_grad_norm must be >= 0")
        self.max_grad_norm = float(max_grad_norm)
        self._gradnorm = None
        if self.max_grad_norm > 0:
            from .gradnorm import GlobalGradNorm
            if n_layers_total is None:
                n_layers_total = self.layers[0].cfg.n_layers_total
            self._gradnorm = GlobalGradNorm(
                n_layers_total, self.layers[0].flat_param.device, clip_group)

    def set_clip_group(self, group) -> None:
        """The process group over the ranks of this optimizer's pipeline."""
        if self._gradnorm is not None:
            self._gradnorm.group = group

    @property
    def clip_group(self):
        return self._gradnorm.group if self._gradnorm is not None else None

    def grad_norm(self) -> float:
        """Global gradient norm of the last step (synchronises)."""
        if self._gradnorm is None:
            raise RuntimeError("grad_norm(): max_grad_norm is 0, no clipping")
        return self._gradnorm.last_norm()

    def skipped_steps(self) -> int:
        """Steps skipped for a non-finite gradient norm (synchronises)."""
        if self._gradnorm is None:
            return 0
        return self._gradnorm.skipped_steps()

    def step(self) -> None:
        import ctypes
        self.step_count += 1
        ext = get_ext()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        gn = self._gradnorm
        if gn is not None:
            gn.local(self.layers)
            gn.combine()
            gn.finish(self.max_grad_norm)
            stats = gn.stats_ptr()
        for l, m, v in zip(self.layers, self._m, self._v):
            p, g = l.flat_param, l.flat_grad
            if gn is None:
                rc = ext.ob_adamw_step(
                    ctypes.c_void_p(p.data_ptr()), ctypes.c_void_p(g.data_ptr()),
                    ctypes.c_void_p(m.data_ptr()), ctypes.c_void_p(v.data_ptr()),
                    p.numel(), self.step_count, self.lr, self.betas[0],
                    self.betas[1], self.eps, self.weight_decay, stream)
            else:
                rc = ext.ob_adamw_step_scaled(
                    ctypes.c_void_p(p.data_ptr()), ctypes.c_void_p(g.data_ptr()),
                    ctypes.c_void_p(m.data_ptr()), ctypes.c_void_p(v.data_ptr()),
                    p.numel(), self.step_count, self.lr, self.betas[0],
                    self.betas[1], self.eps, self.weight_decay, stats, stream)
            check(rc, f"adamw layer {l.layer_id}")
            refresh = getattr(l, "refresh_weights", None)
            if refresh is not None:
                refresh()  # bf16 shadows follow the fp32 master update

    def zero_grad(self) -> None:
        for l in self.layers:
            l.zero_grads()
