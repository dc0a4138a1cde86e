# GlobalGradNorm — the model-wide gradient norm behind max_grad_norm.
#
# The reference left this seam open (`# amp enable check: gradient clipping`
# above self._optimizer.step(), oobleck/execution/pipeline.py:241-244
# there).  Here the norm is global over the model while a rank
# holds only its stage's layers (or its FULL_SHARD shards of them), and
# Oobleck's data-parallel replicas are pipelines with DIFFERENT stage splits
# that must still arrive at the same clip coefficient bit for bit.  So:
#
#   local()    one deterministic multi-tensor fp64 square-norm call into a
#              per-LAYER vector (slot = layer_id), zeros elsewhere;
#   combine()  all-reduce (SUM) of that vector over the pipeline's ranks —
#              a layer's elements are partitioned over the ranks holding it
#              (shard padding is zero), every other rank adds an exact 0;
#   finish()   a device kernel adds the vector in layer order — independent
#              of the stage split — and writes {total_sq, norm, coef,
#              skipped_steps}; the AdamW kernel reads coef from there.
#
# Nothing here synchronises with the host except the last_*/skipped_steps
# readers, which the training step never calls.
from __future__ import annotations

import ctypes

import torch
import torch.distributed as dist


class GlobalGradNorm:
    def __init__(self, n_layers_total: int, device, group=None):
        self.n_layers_total = int(n_layers_total)
        self.device = torch.device(device)
        self.group = group
        # per-layer square norms; stats = {total_sq, norm, coef, skipped}
        self.vec = torch.zeros(self.n_layers_total, dtype=torch.float64,
                               device=self.device)
        self.stats = torch.zeros(4, dtype=torch.float64, device=self.device)
        self._ws: torch.Tensor | None = None

    @staticmethod
    def _stream() -> ctypes.c_void_p:
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def local(self, layers) -> None:
        """vec[layer_id] = sum(flat_grad^2) for this rank's layers (its
        shard of them under FULL_SHARD), 0 for every other layer."""
        from ._ext import check, get_ext
        ext = get_ext()
        self.vec.zero_()
        n = len(layers)
        if n == 0:
            return
        grads = []
        for l in layers:
            sharded = getattr(l, "_sharded", None)
            if sharded is not None:
                sharded.wait_post()  # the sharded grad is read below
            g = l.flat_grad
            assert g.dtype == torch.float32 and g.is_contiguous()
            assert 0 <= l.layer_id < self.n_layers_total
            grads.append(g)
        ptrs = (ctypes.c_void_p * n)(*[g.data_ptr() for g in grads])
        counts = (ctypes.c_int64 * n)(*[g.numel() for g in grads])
        index = (ctypes.c_int32 * n)(*[l.layer_id for l in layers])
        need = int(ext.ob_sqnorm_ws_count(counts, n))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(1, need), dtype=torch.float64,
                                   device=self.device)
        check(ext.ob_sqnorm_multi_f32(
            ptrs, counts, index, n, ctypes.c_void_p(self._ws.data_ptr()),
            ctypes.c_void_p(self.vec.data_ptr()), self._stream()),
            "sqnorm_multi")

    def combine(self) -> None:
        """Sum the per-layer vector over the pipeline's ranks.  Plain torch
        + torch.distributed on whatever device the vector lives on."""
        if self.group is None or dist.get_world_size(self.group) <= 1:
            return
        if self.vec.is_cuda and dist.get_backend(self.group) == "gloo":
            # gloo has no CUDA collectives: stage through host memory (the
            # single-GPU composition tests; production is RCCL)
            host = self.vec.cpu()
            dist.all_reduce(host, group=self.group)
            self.vec.copy_(host)
        else:
            dist.all_reduce(self.vec, group=self.group)

    def finish(self, max_norm: float) -> None:
        from ._ext import check, get_ext
        check(get_ext().ob_clip_finish(
            ctypes.c_void_p(self.vec.data_ptr()), self.n_layers_total,
            max_norm, ctypes.c_void_p(self.stats.data_ptr()), self._stream()),
            "clip_finish")

    def stats_ptr(self) -> ctypes.c_void_p:
        return ctypes.c_void_p(self.stats.data_ptr())

    # -- lazy readers: the only calls that synchronise ----------------------
    def last_norm(self) -> float:
        return float(self.stats[1].item())

    def last_coef(self) -> float:
        """The fp32 clip coefficient of the last step; negative is the skip
        marker (non-finite gradient, nothing was updated)."""
        return float(self.stats[2].item())

    def skipped_steps(self) -> int:
        return int(self.stats[3].item())
