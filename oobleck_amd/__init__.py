# oobleck_amd — MI355X-native rebuild of Oobleck's pipeline-parallel
# execution hot path: hand-written CDNA4 HIP kernels behind a
# C-ABI (include/oobleck_stage.h), driven by a Python host that mirrors the
# reference's OobleckPipeline / Layer / DataParallelEngine surfaces so the
# planner and elastic logic drop in unchanged.
from .config import ModelConfig, TrainingConfig  # noqa: F401


def set_deterministic(on: bool) -> None:
    """Process-wide deterministic mode: fixed-order
    reductions in the bf16 backward, so a training step is a pure function of
    its inputs.  Call before the first Layer is created."""
    from ._ext import set_deterministic as _set
    _set(on)
