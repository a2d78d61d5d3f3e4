"""skellysim_amd — MI355X-native engine for SkellySim's hydrodynamic hot path.

Scope (BASELINE.json north_star / SURVEY.md §8): the Stokeslet / stresslet /
regularized-Stokeslet / rotlet N-body velocity evaluations behind SkellySim's
kernels::Evaluator seam (reference include/kernels.hpp:14-15), rebuilt from
scratch as hand-written HIP/CDNA4 (gfx950) fp64 kernels behind the reference's
own evaluator API, target-sharded across GPUs with RCCL over xGMI.

This package is the PRODUCT path: it requires the in-tree HIP extension
(libskellyhip.so) and a GPU to compute. It never falls back to CPU — the CPU
restatement under oracle/ is test infrastructure only.
"""

from .evaluator import (  # noqa: F401
    Evaluator,
    set_evaluator,
    stokeslet_direct_gpu,
    stresslet_direct_gpu,
    oseen_contract_direct_gpu,
    rotlet_gpu,
    stresslet_times_normal_times_density,
    stokeslet_device,
    stresslet_device,
    oseen_contract_device,
    rotlet_device,
    stresslet_normal_density_device,
    stresslet_times_normal_device,
    oseen_tensor_batched_device,
    stokeslet_grad,
    stresslet_grad,
    oseen_contract_grad,
    rotlet_grad,
    stokeslet_grad_device,
    stresslet_grad_device,
    oseen_contract_grad_device,
    rotlet_grad_device,
    stokeslet_pressure,
    stresslet_pressure,
    oseen_contract_pressure,
    stokeslet_pressure_device,
    stresslet_pressure_device,
    oseen_contract_pressure_device,
    trace_streamlines_device,
    trace_vortexlines_device,
    join_streamlines,
    nearest,
    nearest_device,
)
from .sharded import ShardedPairEvaluator, shard_sizes, allgather_rows  # noqa: F401

__version__ = "0.1.0"
