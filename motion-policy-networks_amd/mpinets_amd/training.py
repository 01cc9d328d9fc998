"""Minimal training driver for ``TrainingMotionPolicyNetwork`` (row N1).

The reference hands the model to a PyTorch-Lightning ``Trainer`` (run_training.py:58-117: Adam from
``configure_optimizers``, ``gradient_clip_val=1.0``, DDP over the GPUs).  Lightning, logging and
checkpoint callbacks are out of scope; this module is the numerical core of one
optimisation step so the new kernels can be driven end to end: forward + losses + backward on the
engine, bucketed gradient all-reduce over RCCL (``shard.allreduce_gradients``), clip, optimizer step.
"""
from __future__ import annotations

from typing import Dict

import torch

from . import shard


def _path_modules(model):
    """The modules whose ``forward`` takes the differentiable path or the inference path by their OWN ``training`` flag:
    the policy, its point-cloud encoder and the encoder's set-abstraction modules.  One of them left in ``eval()`` would
    run the inference kernels inside the step and leave its weights without gradients."""
    enc = getattr(model, "point_cloud_encoder", None)
    return (model,) if enc is None else (model, enc, *enc.SA_modules)


def train_step(model, optimizer: torch.optim.Optimizer, batch: Dict[str, torch.Tensor], batch_idx: int = 0,
               gradient_clip_val: float = 1.0) -> torch.Tensor:
    """One optimisation step; returns the detached loss of this rank's batch."""
    # (Module.train() walks every submodule: 0.25 ms of a 4 ms step at the reference's batch of 10 -- only when a module
    # that picks its path by its own flag is not in training mode)
    if not all(m.training for m in _path_modules(model)):
        model.train()
    optimizer.zero_grad(set_to_none=True)
    loss = model.training_step(batch, batch_idx)
    loss.backward()
    params = [p for group in optimizer.param_groups for p in group["params"] if p.requires_grad]
    shard.allreduce_gradients(params)
    if gradient_clip_val is not None:
        torch.nn.utils.clip_grad_norm_(params, gradient_clip_val)
    optimizer.step()
    return loss.detach()
