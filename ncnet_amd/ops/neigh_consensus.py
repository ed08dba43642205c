"""Symmetric NeighConsensus (stack of Conv4d + ReLU) as one autograd Function.

Reference semantics (lib/model.py:122-153): ``y = conv(x) + swap(conv(swap(x)))``
where ``conv`` is the Conv4d+ReLU stack and ``swap`` exchanges the A and B
axes of the correlation volume.  Because of the ReLUs this is not equivalent
to symmetrised filters, so both branches are computed.

MI355X design:
* both branches (and, in training, the positive and negative pairs) are one
  batch of volumes for every Conv4d launch: the swapped branch is built once
  as a bf16 transposed copy of the 1-channel input (0.8 MB per volume) instead
  of permuting the 16-channel activations;
* hidden activations are channels-last bf16 blocks of 16 channels
  ``[NB, V, I, J, K, L, 16]``; channel counts that are not a multiple of 16
  are zero-padded (zero weights and bias keep them at 0);
* every layer runs on the conv16 MFMA kernels (csrc/conv4d_fwd.hip): 16-channel
  blocks directly (one call per output block; input blocks beyond the first
  are summed as fp32 partials), 1-channel operands through the ij encoding
  (csrc/jshift.hip: the (di, dj) plane offsets move into the channel axis),
  except the forward of a Cout=1 layer, whose MFMA rows are a 4x4 block of
  output planes (conv16_blk_fwd);
  kernel sizes 1, 3, 5, 7 (reference: any size, lib/conv4d.py:58-82);
* bias + ReLU are fused into each conv's epilogue; the backward runs the
  data-gradient convs with the previous layer's ReLU mask fused into their
  epilogue, and the weight gradients with the MFMA wgrad kernels (16 -> 16
  layers and Cout=1 layers on a side HIP stream, overlapped with the
  data-gradient chain);
* ``y = z1 + z2^T`` (the branch un-swap) and, in backward, its transpose plus
  the last layer's ReLU mask are single tiled kernels.
There is no silent PyTorch fallback on the GPU: a configuration without HIP
kernels (even kernel sizes) raises unless config.RUNTIME.allow_torch_fallback
(NCNET_ALLOW_TORCH_FALLBACK=1).

Execution paths: ``select_path`` is the ONE place that picks them (the model's
``process_correlation`` asks it too); ``neigh_consensus`` dispatches on its
answer and ``_ext.DISPATCH`` counts what ran.  This module holds only the
selector, the dispatcher and re-exports; the paths live in ``ops/nc/``, one
module per row group, all on the single-layer primitive ``nc/layers.py``.

| path | when | implementation | tests |
|---|---|---|---|
| ``reference`` | CPU tensors | ``ops/reference.py`` (fp32 oracle) | ``test_nc_general_cpu.py`` |
| ``torch_fallback`` | GPU, no HIP kernels (even kernel size) | the oracle, only with allow_torch_fallback | ``test_gpu_kernels.py`` |
| ``x3_inference`` | precision fp32 / mixed, no autograd | ``nc/x3.py neigh_consensus_x3`` (bf16x3 splits) | ``test_gpu_x3.py`` |
| ``mixed`` | precision mixed, autograd, fast-path shapes | ``nc/x3.py NeighConsensusMixedFn`` (x3 forward, bf16 backward) | ``test_gpu_x3.py`` |
| ``x3_fused`` / ``x3`` | precision fp32 (or mixed off the fast shapes), autograd | ``nc/x3.py NeighConsensusX3FusedFn`` / ``NeighConsensusX3Fn`` | ``test_gpu_x3.py`` |
| ``fused_fp8`` | inference, fp8 mode with nc_fp8, symmetric square (3,3)/(<=16,1) | ``nc/fused.py neigh_consensus_fused_x2_fp8`` (``nc_fused_k3_f8``, csrc/nc_fused.hip) | ``test_gpu_kernels.py`` |
| ``fused`` | inference, (3,3)/(<=16,1), not all-fp8 | ``nc/fused.py neigh_consensus_fused`` (``nc_fused_k3``, hidden layer in LDS) | ``test_gpu_kernels.py``, ``test_gpu_fusion.py`` |
| ``fp8`` | inference, fp8 mode, other 1 -> 16 -> 1 stacks | ``nc/fp8.py neigh_consensus_fp8`` (e4m3 Conv4d) | ``test_gpu_kernels.py`` |
| ``bf16_padded`` / ``bf16`` | everything else (training) | ``nc/train.py NeighConsensusPaddedFn`` / ``NeighConsensusFn`` | ``test_gpu_kernels.py``, ``test_gpu_nc_stages.py`` |
"""
from __future__ import annotations

import torch

from .. import config as _config
from . import _ext
from . import reference as ref
from .nc.fp8 import neigh_consensus_fp8, pin_fp8_weights
from .nc.fused import neigh_consensus_fused, neigh_consensus_fused_x2, neigh_consensus_fused_x2_fp8
from .nc.layers import interleave, layer_kinds, swap_pair
from .nc.train import NeighConsensusFn, NeighConsensusPaddedFn, fast1x_ok
from .nc.x3 import (X3_STAGES, NeighConsensusMixedFn, NeighConsensusX3Fn, NeighConsensusX3FusedFn, neigh_consensus_x3,
                    x3_ablation, x3_dropped, x3_fused_ok)

__all__ = ["neigh_consensus", "select_path", "layer_kinds", "fast1x_ok", "fp8_ok", "X3_STAGES", "x3_ablation", "x3_dropped",
           "x3_fused_ok", "pin_fp8_weights", "neigh_consensus_x3", "neigh_consensus_fp8", "neigh_consensus_fused",
           "neigh_consensus_fused_x2", "neigh_consensus_fused_x2_fp8", "NeighConsensusFn", "NeighConsensusPaddedFn",
           "NeighConsensusX3Fn", "NeighConsensusX3FusedFn", "NeighConsensusMixedFn"]

# Layer-level names that tests and scripts written against the one-file module
# import from here; new code imports them from the module that defines them.
# Functions and constants only: a name that is rebound at run time
# (train.FAST1X, fp8._FP8_PINS, x3._X3_DROP) has no copy here, and replacing one
# of these functions here does not change what the paths call (they resolve
# their helpers, e.g. pack_w1x, in their own modules).
from .nc.fused import FP8_NC_X_SCALE, _fused_weights, _fused_weights_f8_build, _pow2_scale, fused_tiles  # noqa: E402,F401
from .nc.layers import (_nitems, _reduce_wgrad16, blocks_to_ncl, planar_to_blocks, reduce_partials,  # noqa: E402,F401
                        wgrad16_partials, wgrad_groups, wgrad_plane_groups, wgrad_v3_groups, wgrad_v3_ok)
from .nc.train import _stack_bwd, _stack_fwd, pack_w1x  # noqa: E402,F401


def _fused_ok(kinds, kernel_sizes, channels, x) -> bool:
    return (_config.RUNTIME.nc_fused and not torch.is_grad_enabled() and list(kinds) == ["1in", "1out"] and channels[0] <= 16
            and list(kernel_sizes) == [3, 3] and x.shape[2] * x.shape[3] * x.shape[4] * x.shape[5] < 2 ** 30)


def fp8_ok(kinds, channels) -> bool:
    """fp8 NC kernels cover 1 -> (<=16 ->)* -> 1 stacks (one channel block)."""
    return (len(kinds) >= 2 and kinds[0] == "1in" and kinds[-1] == "1out" and all(k == "16" for k in kinds[1:-1])
            and max(channels) <= 16)


def select_path(x: torch.Tensor, weights, channels, symmetric: bool = True, fp8: bool = False,
                precision: str = "bf16", padded: torch.Tensor | None = None) -> str:
    """The execution path ``neigh_consensus`` takes for these arguments (the
    table in the module docstring).  Raises like the ops do on a GPU machine
    without the extension."""
    kernel_sizes = [w.shape[0] for w in weights]
    kinds = layer_kinds(channels, kernel_sizes)
    if not _ext.use_hip(x):
        return "reference"
    if kinds is None:
        return "torch_fallback"
    if precision in ("fp32", "mixed"):
        if not (torch.is_grad_enabled() and (x.requires_grad or any(w.requires_grad for w in weights))):
            return "x3_inference"
        fused = x3_fused_ok(kinds, channels, kernel_sizes, x, symmetric)
        if precision == "mixed" and fused:
            return "mixed"
        return "x3_fused" if fused else "x3"
    # fp8 mode: the fused bf16 stack where it applies (it never writes the
    # hidden volume), unless NCNET_NC_FP8=1 asks for the all-fp8 pipeline: then
    # the fused e4m3 kernel for the symmetric (3,3)/(<=16,1) stack and the fp8
    # Conv4d kernels for the others
    all_fp8 = fp8 and _config.RUNTIME.nc_fp8
    fused = _fused_ok(kinds, kernel_sizes, channels, x)
    if all_fp8 and fused and symmetric and tuple(x.shape[2:4]) == tuple(x.shape[4:6]):
        return "fused_fp8"
    if fused and not all_fp8:
        return "fused"
    if fp8 and not torch.is_grad_enabled() and fp8_ok(kinds, channels):
        return "fp8"
    return "bf16_padded" if padded is not None else "bf16"


def neigh_consensus(x: torch.Tensor, weights, biases, channels, symmetric: bool = True, fp8: bool = False,
                    precision: str = "bf16", padded: torch.Tensor | None = None) -> torch.Tensor:
    """x: [V,1,I,J,K,L] fp32; weights in checkpoint layout [k, out, in, k, k, k].
    Returns [V, C_last, I, J, K, L] fp32.

    Dispatches on ``select_path`` (module docstring table): the (3,3)/(<=16,1)
    inference stack on the fused kernel, ``fp8`` inference on the e4m3 kernels,
    ``precision='fp32'`` / ``'mixed'`` on the bf16x3 kernels, everything else
    with odd kernel sizes <= 7 and any channel counts on the bf16 autograd
    stack.  ``padded``: x's padded bf16 planes for both symmetric branches from
    ``mutual.mutual_matching_padded`` (the bf16 training stack uses them
    instead of padding x itself)."""
    path = select_path(x, weights, channels, symmetric, fp8, precision, padded)
    kernel_sizes = [w.shape[0] for w in weights]
    if path in ("reference", "torch_fallback"):
        if path == "torch_fallback":
            _ext.torch_fallback(f"NeighConsensus kernel sizes {kernel_sizes}")
        return ref.neigh_consensus(x.float(), [w.float() for w in weights], [b.float() for b in biases], symmetric)
    if path in ("x3_inference", "mixed", "x3_fused", "x3"):
        _ext.count("nc_x3")
    if path == "x3_inference":
        return neigh_consensus_x3(x, weights, biases, channels, symmetric)
    if path == "fused_fp8":
        _ext.count("nc_fused_k3_f8")
        return neigh_consensus_fused_x2_fp8(swap_pair(x), weights, biases)
    # every other path takes the input as fp32, contiguous
    xf = x.float().contiguous()
    if path == "fused":
        _ext.count("nc_fused_k3")
        return neigh_consensus_fused(xf, weights, biases, symmetric)
    kinds = tuple(layer_kinds(channels, kernel_sizes))
    if path == "fp8":
        _ext.count("nc_fp8")
        return neigh_consensus_fp8(xf, weights, biases, kinds, symmetric)
    params = interleave(weights, biases)
    if path == "mixed":
        _ext.count("nc_mixed")
        return NeighConsensusMixedFn.apply(xf, kinds, tuple(channels), *params)
    if path == "x3_fused":
        _ext.count("nc_x3_fused")
        return NeighConsensusX3FusedFn.apply(xf, kinds, tuple(channels), *params)
    if path == "x3":
        return NeighConsensusX3Fn.apply(xf, symmetric, kinds, tuple(channels), *params)
    _ext.count("nc_bf16")
    if path == "bf16_padded":
        return NeighConsensusPaddedFn.apply(xf, padded, symmetric, kinds, tuple(channels), *params)
    return NeighConsensusFn.apply(xf, symmetric, kinds, tuple(channels), *params)
