"""Inducing-point initialisation by greedy conditional-variance selection on the device
(csrc/greedy.hip; Burt, Rasmussen, van der Wilk 2020, "Convergence of Sparse Variational
Inference in Gaussian Processes Regression"): a pivoted Cholesky of Kff that picks, M
times, the training input whose variance given the points already chosen is largest.

Unlike k-means it uses the layer's own kernel (ARD lengthscales included), it never picks
a duplicate or near-duplicate row (every chosen point had conditional variance above
``threshold * variance``, so every squared pivot of the Cholesky of Kuu is above it), and
its by-product ``trace`` is tr(Kff - Qff) after every pivot: whether M is enough.

``greedy_variance`` returns host arrays as ``cluster.kmeans`` does, ``greedy_variance_device``
device tensors (the ``*_device`` convention).  The selection is deterministic in the row
order of X: there is no random permutation and no sampling.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import ops
from .cluster import _as_obs, _checked, _device
from .kernels import SquaredExponential

MAX_D = 32             # the kernels' input dimension limit (mgp_hip.h)
DEFAULT_THRESHOLD = 1e-4
DEFAULT_BLOCK = 64     # steps enqueued between two readbacks of the state word


@dataclass
class GreedyVarianceResult:
    """What greedy_variance_device returns; m <= M points, every field a device tensor."""
    Z: torch.Tensor                  # float32 [m, D] = X[indices]
    indices: torch.Tensor            # int64 [m], in the order chosen
    dmax: torch.Tensor               # float64 [m]: the conditional variance of each point when chosen
    trace: torch.Tensor              # float64 [m]: tr(Kff - Qff) after each point
    residual: torch.Tensor           # float64 [N]: diag(Kff - Qff) at the end
    factor: Optional[torch.Tensor]   # float32 [m, N]: rows of the pivoted Cholesky factor, or None
    stopped: bool                    # the threshold ended the selection before M points


def _arguments(X, M, kernel, threshold, block):
    """Every check that needs no device, made before anything is uploaded -> (X as checked,
    M, threshold, block)."""
    if not isinstance(kernel, SquaredExponential):
        raise ValueError(f"greedy variance selection supports SquaredExponential kernels, got {type(kernel).__name__}")
    X = _checked(X, True)
    shape = tuple(X.shape)
    if len(shape) not in (1, 2):
        raise ValueError(f"X must be 1-D or 2-D, got shape {shape}")
    N, D = shape[0], (1 if len(shape) == 1 else shape[1])
    if D < 1 or D > MAX_D:
        raise ValueError(f"X must have 1 to {MAX_D} columns, got {D}")
    if int(M) != M or M < 1 or M > N:
        raise ValueError(f"M must be an integer in [1, N = {N}], got {M}")
    n_ls = kernel.lengthscales.numel()
    if n_ls != 1 and n_ls != D:
        raise ValueError(f"the kernel has {n_ls} lengthscales; X with {D} columns needs 1 or {D}")
    threshold = float(threshold)
    if not threshold >= 0.0 or threshold == float("inf"):
        raise ValueError(f"threshold must be a finite non-negative number, got {threshold}")
    if int(block) != block or block < 1:
        raise ValueError(f"block must be a positive integer, got {block}")
    return X, int(M), threshold, int(block)


def greedy_variance_device(X, M, kernel, threshold=DEFAULT_THRESHOLD, block=DEFAULT_BLOCK, want_factor=False):
    """Up to M rows of X [N, D] (1-D: [N, 1]) by greedy conditional variance under `kernel`
    (a SquaredExponential, scalar or ARD lengthscales) -> GreedyVarianceResult.

    With d = diag(Kff) = variance, each step takes the row j of largest d (ties: the lowest
    index), stops if d[j] <= threshold * variance (then m < M and `stopped`), and otherwise
    appends the pivoted Cholesky row L[i] = (K[:, j] - sum_t L[t] L[t][j]) / sqrt(d[j]) and
    subtracts its square from d.  Kernel values, the dot products, d, dmax and trace are
    float64 on the device; the factor is stored float32 (its only large traffic, N M^2 / 2
    reads), which bounds how far down the selection stays exact.  Measured on the device
    against float64 (profiles/greedy_init_bench.json): d carries an absolute error of 1.5e-7 *
    variance, and down to the default threshold of 1e-4 every pivot on the test inputs is the
    float64 maximum -- that is the floor for an exact selection.  A smaller threshold is
    allowed and stays free of duplicates, but the pivots are no longer optimal: the worst
    relative shortfall against the float64 maximum was 1.3e-4 down to 3e-5, 2.2e-3 down to
    1e-5 and 7.1e-3 down to 1e-6.

    block: steps enqueued between two readbacks of the two-word state; it changes no bit of
    the result.  The cost is one launch per step, O(N M^2) in all."""
    X, M, threshold, block = _arguments(X, M, kernel, threshold, block)
    dev = kernel.device if kernel.device.type == "cuda" else _device()
    X, _ = _as_obs(X, "X", dev)
    N, D = X.shape
    variance, ls = kernel.variance.to(dev), kernel.lengthscales.to(dev)
    ws = ops.greedy_workspace(N, M, D, dev)
    factor = ops.greedy_factor(N, M, dev)
    state = torch.zeros(2, dtype=torch.int32, device=dev)
    ops.greedy_init(N, D, variance, threshold, ws)
    for done in range(0, M, block):
        ops.greedy_steps(X, variance, ls, M, min(block, M - done), factor, ws, state)
        if done + block < M and int(state.cpu()[1]):     # the one readback per block
            break
    indices, Z, dmax, trace, residual, info = ops.greedy_result(X, M, ws)
    m, stopped = (int(v) for v in info.cpu())
    return GreedyVarianceResult(Z=Z[:m], indices=indices[:m], dmax=dmax[:m], trace=trace[:m], residual=residual,
                                factor=factor[:m] if want_factor else None, stopped=bool(stopped))


def greedy_variance(X, M, kernel, threshold=DEFAULT_THRESHOLD):
    """greedy_variance_device with host results -> (Z float64 ndarray [m, D], indices int64
    ndarray [m]), m <= M."""
    r = greedy_variance_device(X, M, kernel, threshold)
    return r.Z.cpu().numpy().astype(np.float64), r.indices.cpu().numpy()


class ConditionalVariance:
    """The call shape of robustgp's initialiser of that name:
    ``Z, indices = ConditionalVariance().compute_initialisation(X, M, kernel)``.  Always the
    deterministic greedy selection in the row order of X (no random permutation, no
    ``sample=True``)."""

    def __init__(self, threshold=DEFAULT_THRESHOLD):
        self.threshold = threshold

    def compute_initialisation(self, training_inputs, M, kernel):
        return greedy_variance(training_inputs, M, kernel, self.threshold)
