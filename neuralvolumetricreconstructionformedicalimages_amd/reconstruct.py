"""Classical iterative reconstruction from the same projections, voxel grid and metrics a NAF is trained and scored on: SIRT
over the forward projector A (`projector.project_scan`) and its transpose A^T (`projector.backproject_scan`).  It is the baseline
the reference took from TIGRE's iterative algorithms, which have no ROCm build.  DESIGN.md section 13.

SIRT, as computed here (1 is the all-ones vector of the matching space, ⊙ the element-wise product):

    R = 1 / (A 1)    where A 1 > 0, else 0          (inverse row sums: one weight per ray)
    C = 1 / (A^T 1)  where A^T 1 > 0, else 0        (inverse column sums: one weight per voxel)
    x <- x + relax * C ⊙ A^T (R ⊙ (b - A x)),   then x <- max(x, 0) if `nonneg`

`relax` must lie in (0, 1].  A has no negative entry, so the spectral radius of C A^T R A is at most 1, and in that range the
R-weighted residual ||b - A x_k||_R = sqrt(sum_r R_r (b - A x_k)_r^2) does not increase from one iteration to the next.  The solver
returns the volume and the list of these norms, one per iteration, each taken before that iteration's update.

The solver is plain array code over two callables and runs on whatever arrays they take (torch tensors on any device, numpy
arrays); only the two operators bound by `sirt` are HIP kernels.
"""
from __future__ import annotations

import math


def _namespace(a):
    import torch
    if isinstance(a, torch.Tensor):
        return torch, torch.clamp
    import numpy as np
    return np, np.clip


def sirt_operators(A, AT, b, n_iter, relax=1.0, nonneg=True, x0=None, callback=None):
    """SIRT over a forward operator `A` (volume -> projections) and its transpose `AT` (projections -> volume), both callables
    on arrays of `b`'s kind.  `x0` is the start (default zeros of the volume's shape), `callback(k, x, residual_norm)` runs after
    every iteration.  Returns (x, residual_norms) with residual_norms[k] = ||b - A x_k||_R, x_0 = x0."""
    relax = float(relax)
    if not (0.0 < relax <= 1.0):
        raise ValueError(f"sirt: relax must be in (0, 1], got {relax}")
    n_iter = int(n_iter)
    if n_iter < 0:
        raise ValueError(f"sirt: n_iter must be >= 0, got {n_iter}")
    xp, clamp = _namespace(b)
    col = AT(xp.ones_like(b))                                   # A^T 1, which also gives the volume's shape
    row = A(xp.ones_like(col))                                  # A 1
    R = xp.where(row > 0, 1.0 / xp.where(row > 0, row, xp.ones_like(row)), xp.zeros_like(row))
    C = xp.where(col > 0, 1.0 / xp.where(col > 0, col, xp.ones_like(col)), xp.zeros_like(col))
    x = xp.zeros_like(col) if x0 is None else x0 + xp.zeros_like(col)      # a copy: the caller's x0 stays as it is
    norms = []
    for k in range(n_iter):
        r = b - A(x)
        norms.append(math.sqrt(float((R * r * r).sum(dtype=xp.float64))))
        x = x + relax * (C * AT(R * r))
        if nonneg:
            x = clamp(x, 0, None)
        if callback is not None:
            callback(k, x, norms[-1])
    return x, norms


def sirt(projections, geo, angles, n_iter=50, relax=1.0, nonneg=True, x0=None, callback=None, views_per_call=None):
    """SIRT reconstruction of `projections` [N, H, W] (float32, on the GPU) taken with `geo` (ConeGeometry) at `angles` ->
    (float32 volume of geo.nVoxel on the projections' device, residual norms).  See the module docstring for the iteration."""
    from . import projector

    def A(x):
        return projector.project_scan(x, geo, angles, views_per_call=views_per_call)

    def AT(y):
        return projector.backproject_scan(y, geo, angles, views_per_call=views_per_call)

    return sirt_operators(A, AT, projections, n_iter, relax=relax, nonneg=nonneg, x0=x0, callback=callback)
