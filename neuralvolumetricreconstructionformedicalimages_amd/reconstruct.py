"""Classical reconstruction from the same projections, voxel grid and metrics a NAF is trained and scored on: SIRT and ASD-POCS
over the forward projector A (`projector.project_scan`) and its transpose A^T (`projector.backproject_scan`), filtered
back-projection (FDK) as one row filter (`filter.filter_rows`) followed by that same A^T, OS-SART over the subset kernels of
`sart` (the same A and A^T restricted to a list of views), FISTA on the TV-penalised least-squares objective over those
kernels and the TV proximal map (`tv.tv_prox`), and CGLS with per-ray weights over the same pair and the vector kernels of `cgls_kernels`.
They are the baselines the reference took from TIGRE, which has no ROCm build.  DESIGN.md sections 13 to 19.

`sirt`, `asd_pocs`, `cgls`, `os_sart`, `fista_tv` and `ray_length_weights` take `kind`: "interpolated" (the default) is the pair above, "siddon" the
ray-voxel intersection projector and its exact transpose (include/naf_hip.h P6 / P7, DESIGN.md sections 20 and 21), the matched
pair for scans made with `project_scan(kind="siddon")`.  A and A^T are always bound to the same kind.  The Siddon transpose sums
with fp32 atomics and has no atomic-free form, so `kind="siddon"` with `deterministic=True` raises ValueError.  `os_sart`
and `fista_tv` run the pair on fused subset kernels of its own (P8), where R = 1 / (A 1) is the row sum the
forward walk keeps beside A x.  `fdk` (its weights are derived for the interpolated A^T) has no such parameter.

SIRT, as computed here (1 is the all-ones vector of the matching space, ⊙ the element-wise product):

    R = 1 / (A 1)    where A 1 > 0, else 0          (inverse row sums: one weight per ray)
    C = 1 / (A^T 1)  where A^T 1 > 0, else 0        (inverse column sums: one weight per voxel)
    x <- x + relax * C ⊙ A^T (R ⊙ (b - A x)),   then x <- max(x, 0) if `nonneg`

`relax` must lie in (0, 1].  A has no negative entry, so the spectral radius of C A^T R A is at most 1, and in that range the
R-weighted residual ||b - A x_k||_R = sqrt(sum_r R_r (b - A x_k)_r^2) does not increase from one iteration to the next.  The solver
returns the volume and the list of these norms, one per iteration, each taken before that iteration's update.

OS-SART (ordered subsets: SART when every subset is one view, SIRT when one subset holds every view).  The views are split into
subsets (`subset_order`); A_s, b_s and R_s are the rows of A, b and R that belong to the views of subset s:

    R = 1 / (A 1) as above;   C_s = 1 / (A_s^T 1)  where A_s^T 1 > 0, else 0      (inverse column sums of the subset's rows)
    beta = relax.  For k in range(n_iter):
        for s in the order of `subsets`:   x <- x + beta * C_s ⊙ A_s^T (R_s ⊙ (b_s - A_s x)),   then x <- max(x, 0) if `nonneg`
        beta *= relax_red

so the volume is corrected once per subset and not once per pass over the data.  The norm reported for iteration k is
sqrt(sum_s ||b_s - A_s x||_{R_s}^2), each subset's residual taken just before that subset's update: no extra projection is made
for it, and with one subset it is SIRT's norm.  `os_sart_operators` is the array code; `os_sart` runs the same iteration on three
HIP kernels (include/naf_hip.h P4), where the row sum of a ray is its length inside the volume (every sample's eight trilinear
weights sum to 1), so R is never stored, and where each C_s is kept after the subset's first visit if all of them fit
`weight_cache_bytes`.

ASD-POCS (Sidky and Pan 2008, as TIGRE runs it, with one SIRT update as the data step and no early stop) is the heuristic of the two
TV-regularised baselines: it has no stated objective, and its result depends on its schedule.  It follows every data step with `tv_steps` normalised steepest-descent steps on the volume's total variation (`tv.tv_descent`, include/naf_hip.h V2):

    beta = relax.  For k in range(n_iter):
        x_prev = x;  x <- x + beta * C ⊙ A^T (R ⊙ (b - A x));  x <- max(x, 0) if `nonneg`;  beta *= relax_red
        dp = ||x - x_prev||_2;  dd = ||A x - b||_2
        if k == 0: dtvg = alpha * dp
        x_data = x;  x <- tv_descent(x, dtvg, tv_steps)          (tv_steps steps of length dtvg each)
        dg = ||x - x_data||_2
        if dg > rmax * dp and dd > 0: dtvg *= alpha_red

FISTA-TV (Beck and Teboulle 2009) is the convergent one.  It minimises

    F(x) = 1/2 ||A x - b||_R^2 + lam * TV(x)   over x >= 0 (if `nonneg`),     ||d||_R^2 = sum_r R_r d_r^2,  R = 1 / (A 1) as above,

with TV the exact isotropic total variation of include/naf_hip.h V3 (no eps).  Its one weight is `lam`; F can be printed, and its
minimiser does not depend on a schedule.  A^T is the exact transpose of A and A has no negative entry, so A^T R A is symmetric with
row sums (A^T R A 1)[v] = (A^T 1)[v] and L = max_v (A^T 1)[v] >= ||A^T R A||_2: a rigorous step bound without a power iteration.

    y_0 = x_0, t_0 = 1.  For k in range(n_iter):
        res = b - A y_k;   norm_k = ||res||_R
        z = y_k + A^T (R ⊙ res) / L
        x_{k+1} = prox_{(lam / L) TV + C}(z)                       (`tv.tv_prox`: `tv_iters` dual iterations, warm-started)
        t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2;   y_{k+1} = x_{k+1} + ((t_k - 1) / t_{k+1}) (x_{k+1} - x_k)

The norm reported for iteration k is taken at the extrapolated point y_k, not at x_k: it is the residual the step needs anyway
and costs no extra projection (y_0 = x_0, and y_k - x_k -> 0 as the iteration converges).  `fista_tv_operators` is the array code;
`fista_tv` runs the same iteration with `sart.residual_scan` (R ⊙ res in one launch) and `sart.backproject_scan` over all views.

CGLS (conjugate gradients on the normal equations A^T W A x = A^T W b; Hestenes and Stiefel 1952, TIGRE's Krylov method) minimises
1/2 ||b - A x||_W^2 with ||d||_W^2 = sum_r w_r d_r^2 and one weight w_r >= 0 per ray (`weights=None`: all ones).  A weight of 0
leaves a ray out, R = 1 / (A 1) (`ray_length_weights`) makes the objective FISTA-TV's data term and the norms comparable with
SIRT's, and exp(-b) (`pwls_weights`) is the statistical weight of `dataset.add_noise`'s model.  No row or column sums are needed:

    r = b - A x0;  s = A^T (w ⊙ r);  p = s;  gamma = ||s||^2
    for k in range(n_iter):
        norm_k = ||r||_W                         (taken before the update, like every other solver's list)
        q = A p;  delta = sum w q^2
        if not gamma > 0 or not delta > 0: stop  (x is a minimiser, or p lies in the null space of W^(1/2) A)
        alpha = gamma / delta;  x += alpha p;  r -= alpha q
        s = A^T (w ⊙ r);  gamma' = ||s||^2;  beta = gamma' / gamma;  p = s + beta p;  gamma = gamma'

The method is linear, so nothing is clamped inside the loop; `nonneg` clamps the returned volume once at the end.  r is the
recurred residual, not b - A x recomputed, and there are no restarts: in float32 the two drift apart over many iterations, which
ten to twenty iterations do not reach.  The finite termination and the monotone ||r||_W rest on A^T being the exact transpose of A,
which it is here.  `cgls_operators` is the array code; `cgls` runs the same iteration with the scalars kept
on the device by three HIP kernels (`cgls_kernels`, include/naf_hip.h K1): fp64 sums in a fixed order, no host read-back per iteration.

FDK (Feldkamp, Davis and Kress, in the form of Kak and Slaney ch. 3, the row spacing taken at the isocentre).  Detector pixel
(u, v), u along the last axis of [N, H, W] (pitch du = dDetector[0], perpendicular to the rotation axis), v along the rows (dv);
cos(gamma) = DSD / sqrt(DSD^2 + u^2 + v^2);  tau = du * DSO / DSD;  t[m] = tau * h(m tau), the taps of `filter.ramp_taps`:

    q_i[r, n] = sum_k t[|n - k|] * cos(gamma)[r, k] * p_i[r, k]            (linear convolution, zero outside the row)
    f(x)      = sum_i w_i * (DSO^2 / U_i(x)^2) * q_i(u*(x), v*(x))         (U_i: depth of x from the source along the central ray)
    w_i       = pi * gap_i / sum_j gap_j                                   (`filter.view_weights`; pi / N for equally spaced views)

For a smooth y the matched transpose deposits y * (len / n) * w_c along every ray; the trilinear weights integrate to the voxel
volume dV and a ray's share of the cross-section at depth U is U^2 du dv / (DSD^2 cos(gamma)), so in the continuum limit
(A^T y)(x) = y(u*, v*) * (dV / (du dv)) * (DSD^2 / U^2) / cos(gamma) for a cone beam and y(u*, v*) * dV / (du dv) for a parallel
one.  The 1 / U^2 of FDK is therefore already in A^T and no second back-projector is needed:

    cone:      x_FDK = A^T y,   y_i = w_i * (DSO^2 / DSD^2) * (du dv / dV) * cos(gamma) * q_i
    parallel:  x_FDK = A^T y,   y_i = w_i * (du dv / dV) * q_i,   with tau = du and no cosine weights

By default there are no short-scan weights: a cone scan that covers less than a full turn is then reconstructed with a bias.
`short_scan="parker"` multiplies p_i[r, k] by Parker's weight of view i and column k (`filter.parker_weights`, inside the filter's
pass) and takes w_i = gap_i, for scans of pi .. 2 pi.  A tilted
(laminographic) scan is refused: its constant and filter direction are not verified here.

Laminographic FBP (`lamino_fbp`, `lamino_fbp_weights`, `lamino_fbp_operators`) is that form for a parallel beam
whose rotation axis is tilted by tau against the detector's rows, over a full turn.  The axis projects onto the detector's row
direction, so the ramp still runs along the rows with tau_taps = du; every frequency outside the missing cone k_r < |k_z| tan(tau) is
seen twice per turn and the Jacobian of (angle, row frequency) -> k carries cos(tau):

    x_FBP = A^T y,   y_i = w_i * cos(tau) * (du dv / dV) * q_i,   sum w_i = pi over the full turn, no cosine weights

`find_center_tilted` / `find_center_tilted_operators` are `find_center` for such a scan (`center.slices_tilted`): sharpness, maximised,
on the slice z = 0; negativity is largest at the true centre there and is refused.

The solvers are plain array code over callables and run on whatever arrays those take (torch tensors on any device, numpy
arrays); only the operators bound by `sirt`, `asd_pocs` and `fdk`, and the whole of `os_sart`, `fista_tv` and `cgls`, are HIP kernels.

`reduce_metal` / `reduce_metal_operators` are no solver but a repair of the projections in front of one: the trace of the metal
voxels of a first reconstruction is in-painted along the detector rows (`metal.inpaint_rows`).  `find_center` /
`find_center_operators` are none either: they find the offset of the detector's column axis that the scan's `offDetector[0]` lacks
(`center.slices`, `center.metrics`), and `recenter` writes it into a scan.
"""
from __future__ import annotations

import math


def _namespace(a):
    import torch
    if isinstance(a, torch.Tensor):
        return torch, torch.clamp
    import numpy as np
    return np, np.clip


def _check_n_iter(who, n_iter):
    n_iter = int(n_iter)
    if n_iter < 0:
        raise ValueError(f"{who}: n_iter must be >= 0, got {n_iter}")
    return n_iter


def _inverse_where_positive(a, xp):
    return xp.where(a > 0, 1.0 / xp.where(a > 0, a, xp.ones_like(a)), xp.zeros_like(a))


def _weights_and_start(A, AT, b, x0, xp):
    """R = 1 / (A 1), C = 1 / (A^T 1) (0 where the sum is not > 0) and the start volume: zeros, or a copy of `x0`."""
    col = AT(xp.ones_like(b))                                   # A^T 1, which also gives the volume's shape
    row = A(xp.ones_like(col))                                  # A 1
    x = xp.zeros_like(col) if x0 is None else x0 + xp.zeros_like(col)      # a copy: the caller's x0 stays as it is
    return _inverse_where_positive(row, xp), _inverse_where_positive(col, xp), x


def _norm(d, xp):
    return math.sqrt(float((d * d).sum(dtype=xp.float64)))


def sirt_operators(A, AT, b, n_iter, relax=1.0, nonneg=True, x0=None, callback=None):
    """SIRT over a forward operator `A` (volume -> projections) and its transpose `AT` (projections -> volume), both callables
    on arrays of `b`'s kind.  `x0` is the start (default zeros of the volume's shape), `callback(k, x, residual_norm)` runs after
    every iteration.  Returns (x, residual_norms) with residual_norms[k] = ||b - A x_k||_R, x_0 = x0."""
    relax = float(relax)
    if not (0.0 < relax <= 1.0):
        raise ValueError(f"sirt: relax must be in (0, 1], got {relax}")
    n_iter = _check_n_iter("sirt", n_iter)
    xp, clamp = _namespace(b)
    R, C, x = _weights_and_start(A, AT, b, x0, xp)
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


def _method(deterministic):
    """`deterministic=True` binds the gather transpose (projector.backproject_scan(method="gather")): no atomics, so a run returns
    the same bits every time; the default keeps the scatter."""
    return "gather" if deterministic else "scatter"


def _check_kind(who, kind, deterministic):
    """`kind` names the projector pair.  The Siddon transpose sums with fp32 atomics and has no atomic-free form, so it cannot be
    combined with `deterministic=True`."""
    from . import projector
    projector.check_kind(kind, who)
    if kind == "siddon" and deterministic:
        raise ValueError(f"{who}: kind='siddon' cannot be deterministic: its transpose sums with fp32 atomics in hardware order, and "
                         "the atomic-free gather transpose exists for the interpolated pair only")
    return kind


def _scan_operators(geo, angles, views_per_call, deterministic, device, kind="interpolated", who="reconstruct"):
    """(A, AT) of a scan on the kernels: `projector.project_scan` and `projector.backproject_scan` over one `Scan`, both of the
    same `kind`, so that AT is the transpose of A."""
    from . import projector
    _check_kind(who, kind, deterministic)
    common = {"views_per_call": views_per_call, "scan": projector.Scan(geo, angles, device), "kind": kind}

    def A(x):
        return projector.project_scan(x, geo, angles, **common)

    def AT(y):
        return projector.backproject_scan(y, geo, angles, method=_method(deterministic), **common)

    return A, AT


def _device_solve_setup(who, projections, geo, angles, x0, deterministic, workspace_views=None, kind="interpolated"):
    """What the solvers that run on the subset kernels start from -> (scan, x, transpose): the `Scan`, the start volume (zeros, or
    a copy of `x0`) and the keyword arguments of `sart.backproject_scan` on the pair of `kind`, with a span table for calls of up to
    `workspace_views` views (default: all) if `deterministic`."""
    import torch

    from . import _abi, projector
    if not isinstance(projections, torch.Tensor) or not projections.is_cuda:
        raise RuntimeError(f"{who}: projections must be a CUDA/HIP tensor (no CPU path)")
    scan = projector.Scan(geo, angles, projections.device)
    if x0 is None:
        x = torch.zeros(scan.dims, device=projections.device, dtype=torch.float32)
    else:
        _abi.check_volume(x0, who, "x0")
        projector.check_geometry(x0, geo)
        x = x0.clone()
    transpose = {"method": _method(deterministic), "scan": scan, "kind": kind}
    if deterministic:
        transpose["workspace"] = projector.gather_workspace(workspace_views or scan.N, scan.H, scan.W, projections.device)
    return scan, x, transpose


def sirt(projections, geo, angles, n_iter=50, relax=1.0, nonneg=True, x0=None, callback=None, views_per_call=None,
         deterministic=False, kind="interpolated"):
    """SIRT reconstruction of `projections` [N, H, W] (float32, on the GPU) taken with `geo` (ConeGeometry) at `angles` ->
    (float32 volume of geo.nVoxel on the projections' device, residual norms).  See the module docstring for the iteration.
    `deterministic=True` takes the atomic-free transpose: two runs return the same bits.  `kind="siddon"` runs A and A^T on the
    ray-voxel intersection pair (naf_hip.h P6 / P7) instead of the interpolated one; it cannot be deterministic."""
    A, AT = _scan_operators(geo, angles, views_per_call, deterministic, projections.device, kind, "sirt")
    return sirt_operators(A, AT, projections, n_iter, relax=relax, nonneg=nonneg, x0=x0, callback=callback)


def subset_order(angles, n_subsets, order="angular-distance", seed=0):
    """Splits the views of a scan into `n_subsets` subsets and orders the subsets -> list of int64 index arrays into `angles`.
    The views are taken in sorted-angle order and dealt round-robin, so every subset spans the scan.  `order`:
    "sequential": as dealt;  "random": a permutation drawn once from `seed`;  "angular-distance" (TIGRE's default idea): start at
    the first subset, then always the subset whose mean angle, as a direction mod pi, is farthest from those already visited
    (largest distance to the nearest visited one; ties go to the one farthest from the last visited, then to the lowest index)."""
    import numpy as np
    angles = np.asarray(angles, dtype=np.float64).reshape(-1)
    N, n_subsets = len(angles), int(n_subsets)
    if not (1 <= n_subsets <= N):
        raise ValueError(f"os_sart: n_subsets must be in [1, {N}] for {N} views, got {n_subsets}")
    by_angle = np.argsort(angles, kind="stable")
    subsets = [by_angle[i::n_subsets].astype(np.int64) for i in range(n_subsets)]
    if order == "sequential":
        visit = list(range(n_subsets))
    elif order == "random":
        visit = [int(i) for i in np.random.default_rng(seed).permutation(n_subsets)]
    elif order == "angular-distance":
        mean = np.array([angles[s].mean() for s in subsets])

        def distance(i, j):
            d = abs(mean[i] - mean[j]) % math.pi
            return min(d, math.pi - d)

        visit, left, tie = [0], list(range(1, n_subsets)), 1e-9
        while left:
            nearest = [min(distance(i, j) for j in visit) for i in left]
            best = [i for i, d in zip(left, nearest) if d >= max(nearest) - tie]
            to_last = [distance(i, visit[-1]) for i in best]
            visit.append(next(i for i, d in zip(best, to_last) if d >= max(to_last) - tie))
            left.remove(visit[-1])
    else:
        raise ValueError(f"os_sart: order must be 'sequential', 'random' or 'angular-distance', got {order!r}")
    return [subsets[i] for i in visit]


def _check_os_sart(relax, relax_red, n_iter):
    relax, relax_red = float(relax), float(relax_red)
    for name, value in (("relax", relax), ("relax_red", relax_red)):
        if not (0.0 < value <= 1.0):
            raise ValueError(f"os_sart: {name} must be in (0, 1], got {value}")
    return relax, relax_red, _check_n_iter("os_sart", n_iter)


def os_sart_operators(A, AT, b, subsets, n_iter, relax=1.0, relax_red=1.0, nonneg=True, x0=None, callback=None):
    """OS-SART over `A(x, views)` (volume -> the projections [len(views), H, W] of those views) and `AT(y, views)` (projections of
    those views -> volume), callables on arrays of the kind of `b` [N, H, W]; `views` is a list of ints.  `subsets` is a list of
    view lists, visited in its order (`subset_order`).  See the module docstring for the iteration.  `callback(k, x,
    residual_norm)` runs after every iteration.  Returns (x, residual_norms)."""
    relax, relax_red, n_iter = _check_os_sart(relax, relax_red, n_iter)
    subsets = [[int(v) for v in s] for s in subsets]
    N = int(b.shape[0])
    if not subsets or any(not s for s in subsets) or any(not (0 <= v < N) for s in subsets for v in s):
        raise ValueError(f"os_sart: subsets must be non-empty lists of view indices in [0, {N}), got {subsets}")
    xp, clamp = _namespace(b)
    C = [_inverse_where_positive(AT(xp.ones_like(b[s]), s), xp) for s in subsets]
    R = _inverse_where_positive(A(xp.ones_like(C[0]), list(range(N))), xp)
    x = xp.zeros_like(C[0]) if x0 is None else x0 + xp.zeros_like(C[0])       # a copy: the caller's x0 stays as it is
    beta, norms = relax, []
    for k in range(n_iter):
        total = 0.0
        for s, Cs in zip(subsets, C):
            Rs = R[s]
            r = b[s] - A(x, s)
            total += float((Rs * r * r).sum(dtype=xp.float64))
            x = x + beta * (Cs * AT(Rs * r, s))
            if nonneg:
                x = clamp(x, 0, None)
        norms.append(math.sqrt(total))
        beta *= relax_red
        if callback is not None:
            callback(k, x, norms[-1])
    return x, norms


def os_sart(projections, geo, angles, n_iter=20, n_subsets=None, order="angular-distance", relax=1.0, relax_red=1.0, nonneg=True,
            x0=None, callback=None, weight_cache_bytes=2 << 30, seed=0, deterministic=False, kind="interpolated"):
    """OS-SART reconstruction of `projections` [N, H, W] (float32, on the GPU) taken with `geo` (ConeGeometry) at `angles` ->
    (float32 volume of geo.nVoxel on the projections' device, residual norms).  `n_subsets=None` is one view per subset (SART);
    the subsets and their order come from `subset_order(angles, n_subsets, order, seed)`.  The iteration of `os_sart_operators`,
    run directly on the subset kernels of `sart`: per subset one residual launch, one paired back-projection and one update.
    If n_subsets volumes fit `weight_cache_bytes`, C_s is built on the subset's first visit and kept; otherwise the column sums
    are rebuilt on every visit in the same march as the numerator.  `callback(k, x, residual_norm)` sees the live volume.
    `deterministic=True` takes the atomic-free transpose for the numerator and the column sums on all three routes: two runs
    return the same bits and the same norms.  `kind="siddon"` runs the same three launches per subset on the ray-voxel intersection
    pair (naf_hip.h P8): R is the exact row sum of the fp32 matrix, taken in the residual's own walk; it cannot be deterministic."""
    import numpy as np
    import torch

    from . import sart
    _check_kind("os_sart", kind, deterministic)
    relax, relax_red, n_iter = _check_os_sart(relax, relax_red, n_iter)
    angles = np.asarray(angles, dtype=np.float64).reshape(-1)
    subsets = subset_order(angles, len(angles) if n_subsets is None else n_subsets, order, seed)
    most = max(len(s) for s in subsets)
    scan, x, transpose = _device_solve_setup("os_sart", projections, geo, angles, x0, deterministic, most, kind)
    lists = [sart.ViewList(s, scan.N, projections.device) for s in subsets]
    y = torch.empty(most, scan.H, scan.W, device=x.device, dtype=torch.float32)
    r = torch.empty_like(y)
    num = torch.zeros_like(x)
    cached = len(lists) * x.numel() * 4 <= int(weight_cache_bytes)
    C = [None] * len(lists)
    den = None if cached else torch.zeros_like(x)
    beta, norms = relax, []
    for k in range(n_iter):
        total = torch.zeros((), device=x.device, dtype=torch.float64)
        for s, views in enumerate(lists):
            ys, rs = sart.residual_scan(x, projections, geo, angles, views, y=y[:len(views)], r=r[:len(views)], scan=scan, kind=kind)
            total += (ys.double() * rs.double()).sum()
            if C[s] is not None:
                sart.backproject_scan(ys, geo, angles, views, num=num, **transpose)
                sart.update(x, num, C[s], beta, nonneg, den_is_reciprocal=True)
            elif cached:
                C[s] = torch.zeros_like(x)
                sart.backproject_scan(ys, geo, angles, views, num=num, den=C[s], **transpose)
                sart.update(x, num, C[s], beta, nonneg)
                C[s] = torch.where(C[s] > 0, 1.0 / C[s], torch.zeros_like(x))
            else:
                sart.backproject_scan(ys, geo, angles, views, num=num, den=den, **transpose)
                sart.update(x, num, den, beta, nonneg, zero_den=True)
        norms.append(math.sqrt(float(total)))
        beta *= relax_red
        if callback is not None:
            callback(k, x, norms[-1])
    return x, norms


def asd_pocs_operators(A, AT, b, n_iter, tv_descent, relax=1.0, relax_red=0.99, alpha=0.002, alpha_red=0.95, rmax=0.95, tv_steps=20,
                       nonneg=True, x0=None, callback=None):
    """ASD-POCS over `A`, `AT` (as in `sirt_operators`) and `tv_descent(x, step, n_steps)`, a callable that returns the volume after
    `n_steps` normalised TV descent steps of length `step` (a Python float) and leaves its argument as it is.  See the module
    docstring for the iteration.  `callback(k, x, entry)` runs after every iteration.  Returns (x, history): one dict per iteration
    with `residual` (dd), `dp`, `dg` and the `dtvg` and `beta` that iteration used."""
    relax, relax_red, alpha, alpha_red, rmax = float(relax), float(relax_red), float(alpha), float(alpha_red), float(rmax)
    for name, value in (("relax", relax), ("relax_red", relax_red), ("alpha_red", alpha_red), ("rmax", rmax)):
        if not (0.0 < value <= 1.0):
            raise ValueError(f"asd_pocs: {name} must be in (0, 1], got {value}")
    if not (alpha > 0.0) or not math.isfinite(alpha):
        raise ValueError(f"asd_pocs: alpha must be > 0 and finite, got {alpha}")
    tv_steps = int(tv_steps)
    if tv_steps < 0:
        raise ValueError(f"asd_pocs: tv_steps must be >= 0, got {tv_steps}")
    n_iter = _check_n_iter("asd_pocs", n_iter)
    xp, clamp = _namespace(b)
    R, C, x = _weights_and_start(A, AT, b, x0, xp)
    beta, dtvg, history = relax, 0.0, []
    for k in range(n_iter):
        x_prev = x
        x = x + beta * (C * AT(R * (b - A(x))))
        if nonneg:
            x = clamp(x, 0, None)
        dp, dd = _norm(x - x_prev, xp), _norm(A(x) - b, xp)
        if k == 0:
            dtvg = alpha * dp
        entry = {"residual": dd, "dp": dp, "dg": 0.0, "dtvg": dtvg, "beta": beta}
        beta *= relax_red
        if tv_steps > 0:
            x_data = x
            x = tv_descent(x, dtvg, tv_steps)
            entry["dg"] = _norm(x - x_data, xp)
        if entry["dg"] > rmax * dp and dd > 0:
            dtvg *= alpha_red
        history.append(entry)
        if callback is not None:
            callback(k, x, entry)
    return x, history


def asd_pocs(projections, geo, angles, n_iter=50, relax=1.0, relax_red=0.99, alpha=0.002, alpha_red=0.95, rmax=0.95, tv_steps=20,
             tv_eps=1e-8, nonneg=True, x0=None, callback=None, views_per_call=None, deterministic=False, kind="interpolated"):
    """ASD-POCS reconstruction of `projections` [N, H, W] (float32, on the GPU) taken with `geo` (ConeGeometry) at `angles` ->
    (float32 volume of geo.nVoxel on the projections' device, history).  The data step is `sirt`'s update, the TV step
    `tv.tv_descent` with `tv_eps`; see the module docstring and `asd_pocs_operators`.  `deterministic=True` takes the atomic-free
    transpose: two runs return the same bits and the same history.  `kind="siddon"` runs the data step on the ray-voxel
    intersection pair (naf_hip.h P6 / P7); it cannot be deterministic."""
    from . import tv
    A, AT = _scan_operators(geo, angles, views_per_call, deterministic, projections.device, kind, "asd_pocs")
    scratch = []

    def descend(x, step, n_steps):
        if not scratch:
            scratch.append(x.new_empty(x.shape))
        out = x.clone()
        tv.tv_descent(out, step, n_steps, eps=tv_eps, scratch=scratch[0])
        return out

    return asd_pocs_operators(A, AT, projections, n_iter, descend, relax=relax, relax_red=relax_red, alpha=alpha, alpha_red=alpha_red,
                              rmax=rmax, tv_steps=tv_steps, nonneg=nonneg, x0=x0, callback=callback)


def _check_fista_tv(n_iter, lam):
    n_iter, lam = _check_n_iter("fista_tv", n_iter), float(lam)
    if not math.isfinite(lam) or lam < 0.0:
        raise ValueError(f"fista_tv: lam must be >= 0 and finite, got {lam}")
    return n_iter, lam


def _next_t(t):
    return (1.0 + math.sqrt(1.0 + 4.0 * t * t)) / 2.0


def fista_tv_operators(A, AT, b, n_iter, prox, lam, nonneg=True, x0=None, callback=None):
    """FISTA on F(x) = 1/2 ||A x - b||_R^2 + lam TV(x) (x >= 0 if `nonneg`) over `A`, `AT` (as in `sirt_operators`) and
    `prox(z, t, nonneg)`, a callable that returns prox_{t TV}(z), restricted to x >= 0 if `nonneg`, and leaves z as it is.  See the
    module docstring for the iteration.  `callback(k, x, residual_norm)` runs after every iteration.  Returns (x, norms) with
    norms[k] = ||b - A y_k||_R taken at the extrapolated point y_k (y_0 = x0), which costs no extra projection; it is not the
    residual of the returned iterates x_k."""
    n_iter, lam = _check_fista_tv(n_iter, lam)
    xp, _ = _namespace(b)
    R, _, x = _weights_and_start(A, AT, b, x0, xp)
    L = float(AT(xp.ones_like(b)).max())                        # max (A^T 1) >= ||A^T R A||_2
    if not L > 0.0:
        raise ValueError(f"fista_tv: max(A^T 1) must be > 0, got {L}: no ray meets the volume")
    y, t, norms = x, 1.0, []
    for k in range(n_iter):
        res = b - A(y)
        norms.append(math.sqrt(float((R * res * res).sum(dtype=xp.float64))))
        x_next = prox(y + AT(R * res) / L, lam / L, nonneg)
        t_next = _next_t(t)
        y = x_next + ((t - 1.0) / t_next) * (x_next - x)
        x, t = x_next, t_next
        if callback is not None:
            callback(k, x, norms[-1])
    return x, norms


DEFAULT_FISTA_TV_LAMBDA = 1e-4          # DESIGN.md section 18's sweep on the synthetic chest scan


def fista_tv(projections, geo, angles, n_iter=30, lam=DEFAULT_FISTA_TV_LAMBDA, tv_iters=20, nonneg=True, x0=None, callback=None,
             deterministic=False, kind="interpolated"):
    """FISTA-TV reconstruction of `projections` [N, H, W] (float32, on the GPU) taken with `geo` (ConeGeometry) at `angles` ->
    (float32 volume of geo.nVoxel on the projections' device, residual norms at the extrapolated points).  The iteration of
    `fista_tv_operators` on the kernels: per iteration one `sart.residual_scan` and one `sart.backproject_scan` over all views
    (the first also returns A^T 1, whose maximum is L) and `tv.tv_prox` with `tv_iters` dual iterations, the dual carried from one
    iteration to the next as a warm start.  `lam` is the weight of TV in F (the module docstring; the default is DESIGN.md section
    18's).  `callback(k, x, residual_norm)` reads the norm back, which otherwise happens once at the end.
    `deterministic=True` takes the atomic-free transpose: two runs return the same bits and the same norms.  `kind="siddon"` runs
    the two scan launches on the ray-voxel intersection pair (naf_hip.h P8); with R = 1 / (A 1) the exact row sum of the fp32 matrix,
    A^T R A 1 = A^T 1 holds for that matrix itself and L stays a rigorous bound.  It cannot be deterministic."""
    import torch

    from . import sart, tv
    _check_kind("fista_tv", kind, deterministic)
    n_iter, lam = _check_fista_tv(n_iter, lam)
    tv_iters = int(tv_iters)
    if tv_iters < 0:
        raise ValueError(f"fista_tv: tv_iters must be >= 0, got {tv_iters}")
    scan, x, transpose = _device_solve_setup("fista_tv", projections, geo, angles, x0, deterministic, kind=kind)
    yw = torch.empty(scan.N, scan.H, scan.W, device=x.device, dtype=torch.float32)
    res = torch.empty_like(yw)
    num = torch.zeros_like(x)
    dual = torch.zeros((3, *scan.dims), device=x.device, dtype=torch.float32)
    y, t, L, norms = x, 1.0, None, []
    for k in range(n_iter):
        sart.residual_scan(y, projections, geo, angles, None, y=yw, r=res, scan=scan, kind=kind)  # yw = R ⊙ res
        norms.append((yw.double() * res.double()).sum())
        if L is None:
            den = torch.zeros_like(x)
            sart.backproject_scan(yw, geo, angles, None, num=num, den=den, **transpose)
            L = float(den.max())
            del den
            if not L > 0.0:
                raise ValueError(f"fista_tv: max(A^T 1) must be > 0, got {L}: no ray meets the volume")
        else:
            sart.backproject_scan(yw, geo, angles, None, num=num.zero_(), **transpose)
        x_next, dual = tv.tv_prox(torch.add(y, num, alpha=1.0 / L), lam / L, tv_iters, nonneg, dual=dual, return_dual=True)
        t_next = _next_t(t)
        y = torch.add(x_next, x_next - x, alpha=(t - 1.0) / t_next)
        x, t = x_next, t_next
        if callback is not None:
            callback(k, x, math.sqrt(float(norms[-1])))
    return x, [math.sqrt(float(v)) for v in norms]


def cgls_operators(A, AT, b, n_iter, weights=None, x0=None, nonneg=True, callback=None):
    """CGLS on 1/2 ||b - A x||_W^2 over `A`, `AT` (as in `sirt_operators`); `weights` is an array of `b`'s kind with one weight
    >= 0 per ray, None for all ones.  See the module docstring for the iteration.  `callback(k, x, residual_norm)` runs after every
    iteration that took a step.  Returns (x, norms) with norms[k] = ||r_k||_W, r the recurred residual; the list ends with the norm
    of the iteration that stopped, if one did (gamma or delta not > 0)."""
    n_iter = _check_n_iter("cgls", n_iter)
    xp, clamp = _namespace(b)
    w = weights

    def weighted(d):
        return d if w is None else w * d

    def wsum(d):
        return float((d * d if w is None else w * d * d).sum(dtype=xp.float64))

    if x0 is None:
        r = b + xp.zeros_like(b)
        s = AT(weighted(r))
        x = xp.zeros_like(s)
    else:
        r = b - A(x0)
        s = AT(weighted(r))
        x = x0 + xp.zeros_like(s)                                # a copy: the caller's x0 stays as it is
    p = s
    gamma = float((s * s).sum(dtype=xp.float64))
    norms = []
    for k in range(n_iter):
        norms.append(math.sqrt(wsum(r)))
        q = A(p)
        delta = wsum(q)
        if not gamma > 0.0 or not delta > 0.0:
            break
        alpha = gamma / delta
        x = x + alpha * p
        r = r - alpha * q
        s = AT(weighted(r))
        gamma_next = float((s * s).sum(dtype=xp.float64))
        p = s + (gamma_next / gamma) * p
        gamma = gamma_next
        if callback is not None:
            callback(k, x, norms[-1])
    if nonneg:
        x = clamp(x, 0, None)
    return x, norms


def cgls(projections, geo, angles, n_iter=15, weights=None, x0=None, nonneg=True, callback=None, views_per_call=None,
         deterministic=False, info=None, kind="interpolated"):
    """CGLS reconstruction of `projections` [N, H, W] (float32, on the GPU) taken with `geo` (ConeGeometry) at `angles` ->
    (float32 volume of geo.nVoxel on the projections' device, residual norms ||r_k||_W).  The iteration of `cgls_operators`:
    A is `projector.project_scan`, A^T `sart.backproject_scan` over all views into a zeroed volume, and the rest three HIP launches
    per iteration (`cgls_kernels.wdot`, `residual_step`, `direction_step`) that keep alpha, beta and the norms on the device, so
    the whole solve is queued without a host read-back; the history and the stop mark are read once at the end, or per iteration
    when a `callback(k, x, residual_norm)` is given (it sees the live, unclamped volume).  `weights` is a float32 [N, H, W] tensor
    on the projections' device, >= 0 and finite (`ray_length_weights`, `pwls_weights`, a mask, or their product).  The norms are cut
    at the iteration that stopped, if one did; `info`, a dict, receives `stopped_at` (that iteration, or None).
    `deterministic=True` takes the atomic-free transpose: with the fixed-order fp64 sums two runs return the same bits and norms.
    `kind="siddon"` takes the ray-voxel intersection pair (naf_hip.h P6 / P7): A is `projector.project_scan(kind="siddon")` and A^T
    `projector.backproject_scan(kind="siddon")` into a zeroed volume, the exact transpose CGLS rests on; the three vector launches
    and the single read-back stay as they are.  It cannot be deterministic."""
    import torch

    from . import _abi, cgls_kernels as K, projector, sart
    n_iter = _check_n_iter("cgls", n_iter)
    _check_kind("cgls", kind, deterministic)
    scan, x, transpose = _device_solve_setup("cgls", projections, geo, angles, x0, deterministic)
    _abi.check_stack(projections, (scan.N, scan.H, scan.W), None, "cgls", "projections")
    w = weights
    if w is not None:
        _abi.check_stack(w, (scan.N, scan.H, scan.W), projections, "cgls", "weights")
        if bool(((w < 0) | ~torch.isfinite(w)).any()):
            raise ValueError("cgls: weights must be >= 0 and finite")

    def A(v):
        return projector.project_scan(v, geo, angles, views_per_call=views_per_call, scan=scan, kind=kind)

    def AT(v, zeroed):
        if kind == "siddon":
            return projector.backproject_scan(v, geo, angles, views_per_call=views_per_call, out=zeroed, scan=scan, kind=kind)
        return sart.backproject_scan(v, geo, angles, None, num=zeroed, **transpose)

    r = projections.clone() if x0 is None else projections - A(x)
    ws = K.Workspace(max(r.numel(), x.numel()), n_iter, projections.device)
    y = r.clone() if w is None else w * r
    s = AT(y, torch.zeros_like(x))
    p = s.clone()
    K.wdot(s, None, K.SLOT_GAMMA[0], ws)
    stopped = None
    for k in range(n_iter):
        q = A(p)
        K.wdot(q, w, K.SLOT_DELTA, ws)
        K.residual_step(r, q, w, y, k, ws)
        AT(y, s.zero_())
        K.wdot(s, None, K.SLOT_GAMMA[(k + 1) & 1], ws)
        K.direction_step(x, p, s, k, ws)
        if callback is not None:
            stopped = ws.stopped_at()
            if stopped is not None:
                break
            callback(k, x, math.sqrt(float(ws.history()[k])))
    history = ws.scalars.tolist()                               # the one read-back of a solve without a callback
    mark = int(history[K.SLOT_STOPPED])
    stopped = mark - 1 if mark > 0 else None
    kept = n_iter if stopped is None else stopped + 1
    norms = [math.sqrt(v) if v >= 0 else math.nan for v in history[K.HISTORY:K.HISTORY + kept]]
    if info is not None:
        info["stopped_at"] = stopped
    if nonneg:
        x.clamp_(min=0)
    return x, norms


def ray_length_weights(geo, angles, device, views_per_call=None, kind="interpolated"):
    """R = 1 / (A 1) where A 1 > 0, else 0: float32 [N, H, W] on `device`, the ray weights of SIRT and of FISTA-TV's data term.
    A is the projector of `kind`; with "siddon" A 1 is the ray's chord length through the volume."""
    import torch

    from . import projector
    projector.check_kind(kind, "ray_length_weights")
    ones = torch.ones(tuple(int(v) for v in geo.nVoxel), device=device, dtype=torch.float32)
    return _inverse_where_positive(projector.project_scan(ones, geo, angles, views_per_call=views_per_call, kind=kind), torch)


def pwls_weights(projections):
    """exp(-b): the expected photon count of a ray relative to the unattenuated beam under `dataset.add_noise`'s transmission
    model, which is the inverse variance of the line integral up to one factor (penalised weighted least squares)."""
    xp, _ = _namespace(projections)
    return xp.exp(-projections)


def _check_align(n_outer, tol):
    n_outer, tol = int(n_outer), float(tol)
    if n_outer < 0:
        raise ValueError(f"align: n_outer must be >= 0, got {n_outer}")
    if not tol >= 0.0:
        raise ValueError(f"align: tol must be >= 0, got {tol}")
    return n_outer, tol


def align_operators(A, solve, b, shift_views, estimate_shifts, n_outer=5, center=True, warm=True, tol=0.02, callback=None):
    """Reprojection alignment (the joint iteration of tomopy's `align_joint`) as array code over callables, on arrays of `b`'s kind
    ([N, H, W]; torch tensors on any device, numpy arrays).  A view's shift is (du, dv) in pixels, `shifts[N, 2] = (du, dv)`, and
    the measured view is the ideal one translated by +shift (align.py).

        A(x)                   volume -> projections [N, H, W]
        solve(a, x0)           projections, start volume or None -> (volume, the solver's last residual norm)
        shift_views(b, S)      the views of b with the shifts S undone
        estimate_shifts(a, p)  -> (delta [N, 2], flags [N]): the translation of every view of a against p; a flagged view comes
                               with the step it is to take (its integer shift, or none at all)

        S = 0
        for k in range(n_outer):
            a = shift_views(b, S)                    always from the original b: blur never accumulates
            x, residual = solve(a, x if warm and k > 0 else None)
            delta, flags = estimate_shifts(a, A(x))
            S += delta
            if center: S -= mean(S) per axis         a common translation is a gauge of the volume, not of the views
            stop when max |delta| < tol              one host read per outer iteration

    `callback(k, x, entry)` runs after every outer iteration with that iteration's reconstruction.  Returns (aligned, S, history):
    `aligned = shift_views(b, S)` for the final S and one dict per outer iteration with `rms` (sqrt of the mean over the views of
    |delta|^2), `max` (the largest |component| of delta), `flagged` (views with a non-zero flag) and `residual`."""
    n_outer, tol = _check_align(n_outer, tol)
    xp, _ = _namespace(b)
    N = int(b.shape[0])
    S = b.new_zeros((N, 2)) if xp.__name__ == "torch" else xp.zeros((N, 2), dtype=b.dtype)
    x, history = None, []
    for k in range(n_outer):
        a = shift_views(b, S)
        x, residual = solve(a, x if warm and k > 0 else None)
        delta, flags = estimate_shifts(a, A(x))
        S = S + delta
        if center:
            S = S - S.mean(0)
        biggest = float(abs(delta).max()) if N else 0.0
        entry = {"rms": math.sqrt(float((delta * delta).sum(dtype=xp.float64)) / max(N, 1)), "max": biggest,
                 "flagged": int((flags != 0).sum()), "residual": residual}
        history.append(entry)
        if callback is not None:
            callback(k, x, entry)
        if biggest < tol:
            break
    return shift_views(b, S), S, history


ALIGN_SOLVERS = ("sirt", "cgls", "os_sart", "fista_tv", "asd_pocs")


def align_projections(projections, geo, angles, n_outer=5, max_shift=4, solver="sirt", n_iter=20, center=True, warm=True, tol=0.02,
                      weights=None, kind="interpolated", deterministic=False, callback=None, **solver_kwargs):
    """Aligns `projections` [N, H, W] (float32, on the GPU) taken with `geo` at `angles` to their own reprojection: per-view detector
    translations of up to `max_shift` pixels per outer iteration (an int, or (Ru, Rv); at most 16) are found and undone ->
    (aligned [N, H, W], shifts float32 [N, 2] = (du, dv), history).  The iteration of `align_operators`: `solver` (one of
    ALIGN_SOLVERS, run for `n_iter` iterations with `**solver_kwargs`, warm-started from the previous outer iteration's volume if
    `warm`) reconstructs, `projector.project_scan` reprojects, `align.estimate_shifts` finds every view's translation and
    `align.shift_views` resamples the ORIGINAL views with the accumulated shifts.  `weights` (float32 [N, H, W] >= 0, None for all
    ones) weigh the squared differences of the shift search, so a mask leaves pixels out; `solver="cgls"` is given them too.
    `kind` and `deterministic` go to the solver and the projector unchanged, and what those refuse stays refused.  The alignment
    kernels add no atomics: with `deterministic=True` on the interpolated pair two runs return the same bits.  `callback(k, x,
    entry)` sees every outer iteration's reconstruction."""
    import torch

    from . import align, projector
    solvers = {"sirt": sirt, "cgls": cgls, "os_sart": os_sart, "fista_tv": fista_tv, "asd_pocs": asd_pocs}
    if solver not in solvers:
        raise ValueError(f"align_projections: solver must be one of {ALIGN_SOLVERS}, got {solver!r}")
    if not isinstance(projections, torch.Tensor) or not projections.is_cuda:
        raise RuntimeError("align_projections: projections must be a CUDA/HIP tensor (no CPU path)")
    _check_align(n_outer, tol)
    _check_kind("align_projections", kind, deterministic)
    scan = projector.Scan(geo, angles, projections.device)
    shape = (scan.N, scan.H, scan.W)
    if projections.dtype != torch.float32 or tuple(projections.shape) != shape or not projections.is_contiguous():
        raise ValueError(f"align_projections: projections must be contiguous float32 {shape}, got {projections.dtype} "
                         f"{tuple(projections.shape)}")
    align.window(max_shift, scan.H, scan.W, "align_projections")
    if solver == "cgls" and weights is not None:
        solver_kwargs = {"weights": weights, **solver_kwargs}
    workspace = align.scores_workspace(scan.N, scan.H, scan.W, max_shift, projections.device)

    def solve(a, x0):
        x, hist = solvers[solver](a, geo, angles, n_iter=n_iter, x0=x0, kind=kind, deterministic=deterministic, **solver_kwargs)
        last = hist[-1] if hist else math.nan
        return x, float(last["residual"] if isinstance(last, dict) else last)

    def A(x):
        return projector.project_scan(x, geo, angles, kind=kind, scan=scan)

    def estimate(a, p):
        return align.estimate_shifts(a, p, max_shift, weights, workspace)

    return align_operators(A, solve, projections, align.shift_views, estimate, n_outer=n_outer, center=center, warm=warm, tol=tol,
                           callback=callback)


def fdk_weights(geo, angles, filter="ram-lak"):
    """What `filter_rows` needs for an FDK reconstruction of a scan of `geo` at `angles`, as float32 numpy arrays, each formed in
    float64 and rounded once: (taps [W], pre [H, W] or None, post [H, W] or None, view_scale [N]).  See the module docstring."""
    from . import filter as F
    import numpy as np
    if geo.mode not in ("cone", "parallel"):
        raise ValueError(f"fdk: mode must be 'cone' or 'parallel', got {geo.mode!r}")
    if float(geo.tilt_angle) != 0.0:
        raise ValueError(f"fdk: a tilted (laminographic) scan is not supported, got tilt_angle {geo.tilt_angle}: its constant and "
                         "filter direction are not verified")
    W = int(geo.nDetector[0])
    du, dv = float(geo.dDetector[0]), float(geo.dDetector[1])
    dV = float(np.prod(np.asarray(geo.dVoxel, dtype=np.float64)))
    w = F.view_weights(angles) * (du * dv / dV)
    if geo.mode == "parallel":
        return F.ramp_taps(W, du, filter), None, None, w.astype(np.float32)
    DSO, DSD = float(geo.DSO), float(geo.DSD)
    cos = F.cosine_weights(geo).astype(np.float32)
    return F.ramp_taps(W, du * DSO / DSD, filter), cos, cos, (w * (DSO / DSD) ** 2).astype(np.float32)


SHORT_SCAN = (None, "parker")


def fdk_short_scan_weights(geo, angles, filter="ram-lak"):
    """`fdk_weights` for a short scan, with Parker's weights: (taps [W], pre, post, view_scale [N], col [N, W]), float32 numpy
    arrays, each formed in float64 and rounded once.  `col` is `filter.parker_weights`, whose refusals apply.  A ray pair's weights
    sum to 1 where a full scan gives each 1/2 of 2 pi, so view i stands for its own angular step: w_i = gap_i
    (`filter.view_gaps`), which is `view_weights` * covered range / pi, times `fdk_weights`' constants."""
    from . import filter as F
    import numpy as np
    taps, pre, post, _ = fdk_weights(geo, angles, filter)
    col = F.parker_weights(geo, angles)
    du, dv = float(geo.dDetector[0]), float(geo.dDetector[1])
    dV = float(np.prod(np.asarray(geo.dVoxel, dtype=np.float64)))
    w = F.view_gaps(angles) * (du * dv / dV)
    if geo.mode == "cone":
        w = w * (float(geo.DSO) / float(geo.DSD)) ** 2
    return taps, pre, post, w.astype(np.float32), col.astype(np.float32)


def fdk_operators(AT, filter_rows, b, geo, angles, filter="ram-lak", nonneg=False, short_scan=None):
    """FDK over the transpose `AT` (projections -> volume, as in `sirt_operators`) and a row filter
    `filter_rows(b, taps, pre, post, view_scale)` that takes the float32 numpy arrays of `fdk_weights` and returns the filtered
    projections as an array of `b`'s kind.  Returns AT(filter_rows(b, ...)), clamped at 0 if `nonneg`.  With
    `short_scan="parker"` the arrays are those of `fdk_short_scan_weights` and the filter is called with a sixth, `col` [N, W]."""
    if short_scan not in SHORT_SCAN:
        raise ValueError(f"fdk: short_scan must be one of {SHORT_SCAN}, got {short_scan!r}")
    if len(b.shape) != 3 or int(b.shape[0]) != len(angles):
        raise ValueError(f"fdk: projections must be [N, H, W] with one view per angle, got {tuple(b.shape)} for {len(angles)} angles")
    if short_scan is None:
        taps, pre, post, view_scale = fdk_weights(geo, angles, filter)
        x = AT(filter_rows(b, taps, pre, post, view_scale))
    else:
        x = AT(filter_rows(b, *fdk_short_scan_weights(geo, angles, filter)))
    if nonneg:
        x = _namespace(b)[1](x, 0, None)
    return x


def fdk(projections, geo, angles, filter="ram-lak", nonneg=False, views_per_call=None, deterministic=False, short_scan=None):
    """FDK reconstruction of `projections` [N, H, W] (float32, on the GPU) taken with `geo` (ConeGeometry, cone or untilted parallel
    beam) at `angles` -> float32 volume of geo.nVoxel on the projections' device.  One pass of `filter.filter_rows` and one of
    `projector.backproject_scan`; see the module docstring.  `deterministic=True` takes the atomic-free transpose: two runs return
    the same bits.  `short_scan="parker"` weighs the rays of a scan of pi .. 2 pi by Parker's weights, inside the filter's pass."""
    import torch

    from . import filter as F

    def on_device(a):
        return None if a is None else torch.tensor(a, device=projections.device)

    def rows(b, taps, pre, post, view_scale, col=None):
        return F.filter_rows(b, on_device(taps), on_device(pre), on_device(post), on_device(view_scale), on_device(col))

    _, AT = _scan_operators(geo, angles, views_per_call, deterministic, projections.device)
    return fdk_operators(AT, rows, projections, geo, angles, filter=filter, nonneg=nonneg, short_scan=short_scan)


def _check_lamino(geo, angles, who="lamino_fbp"):
    """The scans laminographic FBP is derived for: a parallel beam tilted strictly between 0 and 90 degrees, at least two finite
    view angles, a full turn."""
    from . import filter as F
    import numpy as np
    if geo.mode != "parallel":
        raise ValueError(f"{who}: mode must be 'parallel', got {geo.mode!r}: cone-beam laminography is not supported")
    tilt = float(geo.tilt_angle)
    if tilt == 0.0:
        raise ValueError(f"{who}: tilt_angle is 0, which is plain parallel-beam CT: use fdk")
    if not 0.0 < tilt < 90.0:
        raise ValueError(f"{who}: tilt_angle must lie strictly between 0 and 90 degrees, got {geo.tilt_angle}")
    a = np.asarray(angles, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{who}: the view angles must be finite")
    if a.size < 2:
        raise ValueError(f"{who}: at least two views are needed, got {a.size}")
    covered = F.covered_range(a)
    if covered < 2.0 * math.pi - 0.5 * covered / a.size:
        ordered = np.sort(a)
        gap = max(float(np.max(np.diff(ordered))), 2.0 * math.pi - float(ordered[-1] - ordered[0]))      # the wrap-around gap too
        raise ValueError(f"{who}: {a.size} views cover {math.degrees(covered):.1f} degrees (largest gap {math.degrees(gap):.1f} degrees, the one across the turn's end included), "
                         "less than a full turn: every frequency outside the missing cone must be seen twice, and no short-scan weights "
                         "are derived for a tilted axis")
    return math.radians(tilt)


def lamino_fbp_weights(geo, angles, filter="ram-lak"):
    """What `filter_rows` needs for a laminographic FBP of a tilted parallel-beam scan of `geo` at `angles`, as `fdk_weights` returns
    it: (taps [W], None, None, view_scale [N]), float32 numpy arrays formed in float64 and rounded once.  The ramp runs along the
    detector rows with tap spacing du, there are no cosine weights, and view_scale[i] = w_i cos(tilt) du dv / dV with sum w_i = pi over
    the full turn (`filter.view_weights`); DESIGN.md section 35.  ValueError for a cone beam, tilt 0 (use `fdk`), a tilt outside
    (0, 90) degrees, non-finite angles, fewer than two views and views that cover less than a full turn."""
    from . import filter as F
    import numpy as np
    tau = _check_lamino(geo, angles)
    du, dv = float(geo.dDetector[0]), float(geo.dDetector[1])
    dV = float(np.prod(np.asarray(geo.dVoxel, dtype=np.float64)))
    w = F.view_weights(angles) * (math.cos(tau) * du * dv / dV)
    return F.ramp_taps(int(geo.nDetector[0]), du, filter), None, None, w.astype(np.float32)


def lamino_fbp_operators(AT, filter_rows, b, geo, angles, filter="ram-lak", nonneg=False):
    """Laminographic FBP over the transpose `AT` and a row filter `filter_rows(b, taps, pre, post, view_scale)`, as `fdk_operators`:
    AT(filter_rows(b, *lamino_fbp_weights(...))), clamped at 0 if `nonneg`."""
    if len(b.shape) != 3 or int(b.shape[0]) != len(angles):
        raise ValueError(f"lamino_fbp: projections must be [N, H, W] with one view per angle, got {tuple(b.shape)} for {len(angles)} angles")
    x = AT(filter_rows(b, *lamino_fbp_weights(geo, angles, filter)))
    if nonneg:
        x = _namespace(b)[1](x, 0, None)
    return x


def lamino_window(geo):
    """How much of a tilted parallel-beam scan's volume the projector pair's near / far window holds -> (kept, reach), metres along
    the rays from the rotation centre: `kept` is the smaller of the depths the window keeps behind and in front of it, `reach` the
    depth of the volume's furthest corner.  `geometry.get_near_far` places the window about DSO and ignores the tilt, while the
    beam's source plane stands at DSO / cos(tilt); where reach > kept, the voxels deeper than `kept` are cut out of some views' rays
    by A and A^T alike."""
    import numpy as np

    from .geometry import get_near_far
    tau = math.radians(float(geo.tilt_angle))
    near, far = get_near_far(geo)
    source = float(geo.DSO) / math.cos(tau)
    half = 0.5 * np.asarray(geo.sVoxel, dtype=np.float64) + np.abs(np.asarray(geo.offOrigin, dtype=np.float64))
    reach = math.cos(tau) * math.hypot(half[0], half[1]) + math.sin(tau) * float(half[2])
    return min(float(far) - source, source - float(near)), reach


def lamino_fbp(projections, geo, angles, filter="ram-lak", nonneg=False, views_per_call=None, deterministic=False, out=None):
    """Filtered back-projection of a tilted-axis (laminographic) parallel-beam scan: `projections` [N, H, W] (float32, on the GPU)
    taken with `geo` at `angles` over a full turn -> float32 volume of geo.nVoxel on the projections' device (`out`, if given).  One
    pass of `filter.filter_rows` and one of `projector.backproject_scan`, as `fdk`; the frequencies inside the missing cone
    k_r < |k_z| tan(tilt) are not measured and stay zero.  `deterministic=True` takes the atomic-free gather transpose, which accepts
    the tilted beam: two runs return the same bits.  A voxel whose rays the scan's near / far window cuts (`geometry.get_near_far`
    ignores the tilt) receives fewer views, as it does from every solver on this pair: a warning says how deep the window reaches
    (`lamino_window`)."""
    import warnings

    import torch

    from . import filter as F
    from . import projector

    def on_device(a):
        return None if a is None else torch.tensor(a, device=projections.device)

    def rows(b, taps, pre, post, view_scale):
        return F.filter_rows(b, on_device(taps), on_device(pre), on_device(post), on_device(view_scale))

    _check_lamino(geo, angles)
    if not isinstance(projections, torch.Tensor) or not projections.is_cuda:
        raise RuntimeError("lamino_fbp: projections must be a CUDA/HIP tensor (no CPU path)")
    kept, reach = lamino_window(geo)
    if reach > kept:
        warnings.warn(f"lamino_fbp: the scan's near / far window keeps {kept * 1000:.1f} mm along the rays about the rotation centre "
                      f"and the volume reaches {reach * 1000:.1f} mm: voxels deeper than that receive fewer views (the window is "
                      "placed about DSO and ignores the tilt; a smaller DSO in the scan's geometry widens what it keeps)")
    scan = projector.Scan(geo, angles, projections.device)

    def AT(y):
        return projector.backproject_scan(y, geo, angles, views_per_call=views_per_call, out=out, method=_method(deterministic), scan=scan)

    x = lamino_fbp_operators(AT, rows, projections, geo, angles, filter=filter, nonneg=False)
    return x.clamp_(min=0) if nonneg else x


METAL_METHODS = ("li", "nmar")
NMAR_EPS_FRACTION = 1e-3                # eps of the normalised in-painting, as a fraction of the prior sinogram's maximum


def _check_metal(method, air, bone, grow):
    if method not in METAL_METHODS:
        raise ValueError(f"reduce_metal: method must be one of {METAL_METHODS}, got {method!r}")
    if method == "nmar":
        if air is None or bone is None:
            raise ValueError("reduce_metal: method 'nmar' needs air and bone, the thresholds of its prior")
        if not float(air) < float(bone):
            raise ValueError(f"reduce_metal: air must be below bone, got {air} and {bone}")
    if isinstance(grow, bool) or not isinstance(grow, int) or grow < 0:
        raise ValueError(f"reduce_metal: grow must be an int >= 0, got {grow!r}")


def reduce_metal_operators(A, inpaint, dilate, b, initial, threshold, method="li", air=None, bone=None, grow=1):
    """Metal artefact reduction by sinogram in-painting (metal.py) as array code over callables, on arrays of
    `b`'s kind ([N, H, W]; torch tensors on any device, numpy arrays).

        A(x)                         volume -> projections [N, H, W], float32
        inpaint(b, mask, prior, eps) -> (b with the masked pixels in-painted along their rows, counts [N, 2]); prior and eps are
                                     None for `method="li"`
        dilate(mask, grow)           a mask [N, H, W] grown by `grow` pixels along both detector axes -> uint8

        metal = initial > threshold                               the metal voxels of a first reconstruction
        trace = dilate(A(metal as float32) > 0, grow)             the pixels whose ray meets one
        "nmar":  prior = A(metal.prior_volume(initial, metal, air, bone));   eps = 1e-3 max(prior)
        corrected, counts = inpaint(b, trace, prior, eps)

    Returns (corrected, info) with info = {"metal": bool volume, "trace": uint8 [N, H, W], "counts": [N, 2], "initial": initial,
    "prior": the prior sinogram or None, "eps": eps or None}.  A prior sinogram with no positive value (air and bone leave nothing)
    is refused: it would normalise by eps everywhere."""
    from .metal import prior_volume
    _check_metal(method, air, bone, grow)
    xp, _ = _namespace(b)
    metal = initial > threshold
    trace = dilate(A(metal.float() if xp.__name__ == "torch" else metal.astype(xp.float32)) > 0, grow)
    prior, eps = None, None
    if method == "nmar":
        prior = A(prior_volume(initial, metal, air, bone))
        eps = NMAR_EPS_FRACTION * float(prior.max())
        if not eps > 0.0 or not math.isfinite(eps):
            raise ValueError(f"reduce_metal: the prior's sinogram has no finite positive maximum ({eps / NMAR_EPS_FRACTION}): nothing "
                             "of the first reconstruction lies at or above `air`")
    corrected, counts = inpaint(b, trace, prior, eps)
    return corrected, {"metal": metal, "trace": trace, "counts": counts, "initial": initial, "prior": prior, "eps": eps}


def reduce_metal(projections, geo, angles, threshold, method="li", air=None, bone=None, grow=1, initial=None, kind="interpolated",
                 views_per_call=None):
    """Metal artefact reduction of `projections` [N, H, W] (float32, on the GPU) taken with `geo` at `angles` -> (corrected [N, H, W],
    info): the iteration of `reduce_metal_operators` over `projector.project_scan` (of `kind`), `metal.inpaint_rows` and
    `metal.dilate`.  `method="li"` interpolates the sinogram itself, `"nmar"` the sinogram normalised by that of a prior volume with
    the thresholds `air` and `bone` (required then).  `threshold` separates metal in the first reconstruction `initial`
    (float32, geo.nVoxel, on the GPU); `initial=None` takes `fdk(projections, geo, angles)`, so a tilted scan is refused where `fdk`
    refuses it: pass a SIRT or CGLS volume as `initial` there.  `grow` widens the trace by that many detector pixels.  `projections`
    is left as it is."""
    import torch

    from . import _abi, metal, projector
    who = "reduce_metal"
    if not isinstance(projections, torch.Tensor) or not projections.is_cuda:
        raise RuntimeError(f"{who}: projections must be a CUDA/HIP tensor (no CPU path)")
    _check_metal(method, air, bone, grow)
    projector.check_kind(kind, who)
    scan = projector.Scan(geo, angles, projections.device)
    shape = (scan.N, scan.H, scan.W)
    if projections.dtype != torch.float32 or tuple(projections.shape) != shape or not projections.is_contiguous():
        raise ValueError(f"{who}: projections must be contiguous float32 {shape}, got {projections.dtype} {tuple(projections.shape)}")
    if initial is None:
        initial = fdk(projections, geo, angles, views_per_call=views_per_call)
    else:
        _abi.check_volume(initial, who, "initial")
        projector.check_geometry(initial, geo)

    def A(x):
        return projector.project_scan(x.contiguous(), geo, angles, views_per_call=views_per_call, kind=kind, scan=scan)

    def inpaint(b, mask, prior, eps):
        return metal.inpaint_rows(b, mask, prior=prior, eps=eps, counts=True)

    return reduce_metal_operators(A, inpaint, metal.dilate, projections, initial, threshold, method=method, air=air, bone=bone, grow=grow)


CENTER_METRICS = ("negativity", "sharpness")
# Cone scans that cover less than a full turn, by what the float64 rehearsal of DESIGN.md section 34 recovers: the key is
# `short_scan`, the value whether a planted 1.5 px offset came back within one candidate step at 64^3 (180 degrees in 50 views
# without weights: 2.5; with Parker's weights: 1.5 at 180 degrees, 1.0 at 220).
CENTER_CONE_SHORT_SCAN = {None: False, "parker": True}


def center_metric(angles):
    """The score `find_center` takes by default: "negativity" (its minimum) for a scan that covers less than a full turn less half a
    view step, where a wrong centre draws negative tuning forks, and "sharpness" (its maximum) for a full turn, where it doubles
    edges instead."""
    from . import filter as F
    import numpy as np
    theta = F.covered_range(angles)
    return "negativity" if theta < 2.0 * np.pi - 0.5 * theta / max(len(angles), 1) else "sharpness"


def parabola_vertex(x, y):
    """The abscissa of the vertex of the parabola through three points with equally spaced abscissae x[0] < x[1] < x[2]; x[1] where
    the points lie on a line."""
    curve = float(y[0]) - 2.0 * float(y[1]) + float(y[2])
    if curve == 0.0 or not math.isfinite(curve):
        return float(x[1])
    return float(x[1]) + 0.5 * (float(y[0]) - float(y[2])) / curve * (float(x[2]) - float(x[1]))


def _check_center(geo, angles, metric, rows, short_scan):
    from . import center
    from . import filter as F
    center.scalars(geo)                                            # mode, tilt, square slice
    if short_scan not in SHORT_SCAN:
        raise ValueError(f"find_center: short_scan must be one of {SHORT_SCAN}, got {short_scan!r}")
    if metric is not None and metric not in CENTER_METRICS:
        raise ValueError(f"find_center: metric must be one of {CENTER_METRICS} or None, got {metric!r}")
    if geo.mode == "cone":
        if rows is not None:
            raise ValueError("find_center: a cone beam is searched in its mid-plane only, rows must be None")
        if center_metric(angles) == "negativity" and not CENTER_CONE_SHORT_SCAN[short_scan]:
            raise ValueError(f"find_center: a cone scan that covers {math.degrees(F.covered_range(angles)):.1f} degrees, less than a full "
                             f"turn, with short_scan={short_scan!r} is not supported: the float64 rehearsal does not recover a planted "
                             "offset there (DESIGN.md section 34)")
    elif rows is not None:
        H = int(geo.nDetector[1])
        rows = [int(r) for r in rows]
        if not rows or any(r < 0 or r >= H for r in rows):
            raise ValueError(f"find_center: rows must be a non-empty list of detector rows below {H}, got {rows}")
    return rows


def center_rows(geo):
    """The detector rows a parallel-beam search takes by default: the central quarter, at most 8, evenly spread."""
    H = int(geo.nDetector[1])
    count = max(1, min(8, H // 4))
    first = (H - count) // 2
    return list(range(first, first + count))


def find_center_operators(filter_rows, slices, metrics, b, geo, angles, candidates, metric, rows, filter="ram-lak", short_scan=None):
    """The centre-of-rotation search (center.py) as array code over callables, on arrays of `b`'s kind
    ([N, H, W]; torch tensors on any device, numpy arrays).

        filter_rows(b, taps, pre, post, view_scale[, col])   the row filter of `fdk_operators`, here on the rows that are used only
        slices(q, offsets)      filtered rows [S, N, W], K candidate offsets in metres -> slices [S, K, n, n]
        metrics(f)              slices -> [S, K, 2] = (negativity, sharpness)

        cone:      q = the filtered row at v = 0 (`center.midplane_rows`), S = 1;   `rows` must be None
        parallel:  q = the filtered rows `rows` (None: `center_rows`), one slice each
        scores[k] = sum over the slices of the `metric` ("negativity" or "sharpness") of candidate k

    `candidates` are in pixels of the detector.  Returns scores [K], an array of the kind `metrics` returns.  A tilted scan is
    refused where `fdk_weights` refuses it, a cone scan under a full turn by `CENTER_CONE_SHORT_SCAN`."""
    import numpy as np

    from . import center
    rows = _check_center(geo, angles, metric, rows, short_scan)
    if metric not in CENTER_METRICS:
        raise ValueError(f"find_center: metric must be one of {CENTER_METRICS}, got {metric!r}")
    if len(b.shape) != 3 or int(b.shape[0]) != len(angles):
        raise ValueError(f"find_center: projections must be [N, H, W] with one view per angle, got {tuple(b.shape)} for {len(angles)} angles")
    cand = np.asarray(candidates, dtype=np.float64).reshape(-1)
    if not 1 <= cand.size <= center.MAX_K:
        raise ValueError(f"find_center: 1 .. {center.MAX_K} candidates are needed, got {cand.size}")
    weights = fdk_weights(geo, angles, filter) if short_scan is None else fdk_short_scan_weights(geo, angles, filter)
    taps, pre, post, rest = weights[0], weights[1], weights[2], weights[3:]
    xp, _ = _namespace(b)
    blend = None
    if geo.mode == "cone":
        r0, r1, blend = center.midplane_rows(geo)
        rows = [r0, r1]
    elif rows is None:
        rows = center_rows(geo)
    sub = b[:, rows]
    pre = None if pre is None else np.ascontiguousarray(pre[rows])
    post = None if post is None else np.ascontiguousarray(post[rows])
    filtered = filter_rows(sub, taps, pre, post, *rest)
    if blend is None:
        q = xp.swapaxes(filtered, 0, 1)
    else:
        q = ((1.0 - blend) * filtered[:, 0] + blend * filtered[:, 1])[None]
    score = metrics(slices(q, cand * float(geo.dDetector[0])))
    return score[:, :, CENTER_METRICS.index(metric)].sum(0)


def pick_center(candidates, scores, metric, refine=True):
    """The best candidate of a score curve (host arrays): the minimum of "negativity", the maximum of "sharpness" ->
    (offset_px, best index, edge).  `edge`: the best is the first or the last candidate, so the true centre may lie outside the
    grid; nothing is refined then.  Otherwise `refine` takes the vertex of the parabola through the best candidate and its two
    neighbours, kept within half a step of the best."""
    import numpy as np
    cand, s = np.asarray(candidates, dtype=np.float64), np.asarray(scores, dtype=np.float64)
    if cand.shape != s.shape or cand.ndim != 1 or cand.size < 1:
        raise ValueError(f"find_center: one score per candidate is needed, got {s.shape} for {cand.shape}")
    if not np.all(np.isfinite(s)):
        raise ValueError("find_center: a score is not finite")
    best = int(np.argmin(s) if metric == "negativity" else np.argmax(s))
    edge = cand.size > 1 and best in (0, cand.size - 1)
    offset = float(cand[best])
    if refine and not edge and cand.size >= 3:
        half = 0.5 * (cand[best + 1] - cand[best])
        vertex = parabola_vertex(cand[best - 1:best + 2], s[best - 1:best + 2])
        offset = float(min(max(vertex, cand[best] - half), cand[best] + half))
    return offset, best, bool(edge)


def find_center(projections, geo, angles, max_shift=8, step=0.5, metric=None, rows=None, filter="ram-lak", short_scan=None, refine=True):
    """The offset of the detector's column axis that `geo.offDetector[0]` lacks, from `projections` [N, H, W] (float32, on the GPU)
    taken with `geo` at `angles`: one slice per candidate in +-`max_shift` pixels at `step` (`center.candidates`, at most 64) is
    back-projected from rows filtered once (`center.slices`), scored (`center.metrics`) and the best taken.  Returns a dict:
    `offset_px`, `offset` (metres: add it to `geo.offDetector[0]`, or call `recenter`), `best_px` (the best candidate on the grid),
    `candidates` (pixels), `scores`, `metric` and `edge`.

    metric   "negativity" (minimum), "sharpness" (maximum) or None: `center_metric(angles)`
    rows     parallel beam: the detector rows taken as slices (None: `center_rows`); a cone beam is searched in its mid-plane and
             `rows` must be None
    refine   the vertex of the parabola through the best candidate and its neighbours; one host read of K doubles either way
    `edge` is True when the best candidate is the first or the last: a warning is issued and nothing is refined.  A tilted scan is
    refused, and so is a cone scan that covers less than a full turn (`CENTER_CONE_SHORT_SCAN`)."""
    import warnings

    import torch

    from . import center
    from . import filter as F
    if not isinstance(projections, torch.Tensor) or not projections.is_cuda:
        raise RuntimeError("find_center: projections must be a CUDA/HIP tensor (no CPU path)")
    if projections.dtype != torch.float32:
        raise TypeError(f"find_center: projections must be float32, got {projections.dtype}")
    cand = center.candidates(max_shift, step)
    _check_center(geo, angles, metric, rows, short_scan)
    metric = center_metric(angles) if metric is None else metric
    radius = center.mask_radius(geo, max_shift)

    def on_device(a):
        return None if a is None else torch.tensor(a, device=projections.device)

    def filter_rows(b, taps, pre, post, view_scale, col=None):
        return F.filter_rows(b.contiguous(), on_device(taps), on_device(pre), on_device(post), on_device(view_scale), on_device(col))

    def slices(q, offsets):
        return center.slices(q.contiguous(), geo, angles, offsets)

    def scores_of(f):
        return center.metrics(f, geo, radius)

    scores = find_center_operators(filter_rows, slices, scores_of, projections, geo, angles, cand, metric, rows, filter=filter,
                                   short_scan=short_scan).cpu().numpy()
    offset_px, best, edge = pick_center(cand, scores, metric, refine=refine)
    if edge:
        warnings.warn(f"find_center: the best candidate ({cand[best]:+.2f} px) is at the edge of the search range; widen max_shift")
    return {"offset_px": offset_px, "offset": offset_px * float(geo.dDetector[0]), "best_px": float(cand[best]), "candidates": cand,
            "scores": scores, "metric": metric, "edge": edge}


def recenter(data, offset_m):
    """A shallow copy of a scan dict (the pickle schema, lengths in millimetres) with `offset_m` METRES added to `offDetector[0]`,
    and `center_offset`, the sum of all such corrections in millimetres, beside it.  `data` is left as it is."""
    offset_mm = float(offset_m) * 1000.0
    if not math.isfinite(offset_mm):
        raise ValueError(f"recenter: the offset must be finite, got {offset_m}")
    out = dict(data)
    off = [float(v) for v in data["offDetector"]]
    off[0] += offset_mm
    out["offDetector"] = off
    out["center_offset"] = float(data.get("center_offset", 0.0)) + offset_mm
    return out


TILTED_CENTER_METRIC = "sharpness"


def _check_tilted_metric(who, metric):
    """A tilted-axis search is scored by sharpness, maximised.  The missing cone makes a focused laminogram negative beside every
    edge, so negativity is LARGEST at the true centre and tilt: the rule of CT is not offered."""
    if metric == "negativity":
        raise ValueError(f"{who}: metric 'negativity' is not offered for a tilted axis: the missing cone makes a focused laminogram "
                         "negative beside every edge, so negativity is largest at the true value; the score is 'sharpness', maximised")
    if metric not in (None, TILTED_CENTER_METRIC):
        raise ValueError(f"{who}: metric must be {TILTED_CENTER_METRIC!r} or None, got {metric!r}")


def find_center_tilted_operators(filter_rows, slices, metrics, b, geo, angles, candidates, tilts=None, filter="ram-lak"):
    """The centre (and tilt) search of a tilted-axis parallel-beam scan (center.py) as array code over
    callables, on arrays of `b`'s kind ([N, H, W]; torch tensors on any device, numpy arrays).

        filter_rows(b, taps, pre, post, view_scale)   the row filter of `fdk_operators`, on whole views
        slices(q, offsets, tilts)   filtered views [N, H, W], K offsets in metres, K tilts in degrees or None -> the slice z = 0 for
                                    every candidate, [1, K, n, n], each times its own cos(tilt)
        metrics(f)                  slices -> [1, K, 2] = (negativity, sharpness)

    q = the views filtered with view_scale[i] = w_i (`filter.view_weights`; the cosine of `lamino_fbp_weights` is the slices' own),
    scores[k] = the sharpness of candidate k.  `candidates` are in pixels of the detector; `tilts` (degrees, one per candidate) None
    takes the scan's own.  Returns scores [K], an array of the kind `metrics` returns.  The refusals are `lamino_fbp_weights`'."""
    import numpy as np

    from . import center
    from . import filter as F
    _check_lamino(geo, angles, "find_center_tilted")
    center.tilted_scalars(geo)                                     # a square slice
    if len(b.shape) != 3 or int(b.shape[0]) != len(angles):
        raise ValueError(f"find_center_tilted: projections must be [N, H, W] with one view per angle, got {tuple(b.shape)} for "
                         f"{len(angles)} angles")
    cand = np.asarray(candidates, dtype=np.float64).reshape(-1)
    if not 1 <= cand.size <= center.MAX_K:
        raise ValueError(f"find_center_tilted: 1 .. {center.MAX_K} candidates are needed, got {cand.size}")
    du = float(geo.dDetector[0])
    q = filter_rows(b, F.ramp_taps(int(geo.nDetector[0]), du, filter), None, None, F.view_weights(angles).astype(np.float32))
    score = metrics(slices(q, cand * du, tilts))
    return score[0, :, CENTER_METRICS.index(TILTED_CENTER_METRIC)]


def _tilted_search(who, projections, geo, angles, cand_px, tilts, radius, filter):
    """`find_center_tilted_operators` on the kernels -> scores, float64 numpy [K]."""
    import torch

    from . import center
    from . import filter as F
    if not isinstance(projections, torch.Tensor) or not projections.is_cuda:
        raise RuntimeError(f"{who}: projections must be a CUDA/HIP tensor (no CPU path)")
    if projections.dtype != torch.float32:
        raise TypeError(f"{who}: projections must be float32, got {projections.dtype}")

    def on_device(a):
        return None if a is None else torch.tensor(a, device=projections.device)

    def filter_rows(b, taps, pre, post, view_scale):
        return F.filter_rows(b.contiguous(), on_device(taps), on_device(pre), on_device(post), on_device(view_scale))

    def slices(q, offsets, tilts):
        return center.slices_tilted(q, geo, angles, offsets, tilts=tilts)

    def scores_of(f):
        return center.metrics(f, geo, radius)

    return find_center_tilted_operators(filter_rows, slices, scores_of, projections, geo, angles, cand_px, tilts,
                                        filter=filter).cpu().numpy()


def find_center_tilted(projections, geo, angles, max_shift=8, step=0.5, metric=None, filter="ram-lak", refine=True):
    """`find_center` for a tilted-axis (laminographic) parallel-beam scan over a full turn: the offset of the detector's column axis
    that `geo.offDetector[0]` lacks, from `projections` [N, H, W] (float32, on the GPU).  The slice z = 0 is back-projected for every
    candidate in +-`max_shift` pixels at `step` from views filtered once (`center.slices_tilted`), scored by sharpness
    (`center.metrics`) and the maximum taken (`pick_center`).  Returns a dict: `offset_px`, `offset` (metres: `recenter` writes it
    into a scan), `best_px`, `candidates` (pixels), `scores`, `metric` and `edge` (the best candidate is the first or the last: a
    warning is issued and nothing is refined).  `metric="negativity"` raises ValueError: it is largest at the true centre here."""
    import warnings

    from . import center
    who = "find_center_tilted"
    _check_tilted_metric(who, metric)
    cand = center.candidates(max_shift, step)
    _check_lamino(geo, angles, who)
    radius = center.tilted_mask_radius(geo, max_shift)
    scores = _tilted_search(who, projections, geo, angles, cand, None, radius, filter)
    offset_px, best, edge = pick_center(cand, scores, TILTED_CENTER_METRIC, refine=refine)
    if edge:
        warnings.warn(f"{who}: the best candidate ({cand[best]:+.2f} px) is at the edge of the search range; widen max_shift")
    return {"offset_px": offset_px, "offset": offset_px * float(geo.dDetector[0]), "best_px": float(cand[best]), "candidates": cand,
            "scores": scores, "metric": TILTED_CENTER_METRIC, "edge": edge}
