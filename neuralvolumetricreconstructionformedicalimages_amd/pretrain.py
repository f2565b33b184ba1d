"""Start a neural field from a reconstructed volume: `fit_volume` regresses the network onto a volume by point supervision, so that
training on projections begins from, say, one FDK pass instead of from U(-1e-4, 1e-4) tables.  DESIGN.md section 24.

Each step draws `n_points` points uniformly in the volume's box and reads the volume there, in one launch and without any host
traffic (`volume.draw_sample`: a counter-based hash of (seed, step, index, axis), trilinear samples with P1's cell convention), runs
the network's ordinary differentiable path on them -- `encoder.HashEncoder` (the HIP forward, and the binned backward from 2^13
points) and the fp32 `nn.Linear` layers of `network.DensityNetwork` -- takes the mean squared error against the samples and steps a
torch.optim.Adam of its own, built with the hyper-parameters `Trainer` uses and discarded afterwards: the optimiser that training
then runs starts with clean moments.

What it is not: a fused bf16 point-supervised step inside the training kernels.  The fit is a few hundred steps once per run; the
kernels of the fused training step are not touched.

`init_volume_config` parses the `train.init_volume` / `init_steps` / `init_points` keys of a training YAML for `Trainer`.
"""
from __future__ import annotations

import math
import os

import numpy as np

DEFAULT_STEPS = 500
DEFAULT_POINTS = 2 ** 16
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8          # what Trainer builds (trainer.py: betas=(0.9, 0.999), torch's default eps)


def _extent(n_voxel):
    return tuple(int(v) for v in np.asarray(n_voxel).reshape(-1))


def check_fit_arguments(net, volume, geo, n_steps, n_points, lr):
    """The argument checks of `fit_volume`; nothing here touches a device.  Returns (n_steps, n_points, lr)."""
    import torch
    if not hasattr(net, "bound") or not hasattr(net, "encoder") or not callable(net):
        raise ValueError("fit_volume: net must be a field network with .encoder and .bound (network.DensityNetwork)")
    if not isinstance(volume, torch.Tensor) or volume.dim() != 3:
        raise ValueError(f"fit_volume: volume must be a [n1, n2, n3] tensor, got {type(volume).__name__} "
                         f"{tuple(getattr(volume, 'shape', ()))}")
    if volume.dtype != torch.float32:
        raise ValueError(f"fit_volume: volume must be float32, got {volume.dtype}")
    if tuple(volume.shape) != _extent(geo.nVoxel):
        raise ValueError(f"fit_volume: volume has shape {tuple(volume.shape)} but the scan's nVoxel is {_extent(geo.nVoxel)}")
    if np.any(np.asarray(geo.offOrigin, dtype=np.float64) != 0):
        raise ValueError(f"fit_volume: the sampler's box is centred at the origin, got offOrigin {geo.offOrigin}")
    n_steps, n_points, lr = int(n_steps), int(n_points), float(lr)
    if n_steps < 0:
        raise ValueError(f"fit_volume: n_steps must be >= 0, got {n_steps}")
    if not 1 <= n_points < 2 ** 32:
        raise ValueError(f"fit_volume: n_points must be in 1 .. 2^32 - 1, got {n_points}")
    if not (lr > 0 and math.isfinite(lr)):
        raise ValueError(f"fit_volume: lr must be > 0 and finite, got {lr}")
    return n_steps, n_points, lr


def sample_box(geo, bound):
    """(lo, hi, dvoxel): the volume's box |p_a| <= n_a d_a / 2 intersected with +-(bound - 1e-6), the clamp the renderer applies to
    its sample points (float32, as the kernels hold it), and the float32 voxel size."""
    d = np.asarray(geo.dVoxel, dtype=np.float64).astype(np.float32)
    h = (np.asarray(geo.nVoxel, dtype=np.float64) * d.astype(np.float64) / 2.0).astype(np.float32)
    b = np.float32(np.float32(bound) - np.float32(1e-6))
    hi = np.minimum(h, b)
    return -hi, hi, d


def fit_volume(net, volume, geo, n_steps, n_points=DEFAULT_POINTS, lr=1e-3, seed=0):
    """Fit the field `net` to `volume` (CUDA float32 [n1, n2, n3] on the voxel grid of `geo`, a ConeGeometry) with `n_steps` Adam
    steps of `n_points` points each; returns the per-step losses as one float32 device tensor [n_steps] (nothing is read back here).

    Targets are clamped to [0, 1] when the network's last activation is a sigmoid: it cannot reach anything else, and an FDK volume
    has negative voxels and overshoots.  The parameters are updated in place; the caller refreshes whatever shadows it keeps of them
    (`NAFEngine.sync_from_module`).  The draw is keyed by (seed, step): two fits from equal parameters draw equal points."""
    import torch

    from . import volume as V
    n_steps, n_points, lr = check_fit_arguments(net, volume, geo, n_steps, n_points, lr)
    if not volume.is_cuda:
        raise RuntimeError("fit_volume: volume must be a CUDA/HIP tensor (no CPU path)")
    volume = volume.contiguous()
    lo, hi, dvoxel = sample_box(geo, net.bound)
    clamp = getattr(net, "last_activation", None) == "sigmoid"
    losses = torch.zeros(n_steps, dtype=torch.float32, device=volume.device)
    if n_steps == 0:
        return losses
    params = [p for p in net.parameters() if p.requires_grad]
    optimizer = torch.optim.Adam(params, lr=lr, betas=ADAM_BETAS, eps=ADAM_EPS)
    points = torch.empty((n_points, 3), dtype=torch.float32, device=volume.device)
    targets = torch.empty(n_points, dtype=torch.float32, device=volume.device)
    was_training = net.training
    # the encoder's eager range check reads a flag back every call; the drawn points lie inside +-(bound - 1e-6) by construction
    strict = getattr(net.encoder, "strict_range", None)
    if strict:
        net.encoder.strict_range = False
    net.train()
    try:
        with torch.enable_grad():
            for step in range(n_steps):
                V.draw_sample(volume, dvoxel, lo, hi, seed, step, n_points, points_out=points, targets_out=targets)
                if clamp:
                    targets.clamp_(0.0, 1.0)
                optimizer.zero_grad(set_to_none=True)
                loss = ((net(points).reshape(-1) - targets) ** 2).mean()
                loss.backward()
                optimizer.step()
                losses[step] = loss.detach()
    finally:
        if strict:
            net.encoder.strict_range = strict
        net.train(was_training)
    return losses


ANALYTIC_SOURCES = ("fdk", "lamino-fbp")      # reconstruct.fdk / reconstruct.lamino_fbp of the training projections


# ---- the training YAML's keys --------------------------------------------------------------------------------------------------------
def init_volume_config(train_cfg, world_size=1):
    """Parse `train.init_volume` (absent / None: no warm start; "fdk"; "lamino-fbp" for a tilted-axis scan; or a path to a .npy of
    shape nVoxel), `train.init_steps` (default 500) and `train.init_points` (default 2^16) -> None, or
    {"source": "fdk" | "lamino-fbp" | path, "steps": int, "points": int}.
    Raises ValueError on an unknown value and on a world size above 1; touches no device and no process group."""
    source = train_cfg.get("init_volume")
    if source is None:
        return None
    if not isinstance(source, (str, os.PathLike)):
        raise ValueError(f"train.init_volume must be 'fdk' or a path to a .npy volume, got {source!r}")
    source = os.fspath(source)
    if source not in ANALYTIC_SOURCES and not source.endswith(".npy"):
        raise ValueError(f"train.init_volume must be 'fdk' or a path to a .npy volume ('lamino-fbp' for a tilted-axis scan), got {source!r}")
    if int(world_size) > 1:
        # the fit's table gradient is summed with fp32 atomics below 2^13 points and in a per-process order above: ranks that each
        # fitted their own copy would start training from tables that differ, and the data-parallel step assumes replicas
        raise ValueError(f"train.init_volume is single-process only, got a world size of {int(world_size)}: the ranks' fits would "
                         "leave them with different tables")
    steps, points = int(train_cfg.get("init_steps", DEFAULT_STEPS)), int(train_cfg.get("init_points", DEFAULT_POINTS))
    if steps < 0 or not 1 <= points < 2 ** 32:
        raise ValueError(f"train.init_steps must be >= 0 and train.init_points in 1 .. 2^32 - 1, got {steps} and {points}")
    return {"source": source, "steps": steps, "points": points}


def check_init_geometry(init, geo):
    """What can be refused about `init` (from `init_volume_config`) from the scan's geometry alone, before any device work: "fdk"
    on a scan that `reconstruct.fdk` refuses, and a .npy whose header does not say float nVoxel."""
    if init is None:
        return
    if init["source"] == "fdk":
        if geo.mode not in ("cone", "parallel") or float(geo.tilt_angle) != 0.0:
            raise ValueError(f"train.init_volume: 'fdk' needs a scan that reconstruct.fdk accepts (cone or parallel beam, no tilt), got "
                             f"mode {geo.mode!r} with tilt_angle {geo.tilt_angle}; fdk refuses a tilted (laminographic) scan")
        return
    if init["source"] == "lamino-fbp":
        if geo.mode != "parallel" or not 0.0 < float(geo.tilt_angle) < 90.0:
            raise ValueError(f"train.init_volume: 'lamino-fbp' needs a scan that reconstruct.lamino_fbp accepts (a parallel beam tilted "
                             f"strictly between 0 and 90 degrees), got mode {geo.mode!r} with tilt_angle {geo.tilt_angle}")
        return
    shape = np.load(init["source"], mmap_mode="r").shape
    if tuple(shape) != _extent(geo.nVoxel):
        raise ValueError(f"train.init_volume: {init['source']} has shape {tuple(shape)} but the scan's nVoxel is {_extent(geo.nVoxel)}")


def init_volume_tensor(init, geo, projections, angles, device):
    """The volume `init` names, as a CUDA float32 tensor of shape nVoxel: reconstruct.fdk (or reconstruct.lamino_fbp, whose
    refusals apply: a full turn of views) of the training projections clamped at 0, or the .npy file."""
    import torch
    if init["source"] == "fdk":
        from . import reconstruct
        return reconstruct.fdk(projections, geo, angles, nonneg=True).contiguous()
    if init["source"] == "lamino-fbp":
        from . import reconstruct
        return reconstruct.lamino_fbp(projections, geo, angles, nonneg=True).contiguous()
    return torch.tensor(np.load(init["source"]), dtype=torch.float32, device=device).contiguous()
