"""Scan dataset: host-side mirror of `TIGREDataset` (reference src/dataset/tigre.py:220-382).

Same constructor (`path, n_rays, type, device`), same item dictionaries (`rays [n,8]`, `projs`, `coords`, `full_proj`)
and the same pickle schema (tigre.py:230-323; written by format_data.py:25-58 / dataGenerator/generateData.py:153-211).
What differs is the MI355X-first data layout: the reference materialises `rays[N,H,W,8]` for every pixel of every
projection on the device (419 MB at 50x512^2, 24 GB at 720x1024^2, tigre.py:247-255); here only the poses [N,3,4]
live in HBM and rays are generated on demand by `naf_generate_rays` for the pixels a step actually uses.  `.rays`
stays available as a lazy, indexable view for code written against the reference.

Unlike the committed reference cone-beam scans work (`get_rays`, tigre.py:434-437) and
`full_proj` is optional (standard NAF pickles do not have it).
"""
from __future__ import annotations

import pickle

import numpy as np
import torch
from torch.utils.data import Dataset

from .geometry import ConeGeometry, RayGenerator, get_near_far, get_voxels


class _LazyRays:
    """`dataset.rays[i]` -> [H, W, 8] like the reference's precomputed tensor, generated when asked for."""

    def __init__(self, raygen):
        self._g = raygen
        self.shape = (raygen.n_projections, raygen.H, raygen.W, 8)

    def __len__(self):
        return self._g.n_projections

    def __getitem__(self, key):
        if isinstance(key, tuple):                       # rays[index, rows, cols]
            index, rows, cols = key
            pix = int(index) * self._g.pixels_per_projection + rows.long() * self._g.W + cols.long()
            pix = pix.to(self._g.device)                 # index tensors may live on the host, like indexing the reference's tensor
            return self._g.rays_for_pixels(pix.reshape(-1)).reshape(list(pix.shape) + [8])
        return self._g.rays_for_projection(int(key)).reshape(self._g.H, self._g.W, 8)


class TIGREDataset(Dataset):
    """TIGRE dataset (`path` may also be an already loaded dict with the pickle schema)."""

    def __init__(self, path, n_rays=1024, type="train", device="cuda", shard=(0, 1), seed=None):
        """`shard = (rank, world)` (data parallel): every rank draws the SAME `n_rays` pixels per item (shared generator
        seed) and keeps its contiguous slice, so the union over ranks is exactly the single-process batch."""
        super().__init__()
        if isinstance(path, dict):
            data = path
        else:
            with open(path, "rb") as handle:
                data = pickle.load(handle)
        if type not in ("train", "val"):
            raise ValueError("type must be 'train' or 'val'")
        self.geo = ConeGeometry(data)
        self.type = type
        self.n_rays = n_rays
        self.device = torch.device(device)
        self.near, self.far = get_near_far(self.geo)

        split = data[type]
        projs = np.asarray(split["projections"])
        self.projs = torch.tensor(projs, dtype=torch.float32, device=self.device)
        self.full_proj = None
        if data.get("full_proj") is not None:
            self.full_proj = torch.tensor(np.asarray(data["full_proj"]), dtype=torch.complex64, device=self.device)
        self.angles = np.asarray(split["angles"], dtype=np.float64).reshape(-1)
        self.raygen = RayGenerator(self.geo, self.angles, self.device)
        self.rays = _LazyRays(self.raygen)
        self.n_samples = int(data["numTrain"] if type == "train" else data["numVal"])
        H, W = self.raygen.H, self.raygen.W
        rows, cols = torch.meshgrid(torch.arange(H, device=self.device), torch.arange(W, device=self.device), indexing="ij")
        self.coords = torch.stack([rows, cols], -1).reshape(-1, 2).float()     # (row, col) like tigre.py:256-276
        self.image = torch.tensor(np.asarray(data["image"]), dtype=torch.float32, device=self.device)
        self._voxels = None
        # valid (non-zero) pixels per projection, found once (the reference recomputes |proj| > 0 per item, tigre.py:356):
        # after the first pass over the scan an item costs no host synchronisation at all
        self._valid = {}
        self._mask = {}                                  # ptycho mask per projection (train.py:59-60 rebuilds it every step)
        self.shard = (int(shard[0]), int(shard[1]))
        if self.shard[1] > 1 and seed is None:
            seed = 0                                     # ranks must agree on the pixel draw
        self._generator = None
        if seed is not None:
            self._generator = torch.Generator(device=self.device)
            self._generator.manual_seed(int(seed))
        # keyed draws of naf_draw_scan_rays: (seed, item counter) -> one key per item; unseeded datasets start from entropy
        self._draw_seed = int(seed) if seed is not None else int(torch.seed() & 0x7FFFFFFFFFFFFFFF)
        self._draw_count = 0

    @property
    def voxels(self):
        if self._voxels is None:
            self._voxels = torch.tensor(get_voxels(self.geo), dtype=torch.float32, device=self.device)
        return self._voxels

    @property
    def voxel_axes(self):
        """(starts, stops, dims) of the voxel grid: axis k is numpy.linspace(starts[k], stops[k], dims[k]) (tigre.py:388-400)."""
        s = self.geo.sVoxel / 2 - self.geo.dVoxel / 2
        return [-float(v) for v in s], [float(v) for v in s], [int(v) for v in self.geo.nVoxel]

    def __len__(self):
        return self.n_samples

    def set_draw_position(self, items_drawn):
        """Continue the keyed pixel draws after `items_drawn` items (a resumed run: Trainer passes its global step)."""
        self._draw_count = int(items_drawn)

    def _valid_pixels(self, index):
        """Pixels of projection `index` with a non-zero measured value (tigre.py:354-356), as indices inside the projection."""
        index = int(index)
        hit = self._valid.get(index)
        if hit is None:
            flat = self.projs[index].reshape(-1)
            hit = self._valid[index] = torch.nonzero(flat.abs() > 0, as_tuple=False).reshape(-1).contiguous()
        return hit

    def draw_item(self, index):
        """One training item drawn entirely on the device (`naf_draw_scan_rays`): n_rays distinct valid pixels of projection
        `index`, their measured values and rays in one launch -- no randperm sort, no host synchronisation once the
        projection's valid list is cached.  With shard = (rank, world) every rank takes its slice of the SAME draw."""
        index = int(index)
        key = ("flat", index)
        valid = self._valid.get(key)
        if valid is None:
            valid = self._valid[key] = (self._valid_pixels(index) + index * self.raygen.pixels_per_projection).contiguous()
        self._draw_count += 1
        seed = (self._draw_seed * 0x9E3779B97F4A7C15 + self._draw_count * 0xD1B54A32D192ED03) & (2 ** 64 - 1)
        first, count = 0, self.n_rays
        if self.shard[1] > 1:
            from .dist import shard_range
            first, end = shard_range(self.n_rays, *self.shard)
            count = end - first
        pixels, target, rays = self.raygen.draw([valid], self.n_rays, seed, projections=self.projs.reshape(-1), first=first, count=count)
        return pixels - index * self.raygen.pixels_per_projection, target, rays

    def ptycho_mask(self, index, threshold=0.007):
        """`get_ptycho_mask(full_proj[index])` (util.py:196-205), computed once per projection."""
        from .utils import get_ptycho_mask
        index = int(index)
        hit = self._mask.get(index)
        if hit is None:
            hit = self._mask[index] = get_ptycho_mask(self.full_proj[index], threshold=threshold)
        return hit

    def sample_pixels(self, index, n_rays=None, generator=None):
        """`n_rays` distinct valid pixels of projection `index` (tigre.py:356-359: choice without replacement),
        drawn on the device."""
        n_rays = self.n_rays if n_rays is None else n_rays
        valid = self._valid_pixels(index)
        if valid.numel() < n_rays:
            raise ValueError("Cannot take a larger sample than population when 'replace=False'")
        if generator is None:
            generator = self._generator
        perm = torch.randperm(valid.numel(), device=self.device, generator=generator)[:n_rays]
        return valid[perm]

    def __getitem__(self, index):
        if self.type == "train":
            pix, projs, rays = self.draw_item(index)
            W = self.raygen.W
            select_coords = torch.stack([pix // W, pix % W], -1)
            out = {"projs": projs, "rays": rays, "coords": select_coords}
            if self.full_proj is not None:
                out["full_proj"] = self.full_proj[index]
                out["mask"] = self.ptycho_mask(index).reshape(-1)[pix]      # extra key: the mask at the sampled pixels
            return out
        return {"projs": self.projs[index], "rays": self.rays[index]}


def synthetic_scan(n_voxel=64, n_train=50, n_val=8, mode="cone", tilt_angle=0, seed=0, device="cpu", full_proj=False,
                   geometry=None, train_angles=None, metal=None, p_max=None):
    """A complete in-memory scan with the pickle schema, from the analytic phantom (no data ships with the reference).
    Train angles: linspace(0, pi, n+1)[:-1] (generateData.py:175) unless `train_angles` (radians) is given; val angles:
    sorted U(0, pi) with seed 1.  `geometry` overrides the default scanner dict (e.g. the 256 x 356 laminography detector).
    `metal=(count, radius, rho)` plants that many metal spheres in the phantom (`add_metal`, drawn with `seed`; radius in metres)
    and `p_max` ends the detector's dynamic range there (`saturate`); both are stored as `data["metal"]`.  Without them the scan
    is what it has always been."""
    from . import phantom
    from .geometry import angle2pose  # noqa: F401  (documented dependency)

    data = dict(geometry) if geometry is not None else phantom.scan_geometry(n_voxel, mode, tilt_angle)
    tilt_angle = data.get("tilt_angle", tilt_angle)
    if train_angles is not None:
        n_train = len(train_angles)
    geo = ConeGeometry(data)
    table = phantom.ellipsoid_table(seed=seed, extent=float(geo.sVoxel[0]) / 2)
    if tilt_angle:                                       # flat sample for laminography
        table["c"][:, 2] *= 0.3
        table["a"][:, 2] *= 0.3
    if metal is not None:
        count, radius, rho = metal
        table = add_metal(table, count, radius, rho, seed)
    rng = np.random.RandomState(1)
    splits = {"train": np.linspace(0, np.pi, n_train + 1)[:-1] if train_angles is None else np.asarray(train_angles, dtype=np.float64),
              "val": np.sort(rng.uniform(0, np.pi, n_val))}
    dev = torch.device(device)
    for name, angles in splits.items():
        H, W = int(geo.nDetector[1]), int(geo.nDetector[0])
        if dev.type == "cuda":
            gen = RayGenerator(geo, angles, dev)
            projs = torch.stack([phantom.line_integrals(gen.rays_for_projection(i), table).reshape(H, W) for i in range(len(angles))])
        else:                                             # CPU construction for tests: the oracle-free torch formula
            projs = torch.stack([phantom.line_integrals(_rays_cpu(geo, a), table).reshape(H, W) for a in angles])
        if p_max is not None:
            projs = saturate(projs.cpu(), p_max)
        data[name] = {"angles": angles, "projections": projs.cpu().numpy()}
    if metal is not None or p_max is not None:
        data["metal"] = {"spheres": None if metal is None else tuple(metal), "p_max": p_max, "seed": seed}
    data["numTrain"], data["numVal"] = n_train, n_val
    data["image"] = phantom.volume(geo, table, device=dev).cpu().numpy()
    if full_proj:
        data["full_proj"] = data["train"]["projections"].astype(np.complex64)
    return data


def plant_center_offset(geometry, offset_px, **kwargs):
    """`synthetic_scan(geometry=..., **kwargs)` with a wrong centre of rotation planted: the projections are made with
    `offDetector[0]` increased by `offset_px` detector pixels while the returned dict states the nominal `offDetector` of `geometry`
    (the scanner dict, millimetres).  The defect is stored as `data["center_planted"]`; `reconstruct.find_center` finds it."""
    nominal = [float(v) for v in geometry["offDetector"]]
    true = dict(geometry)
    true["offDetector"] = [nominal[0] + float(offset_px) * float(geometry["dDetector"][0]), *nominal[1:]]
    data = synthetic_scan(geometry=true, **kwargs)
    data["offDetector"] = list(geometry["offDetector"])
    data["center_planted"] = {"offset_px": float(offset_px), "offDetector": true["offDetector"]}
    return data


def plant_tilt_error(geometry, error_deg, **kwargs):
    """`synthetic_scan(geometry=..., **kwargs)` of a tilted-axis scan with a wrong tilt planted: the projections are made with
    `tilt_angle` increased by `error_deg` degrees while the returned dict states the nominal `tilt_angle` of `geometry`.  The defect
    is stored as `data["tilt_planted"]`.  No search for it is shipped: sharpness on the slice z = 0 ran to the edge of its grid in
    every rehearsal, and this is how a better score would be rehearsed."""
    nominal = float(geometry.get("tilt_angle", 0))
    if not nominal:
        raise ValueError("plant_tilt_error: the scan has no tilt_angle to be wrong about")
    true = dict(geometry)
    true["tilt_angle"] = nominal + float(error_deg)
    data = synthetic_scan(geometry=true, **kwargs)
    data["tilt_angle"] = geometry["tilt_angle"]
    data["tilt_planted"] = {"error_deg": float(error_deg), "tilt_angle": true["tilt_angle"]}
    return data


def _rays_cpu(geo, angle):
    """Host construction of one projection's rays (only used to synthesise data without a GPU)."""
    from .geometry import angle2pose
    W, H = int(geo.nDetector[0]), int(geo.nDetector[1])
    pose = torch.Tensor(angle2pose(geo.DSO, angle, geo.tilt_angle))
    uu = ((torch.arange(W).float() + 0.5 - W / 2) * float(geo.dDetector[0]) + float(geo.offDetector[0]))[None, :].expand(H, W)
    vv = ((torch.arange(H).float() + 0.5 - H / 2) * float(geo.dDetector[1]) + float(geo.offDetector[1]))[:, None].expand(H, W)
    R, t = pose[:3, :3], pose[:3, 3]
    if geo.mode == "cone":
        dirs = torch.stack([uu / geo.DSD, vv / geo.DSD, torch.ones_like(uu)], -1)
        d = dirs @ R.T
        o = t.expand(d.shape)
    else:
        d = R[:, 2].expand(H, W, 3)
        o = torch.stack([uu, vv, torch.zeros_like(uu)], -1) @ R.T + t
    near, far = get_near_far(geo)
    nf = torch.tensor([near, far], dtype=torch.float32).expand(H, W, 2)
    return torch.cat([o, d, nf], -1).reshape(-1, 8)


NOISE_I0 = 1e5          # photons per pixel of the noise model of scan_from_volume (CTnoise.add(Poisson=1e5) in generateData.py:181)


def scan_from_volume(image, geometry, n_train, n_val, total_angle=180, start_angle=0, random_angle=False, noise=0, seed=0,
                     device="cuda", projector="interpolated"):
    """A complete scan with the pickle schema, projected from a CT volume by the HIP forward projector (projector.py): the
    step dataGenerator/generateData.py:153-211 of the reference does with TIGRE's `Ax`.  `projector` is `project_scan`'s `kind`:
    "interpolated" (the default: trilinear samples) or "siddon" (piecewise-constant voxels, exact chord lengths: the kind `Ax`
    takes by default, and a forward model that is not the one the baselines reconstruct with).

    `image` [n1, n2, n3] (axis 0 = x, voxel centres on the get_voxels grid) and the scanner dict `geometry` (pickle schema,
    millimetres) -> the dict `synthetic_scan` returns, which `TIGREDataset` loads unchanged; `image` is stored as given.
    Train angles: linspace(0, total_angle, n_train + 1)[:-1] or, with `random_angle`, n_train sorted uniform draws in
    [0, total_angle); val angles: n_val sorted uniform draws in [0, 180) degrees; both shifted by `start_angle`
    (generateData.py:174-177,187).  The draws come from numpy RandomState(seed), train first.

    `noise > 0` adds a seeded transmission noise model to both splits: counts I = Poisson(I0 exp(-p)) + Normal(0, noise) with
    I0 = 1e5, then p = -ln(max(I, 1) / I0); negative training values are set to 0 (generateData.py:182).  Parity with
    TIGRE's CTnoise is not pinned."""
    from .projector import check_kind, project_scan

    check_kind(projector, "scan_from_volume")
    data = dict(geometry)
    geo = ConeGeometry(data)
    rng = np.random.RandomState(seed)
    total, start = float(total_angle) / 180 * np.pi, float(start_angle) / 180 * np.pi
    if random_angle:
        train_angles = np.sort(rng.rand(int(n_train)) * total) + start
    else:
        train_angles = np.linspace(0, total, int(n_train) + 1)[:-1] + start
    val_angles = np.sort(rng.rand(int(n_val)) * np.pi) + start
    dev = torch.device(device)
    volume = torch.as_tensor(np.asarray(image), dtype=torch.float32).to(dev).contiguous()
    gen = None
    if noise > 0:
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
    for name, angles in (("train", train_angles), ("val", val_angles)):
        # the default is the call as it has always been made
        projs = project_scan(volume, geo, angles) if projector == "interpolated" else project_scan(volume, geo, angles, kind=projector)
        if noise > 0:
            projs = add_noise(projs, noise, gen)
            if name == "train":
                projs = projs.clamp(min=0.0)
        data[name] = {"angles": angles, "projections": projs.cpu().numpy()}
    data["numTrain"], data["numVal"] = int(n_train), int(n_val)
    data["image"] = image.detach().cpu().numpy() if isinstance(image, torch.Tensor) else image
    return data


def add_noise(projs, noise, generator, i0=NOISE_I0):
    """Transmission noise on line integrals `projs`: I = Poisson(i0 exp(-p)) + Normal(0, noise), p' = -ln(max(I, 1) / i0)."""
    counts = torch.poisson(i0 * torch.exp(-projs.double()), generator=generator)
    counts = counts + float(noise) * torch.randn(counts.shape, generator=generator, device=counts.device, dtype=counts.dtype)
    return (-torch.log(counts.clamp(min=1.0) / i0)).float()


def add_stripes(projs, fraction, sigma, generator):
    """Detector pixels with a wrong gain, on line integrals `projs` [N, H, W] (numpy array or CPU tensor; host side): each of the
    H W pixels is defective with probability `fraction`, a defective pixel has the gain 1 + sigma n with n standard normal (kept
    at 0.1 or above), and the gain multiplies the transmission: p' = -ln(gain exp(-p)).  The gain of a pixel is the same in every
    view, which is what draws a stripe in the sinogram and a ring in the volume.  `generator` is a numpy Generator or an int seed
    for one; equal seeds give equal bits.  Returns float32 of the kind given; `projs` is left as it is."""
    if not 0.0 <= float(fraction) <= 1.0 or float(sigma) < 0.0:
        raise ValueError(f"add_stripes: fraction must be in [0, 1] and sigma >= 0, got {fraction}, {sigma}")
    as_tensor = isinstance(projs, torch.Tensor)
    if as_tensor and projs.is_cuda:
        raise ValueError("add_stripes: projs must be on the host")
    p = (projs.numpy() if as_tensor else np.asarray(projs)).astype(np.float64)
    if p.ndim != 3:
        raise ValueError(f"add_stripes: projs must be [N, H, W], got {p.shape}")
    rng = generator if isinstance(generator, np.random.Generator) else np.random.default_rng(generator)
    defective = rng.random(p.shape[1:]) < float(fraction)
    gain = np.where(defective, np.maximum(1.0 + float(sigma) * rng.standard_normal(p.shape[1:]), 0.1), 1.0)
    out = (-np.log(np.exp(-p) * gain[None])).astype(np.float32)
    return torch.from_numpy(out) if as_tensor else out


def add_metal(table, count, radius, rho, generator):
    """A copy of a `phantom.ellipsoid_table` with `count` spheres of radius `radius` (metres) and density `rho` appended: fillings
    or implants.  Their centres are drawn uniformly in the body ellipsoid (the table's first row) shrunk by `radius`, so every sphere
    lies inside the body.  `generator` is a numpy Generator or an int seed for one; equal seeds give equal bits.  Host side; `table`
    is left as it is.  The metal alone is the last `count` rows of the result."""
    count, radius, rho = int(count), float(radius), float(rho)
    room = np.asarray(table["a"][0], dtype=np.float64) - radius
    if count < 1 or not radius > 0.0 or not rho > 0.0 or not room.min() > 0.0:
        raise ValueError(f"add_metal: count must be >= 1, rho above zero and radius above zero and below the body's semi-axes "
                         f"{tuple(table['a'][0])}, got {count}, {radius}, {rho}")
    rng = generator if isinstance(generator, np.random.Generator) else np.random.default_rng(generator)
    direction = rng.standard_normal((count, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    inside = direction * np.cbrt(rng.random((count, 1))) * room[None]                     # uniform in the shrunk ellipsoid's own frame
    body_R = np.asarray(table["R"][0], dtype=np.float64)                                   # world -> frame, so its transpose leads back
    centres = np.asarray(table["c"][0], dtype=np.float64)[None] + inside @ body_R
    return {"c": np.concatenate([np.asarray(table["c"], dtype=np.float64), centres]),
            "a": np.concatenate([np.asarray(table["a"], dtype=np.float64), np.full((count, 3), radius)]),
            "R": np.concatenate([np.asarray(table["R"], dtype=np.float64), np.broadcast_to(np.eye(3), (count, 3, 3))]),
            "rho": np.concatenate([np.asarray(table["rho"], dtype=np.float64), np.full(count, rho)])}


def saturate(projs, p_max):
    """min(p, p_max) on line integrals `projs` (numpy array or tensor): the end of the detector's dynamic range, below which no
    count is told from none.  A linear, monochromatic metal is consistent data and draws no streaks; a trace that is cut off does.
    Returns float32 of the kind given; `projs` is left as it is."""
    p_max = float(p_max)
    if not p_max > 0.0 or not np.isfinite(p_max):
        raise ValueError(f"saturate: p_max must be finite and above zero, got {p_max}")
    if isinstance(projs, torch.Tensor):
        return projs.float().clamp(max=p_max)
    return np.minimum(np.asarray(projs, dtype=np.float32), np.float32(p_max))


def _host_array(a, who, name, ndim):
    """`a` (numpy array or CPU tensor) as a float64 array of `ndim` dimensions -> (array, whether it was a tensor)."""
    as_tensor = isinstance(a, torch.Tensor)
    if as_tensor and a.is_cuda:
        raise ValueError(f"{who}: {name} must be on the host")
    x = (a.numpy() if as_tensor else np.asarray(a)).astype(np.float64)
    if x.ndim != ndim:
        raise ValueError(f"{who}: {name} must have {ndim} dimensions, got {x.shape}")
    return x, as_tensor


def _numpy_generator(generator):
    return generator if isinstance(generator, np.random.Generator) else np.random.default_rng(generator)


def raw_frames(projs, i0, flat, dark, generator=None):
    """The detector frames behind line integrals `projs` [N, H, W] (numpy array or CPU tensor; host side), the forward model whose
    inverse `frames.condition` is: raw = dark + (flat - dark) exp(-p), with `flat` and `dark` one [H, W] frame each in counts.
    `i0` is the photon count a transmission of one stands for: with a `generator` (a numpy Generator or an int seed for one) the
    transmission takes the Poisson noise of `add_noise`, Poisson(i0 exp(-p)) / i0, before it is scaled; without one the frames are
    noiseless and `i0` is not read.  Computed in float64, returned as float32 of the kind given; equal seeds give equal bits."""
    who = "raw_frames"
    p, as_tensor = _host_array(projs, who, "projs", 3)
    f, _ = _host_array(flat, who, "flat", 2)
    d, _ = _host_array(dark, who, "dark", 2)
    if f.shape != p.shape[1:] or d.shape != p.shape[1:]:
        raise ValueError(f"{who}: flat and dark must be {p.shape[1:]}, got {f.shape} and {d.shape}")
    trans = np.exp(-p)
    if generator is not None:
        if not float(i0) > 0.0:
            raise ValueError(f"{who}: i0 must be above zero, got {i0}")
        trans = _numpy_generator(generator).poisson(float(i0) * trans) / float(i0)
    out = (d[None] + (f - d)[None] * trans).astype(np.float32)
    return torch.from_numpy(out) if as_tensor else out


def add_zingers(raw, fraction, gain, generator, isolation=1):
    """Zingers on frames `raw` [N, H, W] (numpy array or CPU tensor; host side): every sample is drawn with probability `fraction`,
    independently in every view, and a hit sample is multiplied by `gain` (a stray photon adds counts: gain > 1).  A zinger is an
    isolated pixel: walking a view in row-major order, a drawn sample is dropped when a hit already kept lies within `isolation`
    pixels of it along both axes (1: no two hits touch; size - 1: no window of `size` holds two; 0: every draw is kept).  Returns
    (frames as float32 of the kind given, the bool mask [N, H, W] of the hit samples); equal seeds give equal bits."""
    if not 0.0 <= float(fraction) <= 1.0 or not float(gain) > 0.0 or int(isolation) < 0:
        raise ValueError(f"add_zingers: fraction must be in [0, 1], gain above zero and isolation >= 0, got {fraction}, {gain}, "
                         f"{isolation}")
    x, as_tensor = _host_array(raw, "add_zingers", "raw", 3)
    hit = _numpy_generator(generator).random(x.shape) < float(fraction)
    k = int(isolation)
    if k > 0:
        for i, v, u in np.argwhere(hit):                 # row-major: the hits before (v, u) are final
            if hit[i, max(v - k, 0):v, max(u - k, 0):u + k + 1].any() or hit[i, v, max(u - k, 0):u].any():
                hit[i, v, u] = False
    out = np.where(hit, x * float(gain), x).astype(np.float32)
    return (torch.from_numpy(out), torch.from_numpy(hit)) if as_tensor else (out, hit)


def add_dead_pixels(flat, dark, fraction, generator):
    """Dead detector pixels: each of the H W pixels of `flat` and `dark` ([H, W], numpy arrays or CPU tensors; host side) is dead
    with probability `fraction`, and a dead pixel reads its dark value whatever falls on it: flat = dark there.  Returns (flat as
    float32 of the kind given, the bool mask [H, W] of the dead pixels); the frames of such a detector are `raw_frames` of the
    returned flat.  Equal seeds give equal bits."""
    if not 0.0 <= float(fraction) <= 1.0:
        raise ValueError(f"add_dead_pixels: fraction must be in [0, 1], got {fraction}")
    f, as_tensor = _host_array(flat, "add_dead_pixels", "flat", 2)
    d, _ = _host_array(dark, "add_dead_pixels", "dark", 2)
    if f.shape != d.shape:
        raise ValueError(f"add_dead_pixels: flat and dark must have one shape, got {f.shape} and {d.shape}")
    dead = _numpy_generator(generator).random(f.shape) < float(fraction)
    out = np.where(dead, d, f).astype(np.float32)
    return (torch.from_numpy(out), torch.from_numpy(dead)) if as_tensor else (out, dead)
