"""Float64 subset operators and kernel references for the OS-SART tests (include/naf_hip.h, P4) -- not a
test module.  Everything is built from pieces the other oracles already pin: the dense matrix of `_tv_oracle.pocs_case`, restricted
to a view list by slicing or zero-padding its 576-ray blocks, and `_projector_oracle.project_rays`,
`_backproject_oracle.backproject_rays` and `ray_lengths` for the kernel cases."""
import functools

import numpy as np

import _backproject_oracle as B
import _projector_oracle as P
import _tv_oracle as T

POCS_VIEWS, POCS_H, POCS_W = 4, 24, 24
SART_SUBSETS = [[0], [2], [1], [3]]                 # one view per subset, opposite views first
PAIR_SUBSETS = [[0, 2], [1, 3]]

# psnr_3d of the float64 iteration on the rehearsal case at relax 1, as tests/test_sart_cpu.py measures and pins them:
# {iterations: (SIRT, OS-SART over SART_SUBSETS, OS-SART over PAIR_SUBSETS)}
POCS_PSNR = {5: (20.812, 28.573, 24.372), 20: (26.388, 30.531, 28.677)}


@functools.lru_cache(maxsize=None)
def pocs_operators():
    """(A, AT, b, x_true, (geo, rays)) of `_tv_oracle.pocs_case` with b as [4, 24, 24], A(x, views) -> [len(views), 24, 24] and
    AT(y, views) -> volume, plus the case's own (A_all, AT_all, b_flat) for `sirt_operators`."""
    A_all, AT_all, b_flat, x_true, extra = T.pocs_case()
    per = POCS_H * POCS_W
    b = b_flat.reshape(POCS_VIEWS, POCS_H, POCS_W)
    b.setflags(write=False)
    x_true.setflags(write=False)

    def A(x, views):
        return A_all(x).reshape(POCS_VIEWS, POCS_H, POCS_W)[list(views)]

    def AT(y, views):
        full = np.zeros((POCS_VIEWS, per))
        full[list(views)] = np.asarray(y).reshape(len(views), per)
        return AT_all(full.reshape(-1))

    return A, AT, b, x_true, extra, (A_all, AT_all, b_flat)


def view_rays(geo, angles, views):
    """float32 rays [len(views) * H * W, 8] of the listed views, in list order."""
    return B.case_rays(geo, [angles[v] for v in views])


def residual(x, b_views, rays, geo):
    """Float64 (r, y, A x, len) per ray of `rays`: r = b - A x, y = r / len with len the fp32 segment length the kernel holds
    (0 on a miss, where y = 0)."""
    dims = np.asarray(x).shape
    ax = P.project_rays(x, geo.dVoxel, rays, geo.accuracy)
    length = B.ray_lengths(rays, dims, geo.dVoxel, geo.accuracy)
    b = np.asarray(b_views, dtype=np.float64).reshape(-1)
    r = b - ax
    y = np.where(length > 0, r / np.where(length > 0, length, 1.0), 0.0)
    return r, y, ax, length


def backprojection(y, rays, geo, dims):
    """Float64 (A_s^T y, A_s^T 1) over `rays`."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    return (B.backproject_rays(y, geo.dVoxel, rays, dims, geo.accuracy),
            B.backproject_rays(np.ones_like(y), geo.dVoxel, rays, dims, geo.accuracy))
