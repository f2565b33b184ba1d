"""The entry points of the Siddon projector's transpose (include/naf_hip.h P7) are exported, declared and bound, refuse bad
arguments before any launch with a message that names them, and the ABI version is the one existing callers pin.  No GPU needed:
nothing is launched."""
import ctypes
import math
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"naf_backproject_rays_siddon": 9, "naf_backproject_scan_siddon": 8}


def test_symbols_are_declared_bound_and_exported():
    from neuralvolumetricreconstructionformedicalimages_amd import _abi, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "naf_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(naf_[a-z0-9_]+)\s*\(", text))
    lib = _abi.lib()
    raw = ctypes.CDLL(build.LIB_PATH)
    for name, n_args in NAMES.items():
        assert name in declared and name in _abi.SIGNATURES and hasattr(raw, name)
        assert len(_abi.SIGNATURES[name][1]) == n_args and getattr(lib, name).restype is ctypes.c_int
    # one argument fewer than the interpolated counterparts: there is no sample step
    assert len(_abi.SIGNATURES["naf_backproject_rays"][1]) == 10 and len(_abi.SIGNATURES["naf_backproject_scan"][1]) == 9
    assert lib.naf_abi_version() == 6


def test_arguments_are_refused_before_any_launch():
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    lib = _abi.lib()
    vol, rays, values, poses = (ctypes.c_void_p(v) for v in (4096, 8192, 12288, 16384))
    dv = (ctypes.c_float * 3)(1e-3, 7e-4, 1.3e-3)
    dims = (ctypes.c_uint32 * 3)(17, 9, 33)

    def refused(rc, what, who):
        message = lib.naf_last_error()
        return rc == -1 and what in message and who in message

    def rays_call(y=values, r=rays, n_rays=64, n=(17, 9, 33), dvoxel=dv, volume=vol):
        return lib.naf_backproject_rays_siddon(y, r, n_rays, *n, ctypes.byref(dvoxel) if dvoxel is not None else None, volume, None)

    def scan_call(y=values, d=dims, dvoxel=dv, p=poses, n_proj=2, w=24, h=24, DSD=1.5, parallel=0, volume=vol, null_det=False):
        det = _abi.Detector(w, h, 1e-3, 1e-3, 0.0, 0.0, DSD, 0.9, 1.1, parallel)
        return lib.naf_backproject_scan_siddon(y, ctypes.byref(d) if d is not None else None,
                                               ctypes.byref(dvoxel) if dvoxel is not None else None, p, n_proj,
                                               None if null_det else ctypes.byref(det), volume, None)

    R, C = b"backproject_rays_siddon", b"backproject_scan_siddon"
    # empty batches are successful no-ops whatever the pointers
    assert rays_call(y=None, r=None, n_rays=0, dvoxel=None, volume=None) == 0
    assert scan_call(y=None, d=None, dvoxel=None, p=None, n_proj=0, volume=None, null_det=True) == 0
    # rays
    assert refused(rays_call(volume=None), b"null pointer", R)
    assert refused(rays_call(dvoxel=None), b"null pointer", R)
    assert refused(rays_call(r=None), b"null pointer", R)
    assert refused(rays_call(y=None), b"null pointer", R)
    for n in ((0, 9, 33), (17, 0, 33), (17, 9, 0)):
        assert refused(rays_call(n=n), b"zero volume dimension", R)
    for bad in (0.0, -1e-3, math.inf, math.nan):
        for axis in range(3):
            d = (ctypes.c_float * 3)(1e-3, 1e-3, 1e-3)
            d[axis] = bad
            assert refused(rays_call(dvoxel=d), b"voxel size must be > 0", R)
            assert refused(scan_call(dvoxel=d), b"voxel size must be > 0", C)
    assert refused(rays_call(r=ctypes.c_void_p(8200)), b"16-byte aligned", R)
    assert refused(rays_call(n_rays=1 << 40), b"too many rays", R)
    # scan
    assert refused(scan_call(volume=None), b"null pointer", C)
    assert refused(scan_call(d=None), b"null pointer", C)
    assert refused(scan_call(dvoxel=None), b"null pointer", C)
    assert refused(scan_call(p=None), b"null pointer", C)
    assert refused(scan_call(y=None), b"null pointer", C)
    assert refused(scan_call(null_det=True), b"null pointer", C)
    assert refused(scan_call(d=(ctypes.c_uint32 * 3)(17, 0, 33)), b"zero volume dimension", C)
    assert refused(scan_call(w=0), b"empty detector", C)
    assert refused(scan_call(h=0), b"empty detector", C)
    assert refused(scan_call(DSD=0.0), b"DSD must be > 0", C)
    assert refused(scan_call(DSD=-1.0), b"DSD must be > 0", C)
    assert refused(scan_call(DSD=math.nan), b"DSD must be > 0", C)
    assert scan_call(DSD=0.0, parallel=1, n_proj=0) == 0
    assert refused(scan_call(n_proj=0xffffffff, w=0xffff, h=0xffff), b"too many pixels", C)
