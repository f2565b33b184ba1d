"""The entry points of the Siddon projector (include/naf_hip.h P6) are exported, declared and bound, refuse bad arguments before
any launch, and the ABI version is the one existing callers pin.  No GPU needed: nothing is launched."""
import ctypes
import math
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"naf_project_rays_siddon": 9, "naf_project_scan_siddon": 8}


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
    assert len(_abi.SIGNATURES["naf_project_rays"][1]) == 10 and len(_abi.SIGNATURES["naf_project_scan"][1]) == 9
    assert lib.naf_abi_version() == 6


def test_arguments_are_refused_before_any_launch():
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    lib = _abi.lib()
    err = lib.naf_last_error
    vol, rays, out, poses = (ctypes.c_void_p(v) for v in (4096, 8192, 12288, 16384))
    dv = (ctypes.c_float * 3)(1e-3, 7e-4, 1.3e-3)
    dims = (ctypes.c_uint32 * 3)(17, 9, 33)

    def project_rays(volume=vol, n=(17, 9, 33), dvoxel=dv, r=rays, n_rays=64, o=out):
        return lib.naf_project_rays_siddon(volume, *n, ctypes.byref(dvoxel) if dvoxel is not None else None, r, n_rays, o, None)

    def project_scan(volume=vol, d=dims, dvoxel=dv, p=poses, n_proj=2, w=24, h=24, DSD=1.5, parallel=0, o=out, null_det=False):
        det = _abi.Detector(w, h, 1e-3, 1e-3, 0.0, 0.0, DSD, 0.9, 1.1, parallel)
        return lib.naf_project_scan_siddon(volume, ctypes.byref(d) if d is not None else None,
                                           ctypes.byref(dvoxel) if dvoxel is not None else None, p, n_proj,
                                           None if null_det else ctypes.byref(det), o, None)

    # empty batches are successful no-ops whatever the pointers
    assert project_rays(volume=None, dvoxel=None, r=None, n_rays=0, o=None) == 0
    assert project_scan(volume=None, d=None, dvoxel=None, p=None, n_proj=0, o=None, null_det=True) == 0
    # rays
    assert project_rays(volume=None) == -1 and b"null pointer" in err()
    assert project_rays(dvoxel=None) == -1 and b"null pointer" in err()
    assert project_rays(r=None) == -1 and b"null pointer" in err()
    assert project_rays(o=None) == -1 and b"null pointer" in err()
    for n in ((0, 9, 33), (17, 0, 33), (17, 9, 0)):
        assert project_rays(n=n) == -1 and b"zero volume dimension" in err()
    for bad in (0.0, -1e-3, math.inf, math.nan):
        for axis in range(3):
            d = (ctypes.c_float * 3)(1e-3, 1e-3, 1e-3)
            d[axis] = bad
            assert project_rays(dvoxel=d) == -1 and b"voxel size must be > 0" in err()
            assert project_scan(dvoxel=d) == -1 and b"voxel size must be > 0" in err()
    assert project_rays(r=ctypes.c_void_p(8200)) == -1 and b"16-byte aligned" in err()
    assert project_rays(n_rays=1 << 40) == -1 and b"too many rays" in err()
    # scan
    assert project_scan(volume=None) == -1 and b"null pointer" in err()
    assert project_scan(d=None) == -1 and b"null pointer" in err()
    assert project_scan(dvoxel=None) == -1 and b"null pointer" in err()
    assert project_scan(p=None) == -1 and b"null pointer" in err()
    assert project_scan(o=None) == -1 and b"null pointer" in err()
    assert project_scan(null_det=True) == -1 and b"project_scan_siddon: null pointer" in err()
    assert project_scan(d=(ctypes.c_uint32 * 3)(17, 0, 33)) == -1 and b"zero volume dimension" in err()
    assert project_scan(w=0) == -1 and b"empty detector" in err()
    assert project_scan(h=0) == -1 and b"empty detector" in err()
    assert project_scan(DSD=0.0) == -1 and b"DSD must be > 0" in err()
    assert project_scan(DSD=-1.0) == -1 and b"DSD must be > 0" in err()
    assert project_scan(DSD=math.nan) == -1 and b"DSD must be > 0" in err()
    assert project_scan(n_proj=0xffffffff, w=0xffff, h=0xffff) == -1 and b"too many pixels" in err()
    assert all(b"siddon" in m for m in (err(),))
