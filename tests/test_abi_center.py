"""The entry points of the centre-of-rotation search (include/naf_hip.h A5) are exported, declared and bound, refuse bad arguments
before any launch, and the ABI version is the one existing callers pin.  No GPU needed: nothing is launched."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")
NAMES = ("naf_center_slices", "naf_center_metrics_workspace_bytes", "naf_center_metrics")


def test_symbols_are_declared_bound_and_exported():
    from neuralvolumetricreconstructionformedicalimages_amd import _abi, build, center
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "naf_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(naf_[a-z0-9_]+)\s*\(", text))
    lib = _abi.lib()
    raw = ctypes.CDLL(build.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in _abi.SIGNATURES and hasattr(raw, name)
    assert [len(_abi.SIGNATURES[n][1]) for n in NAMES] == [19, 3, 11]
    assert lib.naf_center_slices.restype is ctypes.c_int and lib.naf_center_metrics_workspace_bytes.restype is ctypes.c_size_t
    assert lib.naf_abi_version() == 6
    for define, value in (("NAF_CENTER_MAX_W 16384u", center.MAX_W), ("NAF_CENTER_MAX_K 64u", center.MAX_K),
                          ("NAF_CENTER_MAX_SIZE 4096u", center.MAX_SIZE), ("NAF_CENTER_GROUP 8u", center.GROUP)):
        assert "#define " + define in text and int(define.split()[1][:-1]) == value
    assert any(p.endswith("center.hip") for p in build.sources())
    assert any(p.endswith("center_device.h") for p in build._deps())
    # the declarations are appended: nothing stands after them but the closing of the header
    assert text.index("naf_center_slices") > text.index("naf_inpaint_rows")


def test_slices_arguments_are_refused_before_any_launch():
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    lib = _abi.lib()
    err = lib.naf_last_error
    q, trig, cand, f = (ctypes.c_void_p(v) for v in (1 << 20, 2 << 20, 3 << 20, 4 << 20))

    def call(q=q, trig=trig, cand=cand, S=1, N=3, W=64, K=5, n=16, parallel=0, DSO=1.0, DSD=1.5, du=1e-3, ou=0.0, dx=1e-3, dy=1e-3,
             ox=0.0, oy=0.0, f=f):
        return lib.naf_center_slices(q, trig, cand, S, N, W, K, n, parallel, DSO, DSD, du, ou, dx, dy, ox, oy, f, None)

    def refused(text, **kw):
        return call(**kw) == -1 and text in err() and err().startswith(b"center_slices: ")

    # S n == 0 is a successful no-op whatever else is given
    assert lib.naf_center_slices(None, None, None, 0, 0, 0, 0, 16, 7, NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN, None, None) == 0
    assert lib.naf_center_slices(None, None, None, 1, 0, 0, 0, 0, 7, NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN, None, None) == 0
    for name in ("q", "trig", "cand", "f"):
        assert refused(b"null pointer", **{name: None})
    assert refused(b"at least one view", N=0)
    for W in (0, 16385, 0xffffffff):
        assert refused(b"row width must be in 1 .. 16384", W=W)
    for K in (0, 65, 0xffffffff):
        assert refused(b"number of candidates must be in 1 .. 64", K=K)
    assert refused(b"more than 4096 pixels", n=4097)
    assert refused(b"parallel must be 0 or 1", parallel=2)
    for name in ("du", "ou", "dx", "dy", "ox", "oy"):
        for bad in (NAN, INF, -INF):
            assert refused(b"must be finite", **{name: bad})
    for name in ("du", "dx", "dy"):
        for bad in (0.0, -1e-3):
            assert refused(b"above zero", **{name: bad})
    for name in ("DSO", "DSD"):
        for bad in (NAN, INF, 0.0, -1.0):
            assert refused(b"DSO and DSD must be finite and above zero", **{name: bad})
        assert refused(b"must be 4-byte aligned", parallel=1, f=ctypes.c_void_p((4 << 20) + 2), **{name: NAN})   # not read when parallel
    assert refused(b"the source's orbit crosses the slice", DSO=0.011)          # a 16 mm slice's corner is 11.3 mm out
    assert refused(b"the source's orbit crosses the slice", ox=0.995)
    for name, base in (("q", 1 << 20), ("trig", 2 << 20), ("cand", 3 << 20), ("f", 4 << 20)):
        for off in (1, 2, 3):
            assert refused(b"must be 4-byte aligned", **{name: ctypes.c_void_p(base + off)})
    assert refused(b"more than 2^31 - 1 workgroups", S=1 << 16, n=4096, K=64, N=1, parallel=1)
    # the limits themselves pass every check: the next refusal speaks
    assert refused(b"must be 4-byte aligned", W=16384, K=64, n=4096, parallel=1, f=ctypes.c_void_p((4 << 20) + 1))


def test_metrics_arguments_are_refused_before_any_launch():
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    lib = _abi.lib()
    err = lib.naf_last_error
    f, out, ws = (ctypes.c_void_p(v) for v in (1 << 20, 2 << 20, 3 << 20))
    assert lib.naf_center_metrics_workspace_bytes(1, 1, 16) == 16                  # one workgroup, two doubles
    assert lib.naf_center_metrics_workspace_bytes(3, 5, 46) == 3 * 5 * 2 * 16       # 2116 pixels: two workgroups of 2048
    assert lib.naf_center_metrics_workspace_bytes(1, 1, 4097) == 0
    need = lib.naf_center_metrics_workspace_bytes(2, 5, 33)

    def call(f=f, S=2, K=5, n=33, dx=1e-3, dy=1e-3, r=0.01, out=out, ws=ws, bytes=need):
        return lib.naf_center_metrics(f, S, K, n, dx, dy, r, out, ws, bytes, None)

    def refused(text, **kw):
        return call(**kw) == -1 and text in err() and err().startswith(b"center_metrics: ")

    assert lib.naf_center_metrics(None, 0, 5, 33, NAN, NAN, NAN, None, None, 0, None) == 0
    assert lib.naf_center_metrics(None, 2, 0, 33, NAN, NAN, NAN, None, None, 0, None) == 0
    for name in ("f", "out", "ws"):
        assert refused(b"null pointer", **{name: None})
    assert refused(b"more than 4096 pixels", n=4097)
    for name in ("dx", "dy"):
        for bad in (NAN, INF, 0.0, -1e-3):
            assert refused(b"dx and dy must be finite and above zero", **{name: bad})
    for bad in (NAN, INF, -1e-6):
        assert refused(b"r finite and not below zero", r=bad)
    assert refused(b"must be 4-byte aligned", f=ctypes.c_void_p((1 << 20) + 2))
    for name, base in (("out", 2 << 20), ("ws", 3 << 20)):
        assert refused(b"must be 8-byte aligned", **{name: ctypes.c_void_p(base + 4)})
    assert refused(b"workspace too small", bytes=need - 1)
    assert refused(b"more than 2^31 - 1 workgroups", S=1 << 16, K=64, n=4096, bytes=1 << 62)


def test_python_front_end_refuses_without_a_gpu():
    import numpy as np
    import pytest
    import torch
    import _center_oracle as O
    from neuralvolumetricreconstructionformedicalimages_amd import center, reconstruct as R
    case = next(c for c in O.CASES if c[0] == "K9")
    geo, angles, cand, q = O.case_inputs(case)
    with pytest.raises(RuntimeError, match="no CPU path"):
        center.slices(torch.tensor(q), geo, angles, cand)
    with pytest.raises(RuntimeError, match="no CPU path"):
        center.metrics(torch.zeros(1, 2, 17, 17), geo, 0.01)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.find_center(torch.zeros(3, 4, 63), geo, angles)
    with pytest.raises(ValueError, match="one view per angle"):
        center.slices(torch.tensor(q)[:, :2], geo, angles, cand)
    with pytest.raises(ValueError, match="finite candidates"):
        center.slices(torch.tensor(q), geo, angles, np.zeros(65))
    with pytest.raises(ValueError, match="finite candidates"):
        center.slices(torch.tensor(q), geo, angles, [np.nan])
    with pytest.raises(ValueError, match="must be float32"):
        center.slices(torch.tensor(q).double(), geo, angles, cand)
    with pytest.raises(ValueError, match="radius must be finite"):
        center.metrics(torch.zeros(1, 2, 17, 17), geo, -1.0)
    with pytest.raises(ValueError, match=r"f must be a float32 tensor \[S, K, 17, 17\]"):
        center.metrics(torch.zeros(1, 2, 16, 17), geo, 0.01)
