"""The two walks of csrc/siddon_device.h on the CPU (DESIGN.md sections 20 to 22): tools/siddon_host_check.cpp, built once with
AddressSanitizer and UBSan and run as a process of its own, holds siddon_forward and siddon_transpose bit for bit to its ungrouped
restatement of the walk, and tools/siddon_host_check.py holds their sums to the float64 oracles.  Here it runs on the hand-made ray
sets of both oracles (ties, grazes, constant axes, zero components, NaN / Inf: each at most 32 rays, the smallest of either oracle
among them) with the three value vectors; `python tools/siddon_host_check.py` runs the scan and random sets as well."""
import numpy as np
import pytest

import _host_check
import _siddon_oracle as S
import _siddon_transpose_oracle as T

D = _host_check.load("siddon")
SMALL = [name for name, case in T.ray_sets().items() if len(case[3]) <= 32]

pytestmark = _host_check.needs_compiler


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """(the program, a directory for its files), built once."""
    workdir = str(tmp_path_factory.mktemp("siddon_host_check"))
    return D.build(workdir), workdir


def test_the_small_sets_hold_the_smallest_of_each_oracle():
    for sets in (S.ray_sets(), T.ray_sets()):
        assert min(sets, key=lambda name: len(sets[name][3])) in SMALL
    assert "h non-finite" in SMALL and len(SMALL) >= 5


@pytest.mark.parametrize("name", SMALL)
def test_walks_equal_their_restatement(program, name):
    """Exit status 0, nothing on stderr and zero mismatches (`walk` raises otherwise) for mixed-sign values, every seventh 0 and
    NaN / 0 / Inf; the counts of sent terms are the oracle's and every sum is inside its float64 bound."""
    exe, workdir = program
    dims, dvoxel, volume, rays = T.ray_sets()[name]
    assert D.check_set(S, T, exe, workdir, name, dims, dvoxel, volume, rays) <= 1.0


def test_non_finite_rays_give_nan_or_zero(program):
    """P6's convention on the program's output: NaN where the span is not finite, 0 where it is empty."""
    exe, workdir = program
    dims, dvoxel, volume, rays = T.ray_sets()["h non-finite"]
    want, _ = S.project_rays(volume, dvoxel, rays)
    got = D.walk(exe, workdir, volume, dvoxel, rays)["acc"]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.all(got[~np.isnan(want)] == 0), (got, want)
