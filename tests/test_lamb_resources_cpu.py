"""Register budget of the LAMB kernels (csrc/kernels/lamb.hip), from the compiler's resource
remarks (scripts/prof/kernel_resources.py: a device-only compile with the build's flags, no GPU).
lamb_moments streams 2W + 24 bytes per parameter with about four 8-element register groups live;
scratch or a VGPR spill would multiply its traffic, and no numeric test sees that."""
import os

import pytest

from .test_kernel_resources_cpu import ROOT, _hipcc, _tool


@pytest.fixture(scope="module")
def rows():
    if not os.path.exists(_hipcc()):
        pytest.skip("hipcc is not installed")
    return _tool().kernel_resources(os.path.join(ROOT, "csrc", "kernels", "lamb.hip"))


def test_no_scratch_no_spills(rows):
    names = [r["kernel"] for r in rows]
    # moments: {fp16, fp32} x {vector, scalar} multi-source + 2 dense; apply: {vector, scalar}
    assert sum("lamb_moments_kernel" in k for k in names) == 6, names
    assert sum("lamb_apply_kernel" in k for k in names) == 2, names
    for r in rows:
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0, r
