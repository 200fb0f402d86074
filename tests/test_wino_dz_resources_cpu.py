"""Register / scratch budget of the merged backward transform (csrc/kernels/wino.hip
wino_dz_xf_kernel, plain and with either BN-backward fold), from the compiler's resource remarks
(scripts/prof/kernel_resources.py: a device-only compile with the build's flags, no GPU). It is a
memory-bound kernel that lives on many resident waves: scratch or a VGPR spill would put its
double-buffered loads behind stack traffic, and no numeric test sees that."""
import os
import re

import pytest

from .test_kernel_resources_cpu import ROOT, _hipcc, _tool


@pytest.fixture(scope="module")
def rows():
    if not os.path.exists(_hipcc()):
        pytest.skip("hipcc is not installed")
    out = {}
    for r in _tool().kernel_resources(os.path.join(ROOT, "csrc", "kernels", "wino.hip")):
        m = re.match(r"(?:void )?(?:psx::)?wino_dz_xf_kernel<(.*?)>\(", r["kernel"])
        if m:
            out[m.group(1)] = r
    return out


def test_no_scratch_no_spills(rows):
    assert sorted(rows) == ["0", "1", "2"], rows.keys()  # plain, the shared fold, the apply-rounded fold
    for name, r in rows.items():
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0, (name, r)
        # two 6x6 + two 4x6 hand-over buffers of 64 channels and, with the fold, the three coefficients
        assert r["lds"] == 4 * (2 * 6 * 6 * 64 + 2 * 4 * 6 * 64 + (3 * 64 if name != "0" else 0)), (name, r)
        # 6 waves per workgroup: at least two workgroups per CU (3 waves per SIMD)
        assert r["occupancy"] >= 3, (name, r)
