"""Register / spill / LDS budget of every wino_fused_kernel instantiation, from the compiler's
resource remarks (scripts/prof/kernel_resources.py: a device-only compile with the build's flags,
no GPU). The kernel lives at two waves per SIMD with one workgroup per CU: a VGPR spill, scratch or
a lost wave is a regression that no numeric test sees. Numbers come from the remarks only."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("_kernel_resources",
                                                  os.path.join(ROOT, "scripts", "prof", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _hipcc():
    spec = importlib.util.spec_from_file_location("_psx_build", os.path.join(ROOT, "csrc", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.HIPCC


# SGPR spills the kernel reaches per input kind (template parameter IN, profiles/README.md,
# profiles/r7_wino_fused_resources.jsonl): PLAIN none; BNIN 12-16, all in the BN finalize prologue
# (once per workgroup); BWDIN 26-33, the padding selects it keeps because it has no VGPRs for the
# masks. The parent had 93-110 everywhere.
# These numbers belong to the hipcc that built them. Two constructs in the kernel exist only to
# steer its register allocation (BWDIN tests its flag at run time; the B load past the last k-step
# stays), and this test is their only guard: it is skipped where hipcc is absent, and a compiler
# bump that trips it means re-deriving those two choices and these bounds, not a wrong result.
SGPR_SPILL_BOUND = {0: 0, 1: 16, 2: 33}
# <GG, RES, BWD, MAFF, TWO, IN, HASV> of the launches of the fp32 ResNet-18 step (batch 128) and the
# SGPR spills each one has
HEADLINE = {"4, false, false, false, false, 0, false": 0, "4, false, false, false, false, 1, false": 12,
            "4, false, true, true, false, 2, false": 27, "4, true, true, false, false, 2, false": 29,
            "8, false, false, false, false, 0, false": 0, "8, false, false, false, false, 1, false": 12,
            "8, false, true, true, false, 0, false": 0, "8, false, true, true, false, 2, false": 26,
            "8, true, true, false, true, 2, false": 33}


@pytest.fixture(scope="module")
def rows():
    if not os.path.exists(_hipcc()):
        pytest.skip("hipcc is not installed")
    out = {}
    for r in _tool().kernel_resources(os.path.join(ROOT, "csrc", "kernels", "wino_fused.hip")):
        m = re.match(r"wino_fused_kernel<(.*?)>\(", r["kernel"])
        assert m, r["kernel"]
        out[m.group(1)] = r
    return out


def test_every_instantiation_fits(rows):
    assert len(rows) == 52  # forward 2 x 2 x (2 x 2 + 1), data gradient 2 x 2 x 4 x 2
    for name, r in rows.items():
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0, (name, r)
        assert r["lds"] <= 163840, (name, r)
        assert r["occupancy"] >= 2, (name, r)
        kind = int(name.split(", ")[5])
        assert r["sgpr_spills"] <= SGPR_SPILL_BOUND[kind], (name, r)


def test_headline_instantiations(rows):
    for name, spills in HEADLINE.items():
        assert name in rows, name
        assert rows[name]["sgpr_spills"] <= spills, (name, rows[name])


def test_remark_parser():
    text = ("k.hip:16:1: remark: Function Name: _Z1kv [-Rpass-analysis=kernel-resource-usage]\n"
            "   16 | void k() {\n"
            "k.hip:16:1: remark:     TotalSGPRs: 63 [-Rpass-analysis=kernel-resource-usage]\n"
            "k.hip:16:1: remark:     VGPRs: 46 [-Rpass-analysis=kernel-resource-usage]\n"
            "k.hip:16:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]\n"
            "k.hip:16:1: remark:     Dynamic Stack: False [-Rpass-analysis=kernel-resource-usage]\n"
            "k.hip:16:1: remark:     Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]\n"
            "k.hip:16:1: remark:     SGPRs Spill: 3 [-Rpass-analysis=kernel-resource-usage]\n"
            "k.hip:16:1: remark:     VGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]\n"
            "k.hip:16:1: remark:     LDS Size [bytes/block]: 1024 [-Rpass-analysis=kernel-resource-usage]\n")
    assert _tool().parse_remarks(text) == [{"kernel": "_Z1kv", "sgprs": 63, "vgprs": 46, "scratch": 0, "occupancy": 8,
                                            "sgpr_spills": 3, "vgpr_spills": 0, "lds": 1024}]
