"""The invariants of the server update kernels' fingerprints (scripts/update_kernel_bits.py) that
need no parent build to compare with: on every cell of the script, at its sizes, the 16-byte
aligned and the one-element-offset views of the same data end in the same bits, a multi-source
entry ends in the bits of its dense entry fed the fp32 sum, and two runs agree.

The alignment invariant is what found dc_apply's adaptive form rounding its mean-square update one
way in the 8-per-lane body and another way in the scalar form (profiles/update_kernels_shared.txt,
3): csrc/kernels/dcasgd.hip now spells that fma out."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script():
    spec = importlib.util.spec_from_file_location("_psx_update_kernel_bits",
                                                  os.path.join(ROOT, "scripts", "update_kernel_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def bits():
    """(script module, host inputs, table layout, {cell: hashes} of one run over every cell)."""
    B = _script()
    H, lay = B.host_inputs(), B.table_layout()
    return B, H, lay, {c: B.run_cell(c, H, lay) for c in B.cells()}


def test_cells_cover_every_entry(bits):
    B, _, _, run = bits
    assert {c.entry for c in run} == set(B.ENTRIES)
    for c, h in run.items():
        assert "p" in h and ("img" in h) == bool(c.img), c


def test_alignment_does_not_change_the_bits(bits):
    _, _, _, run = bits
    pairs = [(c, c._replace(off=1)) for c in run if c.off == 0]
    assert pairs
    for a, b in pairs:
        assert run[a] == run[b], (a, run[a], run[b])


def test_multi_equals_dense_fed_the_fp32_sum(bits):
    B, H, lay, run = bits
    checked = 0
    for c, h in run.items():
        if c.entry in B.DENSE_OF:  # the staged updates have a dense entry of their own
            dense = c._replace(entry=B.DENSE_OF[c.entry])
            assert h == run[dense], (c, h, run[dense])
        elif c.entry in ("sgd_apply_multi", "adamw_apply_multi"):  # theirs is one fp32 source
            d = B.run_cell(c, H, lay, dense_sum=True)
            assert h == d, (c, h, d)
        else:
            continue
        checked += 1
    assert checked == sum(c.entry.endswith("_multi") for c in run)


def test_two_runs_agree(bits):
    B, H, lay, run = bits
    for c, h in run.items():
        again = B.run_cell(c, H, lay)
        assert h == again, (c, h, again)
