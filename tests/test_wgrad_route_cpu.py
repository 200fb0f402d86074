"""The weight gradient's launch decision (csrc/kernels/wgrad_v2.hip route_wgrad) through its host
query K.conv_wgrad2_path: a golden table over the ResNet-18 / ResNet-50 layers and one named case
per route kind. Host code only: runs without a GPU.

tests/golden/wgrad_routes.json. Cases: the 11 ResNet-18 (CIFAR) conv shapes at batches 1, 2, 3, 8,
32, 64, 128, 256, 512 and the 20 ResNet-50 (ImageNet) conv shapes of tests/test_conv_v2_gpu.py at
batches 1, 2, 4, 8, 16, 32, 64, in bf16 and fp32, cp / kg by ConvSpec.finalize's rule: 478 rows.
The ``splits`` column was recorded with K.conv_wgrad2_splits on the commit before the route
existed (four hand-copied planners), so the table pins the plans across that refactor; the other
columns are the route's."""
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_routes.json")


def _table():
    with open(GOLDEN) as f:
        t = json.load(f)
    return [dict(zip(t["columns"], r)) for r in t["rows"]]


def _pow2_ceil(v, lo):
    p = lo
    while p < v:
        p *= 2
    return p


def test_golden_table_cases():
    """The table holds the cases its docstring names, padded by ConvSpec.finalize's rule."""
    rows = _table()
    assert len(rows) == 478
    r18 = [r for r in rows if r["hw"] in (32, 16, 8, 4)]
    r50 = [r for r in rows if r["hw"] in (224, 56, 28, 14, 7)]
    assert len(r18) == 11 * 9 * 2 and len(r50) == 20 * 7 * 2
    assert sorted({r["n"] for r in r18}) == [1, 2, 3, 8, 32, 64, 128, 256, 512]
    assert sorted({r["n"] for r in r50}) == [1, 2, 4, 8, 16, 32, 64]
    assert len({tuple(r[k] for k in ("n", "cin", "cout", "hw", "k", "stride", "pad", "f32")) for r in rows}) == 478
    for r in rows:
        assert r["cp"] == _pow2_ceil(r["cin"], 4 if r["f32"] else 8), r
        assert r["kg"] == -(-(r["k"] * r["k"] * r["cp"]) // 64) * 64, r


def test_golden_routes():
    """Every row's whole route; K.conv_wgrad2_splits answers the same split count."""
    from psx.ops import kernels as K
    bad = []
    for r in _table():
        args = (r["n"], r["hw"], r["hw"], r["cp"], r["cout"], r["k"], r["stride"], r["pad"], r["kg"], bool(r["f32"]))
        want = dict(kind=r["kind"], f32=bool(r["f32"]), br=r["br"], bc=r["bc"], ns=r["ns"], splits=r["splits"],
                    kps=r["kps"], pix=r["pix"])
        got = K.conv_wgrad2_path(*args)
        if got != want or K.conv_wgrad2_splits(*args) != r["splits"]:
            bad.append((args, want, got))
    assert not bad, bad[:5]


# (id, (n, h/w, ic, oc, k, stride, pad, f32), expected kind, br, bc, ns): one per route kind and dtype
NAMED = [
    ("tile_bf16_1x1", (8, 56, 64, 64, 1, 1, 0, False), "tile", 64, 64, 3),
    ("tile_bf16_wide_oc", (8, 28, 128, 512, 1, 1, 0, False), "tile", 64, 128, 3),
    ("tile_bf16_wide_k", (59, 14, 512, 64, 3, 1, 1, False), "tile", 128, 64, 3),
    ("tile_f32_strided", (128, 32, 64, 128, 3, 2, 1, True), "tile", 64, 64, 3),
    ("tile_f32_wide_k", (3, 32, 256, 512, 3, 2, 1, True), "tile", 128, 64, 3),
    ("tap_reuse_bf16", (128, 32, 64, 64, 3, 1, 1, False), "tap_reuse", 192, 64, 3),
    ("tap_reuse_bf16_deep_ring", (1, 8, 64, 64, 3, 1, 1, False), "tap_reuse", 192, 64, 6),
    ("tap_reuse_f32", (128, 16, 128, 128, 3, 1, 1, True), "tap_reuse", 192, 64, 3),
    ("tap_reuse_general_bf16", (8, 28, 128, 128, 3, 1, 1, False), "tap_reuse_general", 192, 64, 6),
    ("tap_reuse_general_bf16_3_stages", (2, 28, 256, 512, 3, 1, 1, False), "tap_reuse_general", 192, 64, 3),
    ("tap_reuse_general_bf16_width_4", (7, 4, 512, 1024, 3, 1, 1, False), "tap_reuse_general", 192, 64, 3),
    ("stem7_f32", (4, 224, 4, 64, 7, 2, 3, True), "stem7", 0, 0, 0),
]


@pytest.mark.parametrize("case", NAMED, ids=[c[0] for c in NAMED])
def test_named_route(case):
    from psx.ops import kernels as K
    _, (n, hw, ic, oc, k, s, p, f32), kind, br, bc, ns = case
    kg = -(-(k * k * ic) // 64) * 64
    path = K.conv_wgrad2_path(n, hw, hw, ic, oc, k, s, p, kg, f32)
    assert isinstance(path, dict), ("refused", path)
    assert (path["kind"], path["f32"], path["br"], path["bc"], path["ns"]) == (kind, f32, br, bc, ns), path
    assert path["splits"] == K.conv_wgrad2_splits(n, hw, hw, ic, oc, k, s, p, kg, f32)
    # the splits cover the pixels: kps steps of pix pixels each, the last split not empty
    if kind != "stem7":
        oh = (hw + 2 * p - k) // s + 1
        steps = -(-(n * oh * oh) // path["pix"])
        assert (path["splits"] - 1) * path["kps"] < steps <= path["splits"] * path["kps"], path


def test_refusals():
    """The codes conv_wgrad2 refuses a geometry with come back from the query as they are."""
    from psx.ops import kernels as K
    assert K.conv_wgrad2_path(8, 16, 16, 64, 96, 3, 1, 1, 576, False) == -2    # OC % 64
    assert K.conv_wgrad2_path(8, 16, 16, 64, 64, 3, 1, 1, 600, False) == -2    # Kg % 64
    assert K.conv_wgrad2_path(8, 16, 16, 48, 64, 1, 1, 0, 64, True) == -2      # fp32 tile: IC no power of two
    with pytest.raises(RuntimeError):
        K.conv_wgrad2_splits(8, 16, 16, 64, 96, 3, 1, 1, 576, False)
