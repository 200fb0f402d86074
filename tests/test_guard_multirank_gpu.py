"""--clip-norm over the multi-rank data plane on one MI355X (the RCCL stand-in of
tests/test_multirank_gpu.py): the dedicated server's native serial round launches the guard's
multi-source entry itself, the Python server does the same from apply_sources, and the
single-process loopback sums the wires into the aggregation buffer and takes the dense entry —
all must end in the same bits, with every round clipped; the async Python loop guards push by push."""
import subprocess
import sys

import pytest

from .test_multirank_gpu import ROOT, _env, _json_lines, _torchrun

pytestmark = pytest.mark.gpu

_RUN = r"""
import json, sys
sys.path.insert(0, {root!r})
import psx
from psx.parallel.runner import {fn}
from psx.utils.config import PSConfig
cfg = PSConfig(model="resnet18", batch_size=64, epochs=1, train_samples=1024, eval_every=0, verbose=0, lr=0.1,
               max_steps=4, mode="sync", topology={topo!r}, workers={W}, deterministic=True, clip_norm=0.5,
               momentum=0.9, weight_decay=5e-4).validate()
res = {fn}(cfg, log=lambda *a, **k: None)
if "server" in res:
    s = res["server"]
    print("RESULT " + json.dumps([s["final_param_sha256"], s["global_steps_completed"], s["gradient_guard"],
                                 s["update_time_source"]]))
"""


def _loopback(tmp_path, W):
    loop_py = tmp_path / "loop.py"
    loop_py.write_text(_RUN.format(root=ROOT, fn="run_local", topo="colocated", W=W))
    r = subprocess.run([sys.executable, str(loop_py)], env=_env(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    return _json_lines(r.stdout, "RESULT ")[-1]


def _distributed(tmp_path, world, topology, W, native_sync):
    dist_py = tmp_path / "dist.py"
    dist_py.write_text(_RUN.format(root=ROOT, fn="run_distributed", topo=topology, W=W))
    out = _torchrun(world, [str(dist_py)], extra={"PSX_NATIVE_SYNC": native_sync})
    got = [r for r in _json_lines(out, "RESULT ") if r]
    assert len(got) == 1, out[-3000:]
    return got[0]


def test_dedicated_sync_native_and_python_rounds_match_loopback(tmp_path):
    """World 3, dedicated: the native serial round (csrc/server/sync_loop.cpp launching
    psx_guard_apply_multi), the Python server's rounds and run_local with W = 2 end in the same
    master state bit for bit, all four rounds clipped. (A native round that ignored the guard
    would apply the unclipped gradient: another sha, and no rounds counted.)"""
    ref = _loopback(tmp_path, 2)
    nat = _distributed(tmp_path, 3, "dedicated", 2, "1")
    py = _distributed(tmp_path, 3, "dedicated", 2, "0")
    assert "native sync loop" in nat[3] and "native sync loop" not in py[3], (nat[3], py[3])
    for got in (nat, py):
        assert got[1] == ref[1] == 4, (got, ref)
        assert got[0] == ref[0], (got, ref)
        g = got[2]
        assert (g["rounds"], g["clipped_rounds"], g["skipped_rounds"]) == (4, 4, 0) and g["clip_norm"] == 0.5, got
        assert g == ref[2], (got, ref)


def test_colocated_sync_matches_loopback(tmp_path):
    ref = _loopback(tmp_path, 2)
    got = _distributed(tmp_path, 2, "colocated", 2, "1")
    assert got[1] == ref[1] == 4 and got[0] == ref[0], (got, ref)
    assert (got[2]["rounds"], got[2]["clipped_rounds"], got[2]["skipped_rounds"]) == (4, 4, 0), got
    assert got[2] == ref[2], (got, ref)


_ARUN = r"""
import json, sys
sys.path.insert(0, {root!r})
import psx
from psx.parallel.runner import run_distributed
from psx.utils.config import PSConfig
cfg = PSConfig(model="resnet18", batch_size=64, epochs=1, train_samples=1024, eval_every=0, verbose=0, lr=0.05,
               max_steps=4, mode="async", topology="dedicated", heartbeat_timeout=0, staleness_bound=50,
               clip_norm=0.5, momentum=0.9, weight_decay=5e-4).validate()
res = run_distributed(cfg, log=lambda *a, **k: None)
if "server" in res:
    s = res["server"]
    print("RESULT " + json.dumps([s["async_updates"], s["rejected_pushes"], s["final_param_checksum"],
                                 s["gradient_guard"]]))
"""


def test_distributed_async_python_loop_guards_every_push(tmp_path):
    """Async at world 3 (dedicated): the guard is outside the native event loop's scope, so the
    Python loop serves; every accepted push is one guarded update."""
    script = tmp_path / "arun.py"
    script.write_text(_ARUN.format(root=ROOT))
    out = _torchrun(3, [str(script)], extra={"PSX_FAKECOMM_TIMEOUT_S": "240"})
    recs = [r for r in _json_lines(out, "RESULT ") if r]
    assert len(recs) == 1, out[-3000:]
    accepted, rejected, checksum, guard = recs[0]
    assert accepted > 0 and rejected == 0, recs
    assert checksum == checksum and abs(checksum) < 1e12
    assert guard["rounds"] == accepted and guard["skipped_rounds"] == 0 and guard["clipped_rounds"] > 0, recs
