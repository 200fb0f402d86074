"""--optimizer adamw over the multi-rank data plane on one MI355X (the RCCL stand-in of
tests/test_multirank_gpu.py): bucketed rounds (per-bucket apply_range_sources on the Python server),
serial rounds, the sharded server and the async Python loop. The update is element-wise and the
sources are summed in worker order everywhere, so the sync runs must end in the loopback's bits."""
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
cfg = PSConfig(model="resnet18", batch_size=64, epochs=1, train_samples=1024, eval_every=0, verbose=0, lr=1e-3,
               max_steps=4, mode="sync", topology={topo!r}, workers={W}, deterministic=True, optimizer="adamw",
               weight_decay=1e-2, overlap={overlap!r}).validate()
res = {fn}(cfg, log=lambda *a, **k: None)
if "server" in res:
    s = res["server"]
    print("RESULT " + json.dumps([s["final_param_sha256"], s["global_steps_completed"], s["optimizer"],
                                 s["adamw"]["steps"], s["final_param_checksum"]]))
"""

_LOOPBACK = {}


def _loopback(W, tmp_path):
    """run_local with W simulated workers, once per W for the whole module."""
    if W not in _LOOPBACK:
        loop_py = tmp_path / "loop.py"
        loop_py.write_text(_RUN.format(root=ROOT, fn="run_local", topo="colocated", W=W, overlap=None))
        r = subprocess.run([sys.executable, str(loop_py)], env=_env(), stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
        _LOOPBACK[W] = _json_lines(r.stdout, "RESULT ")[-1]
    return _LOOPBACK[W]


@pytest.mark.parametrize("overlap", [None, False])
@pytest.mark.parametrize("world,topology", [(2, "colocated"), (3, "dedicated")])
def test_distributed_adamw_sync_matches_loopback(world, topology, overlap, tmp_path):
    """Sync at world 2-3 over the native communicator, on the Python server (the native rounds
    decline adamw): the default bucketed round (overlap None resolves to on) and the serial round
    (overlap False) end in run_local's master state with the same W, bit for bit."""
    W = world - 1 if topology == "dedicated" else world
    dist_py = tmp_path / "dist.py"
    dist_py.write_text(_RUN.format(root=ROOT, fn="run_distributed", topo=topology, W=W, overlap=overlap))
    out = _torchrun(world, [str(dist_py)])
    got = [r for r in _json_lines(out, "RESULT ") if r]
    ref = _loopback(W, tmp_path)
    assert len(got) == 1 and got[0][1] == ref[1] == 4, (got, ref)
    assert got[0][2] == ref[2] == "adamw" and got[0][3] == ref[3] == 4
    assert got[0][0] == ref[0], (got, ref)


def test_distributed_adamw_sharded_matches_loopback(tmp_path):
    """--topology sharded at world 2: every rank applies its range with its slices of the moments
    and its own step count. The assertion of the SGD sharded test
    (test_rccl_native_gpu.test_sharded_server_world1_matches_rank0_server): equal step counts and
    checksums within 2e-4."""
    dist_py = tmp_path / "dist.py"
    dist_py.write_text(_RUN.format(root=ROOT, fn="run_distributed", topo="sharded", W=2, overlap=None))
    out = _torchrun(2, [str(dist_py)])
    got = [r for r in _json_lines(out, "RESULT ") if r]
    ref = _loopback(2, tmp_path)
    assert len(got) == 1 and got[0][1] == ref[1] == 4, (got, ref)
    assert got[0][2] == "adamw" and got[0][3] == 4
    a, b = got[0][4], ref[4]
    assert abs(a - b) <= 2e-4 * max(abs(a), abs(b)), (got, ref)


_ARUN = r"""
import json, sys
sys.path.insert(0, {root!r})
import psx
from psx.parallel.runner import run_distributed
from psx.utils.config import PSConfig
cfg = PSConfig(model="resnet18", batch_size=64, epochs=1, train_samples=1024, eval_every=0, verbose=0, lr=1e-3,
               max_steps=4, mode="async", topology="dedicated", heartbeat_timeout=0, staleness_bound=50,
               optimizer="adamw", weight_decay=1e-2).validate()
res = run_distributed(cfg, log=lambda *a, **k: None)
if "server" in res:
    s = res["server"]
    print("RESULT " + json.dumps([s["async_updates"], s["rejected_pushes"], s["final_param_checksum"],
                                 s["optimizer"], s["adamw"]["steps"]]))
"""


def test_distributed_adamw_async(tmp_path):
    """Async at world 3 (dedicated): adamw is outside the native event loop's scope, so the Python
    loop serves; every accepted push is one staleness-weighted AdamW update."""
    script = tmp_path / "arun.py"
    script.write_text(_ARUN.format(root=ROOT))
    out = _torchrun(3, [str(script)], extra={"PSX_FAKECOMM_TIMEOUT_S": "240"})
    recs = [r for r in _json_lines(out, "RESULT ") if r]
    assert len(recs) == 1, out[-3000:]
    accepted, rejected, checksum, opt, steps = recs[0]
    assert accepted > 0 and rejected == 0, recs
    assert checksum == checksum and abs(checksum) < 1e12
    assert opt == "adamw" and steps == accepted
