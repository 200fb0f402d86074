"""--optimizer lamb over the multi-rank data plane on one MI355X (the RCCL stand-in of
tests/test_multirank_gpu.py): the gathered wires go through the multi-source pass of the LAMB
pair, the single-process loopback sums them into the aggregation buffer and takes the dense
entry — both must end in the same bits; the async Python loop applies LAMB push by push."""
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
cfg = PSConfig(model="resnet18", batch_size=64, epochs=1, train_samples=1024, eval_every=0, verbose=0, lr=2e-3,
               max_steps=4, mode="sync", topology={topo!r}, workers={W}, deterministic=True, optimizer="lamb",
               weight_decay=1e-2).validate()
res = {fn}(cfg, log=lambda *a, **k: None)
if "server" in res:
    s = res["server"]
    print("RESULT " + json.dumps([s["final_param_sha256"], s["global_steps_completed"], s["optimizer"],
                                 s["lamb_trust_ratio"], s["lamb"]["steps"]]))
"""


@pytest.mark.parametrize("world,topology", [(2, "colocated"), (3, "dedicated")])
def test_distributed_lamb_sync_matches_loopback(world, topology, tmp_path):
    """A sync run at world 2-3 over the native communicator (wires gathered to rank 0, the
    multi-source lamb_moments + lamb_apply per round, on the Python server: the native rounds
    decline LAMB) ends in the same master state, bit for bit, as run_local with the same W (the
    wires summed into the aggregation buffer by chained fp32 adds, then the dense entry)."""
    W = world - 1 if topology == "dedicated" else world
    dist_py = tmp_path / "dist.py"
    dist_py.write_text(_RUN.format(root=ROOT, fn="run_distributed", topo=topology, W=W))
    out = _torchrun(world, [str(dist_py)])
    got = [r for r in _json_lines(out, "RESULT ") if r]
    loop_py = tmp_path / "loop.py"
    loop_py.write_text(_RUN.format(root=ROOT, fn="run_local", topo="colocated", W=W))
    r = subprocess.run([sys.executable, str(loop_py)], env=_env(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    ref = _json_lines(r.stdout, "RESULT ")[-1]
    assert len(got) == 1 and got[0][1] == ref[1] == 4, (got, ref)
    assert got[0][2] == ref[2] == "lamb" and got[0][4] == ref[4] == 4
    assert got[0][0] == ref[0], (got, ref)
    assert got[0][3] == ref[3] and 0 < ref[3]["min"] <= ref[3]["median"] <= ref[3]["max"], (got, ref)


_ARUN = r"""
import json, sys
sys.path.insert(0, {root!r})
import psx
from psx.parallel.runner import run_distributed
from psx.utils.config import PSConfig
cfg = PSConfig(model="resnet18", batch_size=64, epochs=1, train_samples=1024, eval_every=0, verbose=0, lr=2e-3,
               max_steps=4, mode="async", topology="dedicated", heartbeat_timeout=0, staleness_bound=50,
               optimizer="lamb", weight_decay=1e-2).validate()
res = run_distributed(cfg, log=lambda *a, **k: None)
if "server" in res:
    s = res["server"]
    print("RESULT " + json.dumps([s["async_updates"], s["rejected_pushes"], s["final_param_checksum"],
                                 s["lamb_trust_ratio"], s["lamb"]["steps"]]))
"""


def test_distributed_lamb_async(tmp_path):
    """Async at world 3 (dedicated): LAMB is outside the native event loop's scope, so the Python
    loop serves; every accepted push is one staleness-weighted LAMB update."""
    script = tmp_path / "arun.py"
    script.write_text(_ARUN.format(root=ROOT))
    out = _torchrun(3, [str(script)], extra={"PSX_FAKECOMM_TIMEOUT_S": "240"})
    recs = [r for r in _json_lines(out, "RESULT ") if r]
    assert len(recs) == 1, out[-3000:]
    accepted, rejected, checksum, ratio, steps = recs[0]
    assert accepted > 0 and rejected == 0 and steps == accepted, recs
    assert checksum == checksum and abs(checksum) < 1e12
    assert ratio is not None and 0 < ratio["min"] <= ratio["max"]
