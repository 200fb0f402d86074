"""--fetch-codec q8delta over the multi-rank data plane on one MI355X (the RCCL stand-in of
tests/test_multirank_gpu.py): a sync job whose fetches are one fp32 keyframe and then int8 deltas
ends in the same master state, bit for bit, as the single-process loopback with the same workers;
every worker holds exactly the server's shadow; and the fetched bytes are what the wire says."""
import subprocess
import sys

import pytest

from .test_multirank_gpu import ROOT, _env, _json_lines, _torchrun

pytestmark = pytest.mark.gpu

ARENA = 11_229_732  # ResNet-18 (100 classes): 11,220,132 trainable parameters + 9,600 BN running statistics

_RUN = r"""
import json, sys
sys.path.insert(0, {root!r})
import psx
from psx.parallel.runner import {fn}
from psx.utils.config import PSConfig
cfg = PSConfig(model="resnet18", batch_size=64, epochs=1, train_samples=1024, eval_every=0, verbose=0, lr=0.1,
               max_steps=4, mode="sync", topology={topo!r}, workers={W}, deterministic=True, codec={codec!r},
               fetch_codec="q8delta").validate()
res = {fn}(cfg, log=lambda *a, **k: None)
wk = res["workers"] if "workers" in res else [res["worker"]]
out = dict(workers=[w["local_arena_sha256"] for w in wk if w])
if "server" in res:
    s = res["server"]
    out.update(final=s["final_param_sha256"], shadow=s["fetch_shadow_sha256"], steps=s["global_steps_completed"],
               fetched=s["bytes_fetched"], pushed=s["bytes_pushed"])
print("RESULT " + json.dumps(out))
"""


def _loopback(codec, W, tmp_path, tag=""):
    """run_local with W simulated workers, once per (codec, W, tag)."""
    key = (codec, W, tag)
    if key not in _loopback.cache:
        py = tmp_path / f"loop_{codec}_{W}{tag}.py"
        py.write_text(_RUN.format(root=ROOT, fn="run_local", topo="colocated", W=W, codec=codec))
        r = subprocess.run([sys.executable, str(py)], env=_env(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
        _loopback.cache[key] = _json_lines(r.stdout, "RESULT ")[-1]
    return _loopback.cache[key]


_loopback.cache = {}


def _distributed(world, topology, codec, tmp_path):
    W = world - 1 if topology == "dedicated" else world
    py = tmp_path / "dist.py"
    py.write_text(_RUN.format(root=ROOT, fn="run_distributed", topo=topology, W=W, codec=codec))
    recs = [r for r in _json_lines(_torchrun(world, [str(py)]), "RESULT ") if r]
    srv = [r for r in recs if "final" in r]
    assert len(recs) == world and len(srv) == 1, recs
    return srv[0], [s for r in recs for s in r["workers"]], W


def _check(srv, workers, W, remote, ref):
    from psx.parallel import q8 as Q

    assert srv["steps"] == ref["steps"] == 4, (srv, ref)
    assert srv["final"] == ref["final"], (srv, ref)
    # every worker, on rank 0 or not, holds the server's shadow; the master has moved on since
    assert len(workers) == W and workers == [srv["shadow"]] * W, (srv, workers)
    assert ref["workers"] == [ref["shadow"]] * W, ref
    assert srv["shadow"] == ref["shadow"] != srv["final"], (srv, ref)
    # one fp32 keyframe and three payloads for every worker on another rank
    assert srv["fetched"] == remote * (4 * ARENA + 3 * Q.payload_bytes(ARENA)), srv


@pytest.mark.parametrize("world,topology", [(2, "colocated"), (3, "dedicated")])
def test_distributed_q8delta_sync_matches_loopback(world, topology, tmp_path):
    srv, workers, W = _distributed(world, topology, "fp16", tmp_path)
    _check(srv, workers, W, W - 1 if topology == "colocated" else W, _loopback("fp16", W, tmp_path))


def test_distributed_sign1_push_and_q8delta_fetch(tmp_path):
    """Both directions compressed: the sign1 push payloads and the q8delta fetch."""
    from psx.parallel import sign1 as S

    srv, workers, W = _distributed(2, "colocated", "sign1", tmp_path)
    ref = _loopback("sign1", W, tmp_path)
    _check(srv, workers, W, W - 1, ref)
    assert srv["pushed"] == ref["pushed"] == 4 * W * S.payload_bytes(11_220_132), (srv, ref)


def test_loopback_runs_are_reproducible(tmp_path):
    a, b = _loopback("fp16", 2, tmp_path), _loopback("fp16", 2, tmp_path, tag="_again")
    assert a["final"] == b["final"] and a["shadow"] == b["shadow"] and a["workers"] == b["workers"], (a, b)
