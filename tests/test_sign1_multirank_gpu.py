"""--codec sign1 over the multi-rank data plane on one MI355X (the RCCL stand-in of
tests/test_multirank_gpu.py): gathered payloads applied by sign1_apply_multi end in the same bits
as the single-process loopback (decode into a dense sum + sgd_apply), and the async Python loop
receives and applies sign1 payloads. The two tests of tests/test_q8_multirank_gpu.py, whose run
scripts are reused with the codec's name replaced."""
import subprocess
import sys

import pytest

from .test_multirank_gpu import ROOT, _env, _json_lines, _torchrun
from .test_q8_multirank_gpu import _ARUN, _RUN

pytestmark = pytest.mark.gpu

N = 11_220_132  # ResNet-18 (100 classes) trainable parameters


def _sign1(script: str) -> str:
    assert script.count('codec="q8"') == 1
    return script.replace('codec="q8"', 'codec="sign1"')


@pytest.mark.parametrize("world,topology", [(2, "colocated"), (3, "dedicated")])
def test_distributed_sign1_sync_matches_loopback(world, topology, tmp_path):
    """A sync run at world 2-3 over the native communicator (payloads gathered to rank 0, one
    sign1_apply_multi launch per round) ends in the same master state, bit for bit, as run_local
    with the same W (each payload decoded into the dense sum, then sgd_apply), and counts the
    same bytes: W whole payloads per round."""
    from psx.parallel import sign1 as S

    W = world - 1 if topology == "dedicated" else world
    dist_py = tmp_path / "dist.py"
    dist_py.write_text(_sign1(_RUN).format(root=ROOT, fn="run_distributed", topo=topology, W=W))
    out = _torchrun(world, [str(dist_py)])
    got = [r for r in _json_lines(out, "RESULT ") if r]
    loop_py = tmp_path / "loop.py"
    loop_py.write_text(_sign1(_RUN).format(root=ROOT, fn="run_local", topo="colocated", W=W))
    r = subprocess.run([sys.executable, str(loop_py)], env=_env(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    ref = _json_lines(r.stdout, "RESULT ")[-1]
    assert len(got) == 1 and got[0][1] == ref[1] == 4, (got, ref)
    assert got[0][0] == ref[0], (got, ref)
    assert got[0][2] == ref[2] == 4 * W * S.payload_bytes(N), (got, ref)


def test_distributed_sign1_async(tmp_path):
    """Async at world 3 (dedicated): sign1 is outside the native event loop's scope, so the Python
    loop serves; every push arrives as one whole payload and is applied by the one-source
    sign1_apply_multi."""
    from psx.parallel import sign1 as S

    script = tmp_path / "arun.py"
    script.write_text(_sign1(_ARUN).format(root=ROOT))
    out = _torchrun(3, [str(script)], extra={"PSX_FAKECOMM_TIMEOUT_S": "240"})
    recs = [r for r in _json_lines(out, "RESULT ") if r]
    assert len(recs) == 1, out[-3000:]
    accepted, rejected, nbytes, checksum = recs[0]
    assert accepted > 0 and rejected == 0, recs
    assert nbytes == accepted * S.payload_bytes(N), recs
    assert checksum == checksum and abs(checksum) < 1e12
