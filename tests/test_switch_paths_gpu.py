"""The kernels only an environment variable reaches (read once per process: WTPSE_X3_WGRAD_TW32, WTPSE_X3_MT, WTPSE_X3_HALF_MIN,
WTPSE_TAIL_MAX_WGS), each job of tests/switch_worker.py in a FRESH child process started under its one variable — the environment
copied whole, only that name added, the children one at a time.  The child proves its switch in force, runs its cases and writes the
first_difference messages of every call that is not bit-exact; the list must be empty.  A child that aborts, is killed by a signal,
runs into its time limit or reports an illegal memory access ends the whole run: nothing more is started on the GPU behind it."""
import json
import os
import subprocess
import sys
import time

import pytest

import switch_cases as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "switch_worker.py")
TROUBLE = (134, -6, 139, -11, 124, 137, -9)


@pytest.mark.parametrize("job", list(S.JOBS))
def test_switch_job(job, tmp_path):
    name, value, limit = S.JOBS[job]
    out = str(tmp_path / "out.json")
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, WORKER, job, out], env=dict(os.environ, **{name: value}), stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=limit)
    except subprocess.TimeoutExpired as e:
        tail = (e.stdout or b"")[-1500:]
        pytest.exit("switch job %s (%s=%s) did not finish in %d s; nothing more is started on the GPU.\n%s"
                    % (job, name, value, limit, tail.decode(errors="replace") if isinstance(tail, bytes) else tail), returncode=3)
    tail = "\n".join(r.stdout.splitlines()[-25:])
    if r.returncode in TROUBLE or "illegal memory access" in r.stdout:
        pytest.exit("switch job %s (%s=%s) ended with status %d; nothing more is started on the GPU.\n%s"
                    % (job, name, value, r.returncode, tail), returncode=3)
    print("switch job %s: %.1f s in the parent's clock\n%s" % (job, time.time() - t0, tail))
    assert r.returncode == 0, tail
    with open(out) as f:
        res = json.load(f)
    assert res["proof"] and res["calls"] > 0, res
    assert res["failures"] == [], "%d call(s) not bit-exact under %s=%s:\n  %s" % (len(res["failures"]), name, value, "\n  ".join(res["failures"][:12]))
