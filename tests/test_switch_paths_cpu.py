"""Host side of the launch paths behind environment switches (tests/switch_cases.py, tests/switch_worker.py; profiles/switch_paths.md).
The registry is complete — every WTPSE_ name the library or the package reads is listed with a job, a test or a written reason, and
nothing is listed that is no longer read —, and every job of the worker, started in a child process under its variable with --host,
proves its switch in force and finds its cases in the branches they are listed under.  No GPU."""
import json
import os
import re
import subprocess
import sys

import pytest

import switch_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "switch_worker.py")
PKG = os.path.join(ROOT, "wt-pse-code_amd", "wtpse_hip")


def names_read():
    """{name: [files]} of getenv("WTPSE_...") under csrc/ and environ.get("WTPSE_...") in the package's Python."""
    found = {}
    for base, _, files in os.walk(PKG):
        if os.path.basename(base) in ("_obj", "__pycache__"):
            continue
        for f in files:
            path = os.path.join(base, f)
            in_csrc = os.path.basename(base) == "csrc"
            if in_csrc and f.endswith((".hip", ".h", ".inc")):
                pat = r'getenv\("(WTPSE_[A-Z0-9_]+)"\)'
            elif not in_csrc and f.endswith(".py"):
                pat = r'environ\.get\("(WTPSE_[A-Z0-9_]+)"'
            else:
                continue
            with open(path, errors="replace") as fh:
                for name in re.findall(pat, fh.read()):
                    found.setdefault(name, []).append(os.path.relpath(path, ROOT))
    return found


def test_every_switch_has_a_case_or_a_reason():
    found = names_read()
    assert len(found) >= 25, sorted(found)                  # the scan itself works
    missing = sorted(set(found) - set(S.SWITCHES))
    assert not missing, "switches without a case or a written reason in tests/switch_cases.py: %s" % {n: found[n] for n in missing}
    stale = sorted(set(S.SWITCHES) - set(found))
    assert not stale, "tests/switch_cases.py lists switches nothing reads any more: %s" % stale
    for name, entry in S.SWITCHES.items():
        if isinstance(entry, str):
            path, _, test = entry.partition("::")
            with open(os.path.join(ROOT, path)) as fh:
                assert re.search(r"^def %s\(" % re.escape(test), fh.read(), re.M), (name, entry)
        elif entry[0] == "job":
            assert entry[1:] and all(j in S.JOBS and S.JOBS[j][0] == name for j in entry[1:]), (name, entry)
        else:
            assert entry[0] == "exempt" and len(entry) == 2 and len(entry[1]) > 30, (name, entry)
    used = {j for e in S.SWITCHES.values() if not isinstance(e, str) and e[0] == "job" for j in e[1:]}
    assert used == set(S.JOBS)


@pytest.mark.parametrize("job", list(S.JOBS))
def test_job_proves_its_switch_on_the_host(job, tmp_path):
    """The worker's --host mode in a child under the job's variable: the proof queries and the branches of its cases."""
    name, value, _ = S.JOBS[job]
    out = str(tmp_path / "out.json")
    r = subprocess.run([sys.executable, WORKER, job, out, "--host"], env=dict(os.environ, **{name: value}), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(out) as f:
        res = json.load(f)
    assert res["failures"] == [], res["failures"]
    assert res["proof"], res


@pytest.mark.parametrize("job", [j for j in S.JOBS if j != "tail0"])
def test_job_fails_without_its_switch(job, tmp_path):
    """Without the variable the same job must refuse: it never silently tests the default path."""
    name, value, _ = S.JOBS[job]
    out = str(tmp_path / "out.json")
    env = dict(os.environ, **{name: "0" if value != "0" else "1"})
    r = subprocess.run([sys.executable, WORKER, job, out, "--host"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(out) as f:
        res = json.load(f)
    assert res["failures"] and all(m.startswith("switch not proved in force") for m in res["failures"]), res
