"""One recorded step of each bench workload at its bench shape launches exactly the recorded sequence of (kind, flops) -- which kernel family
ran every layer, in launch order (tests/_route_trace.py; tests/golden/route_traces.json).  A change of a route, a threshold or the layer
order of a model has to update that file on purpose.  The default plan runs in the default selection, the plan variants with --slow."""
import json
import os
import subprocess
import sys

import pytest

import _route_trace as RT

pytestmark = pytest.mark.gpu
CASES = [pytest.param(w, p, marks=() if p == "default" else pytest.mark.slow, id="%s@%s" % (w, p)) for p in RT.PLANS for w in RT.WORKLOADS]


@pytest.mark.parametrize("workload,plan", CASES)
def test_route_trace(workload, plan, tmp_path):
    want = RT.load("%s@%s" % (workload, plan))
    out = str(tmp_path / "trace.json")
    env = dict(os.environ, CATSEG_PLAN="" if plan == "default" else plan)
    # a fresh process: the plan's start-up values come from the environment, and its GPU state is its own
    p = subprocess.run([sys.executable, os.path.join(RT.ROOT, "tests", "_route_trace.py"), workload, out], env=env, timeout=600,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-3000:]
    got = json.load(open(out))
    assert len(want) > 100
    assert RT.diff(got, want) is None, RT.diff(got, want)
