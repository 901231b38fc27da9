"""-m gpu: one test per case of tests/kernel_ledger_mjpegdec.py, run as tests/test_kernel_ledger_jpegdec_gpu.py runs its cases
(launch log on, the kernels that list the case the only ones launched, exact equality).  The valid cases run ahead of the
malformed scans, which are the ledger's last; those of a sampling run once, in a process of their own under a time limit, so that a
decoder which did not come back from one would end that process and fail the test."""
import json
import os
import subprocess
import sys

import pytest

import kernel_ledger_mjpegdec
from kernel_ledger import Outcome

pytestmark = pytest.mark.gpu

CASES = kernel_ledger_mjpegdec.cases()
TESTS = os.path.dirname(os.path.abspath(__file__))
LIMIT_S = 120           # the import of torch and the library, five batches of three small files: seconds
CHILD = ("import json, sys; import kernel_ledger_mjpegdec as k; o = k.broken(sys.argv[1]); "
         "print('OUTCOME ' + json.dumps([sorted(o.launched), o.err, o.bar, o.what]))")


def _in_a_child(name) -> Outcome:
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(TESTS), TESTS] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    res = subprocess.run([sys.executable, "-c", CHILD, name], capture_output=True, text=True, env=env, cwd=TESTS, timeout=LIMIT_S)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("OUTCOME ")][-1]
    launched, err, bar, what = json.loads(line[len("OUTCOME "):])
    return Outcome(frozenset(launched), float(err), float(bar), what)


@pytest.mark.parametrize("kernels,case", [(k, c) for k, _, c in CASES], ids=[f"mjpegdec-{i}" for _, i, _ in CASES])
def test_mjpegdec_kernel_instances(kernels, case):
    out = _in_a_child(*case.params) if case.fn is kernel_ledger_mjpegdec.broken else case.run()
    assert sorted(out.launched) == kernels, f"{case} launched {sorted(out.launched)}, not {kernels}"
    print(f"{case}: {out.what}: {out.err:.0f} bytes differ")
    assert out.err <= out.bar, f"{out.what}: {out.err} bytes differ"
