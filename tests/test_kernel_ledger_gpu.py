"""-m gpu: one test per case of tests/kernel_ledger.py.  Each runs its op entry with the launch log on, checks that the
kernel it stands for was launched, and holds the result to its bar against a float64 (or bit-exact) reference."""
import pytest

import kernel_ledger

pytestmark = pytest.mark.gpu

CASES = kernel_ledger.cases()


@pytest.mark.parametrize("kernel,case", [(k, c) for k, _, c in CASES], ids=[f"{k}-{i}" for k, i, _ in CASES])
def test_kernel_instance(kernel, case):
    out = case.run()
    assert kernel in out.launched, f"{case} launched {sorted(out.launched)}, not {kernel}"
    print(f"{kernel}: {out.what}: err {out.err:.3e} (bar {out.bar:.1e})")
    assert out.err <= out.bar, f"{out.what}: error {out.err:.3e} above {out.bar:.1e}"
