"""-m gpu: one test per case of tests/kernel_ledger_ploss.py, run as tests/test_kernel_ledger_train_gpu.py runs its cases (launch
log on; the kernel launched is exactly the one the case is listed under).  Bit-exact cases report the floats that differ (bar 0),
the two stem directions the larger of their max and mean error ratios against fp32 torch over 4 (bar 1), the two sums their
relative error against a float64 sum (bar 1e-13)."""
import pytest

import kernel_ledger_ploss

pytestmark = pytest.mark.gpu

CASES = kernel_ledger_ploss.cases()


@pytest.mark.parametrize("kernel,case", [(k, c) for k, _, c in CASES], ids=[f"{k}-{i}" for k, i, _ in CASES])
def test_ploss_kernel(kernel, case):
    out = case.run()
    want = kernel_ledger_ploss.launched_by(case)
    assert kernel in want and set(out.launched) == want, f"{case} launched {sorted(out.launched)}, not {sorted(want)}"
    print(f"{kernel}: {out.what}: err {out.err:.3e} (bar {out.bar:.1e})")
    assert out.err <= out.bar, f"{out.what}: error {out.err:.3e} above {out.bar:.1e}"
