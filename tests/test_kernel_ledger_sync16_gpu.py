"""-m gpu: one test per case of tests/kernel_ledger_sync16.py, run as tests/test_kernel_ledger_sync_gpu.py runs its cases
(launch log on, the case's own kernel the only one launched, error within the bar)."""
import pytest

import kernel_ledger_sync16

pytestmark = pytest.mark.gpu

CASES = kernel_ledger_sync16.cases()


@pytest.mark.parametrize("kernel,case", [(k, c) for k, _, c in CASES], ids=[f"{k}-{i}" for k, i, _ in CASES])
def test_sync16_kernel_instance(kernel, case):
    out = case.run()
    assert set(out.launched) == {kernel}, f"{case} launched {sorted(out.launched)}, not {kernel} alone"
    print(f"{kernel}: {out.what}: err {out.err:.3e} (bar {out.bar:.1e})")
    assert out.err <= out.bar, f"{out.what}: error {out.err:.3e} above {out.bar:.1e}"
