"""-m gpu: one test per case of tests/kernel_ledger_jpeg420.py, run as tests/test_kernel_ledger_jpeg_gpu.py runs its cases (launch
log on, the kernels that list the case the only ones launched, exact equality)."""
import pytest

import kernel_ledger_jpeg420

pytestmark = pytest.mark.gpu

CASES = kernel_ledger_jpeg420.cases()


@pytest.mark.parametrize("kernels,case", [(k, c) for k, _, c in CASES], ids=[f"jpeg420-{i}" for _, i, _ in CASES])
def test_jpeg420_kernel_instances(kernels, case):
    out = case.run()
    assert sorted(out.launched) == kernels, f"{case} launched {sorted(out.launched)}, not {kernels}"
    print(f"{case}: {out.what}: {out.err:.0f} bytes differ")
    assert out.err <= out.bar, f"{out.what}: {out.err} bytes differ"
