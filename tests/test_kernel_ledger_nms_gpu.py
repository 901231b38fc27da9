"""-m gpu: one test per case of tests/kernel_ledger_nms.py, run as tests/test_kernel_ledger_face_gpu.py runs its cases
(launch log on, the case's own kernel the only one launched, exact equality)."""
import pytest

import kernel_ledger_nms

pytestmark = pytest.mark.gpu

CASES = kernel_ledger_nms.cases()


@pytest.mark.parametrize("kernel,case", [(k, c) for k, _, c in CASES], ids=[f"{k}-{i}" for k, i, _ in CASES])
def test_nms_kernel_instance(kernel, case):
    out = case.run()
    assert set(out.launched) == {kernel}, f"{case} launched {sorted(out.launched)}, not {kernel} alone"
    print(f"{kernel}: {out.what}: {out.err:.0f} elements differ")
    assert out.err <= out.bar, f"{out.what}: {out.err} elements differ"
