"""-m gpu: one test per case of tests/kernel_ledger_clip.py, run as tests/test_kernel_ledger_nms_gpu.py runs its cases
(launch log on, the case's own kernel the only one launched, exact equality)."""
import pytest

import kernel_ledger_clip

pytestmark = pytest.mark.gpu

CASES = kernel_ledger_clip.cases()


@pytest.mark.parametrize("kernel,case", [(k, c) for k, _, c in CASES], ids=[f"{k}-{i}" for k, i, _ in CASES])
def test_clip_kernel_instance(kernel, case):
    out = case.run()
    assert set(out.launched) == {kernel}, f"{case} launched {sorted(out.launched)}, not {kernel} alone"
    print(f"{kernel}: {out.what}: {out.err:.0f} bytes differ")
    assert out.err <= out.bar, f"{out.what}: {out.err} bytes differ"
