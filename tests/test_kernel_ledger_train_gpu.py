"""-m gpu: one test per case of tests/kernel_ledger_train.py, run as tests/test_kernel_ledger_audio_gpu.py runs its cases (launch
log on; the kernel launched is exactly the instance the case is listed under); the error is the number of floats that differ from
the restatement and the bar is 0."""
import pytest

import kernel_ledger_train

pytestmark = pytest.mark.gpu

CASES = kernel_ledger_train.cases()


@pytest.mark.parametrize("kernel,case", [(k, c) for k, _, c in CASES], ids=[f"{k}-{i}" for k, i, _ in CASES])
def test_train_kernel_instance(kernel, case):
    out = case.run()
    want = kernel_ledger_train.launched_by(case)
    assert kernel in want and set(out.launched) == want, f"{case} launched {sorted(out.launched)}, not {sorted(want)}"
    print(f"{kernel}: {out.what}: {out.err:.0f} floats differ")
    assert out.err <= out.bar, f"{out.what}: {out.err} floats differ from the restatement"
