"""-m gpu: one test per case of tests/kernel_ledger_audio.py, run as tests/test_kernel_ledger_clip_gpu.py runs its cases (launch
log on; the kernels launched are exactly those the case is listed under: one for the front-end entry, three for the normalise
entry); the error is a fraction of the case's derived bar."""
import pytest

import kernel_ledger_audio

pytestmark = pytest.mark.gpu

CASES = kernel_ledger_audio.cases()


@pytest.mark.parametrize("kernel,case", [(k, c) for k, _, c in CASES], ids=[f"{k}-{i}" for k, i, _ in CASES])
def test_audio_kernel_instance(kernel, case):
    out = case.run()
    want = kernel_ledger_audio.launched_by(case)
    assert kernel in want and set(out.launched) == want, f"{case} launched {sorted(out.launched)}, not {sorted(want)}"
    print(f"{kernel}: {out.what}: {out.err:.3f} of the bar")
    assert out.err <= out.bar, f"{out.what}: {out.err} of the bar"
