"""-m gpu: one test per case of tests/kernel_ledger_hb16.py, run as tests/test_kernel_ledger_gpu.py runs its cases (launch
log on, the case's own kernel among the launched ones, error within the bar), and the bf16 rows GEMM at every shape the
bf16 HuBERT forward launches, which must launch the existing bf16 ring instance named for it and nothing else."""
import pytest

import kernel_ledger
import kernel_ledger_hb16

pytestmark = pytest.mark.gpu

CASES = kernel_ledger_hb16.cases()
GEMMS = kernel_ledger_hb16.rows_gemm_cases()


@pytest.mark.parametrize("kernel,case", [(k, c) for k, _, c in CASES], ids=[f"{k}-{i}" for k, i, _ in CASES])
def test_hb16_kernel_instance(kernel, case):
    out = case.run()
    assert kernel in out.launched, f"{case} launched {sorted(out.launched)}, not {kernel}"
    print(f"{kernel}: {out.what}: err {out.err:.3e} (bar {out.bar:.1e})")
    assert out.err <= out.bar, f"{out.what}: error {out.err:.3e} above {out.bar:.1e}"


@pytest.mark.parametrize("kernel,case", GEMMS, ids=[f"{c.params[0]}x{c.params[1]}x{c.params[2]}" for _, c in GEMMS])
def test_rows_gemm_bf16_launches_an_existing_instance(kernel, case):
    out = case.run()
    assert set(out.launched) == {kernel}, f"{case} launched {sorted(out.launched)}, expected {kernel}"
    assert kernel in kernel_ledger.LEDGER
    print(f"{kernel}: {out.what}: err {out.err:.3e} (bar {out.bar:.1e})")
    assert out.err < out.bar, f"{out.what}: error {out.err:.3e} not below {out.bar:.1e}"
