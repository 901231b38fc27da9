"""Every compiled kernel instance has an op-level case in tests/kernel_ledger.py (no GPU): a new instance without one,
or a ledger entry whose kernel is gone, fails here on any machine, naming the kernel."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

import kernel_ledger  # noqa: E402
from calipsync_amd import build  # noqa: E402

pytestmark = pytest.mark.skipif(not kernel_resources.tools_available(), reason="llvm binutils of the ROCm image not found")


@pytest.fixture(scope="module")
def table():
    build.build()                      # no-op when the library is up to date
    if not os.path.isdir(kernel_resources.OBJ_DIR) or not any(f.endswith(".o") for f in os.listdir(kernel_resources.OBJ_DIR)):
        build.build(force=True)        # a library shipped without its objects: compile them
    return kernel_resources.table()


def test_every_kernel_instance_has_a_ledger_case(table):
    missing = sorted(set(table) - set(kernel_ledger.LEDGER))
    stale = sorted(set(kernel_ledger.LEDGER) - set(table))
    assert not missing, f"kernel instances without a case in tests/kernel_ledger.py: {missing}"
    assert not stale, f"ledger entries for kernels the library no longer has: {stale}"


def test_every_ledger_entry_has_a_case():
    empty = [k for k, cs in kernel_ledger.LEDGER.items() if not cs or not all(isinstance(c, kernel_ledger.Case) for c in cs)]
    assert not empty, empty
