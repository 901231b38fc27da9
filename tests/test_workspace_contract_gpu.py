"""-m gpu: the workspace contract (tests/workspace_contract.py).  One test per adapter and variant: the run on a workspace of 0xFF
bytes, of 0x7F bytes, on one a call of the same entry has just used (stale) and on one another handle has just used (foreign)
equals the run on a zeroed workspace bit for bit, output by output and tap by tap.  The 9-then-4 case of the fp32 U-Net is the
adapter `unet-fp32-hubert-b4-after-b9`, stale only."""
import pytest

import workspace_contract as wc

pytestmark = pytest.mark.gpu

ADAPTERS = wc.adapters()


@pytest.mark.parametrize("name,variant", wc.cases())
def test_no_byte_of_the_workspace_on_entry_reaches_an_output(name, variant):
    try:
        wc.check(ADAPTERS[name], variant)
    except RuntimeError as exc:
        if "HIP error" in str(exc) or "hipError" in str(exc) or "illegal memory access" in str(exc):
            pytest.exit(f"{name} [{variant}]: the device reported {exc}: nothing more is started on it in this session", returncode=3)
        raise
