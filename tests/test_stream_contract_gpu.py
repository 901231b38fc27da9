"""-m gpu: the stream contract (tests/stream_contract.py).  The positive control, one test per adapter of the busy-stream
protocol, the two-handle pair on two side streams (the forward gate), and one test per single-launch entry under a busy side
stream."""
import pytest

import stream_contract as sc

pytestmark = pytest.mark.gpu

ADAPTERS = sc.adapters()


def test_work_on_the_null_stream_overtakes_a_busy_side_stream():
    """the positive control everything below relies on: a stream on which it holds exists (of up to 8 pooled ones)"""
    side = sc.independent_stream()
    assert side.cuda_stream != 0
    assert sc._runs_ahead(side)                     # and it holds again on the stream the tests will use


@pytest.mark.parametrize("name", list(ADAPTERS))
def test_call_behind_a_busy_stream_equals_the_null_stream_run(name):
    sc.run_behind(ADAPTERS[name]())


def test_two_handles_on_two_side_streams_pass_the_forward_gate():
    """a HuBERT and a U-Net forward, each behind its own busy stream: the second waits (on the device) for the first handle's
    stream, neither waits on the host, both return their own null-stream results"""
    sc.run_behind(sc.pair(), sc.independent_streams(2))


@pytest.mark.parametrize("entry", list(sc.LEDGER_CASES))
def test_single_launch_entry_under_a_busy_side_stream(entry):
    module, case = sc.LEDGER_CASES[entry]
    sc.run_ledger_behind(module, case)
