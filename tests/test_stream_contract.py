"""No GPU: every entry of include/casync_hip.h that takes a casync_stream is classified exactly once in
tests/stream_contract.py -- an adapter of the busy-stream protocol (ADAPTERS), a ledger case run under a busy side stream
(LEDGER_CASES) or an exemption with its reason (EXEMPT) -- and nothing stale is listed.  A new stream-taking entry without a
classification fails here by name, on any machine."""
import stream_contract as sc


def _problems(entries, adapters, ledger, exempt):
    """one line per entry that is not in exactly one table, and per key that names no entry"""
    out = []
    tables = (("ADAPTERS", adapters), ("LEDGER_CASES", ledger), ("EXEMPT", exempt))
    for e in entries:
        where = [name for name, t in tables if e in t]
        if not where:
            out.append(f"{e} takes a casync_stream and is in none of ADAPTERS, LEDGER_CASES, EXEMPT")
        elif len(where) > 1:
            out.append(f"{e} is classified twice: {where}")
    for name, t in tables:
        out += [f"{name} lists {k}, which include/casync_hip.h does not declare with a casync_stream" for k in t if k not in entries]
    return out


def test_the_header_parses_to_the_stream_taking_entries(tmp_path):
    entries = sc.stream_entries()
    assert len(entries) == len(set(entries)) >= 90
    for known in ("casync_forward", "casync_tap", "casync_op_pw_gemm", "casync_op_pfld_head", "casync_frame_paste_back",
                  "casync_op_mjpegdec_decode", "casync_op_audio_normalize"):
        assert known in entries, known
    for no_stream in ("casync_abi_version", "casync_create", "casync_load_weights_host", "casync_conv3x3_plan", "casync_op_set_dtype"):
        assert no_stream not in entries, no_stream
    # a declaration over several lines, behind a comment that names a stream
    header = tmp_path / "h.h"
    header.write_text("/* casync_old(int, casync_stream s); */\nint casync_op_new(const float* x,\n    int n, casync_stream stream);\n"
                      "int casync_plain(int n);\n")
    assert sc.stream_entries(str(header)) == ["casync_op_new"]


def test_every_stream_taking_entry_is_classified_exactly_once():
    problems = _problems(sc.stream_entries(), sc.ADAPTERS, sc.LEDGER_CASES, sc.EXEMPT)
    assert not problems, "\n".join(problems)


def test_a_missing_or_stale_classification_is_named():
    entries = sc.stream_entries()
    adapters = {k: v for k, v in sc.ADAPTERS.items() if k != "casync_forward_windows"}
    assert _problems(entries, adapters, sc.LEDGER_CASES, sc.EXEMPT) == [
        "casync_forward_windows takes a casync_stream and is in none of ADAPTERS, LEDGER_CASES, EXEMPT"]
    new = entries + ["casync_op_brand_new"]
    assert any(p.startswith("casync_op_brand_new ") for p in _problems(new, sc.ADAPTERS, sc.LEDGER_CASES, sc.EXEMPT))
    twice = dict(sc.EXEMPT, casync_forward="also here")
    assert any(p.startswith("casync_forward is classified twice") for p in _problems(entries, sc.ADAPTERS, sc.LEDGER_CASES, twice))
    stale = dict(sc.LEDGER_CASES, casync_op_gone=next(iter(sc.LEDGER_CASES.values())))
    assert any(p.startswith("LEDGER_CASES lists casync_op_gone") for p in _problems(entries, sc.ADAPTERS, stale, sc.EXEMPT))


def test_the_tables_point_at_things_that_exist():
    made = sc.adapters()
    for entry, names in sc.ADAPTERS.items():
        assert names and all(n in made for n in names), (entry, names)
    for name, factory in made.items():
        a = factory()
        assert a.name == name
        assert a.nosync or a.reason, f"{name} is exempt from `pending` without a reason"
    assert all(a.name in made for a in sc.pair())
    for entry, (module, case) in sc.LEDGER_CASES.items():
        assert case in sc.ledger_known(module), f"{entry}: {case} is not a case of tests/{module}.py"
    for entry, reason in sc.EXEMPT.items():
        assert len(reason) > 20, entry
    assert len(sc.EXEMPT) <= 3          # short: an entry belongs under the protocol or the ledger leg
