"""No GPU: every entry of include/casync_hip.h that takes a `workspace*` or `scratch*` parameter is classified exactly once in
tests/workspace_contract.py -- an adapter of the fill protocol (ADAPTERS) or an exemption with its reason (EXEMPT) -- and nothing
stale is listed.  A new workspace-taking entry without a classification fails here by name, on any machine."""
import workspace_contract as wc


def _problems(entries, adapters, exempt):
    """one line per entry that is not in exactly one table, and per key that names no entry"""
    out = []
    tables = (("ADAPTERS", adapters), ("EXEMPT", exempt))
    for e in entries:
        where = [name for name, t in tables if e in t]
        if not where:
            out.append(f"{e} takes a workspace and is in neither ADAPTERS nor EXEMPT")
        elif len(where) > 1:
            out.append(f"{e} is classified twice: {where}")
    for name, t in tables:
        out += [f"{name} lists {k}, which include/casync_hip.h does not declare with a workspace or scratch parameter" for k in t if k not in entries]
    return out


def test_the_header_parses_to_the_workspace_taking_entries(tmp_path):
    entries = wc.workspace_entries()
    assert len(entries) == len(set(entries)) >= 19
    for known in ("casync_forward", "casync_forward_windows", "casync_profile_forward", "casync_tap", "casync_hubert_forward_tap",
                  "casync_pfld_forward_u8", "casync_s3fd_forward", "casync_sync_forward_tap", "casync_op_jpeg_encode",
                  "casync_op_jpeg420_encode", "casync_op_jpegdec_decode", "casync_op_mjpegdec_decode", "casync_op_audio_normalize"):
        assert known in entries, known
    for none in ("casync_workspace_bytes", "casync_workspace_bytes_h", "casync_hubert_workspace_bytes", "casync_op_jpeg_workspace_bytes",
                 "casync_op_audio_workspace_bytes", "casync_frame_paste_back", "casync_op_pw_gemm", "casync_op_audio_resample"):
        assert none not in entries, none
    # a declaration over several lines, behind a comment that names a workspace; a *_workspace_bytes query is no workspace taker
    header = tmp_path / "h.h"
    header.write_text("/* casync_old(void* workspace_dev); */\nint casync_op_new(const float* x,\n    uint8_t* scratch, int64_t scratch_bytes);\n"
                      "int64_t casync_new_workspace_bytes(int n);\nint casync_last(float* out, void* workspace);\n")
    assert wc.workspace_entries(str(header)) == ["casync_op_new", "casync_last"]


def test_every_workspace_taking_entry_is_classified_exactly_once():
    problems = _problems(wc.workspace_entries(), wc.ADAPTERS, wc.EXEMPT)
    assert not problems, "\n".join(problems)


def test_a_missing_or_stale_classification_is_named():
    entries = wc.workspace_entries()
    adapters = {k: v for k, v in wc.ADAPTERS.items() if k != "casync_forward_windows"}
    assert _problems(entries, adapters, wc.EXEMPT) == ["casync_forward_windows takes a workspace and is in neither ADAPTERS nor EXEMPT"]
    new = entries + ["casync_op_brand_new"]
    assert any(p.startswith("casync_op_brand_new ") for p in _problems(new, wc.ADAPTERS, wc.EXEMPT))
    twice = dict(wc.EXEMPT, casync_forward="also here, with a reason of some length")
    assert any(p.startswith("casync_forward is classified twice") for p in _problems(entries, wc.ADAPTERS, twice))
    stale = dict(wc.ADAPTERS, casync_op_gone=("audio-normalize",))
    assert any(p.startswith("ADAPTERS lists casync_op_gone") for p in _problems(entries, stale, wc.EXEMPT))
    stale = dict(wc.EXEMPT, casync_op_gone_too="it was a one-line forwarder to another entry")
    assert any(p.startswith("EXEMPT lists casync_op_gone_too") for p in _problems(entries, wc.ADAPTERS, stale))


def test_the_tables_point_at_things_that_exist():
    made = wc.adapters()
    for entry, names in wc.ADAPTERS.items():
        assert names and all(n in made for n in names), (entry, names)
    for name, factory in made.items():
        a = factory()
        assert a.name == name and a.entries, name
        assert a.variants and set(a.variants) <= set(wc.VARIANTS), name
        assert tuple(a.variants) == wc.VARIANTS or len(a.reason) > 20, f"{name} leaves variants out without a reason"
        if any(e.startswith("casync_op_jpeg") or e.startswith("casync_op_mjpeg") for e in a.entries):      # integer-bearing scratch
            assert "before any thread reads it" in type(a).__doc__, f"{name}: its docstring does not settle the integers of its scratch"
    assert wc.unet_9_then_4().name in made and wc.unet_9_then_4().variants == ("stale",)
    assert [n for n, _ in wc.cases()] == [n for n, f in made.items() for _ in f().variants]
    for entry, reason in wc.EXEMPT.items():
        assert len(reason) > 20, entry
    assert len(wc.EXEMPT) <= 2          # short: a workspace-taking entry belongs under the protocol
