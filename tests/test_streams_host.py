"""The stream cases of tests/test_gpu_streams.py cover the whole C ABI: its table names exactly the exports of include/neddf_hip.h
that take a stream, minus a short list spelled out with reasons.  A new stream-taking entry point cannot arrive without a case."""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HEADER = os.path.join(ROOT, "include", "neddf_hip.h")


def stream_exports(text):
    """The functions a header text declares with a `void *stream` parameter (the last one everywhere but in the two culled render
    calls, whose occupancy grid follows it), comments stripped as test_capi_exports_every_declared_symbol strips them."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = re.findall(r"\b(?:int|int64_t|void|const\s+char\s*\*)\s*(neddf_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text)
    return {name for name, args in decls if re.search(r"\bvoid\s*\*\s*stream\b", args)}, {name for name, _ in decls}


def table_mismatch(text, table, excluded):
    """(stream-taking exports without a row or an exclusion, rows and exclusions that name no stream-taking export)."""
    have, _ = stream_exports(text)
    named = set(table) | set(excluded)
    return sorted(have - named), sorted(named - have)


def test_the_table_is_the_header():
    import test_gpu_streams as cases
    text = open(HEADER).read()
    have, declared = stream_exports(text)
    from neddf_amd import _lib
    assert declared == {name for name, _, _ in _lib.SYMBOLS}, "the declaration pattern misses part of the header"
    assert len(have) > 60
    uncovered, stale = table_mismatch(text, cases.TABLE, cases.EXCLUDED)
    assert not uncovered, "stream-taking exports without a stream case (tests/test_gpu_streams.py TABLE): %s" % uncovered
    assert not stale, "TABLE / EXCLUDED rows that name no stream-taking export: %s" % stale
    assert not set(cases.TABLE) & set(cases.EXCLUDED)
    # the exclusions: the communicator calls and nothing else, each with its reason
    assert set(cases.EXCLUDED) == {"neddf_gather_pixels", "neddf_gather_pixels_granular", "neddf_comm_wait"}
    assert all(isinstance(r, str) and len(r) > 20 for r in cases.EXCLUDED.values())


def test_every_row_names_a_test_of_the_module():
    import test_gpu_streams as cases
    for name, (test, synchronising) in cases.TABLE.items():
        assert callable(getattr(cases, test, None)) and test.startswith("test_"), "%s: no test %s" % (name, test)
        assert synchronising in (True, False)
    assert callable(cases.test_every_table_row_was_called)


def test_a_missing_row_or_a_new_declaration_is_noticed():
    import test_gpu_streams as cases
    text = open(HEADER).read()
    short = {k: v for k, v in cases.TABLE.items() if k != "neddf_bvh_build"}
    assert table_mismatch(text, short, cases.EXCLUDED) == (["neddf_bvh_build"], [])
    grown = text.replace("int neddf_set_timing(", "int neddf_new_stage(neddf_ctx *ctx, const float *d_x,\n        int64_t n, void *stream);\nint neddf_set_timing(")
    assert grown != text
    assert table_mismatch(grown, cases.TABLE, cases.EXCLUDED) == (["neddf_new_stage"], [])
    # a declaration without a stream parameter asks for no row
    plain = text.replace("int neddf_set_timing(", "int neddf_new_getter(neddf_ctx *ctx, int *out);\nint neddf_set_timing(")
    assert table_mismatch(plain, cases.TABLE, cases.EXCLUDED) == ([], [])


def test_the_delay_rule():
    """50 x the call, 10 x call plus synchronise for a synchronising entry, never below 20 ms, never above 200 ms."""
    import pytest
    from stream_check import delay_rule
    assert delay_rule(0.01, 0.05, False) == 20.0
    assert delay_rule(1.0, 30.0, False) == 50.0
    assert delay_rule(0.1, 9.0, True) == 90.0
    assert delay_rule(0.1, 9.0, False) == 20.0
    with pytest.raises(AssertionError):
        delay_rule(5.0, 5.0, False)
    with pytest.raises(AssertionError):
        delay_rule(0.1, 21.0, True)
