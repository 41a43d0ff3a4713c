"""CPU-side checks of the TSV response rows: the new symbols are declared and exported, the header line, and
kaamer_format_tsv_arrays (the host formatter: what kaamer_format_tsv runs on a result of the library) against the
restatement of search.go:505-554 in tsvref.py, byte for byte, on hand-built results.  No device calls here."""
import ctypes as C
import os
import re

import pytest

import tsvcases
import tsvref
from kaamer_amd import abi, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_ONLY = bool(os.environ.get("KAAMER_HOST_ONLY"))   # the sanitized CPU build holds the host sources only

NEW_SYMBOLS = ["kaamer_format_tsv_header", "kaamer_format_tsv", "kaamer_format_tsv_arrays", "kaamer_index_attach_subject_text",
               "kaamer_index_subject_text_info", "kaamer_tsv_stage_create", "kaamer_tsv_stage_free", "kaamer_tsv_rows_device",
               "kaamer_tsv_rows_finish", "kaamer_tsv_geometry", "kaamer_submit_text_top_tsv_flat", "kaamer_search_text_top_tsv_flat",
               "kaamer_submit_fasta_top_tsv_flat", "kaamer_search_fasta_top_tsv_flat", "kaamer_submit_bgzf_top_tsv_flat",
               "kaamer_search_bgzf_top_tsv_flat", "kaamer_batch_top_tsv", "kaamer_index_set_tsv_bounds"]
HOST_SYMBOLS = ["kaamer_format_tsv_header", "kaamer_format_tsv_arrays"]


def test_new_symbols_declared_and_abi_version_unchanged():
    src = open(os.path.join(ROOT, "include", "kaamer_hip.h")).read()
    assert re.search(r"#define\s+KAAMER_ABI_VERSION\s+4\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kaamer_[a-z_0-9]+)\s*\(", code))
    for n in NEW_SYMBOLS:
        assert n in declared, "include/kaamer_hip.h does not declare %s" % n
        assert n in abi.SYMBOLS, "abi.py does not bind %s" % n


def test_new_symbols_exported(klib):
    for n in (HOST_SYMBOLS if HOST_ONLY else NEW_SYMBOLS):
        assert hasattr(klib, n), "the library lacks %s" % n


@pytest.fixture(scope="module")
def table(klib):
    return tsvcases.standard_table()


@pytest.fixture(scope="module")
def entries(table):
    return tsvref.entries_of(table)


@pytest.mark.parametrize("positions", [False, True])
@pytest.mark.parametrize("annotations", [False, True])
def test_header(klib, table, positions, annotations):
    want = tsvref.header_ref(positions, annotations, table.feature_names)
    assert api.format_tsv_header(positions, annotations, table) == want
    if not annotations:
        assert api.format_tsv_header(positions, annotations, None) == want
    # the short-buffer convention of kaamer_format_positions
    for cap in (1, 5, len(want), len(want) + 1):
        raw = (C.c_char * (cap + 8))()
        C.memset(raw, 0x55, cap + 8)
        need = klib.kaamer_format_tsv_header(int(positions), int(annotations), table._h, C.cast(raw, C.c_char_p), cap)
        got = bytes(raw)
        assert need == len(want) and got[cap:] == b"\x55" * 8
        n = min(len(want), cap - 1)
        assert got[:n] == want[:n] and got[n] == 0


def check(table, entries, names, queries, positions, annotations):
    buf, spans = tsvcases.names_buffer(names)
    want, want_off = tsvref.rows_ref(tsvcases.ref_queries(names, queries), entries, table.feature_names, positions, annotations)
    got, got_off = api.format_tsv(tsvcases.host_top(queries), buf, spans, table, positions, annotations)
    assert got == want
    assert got_off.tolist() == want_off.tolist()
    return got


def test_float_vectors_and_sweep(klib, table, entries):
    for (k, n), text in tsvcases.FLOAT_VECTORS:
        assert tsvref.identity_ref(k, n) == text
        got = check(table, entries, [b"v"], [tsvcases.query(0, n, [(0, k)])], False, False)
        assert got.split(b"\t")[2] == text.encode()
    # what goes wrong quietly: half-up, or the arithmetic in double
    assert "%.2f" % (23 / 160 * 100) == "14.37" and "%.2f" % (47 / 160 * 100) == "29.38"
    names, queries = tsvcases.float_sweep()
    got = check(table, entries, names, queries, False, False)
    assert got.count(b"\n") == len(queries)


@pytest.mark.parametrize("positions", [False, True])
@pytest.mark.parametrize("annotations", [False, True])
def test_rows_on_hand_built_results(klib, table, entries, positions, annotations):
    for name, (names, queries) in tsvcases.standard_cases().items():
        check(table, entries, names, queries, positions, annotations)


def test_specific_rows(klib, table, entries):
    """a few rows spelled out, so that the restatement itself is pinned"""
    names = [b"read/1 first", b"tab\tname here", b" x", b""]
    bits = [True] * 5 + [False] * 3 + [True] * 2
    qs = [tsvcases.query(0, 8, [(12, 1, bits)], start=4, end=33, pos_len=10), tsvcases.query(1, 32, [(2, 1), (tsvcases.MISSING, 1), (3, 1)]),
          tsvcases.query(2, 7, [(11, 7)]), tsvcases.query(3, 2147483647, [(0, 2147483647)], start=0, end=2147483647, pos_len=0)]
    e12, e2 = entries[12], entries[2]
    got = check(table, entries, names, qs, True, True)
    rows = got.split(b"\n")
    f = [b"Organism", b"EC", b"Note"]
    assert rows[0] == b"\t".join([b"read/1", e12["EntryId"], b"12.50", b"8", b"1", b"1", b"4", b"33", b"1", b"20", b"1-6,9-10"] +
                                 [e12["Features"][k] for k in f])
    assert len(e12["Features"][b"Organism"]) == 1000 and e12["Features"][b"EC"] == b""
    assert rows[1] == b"\t".join([b"tab\tname", e2["EntryId"], b"3.12", b"32", b"1", b"0", b"1", b"38", b"1", b"10", b""] +
                                 [e2["Features"][k] for k in f])
    # the missing id second of three: from there on no entry, the third hit's entry included
    assert rows[2] == b"tab\tname\t\t3.12\t32\t1\t0\t1\t38\t1\t0\t\t\t\t"
    assert rows[3] == rows[2]
    assert rows[4] == b"\t".join([b"", entries[11]["EntryId"], b"100.00", b"7", b"7", b"0", b"1", b"13", b"1", b"7", b"", b"", b"", b""])
    assert rows[5].startswith(b"\t0\t100.00\t2147483647\t2147483647\t0\t0\t2147483647\t1\t7\t\t")
    got = check(table, entries, names, qs, False, False)
    assert got.split(b"\n")[0] == b"read/1\t" + e12["EntryId"] + b"\t12.50\t8\t1\tN/A\t4\t33\t1\tN/A"


def test_zero_features_with_annotations(klib):
    t = api.Proteins.from_tsv(b"EntryID\tSequence\nA1\tMKTAYIAKQR\nB2\tACDEFGHIKLMN\n")
    assert t.feature_names == []
    ent = tsvref.entries_of(t)
    got = check(t, ent, [b"q 1"], [tsvcases.query(0, 10, [(1, 4), (0, 2), (5, 1)])], False, True)
    assert got == b"q\tB2\t40.00\t10\t4\tN/A\t1\t16\t1\t12\nq\tA1\t20.00\t10\t2\tN/A\t1\t16\t1\t10\nq\t\t10.00\t10\t1\tN/A\t1\t16\t1\t0\n"
    assert api.format_tsv_header(False, True, t) == tsvref.HEADER.encode() + b"\n"
    # no table at all: every entry prints as missing
    buf, spans = tsvcases.names_buffer([b"q 1"])
    got, _ = api.format_tsv(tsvcases.host_top([tsvcases.query(0, 10, [(1, 4)])]), buf, spans, None, False, True)
    assert got == b"q\t\t40.00\t10\t4\tN/A\t1\t16\t1\t0\n"


def test_short_buffer_and_arguments(klib, table, entries):
    names, queries = tsvcases.standard_cases()["entries"]
    buf, spans = tsvcases.names_buffer(names)
    top = tsvcases.host_top(queries)
    want, _ = tsvref.rows_ref(tsvcases.ref_queries(names, queries), entries, table.feature_names, True, True)
    for cap in (0, 1, 2, 100, len(want) - 1, len(want), len(want) + 1):
        got, need = api.format_tsv(top, buf, spans, table, True, True, cap=cap)
        assert need == len(want)                                   # the length needed, whatever the buffer holds
        assert got == want[:max(min(cap - 1, len(want)), 0)]
    # ExtractPositions on a result without bitmaps
    top.pos_bits = None
    with pytest.raises(abi.KaamerError) as e:
        api.format_tsv(top, buf, spans, table, True, False)
    assert e.value.code == abi.E_ARG
    got, _ = api.format_tsv(top, buf, spans, table, False, False)   # ... which formats without them
    assert got == tsvref.rows_ref(tsvcases.ref_queries(names, queries), entries, table.feature_names, False, False)[0]
    # a record index beyond the names, a span beyond the buffer: an empty name, nothing read
    q = [tsvcases.query(7, 10, [(0, 5)]), tsvcases.query(0, 10, [(0, 5)])]
    spans2 = spans.copy()
    spans2[0]["name_off"], spans2[0]["name_len"] = len(buf) - 1, 2
    got, _ = api.format_tsv(tsvcases.host_top(q), buf, spans2, table, False, False)
    assert [r.split(b"\t")[0] for r in got.split(b"\n")[:2]] == [b"", b""]
