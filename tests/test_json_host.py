"""The JSON response on the host (json_format.cpp): kaamer_json_escape, kaamer_format_json_header / _trailer,
kaamer_format_json_arrays and kaamer_json_protein_value against tests/jsonref.py, an independent restatement of
encoding/json's rules, byte for byte -- and, independent of jsonref, against Python's json module on what it decodes.
No GPU."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import jsoncases
import jsonref
from kaamer_amd import abi, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SYMBOLS = ["kaamer_format_json_header", "kaamer_format_json_trailer", "kaamer_format_json", "kaamer_format_json_arrays", "kaamer_json_escape",
                "kaamer_json_protein_value"]
DEVICE_SYMBOLS = ["kaamer_index_attach_subject_json", "kaamer_index_subject_json_info", "kaamer_json_stage_create", "kaamer_json_stage_free",
                  "kaamer_json_rows_device", "kaamer_json_rows_finish", "kaamer_json_geometry", "kaamer_batch_top_json", "kaamer_index_set_json_bounds"] + \
                 ["kaamer_%s_%s_top_json_flat" % (a, b) for a in ("submit", "search") for b in ("text", "fasta", "bgzf")]


def test_new_symbols_declared_bound_and_exported(klib):
    src = open(os.path.join(ROOT, "include", "kaamer_hip.h")).read()
    assert re.search(r"#define\s+KAAMER_ABI_VERSION\s+4\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kaamer_[a-z_0-9]+)\s*\(", code))
    for n in HOST_SYMBOLS + DEVICE_SYMBOLS:
        assert n in declared, "include/kaamer_hip.h does not declare %s" % n
        assert n in abi.SYMBOLS, "abi.py does not bind %s" % n
        assert hasattr(klib, n), "the library lacks %s" % n
    assert klib.kaamer_abi_version() == 4
    assert "Out of scope: JSON" not in src


# ---------------------------------------------------------------- strings
def _same_escape(data):
    got, want = api.json_escape(data), jsonref.escape(data)
    assert got == want, "%r: %r, expected %r" % (data, got, want)


def test_escape_every_byte_and_every_pair(klib):
    for b in range(256):
        _same_escape(bytes([b]))
    for lead in range(0xC0, 0x100):
        for second in range(256):
            _same_escape(bytes([lead, second]))


CRAFTED = [b"\xc3\xa9", b"\xe2\x82\xac", b"\xf0\x9f\x98\x80", b"\xf4\x8f\xbf\xbf", jsoncases.U2028, jsoncases.U2029, b"a" + jsoncases.U2028 + b"b",
           b"\xe2\x80\xa7", b"\xe2\x80\xaa", b"\xef\xbf\xbd", b"\xc0\x80", b"\xc1\xbf", b"\xe0\x80\x80", b"\xe0\x9f\xbf", b"\xe0\xa0\x80", b"\xed\xa0\x80",
           b"\xed\x9f\xbf", b"\xed\xbf\xbf", b"\xf0\x8f\xbf\xbf", b"\xf0\x90\x80\x80", b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\xf8\x88\x80\x80\x80",
           b"\xfc\x84\x80\x80\x80\x80", b"\xfe", b"\xff", b"\x80", b"\xbf\xbf", b"\xe2", b"\xe2\x82", b"\xe2z", b"\xe2\x82z", b"\xf0\x9f", b"\xf0\x9f\x98",
           b"\xf0\x9f\x98z", b"\xe2\x82\xe2\x82\xac", b"\xc3\xc3\xa9", b"\xf0\xe2\x82\xac", jsoncases.ESCAPES, jsoncases.ESCAPES * 9, b"", b"plain ascii"]


def test_escape_crafted_sequences(klib):
    for s in CRAFTED:
        _same_escape(s)
        _same_escape(b"x" + s + b"y")
    # ... and what the rules say in so many words
    bs = jsoncases.BS
    assert api.json_escape(b'"' + bs + b"\n\r\t") == bs + b'"' + bs + bs + bs + b"n" + bs + b"r" + bs + b"t"
    assert api.json_escape(b"\x08\x0c\x00\x1f") == bs + b"u0008" + bs + b"u000c" + bs + b"u0000" + bs + b"u001f"
    assert api.json_escape(b"<>&\x7f") == bs + b"u003c" + bs + b"u003e" + bs + b"u0026\x7f"
    assert api.json_escape(b"\xc0\x80") == (bs + b"ufffd") * 2
    assert api.json_escape(b"\xe2\x82") == (bs + b"ufffd") * 2
    assert api.json_escape(jsoncases.U2028 + jsoncases.U2029) == bs + b"u2028" + bs + b"u2029"
    assert api.json_escape("é€".encode()) == "é€".encode()


def test_escape_agrees_with_json_module_on_valid_text(klib):
    rng = np.random.RandomState(5)
    for _ in range(300):
        text = "".join(chr(int(c)) for c in rng.choice([0x22, 0x5C, 9, 10, 13, 1, 0x41, 0x7F, 0xE9, 0x20AC, 0x2028, 0x1F600, 0x3C, 0x26], size=rng.randint(0, 12)))
        assert json.loads(b'"' + api.json_escape(text.encode("utf-8")) + b'"') == text


def test_escape_short_buffers(klib):
    data = jsoncases.ESCAPES
    want = jsonref.escape(data)
    for cap in (1, 2, 7, len(want), len(want) + 1):
        buf = abi.C.create_string_buffer(cap)
        assert klib.kaamer_json_escape(data, len(data), buf, cap) == len(want)
        n = min(cap - 1, len(want))
        assert buf.raw[:n] == want[:n] and buf.raw[n] == 0


# ---------------------------------------------------------------- header, trailer, entries
@pytest.fixture(scope="module")
def tables(klib):
    return {name: jsoncases.table(name) for name in jsoncases.TABLES}


def test_header_and_trailer(klib, tables):
    for name, (table, _, features) in tables.items():
        assert table.feature_names == features
        for ann in (False, True):
            assert api.format_json_header(ann, table) == jsonref.header(features, ann)
    assert api.format_json_header(True, None) == b'{"dbProteinFeatures":[],"results":['
    assert api.format_json_header(True, tables["std"][0]) == b'{"dbProteinFeatures":["Organism","EC","Note&more"],"results":['
    assert api.format_json_trailer() == jsonref.trailer() == b"]}"


def test_tables_hold_what_the_cases_say(klib, tables):
    """the two statements of every table agree (so jsonref's entries are the library's)"""
    for name, (table, entries, features) in tables.items():
        ids = sorted(entries)
        for i, got in zip(ids, table.fetch_hits(ids)):
            e = entries[i]
            assert got is not None, (name, i)
            assert (got["EntryId"], got["Sequence"], got["Length"]) == (e["entry_id"], e["sequence"], e["length"]), (name, i)
            assert [got["Features"][k] for k in features] == [v for _, v in e["features"]], (name, i)
        assert table.fetch_hits([jsoncases.MISSING]) == [None]


PROTEIN_VALUES = [dict(entry_id=b"", sequence=b"", length=0, features=[]),
                  dict(entry_id=b"", sequence=b"ACD", length=0, features=[]),
                  dict(entry_id=b"X", sequence=b"", length=0, features=[(b"b", b""), (b"a", b"1")]),
                  dict(entry_id=b"", sequence=b"", length=7, features=[]),
                  dict(entry_id=b"", sequence=b"", length=0, features=[(b"only", b"")]),
                  dict(entry_id=jsoncases.ESCAPES, sequence=jsoncases.ESCAPES, length=2147483647,
                       features=[(b"Zeta", b"z"), (b"alpha", jsoncases.ESCAPES), (b"Alpha", b""), (b"al", b"x"), (b"a<b", b"&"), (b"\xc3\xa9", b"e")])]


def test_protein_values_with_every_omitempty_combination(klib):
    for e in PROTEIN_VALUES:
        assert api.json_protein_value(**e) == jsonref.protein(e), e
    assert api.json_protein_value() == b"{}"
    assert api.json_protein_value(b"X", b"", 0, [(b"b", b""), (b"a", b"1")]) == b'{"EntryId":"X","Features":{"a":"1","b":""}}'


# ---------------------------------------------------------------- objects
@pytest.fixture(scope="module")
def cases(klib):
    return jsoncases.standard_cases()


def _seq_type(c):
    return abi.PROTEIN if c["protein"] else (abi.READS if c["fmt"] == 1 else abi.NUCLEOTIDE)


def _format(c, tables, **kw):
    names, spans = jsoncases.names_buffer(c["names"])
    seqs, offsets = jsoncases.packed(c) if c["protein"] else (None, None)
    return api.format_json(jsoncases.host_top(c), names, spans, tables[c["table"]][0], seqs=seqs, offsets=offsets, seq_type=_seq_type(c),
                           text_format=c["fmt"], positions=c["positions"], **kw)


@pytest.mark.parametrize("name", sorted(jsoncases.standard_cases()))
def test_objects_equal_the_reference(klib, tables, cases, name):
    c = cases[name]
    want, want_off = jsonref.objects(jsoncases.ref_queries(c), tables[c["table"]][1], c["protein"], c["fmt"], c["positions"])
    got, off = _format(c, tables)
    assert got == want
    assert off.tolist() == want_off
    if not any(q["hits"] for q in c["queries"]):
        assert got == b"" and off.tolist() == [0]


def test_many_queries_equal_the_reference(klib, tables):
    for n, seed in ((1, 1), (63, 2), (64, 3), (65, 4), (257, 5)):
        c = jsoncases.many_queries(n, seed)
        want, want_off = jsonref.objects(jsoncases.ref_queries(c), tables["std"][1], False, c["fmt"], False)
        got, off = _format(c, tables)
        assert got == want and off.tolist() == want_off


def test_objects_into_short_buffers(klib, tables, cases):
    c = cases["orfs fasta"]
    want, _ = jsonref.objects(jsoncases.ref_queries(c), tables["std"][1], False, 0, True)
    for cap in (0, 1, 17, len(want), len(want) + 1):
        got, need = _format(c, tables, cap=cap)
        assert need == len(want) and got == want[:max(cap - 1, 0)]


def test_refusals(klib, tables, cases):
    c = cases["orfs fastq"]
    names, spans = jsoncases.names_buffer(c["names"])
    top = jsoncases.host_top(c)
    with pytest.raises(abi.KaamerError) as e:   # nucleotide / reads always print PositionHits
        api.format_json(jsoncases.without_bitmaps(top), names, spans, tables["std"][0], seq_type=abi.READS, text_format=1)
    assert e.value.code == abi.E_ARG and "bitmaps" in str(e.value)
    c = cases["protein"]
    names, spans = jsoncases.names_buffer(c["names"])
    seqs, offsets = jsoncases.packed(c)
    top = jsoncases.without_bitmaps(jsoncases.host_top(c))
    got, _ = api.format_json(top, names, spans, tables["std"][0], seqs=seqs, offsets=offsets)   # no ExtractPositions: none needed
    assert got == jsonref.objects(jsoncases.ref_queries(c), tables["std"][1], True, 0, False)[0]
    with pytest.raises(abi.KaamerError) as e:
        api.format_json(top, names, spans, tables["std"][0], seqs=seqs, offsets=offsets, positions=True)
    assert e.value.code == abi.E_ARG
    top.alignments = [dict(status=1)] * int(top.top_off[-1])   # a result with alignments: -aln JSON is not written
    with pytest.raises(abi.KaamerError) as e:
        api.format_json(top, names, spans, tables["std"][0], seqs=seqs, offsets=offsets)
    assert e.value.code == abi.E_ARG and "alignments" in str(e.value)


@pytest.mark.parametrize("name", sorted(jsoncases.standard_cases()))
def test_response_decodes_to_the_structured_result(klib, tables, name):
    """independent of jsonref: what Python's json module reads back equals the result the objects were written from (the
    cases without invalid UTF-8, which json refuses)"""
    c = jsoncases.standard_cases(valid=True)[name]
    table, entries, features = tables[c["table"]]
    body, off = _format(c, tables)
    doc = json.loads(api.format_json_header(True, table) + body + api.format_json_trailer())
    assert doc["dbProteinFeatures"] == [f.decode() for f in features]
    rep = [q for q in c["queries"] if q["hits"]]
    assert len(doc["results"]) == len(rep) == len(off) - 1
    for obj, q in zip(doc["results"], rep):
        name_ = c["names"][q["src"]].decode("utf-8") if q["src"] < len(c["names"]) else ""
        Q = obj["Query"]
        assert Q["Name"] == name_ and Q["Sequence"] == q["seq"][q["trim"]:].decode("utf-8") and Q["SizeInKmer"] == q["size"]
        assert Q["Type"] == ("Protein Query" if c["protein"] else "DNA Query")
        assert Q["Contig"] == (name_ if (not c["protein"] and c["fmt"] == 0) else "")
        loc = Q["Location"]
        assert (loc["StartPosition"], loc["EndPosition"]) == (q["start"], q["end"])
        assert loc["PlusStrand"] == (q["plus"] and not c["protein"])
        assert loc["StartsAlternative"] == (None if c["protein"] else [])
        S = obj["SearchResults"]
        assert S["Counter"] == {}
        assert [(h["Key"], h["Kmatch"]) for h in S["Hits"]] == [(h["key"], h["kmatch"]) for h in q["hits"]]
        assert all(h["Alignment"]["AlnString"] == "" and h["Alignment"]["BitScore"] == 0 and len(h["Alignment"]) == 13 for h in S["Hits"])
        if c["positions"] or not c["protein"]:
            assert S["PositionHits"] == {str(h["key"]): h["bits"][q["trim"]:] for h in q["hits"]}
            assert list(S["PositionHits"]) == sorted(S["PositionHits"])   # (as strings)
        else:
            assert S["PositionHits"] == {}
        found = []
        for h in q["hits"]:
            if h["key"] not in entries:
                break
            found.append(str(h["key"]))
        assert list(obj["HitEntries"]) == sorted(found)
        for k, v in obj["HitEntries"].items():
            e = entries[int(k)]
            assert v.get("Length", 0) == e["length"] and v.get("EntryId", "") == e["entry_id"].decode() and v.get("Sequence", "") == e["sequence"].decode()
            assert list(v.get("Features", {})) == sorted(f.decode() for f, _ in e["features"])


# ---------------------------------------------------------------- the stand-alone sanitized program
def test_sanitized_program_reports_clean():
    """tools/json_check: the escaper and the formatter under AddressSanitizer + UBSan as a program of their own"""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools", "json_check"), "test"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "json_check:" in r.stdout
