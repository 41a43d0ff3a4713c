"""The three calls of the device makedb TSV reader, as far as a machine without a GPU can see them: exported, declared in the
header and bound in abi.py with the same number of arguments, the argument rules that are checked before any device is
touched, and the header routine the device calls share with kaamer_makedb_tsv, exercised through that reader."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kaamer_makedb_tsv_device", "kaamer_image_build_tsv_device", "kaamer_index_build_tsv")
ARITY = {"kaamer_makedb_tsv_device": 7, "kaamer_image_build_tsv_device": 8, "kaamer_index_build_tsv": 8}
NO_ID = b"TSV file doesn't contain 'EntryID' header"
NO_SEQ = b"TSV file doesn't contain 'Sequence' header"

host_only = pytest.mark.skipif(bool(os.environ.get("KAAMER_HOST_ONLY")), reason="host-only sanitized library: the calls live in the HIP sources")


def _header():
    src = open(os.path.join(ROOT, "include", "kaamer_hip.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


@host_only
def test_symbols_are_exported_declared_and_bound(klib):
    from kaamer_amd import abi
    decl = dict(re.findall(r"\b(kaamer_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", _header()))
    for n in NAMES:
        assert hasattr(klib, n), "libkaamer_hip.so lacks %s" % n
        assert n in decl, "include/kaamer_hip.h does not declare %s" % n
        assert decl[n].count(",") + 1 == ARITY[n] == len(abi.SYMBOLS[n][1]), n
        assert abi.SYMBOLS[n][0] is C.c_int
    from kaamer_amd import api
    assert callable(api.Image.from_tsv_text) and callable(api.Index.from_tsv_text)


def test_rules_of_the_header_comment():
    """the reader's rules stand in the header next to the FASTA reader's, with what is out of scope"""
    src = open(os.path.join(ROOT, "include", "kaamer_hip.h")).read()
    at = src.index("int kaamer_makedb_tsv_device(")
    text = src[src.rindex("The TSV reader on the device", 0, at):at]
    assert src.index("int kaamer_makedb_fasta_device(") < at
    for word in ("lines", "header", "rows", "accept", "table", '"entryid"', '"sequence"', "first H cells", "last such column", "id_base + k",
                 "7 bytes", "upper-cased", ">= 0x80", "header == NULL", "header != NULL", "kaamer_proteins_merge", "kaamer_proteins_count",
                 "KAAMER_E_FORMAT", "KAAMER_E_CAPACITY", "KAAMER_E_ARG", "strict_scanner", "-offset /", "EMBL / GBK", "compressed input",
                 "whole-file driver"):
        assert word in text, word


@host_only
def test_length_is_checked_first(klib):
    """len > 2^32 - 1: KAAMER_E_ARG before anything else -- the text is never read (one byte stands behind the pointer)"""
    from kaamer_amd import abi
    one = b"E"
    for length in (2 ** 32, 2 ** 40, 2 ** 64 - 1):
        h = C.c_void_p()
        assert klib.kaamer_makedb_tsv_device(one, length, None, 0, 0, 0, C.byref(h)) == abi.E_ARG and not h.value
        assert klib.kaamer_makedb_tsv_device(one, length, b"EntryID\tSequence", 16, 0, 0, C.byref(h)) == abi.E_ARG and not h.value
        assert klib.kaamer_makedb_tsv_device(one, length, None, 0, 0, 0, None) == abi.E_ARG
        p, o = C.c_void_p(), C.c_void_p()
        assert klib.kaamer_image_build_tsv_device(one, length, 0, 1, 0.5, 0, C.byref(p), C.byref(o)) == abi.E_ARG
        assert klib.kaamer_index_build_tsv(one, length, 0, 1, 0.5, 0, C.byref(p), C.byref(o)) == abi.E_ARG
        assert not p.value and not o.value
    assert b"2^32" in klib.kaamer_last_error()


@host_only
def test_null_and_shard_arguments(klib):
    from kaamer_amd import abi
    text = b"EntryID\tSequence\na\tACDEFGH\n"
    h, p, o = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert klib.kaamer_makedb_tsv_device(text, len(text), None, 0, 0, 0, None) == abi.E_ARG
    assert klib.kaamer_makedb_tsv_device(None, 5, None, 0, 0, 0, C.byref(h)) == abi.E_ARG and not h.value
    assert klib.kaamer_makedb_tsv_device(text, len(text), b"EntryID\nSequence", 16, 0, 0, C.byref(h)) == abi.E_ARG and not h.value   # '\n' in the header
    for fn in (klib.kaamer_image_build_tsv_device, klib.kaamer_index_build_tsv):
        assert fn(text, len(text), 0, 1, 0.5, 0, None, C.byref(o)) == abi.E_ARG
        assert fn(text, len(text), 0, 1, 0.5, 0, C.byref(p), None) == abi.E_ARG
        assert fn(None, 5, 0, 1, 0.5, 0, C.byref(p), C.byref(o)) == abi.E_ARG
        assert fn(text, len(text), 0, 0, 0.5, 0, C.byref(p), C.byref(o)) == abi.E_ARG   # n_shards = 0
        assert fn(text, len(text), 2, 2, 0.5, 0, C.byref(p), C.byref(o)) == abi.E_ARG   # shard >= n_shards
        assert not p.value and not o.value


@host_only
def test_header_errors_come_before_the_device(klib):
    """the header is read on the host by kaamer_makedb_tsv's routine: its two messages, from either form of the call, with
    no device touched (device -1 would be KAAMER_E_HIP)"""
    from kaamer_amd import abi
    cases = [(b"", None, NO_ID), (b"Sequence\tx\nACDEFGH\ty\n", None, NO_ID), (b"EntryID\tx\na\ty\n", None, NO_SEQ),
             (b"a\tACDEFGH\n", b"", NO_ID), (b"a\tACDEFGH\n", b"name\tSequence", NO_ID), (b"a\tACDEFGH\n", b"entryid\tseq", NO_SEQ)]
    for text, header, msg in cases:
        h = C.c_void_p()
        assert klib.kaamer_makedb_tsv_device(text, len(text), header, len(header or b""), 0, -1, C.byref(h)) == abi.E_FORMAT and not h.value
        assert klib.kaamer_last_error() == msg
        if header is None:
            p, o = C.c_void_p(), C.c_void_p()
            assert klib.kaamer_image_build_tsv_device(text, len(text), 0, 1, 0.5, -1, C.byref(p), C.byref(o)) == abi.E_FORMAT
            assert klib.kaamer_index_build_tsv(text, len(text), 0, 1, 0.5, -1, C.byref(p), C.byref(o)) == abi.E_FORMAT
            assert not p.value and not o.value and klib.kaamer_last_error() == msg


def test_python_forms_keep_the_host_call(klib):
    """device=None is the call that was there before; header / id_base belong to the device reader"""
    from kaamer_amd import api
    text = b"EntryID\tName\tSequence\na\tone\tACDEFGH\nb\ttwo\tACDEFG\nc\tthree\tacdefghik\n"
    p = api.Proteins.from_tsv(text)
    assert p.ids.tolist() == [0, 1] and p.stats()["NumberOfAA"] == 16 and p.feature_names == [b"Name"]
    assert api.Proteins.from_tsv(text, device=None).ids.tolist() == [0, 1]
    with pytest.raises(ValueError):
        api.Proteins.from_tsv(text, header=b"EntryID\tName\tSequence")
    with pytest.raises(ValueError):
        api.Proteins.from_tsv(text, header=b"")
    with pytest.raises(ValueError):
        api.Proteins.from_tsv(text, id_base=1)


def _hits(text):
    """feature names, and (EntryId, Sequence, feature cells in column order) of every record (kaamer_fetch_hits; by position,
    since feature names may repeat)"""
    import numpy as np
    from kaamer_amd import abi, api
    p = api.Proteins.from_tsv(text)
    ids = np.ascontiguousarray(p.ids, dtype=np.uint32)
    ent = (abi.ProteinEntry * max(1, len(ids)))()
    abi.check(abi.lib().kaamer_fetch_hits(p._h, ids.ctypes.data, len(ids), ent))
    out = []
    for e in ent[:len(ids)]:
        assert e.found
        fo = [e.feature_off[i] for i in range(e.n_features + 1)]
        out.append((C.string_at(e.entry_id, e.entry_id_len), C.string_at(e.sequence, e.sequence_len),
                    [C.string_at(e.features + fo[i], fo[i + 1] - fo[i]) if fo[i + 1] > fo[i] else b"" for i in range(e.n_features)]))
    return p.feature_names, out


def _format_error(klib, text):
    from kaamer_amd import abi
    h = C.c_void_p()
    assert klib.kaamer_makedb_tsv(text, len(text), C.byref(h)) == abi.E_FORMAT and not h.value
    return klib.kaamer_last_error()


def test_header_routine_through_the_host_reader(klib):
    """what kaamer_tsv_header decides, seen through kaamer_makedb_tsv"""
    row = (b"a", b"ACDEFGH", [b"x", b"y"])
    # any case of the two names, any column order; feature names as written
    for hdr, line in ((b"EntryID\tSequence\tF1\tf2", b"a\tACDEFGH\tx\ty"), (b"entryid\tSEQUENCE\tF1\tf2", b"a\tACDEFGH\tx\ty"),
                      (b"F1\tsEqUeNcE\tf2\tENTRYID", b"x\tACDEFGH\ty\ta"), (b"Sequence\tF1\tEntryId\tf2", b"ACDEFGH\tx\ta\ty")):
        names, hits = _hits(hdr + b"\n" + line + b"\n")
        assert names == [b"F1", b"f2"] and hits == [row], hdr
    # only ASCII letters are folded; a name with a space or a '\r' inside is a feature
    assert _format_error(klib, b"EntryID \tSequence\na\tACDEFGH\n") == NO_ID
    assert _format_error(klib, b"EntryID\tSequ\xc3\x89nce\na\tACDEFGH\n") == NO_SEQ
    names, hits = _hits(b"EntryID\tSequence\tEntry\rID\r\na\tACDEFGH\tv\r\n")
    assert names == [b"Entry\rID"] and hits == [(b"a", b"ACDEFGH", [b"v"])]
    # duplicate feature names stay separate columns; an empty name is a feature too
    names, hits = _hits(b"F\tEntryID\tF\t\tSequence\n1\ta\t2\t3\tACDEFGH\n")
    assert names == [b"F", b"F", b""] and hits == [(b"a", b"ACDEFGH", [b"1", b"2", b"3"])]
    # a duplicated EntryID / Sequence column: the last one the row HAS wins -- on a short row that is the first
    text = b"EntryID\tSequence\tN\tEntryID\tSequence\n" + b"a\tACDEFGH\tn1\tb\tKLMNPQRST\n" + b"c\tACDEFGHIK\tn2\n" + b"d\tACDEFGH\tn3\t\tKLMNPQR\n" \
           + b"e\tACDEFGH\tn4\tf\n" + b"g\tACDEFGH\tn5\th\tKLM\n"
    names, hits = _hits(text)
    assert names == [b"N"]
    assert hits == [(b"b", b"KLMNPQRST", [b"n1"]), (b"c", b"ACDEFGHIK", [b"n2"]), (b"f", b"ACDEFGH", [b"n4"])]   # empty second EntryId / short second Sequence: rejected
    # both messages, and the texts without a line
    assert _format_error(klib, b"") == NO_ID
    assert _format_error(klib, b"\n") == NO_ID
    assert _format_error(klib, b"Sequence\n") == NO_ID
    assert _format_error(klib, b"x\ty\nEntryID\tSequence\n") == NO_ID   # only the first line is the header
    assert _format_error(klib, b"EntryID\n") == NO_SEQ
    assert _format_error(klib, b"entryid\tentryid\tsequenc\n") == NO_SEQ
    # a header alone, with and without its line end, CRLF
    for text in (b"EntryID\tSequence", b"EntryID\tSequence\n", b"EntryID\tSequence\r\n"):
        names, hits = _hits(text)
        assert names == [] and hits == []
