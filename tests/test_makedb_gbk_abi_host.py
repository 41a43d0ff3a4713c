"""The calls of the device makedb GBK reader, as far as a machine without a GPU can see them: exported, declared in the header
and bound in abi.py with the same number of arguments, the argument rules that are checked before any device is touched, and
the texts the device tests run (gbkcases.py) through the host reader: the hand cases give the records written next to them,
the fuzz generator's texts are not trivial."""
import ctypes as C
import os
import re

import pytest

import gbkcases as G
from test_makedb_embl_abi_host import _records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"kaamer_makedb_gbk_device": 5, "kaamer_image_build_gbk_device": 8, "kaamer_index_build_gbk": 8}

host_only = pytest.mark.skipif(bool(os.environ.get("KAAMER_HOST_ONLY")), reason="host-only sanitized library: the calls live in the HIP sources")


def _header():
    src = open(os.path.join(ROOT, "include", "kaamer_hip.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


@host_only
def test_symbols_are_exported_declared_and_bound(klib):
    from kaamer_amd import abi, api
    decl = dict(re.findall(r"\b(kaamer_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", _header()))
    for n in ARITY:
        assert hasattr(klib, n), "libkaamer_hip.so lacks %s" % n
        assert n in decl, "include/kaamer_hip.h does not declare %s" % n
        assert decl[n].count(",") + 1 == ARITY[n] == len(abi.SYMBOLS[n][1]), n
        assert abi.SYMBOLS[n][0] is C.c_int
    assert "kaamer_text_cut_gbk" not in decl and not hasattr(klib, "kaamer_text_cut_gbk")   # the cut is EMBL's: no second C function
    assert callable(api.Image.from_gbk_text) and callable(api.Index.from_gbk_text)
    for text in (b"", b"//", b"//\r\n", b"LOCUS       x\n//\nLOCUS       y\n", b" //\n", b"// x\n"):
        assert api.text_cut_gbk(text) == api.text_cut_embl(text) == G.cut_ref(text)


def test_from_gbk_keeps_todays_call(klib):
    from kaamer_amd import api
    with pytest.raises(ValueError):
        api.Proteins.from_gbk(G.GBK, nb_before=1)
    assert api.Proteins.from_gbk(G.GBK).ids.tolist() == api.Proteins.from_gbk(G.GBK, device=None).ids.tolist() == [1, 5]


def test_rules_of_the_header_comment():
    """the reader's rules stand in the header behind the EMBL reader's, with what is out of scope, and at the head of the file"""
    src = open(os.path.join(ROOT, "include", "kaamer_hip.h")).read()
    at = src.index("int kaamer_makedb_gbk_device(")
    text = src[src.rindex("The GBK reader on the device", 0, at):at]
    assert src.index("int kaamer_image_build_embl_device(") < at and src.index("int kaamer_index_build_embl(") < src.index("int kaamer_index_build_gbk(")
    words = ("lines", "token", "contribution", "Skip", "drops", "ProteinName", "table", '"//"', '" //"', '"// x"', "LOCUS ACCESSION KEYWORDS", "SOURCE COMMENT REFERENCE DBLINK DBSOURCE",
             "DEFINITION", "VERSION", "ORGANISM", "FEATURES", "ORIGIN", "case-sensitively", "spaces only", "empty token", "state 0", "[12:]", "[10:]", "trailing space",
             "first field", "last such line wins", "upper-cased", ">= 0x80", "2 to 11 bytes", "2 to 9 bytes", "bare ORIGIN", "no field behind column 12", '", partial"',
             "span a join", "fewer than 7 residues", 'first " ["', 'last "]."', "GBK_DEF_FTS", "nb_before + k")
    for word in words + ("kaamer_text_cut_embl", "kaamer_proteins_merge", "gzip", "KAAMER_E_ARG", "KAAMER_E_CAPACITY", "strict_scanner", "-offset /", "whole-file driver",
                         "inflate on the device", "sequence_len == length", "process_gbk_entry"):
        assert word in text, word
    cut = src[src.rindex("/*", 0, src.index("uint64_t kaamer_text_cut_embl(")):src.index("uint64_t kaamer_text_cut_embl(")]
    assert "kaamer_makedb_gbk_device" in cut
    head = open(os.path.join(ROOT, "kaamer_amd", "csrc", "makedb_gbk.hip.inc")).read().split("\nenum", 1)[0]
    for word in words + ("ids", "Launches", "null stream", "me_lines_kernel", "mg_classify_kernel", "mg_lead_kernel", "mg_state_kernel<0>", "mg_state_scan_kernel",
                         "mg_state_kernel<1>", "mg_read_kernel", "mg_fold_kernel<0>", "mg_fold_kernel<1>", "me_term_scan_kernel", "me_ent_scan_kernel", "No\n// atomic"):
        assert word in head, word
    search = open(os.path.join(ROOT, "kaamer_amd", "csrc", "search.hip")).read()
    assert search.index('#include "makedb_embl.hip.inc"') < search.index('#include "makedb_gbk.hip.inc"')


@host_only
def test_length_is_checked_first(klib):
    """len > 2^32 - 1: KAAMER_E_ARG before anything else -- the text is never read (one byte stands behind the pointer)"""
    from kaamer_amd import abi
    one = b"L"
    for length in (2 ** 32, 2 ** 40, 2 ** 64 - 1):
        h = C.c_void_p()
        assert klib.kaamer_makedb_gbk_device(one, length, 0, 0, C.byref(h)) == abi.E_ARG and not h.value
        assert b"2^32" in klib.kaamer_last_error() and b"kaamer_text_cut_embl" in klib.kaamer_last_error()
        assert klib.kaamer_makedb_gbk_device(one, length, 7, 0, None) == abi.E_ARG
        for fn in (klib.kaamer_image_build_gbk_device, klib.kaamer_index_build_gbk):
            p, o = C.c_void_p(), C.c_void_p()
            assert fn(one, length, 0, 1, 0.5, 0, C.byref(p), C.byref(o)) == abi.E_ARG and not p.value and not o.value
            assert b"2^32" in klib.kaamer_last_error() and b"kaamer_text_cut_embl" in klib.kaamer_last_error()


@host_only
def test_null_shard_and_device_arguments(klib):
    from kaamer_amd import abi
    text = G.GBK
    h, p, o = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert klib.kaamer_makedb_gbk_device(text, len(text), 0, 0, None) == abi.E_ARG
    assert klib.kaamer_makedb_gbk_device(None, 5, 0, 0, C.byref(h)) == abi.E_ARG and not h.value
    h = C.c_void_p(1)
    assert klib.kaamer_makedb_gbk_device(text, len(text), 0, -1, C.byref(h)) == abi.E_ARG and not h.value   # no such device, before any is touched
    for fn in (klib.kaamer_image_build_gbk_device, klib.kaamer_index_build_gbk):
        assert fn(text, len(text), 0, 1, 0.5, 0, None, C.byref(o)) == abi.E_ARG
        assert fn(text, len(text), 0, 1, 0.5, 0, C.byref(p), None) == abi.E_ARG
        assert fn(None, 5, 0, 1, 0.5, 0, C.byref(p), C.byref(o)) == abi.E_ARG
        assert fn(text, len(text), 0, 0, 0.5, 0, C.byref(p), C.byref(o)) == abi.E_ARG   # n_shards = 0
        assert fn(text, len(text), 2, 2, 0.5, 0, C.byref(p), C.byref(o)) == abi.E_ARG   # shard >= n_shards
        assert not p.value and not o.value
        p, o = C.c_void_p(1), C.c_void_p(1)
        assert fn(text, len(text), 0, 1, 0.5, -1, C.byref(p), C.byref(o)) == abi.E_ARG and not p.value and not o.value


def test_hand_texts_through_the_host_reader(klib):
    """the records written next to the hand texts are what kaamer_makedb_gbk makes of them (the device tests compare with it),
    and what the restatement of the reference makes of them"""
    from kaamer_amd import api
    from oracle import makedb_ref as R
    assert _records(api.Proteins.from_gbk(G.GBK)) == G.GBK_RECORDS
    for name, (text, want) in G.RULES.items():
        p = api.Proteins.from_gbk(text)
        assert p.feature_names == G.FEATURES
        got = _records(p)
        if want is not None:
            assert got == want, name
        ref = []
        for pid, ent in R._entries(text):
            try:
                r = R.process_gbk(ent)
            except R.RefPanic:
                continue
            if r is not None:
                ref.append((pid, r[0], r[1], r[1], [r[3].get(n, b"") for n in G.FEATURES]))
        assert got == ref, name
    for name, (text, n) in G.ENDS.items():
        assert len(api.Proteins.from_gbk(text)) == n, name


def test_fuzz_texts_are_not_trivial(klib):
    """the floors the generator's texts reach: kept records, every cell, entries the reference panics on, entries dropped by
    ", partial" (across a join among them) and as too short, names the bracket rule shortens (with a " [" that a join forms
    among them); the host reader keeps what the restatement keeps"""
    from kaamer_amd import api
    from oracle import makedb_ref as R
    kept = panics = partial = partial_join = short = cut = cut_join = 0
    filled = [0] * len(G.FEATURES)
    for text in G.fuzz_texts():
        recs = {r[0]: r for r in _records(api.Proteins.from_gbk(text))}
        kept += len(recs)
        for r in recs.values():
            for j, v in enumerate(r[4]):
                filled[j] += v != b""
        n_ref = 0
        for pid, ent in R._entries(text):
            try:
                got = R.process_gbk(ent)
            except R.RefPanic:
                panics += 1
                continue
            pieces = G.name_pieces(ent, R._GBK_STATE)
            name, seps = G.join_name(pieces)
            if got is None:
                if b", partial" in name:
                    partial += 1
                    partial_join += not any(b", partial" in p for p in pieces)
                else:
                    short += 1
                continue
            n_ref += 1
            assert pid in recs and recs[pid][1] == got[0] and recs[pid][2] == got[1]
            if recs[pid][4][0] != name:
                cut += 1
                cut_join += name.index(b" [") in seps
        assert n_ref == len(recs)
    floors = (kept >= 200, min(filled) >= 30, panics >= 50, partial >= 30, partial_join >= 10, short >= 30, cut >= 30, cut_join >= 10)
    assert all(floors), (kept, filled, panics, partial, partial_join, short, cut, cut_join)
