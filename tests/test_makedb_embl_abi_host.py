"""The calls of the device makedb EMBL reader, as far as a machine without a GPU can see them: exported, declared in the header
and bound in abi.py with the same number of arguments, the argument rules that are checked before any device is touched,
kaamer_text_cut_embl against a restatement, and the texts the device tests run (emblcases.py) through the host reader: the
hand cases give the records written next to them, the fuzz generator's texts are not trivial."""
import ctypes as C
import os
import random
import re

import pytest

import emblcases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"kaamer_text_cut_embl": 2, "kaamer_makedb_embl_device": 5, "kaamer_image_build_embl_device": 8, "kaamer_index_build_embl": 8}

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
        assert abi.SYMBOLS[n][0] is (C.c_uint64 if n == "kaamer_text_cut_embl" else C.c_int)
    assert callable(api.Image.from_embl_text) and callable(api.Index.from_embl_text) and callable(api.text_cut_embl)
    with pytest.raises(ValueError):
        api.Proteins.from_embl(E.EMBL, nb_before=1)
    assert api.Proteins.from_embl(E.EMBL, device=None).ids.tolist() == [1, 5]


def test_rules_of_the_header_comment():
    """the reader's rules stand in the header behind the TSV reader's, with what is out of scope"""
    src = open(os.path.join(ROOT, "include", "kaamer_hip.h")).read()
    at = src.index("int kaamer_makedb_embl_device(")
    text = src[src.rindex("The EMBL reader on the device", 0, at):at]
    assert src.index("int kaamer_image_build_tsv_device(") < at
    for word in ("lines", "tag", "Skip", "drops", "order", "separators", "values", "sequence", "table", '"//"', '"// "', '"///"', "ID GN DE OX OS OC DR SQ",
                 "fewer than 5 bytes", "under 12 bytes", "KEGG; GO; BioCyc; HAMAP;", "fewer than two", "under 19 bytes", "under 17 bytes", "Flags: Fragment;",
                 "below 7", "Atoi", '"Name="', "RecName", "SubName", '";;" + v', "last line wins", "greedily", "trailing ';'", "trailing '.'", "[12:]",
                 "upper-cased", ">= 0x80", "sequence_len > length", "nb_before + k", "kaamer_text_cut_embl", "kaamer_proteins_merge", "gzip", "KAAMER_E_ARG",
                 "KAAMER_E_CAPACITY", "GBK", "strict_scanner", "-offset /", "whole-file driver", "compressed input on the device"):
        assert word in text, word
    cut = src[src.rindex("/*", 0, src.index("uint64_t kaamer_text_cut_embl(")):src.index("uint64_t kaamer_text_cut_embl(")]
    for word in ("greatest p <= len", "exactly \"//\"", "'\\r' drop", "0: none", "p = len"):
        assert word in cut, word
    head = open(os.path.join(ROOT, "kaamer_amd", "csrc", "makedb_embl.hip.inc")).read().split("\nenum", 1)[0]
    for word in ("lines", "tag", "Skip", "drops", "GN", "ProteinName", "separators", "values", "sequence", "ids", "Launches", "null stream", "me_lines_kernel",
                 "me_classify_kernel", "me_read_kernel", "me_fold_kernel<0>", "me_fold_kernel<1>", "No atomic"):
        assert word in head, word


@host_only
def test_length_is_checked_first(klib):
    """len > 2^32 - 1: KAAMER_E_ARG before anything else -- the text is never read (one byte stands behind the pointer)"""
    from kaamer_amd import abi
    one = b"I"
    for length in (2 ** 32, 2 ** 40, 2 ** 64 - 1):
        h = C.c_void_p()
        assert klib.kaamer_makedb_embl_device(one, length, 0, 0, C.byref(h)) == abi.E_ARG and not h.value
        assert klib.kaamer_makedb_embl_device(one, length, 7, 0, None) == abi.E_ARG
        p, o = C.c_void_p(), C.c_void_p()
        assert klib.kaamer_image_build_embl_device(one, length, 0, 1, 0.5, 0, C.byref(p), C.byref(o)) == abi.E_ARG
        assert klib.kaamer_index_build_embl(one, length, 0, 1, 0.5, 0, C.byref(p), C.byref(o)) == abi.E_ARG
        assert not p.value and not o.value
    assert b"2^32" in klib.kaamer_last_error() and b"kaamer_text_cut_embl" in klib.kaamer_last_error()


@host_only
def test_null_shard_and_device_arguments(klib):
    from kaamer_amd import abi
    text = E.EMBL
    h, p, o = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert klib.kaamer_makedb_embl_device(text, len(text), 0, 0, None) == abi.E_ARG
    assert klib.kaamer_makedb_embl_device(None, 5, 0, 0, C.byref(h)) == abi.E_ARG and not h.value
    h = C.c_void_p(1)
    assert klib.kaamer_makedb_embl_device(text, len(text), 0, -1, C.byref(h)) == abi.E_ARG and not h.value   # no such device, before any is touched
    for fn in (klib.kaamer_image_build_embl_device, klib.kaamer_index_build_embl):
        assert fn(text, len(text), 0, 1, 0.5, 0, None, C.byref(o)) == abi.E_ARG
        assert fn(text, len(text), 0, 1, 0.5, 0, C.byref(p), None) == abi.E_ARG
        assert fn(None, 5, 0, 1, 0.5, 0, C.byref(p), C.byref(o)) == abi.E_ARG
        assert fn(text, len(text), 0, 0, 0.5, 0, C.byref(p), C.byref(o)) == abi.E_ARG   # n_shards = 0
        assert fn(text, len(text), 2, 2, 0.5, 0, C.byref(p), C.byref(o)) == abi.E_ARG   # shard >= n_shards
        assert not p.value and not o.value
        p, o = C.c_void_p(1), C.c_void_p(1)
        assert fn(text, len(text), 0, 1, 0.5, -1, C.byref(p), C.byref(o)) == abi.E_ARG and not p.value and not o.value


@host_only
def test_text_cut_hand_cases(klib):
    from kaamer_amd import api
    for text, want in ((b"", 0), (b"//", 2), (b"//\n", 3), (b"//\r\n", 4), (b"//\r", 3), (b"//\nID   x\n", 3), (b"ID   x\n//", 9), (b"ID   x\n//\n", 10),
                       (b"ID   x\r\n//\r\nID   y\r\n", 12), (b"// \n", 0), (b"///\n", 0), (b" //\n", 0), (b"//\r\r\n", 0), (b"ID   x\nSQ\n", 0), (b"\n", 0), (b"\n\n//", 4),
                       (b"//\n//", 5), (b"//\n//x", 3), (b"a//\n//\nb//", 7), (b"/", 0), (b"/\n/\n", 0)):
        assert api.text_cut_embl(text) == want == E.cut_ref(text), text
    assert klib.kaamer_text_cut_embl(None, 0) == 0


@host_only
def test_text_cut_random_texts(klib):
    from kaamer_amd import api
    rng = random.Random(E.SEED)
    hits = 0
    for _ in range(3000):
        text = b"".join(rng.choice([b"/", b"/", b"//", b"\n", b"\n", b"\r", b" ", b"x", b"//\n", b"\r\n"]) for _ in range(rng.randrange(0, 14)))
        cut = api.text_cut_embl(text)
        assert cut == E.cut_ref(text), text
        hits += cut > 0
    assert 500 < hits < 2500


def _records(p):
    """(id, EntryId, indexed, stored Sequence, the cells in column order) of every record"""
    from kaamer_amd import abi
    import numpy as np
    ids = np.ascontiguousarray(p.ids, dtype=np.uint32)
    buf, offs = p.packed
    ent = (abi.ProteinEntry * max(1, len(ids)))()
    abi.check(abi.lib().kaamer_fetch_hits(p._h, ids.ctypes.data, len(ids), ent))
    out = []
    for j, e in enumerate(ent[:len(ids)]):
        fo = [e.feature_off[i] for i in range(e.n_features + 1)]
        out.append((int(ids[j]), C.string_at(e.entry_id, e.entry_id_len), bytes(buf[int(offs[j]):int(offs[j + 1])]), C.string_at(e.sequence, e.sequence_len),
                    [C.string_at(e.features + fo[i], fo[i + 1] - fo[i]) if fo[i + 1] > fo[i] else b"" for i in range(e.n_features)]))
    return out


def test_hand_texts_through_the_host_reader(klib):
    """the records written next to the hand texts are what kaamer_makedb_embl makes of them (the device tests compare with it)"""
    from kaamer_amd import api
    assert _records(api.Proteins.from_embl(E.EMBL)) == E.EMBL_RECORDS
    for name, (text, want) in E.RULES.items():
        p = api.Proteins.from_embl(text)
        assert p.feature_names == E.FEATURES
        if want is not None:
            assert _records(p) == want, name
    for name, (text, n) in E.ENDS.items():
        assert len(api.Proteins.from_embl(text)) == n, name


def test_fuzz_texts_are_not_trivial(klib):
    """the floors the generator's texts reach, over all six parts: kept records, every feature, records that hold more than and
    exactly what they declare, entries dropped by a line the reference panics on and entries dropped otherwise"""
    from kaamer_amd import api
    from oracle import makedb_ref as R
    kept = more = exact = skipped = dropped = 0
    filled = [0] * len(E.FEATURES)
    for text in E.fuzz_texts():
        recs = _records(api.Proteins.from_embl(text))
        kept += len(recs)
        for r in recs:
            more += len(r[3]) > len(r[2])
            exact += len(r[3]) == len(r[2])
            for j, v in enumerate(r[4]):
                filled[j] += v != b""
        n_ref = 0
        for _, entry in R._entries(text):
            try:
                got = R.process_embl(entry)
            except R.RefPanic:
                skipped += 1
                continue
            dropped += got is None
            n_ref += got is not None
        assert n_ref == len(recs)
    assert kept >= 200 and min(filled) >= 30 and more >= 30 and exact >= 30 and skipped >= 50 and dropped >= 50, (kept, filled, more, exact, skipped, dropped)
