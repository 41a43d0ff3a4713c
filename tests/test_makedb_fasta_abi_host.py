"""The three calls of the device makedb FASTA reader, as far as a machine without a GPU can see them: exported, declared in the
header and bound in abi.py with the same number of arguments, and the argument rules that are checked before any device is
touched (on a machine without a device anything else would be KAAMER_E_HIP)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kaamer_makedb_fasta_device", "kaamer_image_build_fasta_device", "kaamer_index_build_fasta")
ARITY = {"kaamer_makedb_fasta_device": 6, "kaamer_image_build_fasta_device": 8, "kaamer_index_build_fasta": 8}

pytestmark = pytest.mark.skipif(bool(os.environ.get("KAAMER_HOST_ONLY")), reason="host-only sanitized library: the calls live in the HIP sources")


def _header():
    src = open(os.path.join(ROOT, "include", "kaamer_hip.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def test_symbols_are_exported_declared_and_bound(klib):
    from kaamer_amd import abi
    decl = dict(re.findall(r"\b(kaamer_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", _header()))
    for n in NAMES:
        assert hasattr(klib, n), "libkaamer_hip.so lacks %s" % n
        assert n in decl, "include/kaamer_hip.h does not declare %s" % n
        assert decl[n].count(",") + 1 == ARITY[n] == len(abi.SYMBOLS[n][1]), n
        assert abi.SYMBOLS[n][0] is C.c_int
    from kaamer_amd import api
    assert callable(api.Image.from_fasta_text) and callable(api.Index.from_fasta_text)


def test_rules_of_the_header_comment():
    """the reader's rules stand in the header next to kaamer_makedb_fasta's, with what is out of scope"""
    src = open(os.path.join(ROOT, "include", "kaamer_hip.h")).read()
    at = src.index("int kaamer_makedb_fasta_device(")
    text = src[src.rindex("The FASTA reader on the device", 0, at):at]
    for word in ("lines", "class", "entries", "ids", "header", "sequence", "drops", "table", '", partial"', "kaamer_text_cut_fasta",
                 "kaamer_makedb_text_range", "TSV / EMBL / GBK", "whole-file driver", "compressed input"):
        assert word in text, word


def test_length_is_checked_first(klib):
    """len > 2^32 - 1: KAAMER_E_ARG before anything else -- the text is never read (one byte stands behind the pointer)"""
    from kaamer_amd import abi
    one = b">"
    for length in (2 ** 32, 2 ** 40, 2 ** 64 - 1):
        h = C.c_void_p()
        assert klib.kaamer_makedb_fasta_device(one, length, 0, 0, 0, C.byref(h)) == abi.E_ARG and not h.value
        assert klib.kaamer_makedb_fasta_device(one, length, 0, 0, 0, None) == abi.E_ARG
        p, o = C.c_void_p(), C.c_void_p()
        assert klib.kaamer_image_build_fasta_device(one, length, 0, 1, 0.5, 0, C.byref(p), C.byref(o)) == abi.E_ARG
        assert klib.kaamer_index_build_fasta(one, length, 0, 1, 0.5, 0, C.byref(p), C.byref(o)) == abi.E_ARG
        assert not p.value and not o.value
    assert b"2^32" in klib.kaamer_last_error()


def test_null_and_shard_arguments(klib):
    from kaamer_amd import abi
    text = b">a x\nACDEFGH\n"
    h, p, o = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert klib.kaamer_makedb_fasta_device(text, len(text), 0, 0, 0, None) == abi.E_ARG
    assert klib.kaamer_makedb_fasta_device(None, 5, 0, 0, 0, C.byref(h)) == abi.E_ARG and not h.value
    for fn in (klib.kaamer_image_build_fasta_device, klib.kaamer_index_build_fasta):
        assert fn(text, len(text), 0, 1, 0.5, 0, None, C.byref(o)) == abi.E_ARG
        assert fn(text, len(text), 0, 1, 0.5, 0, C.byref(p), None) == abi.E_ARG
        assert fn(None, 5, 0, 1, 0.5, 0, C.byref(p), C.byref(o)) == abi.E_ARG
        assert fn(text, len(text), 0, 0, 0.5, 0, C.byref(p), C.byref(o)) == abi.E_ARG   # n_shards = 0
        assert fn(text, len(text), 2, 2, 0.5, 0, C.byref(p), C.byref(o)) == abi.E_ARG   # shard >= n_shards
        assert not p.value and not o.value


def test_python_forms_keep_the_host_call(klib):
    """device=None is the call that was there before; nb_before / more belong to the device reader"""
    from kaamer_amd import api
    text = b">a x\nACDEFGH\n>b y, partial\nACDEFGH\n>c\nacdefghik\n"
    p = api.Proteins.from_fasta(text)
    assert p.ids.tolist() == [2, 3] and p.stats()["NumberOfAA"] == 16
    assert api.Proteins.from_fasta(text, device=None).ids.tolist() == [2, 3]
    with pytest.raises(ValueError):
        api.Proteins.from_fasta(text, nb_before=1)
    with pytest.raises(ValueError):
        api.Proteins.from_fasta(text, more=True)
