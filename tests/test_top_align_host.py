"""CPU-side checks of the one-call `-aln` (the alignment of the reported hits inside the top-N call): the new symbols are
declared, bound and exported, the ABI version did not move, the header still compiles as C99, the structs a caller
allocates have the size the header says, and NULL / bad arguments come back as KAAMER_E_ARG.  No device calls here."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_ONLY = bool(os.environ.get("KAAMER_HOST_ONLY"))   # the sanitized CPU build holds the host sources only

NEW_SYMBOLS = ["kaamer_index_attach_proteins", "kaamer_index_align_info", "kaamer_index_set_align_budget",
               "kaamer_topn_align_device", "kaamer_search_batch_top_aln_flat", "kaamer_submit_batch_top_aln_flat",
               "kaamer_batch_top_alignments"]


def test_new_symbols_declared_and_bound():
    from kaamer_amd import abi
    src = open(os.path.join(ROOT, "include", "kaamer_hip.h")).read()
    assert re.search(r"#define\s+KAAMER_ABI_VERSION\s+4\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kaamer_[a-z_0-9]+)\s*\(", code))
    for n in NEW_SYMBOLS:
        assert n in declared, "include/kaamer_hip.h does not declare %s" % n
        assert n in abi.SYMBOLS, "abi.py does not bind %s" % n
    # each new entry point says which Go it replaces
    for ref in ("search.go:483-494", "search.go:454-470", "search.go:492", "search.go:461-463"):
        assert ref in src


@pytest.mark.skipif(HOST_ONLY, reason="host-only sanitized library")
def test_new_symbols_exported(klib):
    for n in NEW_SYMBOLS:
        assert hasattr(klib, n), "libkaamer_hip.so lacks %s" % n
    assert klib.kaamer_abi_version() == 4


def test_struct_sizes():
    """the pair record is 64 bytes on both sides; the structs that existed keep their size (additive only)"""
    from kaamer_amd import abi
    assert C.sizeof(abi.AlignPair) == 64
    assert C.sizeof(abi.TopnAlignOpts) == 40
    assert C.sizeof(abi.TopnAlignments) == 40
    assert C.sizeof(abi.Alignment) == 72
    assert C.sizeof(abi.BatchTop) == 80 + C.sizeof(abi.Counters)
    assert C.sizeof(abi.TopnResult) == 64 and C.sizeof(abi.TopnOpts) == 48 and C.sizeof(abi.WorkspaceOpts) == 64


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "kaamer_hip.h"\n'
                   "int main(void) {\n"
                   "    kaamer_align_pair p; kaamer_topn_align_opts o; kaamer_topn_alignments a;\n"
                   "    (void)p; (void)o; (void)a;\n"
                   "    return (sizeof p == 64 && sizeof o == 40 && sizeof a == 40) ? 0 : 1;\n"
                   "}\n")
    exe = tmp_path / "t"
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0


@pytest.mark.skipif(HOST_ONLY, reason="host-only sanitized library")
def test_null_and_bad_arguments(klib):
    from kaamer_amd import abi
    E = abi.E_ARG
    out = C.c_void_p()
    assert klib.kaamer_index_attach_proteins(None, None) == E
    assert klib.kaamer_index_set_align_budget(None, 1 << 20) == E
    info = (C.c_uint64 * 8)()
    assert klib.kaamer_index_align_info(None, info) == E
    assert klib.kaamer_search_batch_top_aln_flat(None, None, None, 0, abi.PROTEIN, 0.05, 10, 10, 0, b"blosum62", 11, 1, 1, C.byref(out)) == E
    assert out.value is None
    assert klib.kaamer_search_batch_top_aln_flat(None, None, None, 0, abi.PROTEIN, 0.05, 10, 10, 0, b"blosum62", 11, 1, 1, None) == E
    t = C.c_void_p()
    assert klib.kaamer_submit_batch_top_aln_flat(None, None, None, 0, abi.PROTEIN, 0.05, 10, 10, 0, b"blosum62", 11, 1, 1, C.byref(t)) == E
    assert klib.kaamer_submit_batch_top_aln_flat(None, None, None, 0, abi.PROTEIN, 0.05, 10, 10, 0, None, 11, 1, 1, C.byref(t)) == E
    assert t.value is None
    items, text = C.POINTER(abi.Alignment)(), C.POINTER(C.c_char)()
    assert klib.kaamer_batch_top_alignments(None, C.byref(items), C.byref(text)) == E
    assert not bool(items) and not bool(text)
    top, o, a = abi.TopnResult(), abi.TopnAlignOpts(), abi.TopnAlignments()
    assert klib.kaamer_topn_align_device(None, None, C.byref(top), C.byref(o), None, C.byref(a)) == E
    assert klib.kaamer_topn_align_device(None, None, None, None, None, None) == E
    assert klib.kaamer_last_error()
