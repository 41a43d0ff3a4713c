"""The stream and whole-file drivers with -pos / -aln on all three handle kinds (kaamer_stream_open_aln_flat, the replica
forms, kaamer_sharded_stream_*, kaamer_search_file_opts, kaamer_sharded_search_file): what can be said of them without a
device -- they are declared, bound, exported, additive (ABI version 4), and they refuse bad arguments before they touch a
handle."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_ONLY = bool(os.environ.get("KAAMER_HOST_ONLY"))   # the sanitized CPU build holds the host sources only
NEW_SYMBOLS = (
    "kaamer_stream_open_aln_flat",
    "kaamer_replicas_attach_proteins", "kaamer_replica_stream_open_pos_flat", "kaamer_replica_stream_open_aln_flat",
    "kaamer_sharded_stream_open_flat", "kaamer_sharded_stream_open_pos_flat", "kaamer_sharded_stream_open_aln_flat",
    "kaamer_sharded_stream_push", "kaamer_sharded_stream_pop", "kaamer_sharded_stream_pending", "kaamer_sharded_stream_close",
    "kaamer_search_file_opts", "kaamer_sharded_search_file",
)
E_ARG = -1


def test_new_symbols_declared_and_bound():
    from kaamer_amd import abi
    src = open(os.path.join(ROOT, "include", "kaamer_hip.h")).read()
    assert re.search(r"#define\s+KAAMER_ABI_VERSION\s+4\b", src)
    m = re.search(r"#define\s+KAAMER_SHARDED_SETS\s+(\d+)\b", src)
    assert m and int(m.group(1)) == abi.SHARDED_SETS
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kaamer_[a-z_0-9]+)\s*\(", code))
    assert "kaamer_sharded_stream" in re.findall(r"typedef struct (\w+) \1;", code)
    for n in NEW_SYMBOLS:
        assert n in declared, "include/kaamer_hip.h does not declare %s" % n
        assert n in abi.SYMBOLS, "abi.py does not bind %s" % n
    # the two file drivers take the same arguments behind the handle, the callback type is the existing one
    assert abi.SYMBOLS["kaamer_search_file_opts"] == abi.SYMBOLS["kaamer_sharded_search_file"]
    assert len(abi.SYMBOLS["kaamer_search_file_opts"][1]) == 20
    assert "kaamer_chunk_cb cb" in code[code.index("kaamer_sharded_search_file"):]


@pytest.mark.skipif(HOST_ONLY, reason="host-only sanitized library")
def test_new_symbols_exported(klib):
    for n in NEW_SYMBOLS:
        assert hasattr(klib, n), "libkaamer_hip.so lacks %s" % n
    assert klib.kaamer_abi_version() == 4


def _file_args(chunk_seqs):
    """(path .. total) of kaamer_search_file_opts / kaamer_sharded_search_file behind the handle"""
    return (b"/nonexistent/reads.fastq", 1, 0, 2, 0.05, 10, 10, 0, 0, None, 11, 1, 0, chunk_seqs, 1 << 20, 0, None, None, None)


@pytest.mark.skipif(HOST_ONLY, reason="host-only sanitized library")
def test_null_handles(klib):
    h = C.c_void_p()
    offs = (C.c_uint64 * 1)(0)
    out = C.c_void_p()
    assert klib.kaamer_stream_open_aln_flat(None, 1, 0.05, 10, 10, 0, b"blosum62", 11, 1, 1, C.byref(h)) == E_ARG
    assert klib.kaamer_replicas_attach_proteins(None, None) == E_ARG
    assert klib.kaamer_replica_stream_open_pos_flat(None, 1, 0.05, 10, 10, C.byref(h)) == E_ARG
    assert klib.kaamer_replica_stream_open_aln_flat(None, 1, 0.05, 10, 10, 0, b"blosum62", 11, 1, 1, C.byref(h)) == E_ARG
    assert klib.kaamer_sharded_stream_open_flat(None, 1, 0.05, 10, 10, C.byref(h)) == E_ARG
    assert klib.kaamer_sharded_stream_open_pos_flat(None, 1, 0.05, 10, 10, C.byref(h)) == E_ARG
    assert klib.kaamer_sharded_stream_open_aln_flat(None, 1, 0.05, 10, 10, 0, b"blosum62", 11, 1, 1, C.byref(h)) == E_ARG
    assert h.value is None
    assert klib.kaamer_sharded_stream_push(None, None, offs, 0) == E_ARG
    assert klib.kaamer_sharded_stream_pop(None, C.byref(out)) == E_ARG
    assert klib.kaamer_sharded_stream_pending(None) == 0
    klib.kaamer_sharded_stream_close(None)
    assert klib.kaamer_search_file_opts(None, *_file_args(100)) == E_ARG
    assert klib.kaamer_sharded_search_file(None, *_file_args(100)) == E_ARG
    assert b"bad argument" in klib.kaamer_last_error()


@pytest.mark.skipif(HOST_ONLY, reason="host-only sanitized library")
def test_chunk_seqs_zero_and_pop_on_an_empty_stream(klib):
    """The argument checks run before the handle is looked at, and a sharded stream keeps the handle's address without
    reading it until the first push: a block of zeroed memory stands in for a handle here, where no device exists."""
    stand_in = C.create_string_buffer(4096)
    handle = C.cast(stand_in, C.c_void_p)
    assert klib.kaamer_search_file_opts(handle, *_file_args(0)) == E_ARG
    assert b"bad argument" in klib.kaamer_last_error()
    assert klib.kaamer_sharded_search_file(handle, *_file_args(0)) == E_ARG
    assert b"bad argument" in klib.kaamer_last_error()
    assert klib.kaamer_search_file(handle, b"/nonexistent/reads.fastq", 1, 0, 2, 0.05, 10, 10, 0, 1 << 20, 0, None, None, None) == E_ARG
    # alignments asked for without a matrix name
    args = list(_file_args(100))
    args[8] = 1
    assert klib.kaamer_sharded_search_file(handle, *args) == E_ARG
    st = C.c_void_p()
    assert klib.kaamer_sharded_stream_open_flat(handle, 2, 0.05, 10, 0, C.byref(st)) == E_ARG      # MaxResults < 1
    assert klib.kaamer_sharded_stream_open_flat(handle, 2, 0.05, 10, 10, C.byref(st)) == 0
    assert klib.kaamer_sharded_stream_pending(st) == 0
    out = C.c_void_p()
    assert klib.kaamer_sharded_stream_pop(st, C.byref(out)) == E_ARG
    assert b"nothing was pushed" in klib.kaamer_last_error() and out.value is None
    assert klib.kaamer_sharded_stream_push(st, None, None, 0) == E_ARG                              # no offsets
    klib.kaamer_sharded_stream_close(st)
    # the one-index stream: the same answer from kaamer_stream_pop
    assert klib.kaamer_stream_open_flat(handle, 2, 0.05, 10, 10, C.byref(st)) == 0
    assert klib.kaamer_stream_pop(st, C.byref(out)) == E_ARG
    klib.kaamer_stream_close(st)
