"""CPU-side checks of the -aln TSV rows: the new symbols are declared and bound, the header line, the two number formats
on their own, and kaamer_format_tsv_aln_arrays (the host formatter: what kaamer_format_tsv_aln runs on a result of the
library) against the restatement of search.go:556-604 in tsvalnref.py, byte for byte with the line offsets, on hand-built
results.  No device calls here."""
import ctypes as C
import math
import os
import re
import struct

import numpy as np
import pytest

import tsvalncases
import tsvalnref
import tsvcases
import tsvref
from kaamer_amd import abi, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["kaamer_format_tsv_aln_header", "kaamer_format_tsv_aln", "kaamer_format_tsv_aln_arrays", "kaamer_format_double",
               "kaamer_align_finish_pairs", "kaamer_tsv_aln_rows_device", "kaamer_tsv_aln_info", "kaamer_tsv_format_doubles_device",
               "kaamer_index_tsv_aln_info", "kaamer_index_set_tsv_aln_raw_count"] + \
              ["kaamer_%s_%s_top_aln_tsv_flat" % (a, b) for a in ("submit", "search") for b in ("text", "fasta", "bgzf")]
FLAGS = [(False, False), (False, True), (True, False), (True, True)]


def test_new_symbols_declared_bound_and_exported(klib):
    src = open(os.path.join(ROOT, "include", "kaamer_hip.h")).read()
    assert re.search(r"#define\s+KAAMER_ABI_VERSION\s+4\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kaamer_[a-z_0-9]+)\s*\(", code))
    for n in NEW_SYMBOLS:
        assert n in declared, "include/kaamer_hip.h does not declare %s" % n
        assert n in abi.SYMBOLS, "abi.py does not bind %s" % n
        assert hasattr(klib, n), "the library lacks %s" % n
    assert "Out of scope: the -aln TSV form" not in src
    assert abi.E_RANGE == -8 and re.search(r"KAAMER_E_RANGE\s*=\s*-8\b", code)


@pytest.fixture(scope="module")
def table(klib):
    return tsvcases.standard_table()


@pytest.fixture(scope="module")
def entries(table):
    return tsvref.entries_of(table)


@pytest.mark.parametrize("positions,annotations", FLAGS)
def test_header(klib, table, positions, annotations):
    want = tsvalnref.header_ref(positions, annotations, table.feature_names)
    assert api.format_tsv_header(positions, annotations, table, align=True) == want
    assert want.startswith(b"QueryId\tSubjectId\t%Identity\tAlnLength\tMismatches\tGapOpen\tQStart\tQEnd\tSStart\tSEnd\tEvalue\tBitscore")
    if not annotations:
        assert api.format_tsv_header(positions, annotations, None, align=True) == want
    for cap in (1, 5, len(want), len(want) + 1):      # the short-buffer convention of kaamer_format_positions
        raw = (C.c_char * (cap + 8))()
        C.memset(raw, 0x55, cap + 8)
        need = klib.kaamer_format_tsv_aln_header(int(positions), int(annotations), table._h, C.cast(raw, C.c_char_p), cap)
        got = bytes(raw)
        n = min(len(want), cap - 1)
        assert need == len(want) and got[cap:] == b"\x55" * 8 and got[:n] == want[:n] and got[n] == 0


def double_vectors():
    """the doubles the device test prints too: zeros, the ends of the range, every power of two, the doubles around every
    power of ten, carries into the exponent, exact ties, the specials, random bit patterns"""
    def around(x):
        return [math.nextafter(x, -math.inf), x, math.nextafter(x, math.inf)]
    v = [0.0, -0.0, 5e-324, -5e-324, 1.7976931348623157e308, -1.7976931348623157e308]
    v += [math.ldexp(1.0, k) for k in range(-1074, 1024)]
    for k in range(-300, 301):
        v += around(float("1e%d" % k))
    for x in (999999.95, 9.9999995e5, 1000000.5, 1000001.5, 0.125, 0.375, 2.5e-3, -0.125, 0.005, 0.995, 99.995, 9999999.5, 2.0 ** 63, 2.0 ** 64):
        v += around(x)
    v += [math.inf, -math.inf, math.nan]
    rng = np.random.default_rng(20261003)
    v += np.frombuffer(rng.integers(0, 2 ** 64, 100000, dtype=np.uint64).tobytes(), np.float64).tolist()
    return v


def test_double_formats_against_python(klib):
    # what the restatement leans on: Python rounds the exact value half-even, ties included
    assert "%e" % 1000000.5 == "1.000000e+06" and "%e" % 1000001.5 == "1.000002e+06" and "%e" % 999999.95 == "9.999999e+05"
    assert ["%.2f" % x for x in (0.125, 0.375, 2.5e-3, -0.125)] == ["0.12", "0.38", "0.00", "-0.12"]
    assert "%e" % 5e-324 == "4.940656e-324" and "%e" % 9.9999995e5 == "9.999999e+05"
    for x in double_vectors():
        assert api.format_double(x, 0).decode() == tsvalnref.e_ref(x), "%%e of %r (%s)" % (x, struct.pack(">d", x).hex())
        assert api.format_double(x, 1).decode() == tsvalnref.f2_ref(x), "%%.2f of %r (%s)" % (x, struct.pack(">d", x).hex())


def check(table, entries, names, queries, positions, annotations, seq_type):
    naa = table.stats()["NumberOfAA"]
    queries = tsvalncases.with_alignments(queries, naa)
    buf, spans = tsvcases.names_buffer(names)
    protein = abi.seq_type_base(seq_type) == abi.PROTEIN
    want, want_off = tsvalnref.rows_ref(tsvalncases.ref_queries(names, queries), entries, table.feature_names, positions, annotations, protein)
    got, got_off = api.format_tsv(tsvalncases.host_top(queries), buf, spans, table, positions, annotations, align=True, seq_type=seq_type)
    assert got == want
    assert got_off.tolist() == want_off.tolist()
    return got


@pytest.mark.parametrize("seq_type", [abi.PROTEIN, abi.READS, abi.seq_type(abi.NUCLEOTIDE, 4)])
@pytest.mark.parametrize("positions,annotations", FLAGS)
def test_rows_on_hand_built_results(klib, table, entries, positions, annotations, seq_type):
    for name, (names, queries) in tsvalncases.standard_cases().items():
        check(table, entries, names, queries, positions, annotations, seq_type)


def test_specific_rows(klib, table, entries):
    """a few rows spelled out, so that the restatement itself is pinned"""
    names, queries = tsvalncases.standard_cases()["order"]
    rows = [r.split(b"\t") for r in check(table, entries, names, queries, False, False, abi.PROTEIN).split(b"\n")[:-1]]
    ids = [entries[i]["EntryId"] for i in range(11)]
    assert [r[1] for r in rows[:6]] == ids[:6]                                  # equal raw scores keep their rank
    assert [r[1] for r in rows[6:16]] == ids[:10][::-1]                          # increasing ones come out reversed
    assert [r[1] for r in rows[16:22]] == [ids[2], ids[5], ids[0], ids[4], ids[1], ids[3]]   # failed hits behind, in their order
    assert rows[20][2:] == rows[21][2:] == [b"0.00", b"0", b"0", b"0", b"0", b"0", b"0", b"0", b"0.000000e+00", b"0.00"]
    assert [r[1] for r in rows[22:]] == [ids[8], ids[7], b"", b"", b""]           # the missing id ends the query's entries
    assert rows[0][0] == b"read/1" and rows[6][0] == b"second" and rows[16][0] == b"p3"
    # raw 100, 40 columns of which 20 identical, shift 0: BLOSUM62 11 / 1 is lambda 0.267, K 0.041
    bits = (0.267 * 100 - math.log(0.041)) / math.log(2)
    ev = 50.0 * table.stats()["NumberOfAA"] / 2.0 ** bits
    assert rows[0][2:] == [b"50.00", b"40", b"20", b"0", b"1", b"40", b"1", b"40", ("%e" % ev).encode(), ("%.2f" % bits).encode()]
    # ORFs print the location instead of the alignment's query coordinates
    rows_r = [r.split(b"\t") for r in check(table, entries, names, queries, False, False, abi.READS).split(b"\n")[:-1]]
    assert rows_r[0][6:8] == [b"4", b"33"] and rows_r[6][6:8] == [b"200", b"18"] and rows_r[0][:6] == rows[0][:6] and rows_r[0][8:] == rows[0][8:]
    names, queries = tsvalncases.standard_cases()["numbers"]
    rows = [r.split(b"\t") for r in check(table, entries, names, queries, False, False, abi.PROTEIN).split(b"\n")[:-1]]
    assert rows[0][2:10] == [b"NaN", b"0", b"0", b"0", b"1", b"0", b"1", b"0"] and rows[0][10] == b"0.000000e+00"   # len(query) 0
    assert rows[1][2] == b"NaN" and rows[1][10] != b"0.000000e+00" and len(rows) == 16
    assert any(r[10] == b"0.000000e+00" and r[2] != b"0.00" for r in rows[8:14])    # 2^BitScore overflows: EValue 0
    assert float(rows[7][-1]) < float(rows[6][-1]) < 0 < float(rows[5][-1]) < 4.61    # raw -65536, -2072, -1: BitScores below raw 0's, last
    assert rows[-1][3:10] == [b"2147483647"] * 7 and rows[-1][2] == b"100.00"


def test_without_alignments_and_short_buffers(klib, table, entries):
    names, queries = tsvalncases.standard_cases()["bitmaps"]
    queries = tsvalncases.with_alignments(queries, 1000)
    buf, spans = tsvcases.names_buffer(names)
    top = tsvalncases.host_top(queries)
    want, _ = tsvalnref.rows_ref(tsvalncases.ref_queries(names, queries), entries, table.feature_names, True, True, True)
    for cap in (0, 1, 2, 100, len(want) - 1, len(want), len(want) + 1):
        got, need = api.format_tsv(top, buf, spans, table, True, True, cap=cap, align=True)
        assert need == len(want) and got == want[:max(min(cap - 1, len(want)), 0)]
    top.pos_bits = None                                # ExtractPositions on a result without bitmaps
    with pytest.raises(abi.KaamerError) as e:
        api.format_tsv(top, buf, spans, table, True, False, align=True)
    assert e.value.code == abi.E_ARG
    top.alignments = None                              # a result without alignments
    with pytest.raises(abi.KaamerError) as e:
        api.format_tsv(top, buf, spans, table, False, False, align=True)
    assert e.value.code == abi.E_ARG and "alignments" in str(e.value)
    assert api.format_tsv(top, buf, spans, table, False, False)[0].count(b"\n") == len(top.top_pid)   # the plain rows still print
