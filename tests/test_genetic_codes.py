"""The request's genetic code, host side: the library's thirteen tables (kaamer_genetic_code) against the fixture parsed from
the reference's gcode_N maps, the KAAMER_SEQ_TYPE packing, and the soundness of the expected side the GPU tests
(test_gpu_genetic_codes.py) are held against.  No device calls here."""
import ctypes as C
import json
import os
import re

import pytest

import gcoderef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kaamer_hip.h")


def test_fixture_shape():
    fx = gcoderef.fixture()
    assert sorted(int(k) for k in fx) == list(gcoderef.CODES)
    bacteria = json.load(open(os.path.join(ROOT, "tests", "golden", "gcode_bacteria.json")))
    assert fx["11"] == bacteria
    for code, t in fx.items():
        assert sorted(t) == sorted(gcoderef.CODONS)
        assert all(stop == (aa == "*") for aa, start, stop in t.values()), code


@pytest.mark.parametrize("code", (0,) + gcoderef.CODES)
def test_library_table_equals_fixture(klib, code):
    from kaamer_amd import abi
    aa, start = abi.genetic_code(code)
    t = gcoderef.fixture()[str(code or 11)]
    assert len(aa) == len(start) == 64
    for i, codon in enumerate(gcoderef.CODONS):
        assert aa[i] == t[codon][0], (code, codon)
        assert start[i] == ("M" if t[codon][1] else "-"), (code, codon)


@pytest.mark.parametrize("code", (7, 8, 16, 255, -1, 256 + 4))
def test_library_refuses_unknown_codes(klib, code):
    from kaamer_amd import abi
    aa, start = C.create_string_buffer(64), C.create_string_buffer(64)
    assert klib.kaamer_genetic_code(code, aa, start) == abi.E_ARG
    assert str(code).encode() in klib.kaamer_last_error()
    with pytest.raises(abi.KaamerError):
        abi.genetic_code(code)


def _macro(src, name):
    m = re.search(r"#define\s+%s\((\w+)(?:,\s*(\w+))?\)\s+(.*)" % name, src)
    assert m, "include/kaamer_hip.h does not define %s" % name
    return [a for a in m.groups()[:2] if a], m.group(3)


def _c_eval(args, body, *values):
    """a KAAMER_SEQ_TYPE* macro body as Python (casts dropped: every value here is a small non-negative int)"""
    expr = body.replace("(int32_t)", "")
    for a, v in zip(args, values):
        expr = re.sub(r"\b%s\b" % a, str(int(v)), expr)
    assert re.fullmatch(r"[0-9xXa-fA-F()|&<> ]+", expr), expr
    return eval(expr)


def test_seq_type_macro_and_accessors_round_trip():
    from kaamer_amd import abi
    src = open(HEADER).read()
    mk, base, code = _macro(src, "KAAMER_SEQ_TYPE"), _macro(src, "KAAMER_SEQ_TYPE_BASE"), _macro(src, "KAAMER_SEQ_TYPE_GENETIC_CODE")
    for b in (abi.NUCLEOTIDE, abi.PROTEIN, abi.READS):
        assert _c_eval(*mk, b, 0) == abi.seq_type(b) == abi.seq_type(b, 0) == b          # every value that is valid today keeps its meaning
        for g in (0,) + gcoderef.CODES + (255,):
            v = _c_eval(*mk, b, g)
            assert v == abi.seq_type(b, g) == (b | g << 8) and v < 1 << 16
            assert _c_eval(*base, v) == abi.seq_type_base(v) == b
            assert _c_eval(*code, v) == abi.seq_type_genetic_code(v) == g
            assert abi.split_seq_type(v) == (b, g)
    assert abi.GENETIC_CODES == gcoderef.CODES


def test_symbol_declared_bound_and_exported(klib):
    from kaamer_amd import abi
    src = open(HEADER).read()
    assert re.search(r"#define\s+KAAMER_ABI_VERSION\s+4\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert "kaamer_genetic_code" in set(re.findall(r"\b(kaamer_[a-z_0-9]+)\s*\(", code))
    assert "kaamer_genetic_code" in abi.SYMBOLS
    assert hasattr(klib, "kaamer_genetic_code")
    assert klib.kaamer_abi_version() == 4


def test_search_options_carry_the_code():
    from kaamer_amd import search
    assert search.SearchOptions().GeneticCode == 11          # api/server.go:142
    assert search.SearchOptions(GeneticCode=4).GeneticCode == 4


@pytest.fixture(scope="module")
def batches():
    from kaamer_amd import workload
    return gcoderef.make_batches(workload.make_db(1000))


def test_expected_side_reproduces_the_oracle_on_table_11(oracle, batches, monkeypatch):
    """the helper (pyref.get_orfs with the fixture's table swapped in) on table 11 is oracle.get_orfs"""
    for name, seqs in batches.items():
        exp = gcoderef.expected_orfs(monkeypatch, 11, seqs)
        assert exp == [oracle.get_orfs(s) for s in seqs], name
        assert sum(len(e) for e in exp) > (20 if name == "contigs" else 100), name


@pytest.mark.parametrize("code", [c for c in gcoderef.CODES if c != 11])
def test_every_code_changes_every_batch(batches, monkeypatch, code):
    """a kernel that ignores the code cannot pass the GPU tests: each batch's expected ORFs differ from table 11's"""
    for name, seqs in batches.items():
        assert gcoderef.expected_orfs(monkeypatch, code, seqs) != gcoderef.expected_orfs(monkeypatch, 11, seqs), (code, name)
