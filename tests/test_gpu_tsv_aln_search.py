"""The text calls with alignment and the -aln TSV rows in the result (kaamer_search_text_top_aln_tsv_flat and the FASTA /
BGZF forms), end to end on a small table with both attaches: the rows equal kaamer_format_tsv_aln on the same result, the
host formatter on kaamer_search_batch_top_aln_flat over the host-parsed batch, and the restatement of search.go:556-604
(tsvalnref.py); the structured result, alignments included, equals that packed call's.  ~600 FASTQ reads, ~600 protein
queries as 60-column FASTA, the reads as BGZF; MinKMatch 1 / MinKRatio 0 so that weak hits are aligned too."""
import threading

import numpy as np
import pytest

import bgzfmake
import tsvalnref
import tsvref
from kaamer_amd import abi, api, search, workload
from test_gpu_tsv_search import FIELDS, _fasta

pytestmark = pytest.mark.gpu

FLAGS = [(False, False), (False, True), (True, False), (True, True)]
KW = dict(min_k_ratio=0.0, min_k_match=1, max_results=10)
ALIGN = dict(sub_matrix="blosum62", gap_open=11, gap_extend=1)
CASES = {"fastq": abi.READS, "protein": abi.PROTEIN, "bgzf": abi.READS}


@pytest.fixture(scope="module")
def setup(klib, gpu_device):
    db = workload.make_db(300)
    seqs = workload.unpack(db)
    rows = [b"EntryID\tSequence\tOrganism\tEC\tNote"]
    for i, s in enumerate(seqs):
        rows.append(b"\t".join([b"sp|P%05d|X%d_TEST" % (i, i % 7), s, b"Organism number %d" % (i % 11), b"" if i % 5 == 0 else b"1.2.%d.-" % i,
                                b"note " * (i % 9)]))
    table = api.Proteins.from_tsv(b"\n".join(rows) + b"\n")
    reads = workload.unpack(workload.make_reads(db, 600, seed=35))
    fastq = b"".join(b"@read/%d len=%d\n%s\n+\n%s\n" % (i, len(r), r, b"I" * len(r)) for i, r in enumerate(reads))
    prot = workload.unpack(workload.make_protein_queries(db, 600, seed=37))
    texts = dict(fastq=fastq, protein=_fasta([b"query_%d protein %d" % (i, i) for i in range(600)], prot, 60), bgzf=bgzfmake.bgzf_file(fastq, 4096))
    img = table.image()
    ix = api.Index.from_image(img, gpu_device)
    ix.attach_proteins(table)
    ix.attach_subject_text(table)
    yield dict(ix=ix, img=img, table=table, texts=texts, entries=tsvref.entries_of(table), features=table.feature_names,
               seqs=dict(fastq=reads, bgzf=reads, protein=prot))
    ix.close()


def _call(ix, case, text, tsv, align=ALIGN, wait=True):
    kw = dict(seq_type=CASES[case], tsv=tsv, align=align, **KW)
    if case == "fastq":
        return (ix.search_text_top if wait else ix.submit_text_top)(text, **kw)
    if case == "bgzf":
        return (ix.search_bgzf_top if wait else ix.submit_bgzf_top)(text, **kw)
    return (ix.search_fasta_top if wait else ix.submit_fasta_top)(text, **kw)


def _same(a, b, positions):
    assert (a.n_queries, a.n_reported, a.max_results) == (b.n_queries, b.n_reported, b.max_results)
    for f in FIELDS + (("pos_bits_len", "pos_off", "pos_bits") if positions else ()):
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f
    assert a.counters == b.counters
    assert len(a.alignments) == len(b.alignments) == int(a.top_off[-1])
    for x, y in zip(a.alignments, b.alignments):           # bit for bit: NaN compares by its bytes
        assert api.aln_records([x], 1).tobytes() == api.aln_records([y], 1).tobytes()


def _ref_rows(s, got, text, positions, annotations, protein):
    """tsvalnref on the result: its hits are in BitScore order already (the stable sort keeps them)"""
    queries = tsvref.queries_of(got, text, got.text_spans, positions)
    e = 0
    for q in queries:
        for h in q["hits"]:
            h["aln"] = tsvalnref.aln_of(api.aln_records([got.alignments[e]], 1)[0])
            e += 1
    return tsvalnref.rows_ref(queries, s["entries"], s["features"], positions, annotations, protein)


def _check_rows(s, case, got, text, positions, annotations):
    st = CASES[case]
    host, host_off = api.format_tsv(got, text, got.text_spans, s["table"], positions, annotations, align=True, seq_type=st)
    assert got.tsv == host and got.tsv_line_off.tolist() == host_off.tolist()
    want, want_off = _ref_rows(s, got, text, positions, annotations, st == abi.PROTEIN)
    assert got.tsv == want and got.tsv_line_off.tolist() == want_off.tolist()


@pytest.mark.parametrize("positions,annotations", FLAGS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_rows_of_an_aligning_text_call(setup, case, positions, annotations):
    s, ix, text = setup, setup["ix"], setup["texts"][case]
    got = _call(ix, case, text, dict(positions=positions, annotations=annotations))
    assert got.n_reported >= {"fastq": 300, "bgzf": 300, "protein": 300}[case]
    assert len(got.tsv_line_off) == int(got.top_off[-1]) + 1 > got.n_reported
    assert all(a["aln"] is None for a in got.alignments) and any(a["status"] == 0 and a["length"] > 0 for a in got.alignments)
    if not positions:
        assert got.pos_bits is None
    plain_text = got.text if case == "bgzf" else text
    assert case != "bgzf" or plain_text == s["texts"]["fastq"]
    _check_rows(s, case, got, plain_text, positions, annotations)
    # the route a caller had before: the host-parsed batch through the packed call, the rows from the host formatter
    packed = ix.search_top(s["seqs"][case], seq_type=CASES[case], want_positions=positions, align=dict(ALIGN, text=False), **KW)
    _same(got, packed, positions)
    host, host_off = api.format_tsv(packed, plain_text, got.text_spans, s["table"], positions, annotations, align=True, seq_type=CASES[case])
    assert got.tsv == host and got.tsv_line_off.tolist() == host_off.tolist()
    # BitScore descending inside every query
    bits = np.array([a["bitscore"] for a in got.alignments])
    for i in range(got.n_reported):
        b = bits[int(got.top_off[i]):int(got.top_off[i + 1])]
        assert (np.diff(b) <= 0).all()


def test_whole_response_body(setup):
    s, ix = setup, setup["ix"]
    o = search.SearchOptions(SequenceType=abi.PROTEIN, MinKMatch=1, MinKRatio=0.0, Annotations=True, Align=True)
    body = search.TextSearchTsv(ix, s["texts"]["protein"], o, fmt="fasta")
    got = _call(ix, "protein", s["texts"]["protein"], dict(positions=False, annotations=True))
    assert body == tsvalnref.header_ref(False, True, s["features"]) + got.tsv and body.count(b"\n") == 1 + int(got.top_off[-1])


def test_a_first_bound_too_small(setup, gpu_device):
    """a fresh index whose rows' first bounds are far too small: the batch is repeated from the parsed buffers"""
    s = setup
    ix2 = api.Index.from_image(s["img"], gpu_device)
    try:
        ix2.attach_proteins(s["table"])
        ix2.attach_subject_text(s["table"])
        for case, flags in (("fastq", (True, True)), ("protein", (False, True)), ("bgzf", (True, False))):
            tsv = dict(positions=flags[0], annotations=flags[1])
            want = _call(s["ix"], case, s["texts"][case], tsv)
            ix2.set_tsv_bounds(64, 2)
            got = _call(ix2, case, s["texts"][case], tsv)
            _same(got, want, flags[0])
            assert got.tsv == want.tsv and got.tsv_line_off.tolist() == want.tsv_line_off.tolist() and len(got.tsv) > 64
            assert _call(ix2, case, s["texts"][case], tsv).tsv == want.tsv      # ... and from the bounds that call left
    finally:
        ix2.close()


def test_unknown_matrix_prints_zeros(setup):
    """options without a row in AllMatrixScores: status 1 everywhere, the zeros in sortMapByValue order -- the order of the
    call without alignment"""
    s, ix = setup, setup["ix"]
    for case in ("fastq", "protein"):
        text = s["texts"][case]
        got = _call(ix, case, text, dict(positions=True, annotations=True), align=dict(sub_matrix="blosum62", gap_open=3, gap_extend=7))
        plain = _call(ix, case, text, dict(positions=True, annotations=True), align=None)
        assert got.top_pid.tobytes() == plain.top_pid.tobytes() and got.n_reported > 100
        assert all(a["status"] == 1 for a in got.alignments)
        _check_rows(s, case, got, text, True, True)
        for row, prow in zip(got.tsv.split(b"\n")[:-1], plain.tsv.split(b"\n")[:-1]):
            f, pf = row.split(b"\t"), prow.split(b"\t")
            assert f[:2] == pf[:2] and f[2:6] == [b"0.00", b"0", b"0", b"0"] and f[8:12] == [b"0", b"0", b"0.000000e+00", b"0.00"]
            assert f[6:8] == ([b"0", b"0"] if case == "protein" else pf[6:8])
        packed = ix.search_top(s["seqs"][case], seq_type=CASES[case], want_positions=True, align=dict(sub_matrix="blosum62", gap_open=3, gap_extend=7, text=False), **KW)
        _same(got, packed, True)


def test_a_raw_score_outside_the_table_goes_to_the_host(setup, gpu_device):
    """the stages' table cut down to the negative raw scores and a few more: nearly every pair lies outside it, the host
    prints those batches -- the same bytes -- and counts them"""
    s = setup
    ix2 = api.Index.from_image(s["img"], gpu_device)
    try:
        ix2.attach_proteins(s["table"])
        ix2.attach_subject_text(s["table"])
        ix2.set_tsv_aln_raw_count(65536 + 40)
        assert ix2.tsv_aln_info() == dict(host_batches=0, raw_count=65536 + 40)
        for n, case in enumerate(("fastq", "protein", "bgzf")):
            tsv = dict(positions=True, annotations=True)
            want = _call(s["ix"], case, s["texts"][case], tsv)
            assert max(a["raw"] for a in want.alignments) >= 40
            got = _call(ix2, case, s["texts"][case], tsv)
            _same(got, want, True)
            assert got.tsv == want.tsv and got.tsv_line_off.tolist() == want.tsv_line_off.tolist()
            assert ix2.tsv_aln_info()["host_batches"] == n + 1
        assert s["ix"].tsv_aln_info()["host_batches"] == 0
    finally:
        ix2.close()


def test_missing_attaches(setup, gpu_device):
    s = setup
    for attach, missing in (("attach_subject_text", "kaamer_index_attach_proteins"), ("attach_proteins", "kaamer_index_attach_subject_text")):
        ix3 = api.Index.from_image(s["img"], gpu_device)
        try:
            getattr(ix3, attach)(s["table"])
            for case in sorted(CASES):
                for wait in (True, False):
                    with pytest.raises(abi.KaamerError) as e:
                        _call(ix3, case, s["texts"][case], dict(positions=False, annotations=False), wait=wait)
                    assert e.value.code == abi.E_ARG and missing in str(e.value)
        finally:
            ix3.close()


def test_four_concurrent_callers(setup):
    s, ix = setup, setup["ix"]
    fastq = s["texts"]["fastq"]
    recs = fastq.split(b"@read/")[1:]
    parts = [b"".join(b"@read/" + r for r in recs[i::4]) for i in range(4)]
    tsv = dict(positions=True, annotations=True)
    want = [_call(ix, "fastq", p, tsv) for p in parts]
    assert len({w.tsv for w in want}) == 4
    got, errors = [None] * 4, []

    def work(i):
        try:
            for _ in range(3):
                got[i] = _call(ix, "fastq", parts[i], tsv)
                assert got[i].tsv == want[i].tsv
        except Exception as e:   # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for g, w, p in zip(got, want, parts):
        _same(g, w, True)
        _check_rows(s, "fastq", g, p, True, True)
    # tickets: submit, then wait
    tt = _call(ix, "fastq", parts[0], tsv, wait=False)
    tf = _call(ix, "protein", s["texts"]["protein"], tsv, wait=False)
    tb = _call(ix, "bgzf", s["texts"]["bgzf"], tsv, wait=False)
    assert tt.wait().tsv == want[0].tsv
    assert tb.wait().tsv == _call(ix, "fastq", fastq, tsv).tsv
    assert tf.wait().tsv == _call(ix, "protein", s["texts"]["protein"], tsv).tsv
