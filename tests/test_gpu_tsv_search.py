"""The text calls with the TSV rows in the result (kaamer_search_text_top_tsv_flat and the FASTA / BGZF forms): the
structured result equals that of the call without rows, the rows equal the restatement of search.go:505-554 (tsvref.py)
and the host formatter on the same result -- FASTQ reads, protein queries and contigs in FASTA, the reads as BGZF, for
the four combinations of ExtractPositions and Annotations, with MinKMatch 1 / MinKRatio 0 so that small Kmatch occur."""
import re
import threading

import pytest

import bgzfmake
import tsvref
from kaamer_amd import abi, api, search, workload

pytestmark = pytest.mark.gpu

FIELDS = ("rep_query", "meta", "trim", "top_off", "top_pid", "top_kmatch", "top_first_pos", "orf_aa")
FLAGS = [(False, False), (False, True), (True, False), (True, True)]
KW = dict(min_k_ratio=0.0, min_k_match=1, max_results=10)


def _fasta(names, seqs, width):
    out = []
    for n, s in zip(names, seqs):
        out.append(b">" + n + b"\n")
        out.extend(s[i:i + width] + b"\n" for i in range(0, len(s), width))
    return b"".join(out)


@pytest.fixture(scope="module")
def setup(klib, gpu_device):
    db = workload.make_db(300)
    seqs = workload.unpack(db)
    rows = [b"EntryID\tSequence\tOrganism\tEC\tNote"]
    for i, s in enumerate(seqs):
        rows.append(b"\t".join([b"sp|P%05d|X%d_TEST" % (i, i % 7), s, b"Organism number %d" % (i % 11), b"" if i % 5 == 0 else b"1.2.%d.-" % i,
                                b"note " * (i % 9)]))
    table = api.Proteins.from_tsv(b"\n".join(rows) + b"\n")
    assert len(table) == 300 and table.ids.tolist() == list(range(300))
    reads = workload.unpack(workload.make_reads(db, 200, seed=33))
    fastq = b"".join(b"@read/%d len=%d\n%s\n+\n%s\n" % (i, len(r), r, b"I" * len(r)) for i, r in enumerate(reads))
    prot = workload.unpack(workload.make_protein_queries(db, 50, seed=31))
    contigs = [b"".join(reads[a:b]) for a, b in ((0, 60), (60, 130), (130, 200))]
    texts = dict(fastq=fastq, protein=_fasta([b"query_%d\tprotein %d" % (i, i) for i in range(50)], prot, 60),
                 contigs=_fasta([b"contig%d  x" % i for i in range(3)], contigs, 70), bgzf=bgzfmake.bgzf_file(fastq, 4096))
    img = table.image()
    ix = api.Index.from_image(img, gpu_device)
    ix.attach_proteins(table)          # (the subject text then shares the alignment table's id map)
    ix.attach_subject_text(table)
    yield dict(ix=ix, img=img, table=table, texts=texts, entries=tsvref.entries_of(table), features=table.feature_names,
               reads=reads, prot=prot, contigs=contigs)
    ix.close()


CASES = {"fastq": abi.READS, "protein": abi.PROTEIN, "contigs": abi.NUCLEOTIDE, "bgzf": abi.READS}


def _call(ix, case, text, tsv):
    if case == "fastq":
        return ix.search_text_top(text, seq_type=CASES[case], tsv=tsv, **KW)
    if case == "bgzf":
        return ix.search_bgzf_top(text, seq_type=CASES[case], tsv=tsv, **KW)
    return ix.search_fasta_top(text, seq_type=CASES[case], tsv=tsv, **KW)


def _same(a, b):
    assert (a.n_queries, a.n_reported, a.max_results) == (b.n_queries, b.n_reported, b.max_results)
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f
    assert a.counters == b.counters


def _check_rows(s, got, text, positions, annotations):
    want, want_off = tsvref.rows_ref(tsvref.queries_of(got, text, got.text_spans, positions), s["entries"], s["features"], positions, annotations)
    assert got.tsv == want
    assert got.tsv_line_off.tolist() == want_off.tolist()
    host, host_off = api.format_tsv(got, text, got.text_spans, s["table"], positions, annotations)
    assert host == got.tsv and host_off.tolist() == want_off.tolist()


@pytest.mark.parametrize("positions,annotations", FLAGS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_rows_of_a_text_call(setup, case, positions, annotations):
    s, ix, text = setup, setup["ix"], setup["texts"][case]
    plain = _call(ix, case, text, None)
    assert plain.tsv is None and plain.tsv_line_off is None
    got = _call(ix, case, text, dict(positions=positions, annotations=annotations))
    _same(got, plain)
    assert got.text_spans.tobytes() == plain.text_spans.tobytes()
    assert got.n_reported >= {"fastq": 100, "bgzf": 100, "protein": 25, "contigs": 30}[case]
    assert len(got.tsv_line_off) == int(got.top_off[-1]) + 1 > got.n_reported
    seqs = dict(fastq=s["reads"], bgzf=s["reads"], protein=s["prot"], contigs=s["contigs"])[case]
    if positions:                                       # the bitmaps are in the result as the _pos call gives them
        pos = ix.search_top(seqs, seq_type=CASES[case], want_positions=True, **KW)
        _same(got, pos)
        for f in ("pos_bits_len", "pos_off", "pos_bits"):
            assert getattr(got, f).tobytes() == getattr(pos, f).tobytes(), f
    else:
        assert got.pos_bits is None
    plain_text = got.text if case == "bgzf" else text
    assert plain_text == setup["texts"]["fastq"] or case not in ("fastq", "bgzf")
    _check_rows(s, got, plain_text, positions, annotations)


def test_whole_response_body(setup):
    s, ix = setup, setup["ix"]
    o = search.SearchOptions(SequenceType=abi.READS, MinKMatch=1, MinKRatio=0.0, ExtractPositions=True, Annotations=True)
    body = search.TextSearchTsv(ix, s["texts"]["fastq"], o)
    head = tsvref.header_ref(True, True, s["features"])
    got = _call(ix, "fastq", s["texts"]["fastq"], dict(positions=True, annotations=True))
    assert body == head + got.tsv and body.count(b"\n") == 1 + int(got.top_off[-1])
    assert search.SearchOptions().Annotations is False
    o = search.SearchOptions(SequenceType=abi.PROTEIN, MinKMatch=1, MinKRatio=0.0)
    body = search.TextSearchTsv(ix, s["texts"]["protein"], o, fmt="fasta")
    assert body.startswith(tsvref.header_ref(False, False, [])) and re.match(rb"query_\d+\tprotein\tsp\|P\d{5}\|", body.split(b"\n")[1])


def test_a_first_bound_too_small(setup, gpu_device):
    """a fresh index whose rows' first bounds are far too small: the device reports what the rows need, the batch is
    repeated from the parsed buffers, the output is that of the index whose bounds fit"""
    s = setup
    ix2 = api.Index.from_image(s["img"], gpu_device)
    try:
        ix2.attach_subject_text(s["table"])         # (an id map of its own: nothing else is attached)
        assert ix2.subject_text_info()["table_bytes"] > s["ix"].subject_text_info()["table_bytes"]
        ix2.set_tsv_bounds(64, 2)
        for case, flags in (("fastq", (True, True)), ("protein", (False, True)), ("bgzf", (True, False))):
            tsv = dict(positions=flags[0], annotations=flags[1])
            want = _call(s["ix"], case, s["texts"][case], tsv)
            ix2.set_tsv_bounds(64, 2)
            got = _call(ix2, case, s["texts"][case], tsv)
            _same(got, want)
            assert got.tsv == want.tsv and got.tsv_line_off.tolist() == want.tsv_line_off.tolist() and len(got.tsv) > 64
            again = _call(ix2, case, s["texts"][case], tsv)      # ... and from the bounds that call left
            assert again.tsv == want.tsv
    finally:
        ix2.close()


def test_no_subject_text_attached(setup, gpu_device):
    s = setup
    ix3 = api.Index.from_image(s["img"], gpu_device)
    try:
        for case in sorted(CASES):
            with pytest.raises(abi.KaamerError) as e:
                _call(ix3, case, s["texts"][case], dict(positions=False, annotations=False))
            assert e.value.code == abi.E_ARG and "kaamer_index_attach_subject_text" in str(e.value)
        with pytest.raises(abi.KaamerError) as e:
            ix3.submit_text_top(s["texts"]["fastq"], tsv=dict(positions=True), **KW)
        assert e.value.code == abi.E_ARG
        assert _call(ix3, "fastq", s["texts"]["fastq"], None).n_reported > 0      # the calls without rows go on working
    finally:
        ix3.close()


def test_four_concurrent_callers(setup):
    s, ix = setup, setup["ix"]
    fastq = s["texts"]["fastq"]
    recs = fastq.split(b"@read/")[1:]
    parts = [b"".join(b"@read/" + r for r in recs[i::4]) for i in range(4)]
    tsv = dict(positions=True, annotations=True)
    want = [ix.search_text_top(p, seq_type=abi.READS, tsv=tsv, **KW) for p in parts]
    assert len({w.tsv for w in want}) == 4
    got, errors = [None] * 4, []

    def work(i):
        try:
            for _ in range(3):
                got[i] = ix.search_text_top(parts[i], seq_type=abi.READS, tsv=tsv, **KW)
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
        _same(g, w)
        assert g.tsv == w.tsv and g.tsv_line_off.tolist() == w.tsv_line_off.tolist()
        _check_rows(s, g, p, True, True)
    # a ticket: submit, then wait
    t = ix.submit_text_top(parts[0], seq_type=abi.READS, tsv=tsv, **KW)
    assert t.wait().tsv == want[0].tsv
    tf = ix.submit_fasta_top(s["texts"]["protein"], seq_type=abi.PROTEIN, tsv=tsv, **KW)
    tb = ix.submit_bgzf_top(s["texts"]["bgzf"], seq_type=abi.READS, tsv=tsv, **KW)
    assert tb.wait().tsv == _call(ix, "fastq", fastq, tsv).tsv
    assert tf.wait().tsv == _call(ix, "protein", s["texts"]["protein"], tsv).tsv
