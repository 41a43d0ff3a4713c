"""The text calls with the JSON objects in the result (kaamer_search_text_top_json_flat and the FASTA / BGZF forms): the
structured result equals that of the call without objects (and, with bitmaps, that of the packed _pos call), the objects
equal the host formatter on the same result and the restatement of encoding/json's rules (jsonref.py) -- protein queries in
multi-line FASTA with crafted names, FASTQ reads, the reads as BGZF, and a FASTA contig with an ORF whose start codon moves
by more than 64 residues -- with MinKMatch 1 / MinKRatio 0 so that small Kmatch occur."""
import json
import threading

import pytest

import bgzfmake
import jsonref
from kaamer_amd import abi, api, search, workload

pytestmark = pytest.mark.gpu

FIELDS = ("rep_query", "meta", "trim", "top_off", "top_pid", "top_kmatch", "top_first_pos", "orf_aa")
KW = dict(min_k_ratio=0.0, min_k_match=1, max_results=10)
CODON = {b"A": b"GCT", b"C": b"TGT", b"D": b"GAT", b"E": b"GAA", b"F": b"TTT", b"G": b"GGT", b"H": b"CAT", b"I": b"ATT", b"K": b"AAA", b"L": b"CTT",
         b"M": b"ATG", b"N": b"AAT", b"P": b"CCT", b"Q": b"CAA", b"R": b"CGT", b"S": b"TCT", b"T": b"ACT", b"V": b"GTT", b"W": b"TGG", b"Y": b"TAT"}


def _fasta(names, seqs, width):
    out = []
    for n, s in zip(names, seqs):
        out.append(b">" + n + b"\n")
        out.extend(s[i:i + width] + b"\n" for i in range(0, len(s), width))
    return b"".join(out)


def _dna(residues):
    return b"".join(CODON[residues[i:i + 1]] for i in range(len(residues)))


@pytest.fixture(scope="module")
def setup(klib, gpu_device):
    db = workload.make_db(300)
    seqs = workload.unpack(db)
    rows = [b"EntryID\tSequence\tOrganism\tEC\tNote"]
    for i, s in enumerate(seqs):
        rows.append(b"\t".join([b"sp|P%05d|X%d_TEST" % (i, i % 7), s, b"Organism <%d> & \"co\"" % (i % 11), b"" if i % 5 == 0 else b"1.2.%d.-" % i,
                                b"note " * (i % 9)]))
    table = api.Proteins.from_tsv(b"\n".join(rows) + b"\n")
    entries = {i: dict(entry_id=r.split(b"\t")[0], sequence=r.split(b"\t")[1], length=len(r.split(b"\t")[1]),
                       features=list(zip([b"Organism", b"EC", b"Note"], r.split(b"\t")[2:]))) for i, r in enumerate(rows[1:])}
    reads = workload.unpack(workload.make_reads(db, 300, seed=33))
    rnames = [b"read/%d len=%d" % (i, len(r)) for i, r in enumerate(reads)]
    rnames[3], rnames[4], rnames[5] = b"", b'q"uote \\ <&> \xc3\xa9 \xe2\x80\xa8', b"bad \xff\xc0\x80 utf8\t tab"
    fastq = b"".join(b"@%s\n%s\n+\n%s\n" % (n, r, b"I" * len(r)) for n, r in zip(rnames, reads))
    prot = workload.unpack(workload.make_protein_queries(db, 40, seed=31))
    pnames = [b"query_%d\tprotein %d" % (i, i) for i in range(40)]
    pnames[1], pnames[2], pnames[7] = b'say "hi" \\ <b>&amp;</b>', b"\xe2\x82\xac \xf0\x9f\x98\x80 \xe2\x80\xa9 \xed\xa0\x80 \x01\x7f", b""
    written = list(prot)
    written[-2], written[-1] = prot[-2].lower(), prot[-1].lower()   # (every record but the last is upper-cased by the reader)
    searched = list(prot)
    searched[-1] = prot[-1].lower()
    # a contig whose ORF opens with 75 residues that hit nothing, then a start codon and a database protein: the best start
    # codon lies 76 residues in
    subject = max(seqs[:50], key=len)[:120]
    orf = b"M" + b"ACDEFGHIKLNPQRS" * 5 + b"M" + subject
    contig = b"TAA" + _dna(orf) + b"TAA" + reads[0] + reads[1]
    texts = dict(fastq=fastq, protein=_fasta(pnames, written, 60), contigs=_fasta([b"contig one  x", b"c2"], [contig, b"".join(reads[2:40])], 70),
                 bgzf=bgzfmake.bgzf_file(fastq, 4096))
    img = table.image()
    ix = api.Index.from_image(img, gpu_device)
    ix.attach_subject_text(table)
    ix.attach_subject_json(table)      # (shares the subject text's id map)
    yield dict(ix=ix, img=img, table=table, texts=texts, entries=entries, features=table.feature_names, reads=reads, prot=searched,
               contigs=[contig, b"".join(reads[2:40])])
    ix.close()


CASES = {"fastq": abi.READS, "protein": abi.PROTEIN, "contigs": abi.NUCLEOTIDE, "bgzf": abi.READS}
FMT = {"fastq": 1, "bgzf": 1, "protein": 0, "contigs": 0}


def _call(ix, case, text, js, submit=False):
    if case == "fastq":
        return (ix.submit_text_top if submit else ix.search_text_top)(text, seq_type=CASES[case], json=js, **KW)
    if case == "bgzf":
        return (ix.submit_bgzf_top if submit else ix.search_bgzf_top)(text, seq_type=CASES[case], json=js, **KW)
    return (ix.submit_fasta_top if submit else ix.search_fasta_top)(text, seq_type=CASES[case], json=js, **KW)


def _same(a, b):
    assert (a.n_queries, a.n_reported, a.max_results) == (b.n_queries, b.n_reported, b.max_results)
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f
    assert a.counters == b.counters


def _ref_queries(got, text, seqs, protein, bitmaps):
    """the reported queries of a structured result as jsonref.objects takes them"""
    out = []
    for i in range(got.n_reported):
        m, sp = got.meta[i], got.text_spans[int(got.meta[i]["src_seq"])]
        name = text[int(sp["name_off"]):int(sp["name_off"]) + int(sp["name_len"])]
        seq = seqs[int(m["src_seq"])] if protein else got.orf_aa[int(m["aa_off"]):int(m["aa_off"]) + int(m["aa_len"])].tobytes()
        pos = got.positions(i) if bitmaps else {}
        hits = [dict(key=int(got.top_pid[e]), kmatch=int(got.top_kmatch[e]), bits=[bool(b) for b in pos.get(int(got.top_pid[e]), [])])
                for e in range(int(got.top_off[i]), int(got.top_off[i + 1]))]
        out.append(dict(name=name, sequence=seq, size_in_kmer=int(m["size_in_kmer"]), start=int(m["start_position"]), end=int(m["end_position"]),
                        plus=bool(m["plus_strand"]), trim=int(got.trim[i]), hits=hits))
    return out


def _check_objects(s, got, case, text, positions):
    protein = CASES[case] == abi.PROTEIN
    bitmaps = positions or not protein
    seqs = s["prot"] if protein else None
    packed = api.pack_sequences(seqs) if protein else (None, None)
    host, host_off = api.format_json(got, text, got.text_spans, s["table"], seqs=packed[0], offsets=packed[1], seq_type=CASES[case], text_format=FMT[case],
                                     positions=positions)
    assert got.json == host and got.json_obj_off.tolist() == host_off.tolist()
    want, want_off = jsonref.objects(_ref_queries(got, text, seqs, protein, bitmaps), s["entries"], protein, FMT[case], positions)
    assert got.json == want and got.json_obj_off.tolist() == want_off
    assert got.tsv is None


@pytest.mark.parametrize("positions", [False, True])
@pytest.mark.parametrize("case", sorted(CASES))
def test_objects_of_a_text_call(setup, case, positions):
    s, ix, text = setup, setup["ix"], setup["texts"][case]
    plain = _call(ix, case, text, None)
    assert plain.json is None and plain.json_obj_off is None
    got = _call(ix, case, text, dict(positions=positions))
    _same(got, plain)
    assert got.text_spans.tobytes() == plain.text_spans.tobytes()
    assert got.n_reported >= {"fastq": 150, "bgzf": 150, "protein": 25, "contigs": 5}[case]
    assert len(got.json_obj_off) == got.n_reported + 1
    seqs = dict(fastq=s["reads"], bgzf=s["reads"], protein=s["prot"], contigs=s["contigs"])[case]
    if positions or CASES[case] != abi.PROTEIN:          # the bitmaps are in the result as the _pos call gives them
        pos = ix.search_top(seqs, seq_type=CASES[case], want_positions=True, **KW)
        _same(got, pos)
        for f in ("pos_bits_len", "pos_off", "pos_bits"):
            assert getattr(got, f).tobytes() == getattr(pos, f).tobytes(), f
    else:
        assert got.pos_bits is None
    if case == "contigs":
        assert int(got.trim.max()) > 64                  # the bit origin of that ORF's bitmaps is off the word boundary
    _check_objects(s, got, case, got.text if case == "bgzf" else text, positions)


def test_whole_response_body(setup):
    s, ix = setup, setup["ix"]
    o = search.SearchOptions(SequenceType=abi.PROTEIN, MinKMatch=1, MinKRatio=0.0, ExtractPositions=True, Annotations=True)
    body = search.TextSearchJson(ix, s["texts"]["protein"], o, fmt="fasta", proteins=s["table"])
    got = _call(ix, "protein", s["texts"]["protein"], dict(positions=True))
    assert body == jsonref.header(s["features"], True) + got.json + jsonref.trailer()
    o = search.SearchOptions(SequenceType=abi.NUCLEOTIDE, MinKMatch=1, MinKRatio=0.0)
    doc = json.loads(search.TextSearchJson(ix, s["texts"]["contigs"], o, fmt="fasta"))   # (these names are valid UTF-8)
    plain = _call(ix, "contigs", s["texts"]["contigs"], None)
    assert doc["dbProteinFeatures"] == [] and len(doc["results"]) == plain.n_reported
    for i, obj in enumerate(doc["results"]):
        assert obj["Query"]["Contig"] == obj["Query"]["Name"] and obj["Query"]["Type"] == "DNA Query"
        assert obj["Query"]["SizeInKmer"] == int(plain.meta[i]["size_in_kmer"]) and obj["Query"]["Location"]["StartPosition"] == int(plain.meta[i]["start_position"])
        hits = [(h["Key"], h["Kmatch"]) for h in obj["SearchResults"]["Hits"]]
        assert hits == list(zip(plain.top_pid[int(plain.top_off[i]):int(plain.top_off[i + 1])].tolist(),
                                plain.top_kmatch[int(plain.top_off[i]):int(plain.top_off[i + 1])].tolist()))
        assert sorted(obj["HitEntries"]) == sorted(str(k) for k, _ in hits) == sorted(obj["SearchResults"]["PositionHits"])
        assert all(len(v) == obj["Query"]["SizeInKmer"] for v in obj["SearchResults"]["PositionHits"].values())


def test_a_first_bound_too_small(setup, gpu_device):
    """a fresh index whose objects' first bounds are far too small: the device reports what they need, the batch is repeated
    from the parsed buffers, the output is that of the index whose bounds fit"""
    s = setup
    ix2 = api.Index.from_image(s["img"], gpu_device)
    try:
        ix2.attach_subject_json(s["table"])         # (an id map of its own: nothing else is attached)
        assert ix2.subject_json_info()["table_bytes"] > s["ix"].subject_json_info()["table_bytes"]
        for case, positions in (("fastq", False), ("protein", True), ("bgzf", False), ("contigs", False)):
            js = dict(positions=positions)
            want = _call(s["ix"], case, s["texts"][case], js)
            ix2.set_json_bounds(64, 2)
            got = _call(ix2, case, s["texts"][case], js)
            _same(got, want)
            assert got.json == want.json and got.json_obj_off.tolist() == want.json_obj_off.tolist() and len(got.json) > 64
            again = _call(ix2, case, s["texts"][case], js)      # ... and from the bounds that call left
            assert again.json == want.json
    finally:
        ix2.close()


def test_no_subject_json_attached(setup, gpu_device):
    s = setup
    ix3 = api.Index.from_image(s["img"], gpu_device)
    try:
        ix3.attach_subject_text(s["table"])
        for case in sorted(CASES):
            with pytest.raises(abi.KaamerError) as e:
                _call(ix3, case, s["texts"][case], dict(positions=False))
            assert e.value.code == abi.E_ARG and "kaamer_index_attach_subject_json" in str(e.value)
        with pytest.raises(abi.KaamerError) as e:
            _call(ix3, "fastq", s["texts"]["fastq"], dict(positions=True), submit=True)
        assert e.value.code == abi.E_ARG
        assert _call(ix3, "fastq", s["texts"]["fastq"], None).n_reported > 0      # the calls without objects go on working
    finally:
        ix3.close()


def test_four_concurrent_callers(setup):
    s, ix = setup, setup["ix"]
    fastq = s["texts"]["fastq"]
    recs = fastq.split(b"\n@")
    recs = [recs[0]] + [b"@" + r for r in recs[1:]]
    parts = [b"\n".join(recs[i::4]) + (b"\n" if not recs[i::4][-1].endswith(b"\n") else b"") for i in range(4)]
    js = dict(positions=False)
    want = [ix.search_text_top(p, seq_type=abi.READS, json=js, **KW) for p in parts]
    assert len({w.json for w in want}) == 4
    got, errors = [None] * 4, []

    def work(i):
        try:
            for _ in range(3):
                got[i] = ix.search_text_top(parts[i], seq_type=abi.READS, json=js, **KW)
                assert got[i].json == want[i].json
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
        assert g.json == w.json and g.json_obj_off.tolist() == w.json_obj_off.tolist()
        _check_objects(s, g, "fastq", p, False)
    # a ticket: submit, then wait
    t = _call(ix, "fastq", parts[0], js, submit=True)
    assert t.wait().json == want[0].json
    tf = _call(ix, "protein", s["texts"]["protein"], dict(positions=True), submit=True)
    tb = _call(ix, "bgzf", s["texts"]["bgzf"], js, submit=True)
    assert tb.wait().json == _call(ix, "fastq", fastq, js).json
    assert tf.wait().json == _call(ix, "protein", s["texts"]["protein"], dict(positions=True)).json
