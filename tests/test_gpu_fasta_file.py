"""kaamer_search_fasta_file (raw FASTA text -> chunks cut at kaamer_text_cut_fasta -> the device reader -> the replicas) and
search.SearchFile(device_fasta=True) against the host reader's route (kaamer_search_file) on the same file."""
import ctypes as C
import gzip

import pytest

from kaamer_amd import abi, api, search, workload

pytestmark = pytest.mark.gpu

N_READS = 3000
ENDINGS = {"lower": b"", "header": b">a header and nothing behind it\n", "blank": b"\n \n\t\r\n\n"}


def _fasta(names, seqs, width):
    out = []
    for n, s in zip(names, seqs):
        out.append(b">" + n + b"\n")
        out.extend(s[i:i + width] + b"\n" for i in range(0, len(s), width))
    return b"".join(out)


def _gz(text, parts=3):
    """several members, split in the middle of lines"""
    cuts = [0] + [len(text) * k // parts + 7 for k in range(1, parts)] + [len(text)]
    return b"".join(gzip.compress(text[a:b], compresslevel=1) for a, b in zip(cuts, cuts[1:]))


@pytest.fixture(scope="module")
def setup(klib, gpu_device, tmp_path_factory):
    db = workload.make_db(2000)
    reads = workload.unpack(workload.make_reads(db, N_READS, seed=41))
    reads[-1], reads[-2] = reads[-1].lower(), reads[-2].lower()
    base = _fasta([b"read %d" % i for i in range(N_READS)], reads, 1 << 20)
    prot = workload.unpack(workload.make_protein_queries(db, 400, seed=43))
    prot[-1], prot[-2] = prot[-1].lower(), prot[-2].lower()
    ptext = _fasta([b"p%d" % i for i in range(len(prot))], prot, 60)
    d = tmp_path_factory.mktemp("fastafile")
    files, texts = {}, {}
    for end, tail in ENDINGS.items():
        texts[end] = base + tail
        files[end, "plain"] = d / ("r_%s.fa" % end)
        files[end, "gz"] = d / ("r_%s.fa.gz" % end)
        files[end, "plain"].write_bytes(texts[end])
        files[end, "gz"].write_bytes(_gz(texts[end]))
    texts["protein"] = ptext
    files["protein", "plain"] = d / "p.fa"
    files["protein", "gz"] = d / "p.fa.gz"
    files["protein", "plain"].write_bytes(ptext)
    files["protein", "gz"].write_bytes(_gz(ptext))
    # a protein file whose last record is lower-case, is in the database, and has a header-only line and blank lines behind
    # it: that header closes the record, so the reader upper-cases it, searches it and reports it
    closed = workload.unpack(db)[5].lower()
    ctext = _fasta([b"p%d" % i for i in range(len(prot))], prot[:-1] + [closed], 60) + b">a header and nothing behind it\n\n \n"
    texts["protein_closed"], texts["closed_seq"] = ctext, closed
    files["protein_closed", "plain"] = d / "pc.fa"
    files["protein_closed", "gz"] = d / "pc.fa.gz"
    files["protein_closed", "plain"].write_bytes(ctext)
    files["protein_closed", "gz"].write_bytes(_gz(ctext))
    reps = api.Replicas.from_image(api.Image.from_proteins(packed=db), [gpu_device, gpu_device])   # two replicas on the one card
    yield dict(reps=reps, files=files, texts=texts, budget=len(base) // 7, pbudget=len(ptext) // 6)
    reps.close()


def _rows(top, first):
    """{global record: [(location, SizeInKmer, ORF, hits) of every reported ORF of it]}"""
    out = {}
    for i in range(top.n_reported):
        m = top.meta[i]
        a, b = int(top.top_off[i]), int(top.top_off[i + 1])
        aa = bytes(top.orf_aa[int(m["aa_off"]):int(m["aa_off"]) + int(m["aa_len"])])
        row = (int(m["start_position"]), int(m["end_position"]), int(m["plus_strand"]), int(m["size_in_kmer"]), aa,
               top.top_pid[a:b].tolist(), top.top_kmatch[a:b].tolist())
        out.setdefault(first + int(m["src_seq"]), []).append(row)
    return out


def _by_record_host(reps, path, **kw):
    names, hits = [], {}

    def on_chunk(first, reads_h, top):
        seqs, offs, size, nm, noff, plus = api._reads_to_arrays(reads_h)
        assert first == len(names)
        names.extend(nm[int(noff[i]):int(noff[i + 1])] for i in range(len(size)))
        hits.update(_rows(top, first))
    ctr = reps.search_file(str(path), "fasta", chunk_seqs=700, on_chunk=on_chunk, **kw)
    return dict(names=names, hits=hits, counters=ctr)


def _by_record_text(reps, path, budget, **kw):
    names, hits, firsts, texts = [], {}, [], []

    def on_chunk(first, text, top):
        firsts.append(first)
        texts.append(text)
        assert first == len(names)                  # input order: every chunk starts where the last one ended
        sp = top.text_spans
        names.extend(text[int(s["name_off"]):int(s["name_off"]) + int(s["name_len"])] for s in sp)
        hits.update(_rows(top, first))
    ctr = reps.search_fasta_file(str(path), chunk_text_bytes=budget, on_chunk=on_chunk, **kw)
    return dict(names=names, hits=hits, firsts=firsts, texts=texts, counters=ctr)


@pytest.mark.parametrize("kind", ["plain", "gz"])
@pytest.mark.parametrize("end", sorted(ENDINGS))
def test_fasta_file_equals_search_file(setup, end, kind):
    reps, path = setup["reps"], setup["files"][end, kind]
    got = _by_record_text(reps, path, setup["budget"], seq_type=abi.READS, in_flight=0 if kind == "plain" else 1)
    want = _by_record_host(reps, setup["files"][end, "plain"], seq_type=abi.READS)
    assert len(want["names"]) == N_READS and sum(len(v) for v in want["hits"].values()) > 300
    assert len(got["firsts"]) >= 5 and got["firsts"] == sorted(got["firsts"])
    assert b"".join(got["texts"]) == setup["texts"][end] and max(len(t) for t in got["texts"]) <= setup["budget"]
    assert all(t[:1] == b">" for t in got["texts"])
    assert got["names"] == want["names"]
    assert got["hits"] == want["hits"]
    for k in ("n_in", "n_queries"):                 # (the other counters depend on how the file was cut into batches)
        assert got["counters"][k] == want["counters"][k]


def test_other_request_forms(setup):
    reps, path = setup["reps"], setup["files"]["lower", "plain"]
    for kw in (dict(seq_type=abi.NUCLEOTIDE), dict(seq_type=abi.seq_type(abi.READS, 4), max_results=3, min_k_match=12)):
        got = _by_record_text(reps, path, setup["budget"], **kw)
        want = _by_record_host(reps, path, **kw)
        assert got["names"] == want["names"] and got["hits"] == want["hits"] and got["counters"]["n_queries"] == want["counters"]["n_queries"]


@pytest.mark.parametrize("kind", ["plain", "gz"])
def test_search_file_driver_protein(setup, kind):
    reps = setup["reps"]
    o = search.SearchOptions(SequenceType=abi.PROTEIN, ChunkSeqs=90, ChunkTextBytes=setup["pbudget"])
    want = list(search.SearchFile(reps, str(setup["files"]["protein", "plain"]), o))
    assert len(want) > 200
    assert sum(qr["Query"]["Sequence"].islower() for qr in want) <= 1      # the file's last record, if it is reported at all
    got = list(search.SearchFile(reps, str(setup["files"]["protein", kind]), o, device_fasta=True))
    assert got == want


@pytest.mark.parametrize("kind", ["plain", "gz"])
@pytest.mark.parametrize("chunks", ["many", "one"])
def test_search_file_driver_protein_last_record_closed_by_a_header(setup, kind, chunks):
    reps = setup["reps"]
    budget = setup["pbudget"] if chunks == "many" else 1 << 24
    o = search.SearchOptions(SequenceType=abi.PROTEIN, ChunkSeqs=90, ChunkTextBytes=budget)
    want = list(search.SearchFile(reps, str(setup["files"]["protein_closed", "plain"]), o))
    closed = setup["texts"]["closed_seq"].decode("latin-1")
    assert want[-1]["Query"]["Name"] == "p399" and want[-1]["Query"]["Sequence"] == closed.upper() != closed
    assert len(want[-1]["SearchResults"]["Hits"]) >= 1
    got = list(search.SearchFile(reps, str(setup["files"]["protein_closed", kind]), o, device_fasta=True))
    assert got == want


def test_search_file_driver_reads_and_contigs(setup):
    reps = setup["reps"]
    for st in (abi.READS, abi.NUCLEOTIDE):
        o = search.SearchOptions(SequenceType=st, ChunkSeqs=900, ChunkTextBytes=setup["budget"])
        want = list(search.SearchFile(reps, str(setup["files"]["header", "plain"]), o, fmt="fasta"))
        assert len(want) > 300
        assert list(search.SearchFile(reps, str(setup["files"]["header", "gz"]), o, device_fasta=True)) == want
    o = search.SearchOptions(SequenceType=abi.READS, ChunkTextBytes=setup["budget"])
    path = str(setup["files"]["lower", "plain"])
    for bad in (dict(options=search.SearchOptions(SequenceType=abi.READS, ExtractPositions=True)),
                dict(options=search.SearchOptions(SequenceType=abi.PROTEIN, Align=True)),
                dict(options=o, fmt="fastq"),
                dict(options=o, device_parse=True)):
        with pytest.raises(ValueError):
            list(search.SearchFile(reps, path, device_fasta=True, **bad))
    # device_parse keeps its meaning and its refusals
    for bad in (dict(options=o, fmt="fasta"), dict(options=search.SearchOptions(SequenceType=abi.PROTEIN))):
        with pytest.raises(ValueError):
            list(search.SearchFile(reps, path, device_parse=True, **bad))
    with pytest.raises(abi.KaamerError) as e:
        reps.search_text_file(path, fmt="fasta")
    assert e.value.code == abi.E_ARG and "host reader" in str(e.value)


def test_a_callback_that_stops_the_run(setup):
    reps, L = setup["reps"], abi.lib()
    calls = []

    def stop_text(user, first, text, length, spans, n, top):
        calls.append(first)
        return 0 if first == 0 else 7
    c = abi.Counters()
    fn = api.Replicas.TEXT_CHUNK_CB(stop_text)
    rc = L.kaamer_search_fasta_file(reps._h, str(setup["files"]["lower", "plain"]).encode(), abi.READS, 0.05, 10, 10, setup["budget"], 0,
                                    C.cast(fn, C.c_void_p), None, C.byref(c))
    assert rc == abi.E_ARG and b"callback" in L.kaamer_last_error()
    assert calls[0] == 0 and 2 <= len(calls) <= 1 + 3 * 2 and calls == sorted(calls)
    with pytest.raises(ZeroDivisionError):
        reps.search_fasta_file(str(setup["files"]["lower", "plain"]), seq_type=abi.READS, chunk_text_bytes=setup["budget"],
                               on_chunk=lambda first, text, top: 1 // 0)
    seen = []
    reps.search_fasta_file(str(setup["files"]["protein", "plain"]), chunk_text_bytes=setup["pbudget"], on_chunk=lambda first, text, top: seen.append(first))
    assert len(seen) >= 5 and seen[0] == 0


def test_refusals_and_a_record_beyond_four_budgets(setup, tmp_path):
    reps = setup["reps"]
    long_rec = tmp_path / "long.fa"
    long_rec.write_bytes(_fasta([b"long"], [b"ACGT" * 2000], 80) + _fasta([b"next"] * 50, [b"ACGTACGT"] * 50, 80))
    with pytest.raises(abi.KaamerError) as e:
        reps.search_fasta_file(str(long_rec), seq_type=abi.NUCLEOTIDE, chunk_text_bytes=1000)
    assert e.value.code == abi.E_CAPACITY and "kaamer_search_file" in str(e.value)
    seen = []
    reps.search_fasta_file(str(long_rec), seq_type=abi.NUCLEOTIDE, chunk_text_bytes=4100,
                           on_chunk=lambda first, text, top: seen.append((first, len(text), len(top.text_spans))))
    assert len(seen) == 2 and seen[0][0] == 0 and seen[1][0] == seen[0][2] and seen[0][2] + seen[1][2] == 51    # the chunk grows within four budgets
    with pytest.raises(abi.KaamerError) as e:
        reps.search_fasta_file(str(tmp_path / "missing.fa"))
    assert e.value.code == abi.E_IO
    with pytest.raises(abi.KaamerError) as e:
        reps.search_fasta_file(str(long_rec), seq_type=5)
    assert e.value.code == abi.E_ARG
    empty = tmp_path / "empty.fa"
    empty.write_bytes(b"")
    bad_gz = tmp_path / "bad.fa.gz"
    bad_gz.write_bytes(b"\x1f\x8b\x08\xff\xff\xff\xff garbage that is no gzip header")
    for p in (empty, bad_gz):                       # no records, no chunk, no error (as kaamer_search_file)
        seen = []
        reps.search_fasta_file(str(p), on_chunk=lambda first, text, top: seen.append(first))
        assert seen == []
