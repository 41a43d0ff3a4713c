"""kaamer_search_text_file (raw FASTQ text -> chunks -> the device reader -> the replicas) against kaamer_search_file (the
host reader) on the same file: per record of the file the same names and the same reported hits."""
import ctypes as C
import gzip

import numpy as np
import pytest

from kaamer_amd import abi, api, search, workload

pytestmark = pytest.mark.gpu

N_READS = 5000


@pytest.fixture(scope="module")
def setup(klib, gpu_device, tmp_path_factory):
    db = workload.make_db(1000)
    reads = workload.make_reads(db, N_READS, seed=23)
    text = bytes(workload.fastq_text(reads))
    d = tmp_path_factory.mktemp("textfile")
    plain, gz = d / "q.fastq", d / "q.fastq.gz"
    plain.write_bytes(text)
    half = api.text_cut_fastq(text[:len(text) // 2 + 37]) - 11       # two members, split in the middle of a line
    gz.write_bytes(gzip.compress(text[:half], compresslevel=1) + gzip.compress(text[half:], compresslevel=1))
    reps = api.Replicas.from_image(api.Image.from_proteins(packed=db), [gpu_device, gpu_device])   # two replicas on the one card
    want = _by_record_host(reps, plain)
    assert len(want["names"]) == N_READS and sum(len(v) for v in want["hits"].values()) > 500
    yield dict(reps=reps, text=text, plain=plain, gz=gz, want=want, budget=len(text) // 7)
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
    names, hits, firsts = [], {}, []

    def on_chunk(first, reads_h, top):
        seqs, offs, size, nm, noff, plus = api._reads_to_arrays(reads_h)
        firsts.append(first)
        assert first == len(names)
        names.extend(nm[int(noff[i]):int(noff[i + 1])] for i in range(len(size)))
        hits.update(_rows(top, first))
    ctr = reps.search_file(str(path), "fastq", chunk_seqs=700, on_chunk=on_chunk, **kw)
    return dict(names=names, hits=hits, firsts=firsts, counters=ctr)


def _by_record_text(reps, path, budget, **kw):
    names, hits, firsts, sizes = [], {}, [], []

    def on_chunk(first, text, top):
        firsts.append(first)
        sizes.append(len(text))
        assert first == len(names)                  # input order: every chunk starts where the last one ended
        assert text[:1] == b"@"
        sp = top.text_spans
        names.extend(text[int(s["name_off"]):int(s["name_off"]) + int(s["name_len"])] for s in sp)
        hits.update(_rows(top, first))
    ctr = reps.search_text_file(str(path), "fastq", chunk_text_bytes=budget, on_chunk=on_chunk, **kw)
    return dict(names=names, hits=hits, firsts=firsts, sizes=sizes, counters=ctr)


@pytest.mark.parametrize("kind", ["plain", "gz"])
@pytest.mark.parametrize("in_flight", [0, 1])
def test_text_file_equals_search_file(setup, kind, in_flight):
    got = _by_record_text(setup["reps"], setup[kind], setup["budget"], in_flight=in_flight)
    want = setup["want"]
    assert len(got["firsts"]) >= 5 and got["firsts"] == sorted(got["firsts"])
    assert sum(got["sizes"]) == len(setup["text"]) and max(got["sizes"]) <= setup["budget"]
    assert got["names"] == want["names"]
    assert got["hits"] == want["hits"]
    for k in ("n_in", "n_queries"):                 # (the other counters depend on how the file was cut into batches)
        assert got["counters"][k] == want["counters"][k]


def test_other_request_forms(setup):
    reps = setup["reps"]
    for kw in (dict(seq_type=abi.NUCLEOTIDE), dict(seq_type=abi.seq_type(abi.READS, 4), max_results=3, min_k_match=12)):
        got = _by_record_text(reps, setup["plain"], setup["budget"], **kw)
        want = _by_record_host(reps, setup["plain"], **kw)
        assert got["names"] == want["names"] and got["hits"] == want["hits"] and got["counters"]["n_queries"] == want["counters"]["n_queries"]


def test_a_callback_that_stops_the_run(setup):
    reps, L = setup["reps"], abi.lib()
    calls = []

    def stop_host(user, first, reads, top):
        calls.append(("host", first))
        return 1

    def stop_text(user, first, text, length, spans, n, top):
        calls.append(("text", first))
        return 0 if first == 0 else 7
    c = abi.Counters()
    f1 = api.Replicas.CHUNK_CB(stop_host)
    rc_host = L.kaamer_search_file(reps._h, str(setup["plain"]).encode(), 1, 0, abi.READS, 0.05, 10, 10, 700, 1 << 28, 0, C.cast(f1, C.c_void_p), None,
                                   C.byref(c))
    msg_host = L.kaamer_last_error()
    f2 = api.Replicas.TEXT_CHUNK_CB(stop_text)
    rc_text = L.kaamer_search_text_file(reps._h, str(setup["plain"]).encode(), 1, abi.READS, 0.05, 10, 10, setup["budget"], 0, C.cast(f2, C.c_void_p),
                                        None, C.byref(c))
    msg_text = L.kaamer_last_error()
    assert rc_text == rc_host == abi.E_ARG and msg_text == msg_host and b"callback" in msg_text
    # (both drivers drain the chunks in flight after the stop: their callbacks may still run, in order)
    assert [c for c in calls if c[0] == "host"][0] == ("host", 0)
    text_calls = [c[1] for c in calls if c[0] == "text"]
    assert text_calls[0] == 0 and 2 <= len(text_calls) <= 1 + 3 * 2 and text_calls == sorted(text_calls)
    # a Python exception in on_chunk comes out as itself, and the set is usable afterwards
    with pytest.raises(ZeroDivisionError):
        reps.search_text_file(str(setup["plain"]), chunk_text_bytes=setup["budget"], on_chunk=lambda first, text, top: 1 // 0)
    got = _by_record_text(reps, setup["plain"], setup["budget"])
    assert got["hits"] == setup["want"]["hits"]


def test_refusals_and_a_record_beyond_four_budgets(setup, tmp_path):
    reps = setup["reps"]
    long_read = tmp_path / "long.fastq"
    long_read.write_bytes(b"@long\n" + b"ACGT" * 2000 + b"\n+\n" + b"I" * 8000 + b"\n" + b"@next\nACGT\n+\nIIII\n" * 50)
    with pytest.raises(abi.KaamerError) as e:
        reps.search_text_file(str(long_read), chunk_text_bytes=1000)
    assert e.value.code == abi.E_CAPACITY and "kaamer_search_file" in str(e.value)
    seen = []
    reps.search_text_file(str(long_read), chunk_text_bytes=4100, on_chunk=lambda first, text, top: seen.append((first, len(text))))
    assert seen == [(0, 16388), (22, 522)]          # found within four budgets: the chunk grows, the next one is the tail
    with pytest.raises(abi.KaamerError) as e:
        reps.search_text_file(str(setup["plain"]), fmt="fasta")
    assert e.value.code == abi.E_ARG and "host reader" in str(e.value)
    with pytest.raises(abi.KaamerError) as e:
        reps.search_text_file(str(setup["plain"]), seq_type=abi.PROTEIN)
    assert e.value.code == abi.E_ARG
    with pytest.raises(abi.KaamerError) as e:
        reps.search_text_file(str(tmp_path / "missing.fastq"))
    assert e.value.code == abi.E_IO
    empty = tmp_path / "empty.fastq"
    empty.write_bytes(b"")
    bad_gz = tmp_path / "bad.fastq.gz"
    bad_gz.write_bytes(b"\x1f\x8b\x08\xff\xff\xff\xff garbage that is no gzip header")
    for p in (empty, bad_gz):                       # no records, no chunk, no error (as kaamer_search_file)
        seen = []
        reps.search_text_file(str(p), on_chunk=lambda first, text, top: seen.append(first))
        assert seen == []


def test_search_file_driver_with_device_parse(setup):
    reps = setup["reps"]
    o = search.SearchOptions(SequenceType=abi.READS, ChunkSeqs=900, ChunkTextBytes=setup["budget"])
    want = list(search.SearchFile(reps, str(setup["plain"]), o))
    assert len(want) > 500
    assert list(search.SearchFile(reps, str(setup["plain"]), o, device_parse=True)) == want
    assert list(search.SearchFile(reps, str(setup["gz"]), o, device_parse=True)) == want
    for bad in (dict(options=search.SearchOptions(SequenceType=abi.READS, ExtractPositions=True)),
                dict(options=search.SearchOptions(SequenceType=abi.READS, Align=True)),
                dict(options=search.SearchOptions(SequenceType=abi.PROTEIN)),
                dict(options=o, fmt="fasta")):
        with pytest.raises(ValueError):
            list(search.SearchFile(reps, str(setup["plain"]), device_parse=True, **bad))
