"""kaamer_search_bgzf_top_flat (BGZF bytes in: inflated, parsed and searched on the device) against
kaamer_search_text_top_flat of the same text inflated on the host: field for field the same result, plus the inflated text.
Bytes that are not whole BGZF blocks are refused, a block that does not inflate is KAAMER_E_FORMAT naming it, and the text
call keeps refusing gzip bytes."""
import gzip
import threading

import numpy as np
import pytest

import bgzfmake
from kaamer_amd import abi, api, workload

pytestmark = pytest.mark.gpu

N_READS = 2000
FIELDS = ("rep_query", "meta", "trim", "top_off", "top_pid", "top_kmatch", "top_first_pos", "orf_aa", "text_spans", "top_cnt")


@pytest.fixture(scope="module")
def setup(klib, gpu_device):
    db = workload.make_db(1000)
    reads = workload.make_reads(db, N_READS, seed=23)
    text = bytes(workload.fastq_text(reads))
    ix = api.Index.from_image(api.Image.from_proteins(packed=db), gpu_device)
    want = ix.search_text_top(text)
    assert want.n_queries > 0 and want.n_reported > 200 and len(want.text_spans) == N_READS and want.text is None
    yield dict(ix=ix, text=text, want=want)
    ix.close()


def _same(got, want):
    assert (got.n_queries, got.n_reported, got.max_results) == (want.n_queries, want.n_reported, want.max_results)
    for f in FIELDS:
        assert np.array_equal(getattr(got, f), getattr(want, f)), f
    for k in ("n_in", "n_queries", "n_hits"):
        assert got.counters[k] == want.counters[k]


@pytest.mark.parametrize("block_bytes,mode", [(700, "level6"), (701, "level1"), (65280, "level6"), (65280, "level9_mem1")])
def test_bgzf_top_equals_text_top(setup, block_bytes, mode):
    """~700-byte blocks: records straddle most block boundaries, several hundred blocks per call; and full-size blocks"""
    data = bgzfmake.bgzf_file(setup["text"], block_bytes, mode)
    assert gzip.decompress(data) == setup["text"]
    got = setup["ix"].search_bgzf_top(data)
    assert got.text == setup["text"]
    _same(got, setup["want"])


def test_other_request_forms_and_empty_input(setup):
    ix, text = setup["ix"], setup["text"][:60000]
    data = bgzfmake.bgzf_file(text, 3000, eof=False)
    for kw in (dict(seq_type=abi.NUCLEOTIDE), dict(seq_type=abi.seq_type(abi.READS, 4), max_results=3, min_k_match=12)):
        got = ix.search_bgzf_top(data, **kw)
        assert got.text == text
        _same(got, ix.search_text_top(text, **kw))
    for data in (b"", bgzfmake.EOF_BLOCK, bgzfmake.EOF_BLOCK * 3):
        got = ix.search_bgzf_top(data)
        assert got.n_queries == 0 and got.n_reported == 0 and len(got.text_spans) == 0 and (got.text or b"") == b""


def test_submit_wait_from_several_callers(setup):
    ix = setup["ix"]
    data = bgzfmake.bgzf_file(setup["text"], 4000)
    tickets = [ix.submit_bgzf_top(data) for _ in range(3)]
    for t in tickets:
        got = t.wait()
        assert got.text == setup["text"]
        _same(got, setup["want"])
    results = [None] * 4

    def call(i):
        results[i] = ix.search_bgzf_top(data)
    threads = [threading.Thread(target=call, args=(i,)) for i in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for got in results:
        _same(got, setup["want"])


def test_what_is_refused(setup):
    ix, text = setup["ix"], setup["text"]
    good = bgzfmake.bgzf_file(text[:30000], 700)
    blocks, _ = api.bgzf_scan(good)

    def refused(data, code, *words):
        with pytest.raises(abi.KaamerError) as e:
            ix.search_bgzf_top(data)
        assert e.value.code == code
        for w in words:
            assert w in str(e.value), str(e.value)

    refused(gzip.compress(text[:5000]), abi.E_ARG)                                   # ordinary gzip
    refused(good + gzip.compress(text[:5000]), abi.E_ARG)                            # BGZF followed by an ordinary member
    refused(good[:-5], abi.E_ARG)                                                    # cut short inside a block
    refused(text[:5000], abi.E_ARG)                                                  # plain text
    b = 20
    at = int(blocks[b]["comp_off"]) + int(blocks[b]["comp_len"])                     # block 20's trailer
    bad = bytearray(good)
    bad[at] ^= 0x10
    refused(bytes(bad), abi.E_FORMAT, "block 20", "status 7")                        # a flipped bit of its CRC
    bad = bytearray(good)
    bad[int(blocks[b]["comp_off"]) + int(blocks[b]["comp_len"]) // 2] ^= 0x04        # ... of its payload
    refused(bytes(bad), abi.E_FORMAT, "block 20")
    got = ix.search_bgzf_top(good)                                                   # the slot is as good as new
    assert got.text == text[:30000]
    _same(got, ix.search_text_top(text[:30000]))
    # the text call keeps refusing gzip bytes, BGZF included
    for data in (good, gzip.compress(text[:5000])):
        with pytest.raises(abi.KaamerError) as e:
            ix.search_text_top(data)
        assert e.value.code == abi.E_ARG


# ---- the file form: kaamer_search_text_file_opts(device_inflate = 1) against the flag-0 run ------------------------------
@pytest.fixture(scope="module")
def files(setup, gpu_device, tmp_path_factory):
    text = setup["text"]
    d = tmp_path_factory.mktemp("bgzffile")
    small = bgzfmake.bgzf_file(text, 700)                                        # records straddle most block boundaries
    blocks, _ = api.bgzf_scan(small)
    mid = len(blocks) // 2
    out = {}

    def put(name, data):
        (d / name).write_bytes(data)
        out[name] = d / name

    put("small", small)
    put("full", bgzfmake.bgzf_file(text, 65280, "level1"))
    put("no_eof", bgzfmake.bgzf_file(text, 700, eof=False))
    half = len(text) // 2 + 11
    put("two_member_gzip", gzip.compress(text[:half]) + gzip.compress(text[half:]))
    put("bgzf_then_gzip", bgzfmake.bgzf_file(text[:half], 700, eof=False) + gzip.compress(text[half:]))
    bad = bytearray(small)
    bad[int(blocks[mid]["comp_off"]) + int(blocks[mid]["comp_len"]) // 2] ^= 0x04
    put("payload_flipped", bytes(bad))
    bad = bytearray(small)
    bad[int(blocks[mid]["comp_off"]) + int(blocks[mid]["comp_len"])] ^= 0x10
    put("crc_flipped", bytes(bad))
    put("truncated", small[:int(blocks[mid]["comp_off"]) + int(blocks[mid]["comp_len"]) // 2])
    put("plain", text)
    img = api.Image.from_proteins(packed=workload.make_db(1000))
    reps = {1: api.Replicas.from_image(img, [gpu_device]), 2: api.Replicas.from_image(img, [gpu_device, gpu_device])}
    yield dict(paths=out, reps=reps, budget=len(text) // 7, flag0={})
    for r in reps.values():
        r.close()


def _run_file(reps, path, budget, **kw):
    texts, names, hits, firsts = [], [], {}, []

    def on_chunk(first, text, top):
        assert first == len(names)                      # input order
        firsts.append(first)
        texts.append(text)
        sp = top.text_spans
        names.extend(text[int(s["name_off"]):int(s["name_off"]) + int(s["name_len"])] for s in sp)
        for i in range(top.n_reported):
            m = top.meta[i]
            a, b = int(top.top_off[i]), int(top.top_off[i + 1])
            aa = bytes(top.orf_aa[int(m["aa_off"]):int(m["aa_off"]) + int(m["aa_len"])])
            hits.setdefault(first + int(m["src_seq"]), []).append(
                (int(m["start_position"]), int(m["end_position"]), int(m["plus_strand"]), int(m["size_in_kmer"]), aa,
                 top.top_pid[a:b].tolist(), top.top_kmatch[a:b].tolist()))
    ctr = reps.search_text_file(str(path), "fastq", chunk_text_bytes=budget, on_chunk=on_chunk, **kw)
    return dict(texts=texts, names=names, hits=hits, counters=ctr)


def _flag0(files, name):
    if name not in files["flag0"]:
        files["flag0"][name] = _run_file(files["reps"][1], files["paths"][name], files["budget"])
    return files["flag0"][name]


def _check_against_flag0(files, name, n_replicas, in_flight, min_chunks=1):
    want = _flag0(files, name)
    got = _run_file(files["reps"][n_replicas], files["paths"][name], files["budget"], in_flight=in_flight, device_inflate=True)
    assert b"".join(got["texts"]) == b"".join(want["texts"])            # byte for byte what the flag-0 run's callbacks saw
    assert got["names"] == want["names"]                                # records per first_seq + i
    assert got["hits"] == want["hits"]                                  # ... and their reported hits
    assert len(got["texts"]) >= min_chunks
    for t in got["texts"][1:]:                                          # every chunk but the last is followed by one that begins with '@'
        assert t[:1] == b"@"
    for k in ("n_in", "n_queries"):
        assert got["counters"][k] == want["counters"][k]
    return got


@pytest.mark.parametrize("n_replicas", [1, 2])
@pytest.mark.parametrize("in_flight", [1, 3])
@pytest.mark.parametrize("name", ["small", "full"])
def test_file_device_inflate_equals_flag0(setup, files, name, in_flight, n_replicas):
    got = _check_against_flag0(files, name, n_replicas, in_flight, min_chunks=5)
    assert b"".join(got["texts"]) == setup["text"] and len(got["names"]) == N_READS


@pytest.mark.parametrize("name", ["two_member_gzip", "bgzf_then_gzip", "payload_flipped", "crc_flipped", "truncated", "no_eof", "plain"])
def test_file_fallback_equals_flag0(setup, files, name):
    """whatever a gzip file holds, the host inflater takes over where the device route ends: text and hits of the flag-0 run"""
    got = _check_against_flag0(files, name, 2, 3)
    if name in ("two_member_gzip", "bgzf_then_gzip", "no_eof", "plain"):
        assert b"".join(got["texts"]) == setup["text"]
    else:                                                               # zlib's text ends in the damaged block
        assert 0 < len(b"".join(got["texts"])) < len(setup["text"])


def test_file_chunk_without_a_cut(setup, files, tmp_path):
    """a record longer than four budgets: today's KAAMER_E_CAPACITY; one that four budgets hold goes through"""
    long_read = b"@long\n" + b"A" * 8000 + b"\n+\n" + b"I" * 8000 + b"\n@next\nACGT\n+\nIIII\n@z\nAC\n"
    p = tmp_path / "long.gz"
    p.write_bytes(bgzfmake.bgzf_file(long_read, 300))
    for flag in (False, True):
        with pytest.raises(abi.KaamerError) as e:
            files["reps"][1].search_text_file(str(p), "fastq", chunk_text_bytes=1000, device_inflate=flag)
        assert e.value.code == abi.E_CAPACITY and "4 chunk_text_bytes" in str(e.value)
    a = _run_file(files["reps"][1], p, 4100)
    b = _run_file(files["reps"][1], p, 4100, device_inflate=True)
    assert b"".join(b["texts"]) == b"".join(a["texts"]) == long_read and b["names"] == a["names"]


def test_search_file_device_inflate(setup, files):
    from kaamer_amd import search
    o = search.SearchOptions(SequenceType=abi.READS, ChunkTextBytes=files["budget"], ChunkSeqs=700)
    reps = files["reps"][2]
    want = list(search.SearchFile(reps, str(files["paths"]["small"]), o))
    got = list(search.SearchFile(reps, str(files["paths"]["small"]), o, device_parse=True, device_inflate=True))
    assert len(want) > 100 and got == want
    with pytest.raises(ValueError):
        next(search.SearchFile(reps, str(files["paths"]["small"]), o, device_inflate=True))
    with pytest.raises(ValueError):
        next(search.SearchFile(reps, str(files["paths"]["small"]), o, fmt="fasta", device_parse=True, device_inflate=True))
