"""Streams and whole-file drivers with -pos / -aln on all three handle kinds: kaamer_stream_open_aln_flat, the replica
stream's _pos / _aln forms, kaamer_sharded_stream_*, kaamer_search_file_opts, kaamer_sharded_search_file and
search.SearchFile.  They add a FIFO and a file reader around per-chunk calls that exist, so every comparison is exact:
a chunk that comes out of a driver equals, field for field, the one-call form (Index.search_top) of the same chunk on an
unsharded index of the whole database with the whole table attached; once the file drivers are also held against the CPU
oracle.  All replicas and shards sit on device 0."""
import ctypes as C
import gzip

import numpy as np
import pytest

from test_sharded_top_align import ALN, _same_top
from test_top_align import _against_oracle, _fasta, _same

K = 5                                             # MaxResults of every call here
READ_CUTS = (0, 700, 1400, 2100, 2800, 3000)      # what chunk_seqs = 700 makes of 3 000 reads: five chunks, a ragged last one


def _slice(packed, a, b):
    buf, offs = packed
    return np.ascontiguousarray(buf[int(offs[a]):int(offs[b])]), np.ascontiguousarray(offs[a:b + 1] - offs[a])


@pytest.fixture(scope="module")
def world(klib, gpu_device):
    """the database (2 000 proteins, through FASTA text: a table exists to attach), the unsharded index with the table
    attached, the chunks, and a cache of the one-call results they are compared with (each computed once, never changed)"""
    from kaamer_amd import abi, api, workload
    db = workload.make_db(2000, seed=51)
    prot = api.Proteins.from_fasta(_fasta(workload.unpack(db)).encode())
    img = prot.image(device=gpu_device)
    ix = api.Index.from_image(img, gpu_device)
    ix.attach_proteins(prot)
    pq = workload.unpack(workload.make_protein_queries(db, 600, seed=52))
    unrelated = workload.unpack(workload.make_db(12, seed=977))           # a chunk that reports nothing
    pchunks = [api.pack_sequences(c) for c in (pq[:1], pq[1:251], unrelated, pq[251:])]
    reads = workload.make_reads_mix(db, 3000, seed=53)
    rchunks = [_slice(reads, a, b) for a, b in zip(READ_CUTS[:-1], READ_CUTS[1:])]
    w = dict(db=db, prot=prot, img=img, ix=ix, pq=pq, reads=reads, shard_images={},
             chunks={"protein": (abi.PROTEIN, pchunks), "reads": (abi.READS, rchunks)}, refs={})

    def ref(kind, i, pos, aln, packed=None):
        key = (kind, i, bool(pos), bool(aln))
        if key not in w["refs"]:
            seq_type, chunks = w["chunks"][kind]
            w["refs"][key] = ix.search_top(packed=packed if packed is not None else chunks[i], seq_type=seq_type, max_results=K,
                                           want_positions=pos, align=ALN if aln else None)
        return w["refs"][key]

    def sharded(W, table=True):
        if W not in w["shard_images"]:
            w["shard_images"][W] = [prot.image(shard=r, n_shards=W, device=gpu_device) for r in range(W)]
        sx = api.ShardedIndex.from_images(w["shard_images"][W], [gpu_device] * W)
        if table:
            sx.attach_proteins(prot)
        return sx
    w["ref"], w["sharded"] = ref, sharded
    assert ref("protein", 2, False, False).n_reported == 0 and ref("protein", 1, False, False).n_reported > 200
    return w


FORMS = {"plain": (False, False), "pos": (True, False), "aln": (False, True), "pos+aln": (True, True)}


def _drive(st, w, kind, pos, aln, order, expect_busy):
    """pushes the chunks `order` names through the stream, popping one whenever a push says busy, then drains; every
    popped chunk is compared with the one-call form of the same chunk -> how often a push said busy"""
    _, chunks = w["chunks"][kind]
    fifo, busy = [], 0
    for i in order:
        while not st.push(*chunks[i]):
            busy += 1
            assert st.pending == len(fifo) > 0
            _same_top(st.pop(), w["ref"](kind, fifo.pop(0), pos, aln))
        fifo.append(i)
        assert st.pending == len(fifo)
    while fifo:
        _same_top(st.pop(), w["ref"](kind, fifo.pop(0), pos, aln))
    assert st.pending == 0
    assert (busy > 0) == expect_busy
    return busy


# ---------------------------------------------------------------- 1. one index
@pytest.mark.gpu
@pytest.mark.parametrize("kind,pos", (("protein", False), ("protein", True), ("reads", False), ("reads", True)))
def test_one_index_stream_with_alignments(world, gpu_device, kind, pos):
    from kaamer_amd import abi, api
    seq_type, chunks = world["chunks"][kind]
    st = world["ix"].stream(seq_type, max_results=K, want_positions=pos, align=ALN)
    # more chunks than the index has slots (KAAMER_HOST_SLOTS, default 4): the busy path is entered
    _drive(st, world, kind, pos, True, list(range(len(chunks))) * 2, expect_busy=True)
    top = world["ref"](kind, 1, pos, True)
    assert top.alignments and sum(a["status"] == 0 for a in top.alignments) > 100 and (top.pos_bits is not None) == pos
    st.close()
    bare = api.Index.from_image(world["img"], gpu_device)
    with pytest.raises(abi.KaamerError) as ei:
        bare.stream(seq_type, max_results=K, want_positions=pos, align=ALN)
    assert ei.value.code == abi.E_ARG
    bare.close()


# ---------------------------------------------------------------- 2. replicas
@pytest.mark.gpu
def test_replica_stream_positions_and_alignments(world, gpu_device):
    from kaamer_amd import abi, api
    reps = api.Replicas.from_image(world["img"], [gpu_device, gpu_device])
    with pytest.raises(abi.KaamerError) as ei:                 # no table yet
        reps.stream(abi.READS, max_results=K, want_positions=True, align=ALN)
    assert ei.value.code == abi.E_ARG
    reps.attach_proteins(world["prot"])
    for pos, aln in ((True, True), (True, False)):
        st = reps.stream(abi.READS, max_results=K, want_positions=pos, align=ALN if aln else None)
        for i in range(5):
            assert st.push(*world["chunks"]["reads"][1][i])
        assert st.pending == 5
        got = [st.pop() for _ in range(5)]
        refs = [world["ref"]("reads", i, pos, aln) for i in range(5)]
        assert len({r.n_queries for r in refs}) == 5           # the chunks differ: equality below pins the order
        for g, r in zip(got, refs):
            _same_top(g, r)
        st.close()
    reps.close()


# ---------------------------------------------------------------- 3. sharded handle
@pytest.mark.gpu
@pytest.mark.parametrize("form", ("plain", "pos", "aln"))
@pytest.mark.parametrize("W", (1, 2, 3))
def test_sharded_stream_equals_unsharded(world, W, form):
    from kaamer_amd import abi
    pos, aln = FORMS[form]
    sx = world["sharded"](W, table=aln)
    for kind in ("protein", "reads"):
        seq_type, chunks = world["chunks"][kind]
        st = sx.stream(seq_type, max_results=K, want_positions=pos, align=ALN if aln else None)
        # the stream is the handle's only user: the push after KAAMER_SHARDED_SETS un-popped chunks says busy at once
        for i in range(abi.SHARDED_SETS):
            assert st.push(*chunks[i])
        assert st.pending == abi.SHARDED_SETS == 3
        assert not st.push(*chunks[3])
        assert st.pending == 3
        _same_top(st.pop(), world["ref"](kind, 0, pos, aln))
        assert st.push(*chunks[3])                             # after one pop a push succeeds
        for i in (1, 2, 3):
            _same_top(st.pop(), world["ref"](kind, i, pos, aln))
        _drive(st, world, kind, pos, aln, list(range(len(chunks))) + [1, 0], expect_busy=True)
        st.close()
    if aln:
        bare = world["sharded"](W, table=False)
        with pytest.raises(abi.KaamerError) as ei:
            bare.stream(abi.PROTEIN, max_results=K, align=ALN)
        assert ei.value.code == abi.E_ARG
        bare.close()
    sx.close()


@pytest.mark.gpu
def test_sharded_stream_close_drops_what_nobody_popped(world):
    from kaamer_amd import abi
    sx = world["sharded"](2)
    seq_type, chunks = world["chunks"]["reads"]
    st = sx.stream(seq_type, max_results=K, want_positions=True, align=ALN)
    assert st.push(*chunks[0]) and st.push(*chunks[1])
    st.close()                                                 # two sets busy: waited for, dropped, given back
    st = sx.stream(seq_type, max_results=K, want_positions=True, align=ALN)
    for i in range(3):
        assert st.push(*chunks[i])                             # all three sets are free again
    for i in range(3):
        _same_top(st.pop(), world["ref"]("reads", i, True, True))
    st.close()
    # streaming.StreamingSearcher over the sharded handle
    from kaamer_amd import stream
    ss = stream.StreamingSearcher(sx, 700, 1 << 30, seq_type=abi.READS, n_buffers=2, max_results=K)
    seen = []
    ss.run(*world["reads"], on_chunk=lambda a, n, top: seen.append((a, n, top)))
    ss.close()
    assert [(a, n) for a, n, _ in seen] == [(a, b - a) for a, b in zip(READ_CUTS[:-1], READ_CUTS[1:])]
    for i, (_, _, top) in enumerate(seen):
        _same_top(top, world["ref"]("reads", i, False, False))
    sx.close()


# ---------------------------------------------------------------- 4. bounds inside a stream
@pytest.mark.gpu
def test_a_chunk_beyond_the_bounds_is_repeated_inside_pop(world):
    """20 reads, then 2 000, then 20 on W = 2 with alignments and positions, each popped before the next is pushed: every
    chunk runs on the handle's first set, whose segments are sized from the previous chunk's need plus a quarter -- far
    below what the second chunk needs.  It is repeated inside pop and comes back whole."""
    from kaamer_amd import abi
    sx = world["sharded"](2)
    st = sx.stream(abi.READS, max_results=K, want_positions=True, align=ALN)
    attempts = []
    for n, (a, b) in enumerate(((0, 20), (100, 2100), (2500, 2520))):
        chunk = _slice(world["reads"], a, b)
        assert st.push(*chunk)
        top = st.pop()
        _same_top(top, world["ref"]("reads", "bounds%d" % n, True, True, packed=chunk))
        info, pinfo = sx.align_info(), sx.positions_info()
        print("chunk of %d reads:" % (b - a), info, pinfo)
        attempts.append(info["attempts"])
    assert attempts[0] == 1 and attempts[1] > 1
    st.close()
    sx.close()


# ---------------------------------------------------------------- 5. file drivers
@pytest.fixture(scope="module")
def files(world, tmp_path_factory):
    """the 3 000 mixed reads as FASTQ text (names r0 .. r2999), as plain text and as a two-member gzip file cut in the
    middle of a line; 600 protein queries as FASTA with lower-case letters in the last record and in the one before"""
    from kaamer_amd import workload
    d = tmp_path_factory.mktemp("stream_drivers")
    rl = workload.unpack(world["reads"])
    text = "".join("@r%d\n%s\n+\n%s\n" % (i, s.decode(), "I" * len(s)) for i, s in enumerate(rl)).encode()
    plain, gz = d / "reads.fastq", d / "reads.fastq.gz"
    plain.write_bytes(text)
    cut = len(text) // 2 + 3
    gz.write_bytes(gzip.compress(text[:cut], compresslevel=1) + gzip.compress(text[cut:], compresslevel=1))
    pq = [s.decode() for s in world["pq"]]
    pq[598] = pq[598][:20] + pq[598][20:60].lower() + pq[598][60:]      # not the file's last record: upper-cased by the reader
    pq[599] = pq[599][:20] + pq[599][20:60].lower() + pq[599][60:]      # the last record: left as it is
    ptext = "".join(">q%d some words\n%s\n" % (i, s) for i, s in enumerate(pq)).encode()
    fasta = d / "queries.fasta"
    fasta.write_bytes(ptext)
    return dict(text=text, plain=plain, gz=gz, rl=rl, ptext=ptext, fasta=fasta)


def _handle(world, gpu_device, which):
    """two replicas with the table attached, or the W = 2 sharded handle with the table attached"""
    from kaamer_amd import api
    if which == "sharded":
        return world["sharded"](2)
    reps = api.Replicas.from_image(world["img"], [gpu_device, gpu_device])
    reps.attach_proteins(world["prot"])
    return reps


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("plain", "pos", "pos+aln"))
@pytest.mark.parametrize("which", ("replicas", "sharded"))
def test_search_file_chunks(world, files, gpu_device, which, form):
    from kaamer_amd import abi
    pos, aln = FORMS[form]
    h = _handle(world, gpu_device, which)
    L = abi.lib()
    seen = []

    def on_chunk(first, reads_h, top):
        seen.append((first, int(L.kaamer_reads_count(reads_h)), top))
    path = files["gz"] if which == "replicas" else files["plain"]
    total = h.search_file(path, "fastq", seq_type=abi.READS, max_results=K, chunk_seqs=700, in_flight=2, on_chunk=on_chunk,
                                 want_positions=pos, align=ALN if aln else None)
    assert [(f, n) for f, n, _ in seen] == [(a, b - a) for a, b in zip(READ_CUTS[:-1], READ_CUTS[1:])]   # contiguous, in order, ragged last
    for i, (_, _, top) in enumerate(seen):
        _same_top(top, world["ref"]("reads", i, pos, aln))
    summed = {}
    for _, _, top in seen:
        for k, v in top.counters.items():
            summed[k] = summed.get(k, 0) + v
    assert total == summed and total["n_lookup"] > 0 and total["n_hits"] > 0
    h.close()


def _strip_positions(res):
    out = []
    for qr in res:
        qr = dict(qr)
        qr["SearchResults"] = {k: v for k, v in qr["SearchResults"].items() if k != "PositionHits"}
        out.append(qr)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("which", ("replicas", "sharded"))
def test_search_file_driver_reads(world, files, oracle, gpu_device, which):
    from kaamer_amd import abi, search
    h = _handle(world, gpu_device, which)
    ix, text = world["ix"], files["text"]
    path = files["plain"] if which == "replicas" else files["gz"]
    opt = lambda **kw: search.SearchOptions(SequenceType=abi.READS, MaxResults=K, ChunkSeqs=700, InFlight=2, **kw)
    # plain
    got = list(search.SearchFile(h, path, opt(), "fastq"))
    exp = search.FastqSearch(ix, text, opt())
    assert len(got) == len(exp) > 1000
    for g, e in zip(got, exp):
        assert _same(g, e), (g["Query"]["Name"], g, e)
    # with alignments: HitEntries, Alignment, hits in BitScore order
    got_aln = list(search.SearchFile(h, path, opt(Align=True)))
    exp_aln = search.FastqSearch(ix, text, opt(Align=True))
    assert len(got_aln) == len(exp_aln) == len(exp)
    for g, e in zip(got_aln, exp_aln):
        assert _same(g, e), (g["Query"]["Name"], g, e)
    assert all("HitEntries" in g and all("Alignment" in x for x in g["SearchResults"]["Hits"]) for g in got_aln)
    # with positions: everything else equals the full-list route's result, and PositionHits are that route's bitmaps
    # restricted to the reported hits
    got_pos = list(search.SearchFile(h, path, opt(ExtractPositions=True)))
    exp_pos = search.FastqSearch(ix, text, opt(ExtractPositions=True))
    assert len(got_pos) == len(exp_pos) == len(exp)
    for g, e in zip(_strip_positions(got_pos), exp_pos):
        assert _same(g, e), (g["Query"]["Name"], g, e)
    full = ix.search(packed=world["reads"], seq_type=abi.READS, want_positions=True)
    where = {(int(m["src_seq"]), int(m["end_position"]), bool(m["plus_strand"])): q for q, m in enumerate(full.meta)}
    assert len(where) == full.n_queries
    checked = 0
    for g in got_pos:
        loc = g["Query"]["Location"]
        all_pos = full.positions(where[(int(g["Query"]["Name"][1:]), loc["EndPosition"], loc["PlusStrand"])])
        ph = g["SearchResults"]["PositionHits"]
        assert set(ph) == {x["Key"] for x in g["SearchResults"]["Hits"]}
        for key, bits in ph.items():
            assert bits == all_pos[key].tolist() and any(bits)
            checked += 1
    assert checked > 1000
    # ... and a sample of 40 reads against the oracle: every one of them
    oix = oracle.Index.from_proteins(None, ids=world["prot"].ids, packed=world["prot"].packed)
    sample = list(range(0, 3000, 75))
    assert len(sample) == 40
    by_read = {}
    for g in got:
        by_read.setdefault(int(g["Query"]["Name"][1:]), []).append([(x["Key"], x["Kmatch"]) for x in g["SearchResults"]["Hits"]])
    reporting = 0
    for i in sample:
        rep = []
        for o in oracle.get_orfs(files["rl"][i]):
            pid, km, pos = oix.search(o["seq"], want_positions=True)
            keep = 0
            if len(km) and km[0] >= 10:
                _, _, so = oracle.set_best_start_codon(km, pos, oracle.size_in_kmer(o["seq"]), o["starts"], o["plus"], o["seq"], o["start"])
                keep = oracle.filter_results(km, so, max_results=K)
            if keep:
                rep.append(list(zip(pid[:keep].tolist(), km[:keep].tolist())))
        assert by_read.get(i, []) == rep, i
        reporting += bool(rep)
    assert reporting > 20
    n, _ = _against_oracle(oracle, [g for g in got_aln if int(g["Query"]["Name"][1:]) in sample], world["prot"].stats()["NumberOfAA"])
    assert n > 20
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ("replicas", "sharded"))
def test_search_file_driver_protein_fasta(world, files, gpu_device, which):
    """600 protein queries, 599 in the first chunk and the file's last record alone in the second: the reader upper-cases
    every record but the file's last, across the chunk boundary"""
    from kaamer_amd import abi, api, search
    h = _handle(world, gpu_device, which)
    ix, ptext = world["ix"], files["ptext"]
    parsed = api.parse_reads(ptext.decode(), "fasta")
    assert parsed[598]["seq"].isupper() and not parsed[599]["seq"].isupper()
    opt = lambda **kw: search.SearchOptions(SequenceType=abi.PROTEIN, MaxResults=K, ChunkSeqs=599, InFlight=2, **kw)
    for kw in (dict(), dict(ExtractPositions=True), dict(Align=True)):
        got = list(search.SearchFile(h, files["fasta"], opt(**kw)))
        exp = search.ProteinSearch(ix, ptext.decode(), opt(**kw))
        assert len(got) == len(exp) > 400
        for g, e in zip(got, exp):
            assert _same(g, e), (kw, g["Query"]["Name"], g, e)
        assert got[-1]["Query"]["Name"] == "q599 some words" and not got[-1]["Query"]["Sequence"].isupper()
        assert ("PositionHits" in got[0]["SearchResults"]) == bool(kw.get("ExtractPositions"))
    h.close()


# ---------------------------------------------------------------- 6. stopping and failing
@pytest.mark.gpu
@pytest.mark.parametrize("which", ("replicas", "sharded"))
def test_a_callback_that_stops_the_run(world, files, gpu_device, which):
    from kaamer_amd import abi, api
    h = _handle(world, gpu_device, which)
    L = abi.lib()
    calls = []

    def cb(user, first, reads, top):
        calls.append(int(first))
        return 1 if len(calls) == 2 else 0
    cfn = api.Replicas.CHUNK_CB(cb)
    fn = L.kaamer_search_file_opts if which == "replicas" else L.kaamer_sharded_search_file
    c = abi.Counters()
    rc = fn(h._h, str(files["plain"]).encode(), 1, 0, abi.READS, 0.05, 10, K, 1, 1, b"blosum62", 11, 1, 1, 700, 1 << 28, 2,
            C.cast(cfn, C.c_void_p), None, C.byref(c))
    assert rc == abi.E_ARG
    assert calls[:2] == [0, 700] and calls == sorted(calls)
    # nothing stayed busy: the next run on the same handle is complete ...
    seen = []
    h.search_file(files["plain"], "fastq", seq_type=abi.READS, max_results=K, chunk_seqs=700, in_flight=2, want_positions=True, align=ALN,
                         on_chunk=lambda first, reads_h, top: seen.append((first, top)))
    assert [f for f, _ in seen] == list(READ_CUTS[:-1])
    _same_top(seen[4][1], world["ref"]("reads", 4, True, True))
    # ... an exception in a Python callback ends it the same way and comes out as itself ...
    def boom(first, reads_h, top):
        raise KeyError("stop here")
    with pytest.raises(KeyError):
        h.search_file(files["plain"], "fastq", seq_type=abi.READS, max_results=K, chunk_seqs=700, in_flight=2, on_chunk=boom)
    # ... and every slot / set can be taken by a stream
    st = h.stream(abi.READS, max_results=K)
    room = abi.SHARDED_SETS if which == "sharded" else 8
    for i in range(room):
        assert st.push(*world["chunks"]["reads"][1][i % 5])
    assert not st.push(*world["chunks"]["reads"][1][0])
    st.close()
    h.close()


@pytest.mark.gpu
def test_attach_while_a_stream_holds_a_chunk(world):
    from kaamer_amd import abi
    sx = world["sharded"](2)
    st = sx.stream(abi.READS, max_results=K, align=ALN)
    assert st.push(*world["chunks"]["reads"][1][4])
    with pytest.raises(abi.KaamerError) as ei:
        sx.attach_proteins(world["prot"])
    assert ei.value.code == abi.E_BUSY
    _same_top(st.pop(), world["ref"]("reads", 4, False, True))
    sx.attach_proteins(world["prot"])                           # nothing pending: a second attach replaces the first
    assert st.push(*world["chunks"]["reads"][1][4])
    _same_top(st.pop(), world["ref"]("reads", 4, False, True))
    st.close()
    sx.close()
