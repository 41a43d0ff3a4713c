"""The request's genetic code on the device: KAAMER_SEQ_TYPE(type, code) on every form of the call.

The oracle is fixed to table 11, so the expected side of another code is built by gcoderef: ORFs from pyref.get_orfs with
the fixture's table (tests/golden/gcodes.json) swapped in, which then go through the oracle as queries.
test_genetic_codes.py shows, without a device, that this helper reproduces oracle.get_orfs on table 11 and that every code
changes the ORFs of every batch used here.  The database is the 1 000-protein one of test_gpu_reads.py, through FASTA text so
that a table exists to attach; all shards and replicas sit on device 0."""
import ctypes as C
import threading

import numpy as np
import pytest

import gcoderef
from kaamer_amd import abi
from test_gpu_protein import _from_ptr
from test_gpu_reads import _check_reads
from test_sharded_top_align import ALN
from test_top_align import _fasta

pytestmark = pytest.mark.gpu

KIND = {"short": abi.READS, "wide": abi.READS, "contigs": abi.NUCLEOTIDE}
ORDER = (4, 11, 2, 0, 4)     # the no-stale-table sequence: stops move both ways between neighbours


@pytest.fixture(scope="module")
def world(klib, oracle, gpu_device):
    from kaamer_amd import api, workload
    db = workload.make_db(1000)
    prot = api.Proteins.from_fasta(_fasta(workload.unpack(db)).encode())
    img = prot.image(device=gpu_device)
    ix = api.Index.from_image(img, gpu_device)
    ix.attach_proteins(prot)
    oix = oracle.Index.from_proteins(None, ids=prot.ids, packed=prot.packed)
    batches = gcoderef.make_batches(db)
    small = batches["short"][:60] + batches["short"][-94:]      # reads from the database, and the table-specific closings
    batches["small"] = small
    KIND["small"] = abi.READS
    w = dict(db=db, prot=prot, img=img, ix=ix, oix=oix, batches=batches, packed={k: api.pack_sequences(v) for k, v in batches.items()},
             exp=gcoderef.Expected(oracle, oix), orfs={}, tops={}, refs={}, shard_images={}, device=gpu_device)

    def orfs(monkeypatch, code, name):
        key = (code or 11, name)
        if key not in w["orfs"]:
            w["orfs"][key] = gcoderef.expected_orfs(monkeypatch, code or 11, batches[name])
        return w["orfs"][key]

    def exp_top(monkeypatch, code, name):
        key = (code or 11, name)
        if key not in w["tops"]:
            w["tops"][key] = w["exp"].top(orfs(monkeypatch, code, name))
        return w["tops"][key]

    def ref(code, name):
        """the plain search_top result of a batch under a code: the yardstick of the other forms (computed once)"""
        if (code, name) not in w["refs"]:
            w["refs"][(code, name)] = ix.search_top(packed=w["packed"][name], seq_type=abi.seq_type(KIND[name], code))
        return w["refs"][(code, name)]

    def sharded(W, table=False):
        if W not in w["shard_images"]:
            w["shard_images"][W] = [prot.image(shard=r, n_shards=W, device=gpu_device) for r in range(W)]
        sx = api.ShardedIndex.from_images(w["shard_images"][W], [gpu_device] * W)
        if table:
            sx.attach_proteins(prot)
        return sx
    w.update(orfs_of=orfs, exp_top=exp_top, ref=ref, sharded=sharded)
    return w


# ---------------------------------------------------------------- 1. every code, every kernel form
@pytest.mark.parametrize("code", gcoderef.CODES)
def test_every_code_every_kernel_form(world, monkeypatch, code):
    """reads <= 150 nt (translate_reads_kernel<192>), reads of 200 .. 384 nt (<384>), contigs (translate_kernel, one past
    the 4 096-codon piece): ORF strings, positions, strand, StartsAlternative, order, SizeInKmer, hits and lowest match
    position, bit for bit"""
    ix = world["ix"]
    for name in ("short", "wide", "contigs"):
        res = ix.search(packed=world["packed"][name], seq_type=abi.seq_type(KIND[name], code))
        n = gcoderef.check_full(res, world["orfs_of"](monkeypatch, code, name), world["exp"])
        assert n > (20 if name == "contigs" else 100), name
        assert res.counters["n_queries"] == n      # (n_overflow counts queries the G tier took: long ORFs of a code with few stops)


# ---------------------------------------------------------------- 2. the default is untouched
def _same_full(a, b, orfs=True):
    """two BatchResults: the query arrays identical; a query's hit list is a set of (protein id, Kmatch, lowest position)
    entries in no particular order (test_gpu_reads.py compares them as dicts too)"""
    assert a.n_queries == b.n_queries
    for f in ("meta", "hit_cnt") + (("orf_aa", "starts_alt") if orfs else ()):
        assert getattr(a, f).tolist() == getattr(b, f).tolist(), f
    for q in range(a.n_queries):
        assert a.hits(q) == b.hits(q) and a.first_pos(q) == b.first_pos(q), q


@pytest.mark.parametrize("name", ("short", "wide", "contigs"))
def test_default_untouched(world, oracle, name):
    """seq_type alone, KAAMER_SEQ_TYPE(seq_type, 0) and KAAMER_SEQ_TYPE(seq_type, 11): identical arrays, and the oracle's"""
    ix, packed = world["ix"], world["packed"][name]
    res = [ix.search(packed=packed, seq_type=t) for t in (KIND[name], abi.seq_type(KIND[name], 0), abi.seq_type(KIND[name], 11))]
    _check_reads(res[0], world["batches"][name], oracle, world["oix"])
    for r in res[1:]:
        _same_full(res[0], r)
    tops = [ix.search_top(packed=packed, seq_type=t) for t in (KIND[name], abi.seq_type(KIND[name], 11))]
    gcoderef.same_reported(tops[1], tops[0])
    assert tops[1].top_pid.tolist() == tops[0].top_pid.tolist()


# ---------------------------------------------------------------- 3. reported hits
@pytest.mark.parametrize("code", (4, 2))
def test_reported_hits(world, monkeypatch, code):
    """search_top under codes 4 (tga = W: stops go) and 2 (aga / agg stop: stops come) against the expected pipeline:
    reported queries, trim, StartPosition and SizeInKmer after SetBestStartCodon, hits, top_first_pos"""
    for name in ("short", "wide"):
        exp = world["exp_top"](monkeypatch, code, name)
        n = gcoderef.check_top(world["ref"](code, name), exp)
        assert n > 50
        assert exp != world["exp_top"](monkeypatch, 11, name)          # the code changes what is reported
    assert any(e is not None and e["trim"] > 0 for e in world["exp_top"](monkeypatch, code, "short")), "no ORF was trimmed: SetBestStartCodon went unchecked"


# ---------------------------------------------------------------- 4. no stale table
def _device_call(ws, d_buf, d_off, n, nbytes, seq_type, st):
    """one device-resident call -> (ORFs as (src, seq, start, end, plus, size), {query: {pid: Kmatch}})"""
    r = ws.search_device(d_buf.data_ptr(), d_off.data_ptr(), n, nbytes, seq_type=seq_type, stream=st)
    c = ws.finish(st)
    nq = int(_from_ptr(r.d_n_queries, 1, np.uint32)[0])
    assert nq == c["n_queries"]
    from kaamer_amd import api
    meta = _from_ptr(r.d_q, nq * C.sizeof(abi.QueryMeta), np.uint8).view(api.META_DTYPE)
    n_aa = int((meta["aa_off"] + meta["aa_len"]).max()) if nq else 0
    aa = bytes(_from_ptr(r.d_orf_aa, n_aa, np.uint8))
    hit_off = _from_ptr(r.d_hit_off, nq + 1, np.uint64)
    hit_cnt = _from_ptr(r.d_hit_cnt, nq, np.uint32)
    pid = _from_ptr(r.d_hit_pid, int(r.hit_capacity), np.uint32)
    km = _from_ptr(r.d_hit_kmatch, int(r.hit_capacity), np.uint32)
    orfs = [(int(m["src_seq"]), aa[int(m["aa_off"]):int(m["aa_off"]) + int(m["aa_len"])].decode("latin-1"), int(m["start_position"]),
             int(m["end_position"]), bool(m["plus_strand"]), int(m["size_in_kmer"])) for m in meta]
    hits = [dict(zip(pid[int(hit_off[q]):int(hit_off[q]) + int(hit_cnt[q])].tolist(), km[int(hit_off[q]):int(hit_off[q]) + int(hit_cnt[q])].tolist()))
            for q in range(nq)]
    return orfs, hits


def _expected_device(world, monkeypatch, code, name):
    exp, oracle = world["exp"], world["exp"].oracle
    orfs = [(r, o["seq"], o["start"], o["end"], o["plus"], oracle.size_in_kmer(o["seq"]))
            for r, per_seq in enumerate(world["orfs_of"](monkeypatch, code, name)) for o in per_seq]
    hits = []
    for o in orfs:
        pid, km, _ = exp.hits(o[1])
        hits.append(dict(zip(pid.tolist(), km.tolist())))
    return orfs, hits


def test_no_stale_table_on_one_workspace(world, monkeypatch):
    """the device-resident call: codes 4, 11, 2, 0, 4 on ONE workspace, which was created with yet another code"""
    import torch
    from kaamer_amd import api
    buf, offs = world["packed"]["small"]
    ws = api.Workspace(world["ix"], len(buf), len(offs) - 1, seq_type=abi.seq_type(abi.READS, 13), max_queries=8 * len(offs))
    d_buf, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(offs.view(np.int64)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    for code in ORDER:
        got = _device_call(ws, d_buf, d_off, len(offs) - 1, len(buf), abi.seq_type(abi.READS, code), st)
        assert got == _expected_device(world, monkeypatch, code, "small"), code
    ws.close()


def test_no_stale_table_on_host_slots(world, monkeypatch):
    """one index, two threads, each running the sequence of codes through the host calls: slots and their workspaces are
    shared between the codes"""
    ix = world["ix"]
    exp = {c: (world["orfs_of"](monkeypatch, c, "small"), world["exp_top"](monkeypatch, c, "small")) for c in set(ORDER)}
    errors = []

    def worker(shift):
        try:
            for i in range(len(ORDER)):
                code = ORDER[(i + shift) % len(ORDER)]
                t = abi.seq_type(abi.READS, code)
                gcoderef.check_full(ix.search(packed=world["packed"]["small"], seq_type=t), exp[code][0], world["exp"])
                gcoderef.check_top(ix.search_top(packed=world["packed"]["small"], seq_type=t), exp[code][1])
        except BaseException as e:  # noqa: BLE001
            errors.append(repr(e))
    th = [threading.Thread(target=worker, args=(s,)) for s in (0, 2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def test_no_stale_table_on_a_sharded_handle(world, monkeypatch):
    """W = 2 on one device: every shard translates the whole batch with the call's code"""
    sx = world["sharded"](2)
    for code in ORDER:
        t = abi.seq_type(abi.READS, code)
        gcoderef.check_top(sx.search_top(packed=world["packed"]["small"], seq_type=t), world["exp_top"](monkeypatch, code, "small"))
        gcoderef.check_full(sx.search(packed=world["packed"]["small"], seq_type=t), world["orfs_of"](monkeypatch, code, "small"), world["exp"])
    sx.close()


def test_two_streams_keep_their_own_code(world, monkeypatch):
    """two streams with different codes open on one index at once, pushed alternately"""
    ix, packed = world["ix"], world["packed"]["small"]
    a, b = ix.stream(abi.seq_type(abi.READS, 4)), ix.stream(abi.seq_type(abi.READS, 2))
    for _ in range(2):
        assert a.push(*packed) and b.push(*packed)
        gcoderef.check_top(a.pop(), world["exp_top"](monkeypatch, 4, "small"))
        gcoderef.check_top(b.pop(), world["exp_top"](monkeypatch, 2, "small"))
    a.close(); b.close()


# ---------------------------------------------------------------- 5. every form carries it
def _fastq(tmp_path, reads):
    from kaamer_amd import api, workload
    p = tmp_path / "gcode.fastq"
    p.write_bytes(workload.fastq_text(api.pack_sequences(reads)))
    return str(p)


def _file_reads(world):
    """the reads a FASTQ file can carry (the reader keeps lines of [ATGCNatgcn]+ only; an empty record has none)"""
    return [r for r in world["batches"]["small"] if len(r) > 0]


def _collect(chunks):
    def on_chunk(first, reads_h, top):
        chunks.append((first, top))
    return on_chunk


def _same_file(world, chunks, code, reads, cuts):
    from kaamer_amd import api
    assert [c[0] for c in chunks] == list(cuts[:-1])
    for (first, top), a, b in zip(chunks, cuts[:-1], cuts[1:]):
        ref = world["ix"].search_top(packed=api.pack_sequences(reads[a:b]), seq_type=abi.seq_type(abi.READS, code))
        gcoderef.same_reported(top, ref)


def test_every_form_carries_the_code(world, monkeypatch, tmp_path):
    """with code 4, the plain search_top result (held against the expected pipeline by test_reported_hits) is the yardstick:
    the _pos and _aln forms, Index.stream, the replica stream and search_file, the sharded call, stream and file driver
    at W = 2 and 3 return the same reported queries and hits"""
    from kaamer_amd import api
    ix, packed, code = world["ix"], world["packed"]["small"], 4
    t = abi.seq_type(abi.READS, code)
    ref = world["ref"](code, "small")
    gcoderef.check_top(ref, world["exp_top"](monkeypatch, code, "small"))
    assert ref.n_reported > 30
    for kw in (dict(want_positions=True), dict(align=ALN), dict(want_positions=True, align=ALN), dict(flat=False)):
        gcoderef.same_reported(ix.search_top(packed=packed, seq_type=t, **kw), ref)
    gcoderef.same_reported(ix.submit_top(packed=packed, seq_type=t).wait(), ref)
    for kw in (dict(), dict(want_positions=True), dict(align=ALN)):
        st = ix.stream(t, **kw)
        assert st.push(*packed)
        gcoderef.same_reported(st.pop(), ref)
        st.close()
    reads = _file_reads(world)
    path = _fastq(tmp_path, reads)
    cuts = list(range(0, len(reads), 50)) + [len(reads)]
    reps = api.Replicas.from_image(world["img"], [world["device"]] * 2)
    reps.attach_proteins(world["prot"])
    st = reps.stream(t)
    assert st.push(*packed)
    gcoderef.same_reported(st.pop(), ref)
    st.close()
    for kw in (dict(), dict(want_positions=True, align=ALN)):
        chunks = []
        reps.search_file(path, "fastq", seq_type=t, chunk_seqs=50, on_chunk=_collect(chunks), **kw)
        _same_file(world, chunks, code, reads, cuts)
    reps.close()
    for W in (2, 3):
        sx = world["sharded"](W, table=True)
        for kw in (dict(), dict(want_positions=True), dict(align=ALN)):
            gcoderef.same_reported(sx.search_top(packed=packed, seq_type=t, **kw), ref)
        st = sx.stream(t)
        assert st.push(*packed)
        gcoderef.same_reported(st.pop(), ref)
        st.close()
        chunks = []
        sx.search_file(path, "fastq", seq_type=t, chunk_seqs=50, on_chunk=_collect(chunks))
        _same_file(world, chunks, code, reads, cuts)
        sx.close()


def test_sharded_searcher_world_1(world, monkeypatch):
    """the per-rank driver hands the composite to kaamer_search_device: one world-1 run under code 4"""
    import torch
    from kaamer_amd import sharded
    buf, offs = world["packed"]["small"]
    n = len(offs) - 1
    ref = world["ref"](4, "small")
    d_buf, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(offs.view(np.int64)).cuda()
    st = torch.cuda.current_stream()
    ss = sharded.ShardedSearcher(world["ix"], 0, 1, len(buf), n, seq_type=abi.seq_type(abi.READS, 4), max_entries_per_peer=1 << 16)
    assert ss.nucl
    r, c, cm = ss.run(d_buf.data_ptr(), d_off.data_ptr(), n, len(buf), st, topn=dict(max_results=10))
    assert c["n_queries"] == ref.n_queries
    t = ss.last_topn
    tc = sharded.dev_tensor(t.d_top_cnt, ref.n_queries, torch.int32).cpu().numpy()
    tp = sharded.dev_tensor(t.d_top_pid, ref.n_queries * 10, torch.int32).cpu().numpy().view(np.uint32).reshape(-1, 10)
    tk = sharded.dev_tensor(t.d_top_kmatch, ref.n_queries * 10, torch.int32).cpu().numpy().view(np.uint32).reshape(-1, 10)
    rpid, rkm = ref.dense()
    assert tc.tolist() == ref.top_cnt.tolist()
    for q in range(ref.n_queries):
        k = int(tc[q])
        assert tp[q, :k].tolist() == rpid[q, :k].tolist() and tk[q, :k].tolist() == rkm[q, :k].tolist(), q
    ss.close()


# ---------------------------------------------------------------- 6. refusals
BAD = (abi.seq_type(abi.READS, 7), abi.seq_type(abi.READS, 16), abi.READS | 1 << 16)
NAMED = ("genetic code 7", "genetic code 16", "0x10002")


def _refused(fn, named):
    with pytest.raises(abi.KaamerError) as e:
        fn()
    assert e.value.code == abi.E_ARG and named in str(e.value), str(e.value)


def _free_slots(handle, chunk):
    """how many chunks a fresh stream on the handle takes before a push says busy: the slots (sets) nobody holds"""
    st = handle.stream(abi.READS)
    n = 0
    while n < 64 and st.push(*chunk):
        n += 1
    st.close()
    return n


def test_refusals_leave_nothing_held(world, monkeypatch, tmp_path):
    import torch
    from kaamer_amd import api
    ix, packed = world["ix"], world["packed"]["small"]
    tiny = api.pack_sequences(world["batches"]["small"][:5])
    buf, offs = packed
    path = _fastq(tmp_path, _file_reads(world)[:40])
    free = _free_slots(ix, tiny)
    assert free >= 1
    # kaamer_search_device: nothing enqueued, the workspace serves the next call
    ws = api.Workspace(ix, len(buf), len(offs) - 1, seq_type=abi.READS, max_queries=8 * len(offs))
    d_buf, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(offs.view(np.int64)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    for bad, named in zip(BAD, NAMED):
        _refused(lambda: ws.search_device(d_buf.data_ptr(), d_off.data_ptr(), len(offs) - 1, len(buf), seq_type=bad, stream=st), named)
    assert _device_call(ws, d_buf, d_off, len(offs) - 1, len(buf), abi.seq_type(abi.READS, 4), st) == _expected_device(world, monkeypatch, 4, "small")
    ws.close()
    # a flat top call, a stream open, a file call on the unsharded handles
    reps = api.Replicas.from_image(world["img"], [world["device"]])
    for bad, named in zip(BAD, NAMED):
        _refused(lambda: ix.search_top(packed=packed, seq_type=bad), named)
        assert _free_slots(ix, tiny) == free
        _refused(lambda: ix.search(packed=packed, seq_type=bad), named)
        _refused(lambda: ix.stream(bad), named)
        _refused(lambda: reps.stream(bad, want_positions=True), named)
        _refused(lambda: reps.search_file(path, "fastq", seq_type=bad), named)
        _refused(lambda: reps.search_file(str(tmp_path / "no_such_file.fastq"), "fastq", seq_type=bad), named)   # the code is looked at first
    assert _free_slots(ix, tiny) == free
    gcoderef.same_reported(ix.search_top(packed=packed, seq_type=abi.seq_type(abi.READS, 4)), world["ref"](4, "small"))
    chunks = []
    reps.search_file(path, "fastq", seq_type=abi.seq_type(abi.READS, 4), on_chunk=_collect(chunks))
    assert len(chunks) == 1
    reps.close()
    # the sharded flat calls
    sx = world["sharded"](2)
    sfree = _free_slots(sx, tiny)
    assert sfree >= 1
    for bad, named in zip(BAD, NAMED):
        _refused(lambda: sx.search_top(packed=packed, seq_type=bad), named)
        assert _free_slots(sx, tiny) == sfree
        _refused(lambda: sx.search(packed=packed, seq_type=bad), named)
        _refused(lambda: sx.stream(bad), named)
        _refused(lambda: sx.search_file(path, "fastq", seq_type=bad), named)
    assert _free_slots(sx, tiny) == sfree
    gcoderef.same_reported(sx.search_top(packed=packed, seq_type=abi.seq_type(abi.READS, 4)), world["ref"](4, "small"))
    sx.close()


def test_protein_requests_ignore_a_valid_code(world):
    """the reference sends GeneticCode: 11 on protein requests too: a valid code is accepted and changes nothing; an
    invalid one is refused like everywhere"""
    from kaamer_amd import workload
    ix = world["ix"]
    q = workload.make_protein_queries(world["db"], 60, seed=1307)
    plain = ix.search_top(packed=q, seq_type=abi.PROTEIN)
    assert plain.n_reported > 20
    for code in (4, 11):
        got = ix.search_top(packed=q, seq_type=abi.seq_type(abi.PROTEIN, code))
        gcoderef.same_reported(got, plain)
        assert got.top_pid.tolist() == plain.top_pid.tolist()
    full, full4 = ix.search(packed=q, seq_type=abi.PROTEIN), ix.search(packed=q, seq_type=abi.seq_type(abi.PROTEIN, 4))
    _same_full(full, full4, orfs=False)
    _refused(lambda: ix.search_top(packed=q, seq_type=abi.seq_type(abi.PROTEIN, 8)), "genetic code 8")
