"""PositionHits bitmaps of the REPORTED hits on the top-N calls (kaamer_search_batch_top_pos_flat and its submit / stream /
device-resident forms) against the CPU oracle's PositionHits rows.  Every comparison is bit-exact."""
import ctypes as C

import numpy as np
import pytest

from test_top_positions_host import format_positions_ref

pytestmark = pytest.mark.gpu

ALPHA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
OPTS = ((0.05, 10, 10), (0.0, 1, 3), (0.0, 1, 700))


def _dev(ptr, n, dtype):
    from test_gpu_protein import _from_ptr
    return _from_ptr(ptr, n, dtype)


def _oracle_protein(oracle, oix, s, ratio, mink, maxr):
    """-> (SizeInKmer, reported pids, Kmatch, PositionHits rows) of one protein query, or None if nothing is reported"""
    size = oracle.size_in_kmer(s)
    if size < 7:
        return None
    pid, km, pos = oix.search(s, size=size, want_positions=True)
    keep = oracle.filter_results(km, size, ratio, mink, maxr) if len(km) else 0
    if not keep:
        return None
    return size, pid[:keep].tolist(), km[:keep].tolist(), [np.asarray(pos[h], dtype=bool) for h in range(keep)]


def _check_top(top, exp):
    """top: a TopResult asked for positions; exp[q]: _oracle_protein's tuple per query"""
    assert top.pos_bits is not None
    reported = [q for q, e in enumerate(exp) if e is not None]
    assert top.rep_query.tolist() == reported            # queries that report nothing have no entries
    assert len(top.pos_bits_len) == len(reported)
    assert len(top.pos_off) == int(top.top_off[-1]) + 1
    words = 0
    for i, q in enumerate(reported):
        size, pid, km, rows = exp[q]
        a, b = int(top.top_off[i]), int(top.top_off[i + 1])
        assert top.top_pid[a:b].tolist() == pid and top.top_kmatch[a:b].tolist() == km, q
        assert int(top.pos_bits_len[i]) == size, q
        got = top.positions(i)
        assert list(got) == pid
        for h, p in enumerate(pid):
            assert got[p].shape == (size,)
            assert np.array_equal(got[p], rows[h]), (q, p)
            assert int(got[p].sum()) == km[h], (q, p)
        nw = (size + 63) // 64
        assert top.pos_off[a:b].tolist() == [words + j * nw for j in range(b - a)]   # contiguous, in reported order
        words += (b - a) * nw
    assert int(top.pos_off[-1]) == words == len(top.pos_bits)


def _same_hits(a, b):
    assert a.rep_query.tolist() == b.rep_query.tolist()
    assert a.top_off.tolist() == b.top_off.tolist()
    assert a.top_pid.tolist() == b.top_pid.tolist() and a.top_kmatch.tolist() == b.top_kmatch.tolist()
    assert a.top_first_pos.tolist() == b.top_first_pos.tolist()
    assert a.trim.tolist() == b.trim.tolist() and a.meta.tolist() == b.meta.tolist()


def _same_positions(a, b):
    _same_hits(a, b)
    assert a.pos_bits_len.tolist() == b.pos_bits_len.tolist() and a.pos_off.tolist() == b.pos_off.tolist()
    assert np.array_equal(a.pos_bits, b.pos_bits)


@pytest.fixture(scope="module")
def small(klib, oracle, gpu_device):
    from kaamer_amd import api, workload
    db = workload.make_db(1000)
    ix = api.Index.from_image(api.Image.from_proteins(packed=db), gpu_device)
    return db, ix, oracle.Index.from_proteins(None, packed=db)


def _mix(db):
    """the query mix of test_position_bitmaps: incl. a 13-residue one, a too-short one, the longest DB protein"""
    from kaamer_amd import workload
    q = workload.make_protein_queries(db, 60, seed=9)
    return workload.unpack(q) + [workload.unpack(db)[3], b"ACDEFGHIKLMNP", b"AAAA", max(workload.unpack(db), key=len)]


@pytest.mark.parametrize("ratio,mink,maxr", OPTS)
def test_protein_host_call(small, oracle, ratio, mink, maxr):
    db, ix, oix = small
    seqs = _mix(db)
    plain = ix.search_top(seqs, min_k_ratio=ratio, min_k_match=mink, max_results=maxr)
    assert plain.pos_bits is None and plain.pos_off is None and plain.pos_bits_len is None
    top = ix.search_top(seqs, min_k_ratio=ratio, min_k_match=mink, max_results=maxr, want_positions=True)
    _same_hits(top, plain)                               # reported pids / Kmatch unchanged by the flag
    exp = [_oracle_protein(oracle, oix, s, ratio, mink, maxr) for s in seqs]
    assert sum(e is None for e in exp) >= 1 and sum(e is not None for e in exp) >= len(seqs) // 2   # (the oracle's counts: not vacuous)
    _check_top(top, exp)
    # the existing full-list path as a second witness
    full = ix.search(seqs, want_positions=True)
    for i, q in enumerate(top.rep_query.tolist()):
        allpos = full.positions(q)
        for p, bits in top.positions(i).items():
            assert np.array_equal(bits, allpos[p]), (q, p)


def test_g_tier(klib, oracle, gpu_device):
    """the database of test_position_bitmaps_g_tier: 3 000 hits per query, counted in the HBM tier"""
    from kaamer_amd import api
    rng = np.random.default_rng(14)
    core = bytes(ALPHA[rng.integers(0, 20, 70)])
    db = [bytes(ALPHA[rng.integers(0, 20, 6)]) + core[(i % 9):] + bytes(ALPHA[rng.integers(0, 20, 6)]) for i in range(3000)]
    ids = rng.permutation(20000)[:3000].astype(np.uint32)
    ix = api.Index.from_image(api.Image.from_proteins(db, ids=ids), gpu_device)
    oix = oracle.Index.from_proteins(db, ids=ids)
    seqs = [core, bytes(ALPHA[rng.integers(0, 20, 130)]) + core + bytes(ALPHA[rng.integers(0, 20, 70)]), db[11], core[:25]]
    for maxr in (10, 700):
        top = ix.search_top(seqs, min_k_ratio=0.0, min_k_match=1, max_results=maxr, want_positions=True)
        assert top.counters["n_overflow"] >= 2
        exp = [_oracle_protein(oracle, oix, s, 0.0, 1, maxr) for s in seqs]
        assert len(exp[0][1]) == maxr
        _check_top(top, exp)


def test_long_lists(klib, oracle, gpu_device):
    """one motif shared by 6 000 proteins: its k-mers' postings lists take the wave-cooperative scan"""
    from kaamer_amd import api
    rng = np.random.default_rng(9)
    motif = bytes(ALPHA[rng.integers(0, 20, 20)])
    db = []
    for i in range(6000):
        body = bytearray(bytes(ALPHA[rng.integers(0, 20, 60)]))
        body[20:40] = motif
        db.append(bytes(body))
    img = api.Image.from_proteins(db)
    assert img.stats()["max_list"] >= 5000               # the long-list path is entered
    ix = api.Index.from_image(img, gpu_device)
    oix = oracle.Index.from_proteins(db)
    fill = lambda n: bytes(ALPHA[rng.integers(0, 20, n)])
    seqs = [fill(30) + motif + fill(30), db[7], db[4999], motif + fill(3) + motif, fill(200), (fill(10) + motif) * 6]
    for (ratio, mink, maxr) in ((0.05, 10, 10), (0.0, 1, 100)):
        top = ix.search_top(seqs, min_k_ratio=ratio, min_k_match=mink, max_results=maxr, want_positions=True)
        exp = [_oracle_protein(oracle, oix, s, ratio, mink, maxr) for s in seqs]
        assert sum(e is not None for e in exp) >= 5
        _check_top(top, exp)


def test_query_longer_than_65535_kmers(klib, oracle, gpu_device):
    from kaamer_amd import api, workload
    db = workload.make_db(3000, seed=21)
    ix = api.Index.from_image(api.Image.from_proteins(packed=db), gpu_device)
    oix = oracle.Index.from_proteins(None, packed=db)
    recs = workload.unpack(db)
    rng = np.random.default_rng(5)
    long_q = b"".join(recs[int(i)] for i in rng.integers(0, len(recs), 260))
    assert len(long_q) - 6 > 70000
    seqs = [recs[3], long_q, recs[17][:40], long_q[1000:70000]]
    top = ix.search_top(seqs, min_k_ratio=0.0, min_k_match=1, max_results=70, want_positions=True)
    exp = [_oracle_protein(oracle, oix, s, 0.0, 1, 70) for s in seqs]
    assert exp[1][0] > 65535 and len(exp[1][1]) == 70
    _check_top(top, exp)


def _oracle_reads(oracle, oix, reads, ratio, mink, maxr):
    """the literal flow of test_device_topn_reads; per ORF: None, or (untrimmed SizeInKmer, pids, Kmatch, rows, trim)"""
    from kaamer_amd import workload
    out = []
    for read in workload.unpack(reads):
        for o in oracle.get_orfs(read):
            size = oracle.size_in_kmer(o["seq"])
            pid, km, pos = oix.search(o["seq"], size=size, want_positions=True)
            if len(km) == 0 or km[0] < mink:
                out.append(None)
                continue
            et, esp, eso = oracle.set_best_start_codon(km, pos, size, o["starts"], o["plus"], o["seq"], o["start"])
            keep = oracle.filter_results(km, eso, ratio, mink, maxr)
            if not keep:
                out.append(None)
                continue
            out.append((size, pid[:keep].tolist(), km[:keep].tolist(), [np.asarray(pos[h], dtype=bool) for h in range(keep)], int(et)))
    return out


def test_reads(small, oracle):
    from kaamer_amd import abi, workload
    db, ix, oix = small
    reads = workload.make_reads(db, 400, seed=31)
    n_trimmed = 0
    for (ratio, mink, maxr) in ((0.05, 10, 10), (0.0, 1, 2)):
        plain = ix.search_top(packed=reads, seq_type=abi.READS, min_k_ratio=ratio, min_k_match=mink, max_results=maxr)
        top = ix.search_top(packed=reads, seq_type=abi.READS, min_k_ratio=ratio, min_k_match=mink, max_results=maxr, want_positions=True)
        _same_hits(top, plain)
        exp = _oracle_reads(oracle, oix, reads, ratio, mink, maxr)
        assert top.n_queries == len(exp)
        _check_top(top, [e[:4] if e else None for e in exp])
        for i, q in enumerate(top.rep_query.tolist()):
            size, pid, km, rows, et = exp[q]
            assert int(top.trim[i]) == et
            if et > 0:                                   # SetBestStartCodon trimmed it: the bitmaps keep the untrimmed frame
                n_trimmed += 1
                assert int(top.meta["size_in_kmer"][i]) < int(top.pos_bits_len[i]) == size
            a = int(top.top_off[i])
            for h, bits in enumerate(top.positions(i).values()):
                assert int(np.argmax(bits)) == int(top.top_first_pos[a + h])
    assert n_trimmed >= 1


def test_device_resident_form(small, oracle):
    """on its own stream, and with the counting stage on a count stream"""
    import torch
    from kaamer_amd import api
    db, ix, oix = small
    seqs = _mix(db)
    buf, offs = api.pack_sequences(seqs)
    d_buf = torch.from_numpy(buf).cuda()
    d_off = torch.from_numpy(offs.view(np.int64)).cuda()
    torch.cuda.synchronize()
    own, cnt_stream = torch.cuda.Stream(), torch.cuda.Stream()
    n = len(seqs)
    for split in (False, True):
        ws = api.Workspace(ix, len(buf), n, first_pos=1)
        if split:
            ws.set_count_stream(cnt_stream.cuda_stream)
        st = own.cuda_stream
        for (ratio, mink, maxr) in OPTS:
            ws.search_device(d_buf.data_ptr(), d_off.data_ptr(), n, len(buf), stream=st)
            t = ws.topn_device(ratio, mink, maxr, stream=st)
            r = ws.topn_positions_device(t, stream=st)
            ws.finish(st)
            cnt = _dev(t.d_top_cnt, n, np.uint32)
            pid = _dev(t.d_top_pid, n * maxr, np.uint32).reshape(n, maxr)
            base = _dev(r.d_pos_base, n + 1, np.uint64)
            blen = _dev(r.d_pos_bits_len, n, np.int32)
            bits = _dev(r.d_pos_bits, int(base[n]), np.uint64)
            assert int(base[n]) <= r.pos_words_capacity
            for q, s in enumerate(seqs):
                e = _oracle_protein(oracle, oix, s, ratio, mink, maxr)
                if e is None:
                    assert cnt[q] == 0 and blen[q] == 0 and base[q + 1] == base[q]
                    continue
                size, epid, ekm, rows = e
                assert cnt[q] == len(epid) and pid[q, :len(epid)].tolist() == epid and blen[q] == size
                nw = (size + 63) // 64
                assert int(base[q + 1] - base[q]) == len(epid) * nw
                for h in range(len(epid)):
                    w = bits[int(base[q]) + h * nw:int(base[q]) + (h + 1) * nw]
                    got = np.unpackbits(w.view(np.uint8), bitorder="little")[:size].astype(bool)
                    assert np.array_equal(got, rows[h]), (split, q, h)
        ws.close()


def test_submit_in_flight_and_stream(small, oracle):
    from kaamer_amd import abi, api, workload
    db, ix, oix = small
    batches = [workload.make_protein_queries(db, 30, seed=40 + i) for i in range(4)]
    one_shot = [ix.search_top(packed=b, want_positions=True) for b in batches]
    tickets = [ix.submit_top(packed=b, want_positions=True) for b in batches]     # four in flight
    for i in (2, 0, 3, 1):                                                        # waited for out of order
        _same_positions(tickets[i].wait(), one_shot[i])
    t = ix.submit_top(packed=batches[0], want_positions=True)
    t.discard()
    # the stream form: more chunks than slots
    reads = workload.make_reads(db, 420, seed=77)
    recs = workload.unpack(reads)
    chunks = [api.pack_sequences(recs[i:i + 60]) for i in range(0, 420, 60)]
    assert len(chunks) >= 6
    st = ix.stream(seq_type=abi.READS, want_positions=True)
    got, pushed = [], 0
    while len(got) < len(chunks):
        if pushed < len(chunks) and st.push(*chunks[pushed]):
            pushed += 1
            continue
        got.append(st.pop())
    st.close()
    n_rep = 0
    for c, g in zip(chunks, got):
        ref = ix.search_top(packed=c, seq_type=abi.READS, want_positions=True)
        _same_positions(g, ref)
        n_rep += g.n_reported
    assert n_rep > 50


def test_capacity(small, oracle):
    """a bitmap bound that is too small: the host call repeats the batch and returns the full result; the device-resident
    form reports KAAMER_E_CAPACITY and no partial result"""
    import torch
    from kaamer_amd import abi, api
    db, ix, oix = small
    seqs = _mix(db)
    ref = ix.search_top(seqs, want_positions=True)
    assert len(ref.pos_bits) > 100
    ix.set_top_positions_bound(3)
    try:
        small_first = ix.search_top(seqs, want_positions=True)
        t = ix.submit_top(seqs, want_positions=True)
        _same_positions(t.wait(), ref)
    finally:
        ix.set_top_positions_bound(0)
    _same_positions(small_first, ref)
    _check_top(small_first, [_oracle_protein(oracle, oix, s, 0.05, 10, 10) for s in seqs])
    buf, offs = api.pack_sequences(seqs)
    d_buf = torch.from_numpy(buf).cuda()
    d_off = torch.from_numpy(offs.view(np.int64)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    ws = api.Workspace(ix, len(buf), len(seqs), first_pos=1)
    ws.search_device(d_buf.data_ptr(), d_off.data_ptr(), len(seqs), len(buf), stream=st)
    t = ws.topn_device(stream=st)
    r = ws.topn_positions_device(t, max_pos_words=len(ref.pos_bits) - 1, stream=st)
    with pytest.raises(abi.KaamerError) as ei:
        ws.finish(st)
    assert ei.value.code == abi.E_CAPACITY
    assert r.pos_words_capacity == len(ref.pos_bits) - 1
    # exactly enough is enough
    ws.search_device(d_buf.data_ptr(), d_off.data_ptr(), len(seqs), len(buf), stream=st)
    t = ws.topn_device(stream=st)
    r = ws.topn_positions_device(t, max_pos_words=len(ref.pos_bits), stream=st)
    ws.finish(st)
    base = _dev(r.d_pos_base, len(seqs) + 1, np.uint64)
    assert int(base[-1]) == len(ref.pos_bits)
    assert np.array_equal(_dev(r.d_pos_bits, len(ref.pos_bits), np.uint64), ref.pos_bits)


def test_merge_workspace_is_refused_and_plain_results_have_no_positions(small, klib):
    import torch
    from kaamer_amd import abi, api
    db, ix, oix = small
    st = torch.cuda.current_stream().cuda_stream
    ws = api.Workspace(ix, 4096, 8, first_pos=1, max_hits=1 << 16)
    ent_off = torch.tensor([0, 1, 2], dtype=torch.int64).cuda()
    pid = torch.tensor([5, 9], dtype=torch.int32).cuda()
    km = torch.tensor([3, 4], dtype=torch.int32).cuda()
    fp = torch.tensor([0, 1], dtype=torch.int32).cuda()
    size = torch.tensor([20, 30], dtype=torch.int32).cuda()
    ws.merge_device(ent_off.data_ptr(), pid.data_ptr(), km.data_ptr(), fp.data_ptr(), 2, 2, stream=st)
    t = ws.topn_device(0.0, 1, 10, d_size_in_kmer_ptr=size.data_ptr(), stream=st)
    ws.finish(st)
    with pytest.raises(abi.KaamerError) as ei:
        ws.topn_positions_device(t, stream=st)
    assert ei.value.code == abi.E_ARG
    # kaamer_batch_top_positions on a result without positions: NULLs
    buf, offs = api.pack_sequences(_mix(db))
    out = C.POINTER(abi.BatchTop)()
    abi.check(klib.kaamer_search_batch_top_flat(ix._h, buf.ctypes.data, offs.ctypes.data, len(offs) - 1, abi.PROTEIN, 0.05, 10, 10, C.byref(out)))
    pl, po, pb = C.POINTER(C.c_int32)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
    pl2, po2, pb2 = C.POINTER(C.c_int32)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
    try:
        assert out.contents.n_reported > 0
        abi.check(klib.kaamer_batch_top_positions(out, C.byref(pl), C.byref(po), C.byref(pb)))
        assert not bool(pl) and not bool(po) and not bool(pb)
    finally:
        klib.kaamer_batch_top_free(out)
    out = C.POINTER(abi.BatchTop)()
    abi.check(klib.kaamer_search_batch_top_pos_flat(ix._h, buf.ctypes.data, offs.ctypes.data, len(offs) - 1, abi.PROTEIN, 0.05, 10, 10, C.byref(out)))
    try:
        abi.check(klib.kaamer_batch_top_positions(out, C.byref(pl2), C.byref(po2), C.byref(pb2)))
        assert bool(pl2) and bool(po2) and bool(pb2)
    finally:
        klib.kaamer_batch_top_free(out)


def test_formatted_end_to_end(small, oracle, klib):
    """kaamer_format_positions of each reported bitmap == FormatPositionsToString restated, on the oracle's row"""
    db, ix, oix = small
    seqs = _mix(db)
    top = ix.search_top(seqs, want_positions=True)
    n = 0
    for i, q in enumerate(top.rep_query.tolist()):
        size, pid, km, rows = _oracle_protein(oracle, oix, seqs[q], 0.05, 10, 10)
        nw = (size + 63) // 64
        for h, e in enumerate(range(int(top.top_off[i]), int(top.top_off[i + 1]))):
            w = np.ascontiguousarray(top.pos_bits[int(top.pos_off[e]):int(top.pos_off[e]) + nw])
            for wa in (0, 1):
                want = format_positions_ref(rows[h].tolist(), bool(wa)).encode()
                buf = C.create_string_buffer(len(want) + 8)
                assert klib.kaamer_format_positions(w.ctypes.data, size, wa, buf, len(want) + 8) == len(want)
                assert buf.value == want
                n += 1
    assert n > 200
