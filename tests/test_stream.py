"""Streaming driver (chunks of a host batch, double-buffered H2D copies): same reported hits as one
batch through the host-buffer call."""
import numpy as np
import pytest

def test_chunk_bounds_cpu_logic():
    from kaamer_amd.stream import chunk_bounds
    offs = np.cumsum([0] + [150] * 10 + [1000, 20, 0, 0, 150]).astype(np.uint64)
    ch = chunk_bounds(offs, max_seqs=4, max_bytes=1000)
    assert ch[0] == (0, 4) and ch[-1][1] == len(offs) - 1
    assert all(b > a and b - a <= 4 and int(offs[b] - offs[a]) <= 1000 for a, b in ch)
    assert [a for a, _ in ch[1:]] == [b for _, b in ch[:-1]]
    with pytest.raises(ValueError):
        chunk_bounds(offs, max_seqs=4, max_bytes=999)


@pytest.mark.gpu
def test_streamed_reads_equal_one_batch(klib, gpu_device):
    from kaamer_amd import abi, api, stream, workload
    db = workload.make_db(2000, seed=4)
    ix = api.Index.from_image(api.Image.from_proteins(packed=db), gpu_device)
    reads = workload.make_reads(db, 3000, seed=8)
    buf, offs = reads
    ref = ix.search_top(packed=reads, seq_type=abi.READS)
    got_cnt, got_pid, got_km = [], [], []

    def on_chunk(first, n, top):
        pid, km = top.dense()
        assert top.n_reported == int((top.top_cnt > 0).sum())
        got_cnt.append(top.top_cnt.copy()); got_pid.append(pid); got_km.append(km)

    for n_buf in (1, 3, 6):   # 6 > the library's slots: push reports busy and the driver pops first
        got_cnt, got_pid, got_km = [], [], []
        s = stream.StreamingSearcher(ix, max_chunk_seqs=700, max_chunk_bytes=64 * 1024, n_buffers=n_buf)
        total = s.run(buf, offs, on_chunk)
        s.close()
        assert len(got_cnt) >= 5                                       # several chunks, the slots reused
        cnt = np.concatenate(got_cnt); pid = np.concatenate(got_pid); km = np.concatenate(got_km)
        assert total["n_queries"] == ref.n_queries == len(cnt)
        assert total["n_lookup"] == ref.counters["n_lookup"] and total["n_hits"] == ref.counters["n_hits"]
        assert (cnt == ref.top_cnt).all()
        rpid, rkm = ref.dense()
        for q in range(ref.n_queries):
            k = int(cnt[q])
            assert pid[q, :k].tolist() == rpid[q, :k].tolist() and km[q, :k].tolist() == rkm[q, :k].tolist()


@pytest.mark.gpu
def test_concurrent_callers_and_tickets(klib, oracle, gpu_device):
    """the worker pool of search_protein.go:58-118 against one index: N threads call kaamer_search_batch_top at once
    (each on a slot of its own), and one thread keeps several tickets in flight; every result vs the oracle"""
    import threading
    from kaamer_amd import abi, api, workload
    db = workload.make_db(1500, seed=4)
    ix = api.Index.from_image(api.Image.from_proteins(packed=db), gpu_device)
    oix = oracle.Index.from_proteins(None, packed=db)
    batches = [workload.make_protein_queries(db, 60 + 7 * i, seed=20 + i) for i in range(6)] + \
              [workload.make_reads(db, 150 + 10 * i, seed=40 + i) for i in range(3)]
    kinds = [abi.PROTEIN] * 6 + [abi.READS] * 3

    def expected(q, kind):
        out = []
        for s in workload.unpack(q):
            items = [dict(seq=s)] if kind == abi.PROTEIN else oracle.get_orfs(s)
            for o in items:
                seq = o["seq"]
                size = oracle.size_in_kmer(seq)
                if kind == abi.PROTEIN and size < 7:
                    out.append([])
                    continue
                pid, km, pos = oix.search(seq, want_positions=True)
                keep = 0
                if kind == abi.PROTEIN:
                    keep = oracle.filter_results(km, size) if len(km) else 0
                elif len(km) and km[0] >= 10:
                    _, _, size2 = oracle.set_best_start_codon(km, pos, size, o["starts"], o["plus"], seq, o["start"])
                    keep = oracle.filter_results(km, size2)
                out.append(list(zip(pid[:keep].tolist(), km[:keep].tolist())))
        return out

    exp = [expected(q, k) for q, k in zip(batches, kinds)]

    def check(top, e):
        pid, km = top.dense()
        assert top.n_queries == len(e)
        for i, rep in enumerate(e):
            k = int(top.top_cnt[i])
            assert list(zip(pid[i, :k].tolist(), km[i, :k].tolist())) == rep, i

    errors = []

    def worker(i):
        try:
            for r in range(4):
                j = (i + r) % len(batches)
                check(ix.search_top(packed=batches[j], seq_type=kinds[j]), exp[j])
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=worker, args=(i,)) for i in range(8)]   # more threads than slots: some wait for one
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    # tickets: four batches in flight from one thread, waited for in another order
    tk = [ix.submit_top(packed=batches[j], seq_type=kinds[j]) for j in (0, 6, 1, 7)]
    for t, j in sorted(zip(tk, (0, 6, 1, 7)), key=lambda x: -x[1]):
        check(t.wait(), exp[j])


@pytest.mark.gpu
def test_concurrent_full_hit_list_callers(klib, oracle, gpu_device):
    """kaamer_search_batch (full hit lists, positions on request) from eight threads at once on one index: every call
    takes a slot of its own (workspace, staging, stream) -- more threads than slots, protein and read batches mixed, so
    slots are re-made for the other kind while others run -- and every result equals the oracle's"""
    import threading
    from kaamer_amd import abi, api, workload
    db = workload.make_db(1200, seed=14)
    ix = api.Index.from_image(api.Image.from_proteins(packed=db), gpu_device)
    oix = oracle.Index.from_proteins(None, packed=db)
    batches = [workload.make_protein_queries(db, 40 + 9 * i, seed=120 + i) for i in range(5)] + \
              [workload.make_reads(db, 120 + 10 * i, seed=140 + i) for i in range(3)]
    kinds = [abi.PROTEIN] * 5 + [abi.READS] * 3

    def expected(q, kind):
        out = []
        for s in workload.unpack(q):
            for seq in ([s] if kind == abi.PROTEIN else [o["seq"] for o in oracle.get_orfs(s)]):
                if oracle.size_in_kmer(seq) < 7:
                    out.append(({}, {}))
                    continue
                pid, km, pos = oix.search(seq, want_positions=True)
                out.append((dict(zip(pid.tolist(), km.tolist())), {int(p): int(np.argmax(pos[j])) for j, p in enumerate(pid)}))
        return out

    exp = [expected(q, k) for q, k in zip(batches, kinds)]
    errors = []

    def worker(i):
        try:
            for r in range(3):
                j = (i + 3 * r) % len(batches)
                res = ix.search(packed=batches[j], seq_type=kinds[j], want_positions=(i + r) % 4 == 0)
                assert res.n_queries == len(exp[j]), (res.n_queries, len(exp[j]))
                for q, (hits, fp) in enumerate(exp[j]):
                    assert res.hits(q) == hits, (j, q)
                    assert res.first_pos(q) == fp, (j, q)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=worker, args=(i,)) for i in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[:3]


@pytest.mark.gpu
def test_flat_entry_points_equal_the_struct_forms(klib, gpu_device):
    """The cgo-safe forms (every caller buffer a direct argument: include/kaamer_hip.h) return what the
    struct forms return -- kaamer_search_batch_flat, kaamer_search_batch_top_flat, kaamer_submit_batch_top_flat,
    kaamer_stream_open_flat -- for protein and read batches."""
    import ctypes as C
    from kaamer_amd import abi, api, workload
    db = workload.make_db(800, seed=14)
    ix = api.Index.from_image(api.Image.from_proteins(packed=db), gpu_device)
    for q, kind in ((workload.make_protein_queries(db, 90, seed=3), abi.PROTEIN), (workload.make_reads(db, 200, seed=5), abi.READS)):
        a, b = ix.search(packed=q, seq_type=kind, flat=True), ix.search(packed=q, seq_type=kind, flat=False)
        assert a.n_queries == b.n_queries and a.n_queries > 50
        assert all(a.hits(i) == b.hits(i) for i in range(a.n_queries))
        ta, tb = ix.search_top(packed=q, seq_type=kind, flat=True), ix.search_top(packed=q, seq_type=kind, flat=False)
        tc, td = ix.submit_top(packed=q, seq_type=kind, flat=True).wait(), ix.submit_top(packed=q, seq_type=kind, flat=False).wait()
        # the stream opened with flat options
        h = C.c_void_p()
        abi.check(klib.kaamer_stream_open_flat(ix._h, kind, 0.05, 10, 10, C.byref(h)))
        buf, offs = np.ascontiguousarray(q[0]), np.ascontiguousarray(q[1])
        abi.check(klib.kaamer_stream_push(h, buf.ctypes.data, offs.ctypes.data, len(offs) - 1))
        out = C.POINTER(abi.BatchTop)()
        abi.check(klib.kaamer_stream_pop(h, C.byref(out)))
        te = api.TopResult(out)
        klib.kaamer_batch_top_free(out)
        klib.kaamer_stream_close(h)
        assert ta.n_reported > 20
        for t in (tb, tc, td, te):
            assert t.rep_query.tolist() == ta.rep_query.tolist() and t.top_off.tolist() == ta.top_off.tolist()
            assert t.top_pid.tolist() == ta.top_pid.tolist() and t.top_kmatch.tolist() == ta.top_kmatch.tolist()
            assert t.trim.tolist() == ta.trim.tolist()


@pytest.mark.gpu
def test_discarded_tickets_give_their_slots_back(klib, gpu_device):
    """A ticket dropped without wait() (an exception between submit and wait) must not keep its slot busy for good:
    after more discarded tickets than there are slots a further submit still gets one, and kaamer_index_close with a
    ticket in flight waits for it instead of destroying a stream with work queued."""
    import threading
    from kaamer_amd import abi, api, workload
    db = workload.make_db(600, seed=15)
    ix = api.Index.from_image(api.Image.from_proteins(packed=db), gpu_device)
    q = workload.make_protein_queries(db, 70, seed=2)
    ref = ix.search_top(packed=q)
    for i in range(12):   # default: 4 slots
        t = ix.submit_top(packed=q)
        if i % 2:
            t.discard()
        else:
            del t         # __del__ discards
    done = []
    th = threading.Thread(target=lambda: done.append(ix.submit_top(packed=q).wait()))
    th.start()
    th.join(60)
    assert done and done[0].top_pid.tolist() == ref.top_pid.tolist()
    # close while a ticket is in flight: close() waits until another thread has waited for the ticket
    t = ix.submit_top(packed=q)
    res = []
    th = threading.Thread(target=lambda: (__import__("time").sleep(0.3), res.append(t.wait())))
    th.start()
    ix.close()
    th.join(60)
    assert res and res[0].top_pid.tolist() == ref.top_pid.tolist()


@pytest.mark.gpu
def test_four_callers_after_warm_up_are_not_slower_than_two(klib, gpu_device):
    """Round 3's bench reported 120 ms per call with exactly four concurrent callers against 20 with two and 12 with eight:
    the four-caller case was the first to touch slots 2 and 3, and a slot allocates its workspace and pinned staging at
    first use.  With every slot warmed, four callers must not cost more per call than two (loose bound: timing)."""
    import threading
    import time
    from kaamer_amd import abi, api, workload
    db = workload.make_db(3000, seed=21)
    ix = api.Index.from_image(api.Image.from_proteins(packed=db), gpu_device)
    q = workload.make_reads(db, 200000, seed=22)

    def run(n_thr, per):
        def worker():
            for _ in range(per):
                ix.search_top(packed=q, seq_type=abi.READS)
        th = [threading.Thread(target=worker) for _ in range(n_thr)]
        t0 = time.perf_counter()
        for t in th:
            t.start()
        for t in th:
            t.join()
        return (time.perf_counter() - t0) / (n_thr * per)

    run(4, 1)                      # every slot allocates here
    t2, t4 = run(2, 4), run(4, 4)
    assert t4 < 2.0 * t2 + 0.005, "per call: 2 callers %.1f ms, 4 callers %.1f ms" % (t2 * 1e3, t4 * 1e3)


@pytest.mark.gpu
def test_counting_stage_on_its_own_stream(klib, oracle, gpu_device):
    """kaamer_workspace_set_count_stream: prep + probe on the caller's stream, the counting tiers (and the post-steps) on a
    second one, ordered by events inside the library; several batches in a row on two workspaces that share one probe
    stream, protein and reads; results against the oracle, and kaamer_workspace_finish waits for the stage wherever it ran"""
    import torch
    from kaamer_amd import abi, api, workload
    db = workload.make_db(1200, seed=9)
    ix = api.Index.from_image(api.Image.from_proteins(packed=db), gpu_device)
    oix = oracle.Index.from_proteins(None, packed=db)
    probe, c1, c2 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    for kind, make in ((abi.PROTEIN, lambda s: workload.make_protein_queries(db, 120, seed=s)), (abi.READS, lambda s: workload.make_reads(db, 400, seed=s))):
        batches = [make(30 + i) for i in range(4)]
        size = max(len(b[0]) for b in batches)
        wss = [api.Workspace(ix, size, 400, seq_type=kind) for _ in range(2)]
        wss[0].set_count_stream(c1.cuda_stream)
        wss[1].set_count_stream(c2.cuda_stream)
        d = [(torch.from_numpy(b[0]).cuda(), torch.from_numpy(b[1].view(np.int64)).cuda()) for b in batches]
        torch.cuda.synchronize()
        for rep in range(2):
            for i, b in enumerate(batches):
                w = wss[i % 2]
                r = w.search_device(d[i][0].data_ptr(), d[i][1].data_ptr(), len(b[1]) - 1, len(b[0]), stream=probe.cuda_stream)
                if i >= 2:      # the last batch of each workspace is checked; earlier ones are overwritten in flight
                    top = w.topn_device(0.05, 10, 10, best_start_codon=(kind == abi.READS), stream=probe.cuda_stream)
                    c = w.finish(probe.cuda_stream)
                    nq = int(c["n_queries"])
                    from kaamer_amd.sharded import dev_tensor
                    off = dev_tensor(r.d_hit_off, nq, torch.int64).cpu().numpy()
                    cnt = dev_tensor(r.d_hit_cnt, nq, torch.int32).cpu().numpy()
                    pid = dev_tensor(r.d_hit_pid, int(r.hit_capacity), torch.int32).cpu().numpy().view(np.uint32)
                    km = dev_tensor(r.d_hit_kmatch, int(r.hit_capacity), torch.int32).cpu().numpy()
                    seqs = workload.unpack(b)
                    queries = [o["seq"] for s in seqs for o in oracle.get_orfs(s)] if kind == abi.READS else [s for s in seqs]
                    assert nq == len(queries)
                    n = 0
                    for qi, qs in enumerate(queries):
                        exp = {}
                        if kind == abi.READS or oracle.size_in_kmer(qs) >= 7:
                            p_, k_, _ = oix.search(qs)
                            exp = dict(zip(p_.tolist(), k_.tolist()))
                        a = int(off[qi])
                        assert dict(zip(pid[a:a + int(cnt[qi])].tolist(), km[a:a + int(cnt[qi])].tolist())) == exp, (kind, i, qi)
                        n += len(exp)
                    assert n > 100
        for w in wss:
            w.set_count_stream(None)
            w.close()


@pytest.mark.gpu
def test_full_hit_lists_in_two_halves(klib, oracle, gpu_device):
    """kaamer_submit_batch_flat / kaamer_wait_batch: the full-hit-list call (what -pos needs: PositionHits) with several
    batches in flight from one thread, more tickets than slots over time, a discarded ticket; every result equals the
    blocking call's, bitmaps included, and a sample the oracle's"""
    from kaamer_amd import abi, api, workload
    db = workload.make_db(900, seed=19)
    ix = api.Index.from_image(api.Image.from_proteins(packed=db), gpu_device)
    oix = oracle.Index.from_proteins(None, packed=db)
    batches = [(workload.make_protein_queries(db, 80 + 5 * i, seed=50 + i), abi.PROTEIN) for i in range(4)] + \
              [(workload.make_reads(db, 150, seed=70 + i), abi.READS) for i in range(2)]
    refs = [ix.search(packed=q, seq_type=k, want_positions=True) for q, k in batches]
    tickets = [ix.submit(packed=q, seq_type=k, want_positions=True) for q, k in batches[:3]]   # three of the four slots
    ix.submit(packed=batches[3][0], seq_type=batches[3][1]).discard()
    got = [t.wait() for t in tickets]
    got += [ix.submit(packed=q, seq_type=k, want_positions=True).wait() for q, k in batches[3:]]
    for r, g in zip(refs, got):
        assert g.n_queries == r.n_queries
        for i in range(r.n_queries):
            assert g.hits(i) == r.hits(i) and g.first_pos(i) == r.first_pos(i)
        for i in range(0, r.n_queries, 7):
            assert g.positions(i).keys() == r.positions(i).keys()
            for p_ in g.positions(i):
                assert np.array_equal(g.positions(i)[p_], r.positions(i)[p_])
    seqs = workload.unpack(batches[0][0])
    for i in range(0, len(seqs), 9):
        exp = {}
        if oracle.size_in_kmer(seqs[i]) >= 7:
            p_, k_, _ = oix.search(seqs[i])
            exp = dict(zip(p_.tolist(), k_.tolist()))
        assert got[0].hits(i) == exp


@pytest.mark.gpu
def test_full_hit_lists_in_two_halves_grow_their_bounds(klib, oracle, gpu_device):
    """a skewed database (the one of test_zipf_database_parity): a query has thousands of hits, so the bounds a full-list
    call starts from (8 hits per input byte) are too small and kaamer_wait_batch repeats the batch with grown bounds
    from its copy of the input; every {protein id -> Kmatch} and first position vs the oracle"""
    from kaamer_amd import api, workload
    db = workload.make_db_zipf(40000, seed=11, n_motifs=1500, zipf_a=1.0, per_residues=60)
    ix = api.Index.from_image(api.Image.from_proteins(packed=db), gpu_device)
    oix = oracle.Index.from_proteins(None, packed=db)
    q = workload.make_protein_queries(db, 200, seed=12)
    seqs = workload.unpack(q)
    res = ix.submit(packed=q).wait()
    assert res.n_queries == len(seqs)
    # more than the first attempt's hit arrays hold (a fresh slot's workspace: the bound plus a quarter of headroom)
    assert res.counters["n_hits"] > (8 * len(q[0]) + 65536) * 5 // 4
    for i, s in enumerate(seqs):
        exp, fp = {}, {}
        if oracle.size_in_kmer(s) >= 7:
            pid, km, pos = oix.search(s, want_positions=True)
            exp = dict(zip(pid.tolist(), km.tolist()))
            fp = {int(p): int(np.argmax(pos[j])) for j, p in enumerate(pid)}
        assert res.hits(i) == exp, "query %d" % i
        assert res.first_pos(i) == fp, "query %d" % i

