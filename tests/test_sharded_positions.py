"""Full hit lists and PositionHits on a sharded index: exchange blocks with bitmaps (arrays = 4), the one-process handle's
kaamer_sharded_search_batch*, and ShardedSearcher(want_positions=True).  The reference fills PositionHits for every reported
hit under -pos (search.go:416,442-452), whatever the database size: the sharded result must equal the unsharded
kaamer_search_batch bit for bit."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

NEW_SYMBOLS = ("kaamer_exchange_layout_init_positions", "kaamer_exchange_layout_fit_positions", "kaamer_exchange_stats_positions",
               "kaamer_sharded_search_batch", "kaamer_sharded_search_batch_flat", "kaamer_sharded_submit_batch_flat",
               "kaamer_sharded_wait_batch", "kaamer_sharded_full_ticket_discard")


def _bits_off(L):
    return (8 + 2 * L.q_cap + 3 * L.e_cap + 1) & ~1


# ---------------------------------------------------------------- host only
def test_new_symbols_declared_and_exported(klib):
    with open(os.path.join(ROOT, "include", "kaamer_hip.h")) as f:
        hdr = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(klib, name), name


def test_layout_positions_arithmetic(klib):
    from kaamer_amd import abi, sharded
    L = abi.lib()
    cap = abi.ExchangeLayout()
    abi.check(L.kaamer_exchange_layout_init_positions(3, 1, 1000, 5000, 12345, C.byref(cap)))
    assert (cap.world, cap.rank, cap.arrays) == (3, 1, 4)
    assert cap.q_cap == (1000 + 2) // 3 + 1 and cap.e_cap == 5000
    off = _bits_off(cap)
    assert off % 2 == 0 and cap.block_words % 4 == 0
    p_cap = (cap.block_words - off) // 2
    assert 12345 <= p_cap <= 12345 + 2
    assert sharded.pos_words_of(cap) == p_cap
    # one batch's blocks: cut to what it needs, never beyond the capacity
    fit = abi.ExchangeLayout()
    abi.check(L.kaamer_exchange_layout_fit_positions(C.byref(cap), 30, 201, 301, C.byref(fit)))
    assert fit.arrays == 4 and fit.q_cap == 11 and fit.e_cap == 204
    pw = sharded.pos_words_of(fit)
    assert 301 <= pw <= 304 and fit.block_words <= cap.block_words
    assert fit.block_words == (_bits_off(fit) + 2 * 301 + 3) & ~3
    abi.check(L.kaamer_exchange_layout_fit_positions(C.byref(cap), 1 << 30, 1 << 40, 1 << 40, C.byref(fit)))
    assert (fit.q_cap, fit.e_cap, fit.block_words) == (cap.q_cap, cap.e_cap, cap.block_words)
    abi.check(L.kaamer_exchange_layout_fit_positions(C.byref(cap), 30, 201, 1 << 40, C.byref(fit)))
    assert sharded.pos_words_of(fit) <= p_cap + 1 and fit.block_words <= cap.block_words
    # bad arguments
    assert L.kaamer_exchange_layout_init_positions(3, 1, 1000, 5000, 0, C.byref(cap)) == abi.E_ARG
    assert L.kaamer_exchange_layout_init_positions(3, 3, 1000, 5000, 10, C.byref(cap)) == abi.E_ARG
    assert L.kaamer_exchange_layout_init_positions(0, 0, 1000, 5000, 10, C.byref(cap)) == abi.E_ARG
    assert L.kaamer_exchange_layout_init_positions(2, 0, 1000, 5000, 1 << 40, C.byref(cap)) == abi.E_ARG
    old = abi.ExchangeLayout()
    abi.check(L.kaamer_exchange_layout_init(3, 1, 1000, 5000, C.byref(old)))
    assert L.kaamer_exchange_layout_fit_positions(C.byref(old), 30, 201, 301, C.byref(fit)) == abi.E_ARG
    assert L.kaamer_exchange_layout_fit_positions(None, 30, 201, 301, C.byref(fit)) == abi.E_ARG
    assert L.kaamer_exchange_stats_positions(None, 0, (C.c_uint64 * 2)()) == abi.E_ARG
    # the arrays = 3 layout is what it was
    assert (old.arrays, old.q_cap, old.e_cap) == (3, 335, 5000)
    assert old.block_words == (8 + old.q_cap + 3 * old.e_cap + 3) & ~3
    assert sharded.pos_words_of(old) == 0
    assert C.sizeof(abi.ExchangeLayout) == 32


# ---------------------------------------------------------------- GPU
def _positions_equal(got, ref, q):
    a, b = got.positions(q), ref.positions(q)
    assert sorted(a) == sorted(b), q
    for p, bits in b.items():
        assert np.array_equal(a[p], bits), (q, p)
    return a


def _check_full(got, ref, positions, reads=False, oix=None, queries=None):
    """got (sharded) == ref (unsharded kaamer_search_batch): hit sets, query data, bitmaps, counters"""
    assert got.n_queries == ref.n_queries
    for f in ("src_seq", "size_in_kmer", "start_position", "end_position", "plus_strand", "aa_len", "aa_off", "sa_off", "sa_len"):
        assert got.meta[f].tolist() == ref.meta[f].tolist(), f
    if reads:
        assert bytes(got.orf_aa) == bytes(ref.orf_aa)
        assert got.starts_alt.tolist() == ref.starts_alt.tolist()
    assert got.hit_cnt.tolist() == ref.hit_cnt.tolist()
    n = 0
    for q in range(ref.n_queries):
        a, b = got.span(q)
        c, d = ref.span(q)
        gs = sorted(zip(got.hit_pid[a:b].tolist(), got.hit_kmatch[a:b].tolist(), got.hit_first_pos[a:b].tolist()))
        rs = sorted(zip(ref.hit_pid[c:d].tolist(), ref.hit_kmatch[c:d].tolist(), ref.hit_first_pos[c:d].tolist()))
        assert gs == rs, q
        n += len(gs)
        if positions:
            pos = _positions_equal(got, ref, q)
            km = got.hits(q)
            for p, bits in pos.items():
                assert int(bits.sum()) == km[p], (q, p)
            if oix is not None and queries is not None and q % 7 == 0 and len(queries[q]) >= 7:
                pid, _, opos = oix.search(queries[q], want_positions=True)
                for j, p in enumerate(pid.tolist()):
                    assert pos[p].tolist() == opos[j].tolist(), (q, p)
        else:
            assert got.pos_off is None and got.pos_bits is None
    for k in ("n_in", "n_queries", "n_lookup", "n_post", "n_found", "n_hits"):
        assert got.counters[k] == ref.counters[k], k
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("reads", [False, True], ids=["protein", "reads"])
def test_sharded_full_lists_equal_unsharded(klib, oracle, gpu_device, reads):
    from kaamer_amd import abi, api, workload
    db = workload.make_db(600, seed=6)
    oix = oracle.Index.from_proteins(None, packed=db)
    if reads:
        q = workload.make_reads(db, 300, seed=12)
        seq_type, queries = abi.READS, None
    else:
        queries = workload.unpack(workload.make_protein_queries(db, 150, seed=7)) + [max(workload.unpack(db), key=len), b"AAAAAAA", b""]
        q = api.pack_sequences(queries)
        seq_type = abi.PROTEIN
    ix1 = api.Index.from_image(api.Image.from_proteins(packed=db), gpu_device)
    refs = {wp: ix1.search(packed=q, seq_type=seq_type, want_positions=wp) for wp in (False, True)}
    for world in (1, 2, 3, 8):
        sx = api.ShardedIndex.from_images([api.Image.from_proteins(packed=db, shard=r, n_shards=world) for r in range(world)],
                                          [gpu_device] * world)
        for wp in (False, True):
            for rep in range(3):   # flat, struct, submit/wait: the second and third size their blocks from the call before
                if rep == 2:
                    got = sx.submit(packed=q, seq_type=seq_type, want_positions=wp).wait()
                else:
                    got = sx.search(packed=q, seq_type=seq_type, want_positions=wp, flat=(rep == 0))
                assert sx.exchange_info()["adaptive"] == (rep > 0), (world, wp, rep)
                n = _check_full(got, refs[wp], wp, reads=reads, oix=oix, queries=queries)
                assert n > 300
        sx.close()


@pytest.mark.gpu
def test_sharded_positions_g_tier_and_long_query(klib, oracle, gpu_device):
    """queries with 3 000 distinct hits (the G tier on every shard; the OR-merge's HBM table) and one longer than 65 535
    k-mers, through the exchange at W = 2 and 3"""
    from kaamer_amd import api
    rng = np.random.default_rng(14)
    alpha = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    core = bytes(alpha[rng.integers(0, 20, 70)])
    db = [bytes(alpha[rng.integers(0, 20, 6)]) + core[(i % 9):] + bytes(alpha[rng.integers(0, 20, 6)]) for i in range(3000)]
    ids = rng.permutation(20000)[:3000].astype(np.uint32)
    oix = oracle.Index.from_proteins(db, ids=ids)
    seqs = [core, bytes(alpha[rng.integers(0, 20, 130)]) + core + bytes(alpha[rng.integers(0, 20, 70)]), db[11], core[:25]]
    long_q = b"".join(db[int(i)] for i in rng.integers(0, len(db), 900))
    assert len(long_q) - 6 > 65535
    seqs.append(long_q)
    ix1 = api.Index.from_image(api.Image.from_proteins(db, ids=ids), gpu_device)
    ref = ix1.search(seqs, want_positions=True)
    assert ref.counters["n_overflow"] >= 2
    for world in (2, 3):
        sx = api.ShardedIndex.from_images([api.Image.from_proteins(db, ids=ids, shard=r, n_shards=world) for r in range(world)],
                                          [gpu_device] * world)
        got = sx.search(seqs, want_positions=True)
        _check_full(got, ref, True)
        for qi in range(4):   # (the long query: against the unsharded bitmaps above)
            pid, km, pos = oix.search(seqs[qi], want_positions=True)
            g = got.positions(qi)
            if qi < 2:
                assert len(pid) == 3000
            for i, p in enumerate(pid.tolist()):
                assert g[p].tolist() == pos[i].tolist(), (world, qi, p)
        sx.close()


def _long_batch(db_recs, rng, n, k):
    return [b"".join(db_recs[int(i)] for i in rng.integers(0, len(db_recs), k)) for _ in range(n)]


@pytest.mark.gpu
def test_sharded_positions_growth_and_alternation(klib, oracle, gpu_device):
    """a batch of short queries, then as many much longer ones: the second call's bitmap section, sized from the first
    call's need, overflows and the handle repeats the batch -- the result is exact.  Top calls and full calls alternate on
    one handle, the top results unchanged."""
    from kaamer_amd import api, workload
    db = workload.make_db(600, seed=6)
    recs = workload.unpack(db)
    rng = np.random.default_rng(3)
    short = [r[:40] for r in recs[:60]]
    longer = _long_batch(recs, rng, 60, 12)
    ix1 = api.Index.from_image(api.Image.from_proteins(packed=db), gpu_device)
    sx = api.ShardedIndex.from_images([api.Image.from_proteins(packed=db, shard=r, n_shards=2) for r in range(2)], [gpu_device] * 2)
    _check_full(sx.search(short, want_positions=True), ix1.search(short, want_positions=True), True)
    _check_full(sx.search(longer, want_positions=True), ix1.search(longer, want_positions=True), True)
    qs = workload.unpack(workload.make_protein_queries(db, 100, seed=9))
    ref_top = ix1.search_top(qs)
    ref_full = ix1.search(qs, want_positions=True)
    for _ in range(2):
        top = sx.search_top(qs)
        assert top.rep_query.tolist() == ref_top.rep_query.tolist() and top.top_off.tolist() == ref_top.top_off.tolist()
        assert top.top_pid.tolist() == ref_top.top_pid.tolist() and top.top_kmatch.tolist() == ref_top.top_kmatch.tolist()
        _check_full(sx.search(qs, want_positions=True), ref_full, True)
    sx.close()


@pytest.mark.gpu
def test_sharded_calls_grow_their_bounds(klib, oracle, gpu_device):
    """a skewed database (the one of test_zipf_database_parity): a query has thousands of hits, far more than the
    exchange blocks and hit arrays of a first call hold, so the first top call and the first full call on a fresh handle
    (nothing to size the blocks from: not adaptive) each repeat their batch with every bound grown.  Reported hits and
    full hit lists equal the unsharded calls', and a sample the oracle's."""
    from kaamer_amd import api, workload
    db = workload.make_db_zipf(40000, seed=11, n_motifs=1500, zipf_a=1.0, per_residues=60)
    oix = oracle.Index.from_proteins(None, packed=db)
    q = workload.make_protein_queries(db, 200, seed=12)
    seqs = workload.unpack(q)
    ix1 = api.Index.from_image(api.Image.from_proteins(packed=db), gpu_device)
    ref_top = ix1.search_top(packed=q)
    ref_full = ix1.search(packed=q)
    images = [api.Image.from_proteins(packed=db, shard=r, n_shards=2) for r in range(2)]
    sx = api.ShardedIndex.from_images(images, [gpu_device] * 2)
    e_cap = 2 * len(q[0]) // 2 + 65536      # entries per (shard -> owner) block of a first attempt
    top = sx.search_top(packed=q)
    assert not sx.exchange_info()["adaptive"] and sx.exchange_info()["need_entries"] > e_cap
    for f in ("rep_query", "top_off", "top_pid", "top_kmatch"):
        assert getattr(top, f).tolist() == getattr(ref_top, f).tolist(), f
    sx.close()
    sx = api.ShardedIndex.from_images(images, [gpu_device] * 2)
    full = sx.search(packed=q)
    assert not sx.exchange_info()["adaptive"] and sx.exchange_info()["need_entries"] > e_cap
    _check_full(full, ref_full, False)
    sx.close()
    tp, tk = top.dense()
    for i in range(0, len(seqs), 5):
        s = seqs[i]
        exp, keep = {}, 0
        if oracle.size_in_kmer(s) >= 7:
            pid, km, _ = oix.search(s)
            exp = dict(zip(pid.tolist(), km.tolist()))
            keep = oracle.filter_results(km, oracle.size_in_kmer(s)) if len(km) else 0
            assert tp[i, :keep].tolist() == pid[:keep].tolist() and tk[i, :keep].tolist() == km[:keep].tolist(), i
        assert int(top.top_cnt[i]) == keep, i
        assert full.hits(i) == exp, i


@pytest.mark.gpu
def test_protein_search_driver_on_sharded_index(klib, oracle, gpu_device):
    from kaamer_amd import api, search, workload
    db = workload.make_db(600, seed=6)
    qs = workload.unpack(workload.make_protein_queries(db, 60, seed=5))
    text = "".join(">q%d d\n%s\n" % (i, s.decode()) for i, s in enumerate(qs)) + ">short\nACDEFGHIKLMN\n"
    ix1 = api.Index.from_image(api.Image.from_proteins(packed=db), gpu_device)
    sx = api.ShardedIndex.from_images([api.Image.from_proteins(packed=db, shard=r, n_shards=3) for r in range(3)], [gpu_device] * 3)
    opts = search.SearchOptions(ExtractPositions=True)
    got = search.ProteinSearch(sx, text, opts)
    exp = search.ProteinSearch(ix1, text, opts)
    assert got == exp
    assert sum(len(r["SearchResults"]["PositionHits"]) for r in exp) > 50
    sx.close()


def _ranks_worker(rank, world, port, ret, scenario):
    """one of two processes sharing GPU 0: ShardedSearcher(want_positions=True), blocks through the host and gloo"""
    for p_ in (ROOT, HERE):
        sys.path.insert(0, p_)
    import torch
    from kaamer_amd import abi, api, sharded, workload
    from oracle import oracle as O
    from test_sharded import _init_gloo
    _init_gloo(rank, world, port)
    try:
        torch.cuda.set_device(0)
        db = workload.make_db(600, seed=6)
        recs = workload.unpack(db)
        oix = O.Index.from_proteins(None, packed=db)
        ix = api.Index.from_image(api.Image.from_proteins(packed=db, shard=rank, n_shards=world), 0)
        st = torch.cuda.current_stream()
        short = [r[:40] for r in recs[:60]]
        longer = _long_batch(recs, np.random.default_rng(3), 60, 12)
        qs = workload.unpack(workload.make_protein_queries(db, 150, seed=7)) + [b"AAAAAAA", b""]
        mx = sum(len(s) for s in longer) + 64
        ss = sharded.ShardedSearcher(ix, rank, world, mx, 200, max_entries_per_peer=1 << 16, transport="host",
                                     want_positions=True, max_pos_words_per_peer=1 << 21)

        def dev(queries):
            buf, offs = api.pack_sequences(queries)
            return torch.from_numpy(buf).cuda(), torch.from_numpy(offs.view(np.int64)).cuda(), len(offs) - 1, len(buf)

        def check(queries, r):
            n_owned = (len(queries) - rank + world - 1) // world
            cnt = sharded.dev_tensor(r.d_hit_cnt, n_owned, torch.int32).cpu().numpy()
            off = sharded.dev_tensor(r.d_hit_off, n_owned, torch.int64).cpu().numpy()
            tot = int((off + cnt).max()) if n_owned else 0   # (the merge's lists are not in query order)
            pid = sharded.dev_tensor(r.d_hit_pid, tot, torch.int32).cpu().numpy()
            km = sharded.dev_tensor(r.d_hit_kmatch, tot, torch.int32).cpu().numpy()
            poff = sharded.dev_tensor(r.d_pos_off, tot, torch.int64).cpu().numpy()
            nw = int(sharded.dev_tensor(r.d_pos_base, n_owned + 1, torch.int64).cpu().numpy()[-1])
            bits = sharded.dev_tensor(r.d_pos_bits, nw, torch.int64).cpu().numpy().view(np.uint64)
            n = 0
            for i in range(n_owned):
                s = queries[rank + i * world]
                size = O.size_in_kmer(s)
                if size < 7:
                    assert cnt[i] == 0
                    continue
                epid, ekm, epos = oix.search(s, want_positions=True)
                exp = {int(p): (int(k), epos[j]) for j, (p, k) in enumerate(zip(epid, ekm))}
                assert int(cnt[i]) == len(exp), i
                w = (size + 63) // 64
                for h in range(int(off[i]), int(off[i]) + int(cnt[i])):
                    k, bp = exp[int(pid[h])]
                    assert int(km[h]) == k
                    b = np.unpackbits(bits[int(poff[h]):int(poff[h]) + w].view(np.uint8), bitorder="little")[:size].astype(bool)
                    assert b.tolist() == bp.tolist(), (i, int(pid[h]))
                    n += 1
            return n

        if scenario == "exact":
            d = dev(qs)
            for _ in range(3):   # capacity blocks twice, then blocks sized from the batch before last
                r, _, _ = ss.run(d[0].data_ptr(), d[1].data_ptr(), d[2], d[3], st)
                ret["hits%d" % rank] = check(qs, r)
            ret["adaptive%d" % rank] = ss.wire is not ss.layout
        elif scenario == "grow":
            a, b = dev(short), dev(longer)
            for _ in range(2):
                ss.run(a[0].data_ptr(), a[1].data_ptr(), a[2], a[3], st)
            ss.step(b[0].data_ptr(), b[1].data_ptr(), b[2], b[3], st)   # blocks sized from the short batch
            try:
                ss.finish(st)
                ret["raised%d" % rank] = None
            except abi.KaamerError as e:
                ret["raised%d" % rank] = e.code
            need, povf = ss.mws.exchange_stats_positions(0)
            ret["povf%d" % rank] = povf
            r, _, _ = ss.run(b[0].data_ptr(), b[1].data_ptr(), b[2], b[3], st)
            ret["hits%d" % rank] = check(longer, r)
        elif scenario == "nopos":
            d = dev(qs)
            raw = st.cuda_stream
            if rank == 0:   # a merge workspace without positions refuses an arrays = 4 layout and enqueues nothing
                m = api.Workspace(ix, 64, ss.layout.q_cap, max_queries=ss.layout.q_cap, first_pos=1, max_hits=world * ss.layout.e_cap)
                try:
                    m.exchange_merge(ss.layout, ss.recv.data_ptr(), raw)
                    ret["arg"] = None
                except abi.KaamerError as e:
                    ret["arg"] = e.code
                try:
                    m.exchange_stats(0)
                    ret["enqueued"] = True
                except abi.KaamerError:
                    ret["enqueued"] = False
                m.close()
            ss.wire = ss.layout
            ss.ws.search_device(d[0].data_ptr(), d[1].data_ptr(), d[2], d[3], stream=raw)
            ss.ws.exchange_pack(ss.layout, ss.send.data_ptr(), raw)
            if rank == 1:   # this rank's blocks claim no bitmaps
                blocks = ss.send.view(world, -1)
                blocks[:, 1] &= ~16
            ss._alltoall(st)
            ss.mws.exchange_merge(ss.layout, ss.recv.data_ptr(), raw)
            try:
                ss.finish(st)
                ret["raised%d" % rank] = None
            except abi.KaamerError as e:
                ret["raised%d" % rank] = e.code
        ss.close()
        ret["ok%d" % rank] = True
    finally:
        import torch.distributed as dist
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("scenario", ["exact", "grow", "nopos"])
def test_sharded_searcher_positions_two_ranks(klib, oracle, gpu_device, scenario):
    from kaamer_amd import abi
    sys.path.insert(0, HERE)
    from test_sharded import _spawn
    ret = _spawn(_ranks_worker, 2, (scenario,), timeout=300)
    assert ret.get("ok0") and ret.get("ok1"), ret
    if scenario == "exact":
        assert ret["hits0"] > 100 and ret["hits1"] > 100
        assert ret["adaptive0"] and ret["adaptive1"]
    elif scenario == "grow":
        assert ret["raised0"] == ret["raised1"] == abi.E_CAPACITY
        assert ret["povf0"] and ret["povf1"]
        assert ret["hits0"] > 50 and ret["hits1"] > 50
    else:
        assert ret["arg"] == abi.E_ARG and ret["enqueued"] is False
        assert ret["raised0"] == ret["raised1"] == abi.E_CAPACITY
