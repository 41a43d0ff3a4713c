"""PositionHits bitmaps of the REPORTED hits on the one-process sharded handle (kaamer_sharded_search_batch_top_pos_flat and
its submit form): every array equals what kaamer_search_batch_top_pos_flat returns on an unsharded index of the whole
database, and for protein input the CPU oracle's PositionHits rows.  All shards sit on the one device.  Every comparison
is bit-exact."""
import os
import re
import threading

import numpy as np
import pytest

from test_gpu_top_positions import ALPHA, OPTS, _check_top, _mix, _oracle_protein, _same_hits, _same_positions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_ONLY = bool(os.environ.get("KAAMER_HOST_ONLY"))   # the sanitized CPU build holds the host sources only
NEW_SYMBOLS = ("kaamer_sharded_search_batch_top_pos_flat", "kaamer_sharded_submit_batch_top_pos_flat", "kaamer_sharded_positions_info")
WORLDS = (1, 2, 3, 8)


# ---------------------------------------------------------------- host only
def test_new_symbols_declared_and_bound():
    from kaamer_amd import abi
    src = open(os.path.join(ROOT, "include", "kaamer_hip.h")).read()
    assert re.search(r"#define\s+KAAMER_ABI_VERSION\s+4\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kaamer_[a-z_0-9]+)\s*\(", code))
    for n in NEW_SYMBOLS:
        assert n in declared, "include/kaamer_hip.h does not declare %s" % n
        assert n in abi.SYMBOLS, "abi.py does not bind %s" % n


@pytest.mark.skipif(HOST_ONLY, reason="host-only sanitized library")
def test_new_symbols_exported(klib):
    for n in NEW_SYMBOLS:
        assert hasattr(klib, n), "libkaamer_hip.so lacks %s" % n
    assert klib.kaamer_abi_version() == 4


# ---------------------------------------------------------------- GPU
def _sharded(api, gpu_device, W, **kw):
    images = [api.Image.from_proteins(shard=r, n_shards=W, **kw) for r in range(W)]
    return images, api.ShardedIndex.from_images(images, [gpu_device] * W)


@pytest.fixture(scope="module")
def small(klib, oracle, gpu_device):
    from kaamer_amd import api, workload
    db = workload.make_db(1000)
    ix = api.Index.from_image(api.Image.from_proteins(packed=db), gpu_device)
    return db, ix, oracle.Index.from_proteins(None, packed=db)


def _two_shard_hits(api, gpu_device, images, top, packed, seq_type):
    """reported (query, protein) hits whose bits come from at least two shards, by searching every shard image on its own"""
    parts = []
    for im in images:
        ixs = api.Index.from_image(im, gpu_device)
        parts.append(ixs.search(packed=packed, seq_type=seq_type, want_positions=True))
    n = 0
    for i, q in enumerate(top.rep_query.tolist()):
        per_shard = [p.positions(q) for p in parts]
        for pid, bits in top.positions(i).items():
            have = [ps[pid] for ps in per_shard if pid in ps and ps[pid].any()]
            acc = np.zeros_like(bits)
            for h in have:
                assert not (acc & h).any()                   # the shards' parts of one hit are disjoint
                acc |= h
            assert np.array_equal(acc, bits), (q, pid)       # ... and their union is the bitmap
            n += len(have) >= 2
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("W", WORLDS)
def test_protein_equals_unsharded_and_oracle(small, oracle, gpu_device, W):
    from kaamer_amd import abi, api
    db, ix, oix = small
    seqs = _mix(db)
    packed = api.pack_sequences(seqs)
    images, sx = _sharded(api, gpu_device, W, packed=db)
    for k, (ratio, mink, maxr) in enumerate(OPTS):
        ref = ix.search_top(seqs, min_k_ratio=ratio, min_k_match=mink, max_results=maxr, want_positions=True)
        top = sx.search_top(seqs, min_k_ratio=ratio, min_k_match=mink, max_results=maxr, want_positions=True)
        _same_positions(top, ref)
        exp = [_oracle_protein(oracle, oix, s, ratio, mink, maxr) for s in seqs]
        assert sum(e is None for e in exp) >= 1 and sum(e is not None for e in exp) >= len(seqs) // 2   # not vacuous
        _check_top(top, exp)
        if W > 1 and k == 0:
            assert _two_shard_hits(api, gpu_device, images, top, packed, abi.PROTEIN) >= 1
    sx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W", WORLDS)
def test_reads_equal_unsharded(small, gpu_device, W):
    from kaamer_amd import abi, api, workload
    db, ix, oix = small
    reads = workload.make_reads(db, 400, seed=31)
    images, sx = _sharded(api, gpu_device, W, packed=db)
    for k, (ratio, mink, maxr) in enumerate(OPTS):
        ref = ix.search_top(packed=reads, seq_type=abi.READS, min_k_ratio=ratio, min_k_match=mink, max_results=maxr, want_positions=True)
        top = sx.search_top(packed=reads, seq_type=abi.READS, min_k_ratio=ratio, min_k_match=mink, max_results=maxr, want_positions=True)
        assert top.n_queries == ref.n_queries and 0 < top.n_reported < top.n_queries      # some ORFs report, some do not
        _same_positions(top, ref)
        assert bytes(top.orf_aa) == bytes(ref.orf_aa)
        assert len(top.pos_bits) > 0 and int(top.pos_bits.astype(bool).sum()) > 0
        if W > 1 and k == 0:
            assert _two_shard_hits(api, gpu_device, images, top, reads, abi.READS) >= 1
    sx.close()


@pytest.mark.gpu
def test_g_tier_w3(klib, oracle, gpu_device):
    """the database of test_gpu_top_positions.test_g_tier: 3 000 hits per query, counted in the HBM tier"""
    from kaamer_amd import api
    rng = np.random.default_rng(14)
    core = bytes(ALPHA[rng.integers(0, 20, 70)])
    db = [bytes(ALPHA[rng.integers(0, 20, 6)]) + core[(i % 9):] + bytes(ALPHA[rng.integers(0, 20, 6)]) for i in range(3000)]
    ids = rng.permutation(20000)[:3000].astype(np.uint32)
    ix = api.Index.from_image(api.Image.from_proteins(db, ids=ids), gpu_device)
    oix = oracle.Index.from_proteins(db, ids=ids)
    _, sx = _sharded(api, gpu_device, 3, seqs=db, ids=ids)
    seqs = [core, bytes(ALPHA[rng.integers(0, 20, 130)]) + core + bytes(ALPHA[rng.integers(0, 20, 70)]), db[11], core[:25]]
    for maxr in (10, 700):
        ref = ix.search_top(seqs, min_k_ratio=0.0, min_k_match=1, max_results=maxr, want_positions=True)
        top = sx.search_top(seqs, min_k_ratio=0.0, min_k_match=1, max_results=maxr, want_positions=True)
        _same_positions(top, ref)
        exp = [_oracle_protein(oracle, oix, s, 0.0, 1, maxr) for s in seqs]
        assert len(exp[0][1]) == maxr
        _check_top(top, exp)
        if maxr == 700:   # 700 ids per query against the 16 a first ids block provisions: repeated with larger blocks
            assert sx.positions_info()["attempts"] > 1
    sx.close()


@pytest.mark.gpu
def test_protein_first_positions_are_zeros_on_a_g_tier_database(klib, gpu_device):
    """kaamer_hip.h: top_first_pos is zeros for protein input (search.go:416), also for the queries the HBM tier counted,
    with and without positions, unsharded and sharded"""
    from kaamer_amd import api
    rng = np.random.default_rng(14)
    core = bytes(ALPHA[rng.integers(0, 20, 70)])
    db = [bytes(ALPHA[rng.integers(0, 20, 6)]) + core[(i % 9):] + bytes(ALPHA[rng.integers(0, 20, 6)]) for i in range(3000)]
    ix = api.Index.from_image(api.Image.from_proteins(db), gpu_device)
    _, sx = _sharded(api, gpu_device, 2, seqs=db)
    seqs = [core, db[11], core[:25]]
    for h in (ix, sx):
        for pos in (False, True):
            top = h.search_top(seqs, min_k_ratio=0.0, min_k_match=1, max_results=50, want_positions=pos)
            assert top.n_reported == 3 and len(top.top_first_pos) == 150
            assert not top.top_first_pos.any()
    assert ix.search_top(seqs, min_k_ratio=0.0, min_k_match=1, max_results=50).counters["n_overflow"] >= 2   # the G tier was entered
    sx.close()


@pytest.mark.gpu
def test_long_lists_w3(klib, oracle, gpu_device):
    """one motif shared by 6 000 proteins: its k-mers' postings lists take the wave-cooperative scan on their shard"""
    from kaamer_amd import api
    rng = np.random.default_rng(9)
    motif = bytes(ALPHA[rng.integers(0, 20, 20)])
    db = []
    for i in range(6000):
        body = bytearray(bytes(ALPHA[rng.integers(0, 20, 60)]))
        body[20:40] = motif
        db.append(bytes(body))
    ix = api.Index.from_image(api.Image.from_proteins(db), gpu_device)
    oix = oracle.Index.from_proteins(db)
    images, sx = _sharded(api, gpu_device, 3, seqs=db)
    assert max(im.stats()["max_list"] for im in images) >= 5000     # the long-list path is entered on a shard
    fill = lambda n: bytes(ALPHA[rng.integers(0, 20, n)])
    seqs = [fill(30) + motif + fill(30), db[7], db[4999], motif + fill(3) + motif, fill(200), (fill(10) + motif) * 6]
    for (ratio, mink, maxr) in ((0.05, 10, 10), (0.0, 1, 100)):
        ref = ix.search_top(seqs, min_k_ratio=ratio, min_k_match=mink, max_results=maxr, want_positions=True)
        top = sx.search_top(seqs, min_k_ratio=ratio, min_k_match=mink, max_results=maxr, want_positions=True)
        _same_positions(top, ref)
        exp = [_oracle_protein(oracle, oix, s, ratio, mink, maxr) for s in seqs]
        assert sum(e is not None for e in exp) >= 5
        _check_top(top, exp)
    sx.close()


@pytest.mark.gpu
def test_query_longer_than_65535_kmers_w2(klib, oracle, gpu_device):
    from kaamer_amd import api, workload
    db = workload.make_db(3000, seed=21)
    ix = api.Index.from_image(api.Image.from_proteins(packed=db), gpu_device)
    oix = oracle.Index.from_proteins(None, packed=db)
    _, sx = _sharded(api, gpu_device, 2, packed=db)
    recs = workload.unpack(db)
    rng = np.random.default_rng(5)
    long_q = b"".join(recs[int(i)] for i in rng.integers(0, len(recs), 260))
    assert len(long_q) - 6 > 70000
    seqs = [recs[3], long_q, recs[17][:40], long_q[1000:70000]]
    ref = ix.search_top(seqs, min_k_ratio=0.0, min_k_match=1, max_results=70, want_positions=True)
    top = sx.search_top(seqs, min_k_ratio=0.0, min_k_match=1, max_results=70, want_positions=True)
    _same_positions(top, ref)
    exp = [_oracle_protein(oracle, oix, s, 0.0, 1, 70) for s in seqs]
    assert exp[1][0] > 65535 and len(exp[1][1]) == 70
    _check_top(top, exp)
    sx.close()


def _full_equal(got, ref):
    assert got.n_queries == ref.n_queries and got.hit_cnt.tolist() == ref.hit_cnt.tolist()
    for q in range(ref.n_queries):
        assert got.hits(q) == ref.hits(q), q
        a, b = got.positions(q), ref.positions(q)
        assert sorted(a) == sorted(b), q
        for p, bits in b.items():
            assert np.array_equal(a[p], bits), (q, p)


@pytest.mark.gpu
def test_flag_off_and_alternating_calls(small, gpu_device):
    """the flag off: the same hits and no positions; one handle serves a plain top call, a positions call, a full call and a
    positions call again (its workspaces are re-prepared when the kind changes), each equal to its unsharded counterpart"""
    from kaamer_amd import abi, api, workload
    db, ix, oix = small
    seqs = _mix(db)
    reads = workload.make_reads(db, 200, seed=5)
    _, sx = _sharded(api, gpu_device, 3, packed=db)
    ref_plain, ref_pos = ix.search_top(seqs), ix.search_top(seqs, want_positions=True)
    ref_full = ix.search(seqs, want_positions=True)
    ref_reads = ix.search_top(packed=reads, seq_type=abi.READS, want_positions=True)
    for _ in range(2):
        plain = sx.search_top(seqs)
        assert plain.pos_bits is None and plain.pos_off is None and plain.pos_bits_len is None
        _same_hits(plain, ref_plain)
        pos = sx.search_top(seqs, want_positions=True)
        _same_hits(pos, plain)                                # reported pids / Kmatch unchanged by the flag
        _same_positions(pos, ref_pos)
        _full_equal(sx.search(seqs, want_positions=True), ref_full)
        _same_positions(sx.search_top(seqs, want_positions=True), ref_pos)
        _same_positions(sx.search_top(packed=reads, seq_type=abi.READS, want_positions=True), ref_reads)
    sx.close()


@pytest.mark.gpu
def test_three_tickets_from_three_threads(small, gpu_device):
    from kaamer_amd import api, workload
    db, ix, oix = small
    batches = [workload.make_protein_queries(db, 40, seed=60 + i) for i in range(3)]
    refs = [ix.search_top(packed=b, want_positions=True) for b in batches]
    _, sx = _sharded(api, gpu_device, 2, packed=db)
    for _ in range(2):
        tickets, got, errs = [None] * 3, [None] * 3, []
        gate = threading.Barrier(3)

        def submit(i):
            try:
                gate.wait()
                tickets[i] = sx.submit_top(packed=batches[i], want_positions=True)
            except Exception as e:   # noqa: BLE001
                errs.append(e)

        def wait(i):
            try:
                got[i] = tickets[i].wait()
            except Exception as e:   # noqa: BLE001
                errs.append(e)

        for fn in (submit, wait):                             # three in flight before the first is waited for
            th = [threading.Thread(target=fn, args=(i,)) for i in range(3)]
            for t in th:
                t.start()
            for t in th:
                t.join()
            assert not errs, errs
        for i in range(3):
            _same_positions(got[i], refs[i])
    t = sx.submit_top(packed=batches[0], want_positions=True)
    t.discard()
    _same_positions(sx.search_top(packed=batches[1], want_positions=True), refs[1])
    sx.close()


@pytest.mark.gpu
def test_blocks_grow_with_the_batch(small, gpu_device):
    """a tiny batch, then one whose bitmaps outgrow the ids blocks and segments sized from it (need + a quarter): repeated at
    the capacity inside the call, exact; a third call of that size takes one attempt with segments below the capacity"""
    from kaamer_amd import api, workload
    db, ix, oix = small
    tiny = workload.unpack(db)[:2]
    big = workload.make_protein_queries(db, 600, seed=3)
    _, sx = _sharded(api, gpu_device, 2, packed=db)
    _same_positions(sx.search_top(tiny, want_positions=True), ix.search_top(tiny, want_positions=True))
    first = sx.positions_info()
    assert first["attempts"] == 1
    ref = ix.search_top(packed=big, want_positions=True)
    _same_positions(sx.search_top(packed=big, want_positions=True), ref)
    second = sx.positions_info()
    print("tiny:", first, "big:", second)
    assert second["need_words"] > first["need_words"] + first["need_words"] // 4 + 1024     # beyond what the first call sized
    assert second["attempts"] > 1
    assert second["need_words"] * 8 <= second["segment_bytes"]
    _same_positions(sx.search_top(packed=big, want_positions=True), ref)
    third = sx.positions_info()
    print("again:", third)
    assert third["attempts"] == 1
    assert third["need_words"] == second["need_words"]
    assert third["need_words"] * 8 <= third["segment_bytes"] < second["segment_bytes"]       # payload, not capacity
    assert third["ids_block_bytes"] < second["ids_block_bytes"]
    sx.close()


@pytest.mark.gpu
def test_a_failing_shard_fails_the_whole_call(klib, gpu_device):
    """the skewed database of test_sharded_calls_grow_their_bounds: the shards' first searches overflow their hit pools and
    exchange blocks, so the first attempt fails on every owner; the call repeats it as a whole and returns every bit"""
    from kaamer_amd import api, workload
    db = workload.make_db_zipf(40000, seed=11, n_motifs=1500, zipf_a=1.0, per_residues=60)
    q = workload.make_protein_queries(db, 200, seed=12)
    ix1 = api.Index.from_image(api.Image.from_proteins(packed=db), gpu_device)
    ref = ix1.search_top(packed=q, want_positions=True)
    _, sx = _sharded(api, gpu_device, 2, packed=db)
    e_cap = 2 * len(q[0]) // 2 + 65536      # entries per (shard -> owner) block of a first attempt
    top = sx.search_top(packed=q, want_positions=True)
    assert not sx.exchange_info()["adaptive"] and sx.exchange_info()["need_entries"] > e_cap
    assert sx.positions_info()["attempts"] > 1
    _same_positions(top, ref)
    assert int(top.pos_off[-1]) == len(top.pos_bits) > 0
    for i in range(top.n_reported):          # no missing bits: every bitmap has as many as its Kmatch
        a = int(top.top_off[i])
        for h, bits in enumerate(top.positions(i).values()):
            assert int(bits.sum()) == int(top.top_kmatch[a + h]), (i, h)
    sx.close()
