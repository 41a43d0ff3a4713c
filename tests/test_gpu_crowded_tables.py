"""Search parity on crowded bucket tables: the continuation path of probe_kernel (search.hip).

A lookup whose bucket is full and does not hold the key goes on a per-wave ring in LDS and is served later, 64 at a
time, by an iteration of the same loop body: the value it finds overwrites the 0 the regular pass stored, the walk may
pass the last bucket and go on at bucket 0, and a ring iteration may put a lookup back on the ring.  At the default
load factor (0.5) one lookup in twenty gets there and none walks far, so the tables here are built at 0.75, 0.9 and 0.95
(tests/test_table_walk.py prints what such images look like) or have a handful of buckets.

Every test compares hits and first positions with the CPU oracle, and the probe's three counters with the numpy walk of
tests/tableref.py over the very windows the batch looks up: n_lookup and n_found exactly, and n_probe == the number of
buckets the walk read -- an equality, so a probe that stops early, walks too far or serves a ring entry twice fails even
where the hits happen to come out right.  Every test asserts from that walk that its batch enters the branch it is
named for.  Databases, queries and seeds are fixed (tests/test_table_walk.py builds the same ones on the CPU)."""
import numpy as np
import pytest

import tableref
from test_gpu_protein import _check, _oracle_hits
from test_table_walk import crowded_db, oracle_keys, query_windows, random_seqs, tiny_cases, tiny_queries

pytestmark = pytest.mark.gpu


def _walk_batch(oracle, table, okeys, seqs):
    """the windows a protein batch looks up, walked on the CPU -> dict(n_lookup, n_found, n_probe, walked, wrapped, present)"""
    _, wk = query_windows(oracle, seqs)
    return _walk_keys(table, okeys, wk)


def _walk_keys(table, okeys, wk):
    present = np.isin(wk, okeys)
    val, walked, wrapped = table.walk(wk)
    assert ((val != 0) == present).all()          # the CPU leg: the walk finds what the oracle index holds
    return dict(n_lookup=len(wk), n_found=int(present.sum()), n_probe=int(walked.sum()), walked=walked, wrapped=wrapped,
                present=present)


def _check_counters(c, w):
    got = {k: c[k] for k in ("n_lookup", "n_found", "n_probe")}
    assert got == {k: w[k] for k in ("n_lookup", "n_found", "n_probe")}


def _hit_rows(res, q):
    a, b = res.span(q)
    return sorted(zip(res.hit_pid[a:b].tolist(), res.hit_kmatch[a:b].tolist(), res.hit_first_pos[a:b].tolist()))


def _same_batch(a, b, positions=False):
    """two BatchResults field by field (hit lists as sets: the order inside a list is the counting table's)"""
    assert a.n_queries == b.n_queries
    assert a.meta.tolist() == b.meta.tolist()
    assert a.hit_cnt.tolist() == b.hit_cnt.tolist()
    assert bytes(a.orf_aa) == bytes(b.orf_aa) and a.starts_alt.tolist() == b.starts_alt.tolist()
    for q in range(a.n_queries):
        assert _hit_rows(a, q) == _hit_rows(b, q), q
        if positions:
            pa, pb = a.positions(q), b.positions(q)
            assert sorted(pa) == sorted(pb), q
            for p in pa:
                assert np.array_equal(pa[p], pb[p]), (q, p)
    for k in ("n_queries", "n_lookup", "n_found", "n_post", "n_hits", "n_lists", "n_list_ids"):
        assert a.counters[k] == b.counters[k], k


def _same_top(a, b, positions=False):
    assert a.n_queries == b.n_queries and a.rep_query.tolist() == b.rep_query.tolist()
    assert a.top_off.tolist() == b.top_off.tolist()
    assert a.top_pid.tolist() == b.top_pid.tolist() and a.top_kmatch.tolist() == b.top_kmatch.tolist()
    assert a.top_first_pos.tolist() == b.top_first_pos.tolist()
    assert a.trim.tolist() == b.trim.tolist() and a.meta.tolist() == b.meta.tolist()
    if positions:
        assert a.pos_bits_len.tolist() == b.pos_bits_len.tolist() and a.pos_off.tolist() == b.pos_off.tolist()
        assert np.array_equal(a.pos_bits, b.pos_bits)


@pytest.fixture(scope="module")
def crowd(klib, oracle, gpu_device):
    """the database of tests/test_table_walk.py, its oracle index, and the batch of (a) with its oracle results (once)"""
    from kaamer_amd import workload
    db = crowded_db()
    oix = oracle.Index.from_proteins(None, packed=db)
    seqs = workload.unpack(workload.make_protein_queries(db, 300, seed=46)) + random_seqs(np.random.default_rng(46), 50, 30, 120)
    return dict(db=db, oix=oix, okeys=oracle_keys(oix), seqs=seqs, exp=_oracle_hits(oix, oracle, seqs))


@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("load", [0.5, 0.75, 0.9, 0.95])
def test_parity_and_exact_counters_at_every_load(crowd, oracle, gpu_device, tmp_path, load, builder):
    """(a) 300 mutated database proteins and 50 random sequences against the table at every load factor, from the host
    builder's image and from the device builder's: hits and first positions are the oracle's, n_lookup = sum of SizeInKmer,
    n_found = the windows whose key the oracle index holds, n_probe = the buckets the CPU walk reads.  The batch has fewer
    residues than the table has buckets: the nontemporal bucket loads.

    What the walk says about this batch's 103 520 windows (61 401 of them present; printed by the test) -- present windows
    found outside their home bucket / lookups that read three buckets or more (put back on the ring by a ring iteration)
    / longest walk / n_probe:
        load 0.50:  0.9 %,    266,   6,   106 573        load 0.90: 13.4 %, 27 119, 137,   386 288
        load 0.75:  6.1 %,  7 888,  20,   139 428        load 0.95: 16.6 %, 37 794, 584, 1 280 369
    Asserted a third below: at 0.95 a displaced share > 0.11, > 25 000 lookups of three buckets or more, a walk > 389
    buckets; at 0.9 > 0.089, > 18 000, > 91; at 0.75 > 0.041, > 5 250, > 13; at 0.5 only that the ring is entered at all."""
    from kaamer_amd import api
    img = api.Image.from_proteins(packed=crowd["db"], load_factor=load, device=gpu_device if builder == "device" else None)
    t = tableref.table_of(img, tmp_path)
    w = _walk_batch(oracle, t, crowd["okeys"], crowd["seqs"])
    share = float((w["walked"][w["present"]] > 1).mean())
    again, longest = int((w["walked"] >= 3).sum()), int(w["walked"].max())
    print("load %.2f (%s): %d windows, %d buckets; present displaced %.3f, walks >= 3: %d, longest %d, n_probe %d"
          % (load, builder, w["n_lookup"], t.nb, share, again, longest, w["n_probe"]))
    low = {0.5: (0.0, 0, 1), 0.75: (0.041, 5250, 13), 0.9: (0.089, 18000, 91), 0.95: (0.11, 25000, 389)}[load]
    assert share > low[0] and again > low[1] and longest > low[2]
    assert sum(len(s) for s in crowd["seqs"]) < t.nb
    ix = api.Index.from_image(img, gpu_device)
    res = ix.search(crowd["seqs"])
    _check(res, crowd["exp"])
    _check_counters(res.counters, w)
    ix.close()


def test_ring_served_between_windows(crowd, oracle, gpu_device, tmp_path, monkeypatch):
    """(b) One workgroup of four waves per CU (KAAMER_P_PER_CU=1, read when the index's first workspace is created: by
    the first search, host_slot_acquire -> kaamer_workspace_create) and a batch whose lookups that leave their first
    bucket number 128 for every wave of the grid or more: some wave then holds 128 of them, the last window brings at most
    64, so that wave has 64 on its ring while it still has a window to go and serves the ring between two windows.  The
    batch has more residues than the table has buckets: the cached bucket loads.  Sized on the CPU for 256 CUs with a
    quarter to spare (1 400 queries, 481 447 windows: 219 932 such lookups against 131 072)."""
    import torch
    from kaamer_amd import api, workload
    monkeypatch.setenv("KAAMER_P_PER_CU", "1")
    img = api.Image.from_proteins(packed=crowd["db"], load_factor=0.95)
    t = tableref.table_of(img, tmp_path)
    seqs = workload.unpack(workload.make_protein_queries(crowd["db"], 1400, seed=47))
    w = _walk_batch(oracle, t, crowd["okeys"], seqs)
    deferred = int((w["walked"] > 1).sum())
    n_cu = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    print("%d windows, %d leave their first bucket (%.3f); %d CUs" % (w["n_lookup"], deferred, deferred / w["n_lookup"], n_cu))
    assert deferred >= 1.25 * 128 * 4 * 256
    assert deferred >= 128 * 4 * n_cu
    assert sum(len(s) for s in seqs) >= t.nb
    ix = api.Index.from_image(img, gpu_device)
    res = ix.search(seqs)
    _check(res, _oracle_hits(crowd["oix"], oracle, seqs))
    _check_counters(res.counters, w)
    ix.close()


def test_tiny_tables_and_wrap(klib, oracle, gpu_device, tmp_path):
    """(c) The forty tiny databases of tests/test_table_walk.py (fixed seeds; tables of one, two and three buckets, a
    database without proteins), each searched with its own proteins, mutants of them and sequences that share no key with
    it.  Over these batches the CPU walk passes the last bucket and goes on at bucket 0 for present keys and for absent
    ones; hits, first positions and the three counters are exact for every table."""
    from kaamer_amd import api
    wrap_present = wrap_absent = 0
    sizes = set()
    for case, (db, load) in enumerate(tiny_cases()):
        img = api.Image.from_proteins(packed=db, load_factor=load)
        t = tableref.table_of(img, tmp_path)
        sizes.add(t.nb)
        oix = oracle.Index.from_proteins(None, packed=db)
        own, mutants, rnd = tiny_queries(db, case)
        seqs = own + mutants + rnd
        w = _walk_batch(oracle, t, oracle_keys(oix), seqs)
        wrap_present += int((w["wrapped"] & w["present"]).sum())
        wrap_absent += int((w["wrapped"] & ~w["present"]).sum())
        ix = api.Index.from_image(img, gpu_device)
        res = ix.search(seqs)
        _check(res, _oracle_hits(oix, oracle, seqs))
        _check_counters(res.counters, w)
        assert all(res.hits(q) == {} for q in range(len(own) + len(mutants), len(seqs))), case
        ix.close()
    assert sizes >= {1, 2, 3}
    assert wrap_present >= 1 and wrap_absent >= 1, (wrap_present, wrap_absent)


def test_load_factor_is_invisible(crowd, oracle, gpu_device, tmp_path):
    """(d) One database, indexes at load 0.5 and 0.95: the full hit lists with and without PositionHits, the reported hits
    with their bitmaps, and a batch of 2 000 reads (probe_kernel<true>, whose idle lanes issue no load) are the same field
    by field; the reads' ORFs, hits and first positions are the oracle's; n_lookup and n_found are equal between the two
    loads, and n_probe at either load is what the CPU walk reads over the windows of oracle.get_orfs."""
    from kaamer_amd import abi, api, workload
    from test_gpu_reads import _check_reads
    db, oix = crowd["db"], crowd["oix"]
    imgs = {load: api.Image.from_proteins(packed=db, load_factor=load) for load in (0.5, 0.95)}
    tabs = {load: tableref.table_of(imgs[load], tmp_path) for load in imgs}
    ixs = {load: api.Index.from_image(imgs[load], gpu_device) for load in imgs}
    seqs = crowd["seqs"][:100] + crowd["seqs"][-10:] + [workload.unpack(db)[3], b"ACDEFGHIKLMNP", b"AAAA", b""]
    w = {load: _walk_batch(oracle, tabs[load], crowd["okeys"], seqs) for load in imgs}
    assert w[0.95]["n_probe"] > 2 * w[0.5]["n_probe"]
    plain = {load: ixs[load].search(seqs) for load in imgs}
    _same_batch(plain[0.5], plain[0.95])
    withpos = {load: ixs[load].search(seqs, want_positions=True) for load in imgs}
    _same_batch(withpos[0.5], withpos[0.95], positions=True)
    _same_batch(plain[0.95], withpos[0.95])
    top = {load: ixs[load].search_top(seqs, want_positions=True) for load in imgs}
    _same_top(top[0.5], top[0.95], positions=True)
    assert top[0.95].n_reported > 80
    for load in imgs:
        for r in (plain[load], withpos[load]):
            _check_counters(r.counters, w[load])
        _check_counters(top[load].counters, w[load])
    # reads
    reads = workload.make_reads(db, 2000, seed=48)
    rl = workload.unpack(reads)
    got = {load: ixs[load].search(packed=reads, seq_type=abi.READS, want_positions=True) for load in imgs}
    _same_batch(got[0.5], got[0.95], positions=True)
    n_orfs = _check_reads(got[0.95], rl, oracle, oix)
    assert n_orfs > 2000 and got[0.95].counters["n_hits"] > 1500
    orfs = [o["seq"].encode("latin-1") for r in rl for o in oracle.get_orfs(r)]
    packed = oracle.pack(orfs)
    sizes = np.array([oracle.size_in_kmer(s) for s in orfs], dtype=np.int64)
    assert (sizes >= 7).all()
    wk = tableref.encode_windows(packed[0], tableref.window_starts(packed[1], sizes))
    for load in imgs:
        wr = _walk_keys(tabs[load], crowd["okeys"], wk)
        _check_counters(got[load].counters, wr)
    assert wr["n_probe"] > 2 * wr["n_lookup"] and int((wr["walked"][wr["present"]] > 1).sum()) > 1000
    for ix in ixs.values():
        ix.close()


def test_sharded_handle_on_crowded_shards(crowd, oracle, gpu_device, tmp_path):
    """(e) Three hash-prefix shards built at load 0.95 behind one handle (all on one device): the full hit lists and the
    reported hits equal those of the unsharded index at load 0.5.  Every shard's table is as crowded as the unsharded one:
    the walk over the batch's windows leaves the home bucket for present keys on each of them."""
    from kaamer_amd import api
    db = crowd["db"]
    seqs = crowd["seqs"][:150] + crowd["seqs"][-20:] + [b"AAAAAAA", b""]
    ref_ix = api.Index.from_image(api.Image.from_proteins(packed=db), gpu_device)
    ref, ref_top = ref_ix.search(seqs), ref_ix.search_top(seqs)
    imgs = [api.Image.from_proteins(packed=db, shard=s, n_shards=3, load_factor=0.95) for s in range(3)]
    n_lookup = 0
    for s, img in enumerate(imgs):
        w = _walk_batch(oracle, tableref.table_of(img, tmp_path), crowd["okeys"][tableref.shard_of_v(crowd["okeys"], 3) == s], seqs)
        own = w["walked"] > 0
        n_lookup += int(own.sum())
        assert float((w["walked"][w["present"]] > 1).mean()) > 0.11 and int((w["walked"] >= 3).sum()) > 1000
    assert n_lookup == ref.counters["n_lookup"]              # every window is looked up on exactly one shard
    sx = api.ShardedIndex.from_images(imgs, [gpu_device] * 3)
    got, got_top = sx.search(seqs), sx.search_top(seqs)
    assert got.n_queries == ref.n_queries and got.hit_cnt.tolist() == ref.hit_cnt.tolist()
    for f in ("src_seq", "size_in_kmer", "start_position", "end_position", "plus_strand"):
        assert got.meta[f].tolist() == ref.meta[f].tolist(), f
    for q in range(ref.n_queries):
        assert _hit_rows(got, q) == _hit_rows(ref, q), q
    _check(got, _oracle_hits(crowd["oix"], oracle, seqs))
    assert got_top.rep_query.tolist() == ref_top.rep_query.tolist() and got_top.top_off.tolist() == ref_top.top_off.tolist()
    assert got_top.top_pid.tolist() == ref_top.top_pid.tolist() and got_top.top_kmatch.tolist() == ref_top.top_kmatch.tolist()
    assert got_top.trim.tolist() == ref_top.trim.tolist() and got_top.n_reported > 100
    for k in ("n_lookup", "n_post", "n_hits"):
        assert got_top.counters[k] == ref_top.counters[k], k
    sx.close()
    ref_ix.close()
