"""The alignment of the reported hits (`-aln`) in one call on the one-process sharded handle
(kaamer_sharded_search_batch_top_aln_flat, its submit form, kaamer_sharded_index_attach_proteins): every field equals what
kaamer_search_batch_top_aln_flat returns on an unsharded index of the whole database with the whole table attached, and
once the restatement of the aligner (oracle/align_oracle.c).  All shards sit on the one device; the Protein.Sequence table
is partitioned over them by id mod W."""
import os
import re
import threading

import numpy as np
import pytest

from test_top_align import MANY, READS_SEED, _against_oracle, _fasta, _same, check_second_round, indel_queries, many_hits_case, table_without

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_ONLY = bool(os.environ.get("KAAMER_HOST_ONLY"))   # the sanitized CPU build holds the host sources only
NEW_SYMBOLS = ("kaamer_sharded_index_attach_proteins", "kaamer_sharded_search_batch_top_aln_flat", "kaamer_sharded_submit_batch_top_aln_flat")
ALSO = ("kaamer_sharded_index_set_align_budget", "kaamer_sharded_align_info", "kaamer_sharded_index_set_align_timing",
        "kaamer_sharded_align_stage_info")
ALN = dict(sub_matrix="blosum62", gap_open=11, gap_extend=1, text=True)


# ---------------------------------------------------------------- host only
def test_new_symbols_declared_and_bound():
    from kaamer_amd import abi
    src = open(os.path.join(ROOT, "include", "kaamer_hip.h")).read()
    assert re.search(r"#define\s+KAAMER_ABI_VERSION\s+4\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kaamer_[a-z_0-9]+)\s*\(", code))
    for n in NEW_SYMBOLS + ALSO:
        assert n in declared, "include/kaamer_hip.h does not declare %s" % n
        assert n in abi.SYMBOLS, "abi.py does not bind %s" % n


@pytest.mark.skipif(HOST_ONLY, reason="host-only sanitized library")
def test_new_symbols_exported(klib):
    for n in NEW_SYMBOLS + ALSO:
        assert hasattr(klib, n), "libkaamer_hip.so lacks %s" % n
    assert klib.kaamer_abi_version() == 4


# ---------------------------------------------------------------- GPU
def _sharded(api, prot, gpu_device, W, table=None):
    sx = api.ShardedIndex.from_images([prot.image(shard=r, n_shards=W, device=gpu_device) for r in range(W)], [gpu_device] * W)
    if table is not False:
        sx.attach_proteins(prot if table is None else table)
    return sx


def _same_top(got, ref):
    """field for field: order, every alignment number, the three rows, NaN == NaN; the bitmaps where both carry them"""
    assert got.n_queries == ref.n_queries and got.n_reported == ref.n_reported
    assert got.rep_query.tolist() == ref.rep_query.tolist() and got.top_off.tolist() == ref.top_off.tolist()
    assert got.top_pid.tolist() == ref.top_pid.tolist() and got.top_kmatch.tolist() == ref.top_kmatch.tolist()
    assert got.top_first_pos.tolist() == ref.top_first_pos.tolist()
    assert got.trim.tolist() == ref.trim.tolist() and got.meta.tolist() == ref.meta.tolist()
    assert bytes(got.orf_aa) == bytes(ref.orf_aa)
    assert (got.alignments is None) == (ref.alignments is None)
    if ref.alignments is not None:
        assert len(got.alignments) == len(ref.alignments)
        for e, (g, x) in enumerate(zip(got.alignments, ref.alignments)):
            assert _same(g, x), (e, g, x)
    assert (got.pos_bits is None) == (ref.pos_bits is None)
    if ref.pos_bits is not None:
        assert got.pos_bits_len.tolist() == ref.pos_bits_len.tolist() and got.pos_off.tolist() == ref.pos_off.tolist()
        assert np.array_equal(got.pos_bits, ref.pos_bits)


@pytest.fixture(scope="module")
def small(klib, oracle, gpu_device):
    """the 400-protein database (seed 41), the 30 queries of test_protein_batch plus its 40 indel queries, and the
    unsharded one-call result they are compared with (computed once)"""
    from kaamer_amd import api, workload
    db = workload.make_db(400, seed=41)
    prot = api.Proteins.from_fasta(_fasta(workload.unpack(db)).encode())
    ix = api.Index.from_image(prot.image(device=gpu_device), gpu_device)
    ix.attach_proteins(prot)
    qs = workload.unpack(workload.make_protein_queries(db, 30, seed=42)) + indel_queries(workload.unpack(db), 40, 77)
    ref = ix.search_top(qs, max_results=5, align=ALN)
    return dict(db=db, prot=prot, ix=ix, qs=qs, ref=ref)


@pytest.mark.gpu
@pytest.mark.parametrize("W", (1, 2, 3, 8))
def test_protein_equals_unsharded(small, oracle, gpu_device, W):
    from kaamer_amd import api, search
    prot, qs, ref = small["prot"], small["qs"], small["ref"]
    sx = _sharded(api, prot, gpu_device, W)
    top = sx.search_top(qs, max_results=5, align=ALN)
    _same_top(top, ref)
    assert len(top.alignments) > 60 and any(a["aln"] for a in top.alignments)
    info = sx.align_info()
    print("W", W, info)
    assert info["entries"] == 400 - 1 and info["number_of_aa"] == prot.stats()["NumberOfAA"] and info["attempts"] >= 1
    if W > 1:
        # not vacuous: subjects cross devices, and every device holds a reported subject
        crossing, holders = 0, set()
        for i in range(top.n_reported):
            q = int(top.rep_query[i])
            for e in range(int(top.top_off[i]), int(top.top_off[i + 1])):
                p = int(top.top_pid[e])
                crossing += p % W != q % W
                holders.add(p % W)
        assert crossing > 0 and holders == set(range(W))
        assert info["largest_share"] < info["table_bytes"]
        assert info["largest_share"] < small["ix"].align_info()["table_bytes"]
    if W == 3:   # once against the restatement of the aligner, through the drivers (the handle's .proteins: the one-call route)
        qtext = "".join(">q%d\n%s\n" % (i, s.decode()) for i, s in enumerate(qs))
        res = search.ProteinSearch(sx, qtext, search.SearchOptions(MaxResults=5, Align=True))
        n, gaps = _against_oracle(oracle, res, prot.stats()["NumberOfAA"])
        print("alignments %d, gap openings %d" % (n, gaps))
        assert n > 60 and gaps > 20
    sx.close()


@pytest.mark.gpu
def test_reads_w2(small, gpu_device):
    """the aligned query is the ORF after SetBestStartCodon; with positions the bitmaps follow their hits through the re-sort"""
    from kaamer_amd import abi, api, workload
    prot, ix = small["prot"], small["ix"]
    reads = workload.make_reads(small["db"], 400, seed=READS_SEED)
    sx = _sharded(api, prot, gpu_device, 2)
    kw = dict(packed=reads, seq_type=abi.READS, max_results=5)
    ref = ix.search_top(align=ALN, **kw)
    top = sx.search_top(align=ALN, **kw)
    assert int((top.trim > 0).sum()) > 0, "no reported ORF was trimmed: choose another READS_SEED"
    _same_top(top, ref)
    assert sum(a["status"] == 0 for a in top.alignments) > 60
    both_ref = ix.search_top(want_positions=True, align=ALN, **kw)
    both = sx.search_top(want_positions=True, align=ALN, **kw)
    _same_top(both, both_ref)
    plain = sx.search_top(want_positions=True, **kw)
    moved = 0
    for i in range(both.n_reported):
        a, b = int(both.top_off[i]), int(both.top_off[i + 1])
        moved += both.top_pid[a:b].tolist() != plain.top_pid[a:b].tolist()
        gp, pp = both.positions(i), plain.positions(i)
        assert gp.keys() == pp.keys()
        for k in gp:
            assert np.array_equal(gp[k], pp[k]), (i, k)
    assert moved > 0   # else the bitmaps' permutation was exercised nowhere
    sx.close()


@pytest.mark.gpu
def test_edges_w2(klib, gpu_device):
    """the database and queries of test_top_align.test_edges"""
    from kaamer_amd import api, workload
    rng = np.random.default_rng(5)
    base = [s.decode() for s in workload.unpack(workload.make_db(60, seed=9))]
    aa = "ACDEFGHIKLMNPQRSTVWY"
    long_subject = "".join(aa[int(x)] for x in rng.integers(0, 20, 2600))
    recs = list(base)
    recs[3] = recs[3][:40] + "U" + recs[3][41:]               # U in a subject
    recs[5] = recs[5][:30] + "O" + recs[5][31:]               # a subject with a letter outside the alphabet
    recs[7] = long_subject                                    # beyond ALN_WAVE_NS: the long-subject path
    recs.append(recs[-1][:50] + "".join(aa[int(x)] for x in rng.integers(0, 20, 80)))   # shares the previous record's id; this one is stored
    prot = api.Proteins.from_fasta(_fasta(recs).encode())
    ids = prot.ids
    assert ids[-1] == ids[-2]
    ix = api.Index.from_image(prot.image(device=gpu_device), gpu_device)
    ix.attach_proteins(prot)
    sx = _sharded(api, prot, gpu_device, 2)
    assert sx.align_info()["max_subject_len"] == 2600
    queries = [
        ("badletter", base[10][:60] + "O" + base[10][61:120]),
        ("u_query", base[3][:40] + "U" + base[3][41:150]),
        ("star", base[12][:100] + "*"),
        ("long", long_subject[700:900]),
        ("badsubject", base[5][:30] + "A" + base[5][31:150]),
        ("dup", recs[-1][40:]),
        ("nothing", "".join(aa[int(x)] for x in rng.integers(0, 20, 90))),
        ("lower", base[20][:60] + base[20][60:80].lower() + base[20][80:150]),
    ]
    parsed = api.parse_reads("".join(">%s\n%s\n" % q for q in queries), "fasta")
    assert parsed[-1]["seq"][60:80].islower()
    kw = dict(max_results=5, min_k_match=5, min_k_ratio=0.01, align=dict(text=True))
    ref = ix.search_top([q["seq"] for q in parsed], **kw)
    top = sx.search_top([q["seq"] for q in parsed], **kw)
    _same_top(top, ref)
    st = {}
    for i in range(top.n_reported):
        a, b = int(top.top_off[i]), int(top.top_off[i + 1])
        st[queries[int(top.rep_query[i])][0]] = [(int(top.top_pid[e]), top.alignments[e]) for e in range(a, b)]
    assert "nothing" not in st
    assert st["badletter"] and all(al["status"] == 2 for _, al in st["badletter"])
    assert any(al["status"] == 2 for _, al in st["badsubject"])
    assert st["u_query"][0][1]["status"] == 0 and "*" in st["u_query"][0][1]["aln"][0] and "*" in st["u_query"][0][1]["aln"][2]
    assert st["star"][0][1]["status"] == 0
    # the long-subject kernel ran on the query's owner: only ta_wave_kernel<true> finishes a pair whose subject is beyond
    # the wave kernel's row (the other leaves it unaligned), and this one is finished, with the 2600-residue record
    assert any(p == int(ids[7]) and al["status"] == 0 and al["subject_end"] > 700 and al["length"] >= 200 for p, al in st["long"])
    assert len(prot.fetch_hits([int(ids[7])])[0]["Sequence"]) == 2600 > 2048
    assert sx.align_stage_info()["long_waves"] >= 1                 # ... and the owners' stages launched it
    assert any(p == int(ids[-1]) and al["status"] == 0 for p, al in st["dup"])
    assert st["lower"][0][1]["status"] == 0 and st["lower"][0][1]["identity"] < 100.0
    e = sx.search_top([], max_results=5, align=dict(text=True))   # an empty batch
    assert e.n_reported == 0 and e.alignments == []
    sx.close()


@pytest.mark.gpu
def test_hit_without_an_entry_w3(klib, gpu_device):
    """the set-up of test_top_align.test_hit_without_an_entry: the shards hold the whole database, the partitioned table three
    proteins in ten fewer"""
    from kaamer_amd import api, workload
    W = 3
    db = workload.make_db(400, seed=41)
    recs = workload.unpack(db)
    full = api.Proteins.from_fasta(_fasta(recs).encode())
    gone = lambda i: i % 10 in (2, 5, 7)
    sub_text = "".join(">sp|P%05d|N%d%s\n%s\n" % (i, i, " fragment, partial" if gone(i) else "", s.decode()) for i, s in enumerate(recs))
    sub = api.Proteins.from_fasta(sub_text.encode())
    have = set(int(x) for x in sub.ids)
    missing = set(int(x) for x in full.ids) - have
    assert len(missing) >= 100
    ix = api.Index.from_image(full.image(device=gpu_device), gpu_device)
    ix.attach_proteins(sub)
    sx = _sharded(api, full, gpu_device, W, table=sub)
    qs = workload.unpack(workload.make_protein_queries(db, 60, seed=45))
    top = sx.search_top(qs, max_results=8, align=dict(text=True))
    _same_top(top, ix.search_top(qs, max_results=8, align=dict(text=True)))
    plain = sx.search_top(qs, max_results=8)
    on_missing = middle = far = 0
    for i in range(top.n_reported):
        q = int(top.rep_query[i])
        a, b = int(top.top_off[i]), int(top.top_off[i + 1])
        order = plain.top_pid[a:b].tolist()                      # sortMapByValue order
        stat = {int(top.top_pid[e]): top.alignments[e]["status"] for e in range(a, b)}
        first = next((k for k, p in enumerate(order) if p in missing), len(order))
        assert [stat[p] for p in order] == [0] * first + [4] * (len(order) - first), (i, order, stat)
        got = [int(top.top_pid[e]) for e in range(a, b)]
        assert got[first:] == order[first:]                      # BitScore 0: behind the aligned hits, in sortMapByValue order
        on_missing += first < len(order)
        middle += 0 < first < len(order) - 1
        far += first < len(order) and order[first] % W != q % W
    assert on_missing > 0 and middle > 0 and far > 0
    sx.close()


@pytest.mark.gpu
def test_more_than_64_hits_of_one_query_w3(klib, gpu_device):
    """the set-up of test_top_align.test_more_than_64_hits_of_one_query: the second round of tas_pairs_kernel's walk over a
    query's hits, with the full table and with a first id without an entry in that round"""
    from kaamer_amd import api
    W = 3
    recs, qs = many_hits_case()
    full = api.Proteins.from_fasta(_fasta(recs).encode())
    ix = api.Index.from_image(full.image(device=gpu_device), gpu_device)
    ix.attach_proteins(full)
    sx = _sharded(api, full, gpu_device, W)
    plain = sx.search_top(qs, **MANY)
    long_i = plain.rep_query.tolist().index(1)
    assert int(plain.top_off[long_i + 1] - plain.top_off[long_i]) == 70
    _same_top(sx.search_top(qs, align=dict(text=True), **MANY), ix.search_top(qs, align=dict(text=True), **MANY))
    pid = int(plain.top_pid[int(plain.top_off[long_i]) + 66])
    sub = table_without(recs, full, pid)
    ix.attach_proteins(sub)   # (a second attach replaces the first)
    sx.attach_proteins(sub)
    top = sx.search_top(qs, align=dict(text=True), **MANY)
    check_second_round(top, plain, long_i, pid)
    _same_top(top, ix.search_top(qs, align=dict(text=True), **MANY))
    sx.close()


@pytest.mark.gpu
def test_options(small, gpu_device):
    from kaamer_amd import abi, api
    prot, ix, qs = small["prot"], small["ix"], small["qs"]
    sx = _sharded(api, prot, gpu_device, 2)
    plain = sx.search_top(qs, max_results=5)
    assert plain.alignments is None
    for aln in (dict(gap_open=12, gap_extend=2), dict(sub_matrix="blosum45", gap_open=12, gap_extend=2)):
        r = sx.search_top(qs, max_results=5, align=aln)
        assert len(r.alignments) == len(plain.top_pid) > 0 and all(a["status"] == 1 and a["bitscore"] == 0.0 for a in r.alignments)
        assert r.top_pid.tolist() == plain.top_pid.tolist() and r.top_kmatch.tolist() == plain.top_kmatch.tolist()
    bare = _sharded(api, prot, gpu_device, 2, table=False)
    with pytest.raises(abi.KaamerError) as ei:
        bare.search_top(qs, max_results=5, align=dict())
    assert ei.value.code == abi.E_ARG
    bare.close()
    nums = sx.search_top(qs, max_results=5, align=dict(text=False))
    _same_top(nums, ix.search_top(qs, max_results=5, align=dict(text=False)))
    strip = lambda a: {k: v for k, v in a.items() if k != "aln"}
    assert all(_same(strip(a), strip(b)) for a, b in zip(nums.alignments, small["ref"].alignments))
    assert all(a["aln"] is None for a in nums.alignments)
    # calls with and without alignments, with and without positions, alternate on one handle
    refs = {(al, pos): ix.search_top(qs, max_results=5, want_positions=pos, align=ALN if al else None) for al in (0, 1) for pos in (False, True)}
    for _ in range(2):
        for key in ((1, False), (0, False), (1, True), (0, True), (1, False)):
            _same_top(sx.search_top(qs, max_results=5, want_positions=key[1], align=ALN if key[0] else None), refs[key])
    sx.close()


@pytest.mark.gpu
def test_budget_of_one_slab(small, gpu_device):
    from kaamer_amd import api
    sx = _sharded(api, small["prot"], gpu_device, 2)
    _same_top(sx.search_top(small["qs"], max_results=5, align=ALN), small["ref"])
    sx.set_align_budget(1)
    _same_top(sx.search_top(small["qs"], max_results=5, align=ALN), small["ref"])
    sx.set_align_budget(0)
    sx.close()


@pytest.mark.gpu
def test_bounds_grow(small, gpu_device):
    """a 5-query batch, then the 70 queries on the same handle: segments sized from the first call (need + a quarter) are too
    small, the batch is repeated inside wait; the third call takes one attempt with segments within the +25 % rule"""
    from kaamer_amd import api
    ix, qs = small["ix"], small["qs"]
    sx = _sharded(api, small["prot"], gpu_device, 2)
    _same_top(sx.search_top(qs[:5], max_results=5, align=ALN), ix.search_top(qs[:5], max_results=5, align=ALN))
    first = sx.align_info()
    assert first["attempts"] == 1
    _same_top(sx.search_top(qs, max_results=5, align=ALN), small["ref"])
    second = sx.align_info()
    print("tiny:", first, "big:", second)
    assert second["attempts"] > 1 and second["need_bytes"] > first["need_bytes"] + first["need_bytes"] // 4 + 256     # beyond what the first call sized
    _same_top(sx.search_top(qs, max_results=5, align=ALN), small["ref"])
    third = sx.align_info()
    print("again:", third)
    assert third["attempts"] == 1 and third["need_bytes"] == second["need_bytes"]
    assert third["need_bytes"] <= third["segment_bytes"] <= 1.5 * third["need_bytes"]
    sx.close()


@pytest.mark.gpu
def test_three_tickets_from_three_threads(small, gpu_device):
    from kaamer_amd import api
    ix, qs = small["ix"], small["qs"]
    batches = [qs[:30], qs[30:], qs[10:50]]
    refs = [ix.search_top(b, max_results=5, align=ALN) for b in batches]
    sx = _sharded(api, small["prot"], gpu_device, 2)
    for _ in range(2):
        tickets, got, errs = [None] * 3, [None] * 3, []
        gate = threading.Barrier(3)

        def submit(i):
            try:
                gate.wait()
                tickets[i] = sx.submit_top(batches[i], max_results=5, align=ALN)
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
            _same_top(got[i], refs[i])
    t = sx.submit_top(batches[0], max_results=5, align=ALN)
    t.discard()
    _same_top(sx.search_top(batches[1], max_results=5, align=ALN), refs[1])
    sx.close()


@pytest.mark.gpu
def test_a_failing_first_attempt_is_repeated_as_a_whole(klib, gpu_device):
    """the set-up of test_sharded_top_positions.test_a_failing_shard_fails_the_whole_call, with alignments: the shards' first
    searches overflow their hit pools and exchange blocks, so the first attempt fails on every owner.  Nothing of it is
    handed out: the call repeats the batch as a whole and returns every alignment; the next call on the handle succeeds."""
    from kaamer_amd import api, workload
    db = workload.make_db_zipf(40000, seed=11, n_motifs=1500, zipf_a=1.0, per_residues=60)
    q = workload.make_protein_queries(db, 200, seed=12)
    prot = api.Proteins.from_fasta(_fasta(workload.unpack(db)).encode())
    ix1 = api.Index.from_image(prot.image(device=gpu_device), gpu_device)
    ix1.attach_proteins(prot)
    ref = ix1.search_top(packed=q, align=ALN)
    sx = _sharded(api, prot, gpu_device, 2)
    e_cap = 2 * len(q[0]) // 2 + 65536      # entries per (shard -> owner) block of a first attempt
    top = sx.search_top(packed=q, align=ALN)
    assert not sx.exchange_info()["adaptive"] and sx.exchange_info()["need_entries"] > e_cap
    assert sx.align_info()["attempts"] > 1
    _same_top(top, ref)
    assert len(top.alignments) == int(top.top_off[-1]) > 0 and sum(a["status"] == 0 for a in top.alignments) > 200
    _same_top(sx.search_top(packed=q, align=ALN), ref)
    sx.close()


@pytest.mark.gpu
def test_a_call_that_fails_returns_nothing_and_the_next_succeeds(small, gpu_device):
    """a MaxResults for which an owner's result block cannot be allocated (2^31 - 1 hits x 12 bytes per query: terabytes):
    the aligning call ends in an error on search and on submit, hands nothing out and leaves the set free; the calls that
    follow on the handle, sized from before the failure, equal the unsharded call's"""
    from kaamer_amd import abi, api
    qs, ref = small["qs"], small["ref"]
    sx = _sharded(api, small["prot"], gpu_device, 2)
    _same_top(sx.search_top(qs, max_results=5, align=ALN), ref)
    before = sx.align_info()
    for _ in range(4):                       # more failures than the handle has sets: each gives its set back
        with pytest.raises(abi.KaamerError) as ei:
            sx.search_top(qs, max_results=2 ** 31 - 1, align=ALN)
        assert ei.value.code == abi.E_NOMEM
        with pytest.raises(abi.KaamerError):
            sx.submit_top(qs, max_results=2 ** 31 - 1, align=ALN)
    assert sx.align_info() == before         # a call that never ran leaves the last finished call's figures
    _same_top(sx.search_top(qs, max_results=5, align=ALN), ref)
    _same_top(sx.search_top(qs, max_results=5, want_positions=True, align=ALN),
              small["ix"].search_top(qs, max_results=5, want_positions=True, align=ALN))
    assert sx.align_info()["attempts"] == 1
    sx.close()
