"""tests/windowcases.py proves its own fixtures (no GPU): the database has the list lengths it promises, every case meets the
target it claims -- by window_extras, the restated flat layout, and by the oracle's hit counts -- and every target of the
lists (head boundary, xtotal, owner marks, table fill, hint bound, runs; protein and ORF forms) is met by some case."""
import numpy as np
import pytest

import gtierref
import windowcases as wc


@pytest.fixture(scope="module")
def d(oracle):
    return wc.database(oracle)


def test_database_lists(d, oracle):
    assert 3000 < len(d.db) < 12000 and len(set(d.ids.tolist())) == len(d.db) and int((d.ids >= 2 ** 31).sum()) == 1
    assert max(len(p) for p in d.db) <= wc.CORE + 40
    for fam, n in wc.FAMILIES.items():
        f = d.figures(d.core[fam])
        assert f.size == wc.CORE - 6 and (f.cnt == n).all() and f.D == n, fam
        pid, km, _ = d.oix.search(d.core[fam])
        assert len(pid) == n and (km == wc.CORE - 6).all(), fam
    # a list of one is a list when its id cannot be inline (kaamer_layout.h: KH_INLINE_BIT), and only then
    lo, hi = d.figures(d.core["1"]), d.figures(d.core["1hi"])
    assert (lo.n_lists, lo.n_list_ids) == (0, 0) and (hi.n_lists, hi.n_list_ids) == (hi.size, hi.size) and hi.distinct.tolist() == [wc.HI_ID]
    two = d.figures(d.core["2"])
    assert (two.n_lists, two.n_list_ids) == (two.size, 2 * two.size)
    for n, k in d.kmer.items():
        assert d.counts(k + b"WWWWWW").tolist()[0] == n
    for n, c in d.big.items():
        assert len(d.oix.search(c)[0]) == n and (d.counts(c) == n).all()


def test_restated_table_and_layout_by_hand(d, oracle):
    # table_home and the occupancy walk on values worked out by hand
    assert wc.table_home([0, 1, 3], 64).tolist() == [0, (0x9E3779B1 * 64) >> 32, ((3 * 0x9E3779B1 & 0xFFFFFFFF) * 64) >> 32]
    assert wc.table_home([0xFFFFFFFE], 4096).tolist() == [((0xFFFFFFFE * 0x9E3779B1 & 0xFFFFFFFF) * 4096) >> 32]
    same = [i for i in range(2000) if wc.table_home([i], 64)[0] == 63][:3]        # three ids whose home is the last slot: the run wraps
    assert len(same) == 3 and wc.longest_run(same, 64) == 3 and wc.longest_run([5], 64) == 1
    assert wc.longest_run(np.arange(64), 64) == 64 and wc.longest_run(np.arange(640) * 3 + 1, 4096) < 20
    assert [gtierref.table_slots_for(s) for s in (7, 43, 44, 85, 86, 2731, 8300)] == [64, 64, 128, 128, 192, 4096, 4096]
    # the flat layout: 64 positions of F_3 are one window of 128 further ids, two a lane; the 65th position opens window 1
    w = wc.window_extras(d, [d.core["3"][:71]])
    assert len(w) == 2 and w[0].xtotal == 128 and w[0].pref.tolist() == list(range(0, 128, 2)) and w[1].xtotal == 2
    assert w[1].q.tolist() == [0] + [-1] * 63 and w[1].pos[0] == 64
    # two queries share window 0; a query of fewer than 7 k-mers is not searched
    w = wc.window_extras(d, [d.core["2"][:16], b"ACDEFG", d.core["4"][:20]])
    assert len(w) == 1 and w[0].q[:25].tolist() == [0] * 10 + [1] * 14 + [-1] and w[0].xtotal == 10 + 3 * 14 and w[0].pref[10] == 10
    # the single-window condition: 65 tables of 64 slots start in two windows of 4096 slots, 33 in two of 2048
    with pytest.raises(AssertionError):
        wc.window_extras(d, [d.core["2"][:13]] * 65)
    assert len(wc.window_extras(d, [d.core["2"][:13]] * 64)) == 7
    with pytest.raises(AssertionError):
        wc.window_extras(d, [d.core["2"][:13]] * 33, shift=gtierref.GRP_SHIFT)
    # ORFs: oracle.get_orfs order, a pack is the tables that start in 512 slots
    read = wc.nt(d.core["3"][:64])
    orfs = [o["seq"].encode() for o in oracle.get_orfs(read)]
    units = wc.window_extras(d, [read], nucleotide=True, single=False)
    assert sum(len(u) for u in units) >= 1
    assert sum(int((w.q >= 0).sum()) for u in units for w in u) == sum(oracle.size_in_kmer(o) for o in orfs if oracle.size_in_kmer(o) >= 7)
    assert sum(w.xtotal for u in units for w in u) == 2 * 58


def test_compose_junctions(d):
    rng = np.random.default_rng(5)
    seq, at = wc.compose(d, [("4", 42), ("2", 1), ("random", 30)], rng)
    cnt = d.counts(seq)
    assert at == [0, 48, 55] and len(cnt) == 42 + 6 + 1 + 6 + 30
    assert (cnt[:42] == 4).all() and not cnt[42:48].any() and cnt[48] == 2 and not cnt[49:].any()


def _met(d, cases, anywhere):
    met = set()
    for c in cases:
        for claim in c.claims:
            assert wc.check_claim(d, c, claim, anywhere=anywhere), "%r does not meet %r" % (c, claim)
            met.add(claim)
    return met


def test_every_protein_target_is_met(d, oracle):
    # the xtotal targets are the two sides of XIT * 64 and of the end of every round of GRP_LONG_UNROLL chunks behind it
    ends = [gtierref.XIT * 64 + r * gtierref.GRP_LONG_UNROLL * 64 for r in range(3)]
    assert ends == [128, 384, 640] and all(e + k in wc.XTOTALS for e in ends for k in (-1, 0, 1))
    met = _met(d, wc.cases(oracle), False)
    missing = [t for t in wc.required_targets()[0] if t not in met]
    assert not missing, "no case meets %r" % missing
    print("protein targets met: %s" % sorted(met, key=repr))


def test_every_orf_target_is_met(d, oracle):
    cases = wc.orf_cases(oracle)
    met = _met(d, cases, True)
    missing = [t for t in wc.required_targets()[1] if t not in met]
    assert not missing, "no ORF case meets %r" % missing
    print("ORF targets met: %s" % sorted(met, key=repr))
    # both arenas: reads of at most 200 nt (PK_ARENA_ORF) and longer sequences (PK_ARENA_ORF_LONG); the ORF of interest is
    # counted in LDS, not sent on unseen
    assert any(len(c.seqs[0]) <= 192 for c in cases) and any(len(c.seqs[0]) > 200 for c in cases)
    for c in cases:
        if c.name.startswith("d:"):
            assert len(c.seqs[0]) <= 192, c
            sizes = [oracle.size_in_kmer(o["seq"]) for o in oracle.get_orfs(c.seqs[0])]
            assert max(sizes) <= 44 and not any(gtierref.pack_sends_unseen(s, False) for s in sizes), c


def test_oracle_hit_counts(d, oracle):
    """the oracle's distinct hits of every case are what the case says"""
    for c in wc.cases(oracle):
        hits = [len(d.oix.search(q)[0]) for q in c.seqs]
        sizes = [oracle.size_in_kmer(q) for q in c.seqs]
        if c.kind == "a":
            assert hits == [wc.FAMILIES[c.claims[0][1]]], c
        elif c.kind == "d":
            ids, slots = c.claims[0][1:]
            assert hits == [ids] and gtierref.table_slots_for(sizes[0]) == slots, c
            assert c.overflow == {(63, 64): 0, (64, 64): 0, (65, 64): 1, (65, 128): 0, (128, 128): None, (129, 128): 1,
                                  (4096, 4096): None, (4097, 4096): 1}[(ids, slots)], c
        elif c.kind == "e":
            assert 8192 < sizes[-1] < gtierref.LDS_MAX_SIZE and 0 < hits[-1] < gtierref.table_slots_for(sizes[-1]) // 2, c
        elif c.kind == "f":
            assert all(h in (2, 3, 6) for h in hits), c
            if len(c.seqs) == 20:     # every query its own count of 7 for each of the six proteins
                assert all(d.oix.search(q)[1].tolist() == [7] * 6 for q in c.seqs), c
        if len(c.seqs) > 1:           # one unit in the count (units of 1 << GRP_SHIFT + 1 slots) and in the PositionHits pass
            assert wc.window_extras(d, c.seqs) and wc.window_extras(d, c.seqs, shift=gtierref.GRP_SHIFT), c
        if c.kind != "d":
            assert c.overflow == 0, c
    # 0 is exact for a, b, c, e, f and the ORF forms because no table add can run out of probes: at most the longest
    # occupied run of the table is walked, and that is below GRP_MAX_PROBES in every table (d's crowded ones apart)
    for c in wc.cases(oracle) + wc.orf_cases(oracle):
        if c.overflow == 0:
            for q in wc.searched_queries(d, c.seqs, c.nucleotide):
                size = oracle.size_in_kmer(q)
                if size >= 7:
                    f = d.figures(q)
                    assert f.D <= gtierref.table_slots_for(size) and wc.longest_run(f.distinct, gtierref.table_slots_for(size)) < gtierref.GRP_MAX_PROBES, c
