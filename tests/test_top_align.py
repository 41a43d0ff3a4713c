"""The alignment of the reported hits inside the top-N call (kaamer_search_batch_top_aln_flat, its submit / device-resident
forms, kaamer_index_attach_proteins) against the restatement of the aligner (oracle/align_oracle.c) and against the route
it replaces: ProteinSearch / FastqSearch -> FetchHitsInformation -> AlignHits (kaamer_align_pairs), field for field."""
import math
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

READS_SEED = 5   # chosen on the CPU with the oracle: reported ORFs of this batch include trimmed ones (asserted below)


def _fasta(recs, prefix="P"):
    return "".join(">sp|%s%05d|N%d\n%s\n" % (prefix, i, i, s if isinstance(s, str) else s.decode()) for i, s in enumerate(recs))


def _db(n, seed, gpu_device):
    """-> (Proteins, index without a table: the existing route, index with the table attached: the one-call route)"""
    from kaamer_amd import api, workload
    prot = api.Proteins.from_fasta(_fasta(workload.unpack(workload.make_db(n, seed=seed))).encode())
    img = prot.image(device=gpu_device)
    old, new = api.Index.from_image(img, gpu_device), api.Index.from_image(img, gpu_device)
    new.attach_proteins(prot)
    return prot, old, new


def _same(a, b):
    """equality of two results of the drivers, NaN == NaN"""
    if isinstance(a, float) and isinstance(b, float):
        return a == b or (math.isnan(a) and math.isnan(b))
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, list) and isinstance(b, list):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def _routes(driver, old, new, prot, text, opts, gpu_device):
    from kaamer_amd import search
    exp = search.AlignHits(search.FetchHitsInformation(driver(old, text, opts), prot), prot, opts, device=gpu_device)
    opts.Align = True
    got = driver(new, text, opts)
    opts.Align = False
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert _same(g, e), (g["Query"]["Name"], g, e)
    return got


def _against_oracle(oracle, res, n_aa):
    n = gaps = 0
    for qr in res:
        hits = qr["SearchResults"]["Hits"]
        bits = [h["Alignment"]["BitScore"] for h in hits]
        assert bits == sorted(bits, reverse=True)
        for h in hits:
            exp = oracle.align(qr["Query"]["Sequence"], qr["HitEntries"][h["Key"]]["Sequence"], n_aa)
            a = h["Alignment"]
            assert (a["Raw"], a["Length"], a["Mismatches"], a["GapOpenings"]) == (exp["raw"], exp["length"], exp["mismatches"], exp["gap_openings"])
            assert a["BitScore"] == exp["bitscore"] and a["EValue"] == exp["evalue"]
            assert a["Identity"] == exp["identity"] and a["Similarity"] == exp["similarity"]
            assert a["AlnString"] == "\n".join(exp["aln"])
            assert (a["QueryStart"], a["QueryEnd"], a["SubjectStart"], a["SubjectEnd"]) == (exp["q_start"], exp["q_end"], exp["s_start"], exp["s_end"])
            n += 1
            gaps += exp["gap_openings"]
    return n, gaps


def indel_queries(db, n, seed):
    """database members with a few substitutions and two to four insertions / deletions of 1..6 residues each"""
    rng = np.random.default_rng(seed)
    aa = "ACDEFGHIKLMNPQRSTVWY"
    out = []
    for _ in range(n):
        s = list(db[int(rng.integers(0, len(db)))].decode()[:int(rng.integers(120, 400))])
        for _ in range(len(s) // 20):
            s[int(rng.integers(0, len(s)))] = aa[int(rng.integers(0, 20))]
        for _ in range(int(rng.integers(2, 5))):
            at, ln = int(rng.integers(10, len(s) - 10)), int(rng.integers(1, 7))
            if rng.random() < 0.5:
                del s[at:at + ln]
            else:
                s[at:at] = [aa[int(rng.integers(0, 20))] for _ in range(ln)]
        out.append("".join(s).encode())
    return out


def test_protein_batch(klib, oracle, gpu_device):
    """the database and the 30 queries of test_search_then_align_like_query_result_handler, MaxResults 5.  Those queries
    are substitution-only mutants: against this database they give 96 alignments with 3 gap openings in all (the oracle,
    worked out on the CPU), short of the more than 20 the comparison has to cover.  40 queries with insertions and
    deletions are therefore compared in the same call, next to the 30, never instead of them."""
    from kaamer_amd import search, workload
    prot, old, new = _db(400, 41, gpu_device)
    db = workload.make_db(400, seed=41)
    qs = workload.unpack(workload.make_protein_queries(db, 30, seed=42)) + indel_queries(workload.unpack(db), 40, 77)
    qtext = "".join(">q%d\n%s\n" % (i, s.decode()) for i, s in enumerate(qs))
    res = _routes(search.ProteinSearch, old, new, prot, qtext, search.SearchOptions(MaxResults=5), gpu_device)
    n, gaps = _against_oracle(oracle, res, prot.stats()["NumberOfAA"])
    print("alignments %d, gap openings %d" % (n, gaps))
    assert n > 60 and gaps > 20
    info = new.align_info()
    assert info["table_bytes"] > 0 and info["entries"] == 400 - 1 and info["waves"] >= 1   # (the FASTA reader's last two records share an id)


def test_reads_batch(klib, oracle, gpu_device):
    """the aligned query is the ORF after SetBestStartCodon; with positions the bitmaps follow their hits through the re-sort"""
    from kaamer_amd import abi, search, workload
    prot, old, new = _db(400, 41, gpu_device)
    reads = workload.make_reads(workload.make_db(400, seed=41), 400, seed=READS_SEED)
    text = workload.fastq_text(reads)
    res = _routes(search.FastqSearch, old, new, prot, text, search.SearchOptions(SequenceType=abi.READS, MaxResults=5), gpu_device)
    n, _ = _against_oracle(oracle, res, prot.stats()["NumberOfAA"])
    assert n > 60
    aln = dict(sub_matrix="blosum62", gap_open=11, gap_extend=1, text=True)
    top = new.search_top(packed=reads, seq_type=abi.READS, max_results=5, align=aln)
    assert int((top.trim > 0).sum()) > 0, "no reported ORF was trimmed: choose another READS_SEED"
    # Query.Sequence of a trimmed ORF is the ORF without the residues SetBestStartCodon removed: against the untrimmed ORFs
    # of the full-list call (same queries, same order)
    full = new.search(packed=reads, seq_type=abi.READS)
    for i in np.nonzero(top.trim > 0)[0]:
        q, t = int(top.rep_query[i]), int(top.trim[i])
        m = full.meta[q]
        whole = bytes(full.orf_aa[int(m["aa_off"]):int(m["aa_off"]) + int(m["aa_len"])])
        assert int(top.meta["aa_len"][i]) == int(m["aa_len"]) - t
        got = bytes(top.orf_aa[int(top.meta["aa_off"][i]):int(top.meta["aa_off"][i]) + int(top.meta["aa_len"][i])])
        assert got == whole[t:]
        a = int(top.top_off[i])
        al = top.alignments[a]
        assert al["status"] == 0 and al["aln"][0].replace("-", "") == got[al["query_start"] - 1:al["query_end"]].decode()
    plain = new.search_top(packed=reads, seq_type=abi.READS, max_results=5, want_positions=True)
    both = new.search_top(packed=reads, seq_type=abi.READS, max_results=5, want_positions=True, align=aln)
    assert both.rep_query.tolist() == plain.rep_query.tolist() and both.pos_bits_len.tolist() == plain.pos_bits_len.tolist()
    assert both.top_pid.tolist() == top.top_pid.tolist() and [a["raw"] for a in both.alignments] == [a["raw"] for a in top.alignments]
    moved = 0
    for i in range(both.n_reported):
        a, b = int(both.top_off[i]), int(both.top_off[i + 1])
        assert sorted(both.top_pid[a:b].tolist()) == sorted(plain.top_pid[a:b].tolist())
        moved += both.top_pid[a:b].tolist() != plain.top_pid[a:b].tolist()
        gp, pp = both.positions(i), plain.positions(i)
        assert gp.keys() == pp.keys()
        for k in gp:
            assert np.array_equal(gp[k], pp[k]), (i, k)
        km = dict(zip(plain.top_pid[a:b].tolist(), zip(plain.top_kmatch[a:b].tolist(), plain.top_first_pos[a:b].tolist())))
        assert [km[p] for p in both.top_pid[a:b].tolist()] == list(zip(both.top_kmatch[a:b].tolist(), both.top_first_pos[a:b].tolist()))
    print("queries whose hits the re-sort moved: %d of %d" % (moved, both.n_reported))
    assert moved > 0   # else the bitmaps' permutation was exercised nowhere


def test_edges(klib, oracle, gpu_device):
    from kaamer_amd import abi, api, search, workload
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
    img = prot.image(device=gpu_device)
    old, new = api.Index.from_image(img, gpu_device), api.Index.from_image(img, gpu_device)
    new.attach_proteins(prot)
    assert new.align_info()["max_subject_len"] == 2600
    queries = [
        ("badletter", base[10][:60] + "O" + base[10][61:120]),          # a query letter outside the alphabet: status 2
        ("u_query", base[3][:40] + "U" + base[3][41:150]),              # U in the query and in its subject
        ("star", base[12][:100] + "*"),                                 # a query ending in '*'
        ("long", long_subject[700:900]),                                # hits the 2600-residue subject
        ("badsubject", base[5][:30] + "A" + base[5][31:150]),           # hits the subject that holds an O
        ("dup", recs[-1][40:]),                                         # hits the duplicated last id
        ("nothing", "".join(aa[int(x)] for x in rng.integers(0, 20, 90))),
        # the reader upper-cases every record but the last: a lower-case stretch (its k-mers are map misses, the rest of the
        # query finds the hit) that the aligner folds and the identity count, on raw bytes, does not
        ("lower", base[20][:60] + base[20][60:80].lower() + base[20][80:150]),
    ]
    qtext = "".join(">%s\n%s\n" % q for q in queries)
    parsed = api.parse_reads(qtext, "fasta")
    assert parsed[-1]["seq"][60:80].islower() and parsed[0]["seq"].isupper()
    opts = search.SearchOptions(MaxResults=5, MinKMatch=5, MinKRatio=0.01)
    res = _routes(search.ProteinSearch, old, new, prot, qtext, opts, gpu_device)
    by_name = {qr["Query"]["Name"]: qr for qr in res}
    assert "nothing" not in by_name
    top = new.search_top([q["seq"] for q in parsed], max_results=5, min_k_match=5, min_k_ratio=0.01, align=dict(text=True))
    st = {}
    for i in range(top.n_reported):
        name = queries[int(top.rep_query[i])][0]
        a, b = int(top.top_off[i]), int(top.top_off[i + 1])
        st[name] = [(int(top.top_pid[e]), top.alignments[e]) for e in range(a, b)]
    assert st["badletter"] and all(al["status"] == 2 for _, al in st["badletter"])
    assert any(al["status"] == 2 for _, al in st["badsubject"])
    assert st["u_query"][0][1]["status"] == 0 and "*" in st["u_query"][0][1]["aln"][0] and "*" in st["u_query"][0][1]["aln"][2]
    assert st["star"][0][1]["status"] == 0
    assert any(p == int(ids[7]) and al["status"] == 0 and al["subject_end"] > 700 and al["length"] >= 200 for p, al in st["long"])
    assert len(prot.fetch_hits([int(ids[7])])[0]["Sequence"]) == 2600     # the pair's subject is the 2600-residue record
    assert new.align_info()["long_waves"] >= 1
    assert any(p == int(ids[-1]) and al["status"] == 0 for p, al in st["dup"])
    low = st["lower"][0][1]
    assert low["status"] == 0 and low["length"] > 100 and low["gap_openings"] == 0
    cols = [k for k, c in enumerate(low["aln"][0]) if c.islower()]
    assert len(cols) == 20 and low["mismatches"] >= 20 and low["identity"] < 100.0       # identity on raw bytes: a != A ...
    assert all(low["aln"][1][k] == " " and low["aln"][2][k] == low["aln"][0][k].upper() for k in cols)   # ... a map miss marks nothing,
    assert low["raw"] >= sum(int(klib.kaamer_align_matrix_entry(ord(c), ord(c))) for c in base[20][60:80])   # and the DP scored the folded letters
    # an empty batch
    e = new.search_top([], max_results=5, align=dict(text=True))
    assert e.n_reported == 0 and e.alignments == []


def test_hit_without_an_entry(klib, gpu_device):
    """a reported hit id with no entry in the attached table: the index holds the whole database, the table three proteins
    in ten fewer (their records carry ", partial": the FASTA reader drops them without renumbering the others).
    FetchHitsInformation stops a query's loop at the first such id (search.go:461-463), so that hit AND the query's later
    ones keep the empty AlignmentResult and sort behind the aligned ones; against the existing route on the same table"""
    from kaamer_amd import api, search, workload
    db = workload.make_db(400, seed=41)
    recs = workload.unpack(db)
    full = api.Proteins.from_fasta(_fasta(recs).encode())
    gone = lambda i: i % 10 in (2, 5, 7)
    sub_text = "".join(">sp|P%05d|N%d%s\n%s\n" % (i, i, " fragment, partial" if gone(i) else "", s.decode()) for i, s in enumerate(recs))
    sub = api.Proteins.from_fasta(sub_text.encode())
    have = set(int(x) for x in sub.ids)
    missing = set(int(x) for x in full.ids) - have
    assert len(missing) >= 100 and have < set(int(x) for x in full.ids)
    img = full.image(device=gpu_device)
    old, new = api.Index.from_image(img, gpu_device), api.Index.from_image(img, gpu_device)
    new.attach_proteins(sub)
    qs = workload.unpack(workload.make_protein_queries(db, 60, seed=45))
    qtext = "".join(">q%d\n%s\n" % (i, s.decode()) for i, s in enumerate(qs))
    opts = search.SearchOptions(MaxResults=8)
    res = _routes(search.ProteinSearch, old, new, sub, qtext, opts, gpu_device)
    assert any(set(h["Key"] for h in qr["SearchResults"]["Hits"]) - set(qr["HitEntries"]) for qr in res)
    top = new.search_top(qs, max_results=8, align=dict(text=True))
    plain = new.search_top(qs, max_results=8)
    on_missing = later = middle = 0
    for i in range(top.n_reported):
        a, b = int(top.top_off[i]), int(top.top_off[i + 1])
        order = plain.top_pid[a:b].tolist()                      # sortMapByValue order
        stat = {int(top.top_pid[e]): top.alignments[e]["status"] for e in range(a, b)}
        first = next((k for k, p in enumerate(order) if p in missing), len(order))
        # the rule, hit by hit: aligned before the first missing id, status 4 from it on
        assert [stat[p] for p in order] == [0] * first + [4] * (len(order) - first), (i, order, stat)
        got = [int(top.top_pid[e]) for e in range(a, b)]
        assert got[first:] == order[first:]                      # BitScore 0: behind the aligned hits, in sortMapByValue order
        assert all(top.alignments[a + k]["bitscore"] == 0.0 and top.alignments[a + k]["length"] == 0 for k in range(first, len(order)))
        on_missing += first < len(order)
        later += any(p in have for p in order[first + 1:])
        middle += 0 < first < len(order) - 1
    print("queries with a missing hit %d, with a later hit that has an entry %d, with the missing hit in the middle %d" % (on_missing, later, middle))
    assert on_missing > 0 and later > 0 and middle > 0


MANY = dict(min_k_ratio=0.0, min_k_match=1, max_results=70)


def many_hits_case():
    """-> (records of a 400-protein database, three queries): two ordinary queries and, between them, the concatenation of
    the database's 80 shortest records, which reports MaxResults = 70 hits under MANY: more than the 64 a wave classifies
    per round.  (The shortest: the restatement of the aligner costs query x subject.)"""
    from kaamer_amd import workload
    db = workload.make_db(400, seed=43)
    recs = workload.unpack(db)
    pick = sorted(range(390), key=lambda i: (len(recs[i]), i))[:80]   # (the FASTA reader's last two records share an id)
    two = workload.unpack(workload.make_protein_queries(db, 2, seed=44))
    return recs, [two[0], b"".join(recs[i] for i in pick), two[1]]


def table_without(recs, full, pid):
    """the protein table of `recs` without the one record whose id is pid (", partial": dropped without renumbering the others)"""
    from kaamer_amd import api
    ids = full.ids.tolist()
    assert ids.count(pid) == 1
    gone = ids.index(pid)
    sub = api.Proteins.from_fasta("".join(">sp|P%05d|N%d%s\n%s\n" % (i, i, " fragment, partial" if i == gone else "", s.decode())
                                          for i, s in enumerate(recs)).encode())
    assert set(ids) - set(sub.ids.tolist()) == {pid}
    return sub


def check_second_round(top, plain, long_i, pid):
    """the long query's hits, in sortMapByValue order: aligned before the id without an entry, status 4 from it on"""
    a, b = int(top.top_off[long_i]), int(top.top_off[long_i + 1])
    order = plain.top_pid[a:b].tolist()
    stat = {int(top.top_pid[e]): top.alignments[e]["status"] for e in range(a, b)}
    first = order.index(pid)
    assert b - a == 70 and first >= 64
    assert [stat[p] for p in order] == [0] * first + [4] * (len(order) - first), (order, stat)


def test_more_than_64_hits_of_one_query(klib, oracle, gpu_device):
    """a query that reports 70 hits: the second round of ta_pairs_kernel's walk over a query's hits, 64 at a time, and a
    first id without an entry that falls into that round"""
    from kaamer_amd import api, search
    recs, qs = many_hits_case()
    full = api.Proteins.from_fasta(_fasta(recs).encode())
    new = api.Index.from_image(full.image(device=gpu_device), gpu_device)
    new.attach_proteins(full)
    plain = new.search_top(qs, **MANY)
    long_i = plain.rep_query.tolist().index(1)
    assert int(plain.top_off[long_i + 1] - plain.top_off[long_i]) == 70
    qtext = "".join(">q%d\n%s\n" % (i, s.decode()) for i, s in enumerate(qs))
    res = search.ProteinSearch(new, qtext, search.SearchOptions(MaxResults=70, MinKRatio=0.0, MinKMatch=1, Align=True))
    assert len(res[1]["SearchResults"]["Hits"]) == 70
    n, _ = _against_oracle(oracle, res, full.stats()["NumberOfAA"])
    assert n >= 70
    pid = int(plain.top_pid[int(plain.top_off[long_i]) + 66])
    new.attach_proteins(table_without(recs, full, pid))   # (a second attach replaces the first)
    check_second_round(new.search_top(qs, align=dict(text=True), **MANY), plain, long_i, pid)


def test_options(klib, gpu_device):
    from kaamer_amd import abi, api, workload
    prot, old, new = _db(400, 41, gpu_device)
    q = workload.make_protein_queries(workload.make_db(400, seed=41), 30, seed=42)
    plain = new.search_top(packed=q, max_results=5)
    for aln in (dict(gap_open=12, gap_extend=2), dict(sub_matrix="blosum45", gap_open=12, gap_extend=2), dict(sub_matrix="blosum45", gap_open=13, gap_extend=3)):
        r = new.search_top(packed=q, max_results=5, align=aln)
        assert len(r.alignments) == len(plain.top_pid) > 0 and all(a["status"] == 1 and a["bitscore"] == 0.0 for a in r.alignments)
        assert r.top_pid.tolist() == plain.top_pid.tolist() and r.top_kmatch.tolist() == plain.top_kmatch.tolist()
    with pytest.raises(api.abi.KaamerError) as ei:
        old.search_top(packed=q, max_results=5, align=dict())
    assert ei.value.code == abi.E_ARG
    assert plain.alignments is None
    full = new.search_top(packed=q, max_results=5, align=dict(text=True))
    nums = new.search_top(packed=q, max_results=5, align=dict(text=False))
    assert nums.top_pid.tolist() == full.top_pid.tolist()
    strip = lambda a: {k: v for k, v in a.items() if k != "aln"}
    assert [strip(a) for a in nums.alignments] == [strip(a) for a in full.alignments]
    assert all(a["aln"] is None for a in nums.alignments) and any(a["aln"] for a in full.alignments)
    # gap_extend 2 has a row with gap_open 11: other statistics, the same device integers
    r2 = new.search_top(packed=q, max_results=5, align=dict(gap_open=11, gap_extend=2))
    assert all(a["status"] == 0 for a in r2.alignments)


def test_budget_of_one_slab(klib, gpu_device):
    from kaamer_amd import workload
    prot, old, new = _db(400, 41, gpu_device)
    q = workload.make_protein_queries(workload.make_db(400, seed=41), 60, seed=43)
    ref = new.search_top(packed=q, max_results=5, align=dict())
    waves = new.align_info()["waves"]
    new.set_align_budget(1)
    one = new.search_top(packed=q, max_results=5, align=dict())
    assert new.align_info()["waves"] == 1 < waves
    assert one.top_pid.tolist() == ref.top_pid.tolist() and one.alignments == ref.alignments and len(ref.alignments) > 100
    new.set_align_budget(0)


def _existing_numbers(old, prot, packed, max_results, gpu_device):
    """kaamer_search_batch_top_flat + kaamer_fetch_hits + packing + kaamer_align_pairs -> {(query, id): alignment dict}"""
    from kaamer_amd import api, workload
    top = old.search_top(packed=packed, max_results=max_results)
    qs = workload.unpack(packed)
    keys = sorted(set(top.top_pid.tolist()))
    ent = dict(zip(keys, prot.fetch_hits(keys)))
    seqs, where, pairs, sid = [], [], [], {}
    for i in range(top.n_reported):
        q = int(top.rep_query[i])
        qi = len(seqs)
        seqs.append(qs[q])
        for e in range(int(top.top_off[i]), int(top.top_off[i + 1])):
            p = int(top.top_pid[e])
            if p not in sid:
                sid[p] = len(seqs)
                seqs.append(ent[p]["Sequence"])
            pairs.append((qi, sid[p]))
            where.append((q, p))
    got = api.align_pairs(seqs=seqs, pairs=pairs, number_of_aa=prot.stats()["NumberOfAA"], device=gpu_device)
    return top, dict(zip(where, got))


def _check_against(top_new, top_old, exp):
    assert top_new.rep_query.tolist() == top_old.rep_query.tolist() and top_new.top_off.tolist() == top_old.top_off.tolist()
    for i in range(top_new.n_reported):
        q = int(top_new.rep_query[i])
        a, b = int(top_new.top_off[i]), int(top_new.top_off[i + 1])
        assert sorted(top_new.top_pid[a:b].tolist()) == sorted(top_old.top_pid[a:b].tolist())
        order = {int(p): r for r, p in enumerate(top_old.top_pid[a:b].tolist())}
        keyed = [(-top_new.alignments[e]["bitscore"], order[int(top_new.top_pid[e])]) for e in range(a, b)]
        assert keyed == sorted(keyed), q                       # BitScore descending, ties in sortMapByValue order
        for e in range(a, b):
            g, x = top_new.alignments[e], exp[(q, int(top_new.top_pid[e]))]
            assert g == x, (q, int(top_new.top_pid[e]), g, x)


def test_batch_size_and_concurrency(klib, gpu_device):
    """10 000 protein queries, MaxResults 10, against a 5 000-protein database: two threads and three tickets in flight,
    every result against the existing route on the same batch.  How many pairs that is follows from the data, not from the
    code: the database has families of ten, a fifth of the generated queries are random and report nothing, so a query
    reports between 0 and 10 hits (44 290 pairs in all on this batch).  What guards against a vacuous pass is reasoned, not
    observed: every database member used as a query reports at least itself."""
    from kaamer_amd import api, workload
    dbp = workload.make_db(5000, seed=12)
    recs = workload.unpack(dbp)
    prot = api.Proteins.from_fasta(_fasta(recs).encode())
    img = prot.image(device=gpu_device)
    old, new = api.Index.from_image(img, gpu_device), api.Index.from_image(img, gpu_device)
    new.attach_proteins(prot)
    members = [s for s in recs[:1500] if b"X" not in s]
    q = workload.make_protein_queries(dbp, 10000 - len(members), seed=13)
    packed = api.pack_sequences(members + workload.unpack(q))
    top_old, exp = _existing_numbers(old, prot, packed, 10, gpu_device)
    assert len(exp) >= len(members) > 1000
    aln = dict(text=True)
    results = [None, None]

    def worker(k):
        results[k] = new.search_top(packed=packed, max_results=10, align=aln)
    th = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    tickets = [new.submit_top(packed=packed, max_results=10, align=aln) for _ in range(3)]
    results += [t.wait() for t in tickets]
    for r in results:
        assert r is not None
        _check_against(r, top_old, exp)
    # a database member as query: the self hit has identity 100 and Raw = the sum of its BLOSUM62 diagonal
    r = results[0]
    ids = prot.ids
    diag = lambda s: sum(int(klib.kaamer_align_matrix_entry(c, c)) for c in s.replace(b"U", b"*"))
    rep = {int(qq): i for i, qq in enumerate(r.rep_query.tolist())}
    n_self = 0
    for k, s in enumerate(members):
        if recs.index(s) >= len(recs) - 2:
            continue
        i = rep[k]
        a, b = int(r.top_off[i]), int(r.top_off[i + 1])
        own = [e for e in range(a, b) if recs[int(np.nonzero(ids == r.top_pid[e])[0][-1])] == s]
        assert own, k
        g = r.alignments[own[0]]
        assert g["raw"] == diag(s) and g["identity"] == 100.0 and g["length"] == len(s) and g["gap_openings"] == 0
        assert (g["query_start"], g["query_end"], g["subject_start"], g["subject_end"]) == (1, len(s), 1, len(s))
        n_self += 1
    assert n_self > 1000


def test_device_resident_form(klib, gpu_device):
    """kaamer_topn_align_device's integers equal those inside the host call's block"""
    import torch
    from kaamer_amd import abi, api, workload
    from test_gpu_protein import _from_ptr
    prot, old, new = _db(400, 41, gpu_device)
    packed = workload.make_protein_queries(workload.make_db(400, seed=41), 50, seed=44)
    buf, offs = packed
    host = new.search_top(packed=packed, max_results=5, align=dict(text=False))
    exp = {}
    for i in range(host.n_reported):
        for e in range(int(host.top_off[i]), int(host.top_off[i + 1])):
            exp[(int(host.rep_query[i]), int(host.top_pid[e]))] = host.alignments[e]
    d_buf = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(offs).view(np.int64)).cuda()
    torch.cuda.synchronize()
    st = torch.cuda.Stream().cuda_stream
    n = len(offs) - 1
    longest = int(np.diff(offs.astype(np.int64)).max())
    ws = api.Workspace(new, len(buf), n)
    ws.search_device(d_buf.data_ptr(), d_off.data_ptr(), n, len(buf), stream=st)
    t = ws.topn_device(0.05, 10, 5, stream=st)
    r = ws.topn_align_device(t, max_query_len=longest, stream=st)
    ws.finish(st)
    cnt = _from_ptr(t.d_top_cnt, n, np.uint32)
    pid = _from_ptr(t.d_top_pid, n * 5, np.uint32).reshape(n, 5)
    off = _from_ptr(r.d_pair_off, n + 1, np.uint64)
    assert int(off[n]) == len(exp) <= r.pair_capacity and r.n_waves >= 1 and r.slab_bytes > 0
    raw = _from_ptr(r.d_pairs, int(off[n]) * 64, np.uint8)
    pairs = (abi.AlignPair * int(off[n])).from_buffer_copy(raw.tobytes())
    seen = 0
    for q in range(n):
        assert int(off[q + 1] - off[q]) == int(cnt[q])
        for k in range(int(cnt[q])):
            p, h = pairs[int(off[q]) + k], exp[(q, int(pid[q, k]))]
            assert p.status == h["status"] == 0
            assert (p.n_ops, p.mismatches, p.gap_openings, p.raw) == (h["length"], h["mismatches"], h["gap_openings"], h["raw"])
            assert (p.start_i + 1, p.end_i, p.start_j + 1, p.end_j) == (h["query_start"], h["query_end"], h["subject_start"], h["subject_end"])
            assert np.float32(np.float32(p.identical) / np.float32(p.n_ops)) * np.float32(100) == np.float32(h["identity"])
            assert p.query_len == int(offs[q + 1] - offs[q])
            seen += 1
    assert seen == len(exp) > 100
    # a workspace whose last result is a merge is refused (the queries' residues live with the owner's search) ...
    cur = torch.cuda.current_stream().cuda_stream
    ws_m = api.Workspace(new, 4096, 8, first_pos=1, max_hits=1 << 16)
    ent_off = torch.tensor([0, 1, 2], dtype=torch.int64).cuda()
    m_pid = torch.tensor([5, 9], dtype=torch.int32).cuda()
    m_km = torch.tensor([3, 4], dtype=torch.int32).cuda()
    m_fp = torch.tensor([0, 1], dtype=torch.int32).cuda()
    m_size = torch.tensor([20, 30], dtype=torch.int32).cuda()
    ws_m.merge_device(ent_off.data_ptr(), m_pid.data_ptr(), m_km.data_ptr(), m_fp.data_ptr(), 2, 2, stream=cur)
    t_m = ws_m.topn_device(0.0, 1, 10, d_size_in_kmer_ptr=m_size.data_ptr(), stream=cur)
    ws_m.finish(cur)
    with pytest.raises(abi.KaamerError) as ei:
        ws_m.topn_align_device(t_m, stream=cur)
    assert ei.value.code == abi.E_ARG and "merge" in str(ei.value)
    ws_m.close()
    # ... and so is an index without a table
    ws_old = api.Workspace(old, len(buf), n)
    ws_old.search_device(d_buf.data_ptr(), d_off.data_ptr(), n, len(buf), stream=st)
    t_old = ws_old.topn_device(0.05, 10, 5, stream=st)
    with pytest.raises(abi.KaamerError) as ei:
        ws_old.topn_align_device(t_old, stream=st)
    assert ei.value.code == abi.E_ARG and "attach" in str(ei.value)
    ws_old.finish(st)
    ws_old.close()
    ws.close()
