"""The alignment kernels at the places a random shape meets only by chance: strip boundaries (query rows 64 / 65 / 128 /
129), the LDS row's end (subjects of 2047 / 2048 / 2049 letters, where ta_pair switches to the LONG form), gap runs that
lie across a strip's last row, a 'U' run that touches an 'L' run, and the tie rules (first of diag / up / left; the first
best cell in row-major order).  All three device forms -- align_wave_kernel, align_kernel, ta_wave_kernel<false / true> --
against the restatement of the aligner (oracle/align_oracle.c), every field and every column.

The inputs are built once at import, seeded.  test_edge_inputs_carry_what_they_claim proves on the CPU, with the oracle's
census (ko_align_census), that they hold the geometry and the ties they were built for; the GPU tests run subsets of them."""
import math
from collections import namedtuple

import numpy as np
import pytest

from test_top_align import _fasta, _same

AA = "ACDEFGHIKLMNPQRSTVWY"
N_AA = 2 * 10 ** 8
Pair = namedtuple("Pair", "group name q s")

A_NQ = (1, 2, 63, 64, 65, 127, 128, 129, 192)
A_NS = (1, 2, 63, 64, 65, 2047, 2048, 2049, 2111)
LONG_NS = (2047, 2048, 2049)


def _rand(rng, n, letters=AA):
    return "".join(letters[int(x)] for x in rng.integers(0, len(letters), n))


def _per(unit, n):
    return (unit * (n // len(unit) + 1))[:n]


def _build():
    rng = np.random.default_rng(20260411)
    out = []
    # A. the geometry grid: the query is the subject's tail (a shorter subject: repeated and cut), so that many alignments end
    # in the last cell; and unrelated queries against the subjects around the LDS row's end
    sub_a = {ns: _rand(rng, ns) for ns in A_NS}
    for ns in A_NS:
        for nq in A_NQ:
            s = sub_a[ns]
            out.append(Pair("A", "grid %dx%d" % (nq, ns), s[-nq:] if nq <= ns else _per(s, nq), s))
    for ns in LONG_NS:
        for nq in (64, 65, 129):
            out.append(Pair("A", "unrelated %dx%d" % (nq, ns), _rand(rng, nq), sub_a[ns]))
    # B. one gap run at or across a strip's last row (rows 64 and 128): five inserted letters -> a 'U' run over query rows
    # start+1 .. start+5; five deleted ones -> an 'L' run at row start.  Runs of 1, 2 and 9 deleted letters at the boundary row
    # itself come on top (an 'L' run lies at a row 64k for one start in seven only).  Every pair also with the roles swapped.
    b = []
    for bound in (64, 128):
        for start in range(bound - 5, bound + 2):
            s = _rand(rng, 300)
            b.append(Pair("B", "U run b%d start %d" % (bound, start), s[:start] + "WPWPW" + s[start:], s))
            b.append(Pair("B", "L run b%d start %d" % (bound, start), s[:start] + s[start + 5:], s))
        for cut in (1, 2, 9):
            s = _rand(rng, 300)
            b.append(Pair("B", "L run b%d of %d" % (bound, cut), s[:bound] + s[bound + cut:], s))
    out += b + [Pair("B", p.name + " swapped", p.s, p.q) for p in b]
    # C. a 'U' run that touches an 'L' run: two gap features, two gap openings; the touching point before, on and after a
    # strip's last row.  (s without the inserted letters: no letter of it pairs with one of them and moves a run)
    c = []
    for at in (60, 62, 64):
        s = _rand(rng, 120, "ACDEFHIKLMNQRSTVY")
        c.append(Pair("C", "junction %d" % at, s[:at] + "W" * 10 + s[at:], s[:at] + "GPGPGPGP" + s[at:]))
    out += c + [Pair("C", p.name + " swapped", p.s, p.q) for p in c]
    # D. ties: low-complexity and periodic pairs, and repeats (two copies of one stretch: equal best cells in different rows,
    # 64 rows apart for the 24-letter spacer)
    for nq, ns in ((70, 70), (130, 65), (65, 130), (64, 200), (200, 64)):
        out.append(Pair("D", "A %dx%d" % (nq, ns), "A" * nq, "A" * ns))
        out.append(Pair("D", "AG/GA %dx%d" % (nq, ns), _per("AG", nq), _per("GA", ns)))
        out.append(Pair("D", "ACDA/ACD %dx%d" % (nq, ns), _per("ACDA", nq), _per("ACD", ns)))
        out.append(Pair("D", "AS %dx%d" % (nq, ns), _rand(rng, nq, "AS"), _rand(rng, ns, "AS")))
    u = _rand(rng, 40)
    r50, r24, r88, r30 = (_rand(rng, n) for n in (50, 24, 88, 30))
    out.append(Pair("D", "repeat query", u + r50 + u, u))
    out.append(Pair("D", "repeat subject", u, u + r50 + u))
    out.append(Pair("D", "repeat 64 rows apart", u + r24 + u, u))
    out.append(Pair("D", "repeat both", u + r88 + u, u + r30 + u))
    # a gap whose far end is free: behind the inserted letters the query holds 70 A against the subject's 20, and a gap position
    # beyond the first costs the DP nothing, so opening the gap here (diag + GapOpen) equals extending it (up): the only tie
    # the up / left layers meet on a path.  The tie sits in rows 64-70, both sides of a strip's last row.
    z = _rand(rng, 40, "CDEFHIKLMNQRSTVY")
    out.append(Pair("D", "free gap end up", "A" * 70 + "WWW" + z, "A" * 20 + z))
    out.append(Pair("D", "free gap end left", "A" * 20 + z, "A" * 70 + "WWW" + z))
    # E. letters the tallies and the DP read differently, inside or next to a gap run: U ('*' in the strings), lower case
    # (folded by the DP, a map miss for the marks and a mismatch for the identity) and X
    by = {p.name: p for p in out}
    p = by["U run b64 start 62"]
    out.append(Pair("E", "U inside the U run", p.q.replace("WPWPW", "WPUPW"), p.s))
    p = by["L run b128 start 128"]
    out.append(Pair("E", "lower case under the L run", p.q, p.s[:124] + p.s[124:137].lower() + p.s[137:]))
    p = by["junction 62"]
    out.append(Pair("E", "X next to the touching runs", p.q[:61] + "X" + p.q[62:], p.s[:61] + "X" + p.s[62:]))
    return out


PAIRS = _build()
GROUP = {g: [p for p in PAIRS if p.group == g] for g in "ABCDE"}

_EXPECTED = {}


def _expected(oracle, q, s, n_aa):
    """oracle.align, computed once per (query, subject, NumberOfAA); "bad letter" for its ValueError"""
    key = (q, s, n_aa)
    if key not in _EXPECTED:
        try:
            _EXPECTED[key] = oracle.align(q, s, n_aa)
        except ValueError:
            _EXPECTED[key] = "bad letter"
    return _EXPECTED[key]


def _equals_oracle(g, exp, where):
    """every number and every column of one device alignment against the restatement's"""
    if exp == "bad letter":
        assert g["status"] == 2, where
        return
    assert g["status"] == 0, (where, g["status"])
    for k in ("length", "mismatches", "gap_openings", "raw", "bitscore", "evalue", "identity", "similarity"):
        assert g[k] == exp[k] or (isinstance(exp[k], float) and math.isnan(exp[k]) and math.isnan(g[k])), (where, k, g[k], exp[k])
    for k, ke in (("query_start", "q_start"), ("query_end", "q_end"), ("subject_start", "s_start"), ("subject_end", "s_end")):
        assert g[k] == exp[ke], (where, k, g[k], exp[ke])
    assert g["aln"] == exp["aln"], where


def _all_equal_oracle(cases):
    """_equals_oracle over (name, device alignment, expected): every pair is compared before the first difference is raised,
    so that a failure names all the inputs that expose it"""
    bad = []
    for where, g, exp in cases:
        try:
            _equals_oracle(g, exp, where)
        except AssertionError as e:
            bad.append((where, str(e)[:300]))
    assert not bad, "%d pairs differ from the oracle: %s; the first: %s" % (len(bad), [w for w, _ in bad], bad[0][1])


# ---------------------------------------------------------------- CPU: the inputs
CENSUS_KEYS = ("best_ties_same_row", "best_ties_other_row", "best_ties_row_plus_64k", "path_ties_diag", "path_ties_up", "path_ties_left",
               "gap_runs_adjacent", "gap_runs_crossing")


def test_edge_inputs_carry_what_they_claim(oracle):
    """Conditions on the inputs (oracle and census only, no device): each group holds the geometry or the tie it is there for.
    The totals per class are printed (pytest -s)."""
    assert len(GROUP["A"]) == 81 + 9 and len(GROUP["D"]) == 24 + 2 and len(PAIRS) == len(set(p.name for p in PAIRS))
    cells = sum(len(p.q) * len(p.s) for p in PAIRS)
    print("cells per pass:", cells)     # (the grid 6.5e6, the unrelated queries 1.6e6, B's 68 pairs of 300 x 300 6.2e6)
    assert cells < 1.5 * 10 ** 7, cells
    census = {p.name: oracle.align_census(p.q, p.s) for p in PAIRS}
    for g in "ABCDE":
        print(g, {k: sum(census[p.name][k] for p in GROUP[g]) for k in CENSUS_KEYS})
    # A: alignments that end in the last cell, in a strip's first and last row, and beyond column 2040 of the long subjects
    grid = [p for p in GROUP["A"] if p.name.startswith("grid")]
    ends = {p.name: _expected(oracle, p.q, p.s, N_AA) for p in grid}
    in_last_cell = sum((e["q_end"], e["s_end"]) == (len(p.q), len(p.s)) for p, e in ((p, ends[p.name]) for p in grid))
    print("A: pairs ending in (nq, ns):", in_last_cell)
    assert in_last_cell >= 30
    lanes = set((e["q_end"] - 1) % 64 for e in ends.values() if e["length"])
    assert 63 in lanes and 0 in lanes
    for ns in LONG_NS:
        assert any(len(p.s) == ns and ends[p.name]["s_end"] > 2040 for p in grid), ns
    # B: one gap each; 'U' runs across and 'L' runs at rows 64 and 128
    crossing = {}
    for p in GROUP["B"]:
        assert _expected(oracle, p.q, p.s, N_AA)["gap_openings"] == 1, p.name
        for kind_row in census[p.name]["crossings"]:
            crossing[kind_row] = crossing.get(kind_row, 0) + 1
    print("B: runs at strip boundaries:", sorted(crossing.items()))
    for row in (64, 128):
        assert crossing.get(("U", row), 0) >= 4 and crossing.get(("L", row), 0) >= 4, (row, crossing)
    # C: the two runs touch
    for p in GROUP["C"]:
        assert census[p.name]["gap_runs_adjacent"] >= 1 and _expected(oracle, p.q, p.s, N_AA)["gap_openings"] == 2, p.name
    assert set(k for p in GROUP["C"] for k, _ in census[p.name]["crossings"]) == {"U", "L"}
    # D: every class of tie occurs
    for k in CENSUS_KEYS[:6]:
        assert sum(census[p.name][k] for p in GROUP["D"]) > 0, k
    # E: the letter sits in the alignment, next to or inside a gap
    for p, letter in zip(GROUP["E"], ("*", "a-z", "X")):
        e = _expected(oracle, p.q, p.s, N_AA)
        assert e["gap_openings"] >= 1, p.name
        rows = e["aln"][0] + e["aln"][2]
        assert any(c.islower() for c in rows) if letter == "a-z" else letter in rows, p.name


# ---------------------------------------------------------------- GPU: kaamer_align_pairs
@pytest.mark.gpu
@pytest.mark.parametrize("setting", ("default", "lane kernel", "launch per long pair"))
def test_align_pairs_equal_the_restatement(klib, oracle, gpu_device, monkeypatch, setting):
    """every pair of A-E through kaamer_align_pairs.  default: align_wave_kernel up to 2048 letters, align_kernel for 2049 and
    2111; lane kernel: align_kernel for everything (KAAMER_ALIGN_WAVE_NS=0; without the 192-row queries against the long
    subjects: a wave of 64 lanes pads to its largest pair, and align_kernel beyond 2048 letters is in the default run); launch
    per long pair: a direction budget below one 64 x 2047 pair (1 x 2110 x 64 bytes), so each such pair is a launch."""
    from kaamer_amd import api
    env = {"default": {}, "lane kernel": {"KAAMER_ALIGN_WAVE_NS": "0"}, "launch per long pair": {"KAAMER_ALIGN_DIR_BYTES": "100000"}}[setting]
    for k in ("KAAMER_ALIGN_WAVE_NS", "KAAMER_ALIGN_DIR_BYTES"):
        if k in env:
            monkeypatch.setenv(k, env[k])
        else:
            monkeypatch.delenv(k, raising=False)
    todo = [p for p in PAIRS if not (setting == "lane kernel" and len(p.q) == 192 and len(p.s) >= 2047)]
    assert len(todo) == len(PAIRS) - (4 if setting == "lane kernel" else 0)
    seqs, at, pairs = [], {}, []
    for p in todo:
        for x in (p.q, p.s):
            if x not in at:
                at[x] = len(seqs)
                seqs.append(x.encode())
        pairs.append((at[p.q], at[p.s]))
    got = api.align_pairs(seqs=seqs, pairs=pairs, number_of_aa=N_AA, device=gpu_device)
    assert len(got) == len(todo)
    assert not [p.name for p, g in zip(todo, got) if g["status"] == 3]
    _all_equal_oracle((p.name, g, _expected(oracle, p.q, p.s, N_AA)) for p, g in zip(todo, got))


# ---------------------------------------------------------------- GPU: the top-N call
def _table(records, padding):
    """-> (Proteins, {sequence: protein id}); the padding goes last (the FASTA reader's last two records share an id)"""
    from kaamer_amd import api
    prot = api.Proteins.from_fasta(_fasta(list(records) + list(padding)).encode())
    ids = prot.ids.tolist()
    assert len(ids) == len(records) + len(padding) and len(set(ids[:len(records)])) == len(records)
    return prot, {s: ids[i] for i, s in enumerate(records)}


def _unique(xs):
    return list(dict.fromkeys(xs))


def _shares_a_7mer(q, s):
    k = set(s[i:i + 7] for i in range(len(s) - 6))
    return any(q[i:i + 7] in k for i in range(len(q) - 6))


def _reported(top, queries):
    """{(query, protein id): alignment} of a TopResult, hits in BitScore order checked on the way"""
    out = {}
    for i in range(top.n_reported):
        a, b = int(top.top_off[i]), int(top.top_off[i + 1])
        bits = [top.alignments[e]["bitscore"] for e in range(a, b)]
        assert bits == sorted(bits, reverse=True)
        for e in range(a, b):
            out[(queries[int(top.rep_query[i])], int(top.top_pid[e]))] = top.alignments[e]
    return out


def _same_hits(got, ref):
    assert got.rep_query.tolist() == ref.rep_query.tolist() and got.top_off.tolist() == ref.top_off.tolist()
    assert got.top_pid.tolist() == ref.top_pid.tolist()
    assert len(got.alignments) == len(ref.alignments)
    for e, (g, x) in enumerate(zip(got.alignments, ref.alignments)):
        assert _same(g, x), (e, g, x)


SEARCH = dict(min_k_match=1, min_k_ratio=1e-9, max_results=5, align=dict(text=True))


@pytest.fixture(scope="module")
def edge_db(klib, oracle, gpu_device):
    """the table of the subjects of A (63 letters and more), B, C and D's repeats plus 40 generated records, its index with the
    table attached, the matching queries, and the one-call result every test below starts from (computed once)"""
    from kaamer_amd import api, workload
    mine = [p for p in GROUP["A"] + GROUP["B"] + GROUP["C"] if len(p.s) >= 63] + [p for p in GROUP["D"] if p.name.startswith("repeat")]
    records = _unique(p.s for p in mine)
    padding = [s.decode() for s in workload.unpack(workload.make_db(40, seed=23))]
    prot, pid_of = _table(records, padding)
    ix = api.Index.from_image(prot.image(device=gpu_device), gpu_device)
    ix.attach_proteins(prot)
    queries = _unique(p.q for p in mine if len(p.q) >= 7)
    top = ix.search_top(queries, **SEARCH)
    info = ix.align_info()
    return dict(prot=prot, pid_of=pid_of, ix=ix, mine=mine, queries=queries, top=top, info=info, n_aa=prot.stats()["NumberOfAA"],
                padding=padding)


@pytest.mark.gpu
def test_top_call_equals_the_restatement(edge_db, oracle):
    """ta_wave_kernel<false> and <true> (the tallies stepped in reverse on the device) against the oracle: every reported
    (query, hit) pair, whichever hits the search chose; every intended pair was among them"""
    prot, top, info = edge_db["prot"], edge_db["top"], edge_db["info"]
    print(info)
    assert info["max_subject_len"] == 2111 and info["waves"] >= 1 and info["long_waves"] >= 1
    hits = _reported(top, edge_db["queries"])
    assert not [k for k, a in hits.items() if a["status"] == 3]
    subject = {pid: prot.fetch_hits([pid])[0]["Sequence"].decode("latin-1") for pid in set(pid for _, pid in hits)}
    name = {(p.q, edge_db["pid_of"][p.s]): p.name for p in edge_db["mine"]}
    _all_equal_oracle((name.get((q, pid), "%d letters against id %d" % (len(q), pid)), a, _expected(oracle, q, subject[pid], edge_db["n_aa"]))
                      for (q, pid), a in hits.items())
    wanted = [p for p in edge_db["mine"] if p.group in "ABC" and _shares_a_7mer(p.q, p.s)]
    print("reported pairs %d, intended pairs %d" % (len(hits), len(wanted)))
    assert len(wanted) > 100
    for p in wanted:
        assert (p.q, edge_db["pid_of"][p.s]) in hits, p.name
        assert subject[edge_db["pid_of"][p.s]] == p.s


@pytest.mark.gpu
def test_top_call_switches_forms_at_2048(edge_db, gpu_device):
    """subjects of 2047 and 2048 letters are ta_wave_kernel<false>'s, 2049 is <true>'s: a pair waits with a status only its
    own kernel takes up (ta_pair), so a finished pair names the kernel.  With the table's subjects beyond 2048 letters taken
    out no long wave is launched, and the 2047- and 2048-letter pairs come back unchanged."""
    from kaamer_amd import api
    prot, pid_of, hits = edge_db["prot"], edge_db["pid_of"], _reported(edge_db["top"], edge_db["queries"])
    grid = {ns: [p for p in GROUP["A"] if p.name.startswith("grid") and len(p.s) == ns and len(p.q) >= 7] for ns in LONG_NS}
    for ns in LONG_NS:
        assert len(grid[ns]) == 7
        for p in grid[ns]:
            assert len(prot.fetch_hits([pid_of[p.s]])[0]["Sequence"]) == ns       # subject_len of the pair's record
            assert hits[(p.q, pid_of[p.s])]["status"] == 0 and hits[(p.q, pid_of[p.s])]["subject_end"] == ns
    assert edge_db["info"]["long_waves"] >= 1                                     # 2049: finished, and <true> was launched
    short = _unique(p.s for p in edge_db["mine"] if len(p.s) <= 2048)
    prot2, pid2 = _table(short, edge_db["padding"])
    ix2 = api.Index.from_image(prot2.image(device=gpu_device), gpu_device)
    ix2.attach_proteins(prot2)
    queries = [p.q for ns in (2047, 2048) for p in grid[ns]]
    top2 = ix2.search_top(queries, **SEARCH)
    info2 = ix2.align_info()
    assert info2["max_subject_len"] == 2048 and info2["long_waves"] == 0 and info2["waves"] >= 1
    # the batch's longest query (192 rows) against the 2048-letter subject: the slab ta_stage sizes holds exactly this pair
    assert info2["slab_bytes"] == 3 * (2048 + 63) * 64
    hits2 = _reported(top2, queries)
    strip = lambda a: {k: v for k, v in a.items() if k != "evalue"}               # (NumberOfAA differs between the tables)
    for ns in (2047, 2048):
        for p in grid[ns]:
            assert _same(strip(hits2[(p.q, pid2[p.s])]), strip(hits[(p.q, pid_of[p.s])])), p.name
    ix2.close()


@pytest.mark.gpu
def test_top_call_slabs(edge_db):
    """one slab for the whole batch (one persistent wave takes the large pairs and the small ones in turn, in the same slab),
    and the geometry grid's queries alone (the longest query of the batch, 192 rows, is then the one against the 2048-letter
    subject: the pair that fills ta_stage's slab to the byte): the same alignments, nothing with status 3"""
    ix, top, queries = edge_db["ix"], edge_db["top"], edge_db["queries"]
    ix.set_align_budget(1)
    try:
        one = ix.search_top(queries, **SEARCH)
        assert ix.align_info()["waves"] == 1
    finally:
        ix.set_align_budget(0)
    _same_hits(one, top)
    assert not any(a["status"] == 3 for a in one.alignments) and len(one.alignments) > 100
    grid_q = _unique(p.q for p in GROUP["A"] if len(p.s) >= 63 and len(p.q) >= 7)
    assert max(len(q) for q in grid_q) == 192
    alone = ix.search_top(grid_q, **SEARCH)
    assert ix.align_info()["slab_bytes"] == 3 * (2048 + 63) * 64
    ref, got = _reported(top, queries), _reported(alone, grid_q)
    assert got and not any(a["status"] == 3 for a in got.values())
    for k, a in got.items():
        assert _same(a, ref[k]), k[1]


@pytest.mark.gpu
def test_top_call_sharded_w2(klib, gpu_device):
    """the 2049- and 2111-letter subjects in different partitions (ids 0 and 1 of a table split by id mod 2) and the B pairs:
    a query's owner aligns it with subjects gathered from either partition, in slabs sized for the whole table's longest
    subject.  Hit for hit what the unsharded call returns on the same table."""
    from kaamer_amd import api, workload
    from test_sharded_top_align import _same_top, _sharded
    long_p = [p for p in GROUP["A"] if p.name.startswith("grid") and len(p.s) in (2049, 2111) and len(p.q) >= 7]
    records = _unique([p.s for p in long_p] + [p.s for p in GROUP["B"]])
    prot, pid_of = _table(records, [s.decode() for s in workload.unpack(workload.make_db(40, seed=23))])
    assert sorted(pid_of[s] % 2 for s in records[:2]) == [0, 1] and sorted(len(s) for s in records[:2]) == [2049, 2111]
    ix = api.Index.from_image(prot.image(device=gpu_device), gpu_device)
    ix.attach_proteins(prot)
    queries = _unique([p.q for p in long_p] + [p.q for p in GROUP["B"]])
    ref = ix.search_top(queries, **SEARCH)
    sx = _sharded(api, prot, gpu_device, 2)
    top = sx.search_top(queries, **SEARCH)
    _same_top(top, ref)
    assert sx.align_info()["max_subject_len"] == 2111 and sx.align_stage_info()["long_waves"] >= 1
    hits = _reported(top, queries)
    assert not any(a["status"] != 0 for a in hits.values())
    for p in long_p + GROUP["B"]:
        assert (p.q, pid_of[p.s]) in hits, p.name
    sx.close()
    ix.close()


# ---------------------------------------------------------------- GPU: reads
def _as_read(protein):
    """a protein as the nucleotides of one read, first codon of each residue (NCBI table 11)"""
    from kaamer_amd import workload
    aa = np.frombuffer(protein.encode(), dtype=np.uint8)
    return bytes(workload._CODONS[aa, 0].reshape(-1)).upper()


@pytest.mark.gpu
def test_reads_form(edge_db, oracle):
    """two of B's queries as nucleotide reads: the aligned query is the ORF after SetBestStartCodon's trim"""
    from kaamer_amd import abi
    ix, prot = edge_db["ix"], edge_db["prot"]
    by = {p.name: p for p in GROUP["B"]}
    chosen = [by["U run b64 start 62"], by["L run b128 start 128"]]
    reads = [_as_read(p.q) for p in chosen]
    kw = dict(seq_type=abi.READS, min_k_match=1, min_k_ratio=1e-9, max_results=5)
    top = ix.search_top(reads, align=dict(text=True), **kw)
    full = ix.search(reads, seq_type=abi.READS)
    found = set()
    for i in range(top.n_reported):
        q, t = int(top.rep_query[i]), int(top.trim[i])
        m = full.meta[q]
        assert int(top.meta["aa_len"][i]) == int(m["aa_len"]) - t                 # the aligned query: aa_len - trim residues
        orf = bytes(top.orf_aa[int(top.meta["aa_off"][i]):int(top.meta["aa_off"][i]) + int(top.meta["aa_len"][i])]).decode("latin-1")
        whole = bytes(full.orf_aa[int(m["aa_off"]):int(m["aa_off"]) + int(m["aa_len"])]).decode("latin-1")
        assert orf == whole[t:]
        for e in range(int(top.top_off[i]), int(top.top_off[i + 1])):
            pid = int(top.top_pid[e])
            subject = prot.fetch_hits([pid])[0]["Sequence"].decode("latin-1")
            a = top.alignments[e]
            _equals_oracle(a, _expected(oracle, orf, subject, edge_db["n_aa"]), (q, pid))
            for p in chosen:
                if pid == edge_db["pid_of"][p.s] and p.q[t:] in orf and a["gap_openings"] == 1:
                    found.add(p.name)
    assert found == set(p.name for p in chosen)
