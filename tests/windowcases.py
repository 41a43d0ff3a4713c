"""The window steps of the LDS counting kernels (kaamer_amd/csrc/count_window.hip.inc, inlined by count_group_kernel and
count_pack_kernel), pinned by input: one small database with postings lists of chosen lengths, queries composed so that a
window of 64 flat positions carries an exact number of further ids, and a restatement of the flat layout that proves it.

  a  where an id of a list comes from: inline, a list of one (an id of 2^31 or more), ids 1 and 2 in the 16-byte head,
     id 3 the first arena load, ids 4 and 5 across the next unit
  b  xtotal, the further ids of a window: around XIT * 64 = 128 and around every end of a round of GRP_LONG_UNROLL chunks
  c  owner marks: a first item at 127 (max-scan) and at 128 (binary search); all further ids in lane 0 or lane 63
  d  a list against its table: 63, 64, 65 ids in 64 slots, 65, 128, 129 in 128, 4096 and 4097 in 4096
  e  queries of more windows than carry a start hint
  f  runs of equal ids over a change of query; runs that cross the words of a PositionHits bitmap
  g  the ORF forms of a-d (orf_cases)

window_extras is used only to prove that a case meets its target (tests/test_window_cases_host.py); no kernel output is
compared with it.  Test infrastructure; every constant is read from the source (gtierref.py names the lines)."""
import numpy as np

import gtierref
import tableref
from gtierref import ALPHA, GRP_MAX_PROBES, table_slots_for

CORE = 200                  # residues of a family's core: 194 k-mers
FAMILIES = {"1": 1, "1hi": 1, "2": 2, "3": 3, "4": 4, "5": 5, "6": 6, "9": 9, "63": 63, "64": 64, "65": 65, "128": 128, "129": 129}
HEADS = ("1", "1hi", "2", "3", "4", "5", "6", "9")
LONE = (129, 130, 385, 386)  # S_n: n proteins behind ONE k-mer
BIG = (4096, 4097)           # families that share a 13-residue core
HI_ID = 0x80000005           # the id of F_1hi: no inline value can hold it
XTOTALS = (0, 1, 63, 64, 65, 127, 128, 129, 383, 384, 385, 639, 640, 641)
SHIFTS = (7, 20, 57, 58, 64)

# the codon table of tests/test_gpu_window_tail.py
CODON = dict(zip(b"ACDEFGHIKLMNPQRSTVWY", (b"GCT", b"TGT", b"GAT", b"GAA", b"TTT", b"GGT", b"CAT", b"ATT", b"AAA", b"CTG", b"ATG",
                                          b"AAT", b"CCT", b"CAA", b"CGT", b"TCT", b"ACT", b"GTT", b"TGG", b"TAT")))
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def nt(aa):
    return b"".join(CODON[a] for a in aa)


def rc(dna):
    return dna.translate(_COMP)[::-1]


# ---- the table of a query --------------------------------------------------------------------------------------------
def table_home(ids, cap):
    """count_window.hip.inc table_home: (uint32(id * 0x9E3779B1) * cap) >> 32"""
    ids = np.asarray(ids).astype(np.uint64)
    return ((((ids * np.uint64(gtierref.TABLE_MUL)) & np.uint64(0xFFFFFFFF)) * np.uint64(cap)) >> np.uint64(32)).astype(np.int64)


def longest_run(ids, cap):
    """The longest run of occupied slots of a table of `cap` slots that holds the distinct `ids` (gtierref.lds_longest_run's
    argument: with linear probing the set of occupied slots does not depend on the order of the insertions, and no id walks
    more slots than the longest run).  Below GRP_MAX_PROBES, table_probe's cut-off cannot fire."""
    ids = np.unique(np.asarray(ids, dtype=np.uint32))
    assert len(ids) <= cap
    arrive = np.bincount(table_home(ids, cap), minlength=cap).tolist()
    occ = [False] * cap
    carry = 0
    for rnd in range(2):           # the second round takes what the first one carried past the last slot
        for i in range(cap):
            have = carry + (arrive[i] if rnd == 0 else 0)
            if have and not occ[i]:
                occ[i] = True
                have -= 1
            carry = have
    best = run = 0
    for i in range(2 * cap):
        run = run + 1 if occ[i % cap] else 0
        best = max(best, run)
    return min(best, cap)


# ---- the database ----------------------------------------------------------------------------------------------------
class Database:
    """F_L: L proteins around one random core of CORE residues (private flanks of 20): every k-mer of the core has a list of
    exactly L ids.  S_n: n random proteins of 60 residues that contain one fixed 7-mer.  Two families of 4096 and 4097
    proteins of 21 residues around a 13-residue core.  200 random proteins.  Ids are explicit and scattered; F_1hi's is HI_ID."""

    def __init__(self, oracle, seed):
        rng = np.random.default_rng(seed)
        rnd = lambda n: bytes(ALPHA[rng.integers(0, 20, int(n))])   # noqa: E731
        # the residue on either side of a shared k-mer or 13-residue core is one of the first ten letters: a query that
        # puts one of the last ten there (high) shares no k-mer with those proteins but the planted ones -- with random
        # neighbours a twentieth of the n proteins would share the k-mer one position on
        low = lambda: bytes(ALPHA[rng.integers(0, 10, 1)])          # noqa: E731
        self.oracle, self.core, self.kmer, self.big = oracle, {}, {}, {}
        db, hi_at = [], None
        for name, n in FAMILIES.items():
            self.core[name] = rnd(CORE)
            if name == "1hi":
                hi_at = len(db)
            db += [rnd(20) + self.core[name] + rnd(20) for _ in range(n)]
        for n in LONE:
            self.kmer[n] = rnd(7)
            for _ in range(n):
                p, at = bytearray(rnd(60)), int(rng.integers(1, 53))
                p[at - 1:at + 8] = low() + self.kmer[n] + low()
                db.append(bytes(p))
        for n in BIG:
            self.big[n] = rnd(13)
            db += [rnd(3) + low() + self.big[n] + low() + rnd(3) for _ in range(n)]
        self.background = [rnd(100) for _ in range(200)]
        db += self.background
        ids = rng.permutation(len(db)).astype(np.uint32) * np.uint32(3) + np.uint32(1)
        ids[hi_at] = HI_ID
        self.db, self.ids = db, ids
        self.oix = oracle.Index.from_proteins(db, ids=ids)
        self.pairs = np.sort(self.oix.pairs())

    def counts(self, seq):
        """the length of the postings list of every k-mer position of seq"""
        seq = bytes(seq)
        size = max(self.oracle.size_in_kmer(seq), 0)
        keys = tableref.encode_windows(seq, np.arange(size)).astype(np.uint64)
        lo = np.searchsorted(self.pairs, keys << np.uint64(32))
        hi = np.searchsorted(self.pairs, (keys + np.uint64(1)) << np.uint64(32))
        return (hi - lo).astype(np.int64)

    def figures(self, seq):
        return gtierref.Figures(self.oracle, self.oix, seq, pairs=self.pairs)

    def exact(self):
        """every list has the length its family says, F_1hi's single id is the high one"""
        ok = all((self.counts(c) == FAMILIES[f]).all() for f, c in self.core.items())
        ok = ok and all(int(self.counts(k + b"AAAAAA")[0]) == n for n, k in self.kmer.items())
        ok = ok and all((self.counts(c) == n).all() for n, c in self.big.items())
        return ok and (self.figures(self.core["1hi"]).ids == HI_ID).all() and (self.figures(self.core["1"]).ids < gtierref.INLINE_BIT).all()


_db = {}


def database(oracle):
    """the database, built once: the first seed whose random cores and k-mers collide with nothing else"""
    if "db" not in _db:
        for seed in range(20261021, 20261041):
            d = Database(oracle, seed)
            if d.exact():
                _db["db"] = d
                break
        else:
            raise AssertionError("no seed gives exact list lengths")
    return _db["db"]


def compose(d, parts, rng):
    """parts: [(family, n_positions) | ("random", n_positions)] -> (query, first k-mer position of every part).  Every part
    is a slice of n_positions + 6 residues (of its family's core, or random): n_positions k-mers with the family's list
    length, then the six k-mers across the junction to the next part, which must have empty lists -- drawn again if not."""
    for _ in range(200):
        pieces, at, p = [], [], 0
        for fam, n in parts:
            if fam == "random":
                pieces.append(bytes(ALPHA[rng.integers(0, 20, n + 6)]))
            else:
                a = int(rng.integers(0, CORE - (n + 6) + 1))
                pieces.append(d.core[fam][a:a + n + 6])
            at.append(p)
            p += n + 6
        seq = b"".join(pieces)
        cnt = d.counts(seq)
        assert len(cnt) == p - 6
        ok = True
        for i, (fam, n) in enumerate(parts):
            ok = ok and bool((cnt[at[i]:at[i] + n] == (0 if fam == "random" else FAMILIES[fam])).all())
            ok = ok and (i + 1 == len(parts) or bool((cnt[at[i] + n:at[i] + n + 6] == 0).all()))
        if ok:
            return seq, at
    raise AssertionError("no draw of %r with empty junctions" % (parts,))


# ---- the flat layout -------------------------------------------------------------------------------------------------
class Window:
    """one window of 64 flat positions: per lane the query (index among the unit's queries, -1: idle), the position in it,
    the list length, the further ids and their exclusive prefix; xtotal, their sum"""

    def __init__(self, q, pos, cnt):
        self.q, self.pos, self.cnt = q, pos, cnt
        self.extra = np.maximum(cnt - 1, 0)
        self.pref = np.cumsum(self.extra) - self.extra
        self.xtotal = int(self.extra.sum())


def searched_queries(d, seqs, nucleotide):
    """the queries of a batch: the sequences, or the ORFs of every read in oracle.get_orfs order"""
    if not nucleotide:
        return [bytes(s) for s in seqs]
    return [o["seq"].encode("latin-1") for r in seqs for o in d.oracle.get_orfs(r)]


def window_extras(d, seqs, nucleotide=False, shift=None, single=True):
    """The flat layout of a batch: the tables of the searched queries (SizeInKmer >= 7) lie one after the other, a unit (a
    group of count_group_kernel, a pack of count_pack_kernel) is the run of queries whose table STARTS in one window of
    1 << shift slots, and the k-mer positions of a unit's queries, concatenated in query order, are cut into windows of 64.
    -> the windows of the batch's only unit; single=False: a list of units, each a list of windows.
    shift: GRP_SHIFT + 1 for proteins (GRP_SHIFT for the PositionHits pass), PACK_SHIFT_NUCLEOTIDE for ORFs.
    single: every table starts in the first slot window -- sum(slots) <= 1 << shift is enough for that, a last table may
    hang over -- and, for proteins, the unit fits the arena (GRP_FIT slots), or the kernel counts it in two parts.
    An ORF whose table is larger than the wave's arena allows takes its slots of the layout but is sent on uncounted."""
    if shift is None:
        shift = gtierref.PACK_SHIFT_NUCLEOTIDE if nucleotide else gtierref.GRP_SHIFT + 1
    long_orfs = nucleotide and sum(len(s) for s in seqs) > 200 * len(seqs)
    units, start = {}, 0
    for q in searched_queries(d, seqs, nucleotide):
        size = d.oracle.size_in_kmer(q)
        if size < 7:
            continue
        u = units.setdefault(start >> shift, dict(q=[], slots=0))
        if not (nucleotide and gtierref.pack_sends_unseen(size, long_orfs)):
            u["q"].append(q)
        u["slots"] = start + table_slots_for(size) - ((start >> shift) << shift)
        start += table_slots_for(size)
    if single:
        assert len(units) <= 1, "tables start in %d slot windows" % len(units)
        assert nucleotide or all(u["slots"] <= gtierref.GRP_FIT for u in units.values())
    out = []
    for _, u in sorted(units.items()):
        cnts = [d.counts(q) for q in u["q"]]
        n = sum(len(c) for c in cnts)
        pad = -n % 64
        cnt = np.concatenate(cnts + [np.zeros(pad, np.int64)]) if cnts else np.zeros(0, np.int64)
        qi = np.concatenate([np.full(len(c), i) for i, c in enumerate(cnts)] + [np.full(pad, -1)]) if cnts else np.zeros(0, np.int64)
        ps = np.concatenate([np.arange(len(c)) for c in cnts] + [np.zeros(pad, np.int64)]) if cnts else np.zeros(0, np.int64)
        out.append([Window(qi[a:a + 64], ps[a:a + 64], cnt[a:a + 64]) for a in range(0, n + pad, 64)])
    if single:
        return out[0] if out else []
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------
class Case:
    """seqs: the batch.  claims: the targets it says it meets (check_claim).  overflow: the n_overflow the code makes exact
    (0: every table stays in LDS; 1: one query must leave; None: the 96-probe cut-off may or may not fire)."""

    def __init__(self, kind, name, seqs, claims, overflow=0, nucleotide=False, redraw=None):
        self.kind, self.name, self.seqs, self.claims, self.overflow, self.nucleotide = kind, name, list(seqs), list(claims), overflow, nucleotide
        self.redraw = redraw       # rng -> another draw of a single query with the same claims

    def __repr__(self):
        return "%s/%s" % (self.kind, self.name)


def check_claim(d, case, claim, anywhere=False):
    """True if the batch of `case` meets `claim`.  anywhere: in any window of any unit (the ORF forms, whose ORF of
    interest follows the read's other ORFs); else in the window the claim's position says."""
    what = claim[0]
    queries = [q for q in searched_queries(d, case.seqs, case.nucleotide) if d.oracle.size_in_kmer(q) >= 7]
    if what in ("xtotal", "owner", "lone"):
        units = window_extras(d, case.seqs, case.nucleotide, single=False) if anywhere else [window_extras(d, case.seqs, case.nucleotide)]
        wins = [w for u in units for w in u]
        if what == "xtotal":       # (X): the further ids of window 0
            return any(w.xtotal == claim[1] for w in (wins if anywhere else wins[:1]))
        if what == "owner":        # (P): a lane with further ids whose first item is item P
            return any(bool(((w.extra > 0) & (w.pref == claim[1])).any()) for w in (wins if anywhere else wins[:1]))
        pos, n = claim[1:]         # lone (position, n): all n - 1 further ids of the window in the lane of that position
        pick = wins if anywhere else wins[pos // 64:pos // 64 + 1]
        return any(int(w.extra[pos % 64]) == n - 1 == w.xtotal for w in pick)
    if what == "head":             # (family, form): the k-mers of the core slice all meet a list of the family's length
        fam, form = claim[1:]
        L = FAMILIES[fam]
        for q in queries:
            f = d.figures(q)
            hit = f.cnt[f.cnt > 0]
            if len(hit) == 0 or not (hit == L).all() or bool(f.listed[f.cnt > 0].all()) != (fam != "1"):
                continue
            if fam == "1hi" and not (f.ids == HI_ID).all():
                continue
            if form == "mutated" and 0 < len(hit) < f.size and f.size >= CORE - 6:
                return True
            if form == "whole" and len(hit) == CORE - 6 and (anywhere or f.size == CORE - 6):
                return True
            # the first n positions; an ORF form may carry hit-free positions before them
            if form in ("64", "65") and len(hit) == int(form) and (anywhere or f.size == int(form)) and bool((f.cnt[-int(form):] == L).all()):
                return True
        return False
    if what == "fill":             # (ids, slots): a query with exactly `ids` distinct hits in a table of `slots` slots
        return any(table_slots_for(d.oracle.size_in_kmer(q)) == claim[2] and d.figures(q).D == claim[1] for q in queries)
    if what == "hint":             # (n_hint): lists on both sides of the last window with a start hint, in one unit
        wins = window_extras(d, case.seqs)
        n_hint = claim[1]
        return len(wins) > n_hint + 1 and wins[n_hint - 1].xtotal > 0 and wins[n_hint].xtotal > 0 and (len(queries) == 1 or wins[n_hint].q[0] > 0)
    if what == "runs":
        if claim[1] == "query":    # the same id in adjacent lanes of different queries
            w = window_extras(d, case.seqs)[0]
            ids = [d.figures(q).ids[0] for q in queries]
            return len(set(ids)) == 1 and bool((np.diff(w.q[w.q >= 0]) != 0).any()) and bool((w.cnt[w.q >= 0] > 0).all())
        s = claim[1]               # the second query's runs start at flat position s: bit (64 - s) % 64 of its bitmaps
        for shift in (gtierref.GRP_SHIFT, gtierref.GRP_SHIFT + 1):
            wins = window_extras(d, case.seqs, shift=shift)
            flat = np.concatenate([w.q for w in wins])
            if int(np.flatnonzero(flat == 1)[0]) != s or not (d.counts(queries[1]) == 3).all():
                return False
        return True
    raise KeyError(what)


def _stays_in_lds(d, case):
    """0 for n_overflow is exact when no table add can run out of probes: the longest occupied run of every table is below
    GRP_MAX_PROBES (and no list is longer than its table)"""
    long_orfs = case.nucleotide and sum(len(s) for s in case.seqs) > 200 * len(case.seqs)
    for q in searched_queries(d, case.seqs, case.nucleotide):
        size = d.oracle.size_in_kmer(q)
        if size < 7:
            continue
        f, cap = d.figures(q), table_slots_for(size)
        if case.nucleotide and gtierref.pack_sends_unseen(size, long_orfs):
            return False
        if f.D > cap or (f.cnt > cap).any() or size >= gtierref.LDS_MAX_SIZE or longest_run(f.distinct, cap) >= GRP_MAX_PROBES:
            return False
    return True


def _rnd(rng, n):
    return bytes(ALPHA[rng.integers(0, 20, int(n))])


def _high(rng):
    """one of the last ten letters: never next to a shared k-mer in the database (Database)"""
    return bytes(ALPHA[rng.integers(10, 20, 1)])


def hitless(d, rng, n):
    """n random residues none of whose k-mers is in the database"""
    for _ in range(200):
        s = _rnd(rng, n)
        if not d.counts(s).any():
            return s
    raise AssertionError("no hit-free draw of %d residues" % n)


def _mutated(core):
    m = bytearray(core)
    for i in range(15, len(core), 30):   # a substitution every 30 residues: empty lists inside the windows
        m[i] = ALPHA[(ALPHA.tolist().index(m[i]) + 1) % 20]
    return bytes(m)


def _xtotal_parts(x):
    """parts whose window 0 carries x further ids (all lists within the first 64 positions)"""
    return {0: [("1", 64)], 1: [("2", 1), ("random", 40)], 63: [("2", 63), ("random", 20)], 64: [("2", 64)],
            65: [("3", 32), ("2", 1), ("random", 10)], 127: [("4", 42), ("2", 1), ("random", 30)], 128: [("3", 64)], 129: [("4", 43)],
            383: [("9", 47), ("6", 1), ("3", 1)], 384: [("9", 48)], 385: [("9", 48), ("2", 1)],
            # (64 lanes of F_9 carry 512 at most: the values from 639 up take F_64 and F_65, and positions enough that their
            # table has room for the 70 or so distinct hits)
            639: [("64", 10), ("9", 1), ("2", 1), ("random", 130)], 640: [("65", 10), ("random", 150)],
            641: [("65", 10), ("2", 1), ("random", 140)]}[x]


def _lone(d, rng, n, pos, length):
    """a hit-free query of `length` residues with S_n's k-mer planted at k-mer position pos"""
    for _ in range(200):
        q = bytearray(_rnd(rng, length))
        q[pos:pos + 8] = d.kmer[n] + _high(rng)
        if pos:
            q[pos - 1:pos] = _high(rng)
        cnt = d.counts(bytes(q))
        if cnt[pos] == n and int(cnt.sum()) == n:
            return bytes(q)
    raise AssertionError("no draw")


def _fill_query(d, rng, core13, kmers):
    """7 k-mers of a core, then hit-free random residues up to `kmers` k-mers"""
    for _ in range(400):
        q = core13 + (_high(rng) + _rnd(rng, kmers - 8) if kmers > 7 else b"")
        cnt = d.counts(q)
        if len(cnt) == kmers and not cnt[7:].any():
            return q
    raise AssertionError("no draw")


_cases = {}


def cases(oracle):
    """the protein cases a-f, built once"""
    if "protein" in _cases:
        return _cases["protein"]
    d = database(oracle)
    rng = np.random.default_rng(616)
    out = []
    for fam in HEADS:                                                    # ---- a
        c = d.core[fam]
        out.append(Case("a", "F_%s whole core" % fam, [c], [("head", fam, "whole")]))
        out.append(Case("a", "F_%s first 64" % fam, [c[:70]], [("head", fam, "64"), ("xtotal", 64 * (FAMILIES[fam] - 1))]))
        out.append(Case("a", "F_%s first 65" % fam, [c[:71]], [("head", fam, "65")]))
        out.append(Case("a", "F_%s mutated" % fam, [_mutated(c)], [("head", fam, "mutated")]))
    for x in XTOTALS:                                                    # ---- b
        draw = lambda r, x=x: compose(d, _xtotal_parts(x), r)[0]   # noqa: E731
        out.append(Case("b", "xtotal %d" % x, [draw(rng)], [("xtotal", x)], redraw=draw))
    for first, parts in ((127, [("4", 42), ("2", 1), ("5", 1), ("random", 30)]), (128, [("5", 32), ("5", 1), ("random", 30)])):
        draw = lambda r, parts=parts: compose(d, parts, r)[0]      # noqa: E731
        out.append(Case("c", "first item %d" % first, [draw(rng)], [("owner", first)], redraw=draw))
    for n in LONE:
        for pos in (0, 63, 64):
            q = _lone(d, rng, n, pos, 400)
            assert table_slots_for(oracle.size_in_kmer(q)) >= n
            out.append(Case("c", "S_%d at %d" % (n, pos), [q], [("lone", pos, n), ("xtotal", n - 1 if pos < 64 else 0)]))
    for kmers, fams in ((7, ("63", "64", "65")), (43, ("63", "64", "65")), (44, ("65", "128", "129"))):   # ---- d
        for fam in fams:
            L, slots = FAMILIES[fam], table_slots_for(kmers)
            q = _fill_query(d, rng, d.core[fam][40:53], kmers)
            out.append(Case("d", "F_%s in %d k-mers" % (fam, kmers), [q], [("fill", L, slots)], overflow=1 if L > slots else None))
    for n in BIG:
        q = _fill_query(d, rng, d.big[n], 2800 + 7)
        out.append(Case("d", "%d in 4096 slots" % n, [q], [("fill", n, 4096)], overflow=1 if n > 4096 else None))
    n_hint = gtierref.GRP_WQ_WINDOWS                                     # ---- e
    for _ in range(200):
        q = _rnd(rng, 8185) + d.core["3"][100:122] + _rnd(rng, 8192 + 80 + 6 - 8185 - 22)
        cnt = d.counts(q)
        if (cnt[8185:8201] == 3).all() and not cnt[8179:8185].any() and not cnt[8201:8207].any() and len(cnt) == 8192 + 80:
            break
    out.append(Case("e", "one query over window %d" % n_hint, [q], [("hint", n_hint)]))
    short = [p[:13] for p in d.background[:10]]
    for _ in range(200):
        q = _rnd(rng, 8100) + d.core["2"][30:66] + _rnd(rng, 40) + d.core["4"][50:90] + _rnd(rng, 8306 - 8100 - 36 - 40 - 40)
        cnt = d.counts(q)   # (with the 70 positions of the short queries before it: flat 8170-8199 and 8246-8279)
        if len(cnt) == 8300 and (cnt[8100:8130] == 2).all() and (cnt[8176:8210] == 4).all():
            break
    out.append(Case("e", "ten short queries, then one over window %d" % n_hint, short + [q], [("hint", n_hint)]))
    out.append(Case("f", "one F_6 window, 20 times", [d.core["6"][60:73]] * 20, [("runs", "query")]))   # ---- f
    for s in SHIFTS:
        out.append(Case("f", "%d k-mers of F_2, then F_3" % s, [d.core["2"][10:10 + s + 6], d.core["3"]], [("runs", s)]))
    for c in out:   # 0 where no add can run out of probes; d: 64 ids in 64 slots is such a case, 128 in 128 is not
        stays = _stays_in_lds(d, c)
        assert stays or c.kind == "d", c
        assert not (stays and c.overflow == 1), c
        if c.kind == "d" and c.overflow is None and stays:
            c.overflow = 0
    _cases["protein"] = out
    return out


# ---- g: the ORF forms ------------------------------------------------------------------------------------------------
# Left out, because an ORF cannot reach them: the cases of e (8 000 positions) and the families of 4 096 and 4 097 (a table
# of 4 096 slots) -- a table above PK_ARENA - 512 + 64 slots (192 for reads, 576 for longer sequences) goes to the G tier
# uncounted; the 7-k-mer queries of d (an ORF has 21 residues or more: 15 k-mers); the runs of f, which need two queries
# at chosen flat positions.  (A pack holds a dozen windows at most: PK_WHINT = 64 windows with a hint are never used up.)
# The lone lists of 385 and 386 ids need 576 slots: they are planted in queries of 350 residues.
def _orf_form(d, rng, case, aa, max_kmers, aligned):
    """the read that encodes `aa` (behind up to 63 random residues that move its positions to the lanes the claims name,
    when they name any: the read's other ORFs come first in the pack; every 64 tries the query is drawn again), on both
    strands -> [Case, Case] or None"""
    for t in range(3200 if aligned else 1):
        if t and t % 64 == 0:
            aa = case.redraw(rng)
        q = (_rnd(rng, t % 64) if aligned else b"") + aa
        if d.oracle.size_in_kmer(q) > max_kmers:
            continue
        fwd = Case("g", "%s: %s" % (case.kind, case.name), [nt(q)], case.claims, case.overflow, nucleotide=True)
        if q.decode("latin-1") in [o["seq"] for o in d.oracle.get_orfs(fwd.seqs[0])] and all(check_claim(d, fwd, c, anywhere=True) for c in case.claims):
            return [fwd, Case("g", fwd.name + " (minus strand)", [rc(fwd.seqs[0])], [], case.overflow, nucleotide=True)]
    return None


def orf_cases(oracle):
    """the ORF forms of a, b, c and d: the same amino-acid queries back-translated, one read a batch, on both strands; and
    one contig that carries the whole cores"""
    if "orf" in _cases:
        return _cases["orf"]
    d = database(oracle)
    rng = np.random.default_rng(717)
    out, missed = [], []
    for c in cases(oracle):
        aa, max_kmers = c.seqs[0], 384
        if c.kind in ("e", "f") or (c.kind == "d" and ("4096 slots" in c.name or "in 7 k-mers" in c.name)) or (c.kind == "a" and "whole" in c.name):
            continue
        if c.kind == "c" and c.name.startswith("S_"):
            n, pos = c.claims[0][2], c.claims[0][1]
            if pos == 64:
                continue                      # (the pad decides the window: lane 0 is the same target)
            draw = lambda r, n=n, pos=pos: _lone(d, r, n, pos, 350 if n > 130 else 200)   # noqa: E731
            aa = draw(rng)
            c = Case("c", c.name, [aa], [("lone", pos, n)], redraw=draw)
        if c.kind == "d":
            max_kmers = 44                    # reads of at most 150 nt: the 640-slot arena
        if c.kind == "a":
            c = Case("a", c.name, c.seqs, c.claims[:1])
        aligned = any(cl[0] in ("xtotal", "owner", "lone") for cl in c.claims)
        got = _orf_form(d, rng, c, aa, max_kmers, aligned)
        if got is None:
            missed.append(c.name)
        else:
            out += got
    assert not missed, "no ORF form of %r" % missed
    # the contig: every core between a stop codon with a start codon and a stop codon, on alternating strands, between
    # random gaps.  (An ORF that follows a stop codon starts at its first start codon: M and the whole core.)
    gap = lambda: bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 90)])   # noqa: E731
    contig = gap()
    for i, fam in enumerate(HEADS):
        body = b"TAAATG" + nt(d.core[fam]) + b"TAA"
        contig += (body if i % 2 == 0 else rc(body)) + gap()
    c = Case("g", "a: contig of the whole cores", [contig], [("head", fam, "whole") for fam in HEADS], nucleotide=True)
    assert all(check_claim(d, c, cl, anywhere=True) for cl in c.claims)
    out.append(c)
    for c in out:
        stays = _stays_in_lds(d, c)
        assert stays or c.name.startswith("d:"), c
        if c.name.startswith("d:") and c.overflow is None and stays:
            c.overflow = 0
    _cases["orf"] = out
    return out


def required_targets():
    """every target of the lists above: each must be claimed, and met, by at least one case -> (protein, orf)"""
    head = [("head", f, form) for f in HEADS for form in ("whole", "64", "65", "mutated")]
    xt = [("xtotal", x) for x in XTOTALS]
    own = [("owner", 127), ("owner", 128)]
    lone = [("lone", pos, n) for n in LONE for pos in (0, 63, 64)]
    fill = [("fill", 63, 64), ("fill", 64, 64), ("fill", 65, 64), ("fill", 65, 128), ("fill", 128, 128), ("fill", 129, 128)]
    big = [("fill", 4096, 4096), ("fill", 4097, 4096)]
    rest = [("hint", gtierref.GRP_WQ_WINDOWS), ("runs", "query")] + [("runs", s) for s in SHIFTS]
    return head + xt + own + lone + fill + big + rest, head + xt + own + [t for t in lone if t[1] != 64] + fill
