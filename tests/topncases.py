"""A hand-built world for the post-step kernel (topn_kernel: sortMapByValue, SetBestStartCodon, FilterResults), shared by
tests/test_topn_cases_host.py and tests/test_gpu_topn_edges.py: one database, reads whose target ORF meets a designed hit
constellation (start-codon rule, ties, hit counts at the kernel's cache edges), protein queries with all-equal hit lists,
and per case the contract the CPU oracle's result has to meet, so that no case is vacuous.  Pure Python + numpy; the oracle
module is handed in by the caller.  Test infrastructure only.

How a case is made:
  * amino acids are back-translated with codons that are no start codons of table 11, so a start is where the case puts
    ATG and nowhere else in that frame ('I' is never used: all its codons are starts; L and V take CTT and GTT);
  * a read is [TAA] + codons(ORF) + [TAA]: with the leading stop the ORF begins at its ATG (starts[0] == 0), without it
    the ORF is the frame's first one and begins at the read's first codon; without the closing stop it runs off the read;
    the minus-strand form is the reverse complement;
  * a database protein is W + segment + W + segment ... + W with segment = ORF[s : s + Kmatch + 6]: that protein's Kmatch
    with the ORF and s, its first matching position.  'W' never occurs in a crafted ORF or query, so no k-mer across a
    segment's edge matches anything.  Padding hits (Kmatch 1..5, behind position 20) bring a case to its exact hit count.
"""
import numpy as np

CODON = dict(A="GCT", C="TGT", D="GAT", E="GAA", F="TTT", G="GGT", H="CAT", K="AAA", L="CTT", N="AAT", P="CCT", Q="CAA",
             R="CGT", S="TCT", T="ACT", V="GTT", Y="TAT", M="ATG")
ALPHA = "ACDEFGHKLNPQRSTVY"          # no I, no W (the filler), no M (put where a case wants a start)
FILL = "W"
ORF_LEN = 46                         # residues of a crafted ORF without its '*': SizeInKmer 40
BEST = 22                            # Kmatch of a designed best hit: ORF[18:46]
SPECIAL_IDS = (0, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFD, 0xFFFFFFFE)
ORF_COUNTS = (1, 2, 3, 16, 17, 127, 128, 129, 300)     # the G = 16 width: 16 | 17 one key register to two, 128 | 129 cached to re-scan
ORF_TIE_COUNTS = (16, 17, 128, 129)
PROTEIN_TIE_COUNTS = (64, 65, 511, 512, 513)           # the G = 64 width
ORIENTATIONS = ((True, True), (True, False), (False, True), (False, False))   # (plus strand, closed by a stop)

R_EXACT, R_TRIMMED = 22 / 40, 22 / 24
MAX_RESULTS = (1, 2, 3, 10, 15, 16, 17, 18, 65, 126, 127, 128, 129, 130, 299, 300, 301, 700)   # n - 1, n, n + 1 of every count; 65; 700
GATE_OPTS = ((0.05, 10, 10), (0.6, 10, 10), (R_EXACT, 10, 10), (R_TRIMMED, 10, 10), (float(np.nextafter(R_TRIMMED, 1.0)), 10, 10),
             (0.0, 10, 65))
OPTS = GATE_OPTS + tuple((0.0, 1, m) for m in MAX_RESULTS)
ALL = (0.0, 1, 700)                  # every hit reported


def revcomp(nt):
    return nt[::-1].translate(str.maketrans("ACGT", "TGCA"))


class World:
    """the database under construction: protein id -> its segments"""

    def __init__(self, seed=20261020):
        self.rng = np.random.default_rng(seed)
        self.segs = {}
        self.taken = set(SPECIAL_IDS)
        self.cases = []

    def residues(self, n):
        return "".join(ALPHA[i] for i in self.rng.integers(0, len(ALPHA), n))

    def new_ids(self, k):
        """k unused protein ids, uniform over 32 bits (half of them >= 2^31), ascending"""
        out = []
        while len(out) < k:
            v = int(self.rng.integers(0, 0xFFFFFFFF))
            if v not in self.taken:
                self.taken.add(v)
                out.append(v)
        return sorted(out)

    def add_hit(self, pid, seg):
        if not 0 <= pid < 0xFFFFFFFF:
            raise ValueError("protein id 0xFFFFFFFF is reserved")
        assert len(seg) >= 7 and FILL not in seg
        self.segs.setdefault(int(pid), []).append(seg)

    def database(self):
        """-> (sequences, ids uint32) in a shuffled order"""
        ids = sorted(self.segs)
        order = np.random.default_rng(7).permutation(len(ids))
        ids = [ids[i] for i in order]
        return [(FILL + FILL.join(self.segs[p]) + FILL).encode() for p in ids], np.array(ids, np.uint32)


def _orf_case(w, name, n, starts, hits, trim, lead_stop=True, plus=True, closed=True, ids=None, flows=None, reported=None,
              length=ORF_LEN, pads_at=(20, 7, 5), guard=None):
    """one read.  starts: the ORF positions that hold M; hits: [(rank, s, Kmatch)], the designed hits, rank = the order of
    their ids; ids: their ids (else drawn at random places among the case's n ids); the rest of the n hits is padding.
    trim: what SetBestStartCodon must answer when the gate lets it run.  flows: {options: None (gated) | (kept, trim)};
    reported: {options: [ranks]}, the designed hits reported, in order; length: residues of the ORF; pads_at: (first
    position, positions, Kmatch values) of the padding hits; guard: the position of an L written TTA, a stop on the other
    strand"""
    aa = list(w.residues(length))
    for s in starts:
        aa[s] = "M"
    if guard is not None:
        aa[guard] = "L"
    aa = "".join(aa)
    assert not lead_stop or (starts and starts[0] == 0)
    codons = [CODON[a] for a in aa]
    if guard is not None:
        codons[guard] = "TTA"
    nt = ("TAA" if lead_stop else "") + "".join(codons) + ("TAA" if closed else "")
    hits = sorted(hits)
    assert [h[0] for h in hits] == list(range(len(hits))) and len(hits) <= n
    if ids is None:
        pool = w.new_ids(n)
        at = sorted(int(i) for i in w.rng.choice(n, len(hits), replace=False))
        ids = [pool[i] for i in at]
        pads = [p for i, p in enumerate(pool) if i not in set(at)]
    else:
        assert list(ids) == sorted(ids) and len(ids) == len(hits)
        pads = w.new_ids(n - len(hits))
    designed = {}
    for (rank, s, km), pid in zip(hits, ids):
        assert s + km + 6 <= length
        w.add_hit(pid, aa[s:s + km + 6])
        designed[pid] = (km, s)
    for j, pid in enumerate(pads):
        s, km = pads_at[0] + j % pads_at[1], 1 + j % pads_at[2]
        assert s + km + 6 <= length
        w.add_hit(pid, aa[s:s + km + 6])
    c = dict(kind="orf", name="%s n=%d %s %s" % (name, n, "plus" if plus else "minus", "closed" if closed else "open"),
             read=(nt if plus else revcomp(nt)).encode(), orf=aa + ("*" if closed else ""), plus=plus, n=n, starts=list(starts),
             designed=designed, ids=list(ids), trim=trim, flows=dict(flows or {}), reported=dict(reported or {}),
             n_best=sum(1 for h in hits if h[2] == max(x[2] for x in hits)) if hits else 0)
    w.cases.append(c)
    return c


def _start_codon_cases(w):
    S = [0, 16, 26]
    one, tie0 = (0, 18, BEST), (1, 0, BEST)
    # name, smallest n, starts, designed hits, trim, leading stop, flows
    table = [
        # the feasibility case: trim 16, SizeInKmer 40 -> 24; 22/40 < 0.6 <= 22/24: it passes because it was trimmed
        ("one best hit", 1, S, [one], 16, True, {(0.6, 10, 10): (1, 16), (R_EXACT, 10, 10): (1, 16), (R_TRIMMED, 10, 10): (1, 16),
                                                 GATE_OPTS[4]: (0, 16)}),
        # starts at 0, below p, exactly p and p + 1: the <= of dna.go:241 chooses p
        ("starts around p", 1, [0, 10, 18, 19], [one], 18, True, {}),
        ("tie, the higher id matches at 0", 2, S, [one, tie0], 0, True,
         {(0.6, 10, 10): (0, 0), (R_EXACT, 10, 10): (2, 0), (R_TRIMMED, 10, 10): (0, 0)}),
        ("tie, the higher id matches at 1", 2, S, [one, (1, 1, BEST)], 16, True, {}),
        ("tie swapped, the lower id matches at 0", 2, S, [(0, 0, BEST), (1, 18, BEST)], 0, True, {}),
        ("tie swapped, the lower id matches late", 2, S, [(0, 17, BEST), (1, 3, BEST)], 16, True, {}),
        ("three tied, only the last matches at 0", 3, S, [one, (1, 17, BEST), (2, 0, BEST)], 0, True, {}),
        ("three tied, the last matches at 2", 3, S, [one, (1, 17, BEST), (2, 2, BEST)], 16, True, {}),
        # the non-best hit has the lower id
        ("a non-best hit matches at 0", 2, S, [(0, 0, 15), (1, 18, BEST)], 16, True, {}),
        ("starts[0] above the first best position", 1, [20, 30], [(0, 10, BEST)], 0, False, {}),
        ("a single start", 1, [0], [one], 0, True, {}),
        ("the frame's first ORF", 1, [3, 16], [one], 16, False, {}),
        ("no start at all", 1, [], [one], 0, False, {}),
    ]
    for name, n_min, starts, hits, trim, lead, flows in table:
        for n in ORF_COUNTS:
            if n < n_min:
                continue
            for plus, closed in ORIENTATIONS:
                ids = None
                if len(hits) == 2 and n in (17, 129) and (plus, closed) == (True, True):
                    ids = [0, 0xFFFFFFFE]            # the extremes of the key's low word decide the tie
                _orf_case(w, name, n, starts, hits, trim, lead_stop=lead, plus=plus, closed=closed, ids=ids, flows=flows)


def _gate_and_filter_cases(w):
    S = [0, 16, 26]
    for n in (3, 129):
        for plus, closed in ORIENTATIONS:
            # best Kmatch == MinKMatch: reported, trimmed; 10/24 and 10/40 both pass 0.05
            _orf_case(w, "best Kmatch at MinKMatch", n, S, [(0, 18, 10)], 16, plus=plus, closed=closed,
                      flows={(0.05, 10, 10): (1, 16), (0.0, 10, 65): (1, 16)})
            # one below: the reference returns before SetBestStartCodon
            _orf_case(w, "best Kmatch below MinKMatch", n, S, [(0, 18, 9)], 16, plus=plus, closed=closed,
                      flows={(0.05, 10, 10): None, (0.0, 10, 65): None, (0.0, 1, 1): (1, 16)})
            # the same with a tie at the top, which would not trim
            _orf_case(w, "tied best Kmatch below MinKMatch", n, S, [(0, 18, 9), (1, 0, 9)], 0, plus=plus, closed=closed,
                      flows={(0.05, 10, 10): None, (0.0, 1, 2): (2, 0)})
    for n in (8, 130):
        for plus, closed in ORIENTATIONS:
            # MaxResults cuts a run of six tied hits behind the best one: the lower ids stay
            tied = [(r, 18 + r % 3, 15) for r in range(6)]
            hits = [(3, 18, BEST)] + [(r if r < 3 else r + 1, s, km) for r, s, km in tied]
            _orf_case(w, "a cut inside a run of ties", n, S, hits, 16, plus=plus, closed=closed,
                      flows={(0.0, 1, 3): (3, 16), (0.0, 10, 65): (7, 16), (0.05, 10, 10): (7, 16)},
                      reported={(0.0, 1, 3): [3, 0, 1], (0.0, 1, 1): [3], (0.0, 1, 2): [3, 0]})


def _orf_tie_cases(w):
    S = [0, 16, 26]
    for n in ORF_TIE_COUNTS:
        for plus, closed in ORIENTATIONS:
            ids = sorted(list(SPECIAL_IDS) + w.new_ids(n - len(SPECIAL_IDS)))
            _orf_case(w, "all hits tied", n, S, [(r, 18, BEST) for r in range(n)], 16, plus=plus, closed=closed, ids=ids)
            ids = sorted(list(SPECIAL_IDS) + w.new_ids(n - len(SPECIAL_IDS)))
            z = n - 2                                    # id 0xFFFFFFFD: the one tied hit that matches at 0
            _orf_case(w, "all hits tied, one matches at 0", n, S, [(r, 0 if r == z else 18, BEST) for r in range(n)], 0,
                      plus=plus, closed=closed, ids=ids)


def _mix_cases(w):
    """the ORFs of one wave.  A read of 63 nucleotides holds one ORF and no other: frame 1 has the 21 codons an ORF needs,
    frames 2 and 3 have 20, and the TTA in the middle is a stop in the only other frame of 21.  Four such reads at the head
    of the batch are the ORFs 0..3: re-scanned | cached | no hit | gated (wave_mix_groups finds them in the oracle's list)"""
    short = dict(lead_stop=False, closed=False, length=21, pads_at=(8, 3, 3), guard=10)
    _orf_case(w, "mix: re-scanned", 140, [1, 4], [(0, 5, 10)], 4, **short)
    _orf_case(w, "mix: cached", 37, [1, 4], [(0, 5, 10)], 4, **short)
    _orf_case(w, "mix: no hit", 0, [1, 4], [], 0, **short)
    _orf_case(w, "mix: gated", 23, [1, 4], [(0, 5, 9)], 4, flows={(0.05, 10, 10): None}, **short)


def _protein_cases(w):
    for n in PROTEIN_TIE_COUNTS:
        q = w.residues(30)
        ids = sorted(list(SPECIAL_IDS) + w.new_ids(n - len(SPECIAL_IDS)))
        for pid in ids:
            w.add_hit(pid, q[2:28])                      # Kmatch 20 of SizeInKmer 24, for every one of them
        w.cases.append(dict(kind="protein", name="protein query, %d tied hits" % n, query=q.encode(), n=n, ids=ids, kmatch=20))


_world = None


def world():
    """-> the World with every case built (once per process; deterministic)"""
    global _world
    if _world is None:
        w = World()
        _mix_cases(w)
        _start_codon_cases(w)
        _gate_and_filter_cases(w)
        _orf_tie_cases(w)
        _protein_cases(w)
        _world = w
    return _world


def orf_cases():
    return [c for c in world().cases if c["kind"] == "orf"]


def protein_cases():
    return [c for c in world().cases if c["kind"] == "protein"]


def pack(seqs):
    offs = np.zeros(len(seqs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    return np.frombuffer(b"".join(seqs), np.uint8).copy(), offs


def reads():
    """the crafted reads, the wave mix first"""
    return [c["read"] for c in orf_cases()]


def protein_queries():
    """the tied protein queries between ordinary short ones (one too short to be searched)"""
    qs = []
    for c in protein_cases():
        qs += [c["query"], c["query"][:9], c["query"][5:25]]
    return qs


# ---------------------------------------------------------------- the reference's flow, on the oracle
class OrfView:
    """one ORF as the oracle sees it: its hits in reporting order, their first positions, and the reference's post-steps"""

    def __init__(self, O, oix, read_index, o):
        self.O, self.read_index, self.o = O, read_index, o
        self.seq, self.starts, self.plus, self.start = o["seq"], list(o["starts"]), o["plus"], o["start"]
        self.size = O.size_in_kmer(o["seq"])
        self.pid, self.km, self.pos = oix.search(o["seq"], size=self.size, want_positions=True)
        self.n = len(self.km)
        self.fp = self.pos.argmax(axis=1).astype(np.int64) if self.n else np.zeros(0, np.int64)
        self._sbsc = None

    def best_start(self):
        """SetBestStartCodon -> (trim, StartPosition, SizeInKmer)"""
        if self._sbsc is None:
            self._sbsc = self.O.set_best_start_codon(self.km, self.pos, self.size, self.starts, self.plus, self.seq, self.start)
        return self._sbsc

    def flow(self, ratio, mink, maxr):
        """search_fastq.go:119-123 -> None when the gate ends it (no hit, or the best Kmatch below MinKMatch), else
        (kept, trim, StartPosition, SizeInKmer)"""
        if self.n == 0 or self.km[0] < mink:
            return None
        t, sp, so = self.best_start()
        return self.O.filter_results(self.km, so, ratio, mink, maxr), t, sp, so


def reference_orfs(O, oix, read_list):
    """every ORF of the reads, in batch order"""
    return [OrfView(O, oix, ri, o) for ri, r in enumerate(read_list) for o in O.get_orfs(r)]


def target_of(case, views, read_index):
    """the ORF of the case among the views of its read"""
    mine = [v for v in views if v.read_index == read_index and v.seq == case["orf"] and v.plus == case["plus"]]
    assert len(mine) == 1, case["name"]
    return mine[0]


def check_contract(case, v):
    """what the oracle's result of the case's ORF must show, or the case does not test what its name says"""
    name = case["name"]
    assert v.n == case["n"], (name, v.n)
    assert v.starts == case["starts"], (name, v.starts)
    got = dict(zip(v.pid.tolist(), zip(v.km.tolist(), v.fp.tolist())))
    for pid, (km, s) in case["designed"].items():
        assert got[pid] == (km, s), (name, pid, got[pid])
    if case["n_best"] >= 2:
        assert v.km[0] == v.km[1] and int((v.km == v.km[0]).sum()) == case["n_best"], name
        assert v.pid[:case["n_best"]].tolist() == sorted(v.pid[:case["n_best"]].tolist()), name
    if v.n:
        kept, trim, sp, so = v.flow(*ALL)
        assert kept == v.n and trim == case["trim"], (name, trim)
        if trim:
            assert so == v.size - trim and sp == v.start + (3 * trim if v.plus else -3 * trim), name
        else:
            assert (sp, so) == (v.start, v.size), name
        for m in MAX_RESULTS:
            assert v.flow(0.0, 1, m)[0] == min(v.n, m), (name, m)
    for opts, want in case["flows"].items():
        f = v.flow(*opts)
        assert (f if f is None else f[:2]) == want, (name, opts, f)
    for opts, ranks in case["reported"].items():
        assert v.pid[:v.flow(*opts)[0]].tolist() == [case["ids"][r] for r in ranks], (name, opts)


def wave_mix_groups(views, mink=10):
    """the aligned groups of four consecutive ORF indices (qi // 4) that hold an ORF with more than 128 hits (re-scanned),
    one with 1..128 (cached), one without a hit and one that the gate of MinKMatch stops"""
    def kind(v):
        if v.n == 0:
            return "none"
        if v.km[0] < mink:
            return "gated"
        return "rescan" if v.n > 128 else "cached"
    return [g for g in range(len(views) // 4) if {kind(v) for v in views[4 * g:4 * g + 4]} == {"none", "gated", "rescan", "cached"}]


def check_protein_contract(case, pid, km):
    assert len(pid) == case["n"] and pid.tolist() == case["ids"] and set(km.tolist()) == {case["kmatch"]}, case["name"]
    assert pid[0] == 0 and pid[-1] == 0xFFFFFFFE and int((pid >= 2 ** 31).sum()) >= 3, case["name"]
