"""The G tier's stage decisions (kaamer_amd/csrc/count_global.hip.inc), restated for the tests: from the oracle index, the
figures of ONE query that decide which stage of count_global_kernel counts it -- the whole query in the LDS table, the
partition into id-range buckets with guessed or with counted sizes, the table in HBM -- and the recipes of the inputs
that tests/test_gpu_gtier_stages.py sends through each of them.

Test infrastructure only.  Every constant is read from the source; the comment names where."""
import numpy as np

import tableref

LDS_CAP = 1 << 13                   # count_global.hip.inc: BIG_LOG2CAP 13
LDS_LIMIT = LDS_CAP - LDS_CAP // 4  # BigLdsTable::LIMIT: the attempt fails on the insertion that finds this many ids there
LDS_PROBES = 128                    # BigLdsTable::add_n: slots an id walks before the attempt is given up
LDS_MAX_SIZE = 65535                # count_global_kernel: positions are 16 bits of a table word ("size < 65535")
MAX_RANGES = 64                     # G_MAX_RANGES
RANGE_POSTINGS = 16384              # partition phase: R = postings / 16384 + 2
RANGE_MUL = 0x85EBCA6B              # g_range_of
GUESS_SLACK = 2048                  # partition phase, sizes guessed: per + per / 4 + 2048
LONG_LIST = 8                       # lists of more ids than this go to the sink
LONG_SINK_CAP = 960                 # entries of the sink
XIT = 2                             # count_windows: rounds of 64 leftovers a window keeps in registers
HEAD_IDS = 3                        # count_windows: ids that come with a list's head (run-merged by add_runs)
TABLE_MUL = 0x9E3779B1              # BigLdsTable::add_n: home slot = (id * TABLE_MUL) >> (32 - 13)
# what decides that count_pack_kernel sends an ORF on unseen (count_pack.hip.inc: max_table; search.hip: enqueue_count)
GRP_MIN_TABLE, GRP_MAX_TABLE = 64, 4096   # count_group.hip.inc
PK_ARENA_ORF, PK_ARENA_ORF_LONG = 640, 1024   # search.hip
PACK_SHIFT_NUCLEOTIDE = 9           # search.hip: ws->pack_shift
# the LDS tier's window steps (tests/windowcases.py)
INLINE_BIT = 1 << 31                # kaamer_layout.h: KH_INLINE_BIT
GRP_SHIFT = 11                      # count_group.hip.inc: GRP_SHIFT (a protein batch counts units of 1 << GRP_SHIFT + 1 slots)
GRP_FIT = (1 << GRP_SHIFT) - 64 + GRP_MAX_TABLE   # count_group.hip.inc: GRP_FIT, the slots of the group kernel's arena
GRP_MAX_PROBES = 96                 # count_window.hip.inc: GRP_MAX_PROBES
GRP_LONG_UNROLL = 4                 # count_group.hip.inc: GRP_LONG_UNROLL
GRP_WQ_WINDOWS = 128                # count_group.hip.inc: s_wq[2 * 64], filled while "w < 128u"
PK_WHINT = 64                       # count_pack.hip.inc: PK_WHINT

ALPHA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
_M32 = np.uint64(0xFFFFFFFF)


def range_of(ids, R):
    """g_range_of: the bucket of a protein id among R"""
    ids = np.asarray(ids).astype(np.uint64)
    return ((((ids * np.uint64(RANGE_MUL)) & _M32) * np.uint64(R)) >> np.uint64(32)).astype(np.int64)


def lds_longest_run(ids):
    """The longest run of occupied slots the LDS table has once it holds the distinct `ids` (linear probing: the set of
    occupied slots does not depend on the order of the insertions).  No id walks more slots than that, so a run shorter
    than LDS_PROBES says that the 128-probe cut-off cannot fire, whatever order the waves insert in."""
    ids = np.unique(np.asarray(ids, dtype=np.uint32)).astype(np.uint64)
    assert len(ids) < LDS_CAP
    home = ((ids * np.uint64(TABLE_MUL)) & _M32) >> np.uint64(32 - 13)
    arrive = np.bincount(home.astype(np.int64), minlength=LDS_CAP).tolist()
    occ = [False] * LDS_CAP
    carry = 0
    for rnd in range(2):           # the second round takes what the first one carried past the last slot
        for i in range(LDS_CAP):
            have = carry + (arrive[i] if rnd == 0 else 0)
            if have and not occ[i]:
                occ[i] = True
                have -= 1
            carry = have
    best = run = 0
    for i in range(2 * LDS_CAP):
        run = run + 1 if occ[i % LDS_CAP] else 0
        best = max(best, run)
    return min(best, LDS_CAP)


def table_slots_for(size):
    """count_group.hip.inc table_slots_for at scale 1 (a workspace's first batch)"""
    want = (size * 24 >> 4) + 63 & ~63
    return min(max(want, GRP_MIN_TABLE), GRP_MAX_TABLE)


def pack_sends_unseen(size, long_orfs=True):
    """count_pack_kernel hands an ORF to the G tier uncounted (wi.size < 0) when its table is larger than the wave's arena
    allows: PK_ARENA - (1 << pack_shift) + 64 slots"""
    arena = PK_ARENA_ORF_LONG if long_orfs else PK_ARENA_ORF
    return table_slots_for(size) > arena - (1 << PACK_SHIFT_NUCLEOTIDE) + 64


class Figures:
    """What one query's postings look like to count_global_kernel."""

    def __init__(self, oracle, oix, seq, pairs=None):
        seq = bytes(seq)
        self.size = oracle.size_in_kmer(seq)
        assert self.size >= 7
        keys = tableref.encode_windows(seq, np.arange(self.size)).astype(np.uint64)
        pairs = np.sort(oix.pairs()) if pairs is None else pairs        # (key << 32 | id): every list ascending, as the arena holds it
        lo = np.searchsorted(pairs, keys << np.uint64(32))
        hi = np.searchsorted(pairs, (keys + np.uint64(1)) << np.uint64(32))
        cnt = (hi - lo).astype(np.int64)
        off = np.zeros(self.size + 1, dtype=np.int64)
        np.cumsum(cnt, out=off[1:])
        self.P = int(off[-1])                                           # postings behind the query's positions
        at = np.repeat(lo - off[:-1], cnt) + np.arange(self.P, dtype=np.int64)
        self.cnt = cnt
        self.ids = (pairs[at] & _M32).astype(np.uint32)                 # one per (position, id) pair
        self.pos = np.repeat(np.arange(self.size, dtype=np.int64), cnt)
        self.idx = np.arange(self.P, dtype=np.int64) - np.repeat(off[:-1], cnt)   # its index in its list
        self.distinct = np.unique(self.ids)
        self.D = len(self.distinct)
        # the counters a query adds: a list is a value that is not inline, i.e. a key with two ids or more -- or with one
        # id of 2^31 or more, which kaamer_layout.h cannot store inline (KH_INLINE_BIT is the value's top bit)
        first = np.zeros(self.size, dtype=np.uint32)
        first[cnt > 0] = self.ids[off[:-1][cnt > 0]]
        self.listed = (cnt >= 2) | ((cnt == 1) & (first >= np.uint32(INLINE_BIT)))
        self.n_lists = int(self.listed.sum())
        self.n_list_ids = int(cnt[self.listed].sum())
        # partition
        self.R = min(MAX_RANGES, self.P // RANGE_POSTINGS + 2)
        per = self.P // self.R
        self.guess = per + per // 4 + GUESS_SLACK
        rng = range_of(self.ids, self.R)
        self.upper = np.bincount(rng, minlength=self.R)                 # every pair is an item of its own
        self.lower = np.bincount(rng[self.idx >= HEAD_IDS], minlength=self.R)   # only the three head ids are ever run-merged
        self.range_distinct = np.bincount(range_of(self.distinct, self.R), minlength=self.R)
        # long lists
        self.n_long = int((cnt > LONG_LIST).sum())

    def first_positions(self):
        """{id: the lowest position that hits it}"""
        order = np.lexsort((self.pos, self.ids))
        ids, at = np.unique(self.ids[order], return_index=True)
        return dict(zip(ids.tolist(), self.pos[order][at].tolist()))

    # ---- the regimes ----------------------------------------------------------------------------------------------
    def lds_holds(self):
        return self.size < LDS_MAX_SIZE and self.D <= LDS_LIMIT

    def guess_holds(self):
        return bool((self.upper <= self.guess).all())

    def guess_fails(self):
        return bool((self.lower > self.guess).any())

    def bucket_overflows(self):
        """some range has at least 8 000 distinct ids: more than the LDS table takes, with the margin of lds_holds"""
        return bool((self.range_distinct >= 8000).any())

    def buckets_fit(self):
        return bool((self.range_distinct <= 5000).all())

    def sink_overflow(self):
        """long lists beyond the sink's capacity in one sweep: the waves that meet them expand them themselves"""
        return max(0, self.n_long - LONG_SINK_CAP)

    def window_beyond_registers(self):
        """A 64-position window with more than XIT * 64 leftovers among the lists its wave expands itself, whichever
        LONG_SINK_CAP lists the sink takes: the lists it does not take number sink_overflow(), they lie in the windows
        that hold a long list at all, so one of those windows keeps at least the mean; each has at least
        LONG_LIST + 1 - HEAD_IDS leftovers."""
        windows = len(np.unique(np.flatnonzero(self.cnt > LONG_LIST) // 64))
        if windows == 0:
            return False
        least = -(-self.sink_overflow() // windows)
        fewest = int(self.cnt[self.cnt > LONG_LIST].min()) - HEAD_IDS
        return least * fewest > XIT * 64


# ---- inputs -----------------------------------------------------------------------------------------------------------
def _fill(rng, n):
    return bytes(ALPHA[rng.integers(0, 20, int(n))])


def motif_family(rng, n, motif, flank=12):
    """n proteins that share `motif` between random flanks"""
    return [_fill(rng, flank) + motif + _fill(rng, flank) for _ in range(n)]


def input_lds():
    """(a) one 20-residue motif shared by 4 800 proteins -> (db, ids, query)"""
    rng = np.random.default_rng(101)
    motif = _fill(rng, 20)
    return motif_family(rng, 4800, motif), None, _fill(rng, 30) + motif + _fill(rng, 30)


def input_guess_holds():
    """(b) the 14-position x 12 000-id input of tests/test_gpu_edges.py::test_postings_lists_of_ten_thousand"""
    rng = np.random.default_rng(9)
    motif = _fill(rng, 20)
    motif2 = _fill(rng, 12)
    seqs = []
    for i in range(12000):
        body = bytearray(_fill(rng, 60))
        body[20:40] = motif
        if i % 3 == 0:
            body[44:56] = motif2
        seqs.append(bytes(body))
    return seqs, None, _fill(rng, 30) + motif + _fill(rng, 30)


def input_guess_fails():
    """(c) 8 000 proteins behind ONE k-mer, and 40 proteins that share one stretch of 3 000 residues, their ids all in one
    range of the R = 9 that the query's postings (8 000 + 40 x 2 994) give it"""
    rng = np.random.default_rng(103)
    kmer = _fill(rng, 7)
    stretch = _fill(rng, 3000)
    db = [_fill(rng, 11) + kmer + _fill(rng, 11) for _ in range(8000)]
    db += [_fill(rng, 5) + stretch + _fill(rng, 5) for _ in range(40)]
    R = (8000 + 40 * 2994) // RANGE_POSTINGS + 2
    cand = np.arange(8000, 20000)
    ids = np.concatenate([np.arange(8000), cand[range_of(cand, R) == 4][:40]]).astype(np.uint32)
    return db, ids, stretch + kmer


def input_bucket_overflows():
    """(d) 30 000 proteins behind a single k-mer position (the residues next to the k-mer differ between database and
    query, so the windows that overlap it match nothing: the postings are those 30 000 and R is 3)"""
    rng = np.random.default_rng(104)
    kmer = _fill(rng, 7)
    db = [_fill(rng, 10) + b"A" + kmer + b"A" + _fill(rng, 10) for _ in range(30000)]
    return db, None, _fill(rng, 19) + b"C" + kmer + b"C" + _fill(rng, 19)


def input_long_query():
    """(e) a motif of 5 000 proteins inside 66 000 random residues"""
    rng = np.random.default_rng(105)
    motif = _fill(rng, 20)
    return motif_family(rng, 5000, motif), None, _fill(rng, 30000) + motif + _fill(rng, 36000)


_CODON = {a: c for a, c in zip("ACDEFGHIKLMNPQRSTVWY", ("GCT", "TGT", "GAT", "GAA", "TTT", "GGT", "CAT", "ATT", "AAA", "CTT", "ATG", "AAT",
                                                       "CCT", "CAA", "CGT", "TCT", "ACT", "GTT", "TGG", "TAT"))}


def input_fresh():
    """(g) a family of 300 proteins (a 700-residue parent, 5 % substitutions each) and a nucleotide sequence that encodes
    the parent between two stop codons -> (db, ids, dna, parent)"""
    rng = np.random.default_rng(107)
    parent = np.frombuffer(b"M" + _fill(rng, 699), dtype=np.uint8)
    db = []
    for _ in range(300):
        p = parent.copy()
        p[rng.integers(0, 700, 35)] = ALPHA[rng.integers(0, 20, 35)]
        db.append(bytes(p))
    dna = "TAA" + "".join(_CODON[chr(c)] for c in parent) + "TAA"
    return db, None, dna.encode(), bytes(parent)
