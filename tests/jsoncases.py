"""Hand-built inputs for the tests of the JSON response (test_json_host.py on the host formatter, test_gpu_json_rows.py on
the device stage).  A case is a dict: the protein table it reads (TABLES), the request (protein / nucleotide, FASTA or FASTQ
records, ExtractPositions), the records' names, the protein records' sequences and the queries.  From it come the
reference's view (ref_queries, for jsonref.objects), a result as the host formatter takes it (host_top) and the arrays the
device stage takes (device_arrays).  The tables are written down twice: as the text makedb reads, and as the entries the
reference would hold -- so that jsonref never sees the library's view of them.  Test infrastructure."""
import types

import numpy as np

from kaamer_amd import api
from tsvcases import pack_bits, names_buffer   # noqa: F401  (names_buffer: re-exported for the tests)

BS = b"\x5c"
U2028, U2029 = b"\xe2\x80\xa8", b"\xe2\x80\xa9"
# every class of the escaping rules in one string: quote, backslash, the three short forms, control bytes (0x08 and 0x0c have
# no short form), the HTML three, 0x7f, valid 2-, 3- and 4-byte runes, the two separators, and invalid bytes: an overlong
# form, a surrogate, a value beyond U+10FFFF, 0xff, a stray continuation, a rune cut short before an ASCII byte and at the end
ESCAPES = (b'q"' + BS + b"\n\r\t\x01\x08\x0c\x1f<>&\x7f" + "é€\U0001f600".encode("utf-8") + U2028 + U2029 +
           b"\xc0\x80\xed\xa0\x80\xf4\x90\x80\x80\xff\x80\xe2\x82z\xe2\x82")
VALID_ESCAPES = b'q"' + BS + b"\n\r\t\x01\x08\x0c\x1f<>&\x7f" + "é€\U0001f600".encode("utf-8") + U2028 + U2029
AA = b"ACDEFGHIKLMNPQRSTVWY"
MISSING = 100000   # an id no table holds


def residues(n, shift=0):
    return bytes(AA[(i * 7 + shift) % 20] for i in range(n))


# ---------------------------------------------------------------- the tables
FEATURES = [b"Organism", b"EC", b"Note&more"]   # KStats.Features order; byte order: EC, Note&more, Organism
N_STD = 104


def _std_rows():
    """(EntryId, Sequence, [value per FEATURES]) of the TSV table: ids 0, 1, ... in row order"""
    rows = []
    for i in range(N_STD):
        eid = b"E%d" % i
        seq = residues(7 + i % 40, i)
        vals = [b"org %d" % i, b"1.1.%d" % i, b"n" * (i % 19)]
        if i == 0:
            eid = b'id"q' + BS + b"b"
        elif i == 1:
            vals = [b"", b"", b""]
        elif i == 2:   # (a TSV field holds no tab and no line break; every other escape class)
            vals = [b"a<b>c&d", ESCAPES.replace(b"\n", b"").replace(b"\r", b"").replace(b"\t", b""), b"\x01\x7f"]
        elif i == 3:
            seq = residues(5000, 3)
            vals = [b"v" * 1000, b"", b"x"]
        elif i == 4:
            seq = residues(12345, 4)
        rows.append((eid, seq, vals))
    return rows


def _tsv_text(rows, features):
    lines = [b"\t".join([b"EntryID", b"Sequence"] + features)]
    lines += [b"\t".join([e, s] + v) for e, s, v in rows]
    return b"\n".join(lines) + b"\n"


_FASTA = [(b"", b"just a name", residues(9, 1)), (b"sp|P1|X", b"kinase <alpha> & co", residues(30, 2)), (b"noname", None, residues(8, 3)),
          (b"Q9", b'with "quotes"', residues(11, 4)), (b"last", b"the last one", residues(7, 5))]


def table(name):
    """-> (api.Proteins, {id: entry as jsonref takes it}, KStats.Features)"""
    if name == "std":
        rows = _std_rows()
        ent = {i: dict(entry_id=e, sequence=s, length=len(s), features=list(zip(FEATURES, v))) for i, (e, s, v) in enumerate(rows)}
        return api.Proteins.from_tsv(_tsv_text(rows, FEATURES)), ent, FEATURES
    if name == "nofeat":   # no feature columns: Features is left out of every entry
        rows = [(b"N%d" % i, residues(8 + i, i), []) for i in range(5)]
        ent = {i: dict(entry_id=e, sequence=s, length=len(s), features=[]) for i, (e, s, v) in enumerate(rows)}
        return api.Proteins.from_tsv(_tsv_text(rows, [])), ent, []
    if name == "fasta":
        # the FASTA reader: entry k (from 1) is stored under k + 1 -- it is queued when the next header is read -- and the last
        # under the number of headers, where it replaces the one before it; "> name" has an empty EntryId
        text = b"".join(b">" + e + (b" " + n if n is not None else b"") + b"\n" + s + b"\n" for e, n, s in _FASTA)
        ent = {}
        for k, (e, n, s) in enumerate(_FASTA, 1):
            ent[k + 1 if k < len(_FASTA) else k] = dict(entry_id=e, sequence=s, length=len(s), features=[(b"ProteinName", n or b"")])
        return api.Proteins.from_fasta(text), ent, [b"ProteinName"]
    raise KeyError(name)


TABLES = ("std", "nofeat", "fasta")


# ---------------------------------------------------------------- the cases
def query(src, hits, seq=None, start=1, end=None, pos_len=None, trim=0, plus=False):
    """one query: a protein record (seq None: the record's sequence) or an ORF of record `src` (seq: its residues BEFORE the
    trim).  hits = [(protein id, kmatch[, bits as searched])] in reporting order, empty: not reported.  pos_len: bits per
    bitmap as searched (default: the untrimmed SizeInKmer)."""
    hits = [dict(key=int(h[0]), kmatch=int(h[1]), bits=(list(h[2]) if len(h) > 2 else None)) for h in hits]
    return dict(src=int(src), seq=seq, start=int(start), end=end, hits=hits, pos_len=pos_len, trim=int(trim), plus=bool(plus))


def _finish(case):
    """fills what follows from the rest: sequences, sizes, ends, default bitmaps"""
    for q in case["queries"]:
        if q["seq"] is None:
            q["seq"] = case["seqs"][q["src"]] if q["src"] < len(case["seqs"]) else b""
        n = len(q["seq"])
        if q["pos_len"] is None:
            q["pos_len"] = max(n - 6, 0)
        if q["end"] is None:
            q["end"] = n
        q["size"] = n - q["trim"] - 6 - (1 if q["seq"][-1:] == b"*" else 0)
        for h in q["hits"]:
            if h["bits"] is None:
                h["bits"] = [(i * 7 + h["key"]) % 3 == 0 for i in range(q["pos_len"])]
            assert len(h["bits"]) == q["pos_len"]
    return case


def case(table_name, protein, fmt, positions, names, queries, seqs=()):
    return _finish(dict(table=table_name, protein=protein, fmt=fmt, positions=positions, names=list(names), seqs=list(seqs), queries=list(queries)))


def pattern(n, kind):
    return [[True] * n, [False] * n, [i % 2 == 0 for i in range(n)], [60 <= i < 70 for i in range(n)], [i == n - 1 for i in range(n)],
            [i % 64 in (0, 62, 63) for i in range(n)]][kind % 6]


def standard_cases(valid=False):
    """name -> case.  valid: no invalid UTF-8 anywhere (names, sequences, the entries that are hit), for the checks that decode
    the response with Python's json module"""
    c = {}
    E, two = (VALID_ESCAPES, 12) if valid else (ESCAPES, 2)
    names = [b"", b"plain", b"with spaces in it", E, b"x" * 257]
    seqs = [residues(20), residues(7, 1) + b"*", E + residues(10), residues(300, 2), residues(64, 3).lower()]
    hits = [(5, 9), (6, 4)]
    qs = [query(i, hits if i != 1 else [(7, 1)]) for i in range(5)] + [query(9, [(8, 2)])]   # (a record beyond the names and the sequences)
    c["protein"] = case("std", True, 0, False, names, qs, seqs)
    c["protein positions"] = case("std", True, 0, True, names, qs, seqs)
    # ORFs: trim 0, trim > 0 on both strands, unreported ones in between; FASTQ records (Contig "") and FASTA contigs
    orfs = [query(0, [(two, 30, pattern(43, 2)), (5, 12, pattern(43, 3))], seq=residues(49), start=10, end=156, plus=True),
            query(0, []),
            query(0, [(1, 9, pattern(30, 0))], seq=residues(36, 5), start=150 - 3 * 4, end=42, trim=4, plus=False),
            query(1, []), query(1, []),
            query(2, [(7, 25, pattern(29, 5))], seq=residues(35, 9), start=13 + 3 * 6, end=117, trim=6, plus=True),
            query(2, [])]
    rnames = [b"read/1 first", b"read/2", E]
    c["orfs fastq"] = case("std", False, 1, False, rnames, orfs)
    c["orfs fasta"] = case("std", False, 0, True, rnames, orfs)
    # a trim that is no multiple of 64 on bitmaps longer than 128 bits; a trim equal to the bit length; trims at word edges
    long_orf = residues(206, 1)
    qs = [query(0, [(10 + k, 50, pattern(200, k)) for k in range(6)], seq=long_orf, start=7 + 3 * t, end=624, trim=t, plus=True)
          for t in (0, 1, 63, 64, 65, 70, 127, 128, 129, 199, 200)]
    c["trims"] = case("std", False, 1, False, [b"contig one"], qs)
    # map keys sort as strings: 9, 10, 99, 100 together, and ids of every digit count
    qs = [query(0, [(9, 4), (10, 3), (99, 2), (100, 1)]), query(0, [(100, 9), (99, 9), (10, 9), (9, 9)]),
          query(0, [(1, 5), (103, 5), (12, 5), (22, 5), (20, 5), (3, 5), (30, 5), (102, 5), (11, 5), (0, 5)])]
    c["key order"] = case("std", True, 0, True, [b"keys"], qs, [residues(40)])
    # FetchHitsInformation stops at the first id without an entry: first, in the middle, last; 2^32 - 1
    qs = [query(0, [(MISSING, 9), (two, 8), (3, 7)]), query(0, [(two, 9), (MISSING, 8), (3, 7)]), query(0, [(two, 9), (3, 8), (MISSING, 7)]),
          query(0, [(0xFFFFFFFF, 4), (1, 3)]), query(0, [(4, 9)])]
    c["missing"] = case("std", True, 0, True, [b"m"], qs, [residues(15)])
    # every entry of the table: long sequences and values (entries 3 and 4 are longer than any staging buffer), empty values,
    # escapes in the EntryId and in the values
    qs = [query(0, [(p, 50 - r) for r, p in enumerate((10 * k + r) % N_STD for r in range(10)) if not (valid and p == 2)]) for k in range(11)]
    c["entries"] = case("std", True, 0, False, [b"e"], qs, [residues(60)])
    c["no features"] = case("nofeat", True, 0, False, [b"nf"], [query(0, [(3, 2), (0, 1)]), query(0, [(4, 1)])], [residues(12)])
    c["fasta table"] = case("fasta", False, 0, False, [b"ctg"], [query(0, [(k, 9 - k) for k in (2, 3, 4, 5, 1)], seq=residues(30), start=1, end=90, plus=True)])
    # one object far larger than any buffer: a 5 000-residue query with ten bitmaps
    big = residues(5000, 7)
    c["large"] = case("std", True, 0, True, [b"big one"], [query(0, [(3 + r, 100 - r, pattern(4994, r)) for r in range(10)]), query(1, [(1, 1)])],
                      [big, residues(9)])
    c["none reported"] = case("std", True, 0, True, [b"a", b"b"], [query(0, []), query(1, [])], [residues(10), residues(12)])
    c["empty"] = case("std", True, 0, False, [], [])
    return c


def many_queries(n, seed=1):
    """n ORFs of a few records, about a third of them reported, sizes and hit counts mixed"""
    rng = np.random.RandomState(seed)
    qs = []
    for i in range(n):
        ln = int(rng.randint(7, 120))
        k = 0 if rng.rand() < 0.6 else int(rng.randint(1, 6))
        trim = int(rng.randint(0, max(ln - 6, 1))) if rng.rand() < 0.3 else 0
        ids = rng.choice(N_STD, size=k, replace=False)
        qs.append(query(i % 3, [(int(p), int(rng.randint(1, 40))) for p in ids], seq=residues(ln, i), start=int(rng.randint(1, 500)), end=int(rng.randint(1, 500)),
                        trim=trim, plus=bool(i & 1)))
    return case("std", False, int(seed) & 1, False, [b"r0", b"r1 second", b"r2"], qs)


# ---------------------------------------------------------------- views
def ref_queries(c):
    """the queries as jsonref.objects takes them"""
    out = []
    for q in c["queries"]:
        name = c["names"][q["src"]] if q["src"] < len(c["names"]) else b""
        out.append(dict(name=name, sequence=q["seq"][q["trim"]:], size_in_kmer=q["size"], start=q["start"], end=q["end"], plus=q["plus"], trim=q["trim"],
                        hits=q["hits"]))
    return out


def packed(c):
    """the protein records as a packed batch -> (u8 array, u64 offsets)"""
    off = np.zeros(len(c["seqs"]) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in c["seqs"]]) if c["seqs"] else 0
    return np.frombuffer(b"".join(c["seqs"]), np.uint8), off


def host_top(c):
    """the reported queries as a result the host formatter takes (the arrays of an api.TopResult)"""
    rep = [q for q in c["queries"] if q["hits"]]
    top = types.SimpleNamespace()
    top.n_queries, top.n_reported = len(c["queries"]), len(rep)
    top.max_results = max([len(q["hits"]) for q in rep] + [1])
    top.meta = np.zeros(len(rep), api.META_DTYPE)
    top.trim = np.zeros(len(rep), np.int32)
    top.top_off = np.zeros(len(rep) + 1, np.uint64)
    top.pos_bits_len = np.zeros(len(rep), np.int32)
    top.alignments = None
    pid, km, words, poff, aa = [], [], [], [0], b""
    for i, q in enumerate(rep):
        m = top.meta[i]
        m["src_seq"], m["size_in_kmer"], m["start_position"], m["end_position"], m["plus_strand"] = q["src"], q["size"], q["start"], q["end"], int(q["plus"])
        if not c["protein"]:   # q[] carries the window AFTER the trim (kaamer_batch_top)
            aa += b"#" * (i % 3)
            m["aa_off"], m["aa_len"] = len(aa), len(q["seq"]) - q["trim"]
            aa += q["seq"][q["trim"]:]
        top.trim[i] = q["trim"]
        top.pos_bits_len[i] = q["pos_len"]
        for h in q["hits"]:
            pid.append(h["key"])
            km.append(h["kmatch"])
            w = pack_bits(h["bits"])
            words.append(w)
            poff.append(poff[-1] + len(w))
        top.top_off[i + 1] = len(pid)
    top.top_pid = np.array(pid, np.uint32)
    top.top_kmatch = np.array(km, np.uint32)
    top.pos_off = np.array(poff, np.uint64)
    top.pos_bits = np.concatenate(words) if words and sum(len(w) for w in words) else np.zeros(0, np.uint64)
    top.orf_aa = np.frombuffer(aa, np.uint8)
    return top


def without_bitmaps(top):
    t = types.SimpleNamespace(**vars(top))
    t.pos_bits = t.pos_off = t.pos_bits_len = None
    return t


def device_arrays(c, K):
    """the arrays kaamer_json_rows_device takes, as numpy: the fields of kaamer_topn_result and kaamer_topn_positions over ALL
    queries (dense, K slots per query), the queries' meta with the UNTRIMMED residue windows, and the residues"""
    qs = c["queries"]
    nq = len(qs)
    a = types.SimpleNamespace()
    a.meta = np.zeros(max(nq, 1), api.META_DTYPE)
    a.top_cnt = np.zeros(max(nq, 1), np.uint32)
    a.top_pid = np.full(max(nq, 1) * K, 0xDEADBEEF, np.uint32)   # (slots beyond top_cnt are never read)
    a.top_km = np.full(max(nq, 1) * K, 0xDEADBEEF, np.uint32)
    a.start = np.zeros(max(nq, 1), np.int32)
    a.size = np.zeros(max(nq, 1), np.int32)
    a.trim = np.zeros(max(nq, 1), np.int32)
    a.pos_len = np.zeros(max(nq, 1), np.int32)
    a.pos_base = np.zeros(nq + 1, np.uint64)
    words = []
    if c["protein"]:
        seqs, off = packed(c)
        aa = seqs.tobytes()
    else:
        aa = b""
    for i, q in enumerate(qs):
        assert len(q["hits"]) <= K
        m = a.meta[i]
        m["src_seq"], m["end_position"], m["plus_strand"] = q["src"], q["end"], int(q["plus"])
        m["size_in_kmer"], m["start_position"] = 12345, -7   # (the untrimmed ones: the stage must not print them)
        if c["protein"]:
            m["aa_off"], m["aa_len"] = (int(off[q["src"]]), len(q["seq"])) if q["src"] < len(c["seqs"]) else (len(aa) + 5, 3)
        else:
            aa += b"#" * (i % 3)
            m["aa_off"], m["aa_len"] = len(aa), len(q["seq"])
            aa += q["seq"]
        a.top_cnt[i] = len(q["hits"])
        a.start[i], a.size[i], a.trim[i] = q["start"], q["size"], q["trim"]
        a.pos_len[i] = q["pos_len"] if q["hits"] else 0
        nw = 0
        for r, h in enumerate(q["hits"]):
            a.top_pid[i * K + r], a.top_km[i * K + r] = h["key"], h["kmatch"]
            w = pack_bits(h["bits"])
            words.append(w)
            nw += len(w)
        a.pos_base[i + 1] = a.pos_base[i] + np.uint64(nw)
    a.pos_bits = np.concatenate(words + [np.zeros(1, np.uint64)])
    a.aa = np.frombuffer(aa + b"\0", np.uint8)
    a.aa_len = len(aa)
    return a
