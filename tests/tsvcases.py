"""Hand-built inputs for the tests of the TSV rows (test_tsv_host.py on the host formatter, test_gpu_tsv_rows.py on the
device stage): a batch is a list of record names and a list of queries; from it come the reference's view (tsvref.rows_ref),
a result as the host formatter takes it, and the arrays the device stage takes.  Test infrastructure."""
import types

import numpy as np

from kaamer_amd import api

FEATURES = [b"Organism", b"EC", b"Note"]


def query(src, size, hits, start=1, end=None, pos_len=None):
    """one query (a protein record, or an ORF of record `src`): hits = [(protein id, kmatch[, bits])] in reporting order,
    empty: not reported; size: SizeInKmer as printed (an ORF's: after the trim); pos_len: bits per bitmap (as searched)"""
    hits = [dict(key=int(h[0]), kmatch=int(h[1]), bits=(list(h[2]) if len(h) > 2 else None)) for h in hits]
    pos_len = size if pos_len is None else pos_len
    for h in hits:
        if h["bits"] is None:
            h["bits"] = [False] * max(pos_len, 0)
        assert len(h["bits"]) == max(pos_len, 0)
    return dict(src=int(src), size=int(size), start=int(start), end=int(size + 6 if end is None else end), hits=hits, pos_len=int(pos_len))


def make_table(id_lens, value_lens, seq_lens=None):
    """an api.Proteins table (TSV rules: ids 0, 1, ... in row order) whose entry i has an EntryId of id_lens[i] bytes, a
    sequence of seq_lens[i] residues and the three FEATURES with value lengths value_lens[i] (a triple)"""
    rows = [b"EntryID\tSequence\t" + b"\t".join(FEATURES)]
    aa = b"ACDEFGHIKLMNPQRSTVWY"
    for i, (il, vl) in enumerate(zip(id_lens, value_lens)):
        assert il >= 1
        eid = (b"%d_" % i + b"abcdefghijklmnopqrstuvwxyz" * (il // 26 + 1))[:il]
        sl = seq_lens[i] if seq_lens is not None else 7 + i
        seq = (aa * (sl // len(aa) + 1))[:sl]
        vals = [bytes((65 + (i + f + j) % 26) for j in range(n)) for f, n in enumerate(vl)]
        rows.append(eid + b"\t" + seq + b"\t" + b"\t".join(vals))
    return api.Proteins.from_tsv(b"\n".join(rows) + b"\n")


def names_buffer(names, gap=b"\n"):
    """the records' names in one byte buffer (as the header lines of a text lie in it) -> (bytes, SPAN_DTYPE spans)"""
    buf = b""
    spans = np.zeros(len(names), api.SPAN_DTYPE)
    for i, n in enumerate(names):
        buf += b"@"
        spans[i]["name_off"], spans[i]["name_len"] = len(buf), len(n)
        buf += n + gap
    return buf, spans


def ref_queries(names, queries):
    """the reported queries as tsvref.rows_ref takes them"""
    return [dict(name=names[q["src"]] if q["src"] < len(names) else b"", size_in_kmer=q["size"], start=q["start"], end=q["end"], hits=q["hits"])
            for q in queries if q["hits"]]


def pack_bits(bits):
    n = len(bits)
    padded = np.zeros(((n + 63) // 64) * 64, np.uint8)
    padded[:n] = np.asarray(bits, bool)
    return np.packbits(padded, bitorder="little").view(np.uint64) if n else np.zeros(0, np.uint64)


def host_top(queries):
    """the reported queries as a result the host formatter takes (the arrays of an api.TopResult)"""
    rep = [q for q in queries if q["hits"]]
    top = types.SimpleNamespace()
    top.n_queries, top.n_reported = len(queries), len(rep)
    top.max_results = max([len(q["hits"]) for q in rep] + [1])
    top.meta = np.zeros(len(rep), api.META_DTYPE)
    top.top_off = np.zeros(len(rep) + 1, np.uint64)
    pid, km, words, poff = [], [], [], [0]
    top.pos_bits_len = np.zeros(len(rep), np.int32)
    for i, q in enumerate(rep):
        m = top.meta[i]
        m["src_seq"], m["size_in_kmer"], m["start_position"], m["end_position"] = q["src"], q["size"], q["start"], q["end"]
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
    return top


def device_arrays(queries, K):
    """the arrays kaamer_tsv_rows_device takes, as numpy: the fields of kaamer_topn_result and kaamer_topn_positions over ALL
    queries (dense, K slots per query), and the queries' meta"""
    nq = len(queries)
    a = types.SimpleNamespace()
    a.meta = np.zeros(max(nq, 1), api.META_DTYPE)
    a.top_cnt = np.zeros(max(nq, 1), np.uint32)
    a.top_pid = np.full(max(nq, 1) * K, 0xDEADBEEF, np.uint32)   # (slots beyond top_cnt are never read)
    a.top_km = np.full(max(nq, 1) * K, 0xDEADBEEF, np.uint32)
    a.start = np.zeros(max(nq, 1), np.int32)
    a.size = np.zeros(max(nq, 1), np.int32)
    a.pos_len = np.zeros(max(nq, 1), np.int32)
    a.pos_base = np.zeros(nq + 1, np.uint64)
    words = []
    for i, q in enumerate(queries):
        assert len(q["hits"]) <= K
        a.meta[i]["src_seq"], a.meta[i]["end_position"] = q["src"], q["end"]
        a.meta[i]["size_in_kmer"], a.meta[i]["start_position"] = 12345, -7   # (the untrimmed ones: the stage must not print them)
        a.top_cnt[i] = len(q["hits"])
        a.start[i], a.size[i] = q["start"], q["size"]
        a.pos_len[i] = q["pos_len"] if q["hits"] else 0
        nw = 0
        for r, h in enumerate(q["hits"]):
            a.top_pid[i * K + r], a.top_km[i * K + r] = h["key"], h["kmatch"]
            w = pack_bits(h["bits"])
            words.append(w)
            nw += len(w)
        a.pos_base[i + 1] = a.pos_base[i] + np.uint64(nw)
    a.pos_bits = np.concatenate(words + [np.zeros(1, np.uint64)])
    return a


LENS = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257]
MISSING = 1000          # a protein id without an entry in standard_table()
INTS = [0, 9, 10, 99, 100, 2147483647]
FLOAT_VECTORS = [((1, 32), "3.12"), ((3, 32), "9.38"), ((5, 32), "15.62"), ((1, 800), "0.12"), ((23, 160), "14.38"),
                 ((47, 160), "29.37"), ((7, 7), "100.00")]
BITMAP_LENS = [1, 63, 64, 65, 128, 129]


def standard_table():
    """13 entries: EntryId and value lengths over LENS (an EntryId has at least one byte), an entry whose values are all
    empty, one with a 1 000-byte value; Protein.Length from 7 to 12345"""
    id_lens = [max(n, 1) for n in LENS] + [3, 5]
    value_lens = [(LENS[i], LENS[(i + 3) % 11], LENS[(i + 7) % 11]) for i in range(11)] + [(0, 0, 0), (1000, 0, 2)]
    seq_lens = [7, 9, 10, 99, 100, 101, 999, 1000, 12345, 8, 11, 7, 20]
    return make_table(id_lens, value_lens, seq_lens)


N_ENTRIES = 13


def bitmap_patterns(n):
    """all set; alternating; a run across the word boundary; a run reaching the end; only the last bit set; none"""
    pats = [[True] * n, [i % 2 == 0 for i in range(n)], [60 <= i < 70 for i in range(n)], [i >= n - 3 for i in range(n)],
            [i == n - 1 for i in range(n)], [False] * n, [i % 64 in (0, 62, 63) for i in range(n)]]
    return pats


def float_sweep(n_max=400, extra=(65530, 1000003)):
    """every 1 <= k <= n <= n_max, the issue's vectors, and a few k for each large n"""
    qs = [query(0, n, [(k % N_ENTRIES, k)]) for n in range(1, n_max + 1) for k in range(1, n + 1)]
    qs += [query(0, n, [(0, k)]) for (k, n), _ in FLOAT_VECTORS]
    for n in extra:
        qs += [query(0, n, [(1, k)], pos_len=0) for k in (1, 2, 3, 7, n // 3, n // 2, n - 1, n)]
    return [b"sweep"], qs


def standard_cases():
    """name -> (record names, queries): the cases both formatters are checked on (the float sweep is float_sweep())"""
    c = {}
    c["integers"] = ([b"ints"], [query(0, v, [(i % N_ENTRIES, w)], start=w, end=v, pos_len=0)
                                 for i, v in enumerate(INTS) for w in INTS])
    names = [b"", b"nospace", b" leading space", b"tab\tbefore space", b"two  spaces", b"trailing "]
    names += [b"n" * n for n in LENS] + [b"n" * n + b" rest of the header" for n in LENS]
    c["names"] = (names, [query(i, 20 + i, [(i % N_ENTRIES, 5 + i)]) for i in range(len(names))])
    # reads: several ORFs of one record, unreported ones in between, a trimmed start (fewer k-mers printed than searched)
    c["orfs"] = ([b"read/1 first", b"read/2", b"read/3 third"],
                 [query(0, 40, [(2, 30, [i < 30 for i in range(43)]), (5, 12, [i % 5 == 0 for i in range(43)])], start=10, end=138, pos_len=43),
                  query(0, 12, []), query(0, 17, [(1, 9, [True] * 17)], start=150, end=82),
                  query(1, 30, []), query(1, 31, []),
                  query(2, 25, [(7, 25, [True] * 29)], start=13, end=105, pos_len=29), query(2, 9, [])])
    # every entry: EntryId / value lengths, 1 to 10 hits per query
    qs, e = [], 0
    for cnt in (1, 10, 3, 9, 2, 10, 1):
        qs.append(query(len(qs) % 2, 50, [((e + r) % N_ENTRIES, 50 - r) for r in range(cnt)]))
        e += cnt
        qs.append(query(0, 11, []))
    c["entries"] = ([b"q0 x", b"q1"], qs)
    c["missing"] = ([b"m"], [query(0, 60, [(2, 30), (MISSING, 20), (3, 10)]), query(0, 60, [(3, 5)]), query(0, 60, [(0xFFFFFFFF, 4), (1, 3)]),
                             query(0, 60, [(4, 9), (5, 8), (N_ENTRIES, 7)])])
    qs = []
    for n in BITMAP_LENS:
        pats = bitmap_patterns(n)
        qs.append(query(0, n, [((i + n) % N_ENTRIES, sum(p), p) for i, p in enumerate(pats)]))
        qs.append(query(0, n, []))
    c["bitmaps"] = ([b"bits and pieces"], qs)
    c["empty"] = ([], [])
    c["none reported"] = ([b"a", b"b"], [query(0, 10, []), query(1, 12, [])])
    return c
