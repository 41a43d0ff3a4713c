"""Hand-built inputs for the tests of the -aln TSV rows (test_tsv_aln_host.py on the host formatter,
test_gpu_tsv_aln_rows.py on the device stage), on top of tsvcases: a query's hits carry the pair record the alignment stage
leaves (kaamer_align_pair, integers only) in sortMapByValue order.  From a batch come the reference's view
(tsvalnref.rows_ref, its floats by kaamer_align_finish_pairs: the library's own host arithmetic), a result as the host
formatter takes it (hits in BitScore order) and the arrays the device stage takes.  Test infrastructure."""
import numpy as np

import tsvalnref
import tsvcases
from kaamer_amd import api

MISSING = tsvcases.MISSING
N_ENTRIES = tsvcases.N_ENTRIES
RAW_MIN, RAW_MAX = -65536, 65535   # the raw scores the device stage tabulates (kaamer_tsv_aln_rows_device)
RAW_TABLE = RAW_MAX - RAW_MIN + 1   # ... their number (kaamer_tsv_aln_info)


def pair(raw=0, n_ops=0, identical=0, status=0, start_i=0, start_j=0, end_i=0, end_j=0, similar=0, mismatches=0, gap_openings=0, query_len=50):
    """one kaamer_align_pair; status 2 / 3 / 4: the hit keeps the empty AlignmentResult whatever the other fields hold"""
    return dict(status=status, n_ops=n_ops, start_i=start_i, start_j=start_j, end_i=end_i, end_j=end_j, identical=identical, similar=similar,
                mismatches=mismatches, gap_openings=gap_openings, raw=raw, query_len=query_len)


def aligned(raw, cols=40, identical=None, query_len=50, shift=0):
    """a plausible aligned pair of `cols` columns"""
    identical = cols // 2 if identical is None else identical
    return pair(raw=raw, n_ops=cols, identical=identical, similar=min(cols, identical + 3), mismatches=cols - identical, gap_openings=shift % 3,
                start_i=shift, start_j=2 * shift, end_i=shift + cols, end_j=2 * shift + cols, query_len=query_len)


def aquery(src, hits, start=1, end=100, pos_len=0):
    """one query: hits = [(protein id, pair[, bits])] in sortMapByValue order, empty: not reported"""
    q = tsvcases.query(src, pos_len, [(h[0], 1) + ((h[2],) if len(h) > 2 else ()) for h in hits], start=start, end=end, pos_len=pos_len)
    for h, src_h in zip(q["hits"], hits):
        h["pair"] = src_h[1]
    return q


def pair_records(queries):
    """the pair records of all hits, in CSR order"""
    hits = [h for q in queries for h in q["hits"]]
    out = np.zeros(len(hits), api.PAIR_DTYPE)
    for i, h in enumerate(hits):
        for k, v in h["pair"].items():
            out[i][k] = v
        out[i]["entry"], out[i]["off"], out[i]["subject_len"] = 0xDEAD, 0xBEEF, 77   # (never printed)
    return out


def with_alignments(queries, number_of_aa, **options):
    """the queries, every hit with `aln` (the AlignmentResult fields) and `rec` (its kaamer_alignment)"""
    recs = api.align_finish_pairs(pair_records(queries), number_of_aa, **options)
    out, e = [], 0
    for q in queries:
        q = dict(q, hits=[dict(h) for h in q["hits"]])
        for h in q["hits"]:
            h["rec"] = recs[e]
            h["aln"] = tsvalnref.aln_of(recs[e])
            e += 1
        out.append(q)
    return out


def ref_queries(names, queries):
    """the reported queries (with_alignments applied) as tsvalnref.rows_ref takes them"""
    return [dict(name=names[q["src"]] if q["src"] < len(names) else b"", start=q["start"], end=q["end"], hits=q["hits"])
            for q in queries if q["hits"]]


def host_top(queries):
    """the reported queries (with_alignments applied) as a result of an aligning call: hits in BitScore order"""
    ordered = [dict(q, hits=tsvalnref.sorted_hits(q["hits"])) for q in queries]
    top = tsvcases.host_top(ordered)
    recs = [h["rec"] for q in ordered for h in q["hits"]]
    top.alignments = np.array(recs, api.ALN_DTYPE) if recs else np.zeros(0, api.ALN_DTYPE)
    return top


def device_arrays(queries, K):
    """tsvcases.device_arrays plus the two arrays of kaamer_topn_alignments"""
    a = tsvcases.device_arrays(queries, K)
    a.pairs = pair_records(queries)
    a.pair_off = np.zeros(len(queries) + 1, np.uint64)
    a.pair_off[1:] = np.cumsum([len(q["hits"]) for q in queries])
    a.pairs = np.concatenate([a.pairs, np.zeros(1, api.PAIR_DTYPE)])
    return a


def standard_cases():
    """name -> (record names, queries)"""
    c = {}
    # the order: equal raw scores keep their rank, increasing ones come out reversed, failed hits (BitScore 0) in the
    # middle of a query go behind the aligned ones and keep their order
    c["order"] = ([b"read/1 first", b"second x", b"p3"],
                  [aquery(0, [(i, aligned(100, shift=i)) for i in range(6)], start=4, end=33),
                   aquery(0, []),
                   aquery(1, [(i, aligned(50 + 10 * i, cols=30 + i, shift=i)) for i in range(10)], start=200, end=18),
                   aquery(2, [(0, aligned(80)), (1, pair(status=2, raw=999, n_ops=5)), (2, aligned(120)), (3, pair(status=3)), (4, aligned(80, cols=7)),
                              (5, aligned(81))]),
                   aquery(2, [(7, aligned(60)), (8, aligned(200)), (MISSING, pair(status=4)), (9, pair(status=4)), (10, pair(status=4))])])
    # the numbers: no columns (Identity NaN, coordinates 1 and 0), raw 0, the ends of the raw scores the device tabulates,
    # negative raw scores (long gaps under the request's penalties: a negative BitScore sorts behind the failed hits'), an
    # EValue that underflows to a subnormal and to 0, integers at their bounds
    big = 2147483647
    c["numbers"] = ([b"n"],
                    [aquery(0, [(1, pair(raw=0, n_ops=0, query_len=0)), (2, pair(raw=0, n_ops=0, query_len=7))]),
                     aquery(0, [(3, aligned(0, cols=1, identical=1)), (4, aligned(RAW_MAX, cols=3, identical=1)), (5, aligned(1, cols=3, identical=2)),
                                (9, aligned(RAW_MIN, cols=5, identical=2)), (10, aligned(-1, cols=4, identical=2)), (11, aligned(-2072, cols=2320, identical=43))]),
                     aquery(0, [(6, aligned(r, cols=7, identical=3, query_len=big)) for r in (2655, 2656, 2770, 2790, 2800, 3000)]),
                     aquery(0, [(7, pair(raw=33, n_ops=big, identical=big, mismatches=big, gap_openings=big, start_i=big - 1, start_j=big - 1, end_i=big,
                                         end_j=big, query_len=0xFFFFFFFF)),
                                (8, pair(raw=34, n_ops=big, identical=1, query_len=1))], start=-big, end=big)])
    # the float32 Identity: every fraction of small denominators, the ties of %.2f among them (1/32 = 3.125, 1/800 = 0.125)
    qs = [aquery(0, [(k % N_ENTRIES, aligned(40 + k, cols=n, identical=k))]) for n in (3, 7, 32, 160, 800) for k in range(0, n + 1, max(n // 40, 1))]
    c["identity"] = ([b"id sweep"], qs)
    names = [b"", b"nospace", b" leading space", b"tab\tbefore space", b"two  spaces", b"trailing "]
    c["names"] = (names, [aquery(i, [(i % N_ENTRIES, aligned(30 + i)), ((i + 1) % N_ENTRIES, aligned(31 + i))]) for i in range(len(names) + 1)])
    # bitmaps travel with their hit through the sort
    qs = []
    for n in tsvcases.BITMAP_LENS:
        pats = tsvcases.bitmap_patterns(n)
        qs.append(aquery(0, [((i + n) % N_ENTRIES, aligned(10 + 7 * i), p) for i, p in enumerate(pats)], pos_len=n))
        qs.append(aquery(0, []))
    c["bitmaps"] = ([b"bits and pieces"], qs)
    c["empty"] = ([], [])
    c["none reported"] = ([b"a", b"b"], [aquery(0, []), aquery(1, [])])
    return c
