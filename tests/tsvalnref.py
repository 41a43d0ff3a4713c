"""The TSV response of the reference WITH alignment, restated line by line from pkg/search/search.go:556-604 (rows),
:649-660 (header) and :483-494 (the sort), over plain Python data.  Identity is a float32: numpy for the value, `decimal`
for what strconv does with it (its exact value, half-even at the second decimal).  EValue and BitScore are float64: Python's
own "%e" and "%.2f" are correctly rounded on the double's exact value, as strconv is; only the spelling of NaN and the
infinities is Go's.  The positions are FormatPositionsToString(bitmap, true) as test_top_positions_host.py restates it.
Test infrastructure: shared by the host and the device tests of the -aln rows."""
import decimal
import math

import numpy as np

from test_top_positions_host import format_positions_ref

HEADER = "QueryId\tSubjectId\t%Identity\tAlnLength\tMismatches\tGapOpen\tQStart\tQEnd\tSStart\tSEnd\tEvalue\tBitscore"
EMPTY = dict(identity=0.0, length=0, mismatches=0, gap_openings=0, query_start=0, query_end=0, subject_start=0, subject_end=0,
             evalue=0.0, bitscore=0.0)   # the zero AlignmentResult a failed hit keeps


def header_ref(positions, annotations, features):
    """search.go:649 + :651-660"""
    out = HEADER.encode()
    if positions:
        out += b"\tQueryPositions"
    if annotations:
        for annotation in features:
            out += b"\t"
            out += annotation
    out += b"\n"
    return out


def go_special(x):
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "+Inf" if x > 0 else "-Inf"
    return None


def e_ref(x):
    """fmt.Sprintf("%e", float64)"""
    return go_special(x) or "%e" % x


def f2_ref(x):
    """fmt.Sprintf("%.2f", float64)"""
    return go_special(x) or "%.2f" % x


def identity_ref(x):
    """fmt.Sprintf("%.2f", float32)"""
    x = np.float32(x)
    s = go_special(float(x))
    if s:
        return s
    d = decimal.Decimal(float(x))   # exact: a float32 is a double is a finite decimal
    return str(d.quantize(decimal.Decimal("0.01"), rounding=decimal.ROUND_HALF_EVEN))


def sorted_hits(hits):
    """search.go:491-493: BitScore descending; ties keep their order (the library's statement of sort.Slice)"""
    return sorted(hits, key=lambda h: -h["aln"]["bitscore"])


def rows_ref(queries, entries, features, positions, annotations, protein):
    """queries: the reported queries in ascending order, each a dict(name bytes, start, end, hits), hits in sortMapByValue
    order, each a dict(key, aln: the fields of the AlignmentResult[, bits: list of bool]).  entries as tsvref.rows_ref takes
    them: HitEntries is filled BEFORE the sort and stops at the first key without an entry (search.go:454-470).
    protein: SequenceType == PROTEIN.  -> (bytes, line_off)"""
    out, size = [], 0
    line_off = []
    for q in queries:
        hit_entries = {}
        for h in q["hits"]:
            if h["key"] not in entries:
                break
            hit_entries[h["key"]] = entries[h["key"]]
        for h in sorted_hits(q["hits"]):
            e = hit_entries.get(h["key"], dict(EntryId=b"", Length=0, Features={}))
            a = h["aln"]
            line_off.append(size)
            output = q["name"].split(b" ")[0]
            output += b"\t"
            output += e["EntryId"]
            output += b"\t"
            output += identity_ref(a["identity"]).encode()
            output += b"\t"
            output += b"%d" % a["length"]
            output += b"\t"
            output += b"%d" % a["mismatches"]
            output += b"\t"
            output += b"%d" % a["gap_openings"]
            output += b"\t"
            if not protein:
                output += str(q["start"]).encode()
                output += b"\t"
                output += str(q["end"]).encode()
                output += b"\t"
            else:
                output += b"%d" % a["query_start"]
                output += b"\t"
                output += b"%d" % a["query_end"]
                output += b"\t"
            output += b"%d" % a["subject_start"]
            output += b"\t"
            output += b"%d" % a["subject_end"]
            output += b"\t"
            output += e_ref(float(a["evalue"])).encode()
            output += b"\t"
            output += f2_ref(float(a["bitscore"])).encode()
            if positions:
                output += b"\t"
                output += format_positions_ref(list(h["bits"]), True).encode()
            if annotations:
                for annotation in features:
                    output += b"\t"
                    output += e["Features"].get(annotation, b"")
            output += b"\n"
            out.append(output)
            size += len(output)
    line_off.append(size)
    return b"".join(out), np.array(line_off, np.uint64)


def aln_of(rec):
    """an ALN_DTYPE record (kaamer_alignment) -> the AlignmentResult fields rows_ref reads"""
    return {k: (float(rec[k]) if k in ("evalue", "bitscore") else np.float32(rec[k]) if k == "identity" else int(rec[k]))
            for k in EMPTY}
