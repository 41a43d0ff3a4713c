"""The TSV response of the reference without alignment, restated line by line from pkg/search/search.go:505-554 (rows) and
636-662 (header), over plain Python data.  Field 3 uses numpy float32 for the two roundings of
float32(Kmatch) / float32(SizeInKmer) * float32(100) and `decimal` for what strconv does with the float32 (its exact
value, rounded half-even at the second decimal); field 11 is FormatPositionsToString as test_top_positions_host.py
restates it.  Test infrastructure: shared by the host and the device tests of the rows."""
import decimal

import numpy as np

from test_top_positions_host import format_positions_ref

HEADER = "QueryId\tSubjectId\t%KMatchIdentity\tQueryKLength\tKMatch\tGapOpen\tQStart\tQEnd\tSStart\tSEnd"


def header_ref(positions, annotations, features):
    """search.go:645-660 with Align = false"""
    out = HEADER.encode()
    if positions:
        out += b"\tQueryPositions"
    if annotations:
        for annotation in features:
            out += b"\t"
            out += annotation
    out += b"\n"
    return out


def identity_ref(kmatch, size_in_kmer):
    """fmt.Sprintf("%.2f", float32(h.Kmatch) / float32(qR.Query.SizeInKmer) * float32(100.00)), search.go:514"""
    with np.errstate(all="ignore"):
        x = np.float32(np.float32(kmatch) / np.float32(size_in_kmer)) * np.float32(100.0)
    x = np.float32(x)
    if np.isnan(x):
        return "NaN"
    if np.isinf(x):
        return "+Inf" if x > 0 else "-Inf"
    d = decimal.Decimal(float(x))   # exact: a float32 is a double is a finite decimal
    return str(d.quantize(decimal.Decimal("0.01"), rounding=decimal.ROUND_HALF_EVEN))


def rows_ref(queries, entries, features, positions, annotations):
    """queries: the reported queries in ascending order, each a dict(name bytes, size_in_kmer, start, end, hits), hits in
    reporting order, each a dict(key, kmatch[, bits: list of bool, the bitmap as searched]).  entries: {key: dict(EntryId
    bytes, Length, Features {name bytes: value bytes})} -- HitEntries as FetchHitsInformation fills it: a query's loop
    stops at the first key without an entry (search.go:461-463), so from that hit on the lookups give the zero Protein.
    -> (bytes, line_off)"""
    out, size = [], 0
    line_off = []
    for q in queries:
        hit_entries = {}
        for h in q["hits"]:
            if h["key"] not in entries:
                break
            hit_entries[h["key"]] = entries[h["key"]]
        for h in q["hits"]:
            e = hit_entries.get(h["key"], dict(EntryId=b"", Length=0, Features={}))
            line_off.append(size)
            pos_string = ""
            output = q["name"].split(b" ")[0]
            output += b"\t"
            output += e["EntryId"]
            output += b"\t"
            output += identity_ref(h["kmatch"], q["size_in_kmer"]).encode()
            output += b"\t"
            output += str(q["size_in_kmer"]).encode()
            output += b"\t"
            output += str(int(h["kmatch"])).encode()
            output += b"\t"
            if positions:
                pos_string = format_positions_ref(list(h["bits"]), False)
                output += str(pos_string.count(",")).encode()
            else:
                output += b"N/A"
            output += b"\t"
            output += str(q["start"]).encode()
            output += b"\t"
            output += str(q["end"]).encode()
            output += b"\t"
            output += b"1"
            output += b"\t"
            if annotations:
                output += str(e["Length"]).encode()
            else:
                output += b"N/A"
            if positions:
                output += b"\t"
                output += pos_string.encode()
            if annotations:
                for annotation in features:
                    output += b"\t"
                    output += e["Features"].get(annotation, b"")
            output += b"\n"
            out.append(output)
            size += len(output)
    line_off.append(size)
    return b"".join(out), np.array(line_off, np.uint64)


def entries_of(proteins):
    """{key: entry} of an api.Proteins table, resolved as kaamer_fetch_hits does"""
    ids = sorted(set(int(i) for i in proteins.ids))
    return {k: dict(EntryId=e["EntryId"], Length=e["Length"], Features=e["Features"])
            for k, e in zip(ids, proteins.fetch_hits(ids)) if e is not None}


def queries_of(top, names, spans, positions):
    """the `queries` of rows_ref from an api.TopResult and the records' names (bytes + SPAN_DTYPE spans)"""
    out = []
    for i in range(top.n_reported):
        m = top.meta[i]
        s = spans[int(m["src_seq"])]
        name = bytes(names[int(s["name_off"]):int(s["name_off"]) + int(s["name_len"])])
        hits = []
        for e in range(int(top.top_off[i]), int(top.top_off[i + 1])):
            h = dict(key=int(top.top_pid[e]), kmatch=int(top.top_kmatch[e]))
            if positions:
                size = int(top.pos_bits_len[i])
                w = top.pos_bits[int(top.pos_off[e]):int(top.pos_off[e]) + (size + 63) // 64]
                h["bits"] = np.unpackbits(w.view(np.uint8), bitorder="little")[:size].astype(bool).tolist()
            hits.append(h)
        out.append(dict(name=name, size_in_kmer=int(m["size_in_kmer"]), start=int(m["start_position"]), end=int(m["end_position"]),
                        hits=hits))
    return out
