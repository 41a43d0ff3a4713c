"""Host-side mirror of the reference's search drivers (pkg/search/search_protein.go,
search_fastq.go, search_nucleotide.go) over the C ABI: same option names and defaults
(api/server.go:139-152), same per-query flow, results as plain dicts shaped like the
reference's JSON (docs/client.md:131-180).  All compute is in libkaamer_hip.so: readers and
k-mer search; sortMapByValue, SetBestStartCodon and FilterResults run on the device
(kaamer_search_batch_top) unless ExtractPositions asks for the full hit lists + bitmaps, in
which case the host versions of the same C ABI are used.  With SearchOptions.Align and a protein table attached to the
index (Index.attach_proteins) the drivers also return HitEntries and every hit's Alignment, hits in BitScore order: the
alignment of the reported hits runs inside the same call (kaamer_search_batch_top_aln_flat).  Without a table the route
is the one below: FetchHitsInformation, then AlignHits.
"""
import ctypes as C
import queue
import threading
from dataclasses import dataclass

import numpy as np

from . import abi, api

PROTEIN_QUERY, DNA_QUERY = "Protein Query", "DNA Query"  # search.go:46-47


@dataclass
class SearchOptions:  # search.go:56-71 (the fields the hot path reads); defaults api/server.go:139-152
    SequenceType: int = abi.PROTEIN
    MaxResults: int = 10
    MinKMatch: int = 10
    MinKRatio: float = 0.05
    ExtractPositions: bool = False
    Annotations: bool = False     # search.go:65: the TSV rows carry Protein.Length and one column per KStats.Features name
    Align: bool = False           # search.go:65; the alignment step: AlignHits below
    SubMatrix: str = "blosum62"   # api/server.go:149-151
    GapOpen: int = 11
    GapExtend: int = 1
    GeneticCode: int = 11         # search.go:60, api/server.go:142: the 6-frame translation's table (nucleotide / reads requests)
    ChunkSeqs: int = 1 << 20      # SearchFile only (no reference counterpart): records per chunk, chunks in flight (0: three)
    InFlight: int = 0
    ChunkTextBytes: int = 1 << 28  # SearchFile(device_parse=True) only: bytes of text per chunk


_EMPTY_ALN = {"Identity": 0.0, "Similarity": 0.0, "Length": 0, "Mismatches": 0, "GapOpenings": 0, "Raw": 0, "BitScore": 0.0,
              "EValue": 0.0, "AlnString": "", "QueryStart": 0, "QueryEnd": 0, "SubjectStart": 0, "SubjectEnd": 0}


def _one_call(index, o):
    """SearchOptions.Align on an index with an attached protein table: top-N and the alignment of the reported hits in ONE
    call (kaamer_search_batch_top_aln_flat) instead of FetchHitsInformation + AlignHits afterwards"""
    return dict(sub_matrix=o.SubMatrix, gap_open=o.GapOpen, gap_extend=o.GapExtend, text=True) \
        if o.Align and getattr(index, "proteins", None) is not None else None


def _with_alignments(qr, top, i, proteins):
    """QueryResultHandler's additions (search.go:454-494) to one QueryResult from a result with alignments: HitEntries
    and every hit's Alignment; the hits already are in BitScore order"""
    a, b = int(top.top_off[i]), int(top.top_off[i + 1])
    alns = top.alignments[a:b]
    keys = [int(p) for p in top.top_pid[a:b] ]
    found = [k for k, al in zip(keys, alns) if al["status"] != 4]      # (4: no entry; FetchHitsInformation stopped there)
    he = qr.setdefault("HitEntries", {})
    for k, e in zip(found, proteins.fetch_hits(found) if found else []):
        he[k] = {"EntryId": e["EntryId"].decode("latin-1"), "Sequence": e["Sequence"].decode("latin-1"), "Length": e["Length"],
                 "Features": {n.decode("latin-1"): v.decode("latin-1") for n, v in e["Features"].items()}}
    for h, al in zip(qr["SearchResults"]["Hits"], alns):
        h["Alignment"] = dict(_EMPTY_ALN) if al["status"] else {
            "Identity": al["identity"], "Similarity": al["similarity"], "Length": al["length"], "Mismatches": al["mismatches"],
            "GapOpenings": al["gap_openings"], "Raw": al["raw"], "BitScore": al["bitscore"], "EValue": al["evalue"],
            "AlnString": "\n".join(al["aln"]), "QueryStart": al["query_start"], "QueryEnd": al["query_end"],
            "SubjectStart": al["subject_start"], "SubjectEnd": al["subject_end"]}
    return qr


def _sorted_hits(res, q):
    """sortMapByValue (search.go:132-152): Kmatch descending (ties by protein id)"""
    a, b = res.span(q)
    pid = np.ascontiguousarray(res.hit_pid[a:b])
    km = np.ascontiguousarray(res.hit_kmatch[a:b])
    order = np.zeros(b - a, dtype=np.uint32)
    abi.lib().kaamer_sort_hits(pid.ctypes.data, km.ctypes.data, b - a, order.ctypes.data)
    return pid[order], km[order], np.ascontiguousarray(res.hit_first_pos[a:b])[order], order + a


def _filter(km_sorted, size, o):
    """FilterResults (search.go:189-220) -> number of hits kept"""
    km = np.ascontiguousarray(km_sorted, dtype=np.uint32)
    return int(abi.lib().kaamer_filter_results(km.ctypes.data, len(km), size, o.MinKRatio, o.MinKMatch, o.MaxResults))


def ProteinSearch(index, fasta_text, options=None):
    """search_protein.go:27-134 for one FASTA upload -> list of QueryResult dicts"""
    o = options or SearchOptions(SequenceType=abi.PROTEIN)
    queries = api.parse_reads(fasta_text, "fasta")
    if not o.ExtractPositions:
        # sortMapByValue + FilterResults on the device: only the reported hits come back
        aln = _one_call(index, o)
        top = index.search_top([q["seq"] for q in queries], seq_type=abi.PROTEIN, min_k_ratio=o.MinKRatio,
                               min_k_match=o.MinKMatch, max_results=o.MaxResults, align=aln)
        out = []
        for r in range(top.n_reported):   # search_protein.go:74-76, :108: the others are not reported
            q = queries[int(top.rep_query[r])]
            a, b = int(top.top_off[r]), int(top.top_off[r + 1])
            out.append({"Query": {"Sequence": q["seq"], "Name": q["name"], "SizeInKmer": q["size"], "Type": PROTEIN_QUERY,
                                  "Location": {"StartPosition": 1, "EndPosition": len(q["seq"]), "PlusStrand": q["plus"],
                                               "StartsAlternative": []}, "Contig": ""},
                        "SearchResults": {"Hits": [{"Key": int(p), "Kmatch": int(k)}
                                                   for p, k in zip(top.top_pid[a:b], top.top_kmatch[a:b])]}})
            if aln is not None:
                _with_alignments(out[-1], top, r, index.proteins)
        return out
    res = index.search([q["seq"] for q in queries], seq_type=abi.PROTEIN, want_positions=o.ExtractPositions)
    out = []
    for i, q in enumerate(queries):
        if q["size"] < 7:  # search_protein.go:74-76
            continue
        pid, km, _, idx = _sorted_hits(res, i)
        keep = _filter(km, q["size"], o)
        if keep == 0:  # search_protein.go:108
            continue
        qr = {"Query": {"Sequence": q["seq"], "Name": q["name"], "SizeInKmer": q["size"], "Type": PROTEIN_QUERY,
                        "Location": {"StartPosition": 1, "EndPosition": len(q["seq"]), "PlusStrand": q["plus"],
                                     "StartsAlternative": []}, "Contig": ""},
              "SearchResults": {"Hits": [{"Key": int(p), "Kmatch": int(k)} for p, k in zip(pid[:keep], km[:keep])]}}
        if o.ExtractPositions:
            pos = res.positions(i)
            qr["SearchResults"]["PositionHits"] = {int(p): pos[int(p)].tolist() for p in pid[:keep]}
        out.append(qr)
    return out


def _orf_results(index, reads, names, o, seq_type):
    if not o.ExtractPositions:
        # SetBestStartCodon, its gate and FilterResults on the device (kaamer_search_batch_top)
        aln = _one_call(index, o)
        top = index.search_top(reads, seq_type=seq_type, min_k_ratio=o.MinKRatio, min_k_match=o.MinKMatch,
                               max_results=o.MaxResults, align=aln)
        out = []
        for i in range(top.n_reported):
            a, b = int(top.top_off[i]), int(top.top_off[i + 1])
            m = top.meta[i]
            aa = bytes(top.orf_aa[int(m["aa_off"]):int(m["aa_off"]) + int(m["aa_len"])])  # already trimmed
            out.append({"Query": {"Sequence": aa.decode("latin-1"), "Name": names[int(m["src_seq"])],
                                  "SizeInKmer": int(m["size_in_kmer"]), "Type": DNA_QUERY,
                                  "Location": {"StartPosition": int(m["start_position"]), "EndPosition": int(m["end_position"]),
                                               "PlusStrand": bool(m["plus_strand"]), "StartsAlternative": []},
                                  "Contig": ""},
                        "SearchResults": {"Hits": [{"Key": int(p), "Kmatch": int(k)}
                                                   for p, k in zip(top.top_pid[a:b], top.top_kmatch[a:b])]}})
            if aln is not None:
                _with_alignments(out[-1], top, i, index.proteins)
        return out
    res = index.search(reads, seq_type=seq_type, want_positions=o.ExtractPositions)
    out = []
    for i in range(res.n_queries):
        m = res.meta[i]
        pid, km, fp, idx = _sorted_hits(res, i)
        if len(km) == 0 or int(km[0]) < o.MinKMatch:  # search_fastq.go:119
            continue
        aa = bytes(res.orf_aa[int(m["aa_off"]):int(m["aa_off"]) + int(m["aa_len"])])
        sa = np.ascontiguousarray(res.starts_alt[int(m["sa_off"]):int(m["sa_off"]) + int(m["sa_len"])], dtype=np.int32)
        start, size = C.c_int32(int(m["start_position"])), C.c_int32(int(m["size_in_kmer"]))
        kmc, fpc = np.ascontiguousarray(km, dtype=np.uint32), np.ascontiguousarray(fp, dtype=np.uint32)
        trimmed = abi.lib().kaamer_set_best_start_codon(kmc.ctypes.data, fpc.ctypes.data, len(kmc),
                                                        sa.ctypes.data if len(sa) else None, len(sa),
                                                        int(m["plus_strand"]), aa, len(aa), C.byref(start), C.byref(size))
        keep = _filter(km, size.value, o)  # on the possibly shrunk SizeInKmer (dna.go:263-266)
        if keep == 0:
            continue
        out.append({"Query": {"Sequence": aa[trimmed:].decode("latin-1"), "Name": names[int(m["src_seq"])],
                              "SizeInKmer": size.value, "Type": DNA_QUERY,
                              "Location": {"StartPosition": start.value, "EndPosition": int(m["end_position"]),
                                           "PlusStrand": bool(m["plus_strand"]), "StartsAlternative": []},
                              "Contig": ""},
                    "SearchResults": {"Hits": [{"Key": int(p), "Kmatch": int(k)} for p, k in zip(pid[:keep], km[:keep])]}})
    return out


def FastqSearch(index, fastq_text, options=None):
    """search_fastq.go:27-154 (READS) -> list of QueryResult dicts, one per reported ORF"""
    o = options or SearchOptions(SequenceType=abi.READS)
    recs = api.parse_reads(fastq_text, "fastq")
    return _orf_results(index, [r["seq"] for r in recs], [r["name"] for r in recs], o, abi.seq_type(abi.READS, o.GeneticCode))


def NucleotideSearch(index, fasta_text, options=None):
    """search_nucleotide.go:27-160 (contigs in FASTA) -> list of QueryResult dicts"""
    o = options or SearchOptions(SequenceType=abi.NUCLEOTIDE)
    recs = api.parse_reads(fasta_text, "fasta")
    out = _orf_results(index, [r["seq"] for r in recs], [r["name"] for r in recs], o, abi.seq_type(abi.NUCLEOTIDE, o.GeneticCode))
    for qr in out:
        qr["Query"]["Contig"] = qr["Query"]["Name"]  # search.go:305-306
    return out


def _chunk_results(top, recs, o, seq_type, proteins, aligned):
    """the QueryResult dicts of one chunk's TopResult, shaped as ProteinSearch / _orf_results shape theirs; recs: the
    chunk's records (seq, name, size, plus).  PositionHits, when the block carries bitmaps, are those of the reported hits:
    what the reference prints (search.go:520-522,540-543,591-594); for an ORF over the SizeInKmer as searched."""
    out = []
    for i in range(top.n_reported):
        a, b = int(top.top_off[i]), int(top.top_off[i + 1])
        if seq_type == abi.PROTEIN:
            q = recs[int(top.rep_query[i])]
            query = {"Sequence": q["seq"], "Name": q["name"], "SizeInKmer": q["size"], "Type": PROTEIN_QUERY,
                     "Location": {"StartPosition": 1, "EndPosition": len(q["seq"]), "PlusStrand": q["plus"], "StartsAlternative": []},
                     "Contig": ""}
        else:
            m = top.meta[i]
            aa = bytes(top.orf_aa[int(m["aa_off"]):int(m["aa_off"]) + int(m["aa_len"])])  # already trimmed
            name = recs[int(m["src_seq"])]["name"]
            query = {"Sequence": aa.decode("latin-1"), "Name": name, "SizeInKmer": int(m["size_in_kmer"]), "Type": DNA_QUERY,
                     "Location": {"StartPosition": int(m["start_position"]), "EndPosition": int(m["end_position"]),
                                  "PlusStrand": bool(m["plus_strand"]), "StartsAlternative": []},
                     "Contig": name if seq_type == abi.NUCLEOTIDE else ""}  # search.go:305-306
        qr = {"Query": query,
              "SearchResults": {"Hits": [{"Key": int(p), "Kmatch": int(k)} for p, k in zip(top.top_pid[a:b], top.top_kmatch[a:b])]}}
        if top.pos_bits is not None:
            qr["SearchResults"]["PositionHits"] = {p: bits.tolist() for p, bits in top.positions(i).items()}
        if aligned:
            _with_alignments(qr, top, i, proteins)
        out.append(qr)
    return out


class _ConsumerGone(Exception):
    """SearchFile's generator was closed before the file ended"""


_FASTA_SPACE = b" \t\n\v\f\r"


def _fasta_span_seq(text, s, upper):
    """the sequence of a FASTA record from its span: the range's lines, '\\r' dropped, trimmed and joined (the reader's rules)"""
    rng = text[int(s["seq_off"]):int(s["seq_off"]) + int(s["seq_len"])]
    seq = b"".join(ln.strip(_FASTA_SPACE) for ln in rng.split(b"\n"))
    return (seq.upper() if upper else seq).decode("latin-1")   # (bytes.upper: a-z only, as the reader)


def SearchFile(handle, path, options=None, fmt=None, device_parse=False, device_inflate=False, device_fasta=False):
    """FastqSearch / ProteinSearch / NucleotideSearch (search_fastq.go:60-136, search_protein.go:40-118,
    search_nucleotide.go:27-160) over a FILE of any size (gzip included) on an api.Replicas set or an api.ShardedIndex: a
    generator of QueryResult dicts in file order, shaped as the text drivers above shape theirs (options.SequenceType
    picks which; fmt: "fastq" / "fasta", default by SequenceType).  The file goes through kaamer_search_file_opts /
    kaamer_sharded_search_file on a worker thread, a chunk at a time (options.ChunkSeqs records, default 1 << 20); at most
    two converted chunks wait for the consumer.  ExtractPositions: PositionHits of the reported hits, from the block's
    bitmaps.  Align with a table attached to the handle: HitEntries and every hit's Alignment, hits in BitScore order.
    device_parse=True (FASTQ on an api.Replicas set, no ExtractPositions, no Align; anything else: ValueError): the file's
    text is parsed on the device (kaamer_search_text_file, options.ChunkTextBytes of text per chunk) and the names are
    sliced out of each chunk's text by span; the same dicts come out.  device_inflate=True (with device_parse only: else
    ValueError): a BGZF file is also inflated on the device (kaamer_search_text_file_opts); whatever else a gzip file holds
    falls back to the host inflater, the results are the same.
    device_fasta=True (FASTA on an api.Replicas set, any of the three sequence types, no ExtractPositions, no Align;
    anything else: ValueError): the file's FASTA text is parsed on the device (kaamer_search_fasta_file); names -- and for
    PROTEIN the sequences -- are taken out of each chunk's text by span; the same dicts come out."""
    o = options or SearchOptions(SequenceType=abi.READS)
    seq_type = o.SequenceType
    if device_fasta:
        why = None
        if device_parse or device_inflate:
            why = "device_parse / device_inflate are the FASTQ route"
        elif fmt not in (None, "fasta"):
            why = "the file must be FASTA"
        elif seq_type not in (abi.READS, abi.NUCLEOTIDE, abi.PROTEIN):
            why = "unknown SequenceType"
        elif o.ExtractPositions or o.Align:
            why = "ExtractPositions and Align go through the host reader"
        elif not hasattr(handle, "search_fasta_file"):
            why = "the handle has no FASTA text driver (an api.Replicas set has)"
        if why:
            raise ValueError("SearchFile(device_fasta=True): " + why)
        fmt = "fasta"
    fmt = fmt or ("fastq" if seq_type == abi.READS else "fasta")
    if device_inflate and not device_parse:
        raise ValueError("SearchFile(device_inflate=True) needs device_parse=True: the device inflates into the device reader's text buffer")
    if device_parse:
        why = None
        if fmt != "fastq":
            why = "only FASTQ is parsed on the device"
        elif seq_type not in (abi.READS, abi.NUCLEOTIDE):
            why = "FASTQ text is READS or NUCLEOTIDE input"
        elif o.ExtractPositions or o.Align:
            why = "ExtractPositions and Align go through the host reader"
        elif not hasattr(handle, "search_text_file"):
            why = "the handle has no text driver (an api.Replicas set has)"
        if why:
            raise ValueError("SearchFile(device_parse=True): " + why)
    aln = _one_call(handle, o)
    done, stop = object(), threading.Event()
    q = queue.Queue(maxsize=2)

    def put(item):
        while not stop.is_set():
            try:
                q.put(item, timeout=0.1)
                return
            except queue.Full:
                pass
        raise _ConsumerGone()

    def on_chunk(first, reads_h, top):
        seqs, offs, size, names, noff, plus = api._reads_to_arrays(reads_h)
        sb = bytes(seqs)
        recs = [dict(seq=sb[int(offs[i]):int(offs[i + 1])].decode("latin-1"), name=names[int(noff[i]):int(noff[i + 1])].decode("latin-1"),
                     size=int(size[i]), plus=bool(plus[i])) for i in range(len(size))]
        put(_chunk_results(top, recs, o, seq_type, getattr(handle, "proteins", None), aln is not None))

    def on_text_chunk(first, text, top):
        sp = top.text_spans   # names are sliced out of the chunk's text; nothing else of a record is reported for reads
        recs = [dict(name=text[int(s["name_off"]):int(s["name_off"]) + int(s["name_len"])].decode("latin-1")) for s in sp]
        put(_chunk_results(top, recs, o, seq_type, None, False))

    held = []   # device_fasta: the chunk that may hold the file's last record waits for its successor or the file's end

    def fasta_chunk_out(first, text, top, last):
        sp = top.text_spans
        n = len(sp)
        if seq_type == abi.PROTEIN:   # the reported queries carry their own sequence (search_protein.go)
            recs = [None] * n
            for i in set(int(x) for x in top.rep_query):
                s = sp[i]
                # the reader's case rule: only the record still pending at the end of the input keeps its case -- a last
                # record with a header line behind it was closed by that header and is upper-cased like the others
                end = int(s["seq_off"]) + int(s["seq_len"])
                pending = last and i == n - 1 and b"\n>" not in text[end:]
                seq = _fasta_span_seq(text, s, not pending)
                recs[i] = dict(seq=seq, name=text[int(s["name_off"]):int(s["name_off"]) + int(s["name_len"])].decode("latin-1"),
                               size=len(seq) - 6 - (1 if seq.endswith("*") else 0), plus=first == 0 and i == 0)
        else:
            recs = [dict(name=text[int(s["name_off"]):int(s["name_off"]) + int(s["name_len"])].decode("latin-1")) for s in sp]
        put(_chunk_results(top, recs, o, seq_type, None, False))

    def on_fasta_chunk(first, text, top):
        if held:
            fasta_chunk_out(*held.pop(), False)
        held.append((first, text, top))

    def work():
        try:
            if device_fasta:
                handle.search_fasta_file(path, seq_type=abi.seq_type(seq_type, getattr(o, "GeneticCode", 0)), min_k_ratio=o.MinKRatio,
                                         min_k_match=o.MinKMatch, max_results=o.MaxResults,
                                         chunk_text_bytes=int(getattr(o, "ChunkTextBytes", 1 << 28)), in_flight=int(getattr(o, "InFlight", 0)),
                                         on_chunk=on_fasta_chunk)
                if held:
                    fasta_chunk_out(*held.pop(), True)
                put(done)
                return
            if device_parse:
                handle.search_text_file(path, fmt, seq_type=abi.seq_type(seq_type, getattr(o, "GeneticCode", 0)), min_k_ratio=o.MinKRatio,
                                        min_k_match=o.MinKMatch, max_results=o.MaxResults,
                                        chunk_text_bytes=int(getattr(o, "ChunkTextBytes", 1 << 28)), in_flight=int(getattr(o, "InFlight", 0)),
                                        on_chunk=on_text_chunk, **({"device_inflate": True} if device_inflate else {}))
                put(done)
                return
            handle.search_file(path, fmt, seq_type=abi.seq_type(seq_type, getattr(o, "GeneticCode", 0)), min_k_ratio=o.MinKRatio, min_k_match=o.MinKMatch, max_results=o.MaxResults,
                               chunk_seqs=int(getattr(o, "ChunkSeqs", 1 << 20)), in_flight=int(getattr(o, "InFlight", 0)), on_chunk=on_chunk,
                               want_positions=bool(o.ExtractPositions), align=aln)
            put(done)
        except BaseException as e:  # noqa: BLE001  (handed to the consumer)
            if not stop.is_set():
                try:
                    put(e)
                except _ConsumerGone:
                    pass

    th = threading.Thread(target=work, daemon=True)
    th.start()
    try:
        while True:
            item = q.get()
            if item is done:
                return
            if isinstance(item, BaseException):
                raise item
            yield from item
    finally:
        stop.set()   # (a consumer that leaves early: the callback stops the run at the next chunk)
        th.join()


def TextSearchTsv(index, text, options=None, fmt="fastq", proteins=None):
    """The whole TSV response body of a request whose input is text (SetResponseFormatAndHeader + QueryResultHandler,
    search.go:636-662,505-554, OutFormat "tsv" without Align): the header line, then one row per reported hit, written on the
    device in the same call that parses and searches the text (Index.search_text_top / search_fasta_top / search_bgzf_top
    with tsv=...; needs Index.attach_subject_text).  fmt: "fastq", "fasta" or "bgzf" (whole BGZF blocks of FASTQ).
    proteins: the table, for the feature names of the header (default: index.proteins); needed with Annotations."""
    o = options or SearchOptions(SequenceType=abi.READS)
    proteins = proteins if proteins is not None else getattr(index, "proteins", None)
    if o.Annotations and proteins is None:
        raise ValueError("Annotations: the header needs the table's feature names (proteins=...)")
    base = abi.seq_type_base(o.SequenceType)
    st = abi.seq_type(base, o.GeneticCode) if base != abi.PROTEIN else abi.PROTEIN
    kw = dict(seq_type=st, min_k_ratio=o.MinKRatio, min_k_match=o.MinKMatch, max_results=o.MaxResults,
              tsv=dict(positions=o.ExtractPositions, annotations=o.Annotations))
    if o.Align:   # the -aln form (search.go:556-604): the hits aligned in the same call (needs Index.attach_proteins too)
        kw["align"] = dict(sub_matrix=o.SubMatrix, gap_open=o.GapOpen, gap_extend=o.GapExtend)
    if fmt == "fastq":
        top = index.search_text_top(text, **kw)
    elif fmt == "fasta":
        top = index.search_fasta_top(text, **kw)
    elif fmt == "bgzf":
        top = index.search_bgzf_top(text, **kw)
    else:
        raise ValueError("fmt is 'fastq', 'fasta' or 'bgzf'")
    return api.format_tsv_header(o.ExtractPositions, o.Annotations, proteins, align=bool(o.Align)) + top.tsv


def TextSearchJson(index, text, options=None, fmt="fastq", proteins=None):
    """The whole JSON response body of a request whose input is text (SetResponseFormatAndHeader, search.go:672-688; one
    json.Marshal(QueryResult) per reported query, search.go:497-503; the closing bytes, search.go:629-632), OutFormat "json"
    without Align: the objects are written on the device in the same call that parses and searches the text
    (Index.search_text_top / search_fasta_top / search_bgzf_top with json=...; needs Index.attach_subject_json).  fmt:
    "fastq", "fasta" or "bgzf".  proteins: the table, for the feature names of the header (default: index.proteins); needed
    with Annotations."""
    o = options or SearchOptions(SequenceType=abi.READS)
    if o.Align:
        raise ValueError("-aln JSON is not written")
    proteins = proteins if proteins is not None else getattr(index, "proteins", None)
    if o.Annotations and proteins is None:
        raise ValueError("Annotations: the header needs the table's feature names (proteins=...)")
    base = abi.seq_type_base(o.SequenceType)
    st = abi.seq_type(base, o.GeneticCode) if base != abi.PROTEIN else abi.PROTEIN
    kw = dict(seq_type=st, min_k_ratio=o.MinKRatio, min_k_match=o.MinKMatch, max_results=o.MaxResults, json=dict(positions=o.ExtractPositions))
    if fmt == "fastq":
        top = index.search_text_top(text, **kw)
    elif fmt == "fasta":
        top = index.search_fasta_top(text, **kw)
    elif fmt == "bgzf":
        top = index.search_bgzf_top(text, **kw)
    else:
        raise ValueError("fmt is 'fastq', 'fasta' or 'bgzf'")
    return api.format_json_header(o.Annotations, proteins) + top.json + api.format_json_trailer()


def FetchHitsInformation(query_results, proteins):
    """search.go:454-470 for a list of QueryResult dicts: HitEntries[Key] = the Protein entry (protein.proto:
    EntryId, Sequence, Length, Features) of every reported hit, from the protein table makedb built
    (api.Proteins: kaamer_fetch_hits) instead of one ProteinStore point read per hit.  Like the reference, a
    query's loop stops at the first id that has no entry."""
    keys = sorted({h["Key"] for qr in query_results for h in qr["SearchResults"]["Hits"]})
    entries = dict(zip(keys, proteins.fetch_hits(keys))) if keys else {}
    for qr in query_results:
        he = qr.setdefault("HitEntries", {})
        for h in qr["SearchResults"]["Hits"]:
            if h["Key"] in he:
                continue
            e = entries.get(h["Key"])
            if e is None:
                break                      # search.go:461-463: return on the first failed read
            he[h["Key"]] = {"EntryId": e["EntryId"].decode("latin-1"), "Sequence": e["Sequence"].decode("latin-1"),
                            "Length": e["Length"],
                            "Features": {k.decode("latin-1"): v.decode("latin-1") for k, v in e["Features"].items()}}
    return query_results


def AlignHits(query_results, proteins, opts, device=0):
    """The alignment step of QueryResultHandler (search.go:483-494) for a list of QueryResult dicts that went through
    FetchHitsInformation: align.Align(Query.Sequence, HitEntries[hit.Key].Sequence, dbStats, SubMatrix, GapOpen,
    GapExtend) for every reported hit -- all pairs of the batch in ONE device call (kaamer_align_pairs) -- then the hits
    of each query re-sorted by BitScore, descending.  A pair for which Align returns an error ("No matrix found") keeps
    the empty AlignmentResult sortMapByValue gave it (search.go:144)."""
    seqs, index, pairs, where = [], {}, [], []

    def seq_id(s):
        if s not in index:
            index[s] = len(seqs)
            seqs.append(s)
        return index[s]
    for qi, qr in enumerate(query_results):
        q = qr["Query"]["Sequence"].encode("latin-1")
        for hi, h in enumerate(qr["SearchResults"]["Hits"]):
            e = qr.get("HitEntries", {}).get(h["Key"])
            if e is None:
                continue
            pairs.append((seq_id(q), seq_id(e["Sequence"].encode("latin-1"))))
            where.append((qi, hi))
    empty = {"Identity": 0.0, "Similarity": 0.0, "Length": 0, "Mismatches": 0, "GapOpenings": 0, "Raw": 0, "BitScore": 0.0,
             "EValue": 0.0, "AlnString": "", "QueryStart": 0, "QueryEnd": 0, "SubjectStart": 0, "SubjectEnd": 0}
    for qr in query_results:
        for h in qr["SearchResults"]["Hits"]:
            h["Alignment"] = dict(empty)
    if pairs:
        n_aa = proteins.stats()["NumberOfAA"]   # KStats.NumberOfAA (kvstore.KStats)
        got = api.align_pairs(seqs=seqs, pairs=pairs, number_of_aa=n_aa, sub_matrix=getattr(opts, "SubMatrix", "blosum62"),
                              gap_open=getattr(opts, "GapOpen", 11), gap_extend=getattr(opts, "GapExtend", 1), device=device)
        for (qi, hi), a in zip(where, got):
            if a is None or a.get("status"):
                continue
            query_results[qi]["SearchResults"]["Hits"][hi]["Alignment"] = {
                "Identity": a["identity"], "Similarity": a["similarity"], "Length": a["length"], "Mismatches": a["mismatches"],
                "GapOpenings": a["gap_openings"], "Raw": a["raw"], "BitScore": a["bitscore"], "EValue": a["evalue"],
                "AlnString": "\n".join(a["aln"]), "QueryStart": a["query_start"], "QueryEnd": a["query_end"],
                "SubjectStart": a["subject_start"], "SubjectEnd": a["subject_end"]}
    for qr in query_results:   # sort.Slice by BitScore descending (search.go:492-494; ties keep their order here)
        qr["SearchResults"]["Hits"].sort(key=lambda h: -h["Alignment"]["BitScore"])
    return query_results
