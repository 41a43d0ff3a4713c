"""Shared inputs of the tests that run the three response writers next to each other (test_gpu_attach_orders.py,
test_gpu_mixed_formats.py): tsvcases.standard_table(), the same table without its last entry, 16 protein queries as FASTA
that report that entry, and the text call of every format checked against the host formatter.  Test infrastructure."""
import tsvcases
from kaamer_amd import abi, api

KW = dict(min_k_ratio=0.0, min_k_match=1, max_results=10)
ALIGN = dict(sub_matrix="blosum62", gap_open=11, gap_extend=1)
TSV = dict(positions=True, annotations=True)
JSON = dict(positions=True)
FORMATS = ("plain", "tsv", "align+tsv", "json")
LAST = tsvcases.N_ENTRIES - 1        # the id short_table() lacks
_AA = b"ACDEFGHIKLMNPQRSTVWY"       # (the sequences of tsvcases.make_table are prefixes of its repetition)


def short_table(full):
    """standard_table() without its last entry: the ids stay, id LAST has no entry"""
    offs = full.packed[1]
    n = tsvcases.N_ENTRIES - 1
    id_lens = [max(v, 1) for v in tsvcases.LENS] + [3, 5]
    value_lens = [(tsvcases.LENS[i], tsvcases.LENS[(i + 3) % 11], tsvcases.LENS[(i + 7) % 11]) for i in range(11)] + [(0, 0, 0), (1000, 0, 2)]
    short = tsvcases.make_table(id_lens[:n], value_lens[:n], [int(offs[i + 1] - offs[i]) for i in range(n)])
    assert len(full) == n + 1 and short.ids.tolist() == full.ids.tolist()[:n]
    return short


def queries(n=16, seed=0):
    """-> (FASTA text, the sequences): windows of the table's residue cycle, so that every query reports ten entries, the
    20-residue entry LAST among them; names with and without a space"""
    seqs = [(_AA * 4)[(seed + 3 * i) % 20:(seed + 3 * i) % 20 + 27 + i] for i in range(n)]
    names = [(b"q%d_%d" % (seed, i)) + (b" rest %d" % i if i % 3 else b"") for i in range(n)]
    return b"".join(b">" + nm + b"\n" + s + b"\n" for nm, s in zip(names, seqs)), seqs


def call(ix, fmt, text):
    kw = dict(KW)
    if fmt in ("tsv", "align+tsv"):
        kw["tsv"] = TSV
    if fmt == "align+tsv":
        kw["align"] = ALIGN
    if fmt == "json":
        kw["json"] = JSON
    return ix.search_fasta_top(text, seq_type=abi.PROTEIN, **kw)


def check(got, fmt, text, seqs, table):
    """the result of call(): its device bytes equal the host formatter on `table`, the table the format's attach holds; each
    of kaamer_batch_top_tsv / _json gives nothing for the other format's result"""
    assert got.n_reported == len(seqs) and int(got.top_off[-1]) == 10 * len(seqs)
    if fmt == "plain":
        assert got.tsv is None and got.json is None
    elif fmt == "json":
        packed = api.pack_sequences(seqs)
        host, host_off = api.format_json(got, text, got.text_spans, table, seqs=packed[0], offsets=packed[1], seq_type=abi.PROTEIN, text_format=0,
                                         positions=JSON["positions"])
        assert got.json == host and got.json_obj_off.tolist() == host_off.tolist()
        assert got.tsv is None and got.tsv_line_off is None
    else:
        host, host_off = api.format_tsv(got, text, got.text_spans, table, TSV["positions"], TSV["annotations"], align=fmt == "align+tsv",
                                        seq_type=abi.PROTEIN)
        assert got.tsv == host and got.tsv_line_off.tolist() == host_off.tolist()
        assert got.json is None and got.json_obj_off is None
    return got
