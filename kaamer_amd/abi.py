"""ctypes binding of libkaamer_hip.so — one Python declaration per symbol of
include/kaamer_hip.h.  Loading fails loudly if the library has not been built
(`python -m kaamer_amd.build`); there is no fallback implementation.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# KAAMER_LIB points at an alternative build of the same library (tuning experiments only)
LIB_PATH = os.environ.get("KAAMER_LIB") or os.path.join(_HERE, "libkaamer_hip.so")

OK, E_ARG, E_IO, E_NOMEM, E_HIP, E_CAPACITY, E_FORMAT, E_BUSY, E_RANGE = 0, -1, -2, -3, -4, -5, -6, -7, -8
NUCLEOTIDE, PROTEIN, READS = 0, 1, 2
GENETIC_CODES = (1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14, 15)   # the keys of search.GCodes (gcode.go:21-34)


def seq_type(base, genetic_code=0):
    """KAAMER_SEQ_TYPE: the value every `seq_type` argument takes -- the sequence type in bits 0-7, the request's genetic
    code in bits 8-15 (0: the reference's behaviour, table 11).  The library checks the code."""
    return int(base) | (int(genetic_code) << 8)


def seq_type_base(seq_type):
    """KAAMER_SEQ_TYPE_BASE: NUCLEOTIDE / PROTEIN / READS"""
    return int(seq_type) & 0xFF


def seq_type_genetic_code(seq_type):
    """KAAMER_SEQ_TYPE_GENETIC_CODE"""
    return (int(seq_type) >> 8) & 0xFF


def split_seq_type(seq_type):
    return seq_type_base(seq_type), seq_type_genetic_code(seq_type)


def genetic_code(code=0):
    """kaamer_genetic_code: the library's table, codons in t-c-a-g order -> (amino-acid letters, 'M' / '-' start letters)"""
    aa, start = C.create_string_buffer(64), C.create_string_buffer(64)
    check(lib().kaamer_genetic_code(int(code), aa, start))
    return aa.raw.decode("ascii"), start.raw.decode("ascii")


class KaamerError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("kaamer_hip error %d: %s" % (code, msg))
        self.code = code


class Pair(C.Structure):
    _fields_ = [("key", C.c_uint32), ("protein_id", C.c_uint32)]


class ImageStats(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64), ("n_keys", C.c_uint64), ("n_buckets", C.c_uint64),
                ("arena_words", C.c_uint64), ("n_inline", C.c_uint64), ("n_lists", C.c_uint64),
                ("max_list", C.c_uint64), ("n_displaced", C.c_uint64), ("shard", C.c_uint32),
                ("n_shards", C.c_uint32), ("max_protein_id", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


class QueryMeta(C.Structure):
    _fields_ = [("src_seq", C.c_uint32), ("size_in_kmer", C.c_int32), ("start_position", C.c_int32),
                ("end_position", C.c_int32), ("plus_strand", C.c_int32), ("aa_len", C.c_uint32),
                ("aa_off", C.c_uint64), ("sa_off", C.c_uint32), ("sa_len", C.c_uint32)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_in", "n_queries", "n_lookup", "n_probe", "n_found",
                                          "n_post", "n_hits", "n_overflow", "n_lists", "n_list_ids")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class BatchIn(C.Structure):
    _fields_ = [("seqs", C.c_void_p), ("offsets", C.c_void_p), ("n_seqs", C.c_uint32),
                ("seq_type", C.c_int32), ("want_positions", C.c_int32)]


class BatchOut(C.Structure):
    _fields_ = [("n_queries", C.c_uint32), ("q", C.POINTER(QueryMeta)),
                ("hit_off", C.POINTER(C.c_uint64)), ("hit_cnt", C.POINTER(C.c_uint32)), ("hit_pid", C.POINTER(C.c_uint32)),
                ("hit_kmatch", C.POINTER(C.c_uint32)), ("hit_first_pos", C.POINTER(C.c_uint32)),
                ("pos_off", C.POINTER(C.c_uint64)), ("pos_bits", C.POINTER(C.c_uint64)),
                ("orf_aa", C.POINTER(C.c_uint8)), ("starts_alt", C.POINTER(C.c_int32)),
                ("counters", Counters)]


class WorkspaceOpts(C.Structure):
    _fields_ = [("max_seq_bytes", C.c_uint64), ("max_seqs", C.c_uint32), ("max_queries", C.c_uint32),
                ("max_hits", C.c_uint64),
                ("g_tier_slots", C.c_uint64), ("seq_type", C.c_int32), ("first_pos", C.c_uint32), ("want_positions", C.c_uint32),
                ("compact", C.c_uint32), ("max_pos_words", C.c_uint64), ("concurrent_batches", C.c_uint32), ("reserved", C.c_uint32)]


class DeviceResult(C.Structure):
    _fields_ = [("n_queries_cap", C.c_uint32), ("d_n_queries", C.c_void_p), ("d_q", C.c_void_p),
                ("d_hit_off", C.c_void_p), ("d_hit_cnt", C.c_void_p), ("hit_capacity", C.c_uint64), ("d_hit_pid", C.c_void_p),
                ("d_hit_kmatch", C.c_void_p),
                ("d_hit_first_pos", C.c_void_p), ("d_orf_aa", C.c_void_p), ("d_starts_alt", C.c_void_p),
                ("d_counters", C.c_void_p), ("d_pos_off", C.c_void_p), ("d_pos_bits", C.c_void_p),
                ("d_pos_base", C.c_void_p)]


class TopnOpts(C.Structure):
    _fields_ = [("min_k_ratio", C.c_double), ("min_k_match", C.c_int64), ("max_results", C.c_uint32),
                ("best_start_codon", C.c_uint32), ("d_size_in_kmer", C.c_void_p),
                ("orf_source", C.c_void_p), ("q_first", C.c_uint32), ("q_stride", C.c_uint32)]


class ExchangeLayout(C.Structure):
    _fields_ = [("world", C.c_uint32), ("rank", C.c_uint32), ("q_cap", C.c_uint32), ("arrays", C.c_uint32),
                ("e_cap", C.c_uint64), ("block_words", C.c_uint64)]


class BatchTop(C.Structure):
    _fields_ = [("n_queries", C.c_uint32), ("n_reported", C.c_uint32), ("max_results", C.c_uint32),
                ("rep_query", C.POINTER(C.c_uint32)), ("q", C.POINTER(QueryMeta)), ("trim", C.POINTER(C.c_int32)),
                ("top_off", C.POINTER(C.c_uint64)), ("top_pid", C.POINTER(C.c_uint32)),
                ("top_kmatch", C.POINTER(C.c_uint32)), ("top_first_pos", C.POINTER(C.c_uint32)),
                ("orf_aa", C.POINTER(C.c_uint8)), ("counters", Counters)]


class ProteinEntry(C.Structure):
    _fields_ = [("found", C.c_uint32), ("length", C.c_uint32), ("entry_id", C.c_void_p), ("entry_id_len", C.c_uint32),
                ("n_features", C.c_uint32), ("sequence", C.c_void_p), ("features", C.c_void_p), ("feature_off", C.POINTER(C.c_uint64)),
                ("sequence_len", C.c_uint32), ("reserved", C.c_uint32)]


class Alignment(C.Structure):
    _fields_ = [("identity", C.c_float), ("similarity", C.c_float), ("length", C.c_int32), ("mismatches", C.c_int32),
                ("gap_openings", C.c_int32), ("raw", C.c_int32), ("bitscore", C.c_double), ("evalue", C.c_double),
                ("query_start", C.c_int32), ("query_end", C.c_int32), ("subject_start", C.c_int32), ("subject_end", C.c_int32),
                ("aln_off", C.c_uint64), ("status", C.c_int32), ("reserved", C.c_int32)]


class AlignPair(C.Structure):   # kaamer_align_pair: one (query, reported hit) pair as the device leaves it
    _fields_ = [("status", C.c_int32), ("n_ops", C.c_int32), ("start_i", C.c_int32), ("start_j", C.c_int32), ("end_i", C.c_int32),
                ("end_j", C.c_int32), ("identical", C.c_int32), ("similar", C.c_int32), ("mismatches", C.c_int32),
                ("gap_openings", C.c_int32), ("raw", C.c_int32), ("query_len", C.c_uint32), ("off", C.c_uint64),
                ("entry", C.c_uint32), ("subject_len", C.c_uint32)]


class TopnAlignOpts(C.Structure):
    _fields_ = [("sub_matrix", C.c_char * 16), ("gap_open", C.c_int32), ("gap_extend", C.c_int32), ("max_query_len", C.c_uint32),
                ("reserved", C.c_uint32), ("max_pairs", C.c_uint64)]


class TopnAlignments(C.Structure):
    _fields_ = [("d_pair_off", C.c_void_p), ("d_pairs", C.c_void_p), ("pair_capacity", C.c_uint64), ("n_waves", C.c_uint32),
                ("n_long_waves", C.c_uint32), ("slab_bytes", C.c_uint64)]


class TopnResult(C.Structure):
    _fields_ = [("max_results", C.c_uint32), ("d_top_cnt", C.c_void_p), ("d_top_pid", C.c_void_p),
                ("d_top_kmatch", C.c_void_p), ("d_top_first_pos", C.c_void_p), ("d_trim", C.c_void_p),
                ("d_start_position", C.c_void_p), ("d_size_in_kmer", C.c_void_p)]


class TopnPositions(C.Structure):
    _fields_ = [("d_pos_base", C.c_void_p), ("d_pos_bits_len", C.c_void_p), ("d_pos_bits", C.c_void_p),
                ("pos_words_capacity", C.c_uint64)]


class TextSpan(C.Structure):   # kaamer_text_span: name and sequence of one record, as offsets into the text
    _fields_ = [("name_off", C.c_uint32), ("name_len", C.c_uint32), ("seq_off", C.c_uint32), ("seq_len", C.c_uint32)]


class TextParseResult(C.Structure):
    _fields_ = [("n_records", C.c_uint32), ("reserved", C.c_uint32), ("n_lines", C.c_uint64), ("seq_bytes", C.c_uint64),
                ("d_seqs", C.c_void_p), ("d_offsets", C.c_void_p), ("d_spans", C.c_void_p)]


class InflateResult(C.Structure):   # kaamer_inflate_result
    _fields_ = [("n_bad", C.c_uint32), ("first_bad", C.c_uint32), ("out_bytes", C.c_uint64), ("first_bad_status", C.c_uint32),
                ("reserved", C.c_uint32), ("d_status", C.c_void_p)]


class TsvRowsIn(C.Structure):   # kaamer_tsv_rows_in
    _fields_ = [("top", TopnResult), ("d_q", C.c_void_p), ("d_n_queries", C.c_void_p), ("n_queries_cap", C.c_uint32),
                ("n_names", C.c_uint32), ("d_name_bytes", C.c_void_p), ("name_bytes_len", C.c_uint64), ("d_spans", C.c_void_p),
                ("pos", C.POINTER(TopnPositions)), ("extract_positions", C.c_int32), ("annotations", C.c_int32)]


class TsvRowsResult(C.Structure):   # kaamer_tsv_rows_result
    _fields_ = [("d_line_off", C.c_void_p), ("d_counts", C.c_void_p), ("line_off_capacity", C.c_uint64)]


class JsonRowsIn(C.Structure):   # kaamer_json_rows_in
    _fields_ = [("rows", TsvRowsIn), ("d_aa", C.c_void_p), ("aa_len", C.c_uint64), ("seq_type", C.c_int32), ("text_format", C.c_int32)]


class JsonRowsResult(C.Structure):   # kaamer_json_rows_result
    _fields_ = [("d_obj_off", C.c_void_p), ("d_counts", C.c_void_p), ("obj_off_capacity", C.c_uint64)]


class TsvAlnOpts(C.Structure):   # kaamer_tsv_aln_opts
    _fields_ = [("sub_matrix", C.c_char * 16), ("gap_open", C.c_int32), ("gap_extend", C.c_int32), ("seq_type", C.c_int32),
                ("reserved", C.c_int32)]


# The argument groups that recur in the prototypes below, each named once
HANDLE = [C.c_void_p]                                   # an index, a sharded index, a replica set, a stream, a ticket, a stage
BATCH = [C.c_void_p, C.c_void_p, C.c_uint32]            # the packed batch: (seqs, offsets, n_seqs)
SEQ_TYPE = [C.c_int32]                                  # seq_type()
TOP = [C.c_double, C.c_int64, C.c_uint32]               # the top options: (min_k_ratio, min_k_match, max_results)
ALIGN = [C.c_int32, C.c_char_p, C.c_int32, C.c_int32, C.c_int32]   # (want_positions, sub_matrix, gap_open, gap_extend, want_text)
ALIGN_TEXT = ALIGN[1:4]                                 # ... of the text calls: (sub_matrix, gap_open, gap_extend)
ALIGN_FILE = ALIGN[:1] + [C.c_int32] + ALIGN[1:]        # ... of the file drivers: want_aln after want_positions
ROWS = [C.c_int32, C.c_int32]                           # the rows group: (extract_positions, annotations)
TEXT_IN = [C.c_char_p, C.c_uint64]                      # (text, len)
TEXT_HEAD = {"text": TEXT_IN + [C.c_int32] + SEQ_TYPE,  # (text, len, format, seq_type)
             "fasta": TEXT_IN + SEQ_TYPE + [C.c_int32],  # (text, len, seq_type, upper_last)
             "bgzf": TEXT_IN + SEQ_TYPE}                # (bytes, len, seq_type)
TEXT_TAIL = {"": [], "_tsv": ROWS, "_aln_tsv": ROWS + ALIGN_TEXT, "_json": ROWS[:1]}   # what a response format adds behind TOP
OUT = {"search": [C.c_void_p], "submit": [C.POINTER(C.c_void_p)]}   # the two `out` kinds: a kaamer_batch_top **, a ticket *
NEW = [C.POINTER(C.c_void_p)]                           # the handle a create / open / parse call makes
FULL_OUT = [C.POINTER(C.POINTER(BatchOut))]
FILE_IN = [C.c_char_p, C.c_int, C.c_int]                # (path, format, strict_scanner)
CHUNKS = [C.c_uint32, C.c_uint64, C.c_uint32]           # (chunk_seqs, chunk_bytes, in_flight)
TEXT_CHUNKS = [C.c_uint64, C.c_uint32]                  # (chunk_text_bytes, in_flight)
CB = [C.c_void_p, C.c_void_p, C.POINTER(Counters)]      # (cb, user, total)
INFO = (C.c_int, HANDLE + [C.POINTER(C.c_uint64)])      # an info getter: (handle, u64 out[])
ATTACH = (C.c_int, HANDLE + [C.c_void_p])               # (handle, proteins)

# every symbol include/kaamer_hip.h declares: name -> (restype, argtypes).  First the symbols that stand alone, then the
# families, built from the groups above
SYMBOLS = {
    "kaamer_last_error": (C.c_char_p, []),
    "kaamer_abi_version": (C.c_int, []),
    "kaamer_encode_kmer": (C.c_uint32, [C.c_char_p]),
    "kaamer_genetic_code": (C.c_int, [C.c_int32, C.c_char_p, C.c_char_p]),
    "kaamer_shard_of": (C.c_uint32, [C.c_uint32, C.c_uint32]),
    "kaamer_image_build_pairs": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_double] + NEW),
    # (seqs, offsets, ids, n_proteins, shard, n_shards, load_factor[, device], out)
    "kaamer_image_build_proteins": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double] + NEW),
    "kaamer_image_build_proteins_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double,
                                                     C.c_int] + NEW),
    "kaamer_index_build_proteins": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double,
                                              C.c_int] + NEW),
    "kaamer_image_save": (C.c_int, [C.c_void_p, C.c_char_p]),
    "kaamer_image_load": (C.c_int, [C.c_char_p] + NEW),
    "kaamer_image_get_stats": (C.c_int, [C.c_void_p, C.POINTER(ImageStats)]),
    "kaamer_image_free": (None, [C.c_void_p]),
    "kaamer_image_get": (C.c_uint32, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]),
    "kaamer_makedb_text": (C.c_int, TEXT_IN + [C.c_int32, C.c_int32] + NEW),
    "kaamer_proteins_count": (C.c_uint32, [C.c_void_p]),
    "kaamer_proteins_ids": (C.POINTER(C.c_uint32), [C.c_void_p]),
    "kaamer_proteins_seqs": (C.POINTER(C.c_uint8), [C.c_void_p]),
    "kaamer_proteins_offsets": (C.POINTER(C.c_uint64), [C.c_void_p]),
    "kaamer_proteins_n_features": (C.c_uint32, [C.c_void_p]),
    "kaamer_proteins_feature_name": (C.c_char_p, [C.c_void_p, C.c_uint32]),
    "kaamer_proteins_stats": (None, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "kaamer_proteins_save": (C.c_int, [C.c_void_p, C.c_char_p]),
    "kaamer_proteins_load": (C.c_int, [C.c_char_p] + NEW),
    "kaamer_proteins_free": (None, [C.c_void_p]),
    "kaamer_image_build_makedb": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_double] + NEW),
    "kaamer_image_build_makedb_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_double, C.c_int] + NEW),
    "kaamer_fetch_hits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(ProteinEntry)]),
    "kaamer_index_open_image": (C.c_int, [C.c_void_p, C.c_int] + NEW),
    "kaamer_index_open": (C.c_int, [C.c_char_p, C.c_int] + NEW),
    "kaamer_index_close": (None, [C.c_void_p]),
    "kaamer_index_get_stats": (C.c_int, [C.c_void_p, C.POINTER(ImageStats)]),
    "kaamer_batch_free": (None, [C.POINTER(BatchOut)]),
    "kaamer_batch_top_free": (None, [C.c_void_p]),
    "kaamer_workspace_create": (C.c_int, [C.c_void_p, C.POINTER(WorkspaceOpts)] + NEW),
    "kaamer_workspace_free": (None, [C.c_void_p]),
    "kaamer_workspace_set_count_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "kaamer_search_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                       C.c_uint64, C.c_int32, C.c_void_p, C.POINTER(DeviceResult)]),
    "kaamer_merge_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64,
                                      C.c_void_p, C.POINTER(DeviceResult)]),
    "kaamer_exchange_layout_init": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(ExchangeLayout)]),
    "kaamer_workspace_query_capacity": (C.c_uint32, [C.c_void_p]),
    "kaamer_scan_geometry": (None, [C.POINTER(C.c_uint32)]),
    "kaamer_exchange_layout_fit": (C.c_int, [C.POINTER(ExchangeLayout), C.c_uint32, C.c_uint64, C.c_int32, C.POINTER(ExchangeLayout)]),
    "kaamer_exchange_stats": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]),
    "kaamer_exchange_pack": (C.c_int, [C.c_void_p, C.POINTER(ExchangeLayout), C.c_void_p, C.c_void_p]),
    "kaamer_exchange_merge": (C.c_int, [C.c_void_p, C.POINTER(ExchangeLayout), C.c_void_p, C.c_void_p, C.POINTER(DeviceResult)]),
    "kaamer_rccl_alltoall": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]),
    "kaamer_workspace_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Counters)]),
    "kaamer_workspace_kernel_ms_sum": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                 C.POINTER(C.c_double), C.POINTER(C.c_uint32)]),
    "kaamer_topn_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kaamer_index_open_sharded": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_uint32] + NEW),
    "kaamer_index_open_sharded_images": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_uint32] + NEW),
    "kaamer_sharded_index_shards": (C.c_uint32, [C.c_void_p]),
    "kaamer_sharded_index_close": (None, [C.c_void_p]),
    "kaamer_stream_open": (C.c_int, HANDLE + SEQ_TYPE + [C.c_void_p] + NEW),   # the struct form: (index, seq_type, topn_opts, out)
    # the exchange blocks that carry bitmaps
    "kaamer_exchange_layout_init_positions": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64,
                                                        C.POINTER(ExchangeLayout)]),
    "kaamer_exchange_layout_fit_positions": (C.c_int, [C.POINTER(ExchangeLayout), C.c_uint32, C.c_uint64, C.c_uint64,
                                                       C.POINTER(ExchangeLayout)]),
    "kaamer_exchange_stats_positions": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]),
    "kaamer_workspace_reset_timers": (None, [C.c_void_p]),
    "kaamer_workspace_set_timing": (None, [C.c_void_p, C.c_uint32]),
    "kaamer_filter_results": (C.c_int64, [C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_int64, C.c_int64]),
    "kaamer_sort_hits": (None, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "kaamer_set_best_start_codon": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                                C.c_char_p, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "kaamer_reads_count": (C.c_uint32, [C.c_void_p]),
    "kaamer_reads_seqs": (C.POINTER(C.c_uint8), [C.c_void_p]),
    "kaamer_reads_offsets": (C.POINTER(C.c_uint64), [C.c_void_p]),
    "kaamer_reads_size_in_kmer": (C.POINTER(C.c_int32), [C.c_void_p]),
    "kaamer_reads_names": (C.POINTER(C.c_char), [C.c_void_p]),
    "kaamer_reads_name_offsets": (C.POINTER(C.c_uint64), [C.c_void_p]),
    "kaamer_reads_plus_strand": (C.POINTER(C.c_int32), [C.c_void_p]),
    "kaamer_reads_free": (None, [C.c_void_p]),
    "kaamer_index_open_replicas": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.c_uint32] + NEW),
    "kaamer_index_open_replicas_image": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_uint32] + NEW),
    "kaamer_replicas_count": (C.c_uint32, [C.c_void_p]),
    "kaamer_replicas_index": (C.c_void_p, [C.c_void_p, C.c_uint32]),
    "kaamer_replicas_close": (None, [C.c_void_p]),
    # (device, seqs, offsets, n_seqs, pair_query, pair_subject, n_pairs, number_of_aa, sub_matrix, gap_open, gap_extend, out)
    "kaamer_align_pairs": (C.c_int, [C.c_int] + BATCH + [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64] + ALIGN_TEXT + NEW),
    "kaamer_alignments_count": (C.c_uint32, [C.c_void_p]),
    "kaamer_alignments_items": (C.POINTER(Alignment), [C.c_void_p]),
    "kaamer_alignments_text": (C.POINTER(C.c_char), [C.c_void_p]),
    "kaamer_alignments_free": (None, [C.c_void_p]),
    "kaamer_align_matrix_scores": (C.c_int, [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "kaamer_align_matrix_entry": (C.c_int32, [C.c_int32, C.c_int32]),
    "kaamer_reader_open": (C.c_int, FILE_IN + NEW),
    "kaamer_reader_open_fd": (C.c_int, [C.c_int, C.c_int, C.c_int] + NEW),
    "kaamer_reader_next": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64] + NEW),
    "kaamer_reader_done": (C.c_int, [C.c_void_p]),
    "kaamer_reader_records": (C.c_uint64, [C.c_void_p]),
    "kaamer_reader_close": (None, [C.c_void_p]),
    # PositionHits bitmaps of the reported hits on the top-N calls
    "kaamer_topn_positions_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(TopnResult), C.c_uint64, C.c_void_p,
                                               C.POINTER(TopnPositions)]),
    "kaamer_batch_top_positions": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.POINTER(C.c_uint64)),
                                             C.POINTER(C.POINTER(C.c_uint64))]),
    "kaamer_index_set_top_positions_bound": (C.c_int, [C.c_void_p, C.c_uint64]),
    "kaamer_format_positions": (C.c_uint64, [C.c_void_p, C.c_int32, C.c_int32, C.c_char_p, C.c_uint64]),
    # the alignment of the reported hits inside the top-N call
    "kaamer_index_set_align_budget": (C.c_int, [C.c_void_p, C.c_uint64]),
    "kaamer_sharded_index_set_align_budget": (C.c_int, [C.c_void_p, C.c_uint64]),
    "kaamer_sharded_index_set_align_timing": (C.c_int, [C.c_void_p, C.c_int32]),
    "kaamer_topn_align_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(TopnResult), C.POINTER(TopnAlignOpts), C.c_void_p,
                                           C.POINTER(TopnAlignments)]),
    "kaamer_batch_top_alignments": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(Alignment)), C.POINTER(C.POINTER(C.c_char))]),
    "kaamer_align_finish_pairs": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64] + ALIGN_TEXT + [C.c_void_p]),
    # the whole-file driver: (handle, path, format, strict_scanner, seq_type, min_k_ratio, min_k_match, max_results, chunk_seqs,
    # chunk_bytes, in_flight, cb, user, total)
    "kaamer_search_file": (C.c_int, HANDLE + FILE_IN + SEQ_TYPE + TOP + CHUNKS + CB),
    # kaamer-db -merge and the split makedb runs (-offset / -length)
    "kaamer_image_load_factor": (C.c_double, [C.c_void_p]),
    "kaamer_image_merge": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_double] + NEW),
    "kaamer_image_merge_device": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_double, C.c_int] + NEW),
    "kaamer_proteins_merge": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32] + NEW),
    "kaamer_makedb_text_range": (C.c_int, TEXT_IN + [C.c_int32, C.c_int32, C.c_uint64, C.c_uint64] + NEW),
    # FASTQ / FASTA text parsed on the device: the parser, the cut rules, the whole-file drivers
    "kaamer_text_parser_create": (C.c_int, [C.c_int, C.c_uint64, C.c_uint32] + NEW),
    "kaamer_text_parser_create_lines": (C.c_int, [C.c_int, C.c_uint64, C.c_uint32, C.c_uint64] + NEW),
    "kaamer_text_parser_free": (None, [C.c_void_p]),
    "kaamer_parse_fastq_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "kaamer_parse_fasta_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p]),
    "kaamer_text_parser_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(TextParseResult)]),
    "kaamer_text_parser_geometry": (None, [C.POINTER(C.c_uint32)]),
    "kaamer_batch_top_text_spans": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(TextSpan)), C.POINTER(C.c_uint32)]),
    "kaamer_text_cut_fastq": (C.c_uint64, TEXT_IN),
    "kaamer_text_cut_fasta": (C.c_uint64, TEXT_IN),
    # (handle, path, format, seq_type, min_k_ratio, min_k_match, max_results, chunk_text_bytes, in_flight[, device_inflate], cb, user,
    # total); the FASTA driver has no format
    "kaamer_search_text_file": (C.c_int, HANDLE + [C.c_char_p, C.c_int] + SEQ_TYPE + TOP + TEXT_CHUNKS + CB),
    "kaamer_search_text_file_opts": (C.c_int, HANDLE + [C.c_char_p, C.c_int] + SEQ_TYPE + TOP + TEXT_CHUNKS + [C.c_int32] + CB),
    "kaamer_search_fasta_file": (C.c_int, HANDLE + [C.c_char_p] + SEQ_TYPE + TOP + TEXT_CHUNKS + CB),
    # BGZF inflated on the device: the host scan of the block headers, the inflater, the cut on the device
    "kaamer_bgzf_scan": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kaamer_inflater_create": (C.c_int, [C.c_int, C.c_uint64, C.c_uint32] + NEW),
    "kaamer_inflater_free": (None, [C.c_void_p]),
    "kaamer_inflate_bgzf_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]),
    "kaamer_inflater_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(InflateResult)]),
    "kaamer_inflater_geometry": (None, [C.POINTER(C.c_uint32)]),
    "kaamer_text_cut_fastq_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]),
    "kaamer_batch_top_text": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    # the TSV response rows on the host: (extract_positions, annotations, proteins, buf, cap)
    "kaamer_format_tsv_header": (C.c_uint64, ROWS + [C.c_void_p, C.c_char_p, C.c_uint64]),
    "kaamer_format_tsv_aln_header": (C.c_uint64, ROWS + [C.c_void_p, C.c_char_p, C.c_uint64]),
    # (top, name_bytes, name_bytes_len, name_spans, n_names, proteins[, seq_type], extract_positions, annotations, buf, cap, line_off)
    "kaamer_format_tsv": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p] + ROWS
                          + [C.c_void_p, C.c_uint64, C.c_void_p]),
    "kaamer_format_tsv_aln": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p] + SEQ_TYPE + ROWS
                              + [C.c_void_p, C.c_uint64, C.c_void_p]),
    # (top[, alns], pos_bits_len, pos_off, pos_bits, ...the same)
    "kaamer_format_tsv_arrays": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32,
                                             C.c_void_p] + ROWS + [C.c_void_p, C.c_uint64, C.c_void_p]),
    "kaamer_format_tsv_aln_arrays": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                                 C.c_uint32, C.c_void_p] + SEQ_TYPE + ROWS + [C.c_void_p, C.c_uint64, C.c_void_p]),
    "kaamer_format_double": (C.c_uint64, [C.c_double, C.c_int32, C.c_char_p, C.c_uint64]),
    "kaamer_tsv_aln_rows_device": (C.c_int, [C.c_void_p, C.POINTER(TsvRowsIn), C.POINTER(TopnAlignments), C.POINTER(TsvAlnOpts), C.c_void_p,
                                             C.c_uint64, C.c_void_p, C.POINTER(TsvRowsResult)]),
    "kaamer_tsv_format_doubles_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p]),
    "kaamer_index_set_tsv_aln_raw_count": (C.c_int, [C.c_void_p, C.c_uint32]),
    # the JSON response on the host: (annotations, proteins, buf, cap)
    "kaamer_format_json_header": (C.c_uint64, [C.c_int32, C.c_void_p, C.c_char_p, C.c_uint64]),
    "kaamer_format_json_trailer": (C.c_uint64, [C.c_char_p, C.c_uint64]),
    # (top, seqs, offsets, n_seqs, name_bytes, name_bytes_len, name_spans, n_names, proteins, seq_type, text_format,
    #  extract_positions, buf, cap, obj_off)
    "kaamer_format_json": (C.c_int64, [C.c_void_p] + BATCH + [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p,
                                                              C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p]),
    # (top, alns, pos_bits_len, pos_off, pos_bits, ...the same from seqs on)
    "kaamer_format_json_arrays": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + BATCH
                                  + [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_void_p, C.c_uint64, C.c_void_p]),
    "kaamer_json_escape": (C.c_uint64, TEXT_IN + [C.c_char_p, C.c_uint64]),
    "kaamer_json_protein_value": (C.c_uint64, [C.POINTER(ProteinEntry), C.POINTER(C.c_char_p), C.c_char_p, C.c_uint64]),
}

# a database or query text parsed on the host: (text, len, out)
for _name in ("makedb_fasta", "makedb_tsv", "makedb_embl", "makedb_gbk", "parse_fasta", "parse_fastq"):
    SYMBOLS["kaamer_" + _name] = (C.c_int, TEXT_IN + NEW)

# the database FASTA text read on the device: (text, len, nb_before, more, device, out), and the two builds that take the
# text: (text, len, shard, n_shards, load_factor, device, proteins, out)
SYMBOLS["kaamer_makedb_fasta_device"] = (C.c_int, TEXT_IN + [C.c_uint64, C.c_int32, C.c_int] + NEW)
for _name in ("image_build_fasta_device", "index_build_fasta", "image_build_tsv_device", "index_build_tsv", "image_build_embl_device",
              "index_build_embl", "image_build_gbk_device", "index_build_gbk"):
    SYMBOLS["kaamer_" + _name] = (C.c_int, TEXT_IN + [C.c_uint32, C.c_uint32, C.c_double, C.c_int] + NEW + NEW)
# the database TSV rows read on the device: (text, len, header, header_len, id_base, device, out); its two builds are above
SYMBOLS["kaamer_makedb_tsv_device"] = (C.c_int, TEXT_IN + TEXT_IN + [C.c_uint64, C.c_int] + NEW)
# the database EMBL text read on the device: (text, len, nb_before, device, out), its cut rule; its two builds are above
SYMBOLS["kaamer_makedb_embl_device"] = (C.c_int, TEXT_IN + [C.c_uint64, C.c_int] + NEW)
SYMBOLS["kaamer_text_cut_embl"] = (C.c_uint64, TEXT_IN)
# the database GBK text read on the device: (text, len, nb_before, device, out); its cut rule is the EMBL one, its two builds are above
SYMBOLS["kaamer_makedb_gbk_device"] = (C.c_int, TEXT_IN + [C.c_uint64, C.c_int] + NEW)

# the packed-batch calls of an index and of a sharded index; search fills a result, submit a ticket for wait / discard
for _p in ("", "sharded_"):
    # the reported hits, cgo-safe forms: (handle, seqs, offsets, n_seqs, seq_type, min_k_ratio, min_k_match, max_results[,
    # want_positions, sub_matrix, gap_open, gap_extend, want_text], out)
    for _verb, _out in OUT.items():
        for _form, _mid in (("", []), ("_pos", []), ("_aln", ALIGN)):
            SYMBOLS["kaamer_%s%s_batch_top%s_flat" % (_p, _verb, _form)] = (C.c_int, HANDLE + BATCH + SEQ_TYPE + TOP + _mid + _out)
    # ... their struct forms: (handle, batch_in, topn_opts, out)
    SYMBOLS["kaamer_%ssearch_batch_top" % _p] = (C.c_int, HANDLE + [C.c_void_p, C.c_void_p] + OUT["search"])
    SYMBOLS["kaamer_%ssubmit_batch_top" % _p] = (C.c_int, HANDLE + [C.c_void_p, C.c_void_p] + OUT["submit"])
    SYMBOLS["kaamer_%swait_batch_top" % _p] = (C.c_int, HANDLE + OUT["search"])
    SYMBOLS["kaamer_%sticket_discard" % _p] = (None, HANDLE)
    # the full hit lists (PositionHits included): (handle, seqs, offsets, n_seqs, seq_type, want_positions, out)
    SYMBOLS["kaamer_%ssearch_batch_flat" % _p] = (C.c_int, HANDLE + BATCH + SEQ_TYPE + [C.c_int32] + FULL_OUT)
    SYMBOLS["kaamer_%ssubmit_batch_flat" % _p] = (C.c_int, HANDLE + BATCH + SEQ_TYPE + [C.c_int32] + OUT["submit"])
    SYMBOLS["kaamer_%ssearch_batch" % _p] = (C.c_int, HANDLE + [C.POINTER(BatchIn)] + FULL_OUT)
    SYMBOLS["kaamer_%swait_batch" % _p] = (C.c_int, HANDLE + FULL_OUT)
    SYMBOLS["kaamer_%sfull_ticket_discard" % _p] = (None, HANDLE)

# the streams on the three handle kinds; open forms: (handle, seq_type, min_k_ratio, min_k_match, max_results[, want_positions,
# sub_matrix, gap_open, gap_extend, want_text], out)
for _kind in ("stream", "replica_stream", "sharded_stream"):
    for _form, _mid in (("", []), ("_pos", []), ("_aln", ALIGN)):
        SYMBOLS["kaamer_%s_open%s_flat" % (_kind, _form)] = (C.c_int, HANDLE + SEQ_TYPE + TOP + _mid + NEW)
    SYMBOLS["kaamer_%s_push" % _kind] = (C.c_int, HANDLE + BATCH)
    SYMBOLS["kaamer_%s_pop" % _kind] = (C.c_int, HANDLE + OUT["search"])
    SYMBOLS["kaamer_%s_pending" % _kind] = (C.c_uint32, HANDLE)
    SYMBOLS["kaamer_%s_close" % _kind] = (None, HANDLE)

# the whole-file drivers with the bitmaps / alignments of the reported hits: (handle, path, format, strict_scanner, seq_type,
# min_k_ratio, min_k_match, max_results, want_positions, want_aln, sub_matrix, gap_open, gap_extend, want_text, chunk_seqs,
# chunk_bytes, in_flight, cb, user, total)
for _name in ("kaamer_search_file_opts", "kaamer_sharded_search_file"):
    SYMBOLS[_name] = (C.c_int, HANDLE + FILE_IN + SEQ_TYPE + TOP + ALIGN_FILE + CHUNKS + CB)

# the calls that take query text (FASTQ or FASTA text, BGZF blocks of FASTQ) and may write the response on the device:
# (handle, <the kind's head>, min_k_ratio, min_k_match, max_results, <what the format adds>, out)
for _kind, _head in TEXT_HEAD.items():
    for _verb, _out in OUT.items():
        for _form, _tail in TEXT_TAIL.items():
            SYMBOLS["kaamer_%s_%s_top%s_flat" % (_verb, _kind, _form)] = (C.c_int, HANDLE + _head + TOP + _tail + _out)

# the device stages that write the TSV rows / the JSON objects, and what the text calls return of them
for _kind, _in, _res in (("tsv", TsvRowsIn, TsvRowsResult), ("json", JsonRowsIn, JsonRowsResult)):
    SYMBOLS["kaamer_%s_stage_create" % _kind] = (C.c_int, HANDLE + [C.c_uint32, C.c_uint64] + NEW)
    SYMBOLS["kaamer_%s_stage_free" % _kind] = (None, HANDLE)
    # (stage, rows_in, d_out, out_cap, stream, result)
    SYMBOLS["kaamer_%s_rows_device" % _kind] = (C.c_int, HANDLE + [C.POINTER(_in), C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(_res)])
    SYMBOLS["kaamer_%s_rows_finish" % _kind] = (C.c_int, HANDLE + [C.c_void_p, C.POINTER(C.c_uint64)])
    SYMBOLS["kaamer_%s_geometry" % _kind] = (None, [C.POINTER(C.c_uint32)])
    SYMBOLS["kaamer_batch_top_%s" % _kind] = (C.c_int, HANDLE + [C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.POINTER(C.c_uint64))])
    SYMBOLS["kaamer_index_set_%s_bounds" % _kind] = (C.c_int, HANDLE + [C.c_uint64, C.c_uint64])

for _name in ("sharded_exchange_info", "sharded_positions_info", "index_align_info", "sharded_align_info", "sharded_align_stage_info",
              "tsv_aln_info", "index_tsv_aln_info", "index_subject_text_info", "index_subject_json_info"):
    SYMBOLS["kaamer_" + _name] = INFO
for _name in ("index_attach_proteins", "sharded_index_attach_proteins", "replicas_attach_proteins", "index_attach_subject_text",
              "index_attach_subject_json"):
    SYMBOLS["kaamer_" + _name] = ATTACH

SHARDED_SETS = 3   # KAAMER_SHARDED_SETS
FASTA, TSV, EMBL, GBK = 0, 1, 2, 3   # the `format` of kaamer_makedb_text / _range
MAKEDB_LENGTH_ALL = 2 ** 63 - 1      # the default of -length (cmd/kaamer-db/main.go:142: uint(MaxInt))

_lib = None


def lib():
    """Loads libkaamer_hip.so.  `import torch` first when torch is used in the same
    process, so both resolve to ONE HIP runtime (same libamdhip64 SONAME)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libkaamer_hip.so is not built: run `python -m kaamer_amd.build` "
                          "(expected at %s); there is no CPU fallback" % LIB_PATH)
    try:
        import torch  # noqa: F401  (loads torch's libamdhip64 first when torch is installed)
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    host_only = bool(os.environ.get("KAAMER_HOST_ONLY"))  # the sanitized CPU build of the host sources (tools/asan)
    for name, (res, args) in SYMBOLS.items():
        if host_only and not hasattr(L, name):
            continue
        f = getattr(L, name)  # AttributeError if the library lacks a declared symbol
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def error(rc):
    """the KaamerError of a return code, with the message the library kept for it"""
    return KaamerError(rc, (lib().kaamer_last_error() or b"").decode("utf-8", "replace"))


def check(rc):
    if rc != OK:
        raise error(rc)
