// kaamer_internal.h — declarations shared by the translation units of
// libkaamer_hip.so.  Not part of the ABI.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/kaamer_hip.h"
#include "kaamer_layout.h"

struct kaamer_image {
    kh_image_header hdr;
    kh_bucket *buckets;
    uint32_t *arena;
};

// records the thread-local error string and returns `code`
int kaamer_fail(int code, const char *fmt, ...);
int kaamer_image_alloc(kaamer_image *img, uint64_t n_buckets, uint64_t arena_words);
extern "C" void kaamer_stats_from_header(const kh_image_header *h, kaamer_image_stats *out);

// an image whose two arrays live on a device (builder_device.hip); the owner hipFree()s them
struct kaamer_device_image {
    kh_image_header hdr;
    kh_bucket *d_buckets;
    uint32_t *d_arena;
};
int kaamer_build_on_device(const uint8_t *seqs, const uint64_t *offsets, const uint32_t *ids, uint32_t n_proteins,
                           uint32_t shard, uint32_t n_shards, double load, int device, kaamer_device_image *out);
// ... the same build from packed proteins that lie on `device` already (offsets[0] = 0, 32 bytes of slack behind the last
// residue); the three buffers stay the caller's
int kaamer_build_resident(const uint8_t *d_seqs, const uint64_t *d_offsets, const uint32_t *d_ids, uint32_t n_proteins, uint64_t total_res,
                          uint32_t shard, uint32_t n_shards, double load, int device, kaamer_device_image *out);
// the host copy of an image that was made on the device; di's two allocations are freed
int kaamer_device_image_download(kaamer_device_image *di, kaamer_image **out);
// The table of a text whose accepted entries were packed elsewhere (the device readers): arrays of the right sizes for the
// caller to fill with bulk copies (offsets and entry_off n + 1, feature_off n * features + 1, the first 0 each), then
// kaamer_proteins_table_seal for by_id and KStats.  The FASTA reader's feature_names are {"ProteinName"}
struct kaamer_table_arrays {
    uint32_t *ids;
    uint8_t *seqs;
    uint64_t *offsets;
    char *entry_ids;
    uint64_t *entry_off;
    char *features;
    uint64_t *feature_off;
};
kaamer_proteins *kaamer_proteins_table_new(const std::vector<std::string> &feature_names, uint32_t n, uint64_t seq_bytes, uint64_t id_bytes,
                                           uint64_t feature_bytes, kaamer_table_arrays *a);
extern "C" void kaamer_proteins_table_seal(kaamer_proteins *p);
// ... and, for the EMBL reader, the whole strings of the n records that hold more residues than their SQ line declares
// (Protein.Sequence against what is indexed, inputEMBL.go:293-312): record recs[i] stores bytes[off[i] .. off[i + 1]).
// 0, or KAAMER_E_NOMEM
int kaamer_proteins_table_full_seqs(kaamer_proteins *p, const uint32_t *recs, const uint64_t *off, const char *bytes, uint32_t n);
// The header row of a TSV database (inputTSV.go:94-115), one statement for the host reader and the device reader: slot[i] is
// column i's feature index, or one of the two required columns ("entryid" / "sequence" in any ASCII case; each may occur more
// than once).  [b, e): the line without its end (b == NULL: the text has no line).  KAAMER_E_FORMAT with the reader's two
// messages when a required column is missing.
enum { KAAMER_TSV_ENTRY_ID = -1, KAAMER_TSV_SEQUENCE = -2 };
struct kaamer_tsv_columns {
    std::vector<int> slot;
    std::vector<std::string> feature_names;   // as written, duplicates kept
};
int kaamer_tsv_header(const char *b, const char *e, kaamer_tsv_columns *c);
// ... of a text's first line (one trailing '\r' dropped); *rows_at: where the second line starts (len: there is none)
int kaamer_tsv_header_of_text(const char *text, uint64_t len, kaamer_tsv_columns *c, uint64_t *rows_at);
// what kaamer_image_merge and kaamer_image_merge_device check before anything is dereferenced (builder.cpp);
// n_pairs[i] = the pairs input i enumerates
int kaamer_merge_check(const kaamer_image *const *imgs, uint32_t n, uint64_t *n_pairs);
extern "C" void kaamer_proteins_raw(const kaamer_proteins *p, const uint8_t **seqs, const uint64_t **offsets, const uint32_t **ids, uint32_t *n);

// The readers take the bytes of a file: when they start with the gzip signature (what http.DetectContentType calls
// "application/x-gzip": search.go:255-263, inputEMBL.go:76-84) the text is inflated first, all members of the stream
// (Go's gzip.Reader is multistream).  A stream that breaks off or is damaged yields the text up to there, as the
// reference's scanner does (it stops at the read error, whatever was read is processed, the error is not looked at).
// Returns 0, or KAAMER_E_FORMAT when not even the first header is a gzip header (gzip.NewReader fails: no input).
bool kaamer_is_gzip(const char *text, uint64_t len);
int kaamer_gunzip(const char *text, uint64_t len, std::string *out);

// The bytes of a query file as text (host_search.cpp): plain, or gzip inflated incrementally.  One copy for kaamer_reader_*
// and kaamer_search_text_file.  The fd stays the caller's.
struct kaamer_bytes;
int kaamer_bytes_open_fd(int fd, kaamer_bytes **out);                     // sniffs the first 32 bytes (search.go:246-270)
const uint8_t *kaamer_bytes_head(const kaamer_bytes *b, size_t *n);       // ... which are these
bool kaamer_bytes_is_gzip(const kaamer_bytes *b);
size_t kaamer_bytes_read(kaamer_bytes *b, char *dst, size_t cap);         // the next block of text; 0: the input is over
void kaamer_bytes_end(kaamer_bytes *b);                                   // nothing more is handed out
void kaamer_bytes_close(kaamer_bytes *b);
// ... cut into chunks by a cut rule, kaamer_text_cut_fastq or kaamer_text_cut_fasta (the reader half of kaamer_search_text_file
// and kaamer_search_fasta_file; the rules: host_search.cpp).  Once kaamer_text_chunker_done is true, the chunk handed out
// last was the rest of the input.
struct kaamer_text_chunker;
// (fasta: the cut rule is kaamer_text_cut_fasta and the reader speaks as kaamer_search_fasta_file; else kaamer_text_cut_fastq)
kaamer_text_chunker *kaamer_text_chunker_new(kaamer_bytes *src, uint64_t budget, bool fasta = false);   // src stays the caller's
int kaamer_text_chunker_next(kaamer_text_chunker *c, std::vector<char> *chunk, size_t *len);
bool kaamer_text_chunker_done(const kaamer_text_chunker *c);
void kaamer_text_chunker_free(kaamer_text_chunker *c);
void kaamer_text_chunker_prime(kaamer_text_chunker *c, const char *text, size_t len);   // text in front of the source's

// The alignment step's shared statements (align.hip), for the stage that aligns the reported hits of a top-N call
// (search.hip: top_align.hip.inc): the integers of one alignment as the device leaves them ...
struct kaamer_align_ints {
    int32_t n_ops, start_i, start_j, end_i, end_j;   // columns; 0-based cell before the first column, 1-based last cell
    int32_t identical, similar, mismatches, gap_openings, raw;
};
int kaamer_align_dp_open();                 // the aligner's GapOpen (align.go:62-65)
void kaamer_align_matrix(int *m676);        // BLOSUM62 in AAPosInMatrix order, row / column 0 = KAAMER_ALIGN_GAP_COLUMN (read once)
// GetMatrixScores + "BLOSUM62 only": false = every alignment of the request has status 1
bool kaamer_align_options(const char *sub_matrix, int gap_open, int gap_extend, double *lambda, double *k);
// ... the floats of align.go:101-102,137,142 and the coordinates of :153-156 from them (aln_off is left alone)
void kaamer_align_finish(kaamer_alignment *a, const kaamer_align_ints *t, uint64_t query_len, uint64_t number_of_aa, double lambda, double kk);
// ... the 2^BitScore of align.go:142 as kaamer_align_finish computes it (one statement: the device rows tabulate it per raw score)
double kaamer_align_pow2(double bitscore);
// ... and the three rows from the operations (in reverse) and the raw letters; t (may be NULL) receives the tallies
void kaamer_align_rows(const uint8_t *ops_rev, int len, const uint8_t *q, const uint8_t *s, int start_i, int start_j, const int *matrix,
                       int gap_open, int gap_extend, char *rows, kaamer_align_ints *t);
