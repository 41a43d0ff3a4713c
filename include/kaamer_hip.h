/*
 * kaamer_hip.h — C ABI of libkaamer_hip.so, the MI355X (gfx950) k-mer search
 * path for kaamer.
 *
 * This is the drop-in boundary.  The reference (zorino/kaamer) has no FFI; the
 * seam is the Go function boundary between the search drivers and the hot
 * path.  Each entry point cites the reference code it replaces (paths under
 * the reference tree).  A cgo shim binds exactly these symbols — see
 * INTEGRATION.md.
 *
 * Conventions
 *   - every call returns KAAMER_OK (0) or a negative kaamer_status; nothing
 *     throws or aborts (the reference log.Fatal()s);
 *   - kaamer_last_error() returns a thread-local message for the last failure;
 *   - input pointers are borrowed for the duration of the call only (cgo rule);
 *   - outputs of the host-buffer calls are library-owned until the matching
 *     *_free call;
 *   - plain pointers and sizes only, no C++ or torch types;
 *   - cgo safety: NO STRUCT PASSED TO THE LIBRARY NEEDS TO CONTAIN A CALLER POINTER.  Every host-buffer call has a
 *     *_flat form that takes the caller's buffers as direct arguments (cgo pins a Go pointer passed as an argument
 *     for the duration of the call; a Go pointer stored inside a struct that is itself passed by pointer is a
 *     run-time panic, "cgo argument has Go pointer to unpinned Go pointer").  The struct forms (kaamer_batch_in) are
 *     for C / C++ / ctypes callers.  kaamer_topn_opts' pointer fields are device / library handles (NULL from a host
 *     caller), never caller memory.
 */
#ifndef KAAMER_HIP_H
#define KAAMER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KAAMER_ABI_VERSION 4
#define KAAMER_KMER_SIZE 7 /* pkg/search/search.go:45, pkg/makedb/makedb.go:30 */

typedef enum {
    KAAMER_OK = 0,
    KAAMER_E_ARG = -1,       /* bad argument                                   */
    KAAMER_E_IO = -2,        /* file open/read/write/format                    */
    KAAMER_E_NOMEM = -3,     /* host or device allocation failed               */
    KAAMER_E_HIP = -4,       /* a HIP runtime call failed (no device, ...)     */
    KAAMER_E_CAPACITY = -5,  /* a workspace bound was exceeded; enlarge, retry */
    KAAMER_E_FORMAT = -6,    /* index image/version mismatch                   */
    KAAMER_E_BUSY = -7,      /* every host slot holds a batch: wait / pop first */
    KAAMER_E_RANGE = -8      /* a value outside what a device stage tabulates: take the host route (kaamer_tsv_rows_finish) */
} kaamer_status;

/* search.go:41-44 */
enum { KAAMER_NUCLEOTIDE = 0, KAAMER_PROTEIN = 1, KAAMER_READS = 2 };

/* The request's genetic code (SearchOptions.GeneticCode, search.go:60) rides in every `seq_type` argument and field:
 * bits 0-7 are the sequence type above, bits 8-15 the code, every higher bit is 0.  Valid codes are the keys of
 * search.GCodes (gcode.go:21-34): 1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14, 15.  Code 0 -- every seq_type value of
 * before this macro -- is the reference's behaviour: GetORFs consults the bacterial table 11 whatever the request says
 * (dna.go:106), and an explicit 11 gives exactly the same result.  The other codes are honoured where the reference
 * ignores them: the 6-frame translation reads its start / stop / amino-acid classes from that table.  With
 * KAAMER_PROTEIN a valid code is accepted and ignored (the reference sends GeneticCode: 11 on protein requests too).
 * Any other code, or a bit above 15: KAAMER_E_ARG, and the message names the code, before anything is enqueued or a
 * slot is taken.  The code belongs to the search call, or to the open call of a stream or file driver: workspaces, host
 * slots and sharded sets are matched and sized by the sequence type alone (kaamer_workspace_create ignores the code
 * bits) and keep no code from one batch to the next. */
#define KAAMER_SEQ_TYPE(type, genetic_code) ((int32_t)((type) | ((genetic_code) << 8)))
#define KAAMER_SEQ_TYPE_BASE(seq_type) ((int32_t)((seq_type) & 0xFF))
#define KAAMER_SEQ_TYPE_GENETIC_CODE(seq_type) ((int32_t)(((seq_type) >> 8) & 0xFF))

/* The library's own table of a genetic code, codons in t-c-a-g order (ttt, ttc, tta, ttg, tct, ...): aa[i] the amino-acid
 * letter ('*': a stop codon), start[i] 'M' for a start codon and '-' otherwise; no terminator is written.  Code 0 returns
 * table 11.  KAAMER_E_ARG for a code that is not a key of search.GCodes.  Host only. */
int kaamer_genetic_code(int32_t code, char aa[64], char start[64]);

const char *kaamer_last_error(void);
int kaamer_abi_version(void);

typedef struct kaamer_reads kaamer_reads;   /* parsed query records: "Readers" at the end of this file */

/* ------------------------------------------------------------------------- */
/* K-mer codec (host) — replaces K_.EncodeKmer / CreateBytesKey,              */
/* pkg/kvstore/k_store.go:66-76,91-117.                                       */
/* ------------------------------------------------------------------------- */
uint32_t kaamer_encode_kmer(const uint8_t kmer[KAAMER_KMER_SIZE]);

/* ------------------------------------------------------------------------- */
/* Builder — the GPU-layout emitter beside pkg/makedb + pkg/indexdb.           */
/*   pairs  = what makedb's emit loops write into kmer_store                   */
/*            (inputFASTA.go:245-248, inputTSV.go:236-239, inputEMBL.go:309-312,*/
/*            inputGBK.go:296-299): one (key, proteinId) per 7-mer window;     */
/*   build  = indexdb.IndexStore/KeyToList (indexdb.go:68-132) +               */
/*            RemoveDuplicatesFromSlice (kv_store.go:284-305): per key the     */
/*            unique id set; identical sets are stored once (the KComb idea,   */
/*            kcomb_store.go:42-85).                                           */
/* An image is the host copy of one shard's table (buckets + postings arena).  */
/* ------------------------------------------------------------------------- */
typedef struct { uint32_t key; uint32_t protein_id; } kaamer_pair;
typedef struct kaamer_image kaamer_image;

typedef struct {
    uint64_t n_pairs;      /* unique (key,id) pairs in this shard              */
    uint64_t n_keys;       /* distinct keys in this shard                      */
    uint64_t n_buckets;    /* 64-byte buckets                                  */
    uint64_t arena_words;  /* u32 words of the postings arena                  */
    uint64_t n_inline;     /* keys whose single id is stored in the slot       */
    uint64_t n_lists;      /* distinct postings lists in the arena             */
    uint64_t max_list;     /* longest postings list                            */
    uint64_t n_displaced;  /* keys not in their home bucket                    */
    uint32_t shard, n_shards;
    uint32_t max_protein_id;
    uint32_t reserved;
} kaamer_image_stats;

/* shard s of n_shards holds the keys with kaamer_shard_of(key) == s */
uint32_t kaamer_shard_of(uint32_t key, uint32_t n_shards);

int kaamer_image_build_pairs(const kaamer_pair *pairs, uint64_t n, uint32_t shard,
                             uint32_t n_shards, double load_factor, kaamer_image **out);
/* Emit loop + build: every window seqs[off[p]+i .. +7), i in [0,len-7], of
 * every protein with len >= 7, under id ids[p] (ids == NULL: the TSV rule,
 * 0-based running index, inputTSV.go:141-142).
 * Postings lists are laid out in the order in which a walk over the proteins
 * (input order) and their windows (ascending position) first refers to them, a
 * shared list by its first reference (build_pairs: the order of the pairs), so
 * that the lists behind consecutive windows of a protein are neighbours in the
 * arena.  This is a property of where lists sit, not of the image format: same
 * header and version, and an image file written by an earlier build (lists in
 * ascending-key order) loads and searches as before. */
int kaamer_image_build_proteins(const uint8_t *seqs, const uint64_t *offsets,
                                const uint32_t *ids, uint32_t n_proteins, uint32_t shard,
                                uint32_t n_shards, double load_factor, kaamer_image **out);
/* The same build on the device (builder_device.hip): emit, radix sort, unique,
 * set sharing and bucket placement run on `device`; the image that comes back
 * is byte-identical to kaamer_image_build_proteins' (pkg/indexdb/indexdb.go:68-132,
 * pkg/kvstore/kcomb_store.go:42-85 at DB-UR shard size).  Inputs are host buffers. */
int kaamer_image_build_proteins_device(const uint8_t *seqs, const uint64_t *offsets,
                                       const uint32_t *ids, uint32_t n_proteins, uint32_t shard,
                                       uint32_t n_shards, double load_factor, int device,
                                       kaamer_image **out);
int kaamer_image_save(const kaamer_image *img, const char *path);
int kaamer_image_load(const char *path, kaamer_image **out);
int kaamer_image_get_stats(const kaamer_image *img, kaamer_image_stats *out);
void kaamer_image_free(kaamer_image *img);
/* host-side point read of an image (builder self-check; not the search path):
 * returns the number of ids under `key`, copies up to cap of them */
uint32_t kaamer_image_get(const kaamer_image *img, uint32_t key, uint32_t *ids, uint32_t cap);
/* the load factor the image was built with (after the builders' own rule: outside (0.05, 0.95] it became 0.5) */
double kaamer_image_load_factor(const kaamer_image *img);

/* kaamer-db -merge: the union of images of the same shard (pkg/mergedb/mergedb.go:42-135, the kmer_store leg:
 * MergeStores streams every version of every key into store 1; pkg/indexdb/indexdb.go:68-132 then collapses them).
 * Per key the id set is the union of the inputs' sets, a pair present in two inputs is stored once, identical union sets
 * share one list, and a key whose union is one id below 2^31 is inline.  An image does not record which window first
 * referred to a list, so the layout is defined through kaamer_image_build_pairs, whose order is its input's:
 *     merge(img_0 .. img_{n-1}) := kaamer_image_build_pairs(E(img_0) ++ .. ++ E(img_{n-1}), shard, n_shards, load_factor)
 * where E(img) lists first the keys whose slot holds a list offset, by (offset, key) ascending, each as (key, id) for its
 * ids in stored order, then the keys with an inline id by key ascending.  So the lists of img_0 keep their relative order
 * and are followed by what img_1 adds; every counter of kaamer_image_stats equals that of one build over the union of the
 * inputs' proteins at the same load factor (only the order of the lists in the arena differs); and the merge of ONE image
 * built here, at its own load factor, is that image byte for byte (at another load factor: a re-bucketing).
 * KAAMER_E_ARG: n == 0, a null entry, inputs that differ in shard / n_shards / kmer_size / version, a list offset or count
 * that points outside its image's arena (checked before anything is dereferenced).  KAAMER_E_CAPACITY / the builders' own
 * codes for their limits (2^32 - 1 pairs per shard, arena 32 GiB, buckets).  load_factor outside (0.05, 0.95] becomes 0.5. */
int kaamer_image_merge(const kaamer_image *const *imgs, uint32_t n, double load_factor, kaamer_image **out);
/* The same image, byte for byte, made on `device` (merge_device.hip): the inputs' buckets and arenas are uploaded, expanded
 * to pairs there, and the build runs from the sort on as kaamer_image_build_proteins_device's does.  Peak device memory is
 * that of a build over the same number of pairs (two 8-byte buffers of the enumerated pairs) plus the uploaded inputs. */
int kaamer_image_merge_device(const kaamer_image *const *imgs, uint32_t n, double load_factor, int device,
                              kaamer_image **out);

/* ------------------------------------------------------------------------- */
/* makedb — which proteins a database file contributes and under which ids      */
/* (pkg/makedb/inputFASTA.go:95-124,191-250; inputTSV.go:92-142), kept with     */
/* their annotations: the table FetchHitsInformation reads                      */
/* (pkg/search/search.go:454-470, pkg/kvstore/protein.proto) instead of one     */
/* ProteinStore point read per hit.  Text is taken already decompressed.        */
/*   FASTA: record k (1-based) gets id k+1, the last two records share id N     */
/*          (reference behaviour); names with ", partial" and sequences shorter */
/*          than 7 are dropped; sequences are upper-cased; feature: ProteinName */
/*   TSV:   header row with EntryID and Sequence columns (any case); accepted   */
/*          rows get 0-based ids; sequences are NOT upper-cased; every other    */
/*          column is a feature                                                 */
/* ------------------------------------------------------------------------- */
typedef struct kaamer_proteins kaamer_proteins;
int kaamer_makedb_fasta(const char *text, uint64_t len, kaamer_proteins **out);
int kaamer_makedb_tsv(const char *text, uint64_t len, kaamer_proteins **out);
/*   EMBL:  UniProt flat file (pkg/makedb/inputEMBL.go:46-314).  Records end at a line "//"; record k (1-based
 *          ordinal of its "//", empty records use up a number) gets id k.  EntryId = first field of the ID line,
 *          features ProteinName (DE RecName / SubName, " {...};" evidence removed), GeneName, EC, GO, KEGG_ID,
 *          BioCyc_ID, HAMAP, Organism, TaxId (the reference's [12:] drops the id's first digit: kept),
 *          FullTaxonomy.  "Flags: Fragment;" entries are dropped.  The length is the one DECLARED on the SQ line:
 *          entries declaring < 7 are dropped and the k-mers are those of Sequence[:Length].  Not upper-cased, no
 *          ", partial" filter.
 *   GBK:   GenPept flat file (inputGBK.go:45-301).  Same record / id rule.  DEFINITION -> ProteinName (a trailing
 *          " [organism]." removed), VERSION -> EntryId, ORGANISM -> Organism + FullTaxonomy, ORIGIN -> the sequence,
 *          upper-cased; names containing ", partial" and sequences shorter than 7 are dropped.
 *   Where the Go code would panic on a malformed entry (a tag line shorter than the column it slices at, an SQ
 *   length beyond the sequence) the entry is dropped.
 *   -offset / -length (kaamer_makedb_text_range below) follow the scan loops (inputFASTA.go:64-125, inputEMBL.go:66-119,
 *   inputGBK.go:94-118): proteinNb counts '>' headers (FASTA) or "//" lines (EMBL, GBK), text is gathered only while
 *   proteinNb >= offset, and at proteinNb >= offset + length (Go uint: 64 bits, wrapping) the pending entry is queued and
 *   the scan ends.  Ids stay the loop's proteinNb: a FASTA range holds records offset .. offset + length - 1 under ids
 *   k + 1, an EMBL / GBK range records offset + 1 .. offset + length under ids k, so consecutive ranges partition the file
 *   and only the range that reaches the end of a FASTA file has two records share the last id.  (The FASTA loop leaves the
 *   entry in place when it breaks, so its closing statement, :120-124, queues that record a second time under the same id:
 *   reproduced; the record and the KStats counters count it twice.) */
int kaamer_makedb_embl(const char *text, uint64_t len, kaamer_proteins **out);
int kaamer_makedb_gbk(const char *text, uint64_t len, kaamer_proteins **out);
/* The four readers behind one entry point (format: 0 FASTA, 1 TSV, 2 EMBL, 3 GBK), with the reference's scanner limit on
 * request: strict_scanner = 1 ends the input at a line of 1 048 576 bytes or more, as bufio.Scanner with a 1 MiB buffer does
 * (inputFASTA.go:88-89 and the same two lines in the other readers): what was read before the line is processed as if the
 * file ended there.  strict_scanner = 0 (what the four functions above do) reads lines of any length. */
int kaamer_makedb_text(const char *text, uint64_t len, int32_t format, int32_t strict_scanner, kaamer_proteins **out);
/* kaamer_makedb_text with the scan loops' -offset / -length (cmd/kaamer-db/main.go:141-142; the rule is stated above).
 * offset = 0, length = INT64_MAX (the flags' defaults) is kaamer_makedb_text; TSV ignores both (inputTSV.go:40-145 never
 * reads them). */
int kaamer_makedb_text_range(const char *text, uint64_t len, int32_t format, int32_t strict_scanner,
                             uint64_t offset, uint64_t length, kaamer_proteins **out);
/* kaamer-db -merge, the protein_store leg + KStats (mergedb.go:91-98): the records of every table in argument order; when
 * an id occurs more than once the later record wins in kaamer_fetch_hits (store 2's Protein overwrites store 1's,
 * mergedb.go:98); kaamer_proteins_stats is the SUM of the inputs' counters, duplicates included (mergedb.go:91-93).
 * Divergence: the reference keeps the first database's KStats.Features; this table is dense per feature, so inputs whose
 * feature names differ are refused (KAAMER_E_ARG).  n == 0 or a null entry: KAAMER_E_ARG. */
int kaamer_proteins_merge(const kaamer_proteins *const *tables, uint32_t n, kaamer_proteins **out);
uint32_t kaamer_proteins_count(const kaamer_proteins *p);           /* accepted proteins       */
const uint32_t *kaamer_proteins_ids(const kaamer_proteins *p);      /* their protein ids       */
const uint8_t *kaamer_proteins_seqs(const kaamer_proteins *p);      /* packed sequences        */
const uint64_t *kaamer_proteins_offsets(const kaamer_proteins *p);  /* count + 1               */
uint32_t kaamer_proteins_n_features(const kaamer_proteins *p);      /* KStats.Features         */
const char *kaamer_proteins_feature_name(const kaamer_proteins *p, uint32_t i);
void kaamer_proteins_stats(const kaamer_proteins *p, uint64_t out[3]); /* KStats: NumberOfProteins, NumberOfAA, NumberOfKmers */
int kaamer_proteins_save(const kaamer_proteins *p, const char *path);
int kaamer_proteins_load(const char *path, kaamer_proteins **out);
void kaamer_proteins_free(kaamer_proteins *p);
/* emit loops + indexdb collapse over the accepted proteins under their ids -> one shard's image */
int kaamer_image_build_makedb(const kaamer_proteins *p, uint32_t shard, uint32_t n_shards, double load_factor,
                              kaamer_image **out);
/* the same on `device` (kaamer_image_build_proteins_device) */
int kaamer_image_build_makedb_device(const kaamer_proteins *p, uint32_t shard, uint32_t n_shards,
                                     double load_factor, int device, kaamer_image **out);
/* The FASTA reader on the device (makedb_fasta.hip.inc): the text is uploaded, read there, and the table comes back by bulk
 * copies.  It computes kaamer_makedb_fasta's rules, stated per line (they are not the query reader's, kaamer_parse_fasta):
 *   lines    split at '\n'; a last piece without '\n' is a line; one trailing '\r' is dropped; a line that is empty after
 *            that is skipped (the documented divergence: the reference panics there)
 *   class    H: the first byte is '>'.  S: every other non-empty line.  Nothing is trimmed: leading, trailing and interior
 *            spaces and tabs, an interior '\r' and a '>' inside the line are sequence bytes, whitespace-only lines are S lines
 *   entries  an H line and the S lines up to the next H line; S lines in front of the first H line form an entry of their
 *            own with an empty EntryId and an empty name
 *   ids      N = the H lines of the text; the entry the k-th H line opens gets id min(k + 1, N) as uint32 (the last two
 *            entries share N), the entry without a header min(1, N); ids are not renumbered after drops
 *   header   EntryId: the bytes after '>' up to the line's first ' '; ProteinName: everything after that space
 *   sequence the entry's S lines concatenated, a-z -> A-Z, every other byte (>= 0x80 included) as it is
 *   drops    ProteinName contains ", partial" (in the name only: ">abc, partial" has EntryId "abc," and is kept); fewer
 *            than 7 sequence bytes
 *   table    feature_names = {"ProteinName"}; KStats over the accepted entries
 * A text holds at most 2^32 - 1 bytes (KAAMER_E_ARG beyond, before anything else is looked at: cut at kaamer_text_cut_fasta);
 * one that starts with the gzip signature is taken as text, as kaamer_makedb_fasta takes it; a text with more lines than the
 * reader indexes is KAAMER_E_CAPACITY, never a partial table.  Out of scope here: -offset / -length and strict_scanner (they
 * stay on kaamer_makedb_text_range), TSV / EMBL / GBK, compressed input, a whole-file driver.
 *
 * kaamer_makedb_fasta's table from `text`, made on `device`: the scan loop started with proteinNb = nb_before and an
 * empty pending entry; more = 1: input follows, the pending entry at the end is queued under N + 1 as the next header
 * would do.  nb_before = 0, more = 0 is kaamer_makedb_fasta, field for field.  Pieces cut at kaamer_text_cut_fasta,
 * each with the number of '>' lines in front of it and more = 1 on all but the last, merged with
 * kaamer_proteins_merge, are the whole text's table. */
int kaamer_makedb_fasta_device(const char *text, uint64_t len, uint64_t nb_before, int32_t more, int device,
                               kaamer_proteins **out);
/* text -> table + one shard's image; the sequences never leave the device between the reader and the builder.
 * Image: byte for byte kaamer_image_build_makedb(kaamer_makedb_fasta(text)).  A bad shard: KAAMER_E_ARG. */
int kaamer_image_build_fasta_device(const char *text, uint64_t len, uint32_t shard, uint32_t n_shards,
                                    double load_factor, int device, kaamer_proteins **proteins, kaamer_image **image);
/* The TSV reader on the device (makedb_tsv.hip.inc): the rows are uploaded, read there, and the table with its feature
 * columns comes back by bulk copies.  It computes kaamer_makedb_tsv's rules, stated per line:
 *   lines    split at '\n'; a last piece without '\n' is a line; one trailing '\r' is dropped
 *   header   the first line, split at every '\t' (read on the host, by the routine kaamer_makedb_tsv reads it with): a
 *            column whose ASCII-lower-cased name is "entryid" is an EntryId column, "sequence" a Sequence column; every other
 *            column is a feature, in column order, its name as written; duplicate feature names stay separate columns.  No
 *            line at all or no EntryID column: KAAMER_E_FORMAT "TSV file doesn't contain 'EntryID' header"; no Sequence
 *            column: the same with 'Sequence'
 *   rows     every later line, an empty one included; its cells are the pieces between tabs.  Of H header columns only the
 *            first H cells count: further cells are ignored (the documented divergence: the reference panics there),
 *            missing cells are empty.  Where the header names EntryID or Sequence more than once, the last such column
 *            that the row has wins
 *   accept   a row whose Sequence cell has 7 bytes or more and whose EntryId cell is not empty; the k-th accepted row
 *            (0-based) gets id id_base + k as uint32.  Nothing is upper-cased, nothing is trimmed (an interior '\r' is a
 *            byte of its cell), bytes >= 0x80 stay as they are.  A rejected row takes no room anywhere
 *   table    feature_names = the header's feature columns; features protein-major, n * n_features + 1 offsets; KStats over
 *            the accepted rows
 * A text holds at most 2^32 - 1 bytes (KAAMER_E_ARG beyond, before anything else is looked at: cut at any '\n'); a text with
 * more lines than the reader indexes (2^32 - 16), or whose accepted rows times feature columns exceed that many cells, is
 * KAAMER_E_CAPACITY, never a partial table.  Out of scope here: strict_scanner (it stays on kaamer_makedb_text), -offset /
 * -length (the TSV loop ignores both), EMBL / GBK, compressed input, a whole-file driver.
 *
 * header == NULL: the first line of `text` is the header; with id_base = 0 the table is kaamer_makedb_tsv(text), field for
 * field.  header != NULL: `header` (header_len bytes, no '\n' in it: KAAMER_E_ARG) is the header line without its line end and
 * every line of `text` is a row.  That is the form for a file larger than one text: cut it at any '\n', give every piece the
 * header and the number of rows accepted in front of it (kaamer_proteins_count of the pieces before), merge the tables
 * with kaamer_proteins_merge: the whole text's table. */
int kaamer_makedb_tsv_device(const char *text, uint64_t len, const char *header, uint64_t header_len,
                             uint64_t id_base, int device, kaamer_proteins **out);
/* text (header line first) -> table + one shard's image; the sequences never leave the device between the reader and the
 * builder.  Image: byte for byte kaamer_image_build_makedb(kaamer_makedb_tsv(text)).  A bad shard: KAAMER_E_ARG. */
int kaamer_image_build_tsv_device(const char *text, uint64_t len, uint32_t shard, uint32_t n_shards,
                                  double load_factor, int device, kaamer_proteins **proteins, kaamer_image **image);
/* The EMBL reader on the device (makedb_embl.hip.inc): the text of a UniProt flat file (-f embl) is uploaded, read there,
 * and the table with its ten feature columns comes back by bulk copies.  It computes kaamer_makedb_embl's rules
 * (process_embl_entry is their statement), per line:
 *   lines    split at '\n'; a last piece without '\n' is a line; one trailing '\r' is dropped.  A line that is then exactly
 *            "//" ends an entry and takes a number, even when the entry is empty; "// ", "///" and "//\r\r" are ordinary
 *            lines.  Lines shorter than 2 bytes are ignored; what lies behind the last "//" is never queued
 *   tag      the first two bytes; only ID GN DE OX OS OC DR SQ and two spaces matter, every other line is skipped without
 *            being read further
 *   Skip     drops the whole entry: a line of a read tag with fewer than 5 bytes (a two-space line of 2 to 4 bytes too; a GN
 *            line that short holds no "Name=" and is not read); ID / OX / DR with no field behind column 5; an OX first
 *            field under 12 bytes; a matched DR (KEGG; GO; BioCyc; HAMAP;) without a second field; SQ with fewer than two
 *            fields; a DE line under 19 bytes that is RecName or SubName, or under 17 bytes that is EC; a declared length
 *            above the residues held
 *   drops    a DE line whose [5:] contains none of RecName, SubName, EC= but contains "Flags: Fragment;"; a declared length
 *            below 7 (the last SQ line wins, a number Atoi refuses is 0)
 *   order    GN is looked at only while GeneName is empty: among the GN lines that contain "Name=" anywhere, the first that
 *            is malformed (no field, or a first field under 5 bytes) or yields a non-empty value decides: Skip, or the value.
 *            ProteinName: the last RecName line resets it, each later SubName appends ";;" + v if the value so far is
 *            non-empty, else becomes the value; without a RecName the same from the first SubName.  EC, TaxId, EntryId: the
 *            last line wins
 *   separators  Organism (" ") and the four DR columns (";") in front of every contribution but the first, even when earlier
 *            ones were empty; FullTaxonomy " " only when what is gathered so far is non-empty
 *   values   " {.*};" is removed greedily (first " {" to the last "};" behind it), then all trailing ';' are cut, which may
 *            reach in front of the removed span; OS loses all trailing '.'; GN is field 0 [5:], OX field 0 [12:], the DR value
 *            field 1, each less its trailing ';'; fields split at ' ' and '\t'..'\r'
 *   sequence every two-space line's bytes behind column 5 with ' ' removed, wherever the line stands; nothing is upper-cased,
 *            bytes >= 0x80 stay.  Indexed is Sequence[:declared]; kaamer_fetch_hits returns sequence_len > length with the
 *            whole string for an entry that holds more
 *   table    feature_names = EMBL_DEF_FTS (ProteinName GeneName EC GO KEGG_ID BioCyc_ID HAMAP Organism TaxId FullTaxonomy);
 *            KStats over the kept entries
 * A text holds at most 2^32 - 1 bytes (KAAMER_E_ARG beyond, before anything else is looked at: cut at kaamer_text_cut_embl).
 * One that starts with the gzip signature is inflated on the host first, as kaamer_makedb_embl does, and an inflated text
 * beyond 2^32 - 1 bytes is KAAMER_E_ARG.  A text with more lines than the reader indexes (2^32 - 16) is KAAMER_E_CAPACITY,
 * never a partial table.  Out of scope here: GBK, -offset / -length and strict_scanner (they stay on
 * kaamer_makedb_text_range), a whole-file driver, compressed input on the device.
 *
 * nb_before: the "//" lines in front of this text; record k of it (1-based ordinal of its "//") gets id
 * (uint32_t)(nb_before + k).  nb_before = 0 is kaamer_makedb_embl(text), field for field, for every input.  Pieces cut at
 * kaamer_text_cut_embl, each with the "//" count in front of it, merged with kaamer_proteins_merge, are the whole text's
 * table. */
int kaamer_makedb_embl_device(const char *text, uint64_t len, uint64_t nb_before, int device, kaamer_proteins **out);
/* text -> table + one shard's image; the builder sees the indexed prefixes where they lie on the device.  Image: byte for
 * byte kaamer_image_build_makedb(kaamer_makedb_embl(text)).  A bad shard: KAAMER_E_ARG. */
int kaamer_image_build_embl_device(const char *text, uint64_t len, uint32_t shard, uint32_t n_shards,
                                   double load_factor, int device, kaamer_proteins **proteins, kaamer_image **image);
/* The GBK reader on the device (makedb_gbk.hip.inc): the text of a GenBank / GenPept flat file (-f gbk) is uploaded, read
 * there, and the table with its three feature columns comes back by bulk copies.  It computes kaamer_makedb_gbk's rules
 * (process_gbk_entry is their statement; where these words and that code differ, the code holds):
 *   lines    split at '\n'; a last piece without '\n' is a line; one trailing '\r' is dropped.  A line that is then exactly
 *            "//" ends an entry and takes a number, even when the entry is empty.  Lines shorter than 2 bytes change nothing
 *            and contribute nothing; what lies behind the last "//" belongs to no entry
 *   token    the line with leading and trailing ' ' removed (spaces only, not tabs), up to its first ' '; an all-space line
 *            has the empty token.  Compared case-sensitively, it sets the section state: 0 for LOCUS ACCESSION KEYWORDS
 *            SOURCE COMMENT REFERENCE DBLINK DBSOURCE, 1 DEFINITION, 2 VERSION, 3 ORGANISM, 4 FEATURES, 5 ORIGIN, 6 "//"
 *            (" //" and "// x" are such lines inside an entry).  Any other token leaves the state as it is, every entry
 *            starts in state 0, and a continuation line whose first word happens to be a keyword switches the state
 *   contribution  under the state after the line's own token.  1: [12:] is appended to ProteinName, " " in front when what
 *            is gathered so far is non-empty (an all-space line of 12 bytes or more adds a trailing space).  2: EntryId is
 *            the first field of [12:], fields split at ' ' and '\t'..'\r'; the last such line wins.  3: while Organism is
 *            empty, [12:] becomes Organism (an empty [12:] leaves it empty, the next line tries again); otherwise [12:] is
 *            appended to FullTaxonomy, " " in front when that is non-empty.  5: [10:] with every ' ' removed and 'a'..'z'
 *            upper-cased, other bytes (>= 0x80 too) as they are; the ORIGIN line itself contributes this way.  0, 4, 6:
 *            nothing
 *   Skip     drops the whole entry, where the reference would panic: a line of 2 to 11 bytes in state 1, 2 or 3; a line of
 *            2 to 9 bytes in state 5, a bare ORIGIN among them; a state-2 line with no field behind column 12
 *   drops    the joined ProteinName contains ", partial" (the match may span a join: one line ends in ',' and the next
 *            one's [12:] starts with "partial"); fewer than 7 residues
 *   ProteinName, last step  from the first " [" to the last "]." behind it is removed, on the joined string; the " [" may
 *            be a join's space in front of a line that starts with '['
 *   table    feature_names = GBK_DEF_FTS (ProteinName Organism FullTaxonomy); KStats over the kept entries.  GBK declares
 *            no length, so no record has a whole string beside its indexed one: sequence_len == length
 * A text holds at most 2^32 - 1 bytes (KAAMER_E_ARG beyond, before anything else is looked at: cut at kaamer_text_cut_embl,
 * whose terminator is GBK's too).  One that starts with the gzip signature is inflated on the host first, as
 * kaamer_makedb_gbk does, and an inflated text beyond 2^32 - 1 bytes is KAAMER_E_ARG.  A text with more lines than the reader
 * indexes (2^32 - 16) is KAAMER_E_CAPACITY, never a partial table.  Out of scope here: -offset / -length and strict_scanner
 * (they stay on kaamer_makedb_text_range), a whole-file driver, inflate on the device.
 *
 * nb_before: the "//" lines in front of this text; record k of it (1-based ordinal of its "//") gets id
 * (uint32_t)(nb_before + k).  nb_before = 0 is kaamer_makedb_gbk(text), field for field, for every input.  Pieces cut at
 * kaamer_text_cut_embl, each with the "//" count in front of it, merged with kaamer_proteins_merge, are the whole text's
 * table. */
int kaamer_makedb_gbk_device(const char *text, uint64_t len, uint64_t nb_before, int device, kaamer_proteins **out);
/* text -> table + one shard's image; the builder sees the sequences where they lie on the device.  Image: byte for byte
 * kaamer_image_build_makedb(kaamer_makedb_gbk(text)).  A bad shard: KAAMER_E_ARG. */
int kaamer_image_build_gbk_device(const char *text, uint64_t len, uint32_t shard, uint32_t n_shards,
                                  double load_factor, int device, kaamer_proteins **proteins, kaamer_image **image);
/* One Protein entry (protein.proto).  Pointers go into the table and stay valid until it is freed;
 * feature i is features[feature_off[i] .. feature_off[i+1]). */
typedef struct {
    uint32_t found;             /* 0: no protein under this id (entry zeroed) */
    uint32_t length;            /* Protein.Length (EMBL: the length the SQ line */
                                /* declares; what was indexed)                 */
    const char *entry_id;       /* Protein.EntryId, entry_id_len bytes         */
    uint32_t entry_id_len;
    uint32_t n_features;
    const uint8_t *sequence;    /* Protein.Sequence, sequence_len bytes        */
    const char *features;
    const uint64_t *feature_off; /* n_features + 1                             */
    uint32_t sequence_len;      /* = length, except for an EMBL entry that     */
                                /* holds more residues than its SQ line        */
                                /* declares: the reference indexes             */
                                /* Sequence[:Length] and stores all of it      */
                                /* (inputEMBL.go:293-312)                      */
    uint32_t reserved;
} kaamer_protein_entry;
/* FetchHitsInformation (search.go:454-470) for n protein ids at once */
int kaamer_fetch_hits(const kaamer_proteins *p, const uint32_t *ids, uint32_t n, kaamer_protein_entry *out);

/* ------------------------------------------------------------------------- */
/* Index handle — replaces the read side of kvstore.KVStoresNew               */
/* (kv_stores.go:46-104) and KVStore.GetValueFromBadger (kv_store.go:179-204): */
/* the table lives in the HBM of one device.                                   */
/* ------------------------------------------------------------------------- */
typedef struct kaamer_index kaamer_index;

int kaamer_index_open_image(const kaamer_image *img, int device, kaamer_index **out);
/* makedb -> serving without an image in between: kaamer_image_build_proteins_device's
 * table stays on `device` and becomes the index. */
int kaamer_index_build_proteins(const uint8_t *seqs, const uint64_t *offsets, const uint32_t *ids,
                                uint32_t n_proteins, uint32_t shard, uint32_t n_shards,
                                double load_factor, int device, kaamer_index **out);
/* text -> table + serving index (kaamer_index_build_proteins' hand-over: the table stays on the device); the reader is
 * kaamer_makedb_fasta_device's */
int kaamer_index_build_fasta(const char *text, uint64_t len, uint32_t shard, uint32_t n_shards, double load_factor,
                             int device, kaamer_proteins **proteins, kaamer_index **out);
/* ... the same from a TSV text (header line first); the reader is kaamer_makedb_tsv_device's */
int kaamer_index_build_tsv(const char *text, uint64_t len, uint32_t shard, uint32_t n_shards, double load_factor,
                           int device, kaamer_proteins **proteins, kaamer_index **out);
/* ... the same from an EMBL text; the reader is kaamer_makedb_embl_device's */
int kaamer_index_build_embl(const char *text, uint64_t len, uint32_t shard, uint32_t n_shards, double load_factor,
                            int device, kaamer_proteins **proteins, kaamer_index **out);
/* ... the same from a GBK text; the reader is kaamer_makedb_gbk_device's */
int kaamer_index_build_gbk(const char *text, uint64_t len, uint32_t shard, uint32_t n_shards, double load_factor,
                           int device, kaamer_proteins **proteins, kaamer_index **out);
int kaamer_index_open(const char *path, int device, kaamer_index **out);
void kaamer_index_close(kaamer_index *ix);
int kaamer_index_get_stats(const kaamer_index *ix, kaamer_image_stats *out);

/* ------------------------------------------------------------------------- */
/* Search — replaces, per query, the block keyChan / KmerSearch /              */
/* StoreMatchPositions / sortMapByValue (search_protein.go:78-105,             */
/* search_fastq.go:94-118, search_nucleotide.go:91-115; search.go:414-452) and,*/
/* for nucleotide input, the preceding GetORFs call (dna.go:65-181;            */
/* search_fastq.go:74, search_nucleotide.go:136).                              */
/* ------------------------------------------------------------------------- */

/* One query handed to KmerSearch: a protein record, or one ORF of a read.     */
typedef struct {
    uint32_t src_seq;        /* index of the input sequence it came from       */
    int32_t size_in_kmer;    /* Query.SizeInKmer (search.go:290-293)           */
    int32_t start_position;  /* Location (dna.go:35-40); proteins: 1           */
    int32_t end_position;    /*                          proteins: len         */
    int32_t plus_strand;
    uint32_t aa_len;         /* residues of Query.Sequence                     */
    uint64_t aa_off;         /* into orf_aa (reads) / the input seqs (protein) */
    uint32_t sa_off, sa_len; /* Location.StartsAlternative, into starts_alt    */
} kaamer_query_meta;

/* Exact work counters of one batch, counted by the kernels themselves.        */
typedef struct {
    uint64_t n_in;       /* input bytes read (residues / nucleotides)          */
    uint64_t n_queries;  /* queries searched (proteins, or ORFs)               */
    uint64_t n_lookup;   /* k-mer lookups = KeyPos handed to KmerSearch        */
    uint64_t n_probe;    /* 64-byte buckets inspected (>= n_lookup)            */
    uint64_t n_found;    /* lookups whose key is present                       */
    uint64_t n_post;     /* postings expanded = sum |index[key]| over found    */
    uint64_t n_hits;     /* (query, protein) result pairs                      */
    uint64_t n_overflow; /* queries counted by the G tier: a table beyond a   */
                         /* wave's LDS arena, or more distinct hits than it    */
    uint64_t n_lists;    /* found lookups resolved through an arena list       */
                         /* (the others carry their single id in the slot)     */
    uint64_t n_list_ids; /* protein ids read from arena lists (<= n_post)      */
} kaamer_counters;

typedef struct {
    const uint8_t *seqs;      /* packed sequences, caller-owned                */
    const uint64_t *offsets;  /* n_seqs + 1                                    */
    uint32_t n_seqs;
    int32_t seq_type;         /* KAAMER_NUCLEOTIDE / PROTEIN / READS, or       */
                              /* KAAMER_SEQ_TYPE(type, genetic code)           */
    int32_t want_positions;   /* SearchOptions.ExtractPositions (search.go:64) */
} kaamer_batch_in;

typedef struct {
    uint32_t n_queries;
    const kaamer_query_meta *q;
    const uint64_t *hit_off;     /* CSR: hits of query i are [hit_off[i],      */
                                 /* hit_off[i+1]); n_queries + 1 entries       */
    const uint32_t *hit_cnt;     /* hits of each query                         */
    const uint32_t *hit_pid;     /* Hit.Key      (search.go:111-115)           */
    const uint32_t *hit_kmatch;  /* Hit.Kmatch; unsorted within a query        */
    const uint32_t *hit_first_pos; /* lowest query position that matched the   */
                                 /* hit: all SetBestStartCodon needs           */
                                 /* (dna.go:225-237)                           */
    const uint64_t *pos_off;     /* per hit, word offset into pos_bits; NULL   */
    const uint64_t *pos_bits;    /* PositionHits bitmaps (search.go:442-452),  */
                                 /* size_in_kmer bits per hit; NULL unless     */
                                 /* want_positions                             */
    const uint8_t *orf_aa;       /* reads/nucleotide: ORF amino-acid strings   */
    const int32_t *starts_alt;
    kaamer_counters counters;
} kaamer_batch_out;

/* May be called from any number of threads on one index (the worker pool of
 * search_protein.go:58-118): a call takes one of four slots -- workspace, staging,
 * stream -- and callers beyond the slots wait for one. */
int kaamer_search_batch(kaamer_index *ix, const kaamer_batch_in *in, kaamer_batch_out **out);
/* the same call with the caller's buffers as direct arguments (the form a cgo shim binds, see the conventions above) */
int kaamer_search_batch_flat(kaamer_index *ix, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs,
                             int32_t seq_type, int32_t want_positions, kaamer_batch_out **out);
void kaamer_batch_free(kaamer_batch_out *out);
/* The call in two halves (the worker pool of search_protein.go:58-118 when the full hit lists are wanted -- -pos reads
 * PositionHits -- without a blocked thread per batch): submit copies the caller's buffers, takes one of the four slots
 * (blocks while all are busy) and enqueues; wait brings the hit lists to the host, repeating the batch from the copy when a
 * workspace bound was too small, and gives the slot back.  A ticket is waited for, or discarded, exactly once. */
typedef struct kaamer_full_ticket kaamer_full_ticket;
int kaamer_submit_batch_flat(kaamer_index *ix, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs,
                             int32_t seq_type, int32_t want_positions, kaamer_full_ticket **ticket);
int kaamer_wait_batch(kaamer_full_ticket *ticket, kaamer_batch_out **out);
void kaamer_full_ticket_discard(kaamer_full_ticket *ticket);

/* ------------------------------------------------------------------------- */
/* Device-resident form of the same call: inputs already in HBM, results left  */
/* in HBM, everything enqueued on the caller's HIP stream, no host sync.       */
/* (Used by bench.py and by callers that pipeline batches; `stream` is a       */
/* hipStream_t passed as void*.)                                               */
/* ------------------------------------------------------------------------- */
typedef struct kaamer_workspace kaamer_workspace;

typedef struct {
    uint64_t max_seq_bytes;  /* largest packed input batch                     */
    uint32_t max_seqs;       /* most input sequences per batch                 */
    uint32_t max_queries;    /* most queries (ORFs) per batch; 0 = derive      */
    uint64_t max_hits;       /* most (query,protein) pairs per batch; 0=derive */
                             /* (from the input size).  It also bounds how far */
                             /* the per-query counting tables may grow on a     */
                             /* database where a k-mer meets several proteins:  */
                             /* every batch leaves the next one's table scale   */
                             /* (hits per k-mer x 1.9, <= 8) on the device, cut */
                             /* to what these arrays hold -- provision ~4 hits  */
                             /* per k-mer of the batch on such a database       */
    uint64_t g_tier_slots;   /* HBM counting-table slots for queries whose     */
                             /* distinct hits exceed the on-chip tiers; 0 = def*/
    int32_t seq_type;        /* KAAMER_PROTEIN, or KAAMER_NUCLEOTIDE / READS   */
                             /* (adds the 6-frame translation buffers); the    */
                             /* genetic-code bits are ignored: the code is the */
                             /* search call's (KAAMER_SEQ_TYPE)                */
    uint32_t first_pos;      /* hit_first_pos: 0 = as the reference fills      */
                             /* PositionHits (nucleotide/reads only,           */
                             /* search.go:416), 1 = always, 2 = never (zeros)  */
    uint32_t want_positions; /* full PositionHits bitmaps (ExtractPositions)   */
    uint32_t compact;        /* 1: finish with the hit lists packed in query   */
                             /* order (hit_off is a CSR offset array, one more */
                             /* scan + copy pass); 0: leave every list where   */
                             /* the counting kernel wrote it (hit_off[q],      */
                             /* hit_cnt[q] address a sparse array)             */
    uint64_t max_pos_words;  /* u64 words of bitmap storage; 0 = 8 x max_hits  */
    uint32_t concurrent_batches; /* batches the caller keeps in flight on this  */
                             /* index at once (other workspaces on other        */
                             /* streams); 0 / 1: a batch has the device to      */
                             /* itself.  With 2 or more the counting kernel of   */
                             /* a protein batch takes ONE workgroup per CU       */
                             /* instead of three, which leaves registers and     */
                             /* wave slots for the neighbours' probe kernels:    */
                             /* -8 % per batch with three in flight, +30 % for a */
                             /* batch that runs alone                            */
    uint32_t reserved;
} kaamer_workspace_opts;

typedef struct {
    uint32_t n_queries_cap;
    const uint32_t *d_n_queries;        /* device scalar                       */
    const kaamer_query_meta *d_q;
    const uint64_t *d_hit_off;          /* first hit of each query; with       */
                                        /* opts.compact also [n] = total (CSR) */
    const uint32_t *d_hit_cnt;          /* n_queries: hits of each query       */
    uint64_t hit_capacity;              /* entries of the three hit arrays     */
    const uint32_t *d_hit_pid;
    const uint32_t *d_hit_kmatch;
    const uint32_t *d_hit_first_pos;
    const uint8_t *d_orf_aa;
    const int32_t *d_starts_alt;
    const kaamer_counters *d_counters;  /* device copy, valid after the stream */
    const uint64_t *d_pos_off;          /* per hit: first word of its bitmap   */
    const uint64_t *d_pos_bits;         /* NULL unless want_positions          */
    const uint64_t *d_pos_base;         /* per query: first word; [n] = total  */
} kaamer_device_result;

int kaamer_workspace_create(kaamer_index *ix, const kaamer_workspace_opts *opts,
                            kaamer_workspace **out);
void kaamer_workspace_free(kaamer_workspace *ws);
int kaamer_search_device(kaamer_index *ix, kaamer_workspace *ws, const uint8_t *d_seqs,
                         const uint64_t *d_offsets, uint32_t n_seqs, uint64_t seq_bytes,
                         int32_t seq_type, void *stream, kaamer_device_result *out);
/* Two-stream form for callers that keep batches in flight: after this call, kaamer_search_device enqueues prep and
 * probe on ITS `stream` argument and everything behind the probe kernel (counting tiers, finalize; kaamer_topn_device
 * follows) on `count_stream`, ordered by events inside the library.  With ONE probe stream shared by all batches and the
 * workspaces' counting stages on one or two count streams, the device always holds one probe kernel (bound by memory
 * requests) next to the counting kernels of earlier batches (bound by latency) instead of whatever mix independent
 * streams drift into.  kaamer_workspace_finish and the exchange calls wait for the counting stage wherever it ran.
 * stream = NULL: back to one stream. */
int kaamer_workspace_set_count_stream(kaamer_workspace *ws, void *count_stream);
/* Sharded index (the table split by hash prefix over several devices): every shard
 * searches the whole batch for the keys it owns, the partial hit lists travel to the
 * query's owner (all-to-all, done by the caller), and the owner merges them here:
 * entries [ent_off[q], ent_off[q+1]) are the partial (protein id, Kmatch, first position)
 * of query q from all shards; Kmatch adds up, first positions take the minimum.
 * Results (CSR) replace the workspace's last result; finish as after a search. */
int kaamer_merge_device(kaamer_workspace *ws, const uint64_t *d_ent_off, const uint32_t *d_pid,
                        const uint32_t *d_kmatch, const uint32_t *d_first_pos, uint32_t n_queries,
                        uint64_t n_entries, void *stream, kaamer_device_result *out);
/* Post-steps of the workspace's last search (or merge) on the device, one wave per
 * query: sortMapByValue (search.go:132-152; ties by ascending protein id),
 * for nucleotide/reads input SetBestStartCodon (dna.go:198-272) with its gate
 * hits[0].Kmatch >= MinKMatch (search_fastq.go:119-123), then FilterResults
 * (search.go:189-220).  Only the hits a caller returns leave the device:
 * max_results entries per query instead of the full hit lists. */
typedef struct {
    double min_k_ratio;        /* SearchOptions.MinKRatio  (default 0.05)      */
    int64_t min_k_match;       /* SearchOptions.MinKMatch  (default 10)        */
    uint32_t max_results;      /* SearchOptions.MaxResults (default 10)        */
    uint32_t best_start_codon; /* 1: SetBestStartCodon first (nucleotide/reads)*/
    const int32_t *d_size_in_kmer; /* device, per query; NULL = the search's   */
                               /* own queries; after a merge: this, or orf_source */
    /* merged results of a sharded index: result i belongs to query             */
    /* q_first + i * q_stride of ANOTHER workspace's last search (the owner's    */
    /* own translation of the batch: rank r owns queries r, r+W, ...), whose     */
    /* ORFs, StartsAlternative and SizeInKmer the post-steps then use            */
    /* (SetBestStartCodon included).  NULL: the workspace's own queries.         */
    const struct kaamer_workspace *orf_source;
    uint32_t q_first, q_stride;
} kaamer_topn_opts;

typedef struct {
    uint32_t max_results;
    const uint32_t *d_top_cnt;        /* per query: hits kept; 0 = not reported */
    const uint32_t *d_top_pid;        /* [q * max_results + r], r < d_top_cnt[q], */
    const uint32_t *d_top_kmatch;     /* in sortMapByValue order                */
    const uint32_t *d_top_first_pos;
    const int32_t *d_trim;            /* residues SetBestStartCodon removed     */
    const int32_t *d_start_position;  /* Location.StartPosition afterwards      */
    const int32_t *d_size_in_kmer;    /* Query.SizeInKmer afterwards            */
} kaamer_topn_result;

int kaamer_topn_device(kaamer_workspace *ws, const kaamer_topn_opts *opts, void *stream,
                       kaamer_topn_result *out);
/* PositionHits (search.go:442-452) of the hits kaamer_topn_device kept, and of those only: the reference fills a bitmap
 * for every hit of a query and prints them for the at most MaxResults hits it reports (search.go:520-522,540-543,
 * 591-594).  Enqueued on `stream` behind kaamer_topn_device (`top` is its result; on the count stream when the
 * workspace's counting stage runs there, like kaamer_topn_device itself).  For every query q with d_top_cnt[q] > 0 and
 * every kept hit r < d_top_cnt[q]:
 *     words_q = ceil(d_pos_bits_len[q] / 64) u64 words at d_pos_bits + d_pos_base[q] + r * words_q,
 *     bit pos set iff d_top_pid[q * max_results + r] is in index[key(pos)], pos in [0, d_pos_bits_len[q]);
 * d_pos_bits_len[q] is the query's SizeInKmer AS SEARCHED -- for an ORF the untrimmed one: the reference stores the
 * positions before SetBestStartCodon and never re-bases them (search_fastq.go:94-123, dna.go:252-270), exactly as
 * d_top_first_pos is relative to the untrimmed ORF -- and 0 for a query that reports nothing (no words either);
 * d_pos_base[n_queries] is the total.
 * max_pos_words: u64 words of bitmap storage (allocated on first use, grow-only); 0 = (residue positions of the
 * workspace / 64 + max_queries) x f, f = min(max_results, 16) for protein and 1 for nucleotide / reads workspaces: room
 * for every query to report f hits.  A batch that needs more is reported as KAAMER_E_CAPACITY by
 * kaamer_workspace_finish, never a partial result.  KAAMER_E_ARG when the workspace's last result is a merge
 * (kaamer_merge_device / kaamer_exchange_merge): the probe results the bitmaps are read from live on the shards. */
typedef struct {
    const uint64_t *d_pos_base;       /* [n_queries + 1] first word of each query's bitmaps */
    const int32_t *d_pos_bits_len;    /* [n_queries] bits per bitmap                        */
    const uint64_t *d_pos_bits;
    uint64_t pos_words_capacity;      /* the bound this call ran with                       */
} kaamer_topn_positions;
int kaamer_topn_positions_device(kaamer_index *ix, kaamer_workspace *ws, const kaamer_topn_result *top, uint64_t max_pos_words,
                                 void *stream, kaamer_topn_positions *out);

/* Host-buffer call that returns what the reference's drivers report
 * (search_protein.go:105-112, search_fastq.go:118-126): the queries FilterResults left
 * with at least one hit, their hits in sortMapByValue order, after SetBestStartCodon
 * for nucleotide / reads input (best_start_codon is set from in->seq_type).  The
 * packing is done on the device: only the reported queries, their hits (CSR) and their
 * ORF residues cross PCIe.  q[i] carries Location.StartPosition, SizeInKmer and the
 * Sequence window (aa_off, aa_len) as they are after SetBestStartCodon; aa_off indexes
 * orf_aa below (nucleotide / reads) or the caller's own input (protein). */
typedef struct {
    uint32_t n_queries;             /* queries (proteins / ORFs) searched      */
    uint32_t n_reported;            /* those with a hit left after the filter  */
    uint32_t max_results;
    const uint32_t *rep_query;      /* [n_reported] index among the n_queries, */
                                    /* ascending (ORFs: the reference's order) */
    const kaamer_query_meta *q;     /* [n_reported]                            */
    const int32_t *trim;            /* residues removed from the ORF head      */
    const uint64_t *top_off;        /* [n_reported + 1] CSR into the arrays    */
    const uint32_t *top_pid;
    const uint32_t *top_kmatch;
    const uint32_t *top_first_pos;  /* relative to the untrimmed ORF; zeros for */
                                    /* protein input (search.go:416)            */
    const uint8_t *orf_aa;          /* reported ORFs' residues, concatenated   */
    kaamer_counters counters;
} kaamer_batch_top;

int kaamer_search_batch_top(kaamer_index *ix, const kaamer_batch_in *in, const kaamer_topn_opts *top,
                            kaamer_batch_top **out);
void kaamer_batch_top_free(kaamer_batch_top *out);

/* The same call in two halves, for callers that keep several batches in flight: the worker pool of
 * search_protein.go:58-118 (N goroutines against shared read-only stores) becomes N callers against one index, each
 * batch on a slot of its own (workspace, stream, pinned staging, result block; KAAMER_HOST_SLOTS of them, default 4).
 * kaamer_search_batch_top is submit + wait and may be called from any number of threads concurrently.
 *   submit  takes a free slot (blocks while all are busy), COPIES the caller's buffers (they are borrowed for the
 *           call only), enqueues host-to-device copy, search, post-steps and ONE device-to-host copy of the packed
 *           result, and returns;
 *   wait    blocks until that batch is done, returns its result (free it with kaamer_batch_top_free) and releases the
 *           slot and the ticket.  A ticket must be waited for exactly once, by any thread. */
typedef struct kaamer_ticket kaamer_ticket;
int kaamer_submit_batch_top(kaamer_index *ix, const kaamer_batch_in *in, const kaamer_topn_opts *top, kaamer_ticket **ticket);
int kaamer_wait_batch_top(kaamer_ticket *ticket, kaamer_batch_top **out);
/* A ticket nobody will wait for (an error between submit and wait on the caller's side): lets the batch run out, drops
 * its result and gives the slot back.  Without it the slot stays busy for good; kaamer_index_close waits for every
 * slot to be given back. */
void kaamer_ticket_discard(kaamer_ticket *ticket);
/* cgo-safe forms: the caller's buffers and SearchOptions.MinKRatio / MinKMatch / MaxResults (search.go:56-71) as direct
 * arguments; best_start_codon follows from seq_type as in the struct forms. */
int kaamer_search_batch_top_flat(kaamer_index *ix, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs,
                                 int32_t seq_type, double min_k_ratio, int64_t min_k_match, uint32_t max_results,
                                 kaamer_batch_top **out);
int kaamer_submit_batch_top_flat(kaamer_index *ix, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs,
                                 int32_t seq_type, double min_k_ratio, int64_t min_k_match, uint32_t max_results,
                                 kaamer_ticket **ticket);

/* The same calls for a request with ExtractPositions (-pos; nucleotide / reads requests always, search.go:416): the
 * PositionHits bitmaps of the REPORTED hits (what FormatPositionsToString is called on, search.go:520-522,540-543,
 * 591-594) ride in the same packed block, so a call still costs one device-to-host copy and at most max_results
 * bitmaps per query cross PCIe instead of one per (query, protein) hit (kaamer_search_batch_flat with want_positions).
 * Arguments and result as the forms above; a ticket is waited for with kaamer_wait_batch_top or dropped with
 * kaamer_ticket_discard.  The bitmap storage is a bound like every other (kaamer_topn_positions_device states the
 * rule): a batch beyond it is repeated with a larger one inside the call. */
int kaamer_search_batch_top_pos_flat(kaamer_index *ix, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs,
                                     int32_t seq_type, double min_k_ratio, int64_t min_k_match, uint32_t max_results,
                                     kaamer_batch_top **out);
int kaamer_submit_batch_top_pos_flat(kaamer_index *ix, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs,
                                     int32_t seq_type, double min_k_ratio, int64_t min_k_match, uint32_t max_results,
                                     kaamer_ticket **ticket);
/* The bitmaps of a result (kaamer_batch_top itself is unchanged): reported query i has pos_bits_len[i] bits per bitmap --
 * its SizeInKmer as searched, for an ORF the untrimmed one (q[i].size_in_kmer is the trimmed one; top_first_pos is
 * relative to the same untrimmed ORF) -- and entry e of the CSR arrays (top_pid[e], ...) has its
 * ceil(pos_bits_len[i] / 64) words at pos_bits + pos_off[e]; pos_off has top_off[n_reported] + 1 entries, the last one
 * the total.  All three are NULL for a result that was not asked for positions (on the sharded handle: every result
 * but those of kaamer_sharded_search_batch_top_pos_flat / kaamer_sharded_submit_batch_top_pos_flat); they live as long
 * as the result does. */
int kaamer_batch_top_positions(const kaamer_batch_top *out, const int32_t **pos_bits_len, const uint64_t **pos_off,
                               const uint64_t **pos_bits);
/* The FIRST bitmap bound (u64 words) of the host calls above on this index, for callers who know how densely their
 * batches report; 0 (default): the rule.  A batch beyond it is repeated with the rule's bound. */
int kaamer_index_set_top_positions_bound(kaamer_index *ix, uint64_t words);

/* Streaming (BASELINE configs[4]: reads streamed host -> GPU with double-buffered copies): a FIFO of batches with
 * fixed options.  push copies chunk i + 1 and starts it while chunk i is still being searched; pop returns the
 * oldest chunk's reported hits.  push returns KAAMER_E_BUSY instead of blocking when every slot holds one of this
 * stream's own chunks: pop first.  One thread per stream; several streams may share an index. */
typedef struct kaamer_stream kaamer_stream;
int kaamer_stream_open(kaamer_index *ix, int32_t seq_type, const kaamer_topn_opts *top, kaamer_stream **out);
int kaamer_stream_open_flat(kaamer_index *ix, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                            uint32_t max_results, kaamer_stream **out);
/* a stream whose results carry the bitmaps of the reported hits (kaamer_batch_top_positions); push / pop / close as above */
int kaamer_stream_open_pos_flat(kaamer_index *ix, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                uint32_t max_results, kaamer_stream **out);
/* ... and the alignment of every reported hit (FastqSearch / ProteinSearch with -aln chunk by chunk, search_fastq.go:60-136 +
 * search.go:483-494): a push goes the way kaamer_submit_batch_top_aln_flat goes, arguments as there; pop returns a block
 * that kaamer_batch_top_alignments (and, with want_positions, kaamer_batch_top_positions) read.  KAAMER_E_ARG when no
 * table is attached to the index (kaamer_index_attach_proteins, declared below). */
int kaamer_stream_open_aln_flat(kaamer_index *ix, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                uint32_t max_results, int32_t want_positions, const char *sub_matrix, int32_t gap_open,
                                int32_t gap_extend, int32_t want_text, kaamer_stream **out);
int kaamer_stream_push(kaamer_stream *st, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs);
int kaamer_stream_pop(kaamer_stream *st, kaamer_batch_top **out);
uint32_t kaamer_stream_pending(const kaamer_stream *st);
void kaamer_stream_close(kaamer_stream *st);

/* ------------------------------------------------------------------------- */
/* Sharded index, the exchange step as device code (no reference counterpart:  */
/* kaamer is one process; the result must equal the per-query block            */
/* search_fastq.go:94-118 / search_protein.go:78-105 run against the whole DB). */
/* One process per GPU; rank r holds shard r (kaamer_image_build_* (r, W)),     */
/* every rank searches the WHOLE batch (nucleotide input: every rank            */
/* translates, so all ranks number the ORFs alike), query q is owned by rank    */
/* q mod W.  Per batch, on the caller's stream and without host synchronisation: */
/*   kaamer_search_device(shard)           partial hit lists of all queries      */
/*   kaamer_exchange_pack                  -> W fixed-size blocks, one per owner  */
/*   all-to-all with equal splits          grouped ncclSend/ncclRecv (RCCL over   */
/*                                         xGMI), the caller's communicator, or   */
/*                                         kaamer_rccl_alltoall below             */
/*   kaamer_exchange_merge(owner ws)       received blocks -> merged hit lists of  */
/*                                         the owned queries (integer sums: bit-   */
/*                                         identical to the one-device result)     */
/*   kaamer_topn_device(owner ws, orf_source = the search workspace, q_first =     */
/*                      rank, q_stride = W)                                        */
/* Block capacities are bounds like every workspace bound: exceeding them is      */
/* reported as KAAMER_E_CAPACITY by kaamer_workspace_finish, never a partial       */
/* result.  First positions travel only when the search workspace computes them    */
/* (opts.first_pos = 1, or nucleotide / reads input); create the owner's merge      */
/* workspace with the same explicit setting (1 or 2) -- an owner that wants them    */
/* and receives blocks without them reports the same error.                         */
/* ------------------------------------------------------------------------- */
typedef struct {
    uint32_t world, rank;
    uint32_t q_cap;        /* owned queries a block can describe                 */
    uint32_t arrays;       /* entry arrays in a block: 3 = id, Kmatch, first     */
                           /* position; 2 = no first positions (0 reads as 3);   */
                           /* 4 = the three + PositionHits bitmaps (below)       */
    uint64_t e_cap;        /* partial (id, Kmatch, first position) entries/block */
    uint64_t block_words;  /* u32 words per block; send / receive buffers hold   */
                           /* world blocks                                       */
} kaamer_exchange_layout;

/* max_queries: the search workspace's query capacity (kaamer_workspace_query_capacity).  This is the CAPACITY layout:
 * send / receive buffers hold world * block_words words of it. */
int kaamer_exchange_layout_init(uint32_t world, uint32_t rank, uint32_t max_queries,
                                uint64_t max_entries_per_peer, kaamer_exchange_layout *out);
/* The layout of ONE batch inside the same buffers: blocks for n_queries queries of the batch and entries_per_block
 * partial entries (both cut to the capacity layout), without room for first positions when the workspaces do not
 * compute them (with_first_pos = 0: first_pos = 2 on both workspaces).  What the all-to-all moves is world blocks of THIS layout's
 * block_words, contiguous from the start of the buffers -- payload, not capacity.  Every rank must use the same layout
 * for a batch: derive the two figures from kaamer_exchange_stats of an earlier batch (identical on all ranks) plus a
 * margin; a batch that does not fit fails on every rank with KAAMER_E_CAPACITY and is repeated with the capacity
 * layout. */
int kaamer_exchange_layout_fit(const kaamer_exchange_layout *capacity, uint32_t n_queries, uint64_t entries_per_block,
                               int32_t with_first_pos, kaamer_exchange_layout *out);
/* What the W block headers of an earlier kaamer_exchange_merge on `merge_ws` said, the same on every rank:
 * out = { merge sequence number, queries of the batch, entries the largest block between ANY pair of ranks needed,
 * non-zero if a block overflowed }.  back = 0: the last merge enqueued, 1: the one before.  Waits for that merge's
 * header scan only (an event), not for the stream. */
int kaamer_exchange_stats(kaamer_workspace *merge_ws, uint32_t back, uint64_t out[4]);
uint32_t kaamer_workspace_query_capacity(const kaamer_workspace *ws);
/* The prefix scan behind every offset array of a workspace (hit offsets, bitmap bases, pair offsets, piece offsets; tests
 * put their boundary cases there): out[0] threads per workgroup, out[1] counts per thread, out[2] counts per tile
 * (out[0] * out[1]), out[3] the greatest bound -- the batch's sequence count, the workspace's query capacity or the piece
 * bound, by caller -- that one workgroup scans tile after tile with a carry; above it three launches scan one tile per
 * workgroup. */
void kaamer_scan_geometry(uint32_t out[4]);
/* Blocks that carry PositionHits (search.go:442-452; -pos, cmd/kaamer/main.go:69) through the exchange: arrays = 4.
 * The block is the arrays = 3 block with two more sections:
 *     [8 + q_cap .. 8 + 2 q_cap)  per owned query: SizeInKmer (every shard translates alike: the W blocks must agree)
 *     then pid, kmatch, first_pos [e_cap] each as before, then, from u32 word
 *         bits_off = (8 + 2 q_cap + 3 e_cap) rounded up to an even word  (8-byte aligned),
 *     p_cap = (block_words - bits_off) / 2 u64 words of bitmaps: entry j of owned query i has ceil(SizeInKmer_i / 64)
 *     words at bits_off + 2 (bbase[i] + j words_i), bbase = exclusive scan of entries_i x words_i.
 * Header word [6] = bitmap words this block needed, [7] = the largest [6] over the sender's W blocks, status bit 4 =
 * bitmaps inside.  A bitmap section that does not fit sets the overflow bits as the entries do (KAAMER_E_CAPACITY on
 * every rank).  Both workspaces need want_positions = 1 and first_pos = 1; the merge ORs each received bitmap into its
 * merged hit's (the shards' bitmaps of one hit are disjoint: bit-identical to the unsharded search) and returns them in
 * kaamer_device_result.d_pos_off / d_pos_bits / d_pos_base as a search does. */
int kaamer_exchange_layout_init_positions(uint32_t world, uint32_t rank, uint32_t max_queries, uint64_t max_entries_per_peer,
                                          uint64_t max_pos_words_per_peer, kaamer_exchange_layout *out);
/* the payload-sized layout of one batch (kaamer_exchange_layout_fit) with room for pos_words_per_block bitmap words;
 * `capacity` must be an arrays = 4 layout; never beyond it */
int kaamer_exchange_layout_fit_positions(const kaamer_exchange_layout *capacity, uint32_t n_queries, uint64_t entries_per_block,
                                         uint64_t pos_words_per_block, kaamer_exchange_layout *out);
/* the bitmap half of kaamer_exchange_stats: out = { bitmap words the largest block between ANY pair of ranks needed,
 * non-zero if a bitmap section overflowed } (zeros after a merge of blocks without bitmaps) */
int kaamer_exchange_stats_positions(kaamer_workspace *merge_ws, uint32_t back, uint64_t out[2]);
/* the last search of `search_ws` -> d_send[world * block_words] */
int kaamer_exchange_pack(kaamer_workspace *search_ws, const kaamer_exchange_layout *layout,
                         uint32_t *d_send, void *stream);
/* d_recv[world * block_words] (block s = what rank s sent to this rank) -> merged results in
 * `merge_ws` (max_queries >= layout->q_cap, max_hits >= world * layout->e_cap, first_pos = 1 or 2: the same explicit
 * setting as the search workspace).  Blocks whose headers do not describe ONE batch (ranks on different batches, a
 * stale buffer), blocks that overflowed, and blocks of a sender whose own search failed all make the merge an error
 * (KAAMER_E_CAPACITY at kaamer_workspace_finish): never a partial result. */
int kaamer_exchange_merge(kaamer_workspace *merge_ws, const kaamer_exchange_layout *layout,
                          const uint32_t *d_recv, void *stream, kaamer_device_result *out);
/* Grouped ncclSend / ncclRecv of world equal blocks on `stream` with the caller's ncclComm_t.
 * The library does not link RCCL: the symbols are taken from the process (or librccl.so.1). */
int kaamer_rccl_alltoall(void *nccl_comm, const void *d_send, void *d_recv, uint64_t bytes_per_peer,
                         uint32_t world, void *stream);

/* ------------------------------------------------------------------------- */
/* One process, one handle, several devices: the reference server   */
/* is ONE process that opens its stores once and fans out goroutines            */
/* (api/server.go:47-65, search_fastq.go:60-66).  image i / paths[i] is shard i  */
/* of n_shards (kaamer_image_build_* (i, n_shards)) and is made resident on      */
/* devices[i] (the same device may appear more than once).  A call drives all    */
/* shards from the calling thread: every shard searches the whole batch for the  */
/* keys it owns, every owner (query q: shard q mod n_shards) pulls its blocks     */
/* with peer copies over xGMI, merges, runs the post-steps; the reported queries  */
/* come back in batch order, exactly what kaamer_search_batch_top returns on an   */
/* unsharded index.  No communicator, no second process.  Any number of threads   */
/* may call on one handle: a call takes one of three sets of per-shard            */
/* workspaces, buffers and streams; callers beyond the sets wait for one.         */
/* ------------------------------------------------------------------------- */
typedef struct kaamer_sharded_index kaamer_sharded_index;
int kaamer_index_open_sharded(const char *const *paths, const int *devices, uint32_t n_shards, kaamer_sharded_index **out);
int kaamer_index_open_sharded_images(const kaamer_image *const *images, const int *devices, uint32_t n_shards,
                                     kaamer_sharded_index **out);
uint32_t kaamer_sharded_index_shards(const kaamer_sharded_index *sx);
void kaamer_sharded_index_close(kaamer_sharded_index *sx);
int kaamer_sharded_search_batch_top(kaamer_sharded_index *sx, const kaamer_batch_in *in, const kaamer_topn_opts *top,
                                    kaamer_batch_top **out);
/* The call in two halves (the worker pool of search_protein.go:58-118 against one sharded handle without a blocked
 * thread per batch): submit takes a free set, copies the caller's buffers, enqueues the batch on every device and
 * returns; wait collects the result (repeating the batch from the staging copy when a bound was too small) and gives
 * the set back.  A ticket is waited for, or discarded, exactly once. */
typedef struct kaamer_sharded_ticket kaamer_sharded_ticket;
int kaamer_sharded_submit_batch_top(kaamer_sharded_index *sx, const kaamer_batch_in *in, const kaamer_topn_opts *top,
                                    kaamer_sharded_ticket **ticket);
int kaamer_sharded_wait_batch_top(kaamer_sharded_ticket *ticket, kaamer_batch_top **out);
void kaamer_sharded_ticket_discard(kaamer_sharded_ticket *ticket);
/* cgo-safe forms (see the conventions at the top) */
int kaamer_sharded_search_batch_top_flat(kaamer_sharded_index *sx, const uint8_t *seqs, const uint64_t *offsets,
                                         uint32_t n_seqs, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                         uint32_t max_results, kaamer_batch_top **out);
int kaamer_sharded_submit_batch_top_flat(kaamer_sharded_index *sx, const uint8_t *seqs, const uint64_t *offsets,
                                         uint32_t n_seqs, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                         uint32_t max_results, kaamer_sharded_ticket **ticket);
/* The same calls for a request with ExtractPositions (-pos; nucleotide / reads requests always, search.go:416): the
 * PositionHits bitmaps of the REPORTED hits (search.go:442-452 fills them, search.go:520-522,540-543,591-594 prints
 * them: at most max_results per query), bit for bit what kaamer_search_batch_top_pos_flat returns on an unsharded index
 * of the whole database; read them with kaamer_batch_top_positions.  The reported hits are known at the owner after
 * the merge while the probe results live on the shards, so one more round trip follows the top-N step on the same
 * streams: every owner sends the ids of its reported hits to every shard, every shard makes the bitmaps its own keys
 * give, the owner ORs the W parts (disjoint) into its result block.  Only the reported hits' bitmaps cross devices
 * (kaamer_sharded_search_batch_flat with want_positions moves those of every hit).  The ids blocks and the bitmap
 * segments are bounds like every other (the rule of kaamer_topn_positions_device, divided over the owners; sized from
 * the previous call's need when there was one): a batch beyond them is repeated inside the wait, never returned in
 * part.  A ticket is waited for with kaamer_sharded_wait_batch_top or dropped with kaamer_sharded_ticket_discard. */
int kaamer_sharded_search_batch_top_pos_flat(kaamer_sharded_index *sx, const uint8_t *seqs, const uint64_t *offsets,
                                             uint32_t n_seqs, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                             uint32_t max_results, kaamer_batch_top **out);
int kaamer_sharded_submit_batch_top_pos_flat(kaamer_sharded_index *sx, const uint8_t *seqs, const uint64_t *offsets,
                                             uint32_t n_seqs, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                             uint32_t max_results, kaamer_sharded_ticket **ticket);
/* That round trip of the last finished call with positions on the handle's first set (no Go counterpart: the reference
 * is one process, search_fastq.go:94-118): out = { bytes of one ids block as it travelled, bytes of one (shard ->
 * owner) bitmap segment as it travelled, bitmap words the largest segment needed, attempts the call took }. */
int kaamer_sharded_positions_info(kaamer_sharded_index *sx, uint64_t out[4]);
/* The full hit lists of a batch on the sharded handle: what kaamer_search_batch returns on an unsharded index of the
 * whole database (the worker pool of search_protein.go:58-118 / search_fastq.go:94-118 when -pos asks for
 * PositionHits, search.go:416,442-452): the same queries in the same order, each with the same (id, Kmatch, first
 * position) set (unordered within a query, as there), the same q / orf_aa / starts_alt and, with want_positions, the
 * same bitmaps.  Every shard searches and packs, every owner merges, compacts and copies its queries back; the host
 * interleaves them into batch order.  Free the result with kaamer_batch_free. */
int kaamer_sharded_search_batch(kaamer_sharded_index *sx, const kaamer_batch_in *in, kaamer_batch_out **out);
int kaamer_sharded_search_batch_flat(kaamer_sharded_index *sx, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs,
                                     int32_t seq_type, int32_t want_positions, kaamer_batch_out **out);
/* in two halves, as kaamer_submit_batch_flat / kaamer_wait_batch (wait repeats the batch from the staging copy with
 * grown bounds when one was too small) */
typedef struct kaamer_sharded_full_ticket kaamer_sharded_full_ticket;
int kaamer_sharded_submit_batch_flat(kaamer_sharded_index *sx, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs,
                                     int32_t seq_type, int32_t want_positions, kaamer_sharded_full_ticket **ticket);
int kaamer_sharded_wait_batch(kaamer_sharded_full_ticket *ticket, kaamer_batch_out **out);
void kaamer_sharded_full_ticket_discard(kaamer_sharded_full_ticket *ticket);
/* The exchange of the last finished call on the handle's first set: out = { bytes of one (shard -> owner) block as it
 * travelled, entries the largest block needed, queries of the batch, 1 if the blocks were sized from the previous
 * call's need (payload) rather than the buffers' capacity }. */
int kaamer_sharded_exchange_info(kaamer_sharded_index *sx, uint64_t out[4]);

/* ------------------------------------------------------------------------- */
/* One process, the same database on several devices (SURVEY 8e "replicas only": */
/* a database that fits one device is not sharded, the query stream is split;     */
/* BASELINE configs[4]).  The reference is ONE server process (api/server.go:47-65) */
/* whose FastqSearch takes a file (search_fastq.go:60-136).                        */
/* ------------------------------------------------------------------------- */
typedef struct kaamer_replicas kaamer_replicas;
/* the image is read once and made resident on every devices[i] */
int kaamer_index_open_replicas(const char *path, const int *devices, uint32_t n, kaamer_replicas **out);
int kaamer_index_open_replicas_image(const kaamer_image *img, const int *devices, uint32_t n, kaamer_replicas **out);
uint32_t kaamer_replicas_count(const kaamer_replicas *r);
kaamer_index *kaamer_replicas_index(const kaamer_replicas *r, uint32_t i);   /* replica i: every single-index call works on it */
void kaamer_replicas_close(kaamer_replicas *r);
/* A FIFO of chunks over the set: chunk k goes to replica k mod n (its own slots, stream and staging), pop returns the
 * chunks in push order.  push returns KAAMER_E_BUSY when every slot of the replica whose turn it is holds one of this
 * stream's chunks: pop first.  One thread per stream. */
typedef struct kaamer_replica_stream kaamer_replica_stream;
int kaamer_replica_stream_open_flat(kaamer_replicas *r, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                    uint32_t max_results, kaamer_replica_stream **out);
int kaamer_replica_stream_push(kaamer_replica_stream *rs, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs);
int kaamer_replica_stream_pop(kaamer_replica_stream *rs, kaamer_batch_top **out);
uint32_t kaamer_replica_stream_pending(const kaamer_replica_stream *rs);
void kaamer_replica_stream_close(kaamer_replica_stream *rs);
/* FastqSearch / ProteinSearch over a FILE of any size (search_fastq.go:60-136, search_protein.go:40-118: reader ->
 * queryChan -> workers -> result handler): kaamer_reader_* (incremental, gzip; strict_scanner as there) feeds chunks of
 * at most chunk_seqs records / about chunk_bytes of sequence round-robin to the replicas, up to in_flight chunks per
 * replica in flight (0: three); `cb` is called once per chunk, in input order, with the chunk's records and its
 * reported hits (both valid during the call only); first_seq = index of the chunk's first record in the file;
 * rep_query / q[].src_seq of `top` count from the chunk's first record.  A non-zero return of cb stops the run.
 * `total` (may be NULL) receives the summed work counters.  Memory: in_flight x replicas chunks, whatever the file size. */
typedef int (*kaamer_chunk_cb)(void *user, uint64_t first_seq, const kaamer_reads *chunk, const kaamer_batch_top *top);
int kaamer_search_file(kaamer_replicas *r, const char *path, int format, int strict_scanner, int32_t seq_type,
                       double min_k_ratio, int64_t min_k_match, uint32_t max_results, uint32_t chunk_seqs,
                       uint64_t chunk_bytes, uint32_t in_flight, kaamer_chunk_cb cb, void *user, kaamer_counters *total);

/* The same drivers for a request with -pos (search.go:416,442-452,520-522) and -aln (search.go:454-470,483-494).
 * kaamer_replicas_attach_proteins: kaamer_index_attach_proteins on every replica, the same rules (the table is borrowed,
 * a second attach replaces the first, not while calls are in flight); a failure on replica i is reported as such and
 * leaves replicas 0 .. i-1 attached. */
int kaamer_replicas_attach_proteins(kaamer_replicas *r, const kaamer_proteins *p);
/* replica streams whose chunks carry the bitmaps (kaamer_stream_open_pos_flat on every replica) and the alignments
 * (kaamer_stream_open_aln_flat on every replica) of the reported hits; push / pop / pending / close as above */
int kaamer_replica_stream_open_pos_flat(kaamer_replicas *r, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                        uint32_t max_results, kaamer_replica_stream **out);
int kaamer_replica_stream_open_aln_flat(kaamer_replicas *r, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                        uint32_t max_results, int32_t want_positions, const char *sub_matrix,
                                        int32_t gap_open, int32_t gap_extend, int32_t want_text, kaamer_replica_stream **out);
/* kaamer_search_file for such a request (FastqSearch / ProteinSearch / NucleotideSearch over a file with -pos / -aln,
 * search_fastq.go:60-136, search_protein.go:40-118, search_nucleotide.go:27-160): want_positions != 0: `top` of the
 * callback carries the chunk's bitmaps (kaamer_batch_top_positions); want_aln != 0: its alignments
 * (kaamer_batch_top_alignments; sub_matrix / gap_open / gap_extend / want_text as kaamer_search_batch_top_aln_flat takes
 * them, sub_matrix may be NULL otherwise), hits in BitScore order.  Everything else as kaamer_search_file, which is this
 * call with both switched off. */
int kaamer_search_file_opts(kaamer_replicas *r, const char *path, int format, int strict_scanner, int32_t seq_type,
                            double min_k_ratio, int64_t min_k_match, uint32_t max_results, int32_t want_positions,
                            int32_t want_aln, const char *sub_matrix, int32_t gap_open, int32_t gap_extend, int32_t want_text,
                            uint32_t chunk_seqs, uint64_t chunk_bytes, uint32_t in_flight, kaamer_chunk_cb cb, void *user,
                            kaamer_counters *total);

/* ------------------------------------------------------------------------- */
/* The same two drivers on the one-process sharded handle: a database larger    */
/* than one device behind FastqSearch / ProteinSearch / NucleotideSearch over a  */
/* file of any size (search_fastq.go:60-136, search_protein.go:40-118,            */
/* search_nucleotide.go:27-160; BASELINE configs[3]).                              */
/* ------------------------------------------------------------------------- */
/* A FIFO of kaamer_sharded_ticket with fixed options, the contract of kaamer_stream_*: push copies the chunk and starts
 * it on a free set of the handle, pop is kaamer_sharded_wait_batch_top on the oldest chunk (a chunk beyond a bound is
 * repeated inside it; a chunk whose wait fails is consumed), close lets run out and drops what nobody popped.  The
 * handle has KAAMER_SHARDED_SETS sets: push returns KAAMER_E_BUSY, without waiting, when the stream holds that many
 * chunks, or when it holds at least one and other callers hold the rest: pop first.  A stream that holds nothing waits
 * for a set like any other caller.  One thread per stream; other threads may go on calling the handle.  The _pos form's
 * results carry the bitmaps of the reported hits (kaamer_sharded_submit_batch_top_pos_flat per chunk), the _aln form's
 * their alignments (kaamer_sharded_submit_batch_top_aln_flat per chunk; KAAMER_E_ARG when no table is attached);
 * kaamer_sharded_index_attach_proteins returns KAAMER_E_BUSY while a stream holds a chunk. */
#define KAAMER_SHARDED_SETS 3
typedef struct kaamer_sharded_stream kaamer_sharded_stream;
int kaamer_sharded_stream_open_flat(kaamer_sharded_index *sx, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                    uint32_t max_results, kaamer_sharded_stream **out);
int kaamer_sharded_stream_open_pos_flat(kaamer_sharded_index *sx, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                        uint32_t max_results, kaamer_sharded_stream **out);
int kaamer_sharded_stream_open_aln_flat(kaamer_sharded_index *sx, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                        uint32_t max_results, int32_t want_positions, const char *sub_matrix,
                                        int32_t gap_open, int32_t gap_extend, int32_t want_text, kaamer_sharded_stream **out);
int kaamer_sharded_stream_push(kaamer_sharded_stream *st, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs);
int kaamer_sharded_stream_pop(kaamer_sharded_stream *st, kaamer_batch_top **out);
uint32_t kaamer_sharded_stream_pending(const kaamer_sharded_stream *st);
void kaamer_sharded_stream_close(kaamer_sharded_stream *st);
/* kaamer_search_file_opts on the sharded handle: same arguments, same callback (rep_query / q[].src_seq of `top` count
 * from the chunk's first record), same result as on an unsharded index of the whole database.  in_flight counts chunks
 * per HANDLE: 0 means 3, more than KAAMER_SHARDED_SETS is cut to that. */
int kaamer_sharded_search_file(kaamer_sharded_index *sx, const char *path, int format, int strict_scanner, int32_t seq_type,
                               double min_k_ratio, int64_t min_k_match, uint32_t max_results, int32_t want_positions,
                               int32_t want_aln, const char *sub_matrix, int32_t gap_open, int32_t gap_extend,
                               int32_t want_text, uint32_t chunk_seqs, uint64_t chunk_bytes, uint32_t in_flight,
                               kaamer_chunk_cb cb, void *user, kaamer_counters *total);

/* Waits for `stream`, copies the counters to the host and reports a deferred
 * KAAMER_E_CAPACITY if a device-side bound was exceeded during the batch. */
int kaamer_workspace_finish(kaamer_workspace *ws, void *stream, kaamer_counters *out);
/* Kernel timers.  kaamer_workspace_set_timing(ws, k): k = 0 (default) records no
 * events; k >= 1 brackets the kernels of every k-th kaamer_search_device call with
 * HIP events on the caller's stream (each record idles the stream for a few
 * microseconds, hence the sampling).  kaamer_workspace_kernel_ms_sum returns the
 * times (ms) summed over the n_calls sampled calls since the previous
 * kaamer_workspace_reset_timers (at most 1024 are kept):
 *   probe_ms  the probe kernel (the dominant kernel: one 64-B bucket per lookup)
 *   count_ms  the counting tiers (postings expansion + per-protein counting)
 *   total_ms  the whole batch, prep to CSR
 * The stream must have been synchronised (kaamer_workspace_finish does). */
int kaamer_workspace_kernel_ms_sum(kaamer_workspace *ws, double *probe_ms, double *count_ms,
                                   double *total_ms, uint32_t *n_calls);
void kaamer_workspace_reset_timers(kaamer_workspace *ws);
void kaamer_workspace_set_timing(kaamer_workspace *ws, uint32_t every);

/* ------------------------------------------------------------------------- */
/* Host post-steps kept bit-compatible with the reference (they stay on the    */
/* host in the Go integration; exported so non-Go callers get the same         */
/* results).                                                                   */
/* ------------------------------------------------------------------------- */
/* QueryResult.FilterResults, search.go:189-220: hits sorted by Kmatch desc;
 * returns how many (a prefix) survive MinKRatio / MinKMatch / MaxResults.     */
int64_t kaamer_filter_results(const uint32_t *kmatch_sorted, int64_t n_hits, int32_t size_in_kmer,
                              double min_k_ratio, int64_t min_k_match, int64_t max_results);
/* sortMapByValue, search.go:132-152: order hit indices by Kmatch descending;
 * ties (nondeterministic in the reference) are broken by ascending protein id. */
void kaamer_sort_hits(const uint32_t *pid, const uint32_t *kmatch, int64_t n_hits, uint32_t *order);
/* FormatPositionsToString, search.go:694-742, byte for byte, on one bitmap of n_bits positions (bit pos of word
 * pos / 64): the maximal runs of set positions as "start-end", comma separated, 1-based, where end is ONE PAST the run's
 * last set position (the reference closes a run at the first unset position and prints that position's number), or
 * n_bits for a run that reaches the end; with_alignment adds KAAMER_KMER_SIZE - 1 to every end (the residues the last
 * k-mer covers).  Writes at most cap bytes into buf, NUL-terminated when cap > 0, and returns the length of the whole
 * string without the NUL: a return >= cap means buf was too short.  buf may be NULL with cap 0.  (The TSV writer's hit
 * count, strings.Count(posString, ","), is derived from the string by the caller -- or the whole row is written by
 * kaamer_format_tsv / the *_tsv_flat calls, at the end of this file.) */
uint64_t kaamer_format_positions(const uint64_t *bits, int32_t n_bits, int32_t with_alignment, char *buf, uint64_t cap);

/* SetBestStartCodon, dna.go:198-272: hits in sortMapByValue order with their first
 * matching positions; trims the ORF to the start codon preceding the first best-hit
 * position.  Returns the residues trimmed (0 = unchanged); start_position and
 * size_in_kmer are updated like dna.go:252-267. */
int32_t kaamer_set_best_start_codon(const uint32_t *kmatch_sorted, const uint32_t *first_pos_sorted,
                                    int64_t n_hits, const int32_t *starts_alt, int32_t n_starts,
                                    int32_t plus_strand, const uint8_t *orf_aa, uint32_t aa_len,
                                    int32_t *start_position, int32_t *size_in_kmer);

/* ------------------------------------------------------------------------- */
/* Alignment of the reported hits (`-aln`) — replaces, for all (query, hit) pairs */
/* of a batch at once, the loop of QueryResultHandler (search.go:483-494) over     */
/* align.Align (pkg/align/align.go:46-161): local alignment with affine gaps on    */
/* the device (one lane per pair), then the reference's own arithmetic on the host: */
/* Identity / Similarity (float32), Length, Mismatches, GapOpenings, Raw, BitScore  */
/* = (lambda * Raw - ln K) / ln 2, EValue = len(query) * NumberOfAA / 2^BitScore,    */
/* the 1-based inclusive coordinates and AlnString's three rows.                    */
/* The aligner itself is github.com/biogo/biogo v1.0.1 (align.SWAffine on          */
/* matrix.BLOSUM62 with GapOpen -11, align.go:62-67 -- fixed, whatever the options   */
/* are), which is not part of the reference tree: the recurrence is restated from    */
/* its published algorithm and its tie-breaking is not pinned by anything in the     */
/* reference.                                                  */
/* ------------------------------------------------------------------------- */
typedef struct {
    float identity, similarity;   /* AlignmentResult.Identity / .Similarity (percent, float32)     */
    int32_t length;               /* columns of the alignment = len of each row of AlnString        */
    int32_t mismatches, gap_openings, raw;
    double bitscore, evalue;
    int32_t query_start, query_end, subject_start, subject_end;   /* 1-based, inclusive             */
    uint64_t aln_off;             /* into kaamer_alignments_text: query row, match row, subject row, */
                                  /* `length` bytes each (AlnString joins them with '\n')            */
    int32_t status;               /* 0 aligned; 1 "No matrix found" (GetMatrixScores: the reference  */
                                  /* keeps an empty AlignmentResult; also any matrix but BLOSUM62,    */
                                  /* whose data the similarity marks need); 2 a letter outside the    */
                                  /* protein alphabet "-ABCDEFGHIJKLMNPQRSTVWXYZ*" (SWAffine fails);   */
                                  /* 3 a sequence too long                                            */
    int32_t reserved;
} kaamer_alignment;
typedef struct kaamer_alignments kaamer_alignments;
/* pair i aligns sequence pair_query[i] (the Query.Sequence) with sequence pair_subject[i] (the hit's Protein.Sequence) of
 * the packed buffer (seqs, offsets[n_seqs + 1]); number_of_aa = KStats.NumberOfAA (kaamer_proteins_stats); sub_matrix /
 * gap_open / gap_extend = SearchOptions.SubMatrix / GapOpen / GapExtend (defaults "blosum62", 11, 1: api/server.go:149-151).
 * All caller buffers are direct arguments (cgo-safe).  Results in pair order. */
int kaamer_align_pairs(int device, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs,
                       const uint32_t *pair_query, const uint32_t *pair_subject, uint32_t n_pairs,
                       uint64_t number_of_aa, const char *sub_matrix, int32_t gap_open, int32_t gap_extend,
                       kaamer_alignments **out);
uint32_t kaamer_alignments_count(const kaamer_alignments *a);
const kaamer_alignment *kaamer_alignments_items(const kaamer_alignments *a);
const char *kaamer_alignments_text(const kaamer_alignments *a);
void kaamer_alignments_free(kaamer_alignments *a);
/* GetMatrixScores (matrixScores.go:107-115): KAAMER_E_ARG ("No matrix found") when the table has no such row */
int kaamer_align_matrix_scores(const char *sub_matrix, int32_t gap_open, int32_t gap_extend, double *lambda, double *k);
/* GetAlnScoreAA on BLOSUM62 (matrixScores.go:125-127): letters of AAPosInMatrix, anything else reads as '-' */
int32_t kaamer_align_matrix_entry(int32_t a, int32_t b);

/* ------------------------------------------------------------------------- */
/* Alignment of the reported hits INSIDE the top-N call (`-aln` in one call):     */
/* QueryResultHandler (search.go:483-494) aligns every reported hit with its query */
/* (align.Align(query.Sequence, HitEntries[hit.Key].Sequence, ...)) and re-sorts    */
/* the hits by BitScore (search.go:492).  With the database's Protein.Sequence      */
/* table resident next to the index, the alignment of the reported hits is enqueued  */
/* behind kaamer_topn_device on the same stream: no download of the hits, no lookup, */
/* no packing, no upload, no rounds in between; only the per-pair integers and, on   */
/* request, the operations come back, in the same packed block.  Matrix, gap column  */
/* and tie rules are kaamer_align_pairs' own (one statement, align.hip); the numbers  */
/* equal that call's bit for bit.  On one device, and on the one-process sharded       */
/* handle (below).  kaamer_stream_open_aln_flat, kaamer_replica_stream_open_aln_flat,   */
/* kaamer_search_file_opts and the sharded stream / file driver put the same call        */
/* behind a FIFO and a file reader.                                                       */
/* ------------------------------------------------------------------------- */
/* HitEntries (FetchHitsInformation, search.go:454-470) made resident: every entry's stored Protein.Sequence
 * (kaamer_protein_entry.sequence / sequence_len, not the Length clip), its letter codes, a "letter outside the
 * alphabet" flag and its length go to the index's device, with an id -> entry map that resolves an id exactly as
 * kaamer_fetch_hits does (a later record with the same id wins: the FASTA reader's duplicated last id); KStats.NumberOfAA
 * (EValue, align.go:142) is taken from the table.  The device copy is the library's; the TABLE ITSELF IS BORROWED and
 * must outlive the index, or the next attach (results with text read the subjects' letters from it).  A second attach
 * replaces the first; kaamer_index_close frees the device copy.  Not to be called while calls are in flight on the
 * index.  KAAMER_ALIGN_GAP_COLUMN is read once per process, not per call. */
int kaamer_index_attach_proteins(kaamer_index *ix, const kaamer_proteins *p);
/* out = { bytes of HBM the attached table takes (0: none attached), entries, longest stored sequence, NumberOfAA,
 * direction-array budget in bytes, resident waves of the last alignment stage on the index, bytes of one direction slab
 * of that stage, resident waves of its long-subject kernel (0: not launched) } */
int kaamer_index_align_info(const kaamer_index *ix, uint64_t out[8]);
/* Bytes of direction array (one byte per cell: ceil(nq / 64) x (ns + 63) x 64 per pair) ONE grid of the alignment stage of
 * ONE call may hold.  The stage runs a grid of waves, each the owner of one slab sized for the batch's longest query
 * against the table's longest subject (capped at 2048, the wave kernel's LDS row), that take pairs by ticket: the budget
 * sets the number of waves, never the result -- at least one, and no more than five per compute unit (what the kernel's
 * LDS lets run at once; a sizing rule: nothing depends on the waves being resident together).  The few pairs with a
 * longer subject run on a second grid whose slabs (the table's longest subject) take up to the same budget again.
 * The slabs belong to the workspace: a host call keeps them with its slot, so HBM in use is up to 2 x budget x the slots
 * that have served an aligning call (KAAMER_HOST_SLOTS, default 4: up to 32 GiB at the default; the DB-SP protein batch
 * takes 4.3 GB + 4 GiB per slot).  Lower the budget where that is too much.  0: the default (4 GiB). */
int kaamer_index_set_align_budget(kaamer_index *ix, uint64_t bytes);

/* One (query, reported hit) pair as the device leaves it: integers only (align.go:87-133 from the traceback). */
typedef struct {
    int32_t status;               /* kaamer_alignment.status: 0, 2, 3; 4 = the hit id has no entry in the attached table, */
                                  /* or follows such a hit of its query: FetchHitsInformation stops there               */
                                  /* (search.go:461-463) and the hit keeps the empty AlignmentResult                     */
    int32_t n_ops;                /* columns                                                                              */
    int32_t start_i, start_j;     /* 0-based cell before the first column (QueryStart = start_i + 1 when n_ops > 0)       */
    int32_t end_i, end_j;         /* QueryEnd, SubjectEnd                                                                 */
    int32_t identical, similar, mismatches, gap_openings, raw;
    uint32_t query_len;           /* len(Query.Sequence): the trimmed ORF (EValue, align.go:142)                          */
    uint64_t off;                 /* host-buffer form: first operation in the block's operations section                  */
    uint32_t entry;               /* entry of the attached table                                                          */
    uint32_t subject_len;
} kaamer_align_pair;
typedef struct {
    char sub_matrix[16];          /* SearchOptions.SubMatrix / GapOpen / GapExtend (api/server.go:149-151)                */
    int32_t gap_open, gap_extend;
    uint32_t max_query_len;       /* residues of the batch's longest query (sizes the direction slabs; a longer query's   */
                                  /* pairs get status 3); 0: the workspace's max_seq_bytes (ample, and costly)            */
    uint32_t reserved;
    uint64_t max_pairs;           /* pair records to provision; 0: min(max_queries x max_results, max_hits)               */
} kaamer_topn_align_opts;
typedef struct {
    const uint64_t *d_pair_off;          /* [n_queries + 1] pair e = d_pair_off[q] + r is hit r of query q (d_top_pid order) */
    const kaamer_align_pair *d_pairs;
    uint64_t pair_capacity;
    uint32_t n_waves, n_long_waves;      /* resident waves of the two kernels                                             */
    uint64_t slab_bytes;                 /* one wave's direction slab                                                     */
} kaamer_topn_alignments;
/* The device-resident form: enqueued on `stream` behind kaamer_topn_device (`top` is its result; on the count stream when
 * the workspace's counting stage runs there), no host synchronisation.  Options without a row in AllMatrixScores, or a
 * matrix other than BLOSUM62: KAAMER_E_ARG (the host calls below report status 1 per item instead).  More pairs than
 * provisioned: KAAMER_E_CAPACITY at kaamer_workspace_finish.  KAAMER_E_ARG when no table is attached or the workspace's
 * last result is a merge. */
int kaamer_topn_align_device(kaamer_index *ix, kaamer_workspace *ws, const kaamer_topn_result *top,
                             const kaamer_topn_align_opts *opts, void *stream, kaamer_topn_alignments *out);
/* kaamer_search_batch_top_flat / kaamer_search_batch_top_pos_flat (want_positions != 0) with the alignment of every
 * reported hit in the same call and the same packed block (replaces search.go:454-470 + :483-494 for the whole batch).
 * In the result the hits of every reported query are in the reference's FINAL order: BitScore descending, ties in
 * sortMapByValue order (top_pid, top_kmatch, top_first_pos and the bitmaps' pos_off permuted together).  A hit whose
 * alignment failed keeps the empty AlignmentResult (BitScore 0).  Options without a row in AllMatrixScores, or a matrix
 * other than BLOSUM62: every item has status 1 and the hits stay in sortMapByValue order.  want_text = 0: numbers only
 * (no operations cross PCIe).  KAAMER_E_ARG when no table is attached.  A ticket is waited for with
 * kaamer_wait_batch_top or dropped with kaamer_ticket_discard. */
int kaamer_search_batch_top_aln_flat(kaamer_index *ix, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs,
                                     int32_t seq_type, double min_k_ratio, int64_t min_k_match, uint32_t max_results,
                                     int32_t want_positions, const char *sub_matrix, int32_t gap_open, int32_t gap_extend,
                                     int32_t want_text, kaamer_batch_top **out);
int kaamer_submit_batch_top_aln_flat(kaamer_index *ix, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs,
                                     int32_t seq_type, double min_k_ratio, int64_t min_k_match, uint32_t max_results,
                                     int32_t want_positions, const char *sub_matrix, int32_t gap_open, int32_t gap_extend,
                                     int32_t want_text, kaamer_ticket **ticket);
/* The alignments of a result (kaamer_batch_top itself is unchanged): items[e] belongs to entry e of the CSR arrays
 * (top_pid[e], ...); status as kaamer_alignment states it, plus 4 (kaamer_align_pair.status); aln_off points into `text`
 * (three rows of `length` bytes), which is NULL for a result without text.  Both NULL for a result of a call without
 * alignments.  They live as long as the result does. */
int kaamer_batch_top_alignments(const kaamer_batch_top *out, const kaamer_alignment **items, const char **text);
/* Test and measurement entry: the floats and coordinates of such a result for pair records the caller holds (read back behind
 * kaamer_topn_align_device, or built by hand): out[i] is what the items above would carry for pairs[i] -- status != 0
 * keeps the empty AlignmentResult, options without a row in AllMatrixScores give status 1 -- aln_off 0.  Host only. */
int kaamer_align_finish_pairs(const kaamer_align_pair *pairs, uint64_t n, uint64_t number_of_aa, const char *sub_matrix,
                              int32_t gap_open, int32_t gap_extend, kaamer_alignment *out);

/* The same on the one-process sharded handle (kaamer_index_open_sharded): replaces search.go:454-470 + :483-494 for a
 * database larger than one device.  The reported hits of a query are known at its owner (device q mod W) only; the
 * Protein.Sequence table is PARTITIONED, not replicated: device s of the handle receives the entries whose protein id
 * satisfies id mod W == s -- their stored bytes, an offsets array and a local id -> entry map indexed by id / W -- so
 * per-device HBM is about 1 / W of the sequence bytes and no device holds another's entries.  Ids resolve as
 * kaamer_fetch_hits resolves them (a later record with the same id wins).  One more exchange behind top-N brings the
 * subjects of the reported hits, and only those, to the owner, which aligns them there.  The rules of
 * kaamer_index_attach_proteins carry over: the table is borrowed and must outlive the handle (or the next attach), a
 * second attach replaces the first, KAAMER_E_BUSY while calls are in flight, NumberOfAA / the longest stored sequence /
 * the BLOSUM62 matrix are kept per handle, kaamer_sharded_index_close frees the device copies. */
int kaamer_sharded_index_attach_proteins(kaamer_sharded_index *sx, const kaamer_proteins *p);
/* The direction-array budget of each owner's alignment stage: kaamer_index_set_align_budget's meaning, per owner. */
int kaamer_sharded_index_set_align_budget(kaamer_sharded_index *sx, uint64_t bytes);
/* out = { table bytes over all devices (0: none attached), the largest device's share, entries, longest stored sequence,
 * NumberOfAA, bytes of the largest (holder -> owner) subject segment as it travelled in the last finished aligning call on
 * the handle's first set, bytes that segment needed, attempts of that call } */
int kaamer_sharded_align_info(kaamer_sharded_index *sx, uint64_t out[8]);
/* Measurement (no Go counterpart): on != 0 brackets the three stages of every later aligning call with HIP events on the
 * per-shard streams (no host synchronisation is added; off by default).  kaamer_sharded_align_stage_info: of the last
 * finished aligning call on the handle's first set, out = { 1 if timing is on, microseconds of the gather stage (all owners'
 * segments of one holder; the slowest holder), of the assemble stage (headers, layout, pairs kernel; the slowest owner), of
 * the alignment stage (wave kernels and finish; the slowest owner) -- zeros while timing is off --, bytes of one ids block
 * as it travelled, and of the owners' alignment stages the largest number of resident waves, bytes of one direction slab,
 * resident waves of the long-subject kernel (0: not launched on any owner) } */
int kaamer_sharded_index_set_align_timing(kaamer_sharded_index *sx, int32_t on);
int kaamer_sharded_align_stage_info(kaamer_sharded_index *sx, uint64_t out[8]);
/* kaamer_sharded_search_batch_top_flat / _top_pos_flat (want_positions != 0) with the alignment of every reported hit in
 * the same call (search.go:454-470 + :483-494 for the whole batch): what kaamer_search_batch_top_aln_flat returns on an
 * unsharded index of the whole database with the whole table attached, field for field, read with
 * kaamer_batch_top_alignments / kaamer_batch_top_positions.  A subject segment or an alignment section that is too
 * small repeats the batch inside kaamer_sharded_wait_batch_top with that bound grown alone; never a partial result; a
 * failure on any shard or owner fails the call.  KAAMER_E_ARG when no table is attached to the handle.  A ticket is
 * waited for with kaamer_sharded_wait_batch_top or dropped with kaamer_sharded_ticket_discard. */
int kaamer_sharded_search_batch_top_aln_flat(kaamer_sharded_index *sx, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs,
                                             int32_t seq_type, double min_k_ratio, int64_t min_k_match, uint32_t max_results,
                                             int32_t want_positions, const char *sub_matrix, int32_t gap_open, int32_t gap_extend,
                                             int32_t want_text, kaamer_batch_top **out);
int kaamer_sharded_submit_batch_top_aln_flat(kaamer_sharded_index *sx, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs,
                                             int32_t seq_type, double min_k_ratio, int64_t min_k_match, uint32_t max_results,
                                             int32_t want_positions, const char *sub_matrix, int32_t gap_open, int32_t gap_extend,
                                             int32_t want_text, kaamer_sharded_ticket **ticket);

/* ------------------------------------------------------------------------- */
/* Readers — GetQueriesFasta / GetQueriesFastq (search.go:222-412) on a text   */
/* buffer (already decompressed): packed sequences + SizeInKmer + names, with  */
/* the reference's quirks (every FASTA record but the last is upper-cased; '*' */
/* rule; FASTQ sequence lines must match ^[ATGCNatgcn]+$).                     */
/* ------------------------------------------------------------------------- */
/* `text` is the bytes of the file.  Bytes that start with the gzip signature (what the reference's
 * http.DetectContentType calls application/x-gzip, search.go:255-263, 361-366) are inflated first: every member of the
 * stream (Go's gzip.Reader is multistream); a stream that breaks off or is damaged reads as what inflated before that
 * (the reference's scanner stops at the read error and processes what it got); a first header that is no gzip header
 * gives an EMPTY read set (gzip.NewReader fails, GetQueriesFasta prints the error and returns without a query,
 * search.go:259-263).  kaamer_makedb_embl / _gbk inflate the same way (inputEMBL.go:76-84, inputGBK.go:75-83) but report
 * a bad first header as KAAMER_E_FORMAT (the reference log.Fatal()s there); the FASTA and TSV makedb readers have no gzip
 * branch in the reference. */
int kaamer_parse_fasta(const char *text, uint64_t len, kaamer_reads **out);
int kaamer_parse_fastq(const char *text, uint64_t len, kaamer_reads **out);
uint32_t kaamer_reads_count(const kaamer_reads *r);
const uint8_t *kaamer_reads_seqs(const kaamer_reads *r);
const uint64_t *kaamer_reads_offsets(const kaamer_reads *r);       /* count + 1 */
const int32_t *kaamer_reads_size_in_kmer(const kaamer_reads *r);
const char *kaamer_reads_names(const kaamer_reads *r);
const uint64_t *kaamer_reads_name_offsets(const kaamer_reads *r);  /* count + 1 */
/* Location.PlusStrand as the reference's reader leaves it: 1 for the first record, 0 (Go's zero value) for every
 * following one (search.go:297,399 rebuild the Query without a Location); protein results report it unchanged.
 * Not reproduced: bufio.Scanner's 1 MiB line limit (search.go:273-274: a longer line silently ends the
 * reference's scan) -- lines of any length are read. */
const int32_t *kaamer_reads_plus_strand(const kaamer_reads *r);
void kaamer_reads_free(kaamer_reads *r);

/* The same readers over a FILE, in chunks (search.go:240-283: open, sniff 32 bytes, gzip.NewReader when they carry the
 * gzip signature, bufio.Scanner line by line): a read set of any size goes through bounded memory -- BASELINE
 * configs[4].  format: 0 = GetQueriesFasta, 1 = GetQueriesFastq.  kaamer_reader_next hands out the next records -- up
 * to max_seqs of them, stopping once about max_bytes of sequence are in the chunk -- as a kaamer_reads (accessors above;
 * free it with kaamer_reads_free), ready for kaamer_stream_push / kaamer_replica_stream_push; a chunk with zero records
 * and kaamer_reader_done() = 1 is the end.  The rules that span records hold across chunks: FASTA upper-cases every
 * record but the LAST of the file, PlusStrand is 1 on the file's first record only.  gzip: every member, a stream that
 * breaks off or is damaged reads as what inflated before; a first header that is no gzip header: no records.
 * strict_scanner = 1 additionally reproduces what the reference's scanner setup does to unusual input: a line of
 * 1 048 576 bytes or more ends the input there (bufio.Scanner with a 1 MiB buffer returns false, search.go:273-274; the
 * record being read is emitted as the last one), and a file whose first 32 bytes are not what http.DetectContentType
 * calls "text/plain; charset=utf-8" (a UTF-16 byte-order mark, a control byte) yields no records (search.go:266-270).
 * strict_scanner = 0 reads lines of any length. */
typedef struct kaamer_reader kaamer_reader;
int kaamer_reader_open(const char *path, int format, int strict_scanner, kaamer_reader **out);
int kaamer_reader_open_fd(int fd, int format, int strict_scanner, kaamer_reader **out); /* fd stays the caller's */
int kaamer_reader_next(kaamer_reader *rd, uint32_t max_seqs, uint64_t max_bytes, kaamer_reads **out);
int kaamer_reader_done(const kaamer_reader *rd);
uint64_t kaamer_reader_records(const kaamer_reader *rd);   /* records handed out so far */
void kaamer_reader_close(kaamer_reader *rd);

/* ------------------------------------------------------------------------- */
/* FASTQ text parsed on the device — GetQueriesFastq (search.go:324-412) as a  */
/* data-parallel job: raw text in, the reported hits out.  The host readers    */
/* above remain the route for strict_scanner, -pos / -aln and the sharded      */
/* handle.  FASTA text has calls of its own: the last section of this file.    */
/* ------------------------------------------------------------------------- */
/* The reader's rules, per line (search.go:370-410; the kernels in parse_text.hip.inc compute exactly this):
 *   lines    split at '\n'; a last piece without '\n' is a line; one trailing '\r' is dropped (bufio.ScanLines)
 *   class    X (ignored): empty after the '\r' drop.  H: the first byte is '@' (search.go:380).  S: every byte is one of
 *            ATGCNatgcn (search.go:340,386).  X: anything else.  A quality line that starts with '@' is an H and one made
 *            of those ten letters only is an S: both quirks of the reference are kept.
 *   records  X lines are ignored.  A record is every S line whose next non-X line is an H, or that has no next non-X line
 *            (of a run of S lines the last one wins: search.go:386-388).  Its sequence is that line's bytes, no case
 *            change; its name is what follows the '@' of the nearest preceding H line, empty when no H precedes (the very
 *            start of a file only); SizeInKmer = len - 6 (search.go:395,407).  PlusStrand is 1 on the file's first record
 *            only (search.go:399): host bookkeeping, not part of the parse.
 *   chunks   a text may be cut at any p with text[p-1] == '\n' and text[p] == '@': the pieces, parsed independently, give
 *            the records of the whole text in order (kaamer_text_cut_fastq).
 * Out of scope here: strict_scanner, -pos / -aln on the text forms (the bitmaps of the reported hits do come with the
 * calls that return TSV rows, kaamer_submit_text_top_tsv_flat at the end of this file), the sharded handle, a reader thread.
 * The response rows of a text request are no longer the host's to write: same calls.  (Inflating on
 * the device: the BGZF section below.  FASTA on the device: the section after it, with entry points of its own -- the
 * calls of this section keep refusing format 0.) */
typedef struct kaamer_text_parser kaamer_text_parser;
/* name and sequence of one record as ranges of the text.  FASTQ: text[seq_off, seq_off + seq_len) IS the sequence.  FASTA:
 * seq_off is the record's first kept byte and seq_len reaches to one past its last kept byte, so the range covers the line
 * breaks and trimmed bytes in between (and no header line): the packed length is offsets[i + 1] - offsets[i], not seq_len. */
typedef struct { uint32_t name_off, name_len, seq_off, seq_len; } kaamer_text_span;   /* into the text */
typedef struct {
    uint32_t n_records;
    uint32_t reserved;
    uint64_t n_lines;                   /* lines as the reader counts them */
    uint64_t seq_bytes;                 /* = offsets[n_records] */
    const uint8_t *d_seqs;              /* device: the records' sequences back to back: what kaamer_search_device takes */
    const uint64_t *d_offsets;          /* device: n_records + 1 */
    const kaamer_text_span *d_spans;    /* device: n_records */
} kaamer_text_parse_result;
/* A parser holds the device buffers for texts of up to max_text_bytes (at most 2^32 - 1: spans are 32-bit; longer texts
 * are KAAMER_E_ARG -- cut them) with up to max_records records.  Lines are bounded by max_text_bytes / 16 +
 * 4 max_records + 1024 (a FASTQ record is four lines).  A text beyond either bound sets a status word on the device:
 * kaamer_text_parser_finish then returns KAAMER_E_CAPACITY, never a partial result, and the parser stays usable. */
int kaamer_text_parser_create(int device, uint64_t max_text_bytes, uint32_t max_records, kaamer_text_parser **out);
void kaamer_text_parser_free(kaamer_text_parser *p);
/* Enqueues the parse of d_text[0, n_bytes) on `stream` (a hipStream_t; NULL: the default stream).  d_text stays the
 * caller's, must start at a 16-byte boundary (any hipMalloc'd buffer does) and must not change before the parse is done.
 * Bytes that start with the gzip signature are parsed as they are (text): inflate first. */
int kaamer_parse_fastq_device(kaamer_text_parser *p, const uint8_t *d_text, uint64_t n_bytes, void *stream);
/* Waits for the last parse enqueued on `stream`: the counts and the device pointers, valid until the next parse. */
int kaamer_text_parser_finish(kaamer_text_parser *p, void *stream, kaamer_text_parse_result *out);
/* What the kernels' tiling is made of (tests put their boundary cases there): out[0] bytes a lane reads at once, out[1]
 * bytes a wave reads at once, out[2] bytes of text per workgroup, out[3] lines per workgroup of the record passes.
 * Lines are classified and copied by position, not per line: there is no line length at which the code path changes. */
void kaamer_text_parser_geometry(uint32_t out[4]);

/* Host-buffer search that takes TEXT instead of a packed batch (search_fastq.go:60-136 with the reader inside): the text
 * is uploaded to the slot, parsed on the slot's stream, then searched exactly as kaamer_submit_batch_top_flat searches the
 * packed batch -- wait, the repeat of a batch beyond a bound (from the parsed buffers: the text is not parsed again),
 * discard and the packed block are those of kaamer_ticket.  The submit call waits once for the two counts of the parse
 * (records, sequence bytes: one small copy): kaamer_search_device takes n_seqs from the host, so this cannot be avoided.
 * format: 1 (FASTQ); 0 (FASTA) is KAAMER_E_ARG -- use kaamer_submit_fasta_top_flat, or the host reader (kaamer_parse_fasta +
 * kaamer_search_batch_top_flat).
 * seq_type: base KAAMER_READS or KAAMER_NUCLEOTIDE (NucleotideSearch takes FASTQ too, search_nucleotide.go:38-39), the
 * genetic code in bits 8-15 as on every call; KAAMER_PROTEIN is KAAMER_E_ARG.  Text that starts with the gzip signature is
 * KAAMER_E_ARG: kaamer_search_text_file inflates (zlib, on the host), and whole BGZF blocks have a call of their own
 * (kaamer_search_bgzf_top_flat below).  `text` is borrowed for the call (one pointer: cgo-safe).
 * The slot's parser and text staging (pinned host + device) are allocated at the first text call on it: an index that
 * never sees text allocates nothing for it.  rep_query / q[].src_seq of the result index the records of the text. */
int kaamer_submit_text_top_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t format, int32_t seq_type,
                                double min_k_ratio, int64_t min_k_match, uint32_t max_results, kaamer_ticket **ticket);
int kaamer_search_text_top_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t format, int32_t seq_type,
                                double min_k_ratio, int64_t min_k_match, uint32_t max_results, kaamer_batch_top **out);
/* The spans of the text's records (16 bytes each; the caller holds the text): views into `out`, NULL / 0 for a result of
 * a call that took a packed batch. */
int kaamer_batch_top_text_spans(const kaamer_batch_top *out, const kaamer_text_span **spans, uint32_t *n_records);

/* The greatest valid cut p in [1, len): text[p-1] == '\n' and text[p] == '@'; 0: none. */
uint64_t kaamer_text_cut_fastq(const char *text, uint64_t len);
/* FastqSearch over a FILE (search_fastq.go:60-136) with the reader on the device: raw bytes (plain, or gzip inflated
 * incrementally by the byte source kaamer_reader_* uses, with its rules: every member, a broken stream reads as what
 * inflated before, a first header that is no gzip header yields no records) are collected into chunks of about
 * chunk_text_bytes, each cut at kaamer_text_cut_fastq with the tail carried into the next, dealt round-robin to the
 * replicas with up to in_flight chunks per replica (0: three) and searched by kaamer_submit_text_top_flat.  cb is called
 * once per chunk, in input order; `top` indexes the chunk's records from 0, first_seq is the chunk's first record in the
 * file.  A chunk without a cut goes on reading up to 4 chunk_text_bytes; beyond that: KAAMER_E_CAPACITY (use
 * kaamer_search_file).  Memory: in_flight x replicas chunks.  Errors drain the chunks in flight, counters are summed and
 * a non-zero return of cb stops the run with KAAMER_E_ARG, as in kaamer_search_file (it is the same loop). */
typedef int (*kaamer_text_chunk_cb)(void *user, uint64_t first_seq, const char *text, uint64_t len,
                                    const kaamer_text_span *spans, uint32_t n_records, const kaamer_batch_top *top);
int kaamer_search_text_file(kaamer_replicas *r, const char *path, int format, int32_t seq_type, double min_k_ratio,
                            int64_t min_k_match, uint32_t max_results, uint64_t chunk_text_bytes, uint32_t in_flight,
                            kaamer_text_chunk_cb cb, void *user, kaamer_counters *total);

/* ------------------------------------------------------------------------- */
/* BGZF inflated on the device.  BGZF (what bgzip, htslib and most sequencer  */
/* pipelines write) is a run of independent gzip members of at most 64 KiB of */
/* text each, every member's compressed size in its header and its inflated   */
/* size and CRC-32 in its trailer: the host finds the blocks without          */
/* inflating, every block is inflated by a wave of its own (inflate.hip.inc). */
/* Ordinary single-member gzip, BGZF-compressed FASTA, -pos / -aln and the    */
/* sharded handle stay with the host readers above.                           */
/* ------------------------------------------------------------------------- */
/* One block: the deflate payload is bytes[comp_off, comp_off + comp_len) -- what lies between the member's header and
 * its 8-byte trailer -- and inflates to isize bytes (at most 65536) with CRC-32 crc. */
typedef struct { uint64_t comp_off; uint32_t comp_len, isize, crc, reserved; } kaamer_bgzf_block;
/* CPU only.  Walks the member headers of bytes[0, len) without inflating: a BGZF header is 1f 8b 08, FLG exactly 4, and an
 * extra field that holds (walked subfield by subfield) a subfield 'B' 'C' with SLEN 2, whose value is the member's size
 * minus 1 (BSIZE).  Fills blocks[0, min(*n_blocks, cap)) and stops at the first member that is no BGZF block or is not whole
 * in the buffer -- also one without the BC subfield, with BSIZE + 1 below header + trailer, or with ISIZE above 65536.
 * *n_blocks: the whole blocks found (it may exceed cap: call again with more room); *consumed: where the walk stopped
 * (== len: the buffer is whole BGZF blocks).  The 28-byte empty end-of-file block is an ordinary block with isize 0.
 * blocks may be NULL when cap is 0. */
int kaamer_bgzf_scan(const uint8_t *bytes, uint64_t len, kaamer_bgzf_block *blocks, uint64_t cap, uint64_t *n_blocks,
                     uint64_t *consumed);

typedef struct kaamer_inflater kaamer_inflater;
typedef struct {
    uint32_t n_bad;                     /* blocks whose status is not 0 */
    uint32_t first_bad;                 /* the first of them (0xFFFFFFFF: none) */
    uint64_t out_bytes;                 /* the sum of the blocks' isize */
    uint32_t first_bad_status;          /* its status word (0: none) */
    uint32_t reserved;
    const uint32_t *d_status;           /* device: one word per block */
} kaamer_inflate_result;
/* An inflater holds the per-block device words for calls of up to max_blocks blocks and max_comp_bytes compressed bytes. */
int kaamer_inflater_create(int device, uint64_t max_comp_bytes, uint32_t max_blocks, kaamer_inflater **out);
void kaamer_inflater_free(kaamer_inflater *inf);
/* Enqueues on `stream` the inflate of d_blocks[0, n_blocks) (device, 8-byte aligned; comp_off relative to d_comp, which
 * holds comp_bytes bytes: a block whose payload is not inside them is status 4 and is not read): block b
 * goes to d_out + (the sum of isize of the blocks before it) -- the text of the blocks back to back, at any alignment.
 * Every block is a full RFC 1951 inflate (stored, fixed and dynamic blocks, any number of them) checked against isize and
 * crc, and ends with a status word: 0 good; 1 bad block type, stored length mismatch or payload left behind the final
 * block; 2 over-subscribed or incomplete code; 3 invalid symbol or distance (BGZF blocks share no window: a distance
 * beyond the block's own output is invalid); 4 input exhausted; 5 more output than ISIZE (or than out_cap holds); 6 less
 * output than ISIZE; 7 CRC-32 mismatch.  No input makes the kernel read outside a block's payload or write outside the
 * block's isize bytes.  The bytes of a bad block's output are unspecified. */
int kaamer_inflate_bgzf_device(kaamer_inflater *inf, const uint8_t *d_comp, uint64_t comp_bytes, const kaamer_bgzf_block *d_blocks,
                               uint32_t n_blocks, uint8_t *d_out, uint64_t out_cap, void *stream);
/* Waits for the last inflate enqueued on `stream`; d_status is valid until the next inflate. */
int kaamer_inflater_finish(kaamer_inflater *inf, void *stream, kaamer_inflate_result *out);
/* The tiling (tests put their boundary cases there): out[0] bytes of output per lane of the CRC, out[1] BGZF blocks (waves)
 * per workgroup, out[2] bytes of text per workgroup of the cut kernel, out[3] threads of the one workgroup that scans the
 * blocks' sizes into their offsets: each takes ceil(n_blocks / out[3]) blocks in a row. */
void kaamer_inflater_geometry(uint32_t out[4]);
/* kaamer_text_cut_fastq of a text that lives on the device (the caller of the device inflate never holds it): waits. */
int kaamer_text_cut_fastq_device(int device, const uint8_t *d_text, uint64_t n_bytes, void *stream, uint64_t *cut);

/* kaamer_submit_text_top_flat / kaamer_search_text_top_flat for FASTQ that is BGZF-compressed: `bytes` must be whole BGZF
 * blocks (kaamer_bgzf_scan consumes all of them; anything else -- ordinary gzip, plain text, a block cut short -- is
 * KAAMER_E_ARG, and kaamer_submit_text_top_flat keeps refusing gzip bytes: this call is the opt-in).  The compressed bytes
 * and the block table are uploaded to the slot (about a fifth of the text's bytes), then inflated, parsed and searched on
 * the slot's stream.  A block that does not inflate is KAAMER_E_FORMAT, with the block's index and its status word in
 * kaamer_last_error: hand such bytes to the host inflater.  The spans of kaamer_batch_top_text_spans index the INFLATED
 * text, which is copied back with the result: kaamer_batch_top_text (a view into `out`; NULL / 0 for any other call's
 * result).  `bytes` is borrowed for the call. */
int kaamer_submit_bgzf_top_flat(kaamer_index *ix, const uint8_t *bytes, uint64_t len, int32_t seq_type, double min_k_ratio,
                                int64_t min_k_match, uint32_t max_results, kaamer_ticket **ticket);
int kaamer_search_bgzf_top_flat(kaamer_index *ix, const uint8_t *bytes, uint64_t len, int32_t seq_type, double min_k_ratio,
                                int64_t min_k_match, uint32_t max_results, kaamer_batch_top **out);
int kaamer_batch_top_text(const kaamer_batch_top *out, const char **text, uint64_t *len);

/* kaamer_search_text_file with one more argument.  device_inflate = 0 is kaamer_search_text_file.  device_inflate = 1:
 *   plain files   take that path too;
 *   a gzip file   is read raw and scanned with kaamer_bgzf_scan; whole blocks are grouped until their ISIZEs reach
 *                 chunk_text_bytes.  The device text of chunk k is the tail of chunk k-1 (a short plain upload) followed by
 *                 its blocks' output (out offsets: the prefix sum of ISIZE behind the tail); it is cut on the device at
 *                 kaamer_text_cut_fastq's place (the last chunk: at its end), [0, cut) is parsed and searched, [cut, end)
 *                 comes back as the next tail.  A chunk without a cut takes one more budget of blocks, up to four, then
 *                 fails with kaamer_search_text_file's KAAMER_E_CAPACITY.  The callback keeps its contract: text, len is
 *                 the chunk's inflated text [0, cut) -- the copy brought back from the device -- with spans into it.
 *   fallback      as soon as a chunk reports a bad block, the scan meets a member that is no BGZF block (ordinary gzip,
 *                 FNAME set, ...) or the file ends inside a block, the file's position at that chunk's first block goes to
 *                 the host inflater with the pending tail in front, and the rest of the file runs on the flag-0 route.
 * The concatenated text the callbacks see is byte for byte the flag-0 run's, for every file; the chunk boundaries differ.
 * The submit of a device chunk waits twice on the replica's stream (status words + cut, then the parse's counts: the
 * parser takes the text's length from the host). */
int kaamer_search_text_file_opts(kaamer_replicas *r, const char *path, int format, int32_t seq_type, double min_k_ratio,
                                 int64_t min_k_match, uint32_t max_results, uint64_t chunk_text_bytes, uint32_t in_flight,
                                 int32_t device_inflate, kaamer_text_chunk_cb cb, void *user, kaamer_counters *total);

/* ------------------------------------------------------------------------- */
/* FASTA text parsed on the device — GetQueriesFasta (search.go:222-322), the  */
/* reader of ProteinSearch and, for requests that are not FASTQ, of            */
/* NucleotideSearch and FastqSearch (search_nucleotide.go, search_fastq.go).   */
/* The FASTQ calls above keep refusing format 0: FASTA has these entry points. */
/* ------------------------------------------------------------------------- */
/* The reader's rules (the host's statement: kaamer_parse_fasta; the kernels in parse_fasta.hip.inc compute exactly this):
 *   lines    split at '\n'; a last piece without '\n' is a line; one trailing '\r' is dropped (bufio.ScanLines)
 *   trim     leading and trailing bytes out of ' ' \t \n \v \f \r are removed from a non-header line (search.go:309; ASCII
 *            only: 0x85, 0xA0, 0x1C-0x1F, 0x00 and every byte >= 0x80 are ordinary bytes).  Interior whitespace is kept.
 *   class    H: non-empty after the '\r' drop and the first byte is '>' -- tested before any trim, so " >x" is a sequence
 *            line that contributes ">x".  S: any other line with a byte left after the trim.  X: empty and whitespace-only
 *            lines (search.go:285-287).
 *   records  X lines are ignored.  A record is a maximal run of S lines with no H line between them; its sequence is the
 *            concatenation of their trimmed bytes.  Its name is what follows the '>' of the nearest preceding H line, the
 *            '\r' dropped and nothing else trimmed; empty when no H precedes (the first record only).  Headers with no S
 *            line before the next header produce nothing.
 *   case     every record but the LAST of the input has a-z mapped to A-Z (search.go:295 against :313-320); the last is
 *            copied as it is -- precisely: the record still pending at the end of the input.  A last record with a header
 *            line behind it (">a\nacgt\n>b\n") was closed by that header and is upper-cased like the others, on the host
 *            reader and here.  upper_last = 1: more input follows this text, the pending record is upper-cased too.
 *   size     SizeInKmer (len - 6, minus 1 when the last byte is '*') is derived from the packed bytes by the search
 *            kernels; the parser does not produce it.
 *   spans    name_off / name_len as for FASTQ; seq_off / seq_len: see kaamer_text_span (the range spans line breaks).
 *   chunks   kaamer_text_cut_fasta.
 * Out of scope here: BGZF-compressed FASTA, -pos / -aln on the text forms, the sharded handle, strict_scanner. */
/* kaamer_text_parser_create with a line bound of the caller's: max_lines below the FASTQ rule (max_text_bytes / 16 +
 * 4 max_records + 1024) is raised to it.  FASTA at narrow line widths has more lines than that rule allows. */
int kaamer_text_parser_create_lines(int device, uint64_t max_text_bytes, uint32_t max_records, uint64_t max_lines,
                                    kaamer_text_parser **out);
/* kaamer_parse_fastq_device for FASTA: the same parser object, kaamer_text_parser_finish and kaamer_text_parse_result,
 * the same demands on d_text.  The per-line words only FASTA needs are allocated at the parser's first FASTA text. */
int kaamer_parse_fasta_device(kaamer_text_parser *p, const uint8_t *d_text, uint64_t n_bytes, int32_t upper_last, void *stream);
/* CPU only.  The greatest p in [1, len) with text[p-1] == '\n', text[p] == '>' and at least one S line, complete or not, in
 * [p, len) (a partial last line counts when its first byte is not '>' and it holds a non-space byte); 0: none.  The S
 * line guarantees that a record follows the cut: every piece in front of a cut is parsed with upper_last = 1, the piece
 * at the end of the input with 0, and the pieces' records are the records of the whole. */
uint64_t kaamer_text_cut_fasta(const char *text, uint64_t len);
/* CPU only.  Where an EMBL text may be cut (kaamer_makedb_embl_device): the greatest p <= len such that text[0, p) ends with
 * the line end of a line that is exactly "//" after the '\r' drop; 0: none.  A final "//" without '\n' counts only when it
 * is the text's last line, and then p = len: of a prefix that ends inside a line this holds only if the input ends there.
 * A GBK entry ends at the same line, so this is the cut for kaamer_makedb_gbk_device too. */
uint64_t kaamer_text_cut_embl(const char *text, uint64_t len);
/* kaamer_submit_text_top_flat / kaamer_search_text_top_flat for FASTA text (search_protein.go:38-120, search_nucleotide.go,
 * search_fastq.go with GetQueriesFasta inside): the same slot, ticket, wait, repeat beyond a bound (from the parsed
 * buffers), discard and kaamer_batch_top_text_spans.  seq_type: base KAAMER_PROTEIN, KAAMER_NUCLEOTIDE or KAAMER_READS, the
 * genetic code in bits 8-15.  Text that starts with the gzip signature is KAAMER_E_ARG; so is text above 2^32 - 1 bytes
 * (cut it: kaamer_text_cut_fasta).  `text` is borrowed for the call (one pointer: cgo-safe).
 * Against kaamer_parse_fasta + kaamer_search_batch_top_flat on the same text, one caller (profiles/r17_fasta_parse.md): 4.3x
 * for 10 000 protein queries (3.7 MB of text: 0.76 against 3.23 ms), 8.5x for 1 M two-line reads, 7.7x for 300 MB of contigs;
 * with four callers 3.7x to 4.0x.  No measured input is slower on the text route. */
int kaamer_submit_fasta_top_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t seq_type, int32_t upper_last,
                                 double min_k_ratio, int64_t min_k_match, uint32_t max_results, kaamer_ticket **ticket);
int kaamer_search_fasta_top_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t seq_type, int32_t upper_last,
                                 double min_k_ratio, int64_t min_k_match, uint32_t max_results, kaamer_batch_top **out);
/* ProteinSearch / NucleotideSearch / FastqSearch over a FASTA FILE: kaamer_search_text_file's byte source (plain or gzip,
 * with its rules), chunk loop and callback, the chunks cut at kaamer_text_cut_fasta; every chunk but the file's last is
 * parsed with upper_last = 1.  A chunk without a cut goes on reading up to 4 chunk_text_bytes; beyond that:
 * KAAMER_E_CAPACITY (use kaamer_search_file).  An empty file, or a first header that is no gzip header: no chunk, no error. */
int kaamer_search_fasta_file(kaamer_replicas *r, const char *path, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                             uint32_t max_results, uint64_t chunk_text_bytes, uint32_t in_flight, kaamer_text_chunk_cb cb,
                             void *user, kaamer_counters *total);

/* ------------------------------------------------------------------------- */
/* The TSV response rows (QueryResultHandler, search.go:505-554, the form     */
/* without alignment; header line: SetResponseFormatAndHeader,                 */
/* search.go:636-662): one line per reported hit, reported queries ascending,  */
/* hits in reporting order, fields separated by '\t', the line ended by '\n'.  */
/*    1 QueryId          strings.Split(Query.Name, " ")[0]: the bytes before   */
/*                       the first 0x20 (a tab is an ordinary byte); an ORF    */
/*                       takes the name of record q[].src_seq                  */
/*    2 SubjectId        HitEntries[Key].EntryId                               */
/*    3 %KMatchIdentity  "%.2f" of float32(Kmatch) / float32(SizeInKmer) *     */
/*                       float32(100): two float32 roundings, then the exact   */
/*                       value rounded half-even at the second decimal         */
/*    4 QueryKLength     SizeInKmer (an ORF's: after SetBestStartCodon)        */
/*    5 KMatch                                                                 */
/*    6 GapOpen          ExtractPositions: the ',' of field 11; else "N/A"     */
/*  7 8 QStart QEnd      Location.StartPosition (after the trim), EndPosition  */
/*    9 SStart           "1"                                                   */
/*   10 SEnd             Annotations: Protein.Length; else "N/A"               */
/*   11 QueryPositions   ExtractPositions only: kaamer_format_positions(bitmap,*/
/*                       bits as searched, 0)                                  */
/*  12.. one per KStats.Features name, Annotations only: the entry's value     */
/* FetchHitsInformation stops a query's loop at the first id without an entry  */
/* (search.go:461-463): from that hit on, in reporting order, every hit of the */
/* query prints an empty SubjectId, 0 as Length and empty feature values.      */
/* The -aln form has its own section below (host formatter and device stage).  */
/* Out of scope: the file drivers and streams, the sharded handle and the      */
/* packed-batch calls on the device -- those have the host formatter, and the  */
/* device stage takes names as bytes + spans, so a packed form is host         */
/* plumbing only.  (-fmt json: the JSON section at the end of this file.)      */
/* ------------------------------------------------------------------------- */
/* SetResponseFormatAndHeader, search.go:645-660, Align = false.  proteins (its feature names) may be NULL without
 * annotations.  The conventions of kaamer_format_positions: at most cap bytes, NUL-terminated when cap > 0, the return is
 * the whole length without the NUL; need = f(NULL, 0). */
uint64_t kaamer_format_tsv_header(int32_t extract_positions, int32_t annotations, const kaamer_proteins *proteins, char *buf,
                                  uint64_t cap);
/* The rows of any kaamer_batch_top (packed, _pos, sharded or text), on the caller's thread: what QueryResultHandler's
 * `output += ...` per field does (search.go:505-554).  Names: record i of the input is name_bytes[name_spans[i].name_off,
 * + name_len) -- a text result passes the caller's text and kaamer_batch_top_text_spans; n_names records (q[].src_seq beyond
 * it prints an empty name).  proteins: the table kaamer_fetch_hits reads; NULL prints every entry as missing.
 * line_off (may be NULL): top_off[n_reported] + 1 entries, the first byte of every row and the total.  Returns the whole
 * length (buf and cap as above: need = f(NULL, 0)), or a negative code: KAAMER_E_ARG for a bad argument and for
 * extract_positions on a result without bitmaps (kaamer_batch_top_positions gives NULL). */
int64_t kaamer_format_tsv(const kaamer_batch_top *top, const char *name_bytes, uint64_t name_bytes_len,
                          const kaamer_text_span *name_spans, uint32_t n_names, const kaamer_proteins *proteins,
                          int32_t extract_positions, int32_t annotations, char *buf, uint64_t cap, uint64_t *line_off);
/* The same on a result whose arrays the caller holds itself (one built by hand, or by another library): the three arrays
 * of kaamer_batch_top_positions as arguments, all NULL without extract_positions.  Host only. */
int64_t kaamer_format_tsv_arrays(const kaamer_batch_top *top, const int32_t *pos_bits_len, const uint64_t *pos_off,
                                 const uint64_t *pos_bits, const char *name_bytes, uint64_t name_bytes_len,
                                 const kaamer_text_span *name_spans, uint32_t n_names, const kaamer_proteins *proteins,
                                 int32_t extract_positions, int32_t annotations, char *buf, uint64_t cap, uint64_t *line_off);

/* ------------------------------------------------------------------------- */
/* The -aln TSV rows (QueryResultHandler, search.go:556-604; header line       */
/* search.go:649 + :651-660): one line per reported hit of a result that        */
/* carries alignments, in the result's own order (BitScore descending, ties in  */
/* sortMapByValue order).                                                       */
/*    1 QueryId, 2 SubjectId   as above.  FetchHitsInformation stops BEFORE the  */
/*                     sort, so the hits without an entry are those with status  */
/*                     4 (and, in a result that was not aligned -- status 1,     */
/*                     sortMapByValue order -- those behind a missing id)        */
/*    3 %Identity      "%.2f" of the float32 Alignment.Identity: its exact      */
/*                     value, half-even at the second decimal; NaN when the      */
/*                     alignment has no columns                                  */
/*  4 5 6 AlnLength Mismatches GapOpen   Alignment.Length / .Mismatches /        */
/*                     .GapOpenings                                              */
/*  7 8 QStart QEnd    base sequence type PROTEIN: Alignment.QueryStart /        */
/*                     QueryEnd; else Location.StartPosition / EndPosition       */
/* 9 10 SStart SEnd    Alignment.SubjectStart / SubjectEnd                       */
/*   11 Evalue         "%e" of the float64 Alignment.EValue: d.dddddde+XX, its   */
/*                     exact value rounded half-even at the sixth decimal, the    */
/*                     exponent with at least two digits                          */
/*   12 Bitscore       "%.2f" of the float64 Alignment.BitScore                  */
/*   13 QueryPositions ExtractPositions only: kaamer_format_positions(bitmap,    */
/*                     bits as searched, 1)                                      */
/*  14.. the annotation columns, Annotations only                                */
/* The floats print as strconv prints them: every finite value exactly,          */
/* subnormals included; "NaN", "+Inf", "-Inf".  A hit with the empty             */
/* AlignmentResult (kaamer_alignment.status != 0) prints its zeros:              */
/* 0.00 0 0 0 <QStart> <QEnd> 0 0 0.000000e+00 0.00.                             */
/* Out of scope: AlnString, and -aln JSON (the JSON section at the end of this   */
/* file writes results without alignments).  The device stage (below) serves     */
/* device-resident pair records and the text calls (kaamer_*_top_aln_tsv_flat);  */
/* the sharded handle, streams, file drivers and the packed-batch calls format   */
/* these rows with the host formatter.                                           */
/* ------------------------------------------------------------------------- */
uint64_t kaamer_format_tsv_aln_header(int32_t extract_positions, int32_t annotations, const kaamer_proteins *proteins, char *buf,
                                      uint64_t cap);
/* The rows of any kaamer_batch_top that carries alignments (kaamer_batch_top_alignments gives them), on the caller's
 * thread.  Arguments and conventions as kaamer_format_tsv; seq_type: the request's (its base decides fields 7 and 8).
 * KAAMER_E_ARG on a result without alignments, and for extract_positions on a result without bitmaps. */
int64_t kaamer_format_tsv_aln(const kaamer_batch_top *top, const char *name_bytes, uint64_t name_bytes_len,
                              const kaamer_text_span *name_spans, uint32_t n_names, const kaamer_proteins *proteins,
                              int32_t seq_type, int32_t extract_positions, int32_t annotations, char *buf, uint64_t cap,
                              uint64_t *line_off);
/* The same on a result whose arrays the caller holds itself: alns[e] belongs to entry e of the CSR arrays (NULL:
 * KAAMER_E_ARG), the three arrays of kaamer_batch_top_positions all NULL without extract_positions.  top_kmatch is not
 * read.  Host only. */
int64_t kaamer_format_tsv_aln_arrays(const kaamer_batch_top *top, const kaamer_alignment *alns, const int32_t *pos_bits_len,
                                     const uint64_t *pos_off, const uint64_t *pos_bits, const char *name_bytes,
                                     uint64_t name_bytes_len, const kaamer_text_span *name_spans, uint32_t n_names,
                                     const kaamer_proteins *proteins, int32_t seq_type, int32_t extract_positions,
                                     int32_t annotations, char *buf, uint64_t cap, uint64_t *line_off);
/* Test entry: one float64 as fields 11 (mode 0: "%e") and 12 (mode 1: "%.2f") print it; buf / cap / the return as above. */
uint64_t kaamer_format_double(double value, int32_t mode, char *buf, uint64_t cap);

/* What the rows need of the protein table, resident next to the index: every entry's EntryId bytes, its Length and its
 * annotation columns pre-joined on the host ('\t' + value per KStats.Features name, in order: the device only copies
 * bytes), with offsets and an id -> entry map that resolves ids as kaamer_fetch_hits does (shared with
 * kaamer_index_attach_proteins' map when both are attached in that order; else one of its own).  The table is read during
 * the call only.  A second attach replaces the first; KAAMER_E_BUSY with calls in flight; freed by kaamer_index_close. */
int kaamer_index_attach_subject_text(kaamer_index *ix, const kaamer_proteins *proteins);
/* out[0] HBM bytes, out[1] entries, out[2] the longest row suffix (EntryId + Length digits + annotation columns), out[3]
 * feature names; zeros when nothing is attached */
int kaamer_index_subject_text_info(const kaamer_index *ix, uint64_t out[4]);

/* The rows on the device (tsv_rows.hip.inc), enqueued on `stream` behind kaamer_topn_device -- and behind
 * kaamer_topn_positions_device with extract_positions.  Plain device arrays: a workspace's, or fabricated ones. */
typedef struct {
    kaamer_topn_result top;             /* max_results, d_top_cnt, d_top_pid, d_top_kmatch, d_start_position,          */
                                        /* d_size_in_kmer (d_top_first_pos and d_trim are not read)                    */
    const kaamer_query_meta *d_q;       /* src_seq and end_position of every query                                     */
    const uint32_t *d_n_queries;        /* device scalar, as the workspace holds it                                    */
    uint32_t n_queries_cap;             /* its bound: what the launches are sized by                                   */
    uint32_t n_names;                   /* records the spans describe                                                  */
    const uint8_t *d_name_bytes;        /* the text the spans index ...                                                */
    uint64_t name_bytes_len;            /* ... and its length: a span beyond it prints an empty name                   */
    const kaamer_text_span *d_spans;    /* name_off / name_len are read                                                */
    const kaamer_topn_positions *pos;   /* NULL unless extract_positions                                               */
    int32_t extract_positions, annotations;
} kaamer_tsv_rows_in;
typedef struct {
    const uint64_t *d_line_off;         /* [lines + 1] first byte of every row in d_out, in CSR order; the total        */
    const uint64_t *d_counts;           /* device: {lines, bytes}                                                       */
    uint64_t line_off_capacity;         /* entries d_line_off holds                                                     */
} kaamer_tsv_rows_result;
/* The stage's own buffers (per-query sizes, their scan, the line offsets), for up to max_queries queries and max_lines
 * rows; one stage serves one stream at a time. */
typedef struct kaamer_tsv_stage kaamer_tsv_stage;
int kaamer_tsv_stage_create(kaamer_index *ix, uint32_t max_queries, uint64_t max_lines, kaamer_tsv_stage **out);
void kaamer_tsv_stage_free(kaamer_tsv_stage *st);
/* A length pass (a lane per query: digits, field lengths, for field 11 the runs of the bitmap words), a 64-bit scan of
 * the tiles' sizes, the rows' offsets, and the write pass.  The write pass works on tiles of out[0] consecutive queries, a
 * lane per query: the tile's rows are one contiguous byte range of d_out, which the workgroup builds in LDS in windows of
 * out[1] bytes (aligned to multiples of out[1] in d_out) -- names, ids and annotation values are byte copies at arbitrary
 * alignment, and LDS takes those at no cost -- and stores with out[2] bytes per lane, consecutive lanes consecutive
 * addresses.  d_out must start at a 16-byte boundary.  Rows beyond out_cap bytes or max_lines set a status word:
 * kaamer_tsv_rows_finish then returns KAAMER_E_CAPACITY and nothing of d_out is to be read; the stage stays usable.
 * KAAMER_E_ARG naming kaamer_index_attach_subject_text when nothing is attached. */
int kaamer_tsv_rows_device(kaamer_tsv_stage *st, const kaamer_tsv_rows_in *in, char *d_out, uint64_t out_cap, void *stream,
                           kaamer_tsv_rows_result *out);
/* waits for `stream`; counts[0] rows, counts[1] bytes (also filled with what was needed on KAAMER_E_CAPACITY).  Serves
 * both forms; after kaamer_tsv_aln_rows_device also KAAMER_E_RANGE (see there). */
int kaamer_tsv_rows_finish(kaamer_tsv_stage *st, void *stream, uint64_t counts[2]);
/* out[0] queries per tile, out[1] bytes per LDS window, out[2] bytes a lane stores at once, out[3] threads per workgroup */
void kaamer_tsv_geometry(uint32_t out[4]);

/* The -aln rows on the device (tsv_aln_rows.hip.inc), enqueued on `stream` behind kaamer_topn_align_device (and behind
 * kaamer_topn_positions_device with extract_positions): stage, in, d_out, out_cap and the result as
 * kaamer_tsv_rows_device takes and gives them (in->top.d_top_kmatch and d_size_in_kmer are not read); alns: the pair
 * records of the same batch; opts: the request's matrix options -- those the alignment stage ran with -- and its sequence
 * type, whose base decides fields 7 and 8.  Needs both attaches: kaamer_index_attach_subject_text, and
 * kaamer_index_attach_proteins for NumberOfAA (KAAMER_E_ARG names the missing one).  max_results up to 65535.
 *   order    a lane per query sorts its hits by BitScore, descending and stable, once; the three passes read that order.
 *            The missing-entry rule is the host formatter's: the hits it covers carry status 4.
 *   floats   Identity, BitScore and EValue are kaamer_align_finish's, bit for bit.  BitScore and 2^BitScore come from a
 *            table per raw score that the host fills with that function's own arithmetic for the call's options (kept by
 *            the stage while the options stay); the remaining operations are IEEE-rounded on the device.  The table
 *            holds the raw scores -65536 .. 65535 (the reference's tally with the request's gap penalties goes below 0 on
 *            alignments with long gaps).  A pair with a raw score outside it is never printed: the stage counts
 *            such pairs, kaamer_tsv_rows_finish returns KAAMER_E_RANGE and nothing of d_out is to be read -- that batch's
 *            rows are the host formatter's (kaamer_format_tsv_aln).  The stage keeps ONE table: callers that alternate
 *            option sets on one stage refill it (131072 evaluations and a wait for the stream) at every change.
 *   numbers  "%e" and "%.2f" print every finite double exactly (a multi-word routine whose limbs live in LDS).
 * The capacity rule is kaamer_tsv_rows_device's. */
typedef struct {
    char sub_matrix[16];          /* SearchOptions.SubMatrix / GapOpen / GapExtend                                       */
    int32_t gap_open, gap_extend;
    int32_t seq_type;             /* the request's                                                                        */
    int32_t reserved;
} kaamer_tsv_aln_opts;
int kaamer_tsv_aln_rows_device(kaamer_tsv_stage *st, const kaamer_tsv_rows_in *in, const kaamer_topn_alignments *alns,
                               const kaamer_tsv_aln_opts *opts, char *d_out, uint64_t out_cap, void *stream,
                               kaamer_tsv_rows_result *out);
/* of the stage's last -aln call, after kaamer_tsv_rows_finish: out[0] pairs with a raw score outside the table, out[1]
 * raw scores the table holds, out[2] tables the stage has filled so far */
int kaamer_tsv_aln_info(const kaamer_tsv_stage *st, uint64_t out[4]);
/* Test entry: n doubles on the current device, each printed as field 11 (mode 0: "%e") or field 12 (mode 1: "%.2f")
 * prints it, by the device functions the stage uses, into a 32-byte slot of d_out, NUL-padded (a longer text -- "%.2f"
 * of 1e29 and beyond -- is cut at 31 bytes).  Waits for the device. */
int kaamer_tsv_format_doubles_device(const double *d_values, uint64_t n, int32_t mode, char *d_out);

/* The text calls with the rows in the result: what a host shim calls instead of QueryResultHandler + QueryResultWriter's
 * per-field `output += ...` (search.go:505-554) -- it writes the header (kaamer_format_tsv_header) and then the bytes of
 * kaamer_batch_top_tsv to the response.  Arguments, slot, ticket, wait, discard, spans (and text, for BGZF) as
 * kaamer_submit_text_top_flat / kaamer_submit_fasta_top_flat / kaamer_submit_bgzf_top_flat, plus SearchOptions.ExtractPositions
 * and SearchOptions.Annotations.  The stage follows the packing of the block on the slot's stream; with extract_positions
 * the ticket asks for the bitmaps as the _pos calls do, and kaamer_batch_top_positions gives them as well.  The structured
 * result is that of the call without rows.  The rows and their line offsets have a buffer of their own next to the block
 * (the block's format is unchanged: one more device-to-host copy); its two bounds, bytes and rows, start from what the
 * slot's previous call needed plus a quarter, and a batch beyond them is repeated from the parsed buffers with what it
 * reported to need.  KAAMER_E_ARG naming kaamer_index_attach_subject_text when nothing is attached. */
int kaamer_submit_text_top_tsv_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t format, int32_t seq_type,
                                    double min_k_ratio, int64_t min_k_match, uint32_t max_results, int32_t extract_positions,
                                    int32_t annotations, kaamer_ticket **ticket);
int kaamer_search_text_top_tsv_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t format, int32_t seq_type,
                                    double min_k_ratio, int64_t min_k_match, uint32_t max_results, int32_t extract_positions,
                                    int32_t annotations, kaamer_batch_top **out);
int kaamer_submit_fasta_top_tsv_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t seq_type, int32_t upper_last,
                                     double min_k_ratio, int64_t min_k_match, uint32_t max_results, int32_t extract_positions,
                                     int32_t annotations, kaamer_ticket **ticket);
int kaamer_search_fasta_top_tsv_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t seq_type, int32_t upper_last,
                                     double min_k_ratio, int64_t min_k_match, uint32_t max_results, int32_t extract_positions,
                                     int32_t annotations, kaamer_batch_top **out);
int kaamer_submit_bgzf_top_tsv_flat(kaamer_index *ix, const uint8_t *bytes, uint64_t len, int32_t seq_type, double min_k_ratio,
                                    int64_t min_k_match, uint32_t max_results, int32_t extract_positions, int32_t annotations,
                                    kaamer_ticket **ticket);
int kaamer_search_bgzf_top_tsv_flat(kaamer_index *ix, const uint8_t *bytes, uint64_t len, int32_t seq_type, double min_k_ratio,
                                    int64_t min_k_match, uint32_t max_results, int32_t extract_positions, int32_t annotations,
                                    kaamer_batch_top **out);
/* The same three calls with the alignment of the reported hits in between (`-aln -fmt tsv` in one call, search.go:483-494
 * + :556-604): arguments as their _tsv_ twins plus SearchOptions.SubMatrix / GapOpen / GapExtend.  The alignment stage
 * (kaamer_search_batch_top_aln_flat's, want_text = 0) follows the packing of the block on the slot's stream and the -aln
 * rows (kaamer_tsv_aln_rows_device's kernels) follow it, on the pair records in the block.  The structured result is that
 * of the _aln_flat call with want_text = 0 -- numbers only: the TSV form has no AlnString and a text call keeps no host
 * copy of the queries -- read with kaamer_batch_top_alignments (and kaamer_batch_top_positions with extract_positions);
 * kaamer_batch_top_tsv gives the rows, in the result's own order.  Both stages keep their repeat-on-too-small-bounds
 * rule.  Options without a row in AllMatrixScores (or a matrix other than BLOSUM62): every item has status 1 and every
 * row prints the zeros, in sortMapByValue order.  A batch with a raw score outside the stage's table is printed by the
 * host formatter inside kaamer_wait_batch_top, from the finished result and the table of kaamer_index_attach_proteins
 * (attach the same table twice): the same bytes, counted in kaamer_index_tsv_aln_info.  KAAMER_E_ARG naming
 * kaamer_index_attach_proteins or kaamer_index_attach_subject_text when that attach is missing.  The alignment stage
 * sizes its slabs by the longest record, which a text call learns from the spans: one more wait at submit. */
int kaamer_submit_text_top_aln_tsv_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t format, int32_t seq_type,
                                        double min_k_ratio, int64_t min_k_match, uint32_t max_results, int32_t extract_positions,
                                        int32_t annotations, const char *sub_matrix, int32_t gap_open, int32_t gap_extend,
                                        kaamer_ticket **ticket);
int kaamer_search_text_top_aln_tsv_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t format, int32_t seq_type,
                                        double min_k_ratio, int64_t min_k_match, uint32_t max_results, int32_t extract_positions,
                                        int32_t annotations, const char *sub_matrix, int32_t gap_open, int32_t gap_extend,
                                        kaamer_batch_top **out);
int kaamer_submit_fasta_top_aln_tsv_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t seq_type, int32_t upper_last,
                                         double min_k_ratio, int64_t min_k_match, uint32_t max_results, int32_t extract_positions,
                                         int32_t annotations, const char *sub_matrix, int32_t gap_open, int32_t gap_extend,
                                         kaamer_ticket **ticket);
int kaamer_search_fasta_top_aln_tsv_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t seq_type, int32_t upper_last,
                                         double min_k_ratio, int64_t min_k_match, uint32_t max_results, int32_t extract_positions,
                                         int32_t annotations, const char *sub_matrix, int32_t gap_open, int32_t gap_extend,
                                         kaamer_batch_top **out);
int kaamer_submit_bgzf_top_aln_tsv_flat(kaamer_index *ix, const uint8_t *bytes, uint64_t len, int32_t seq_type, double min_k_ratio,
                                        int64_t min_k_match, uint32_t max_results, int32_t extract_positions, int32_t annotations,
                                        const char *sub_matrix, int32_t gap_open, int32_t gap_extend, kaamer_ticket **ticket);
int kaamer_search_bgzf_top_aln_tsv_flat(kaamer_index *ix, const uint8_t *bytes, uint64_t len, int32_t seq_type, double min_k_ratio,
                                        int64_t min_k_match, uint32_t max_results, int32_t extract_positions, int32_t annotations,
                                        const char *sub_matrix, int32_t gap_open, int32_t gap_extend, kaamer_batch_top **out);
/* out[0] batches of those calls whose rows the host printed (a raw score outside the table), out[1] raw scores the table
 * holds.  Test entry: kaamer_index_set_tsv_aln_raw_count makes the table of every stage of the index hold only the first n
 * raw scores from -65536 on (0: all), so that the host path can be reached with ordinary scores; KAAMER_E_BUSY with calls
 * in flight. */
int kaamer_index_tsv_aln_info(kaamer_index *ix, uint64_t out[2]);
int kaamer_index_set_tsv_aln_raw_count(kaamer_index *ix, uint32_t n);
/* The rows of a result: views that live as long as it does; line_off has top_off[n_reported] + 1 entries.  NULL / 0 for a
 * result of any other call (format it on the host: kaamer_format_tsv). */
int kaamer_batch_top_tsv(const kaamer_batch_top *out, const char **text, uint64_t *len, const uint64_t **line_off);
/* The FIRST bounds of the rows (bytes, rows) on every slot of this index, for callers who know what their batches print;
 * 0: the rule.  A batch beyond them is repeated as stated above.  KAAMER_E_BUSY with calls in flight. */
int kaamer_index_set_tsv_bounds(kaamer_index *ix, uint64_t bytes, uint64_t lines);

/* ------------------------------------------------------------------------- */
/* The JSON response (-fmt json: QueryResultHandler, search.go:497-503, one    */
/* json.Marshal(QueryResult) per reported query, Align = false; the opening    */
/* bytes: SetResponseFormatAndHeader, search.go:672-688; the closing bytes:    */
/* search.go:629-632).  An object is Go's struct field order, no whitespace:   */
/*  {"Query":{"Sequence":s,"Name":s,"SizeInKmer":n,"Type":s,                   */
/*            "Location":{"StartPosition":n,"EndPosition":n,"PlusStrand":b,    */
/*                        "StartsAlternative":a},"Contig":s},                  */
/*   "SearchResults":{"Counter":{},"Hits":[...],"PositionHits":{...}},         */
/*   "HitEntries":{...}}                                                       */
/*  Query     a protein request: Type "Protein Query", Sequence the record as   */
/*            searched (the last record's case rule included), StartPosition   */
/*            1, PlusStrand false -- the zero value (search.go:297-303) --,    */
/*            StartsAlternative null (a nil slice), Contig "".  An ORF         */
/*            (nucleotide / reads): Type "DNA Query", Sequence the residues    */
/*            after the trim, Location as after SetBestStartCodon,             */
/*            StartsAlternative [] (dna.go:270), Contig "" for FASTQ records   */
/*            and the record's name for FASTA records (search.go:304-307).     */
/*            Name is the record's whole name (the TSV cuts it at a space).    */
/*  Counter   {}: docs/client.md:147.  The counters library is not part of     */
/*            the reference tree; its marshalled form is taken from there.     */
/*  Hits      [{"Key":id,"Kmatch":n,"Alignment":{...}}] in reporting order;    */
/*            Alignment is the empty AlignmentResult (search.go:144): the      */
/*            thirteen fields of align.go:17-31, zeros as 0, AlnString "".     */
/*  PositionHits  {} for a protein request without ExtractPositions; else one  */
/*            member per reported hit (FilterResults deletes the others,       */
/*            search.go:216-218): the bitmap as searched with the first `trim` */
/*            bits dropped (dna.go:260-262) as [true,false,...]; no bit left:  */
/*            [].                                                              */
/*  HitEntries  one member per reported hit up to, not including, the first id */
/*            without an entry (FetchHitsInformation returns there,            */
/*            search.go:461-463): the Protein with its omitempty tags          */
/*            (protein.pb.go:24-27) -- EntryId, Sequence, Length left out when */
/*            empty or 0, Features when it has no members; an empty feature    */
/*            value is kept; feature names in byte order (Go's map-key order). */
/*  map keys  of PositionHits and HitEntries: the ids as decimal strings,      */
/*            sorted AS STRINGS ("10" < "100" < "9": encoding/json's rule).    */
/*  strings   as encoding/json escapes them with HTML escaping on: '"' and '\' */
/*            get a backslash; \n \r \t; every other byte below 0x20 is        */
/*            \u00XX in lower-case hex -- 0x08 and 0x0c too: the Go release    */
/*            go.mod names has no \b / \f forms, and this library follows it;  */
/*            '<' '>' '&' are \u003c \u003e \u0026; 0x7f is copied.  Bytes   */
/*            from 0x80 up are decoded by utf8.DecodeRune's rules: an invalid*/
/*            byte (a stray continuation, a truncated sequence, an overlong  */
/*            form, a surrogate, a value beyond U+10FFFF) prints \ufffd, one */
/*            per byte; U+2028 / U+2029 print \u2028 / \u2029; every other   */
/*            rune is copied.                                                  */
/* Objects are joined by one ',' (none before the first, none after the last); */
/* a shim writes the header, the bytes of every non-empty batch with ','       */
/* between them, and the trailer.  Objects come in reported-query order (the   */
/* reference's order across its handler goroutines is not deterministic).      */
/* Out of scope: -aln JSON (shortest-round-trip floats and AlnString): a       */
/* result that carries alignments is refused with KAAMER_E_ARG.  The file      */
/* drivers, streams, the sharded handle and the packed-batch calls have the    */
/* host formatter; the device stage serves the text calls.                     */
/* ------------------------------------------------------------------------- */
/* {"dbProteinFeatures":[ + the KStats.Features names, each in quotes, comma-separated and NOT escaped (search.go:672-688
 * writes them so), with annotations only + ],"results":[ .  buf / cap / the return as kaamer_format_tsv_header. */
uint64_t kaamer_format_json_header(int32_t annotations, const kaamer_proteins *proteins, char *buf, uint64_t cap);
/* ]} */
uint64_t kaamer_format_json_trailer(char *buf, uint64_t cap);
/* The objects of any kaamer_batch_top without alignments (packed, _pos, sharded or text), on the caller's thread.
 * seqs / offsets / n_seqs: the packed input of a protein request (record i is seqs[offsets[i], offsets[i + 1]); a text
 * result: what kaamer_parse_fasta gives for the text) -- NULL / 0 for nucleotide / reads, whose Sequence is the result's
 * orf_aa; a record beyond n_seqs prints "".  Names as kaamer_format_tsv takes them.  text_format: 0 FASTA records (Contig
 * is the name), 1 FASTQ records (Contig is "").  The bitmaps are required -- KAAMER_E_ARG on a result without -- when the
 * base of seq_type is not KAAMER_PROTEIN or extract_positions is set.  obj_off (may be NULL): n_reported + 1 entries, the
 * '{' of every object and the total.  Returns the whole length (need = f(NULL, 0)) or a negative code. */
int64_t kaamer_format_json(const kaamer_batch_top *top, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs,
                           const char *name_bytes, uint64_t name_bytes_len, const kaamer_text_span *name_spans, uint32_t n_names,
                           const kaamer_proteins *proteins, int32_t seq_type, int32_t text_format, int32_t extract_positions,
                           char *buf, uint64_t cap, uint64_t *obj_off);
/* The same on a result whose arrays the caller holds itself: alns must be NULL (KAAMER_E_ARG otherwise), the three arrays
 * of kaamer_batch_top_positions all NULL when no bitmaps are required.  Host only. */
int64_t kaamer_format_json_arrays(const kaamer_batch_top *top, const kaamer_alignment *alns, const int32_t *pos_bits_len,
                                  const uint64_t *pos_off, const uint64_t *pos_bits, const uint8_t *seqs, const uint64_t *offsets,
                                  uint32_t n_seqs, const char *name_bytes, uint64_t name_bytes_len,
                                  const kaamer_text_span *name_spans, uint32_t n_names, const kaamer_proteins *proteins,
                                  int32_t seq_type, int32_t text_format, int32_t extract_positions, char *buf, uint64_t cap,
                                  uint64_t *obj_off);
/* Test entry: the bytes of one string as they stand between its quotes; buf / cap / the return as above. */
uint64_t kaamer_json_escape(const uint8_t *bytes, uint64_t len, char *buf, uint64_t cap);
/* Test entry: one HitEntries value, json.Marshal(Protein) of an entry the caller may have built by hand (`found` is not
 * read); feature_names: entry->n_features of them, NUL-terminated (NULL: Features is left out). */
uint64_t kaamer_json_protein_value(const kaamer_protein_entry *entry, const char *const *feature_names, char *buf, uint64_t cap);

/* What the objects need of the protein table, resident next to the index: every entry's HitEntries value (the Protein
 * object, sequence and annotations included), rendered once on the host by the formatter's own code -- the device only
 * copies -- each at a 16-byte boundary, with offsets and the id -> entry map of kaamer_index_attach_subject_text (shared
 * with it, or with kaamer_index_attach_proteins, when one of them holds the same table; else one of its own).  HBM cost:
 * about the database's residues plus its annotations plus 40 bytes per entry.  A second attach replaces the first;
 * KAAMER_E_BUSY with calls in flight; freed by kaamer_index_close. */
int kaamer_index_attach_subject_json(kaamer_index *ix, const kaamer_proteins *proteins);
/* out[0] HBM bytes, out[1] entries, out[2] the longest entry's bytes, out[3] 0; zeros when nothing is attached */
int kaamer_index_subject_json_info(const kaamer_index *ix, uint64_t out[4]);

/* The objects on the device (json_rows.hip.inc), enqueued on `stream` behind kaamer_topn_device and -- where bitmaps are
 * required -- kaamer_topn_positions_device.  Plain device arrays: a workspace's, or fabricated ones. */
typedef struct {
    kaamer_tsv_rows_in rows;            /* as the TSV stage takes it; also read: top.d_trim (NULL: no trim), d_q[].aa_off / */
                                        /* aa_len / plus_strand (the UNTRIMMED window: the stage drops top.d_trim[q]        */
                                        /* residues itself); annotations is not read; extract_positions: PROTEIN only        */
    const uint8_t *d_aa;                /* what aa_off indexes: the packed sequences (protein) / the ORF residues            */
    uint64_t aa_len;                    /* its length: a window beyond it prints ""                                          */
    int32_t seq_type;                   /* the request's                                                                     */
    int32_t text_format;                /* 0 FASTA records, 1 FASTQ records (Contig)                                         */
} kaamer_json_rows_in;
typedef struct {
    const uint64_t *d_obj_off;          /* [objects + 1] the '{' of every object in d_out; the total                         */
    const uint64_t *d_counts;           /* device: {objects, bytes}                                                          */
    uint64_t obj_off_capacity;          /* entries d_obj_off holds                                                           */
} kaamer_json_rows_result;
/* The stage's own buffers (per-query lengths, key orders, tile sums, object offsets) for up to max_queries queries and
 * max_objects objects; one stage serves one stream at a time. */
typedef struct kaamer_json_stage kaamer_json_stage;
int kaamer_json_stage_create(kaamer_index *ix, uint32_t max_queries, uint64_t max_objects, kaamer_json_stage **out);
void kaamer_json_stage_free(kaamer_json_stage *st);
/* Three kernels: lengths, a 64-bit scan, the write pass.  Queries are taken in tiles of out[0]; a WAVE takes one reported
 * query of its tile at a time, so the 64 lanes share every piece of an object: a string is escaped 64 bytes per step
 * (per-lane expansion lengths, a wave prefix sum), a bitmap is expanded 64 bits per step (the trim shifts the bit origin
 * off the word boundary: two words are funnelled), entries and literals are copied 16 bytes per lane.  The keys of a
 * query are ordered once, in the length pass (rank by comparison, max_results^2 / 64 steps per reported query;
 * max_results up to 65535), and the write pass reads that order.  One function, json_object, serves both passes.  A wave
 * builds its object in an LDS buffer of out[1] bytes and stores it in runs aligned to 16 bytes in d_out, out[2] bytes per
 * lane, consecutive lanes consecutive addresses; only the first and last bytes of an object, which share a 16-byte chunk
 * with its neighbours, go out as single bytes.  d_out must start at a 16-byte boundary.  The capacity rule is
 * kaamer_tsv_rows_device's: objects beyond out_cap bytes or max_objects set a status word, kaamer_json_rows_finish
 * returns KAAMER_E_CAPACITY with what was needed, nothing of d_out is to be read, the stage stays usable.  KAAMER_E_ARG
 * naming kaamer_index_attach_subject_json when nothing is attached. */
int kaamer_json_rows_device(kaamer_json_stage *st, const kaamer_json_rows_in *in, char *d_out, uint64_t out_cap, void *stream,
                            kaamer_json_rows_result *out);
/* waits for `stream`; counts[0] objects, counts[1] bytes (also filled with what was needed on KAAMER_E_CAPACITY) */
int kaamer_json_rows_finish(kaamer_json_stage *st, void *stream, uint64_t counts[2]);
/* out[0] queries per tile, out[1] bytes of a wave's LDS buffer, out[2] bytes a lane stores at once, out[3] threads per
 * workgroup */
void kaamer_json_geometry(uint32_t out[4]);

/* The text calls with the objects in the result: what a host shim calls instead of QueryResultHandler's json.Marshal
 * (search.go:497-503) -- it writes the header (kaamer_format_json_header), the bytes of kaamer_batch_top_json of every
 * non-empty batch with ',' between them, and the trailer.  Arguments, slot, ticket, wait, discard, spans (and text, for BGZF)
 * as the _tsv_ twins take them, without `annotations` (an object always carries its entries).  extract_positions matters for
 * KAAMER_PROTEIN only: KAAMER_READS / KAAMER_NUCLEOTIDE requests always ask for the bitmaps, as the _pos calls do
 * (search.go:416), and kaamer_batch_top_positions gives them as well.  Contig is the record's name for the FASTA call and ""
 * for the FASTQ and BGZF calls.  The stage follows the packing of the block on the slot's stream; the structured result is
 * that of the call without objects.  The objects and their offsets have a buffer of their own next to the block (the
 * block's format is unchanged: one more device-to-host copy); its two bounds, bytes and objects, start from what the slot's
 * previous call needed plus a quarter, and a batch beyond them is repeated from the parsed buffers with what it reported to
 * need.  KAAMER_E_ARG naming kaamer_index_attach_subject_json when nothing is attached. */
int kaamer_submit_text_top_json_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t format, int32_t seq_type,
                                     double min_k_ratio, int64_t min_k_match, uint32_t max_results, int32_t extract_positions,
                                     kaamer_ticket **ticket);
int kaamer_search_text_top_json_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t format, int32_t seq_type,
                                     double min_k_ratio, int64_t min_k_match, uint32_t max_results, int32_t extract_positions,
                                     kaamer_batch_top **out);
int kaamer_submit_fasta_top_json_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t seq_type, int32_t upper_last,
                                      double min_k_ratio, int64_t min_k_match, uint32_t max_results, int32_t extract_positions,
                                      kaamer_ticket **ticket);
int kaamer_search_fasta_top_json_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t seq_type, int32_t upper_last,
                                      double min_k_ratio, int64_t min_k_match, uint32_t max_results, int32_t extract_positions,
                                      kaamer_batch_top **out);
int kaamer_submit_bgzf_top_json_flat(kaamer_index *ix, const uint8_t *bytes, uint64_t len, int32_t seq_type, double min_k_ratio,
                                     int64_t min_k_match, uint32_t max_results, int32_t extract_positions, kaamer_ticket **ticket);
int kaamer_search_bgzf_top_json_flat(kaamer_index *ix, const uint8_t *bytes, uint64_t len, int32_t seq_type, double min_k_ratio,
                                     int64_t min_k_match, uint32_t max_results, int32_t extract_positions, kaamer_batch_top **out);
/* The objects of a result: views that live as long as it does; obj_off has n_reported + 1 entries.  NULL / 0 for a result of
 * any other call (format it on the host: kaamer_format_json); kaamer_batch_top_tsv gives NULL for a result of these. */
int kaamer_batch_top_json(const kaamer_batch_top *out, const char **text, uint64_t *len, const uint64_t **obj_off);
/* The FIRST bounds of the objects (bytes, objects) on every slot of this index, for callers who know what their batches
 * print; 0: the rule.  A batch beyond them is repeated as stated above.  KAAMER_E_BUSY with calls in flight. */
int kaamer_index_set_json_bounds(kaamer_index *ix, uint64_t bytes, uint64_t objects);

#ifdef __cplusplus
}
#endif
#endif /* KAAMER_HIP_H */
