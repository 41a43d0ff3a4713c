// tsv_format.cpp — the TSV response rows on the host (QueryResultHandler, search.go:505-554, the form without alignment,
// and :556-604, the -aln form; SetResponseFormatAndHeader, search.go:636-662).  This is the statement of the contract in
// the library and the route of every result that is not a device text result; tsv_rows.hip.inc and tsv_aln_rows.hip.inc
// write the same bytes on the device.  Pure host code, part of the sanitized CPU build (tools/asan).
#include "kaamer_internal.h"
#include "fmt_double.h"
#include "fmt_out.h"

#include <cmath>
#include <cstring>

namespace {

// fmt.Sprintf("%.2f", float32(kmatch) / float32(size) * float32(100)), search.go:514: the quotient and the product are
// each rounded to float32; strconv then prints the float32's EXACT value to two decimals, ties to even.  A float32 times
// 100 is exact in double (24 + 7 bits), so hundredths = x * 100.0 has no error and the tie is decided on its parity.
void put_identity(Out &o, uint32_t kmatch, int32_t size)
{
    volatile float quotient = (float)kmatch / (float)size;   // (volatile: no wider intermediate, whatever the flags)
    volatile float x = quotient * 100.0f;
    const float xv = x;
    if (std::isnan(xv)) { o.lit("NaN"); return; }
    if (std::isinf(xv)) { o.lit(xv > 0 ? "+Inf" : "-Inf"); return; }
    const bool neg = std::signbit(xv);
    const double v = std::fabs((double)xv) * 100.0;
    const double fl = std::floor(v), frac = v - fl;
    uint64_t cents = (uint64_t)fl;
    if (frac > 0.5 || (frac == 0.5 && (cents & 1))) cents++;
    if (neg) o.put('-');
    o.put_u64(cents / 100);
    o.put('.');
    o.put((char)('0' + cents / 10 % 10));
    o.put((char)('0' + cents % 10));
}

// strings.Split(Query.Name, " ")[0] of record src_seq: NULL / 0 for a record beyond the names or a span beyond the bytes
const char *query_id(const kaamer_query_meta &q, const char *name_bytes, uint64_t name_bytes_len, const kaamer_text_span *name_spans, uint32_t n_names,
                     uint64_t *len)
{
    *len = 0;
    if (q.src_seq >= n_names) return nullptr;
    const kaamer_text_span &sp = name_spans[q.src_seq];
    if ((uint64_t)sp.name_off + sp.name_len > name_bytes_len || !name_bytes) return nullptr;
    const char *name = name_bytes + sp.name_off;
    const void *space = memchr(name, ' ', sp.name_len);
    *len = space ? (uint64_t)((const char *)space - name) : sp.name_len;
    return name;
}

}  // namespace

extern "C" {

uint64_t kaamer_format_tsv_header(int32_t extract_positions, int32_t annotations, const kaamer_proteins *proteins, char *buf, uint64_t cap)
{
    Out o(buf, cap);
    o.lit("QueryId\tSubjectId\t%KMatchIdentity\tQueryKLength\tKMatch\tGapOpen\tQStart\tQEnd\tSStart\tSEnd");
    if (extract_positions) o.lit("\tQueryPositions");
    if (annotations && proteins)
        for (uint32_t i = 0, n = kaamer_proteins_n_features(proteins); i < n; i++) {
            o.put('\t');
            o.lit(kaamer_proteins_feature_name(proteins, i));
        }
    o.put('\n');
    o.finish();
    return o.len;
}

// search.go:649 + :651-660
uint64_t kaamer_format_tsv_aln_header(int32_t extract_positions, int32_t annotations, const kaamer_proteins *proteins, char *buf, uint64_t cap)
{
    Out o(buf, cap);
    o.lit("QueryId\tSubjectId\t%Identity\tAlnLength\tMismatches\tGapOpen\tQStart\tQEnd\tSStart\tSEnd\tEvalue\tBitscore");
    if (extract_positions) o.lit("\tQueryPositions");
    if (annotations && proteins)
        for (uint32_t i = 0, n = kaamer_proteins_n_features(proteins); i < n; i++) {
            o.put('\t');
            o.lit(kaamer_proteins_feature_name(proteins, i));
        }
    o.put('\n');
    o.finish();
    return o.len;
}

// search.go:556-604: the rows of a result whose hits carry alignments (alns[e] belongs to entry e, the hits in the result's
// own order: BitScore descending).  Identity is a float32, widened exactly; EValue and BitScore are the doubles as they are.
int64_t kaamer_format_tsv_aln_arrays(const kaamer_batch_top *top, const kaamer_alignment *alns, const int32_t *pos_bits_len, const uint64_t *pos_off,
                                     const uint64_t *pos_bits, const char *name_bytes, uint64_t name_bytes_len, const kaamer_text_span *name_spans,
                                     uint32_t n_names, const kaamer_proteins *proteins, int32_t seq_type, int32_t extract_positions, int32_t annotations,
                                     char *buf, uint64_t cap, uint64_t *line_off)
{
    if (!top || (top->n_reported && (!top->q || !top->top_off || !top->top_pid)) || (n_names && !name_spans))
        return kaamer_fail(KAAMER_E_ARG, "format_tsv_aln: bad argument");
    if (!alns) return kaamer_fail(KAAMER_E_ARG, "format_tsv_aln: a result without alignments (ask for them: the _aln calls)");
    if (extract_positions && top->n_reported && (!pos_bits_len || !pos_off || !pos_bits))
        return kaamer_fail(KAAMER_E_ARG, "format_tsv_aln: ExtractPositions on a result without bitmaps (ask for them: want_positions)");
    const uint32_t nf = (annotations && proteins) ? kaamer_proteins_n_features(proteins) : 0;
    const bool protein = KAAMER_SEQ_TYPE_BASE(seq_type) == KAAMER_PROTEIN;
    Out o(buf, cap);
    KfmtArray limbs;
    std::vector<char> positions;
    for (uint32_t i = 0; i < top->n_reported; i++) {
        const kaamer_query_meta &q = top->q[i];
        uint64_t name_len = 0;
        const char *name = query_id(q, name_bytes, name_bytes_len, name_spans, n_names, &name_len);
        // FetchHitsInformation returned at a missing id, BEFORE the sort: no entry from that hit on in sortMapByValue order
        // (search.go:461-463).  Those hits carry status 4; a result that was not aligned (status 1) is still in that order.
        bool gone = false;
        for (uint64_t e = top->top_off[i]; e < top->top_off[i + 1]; e++) {
            if (line_off) line_off[e] = o.len;
            const kaamer_alignment &a = alns[e];
            kaamer_protein_entry ent;
            memset(&ent, 0, sizeof ent);
            if (a.status != 4 && !(gone && a.status == 1) && proteins) (void)kaamer_fetch_hits(proteins, &top->top_pid[e], 1, &ent);
            if (!ent.found) { gone = true; memset(&ent, 0, sizeof ent); }
            o.put(name, name_len);
            o.put('\t');
            o.put(ent.entry_id, ent.entry_id_len);
            o.put('\t');
            kfmt_fixed2(o, (double)a.identity, limbs);
            o.put('\t');
            o.put_int(a.length);
            o.put('\t');
            o.put_int(a.mismatches);
            o.put('\t');
            o.put_int(a.gap_openings);
            o.put('\t');
            o.put_int(protein ? a.query_start : q.start_position);
            o.put('\t');
            o.put_int(protein ? a.query_end : q.end_position);
            o.put('\t');
            o.put_int(a.subject_start);
            o.put('\t');
            o.put_int(a.subject_end);
            o.put('\t');
            kfmt_exp6(o, a.evalue, limbs);
            o.put('\t');
            kfmt_fixed2(o, a.bitscore, limbs);
            if (extract_positions) {
                const uint64_t pos_len = kaamer_format_positions(pos_bits + pos_off[e], pos_bits_len[i], 1, nullptr, 0);
                positions.resize((size_t)pos_len + 1);
                (void)kaamer_format_positions(pos_bits + pos_off[e], pos_bits_len[i], 1, positions.data(), pos_len + 1);
                o.put('\t');
                o.put(positions.data(), pos_len);
            }
            for (uint32_t f = 0; f < nf; f++) {
                o.put('\t');
                if (ent.found && f < ent.n_features) o.put(ent.features + ent.feature_off[f], ent.feature_off[f + 1] - ent.feature_off[f]);
            }
            o.put('\n');
        }
    }
    if (line_off) line_off[top->n_reported ? top->top_off[top->n_reported] : 0] = o.len;
    o.finish();
    return (int64_t)o.len;
}

// the same two formats of one double on their own: what the device's kaamer_tsv_format_doubles_device is held against
uint64_t kaamer_format_double(double value, int32_t mode, char *buf, uint64_t cap)
{
    Out o(buf, cap);
    KfmtArray limbs;
    if (mode == 0) kfmt_exp6(o, value, limbs);
    else kfmt_fixed2(o, value, limbs);
    o.finish();
    return o.len;
}

int64_t kaamer_format_tsv_arrays(const kaamer_batch_top *top, const int32_t *pos_bits_len, const uint64_t *pos_off, const uint64_t *pos_bits,
                                 const char *name_bytes, uint64_t name_bytes_len, const kaamer_text_span *name_spans, uint32_t n_names,
                                 const kaamer_proteins *proteins, int32_t extract_positions, int32_t annotations, char *buf, uint64_t cap,
                                 uint64_t *line_off)
{
    if (!top || (top->n_reported && (!top->q || !top->top_off || !top->top_pid || !top->top_kmatch)) || (n_names && !name_spans))
        return kaamer_fail(KAAMER_E_ARG, "format_tsv: bad argument");
    if (extract_positions && top->n_reported && (!pos_bits_len || !pos_off || !pos_bits))
        return kaamer_fail(KAAMER_E_ARG, "format_tsv: ExtractPositions on a result without bitmaps (ask for them: the _pos calls)");
    const uint32_t nf = (annotations && proteins) ? kaamer_proteins_n_features(proteins) : 0;
    Out o(buf, cap);
    std::vector<char> positions;
    for (uint32_t i = 0; i < top->n_reported; i++) {
        const kaamer_query_meta &q = top->q[i];
        uint64_t name_len = 0;
        const char *name = query_id(q, name_bytes, name_bytes_len, name_spans, n_names, &name_len);
        bool gone = false;   // FetchHitsInformation returned at a missing id: no entry from that hit on (search.go:461-463)
        for (uint64_t e = top->top_off[i]; e < top->top_off[i + 1]; e++) {
            if (line_off) line_off[e] = o.len;
            kaamer_protein_entry ent;
            memset(&ent, 0, sizeof ent);
            if (!gone && proteins) (void)kaamer_fetch_hits(proteins, &top->top_pid[e], 1, &ent);
            if (!ent.found) { gone = true; memset(&ent, 0, sizeof ent); }
            o.put(name, name_len);
            o.put('\t');
            o.put(ent.entry_id, ent.entry_id_len);
            o.put('\t');
            put_identity(o, top->top_kmatch[e], q.size_in_kmer);
            o.put('\t');
            o.put_int(q.size_in_kmer);
            o.put('\t');
            o.put_u64(top->top_kmatch[e]);
            o.put('\t');
            uint64_t pos_len = 0;
            if (extract_positions) {
                pos_len = kaamer_format_positions(pos_bits + pos_off[e], pos_bits_len[i], 0, nullptr, 0);
                positions.resize((size_t)pos_len + 1);
                (void)kaamer_format_positions(pos_bits + pos_off[e], pos_bits_len[i], 0, positions.data(), pos_len + 1);
                uint64_t commas = 0;
                for (uint64_t k = 0; k < pos_len; k++) commas += positions[(size_t)k] == ',';
                o.put_u64(commas);
            } else {
                o.lit("N/A");
            }
            o.put('\t');
            o.put_int(q.start_position);
            o.put('\t');
            o.put_int(q.end_position);
            o.lit("\t1\t");
            if (annotations) o.put_u64(ent.length);
            else o.lit("N/A");
            if (extract_positions) {
                o.put('\t');
                o.put(positions.data(), pos_len);
            }
            for (uint32_t f = 0; f < nf; f++) {
                o.put('\t');
                if (ent.found && f < ent.n_features) o.put(ent.features + ent.feature_off[f], ent.feature_off[f + 1] - ent.feature_off[f]);
            }
            o.put('\n');
        }
    }
    if (line_off) line_off[top->n_reported ? top->top_off[top->n_reported] : 0] = o.len;
    o.finish();
    return (int64_t)o.len;
}

}  // extern "C"
