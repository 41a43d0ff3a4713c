// json_format.cpp — the JSON response on the host (QueryResultHandler, search.go:497-503: json.Marshal(qR) per reported
// query; SetResponseFormatAndHeader, search.go:672-688, and the closing bytes, search.go:629-632), the form without
// alignment.  This is the statement of the contract in the library (the rules: the JSON section of kaamer_hip.h) and the
// route of every result that is not a device text result; json_rows.hip.inc writes the same bytes on the device, and
// kaamer_index_attach_subject_json renders the entries it uploads with kaamer_json_protein_value below.  Pure host code,
// part of the sanitized CPU build (tools/json_check).
#include "kaamer_internal.h"
#include "fmt_out.h"

#include <algorithm>
#include <cstring>

namespace {

// utf8.DecodeRune on s[0, n), n >= 1 and s[0] >= 0x80: the size of the rune, or 0 for the size-1 RuneError (a stray
// continuation, a truncated sequence, an overlong form, a surrogate, a value beyond U+10FFFF, 0xF5 and above)
inline uint32_t utf8_size(const uint8_t *s, uint64_t n)
{
    const uint8_t b0 = s[0];
    uint8_t lo = 0x80, hi = 0xBF;
    uint32_t size;
    if (b0 >= 0xC2 && b0 <= 0xDF) size = 2;
    else if (b0 >= 0xE0 && b0 <= 0xEF) { size = 3; if (b0 == 0xE0) lo = 0xA0; if (b0 == 0xED) hi = 0x9F; }
    else if (b0 >= 0xF0 && b0 <= 0xF4) { size = 4; if (b0 == 0xF0) lo = 0x90; if (b0 == 0xF4) hi = 0x8F; }
    else return 0;
    if (n < size || s[1] < lo || s[1] > hi) return 0;
    for (uint32_t k = 2; k < size; k++)
        if (s[k] < 0x80 || s[k] > 0xBF) return 0;
    return size;
}

// encodeState.string with escapeHTML (encoding/json of the Go release go.mod names: no \b and \f forms), without the quotes
void put_escaped(Out &o, const uint8_t *s, uint64_t n)
{
    static const char hex[] = "0123456789abcdef";
    for (uint64_t i = 0; i < n;) {
        const uint8_t b = s[i];
        if (b < 0x80) {
            i++;
            if (b == '"' || b == '\\') { o.put('\\'); o.put((char)b); }
            else if (b == '\n') o.lit("\\n");
            else if (b == '\r') o.lit("\\r");
            else if (b == '\t') o.lit("\\t");
            else if (b < 0x20 || b == '<' || b == '>' || b == '&') { o.lit("\\u00"); o.put(hex[b >> 4]); o.put(hex[b & 15]); }
            else o.put((char)b);
            continue;
        }
        const uint32_t size = utf8_size(s + i, n - i);
        if (!size) { o.lit("\\ufffd"); i++; continue; }
        if (size == 3 && b == 0xE2 && s[i + 1] == 0x80 && (s[i + 2] == 0xA8 || s[i + 2] == 0xA9)) o.lit(s[i + 2] == 0xA8 ? "\\u2028" : "\\u2029");
        else o.put(reinterpret_cast<const char *>(s + i), size);
        i += size;
    }
}

void put_string(Out &o, const void *s, uint64_t n)
{
    o.put('"');
    if (n) put_escaped(o, static_cast<const uint8_t *>(s), n);
    o.put('"');
}

// json.Marshal(kvstore.Protein), protein.pb.go:24-27: every field omitempty; map keys in byte order.  names: one per feature
void put_protein(Out &o, const kaamer_protein_entry &ent, const char *const *names, std::vector<uint32_t> &order)
{
    const char *sep = "";
    o.put('{');
    if (ent.entry_id_len) { o.lit("\"EntryId\":"); put_string(o, ent.entry_id, ent.entry_id_len); sep = ","; }
    if (ent.sequence_len) { o.lit(sep); o.lit("\"Sequence\":"); put_string(o, ent.sequence, ent.sequence_len); sep = ","; }
    if (ent.length) { o.lit(sep); o.lit("\"Length\":"); o.put_u64(ent.length); sep = ","; }
    if (ent.n_features && names) {
        order.resize(ent.n_features);
        for (uint32_t f = 0; f < ent.n_features; f++) order[f] = f;
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            const size_t la = strlen(names[a]), lb = strlen(names[b]);
            const int c = memcmp(names[a], names[b], la < lb ? la : lb);
            return c ? c < 0 : la < lb;
        });
        o.lit(sep);
        o.lit("\"Features\":{");
        for (uint32_t k = 0; k < ent.n_features; k++) {
            const uint32_t f = order[k];
            if (k) o.put(',');
            put_string(o, names[f], strlen(names[f]));
            o.put(':');
            put_string(o, ent.features + ent.feature_off[f], ent.feature_off[f + 1] - ent.feature_off[f]);
        }
        o.put('}');
    }
    o.put('}');
}

std::vector<const char *> feature_names(const kaamer_proteins *proteins)
{
    std::vector<const char *> names;
    for (uint32_t i = 0, n = proteins ? kaamer_proteins_n_features(proteins) : 0; i < n; i++) names.push_back(kaamer_proteins_feature_name(proteins, i));
    return names;
}

// the decimal string of an id, and the order encoding/json gives integer map keys: as strings
struct Key {
    char s[11];
    uint8_t n;
    uint64_t e;   // the entry of the CSR arrays
    bool operator<(const Key &b) const
    {
        const int c = memcmp(s, b.s, n < b.n ? n : b.n);
        return c ? c < 0 : n < b.n;
    }
};

Key make_key(uint32_t id, uint64_t e)
{
    Key k;
    char tmp[10];
    int n = 0;
    do { tmp[n++] = (char)('0' + id % 10); id /= 10; } while (id);
    k.n = (uint8_t)n;
    for (int i = 0; i < n; i++) k.s[i] = tmp[n - 1 - i];
    k.s[n] = '\0';
    k.e = e;
    return k;
}

const char EMPTY_ALIGNMENT[] =
    "{\"Identity\":0,\"Similarity\":0,\"Length\":0,\"Mismatches\":0,\"GapOpenings\":0,\"Raw\":0,\"BitScore\":0,\"EValue\":0,\"AlnString\":\"\","
    "\"QueryStart\":0,\"QueryEnd\":0,\"SubjectStart\":0,\"SubjectEnd\":0}";

}  // namespace

extern "C" {

uint64_t kaamer_json_protein_value(const kaamer_protein_entry *ent, const char *const *feature_names, char *buf, uint64_t cap)
{
    Out o(buf, cap);
    std::vector<uint32_t> order;
    if (ent) put_protein(o, *ent, feature_names, order);
    o.finish();
    return o.len;
}

uint64_t kaamer_json_escape(const uint8_t *bytes, uint64_t len, char *buf, uint64_t cap)
{
    Out o(buf, cap);
    if (bytes && len) put_escaped(o, bytes, len);
    o.finish();
    return o.len;
}

uint64_t kaamer_format_json_header(int32_t annotations, const kaamer_proteins *proteins, char *buf, uint64_t cap)
{
    Out o(buf, cap);
    o.lit("{\"dbProteinFeatures\":[");
    if (annotations && proteins)
        for (uint32_t i = 0, n = kaamer_proteins_n_features(proteins); i < n; i++) {
            if (i) o.put(',');
            o.put('"');
            o.lit(kaamer_proteins_feature_name(proteins, i));   // as the reference writes them: not escaped
            o.put('"');
        }
    o.lit("],\"results\":[");
    o.finish();
    return o.len;
}

uint64_t kaamer_format_json_trailer(char *buf, uint64_t cap)
{
    Out o(buf, cap);
    o.lit("]}");
    o.finish();
    return o.len;
}

int64_t kaamer_format_json_arrays(const kaamer_batch_top *top, const kaamer_alignment *alns, const int32_t *pos_bits_len, const uint64_t *pos_off,
                                  const uint64_t *pos_bits, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, const char *name_bytes,
                                  uint64_t name_bytes_len, const kaamer_text_span *name_spans, uint32_t n_names, const kaamer_proteins *proteins,
                                  int32_t seq_type, int32_t text_format, int32_t extract_positions, char *buf, uint64_t cap, uint64_t *obj_off)
{
    if (!top || (top->n_reported && (!top->q || !top->top_off || !top->top_pid || !top->top_kmatch)) || (n_names && !name_spans) || (n_seqs && (!seqs || !offsets)))
        return kaamer_fail(KAAMER_E_ARG, "format_json: bad argument");
    if (alns) return kaamer_fail(KAAMER_E_ARG, "format_json: a result with alignments (-aln JSON is not written here)");
    const bool protein = KAAMER_SEQ_TYPE_BASE(seq_type) == KAAMER_PROTEIN;
    const bool positions = !protein || extract_positions;   // search.go:416
    if (positions && top->n_reported && (!pos_bits_len || !pos_off || !pos_bits))
        return kaamer_fail(KAAMER_E_ARG, "format_json: PositionHits on a result without bitmaps (ask for them: the _pos calls)");
    if (!protein && top->n_reported && !top->orf_aa) return kaamer_fail(KAAMER_E_ARG, "format_json: a result without ORF residues");
    Out o(buf, cap);
    std::vector<Key> keys;
    std::vector<uint32_t> order;
    const std::vector<const char *> names = feature_names(proteins);
    for (uint32_t i = 0; i < top->n_reported; i++) {
        const kaamer_query_meta &q = top->q[i];
        if (i) o.put(',');
        if (obj_off) obj_off[i] = o.len;
        const char *name = nullptr;
        uint64_t name_len = 0;
        if (q.src_seq < n_names && name_bytes && (uint64_t)name_spans[q.src_seq].name_off + name_spans[q.src_seq].name_len <= name_bytes_len) {
            name = name_bytes + name_spans[q.src_seq].name_off;
            name_len = name_spans[q.src_seq].name_len;
        }
        o.lit("{\"Query\":{\"Sequence\":");
        if (protein) {
            if (q.src_seq < n_seqs) put_string(o, seqs + offsets[q.src_seq], offsets[q.src_seq + 1] - offsets[q.src_seq]);
            else o.lit("\"\"");
        } else {
            put_string(o, top->orf_aa + q.aa_off, q.aa_len);
        }
        o.lit(",\"Name\":");
        put_string(o, name, name_len);
        o.lit(",\"SizeInKmer\":");
        o.put_int(q.size_in_kmer);
        o.lit(protein ? ",\"Type\":\"Protein Query\"" : ",\"Type\":\"DNA Query\"");
        o.lit(",\"Location\":{\"StartPosition\":");
        o.put_int(q.start_position);
        o.lit(",\"EndPosition\":");
        o.put_int(q.end_position);
        o.lit(!protein && q.plus_strand ? ",\"PlusStrand\":true" : ",\"PlusStrand\":false");
        o.lit(protein ? ",\"StartsAlternative\":null}" : ",\"StartsAlternative\":[]}");
        o.lit(",\"Contig\":");
        if (!protein && text_format == 0) put_string(o, name, name_len);
        else o.lit("\"\"");
        o.lit("},\"SearchResults\":{\"Counter\":{},\"Hits\":[");
        const uint64_t e0 = top->top_off[i], e1 = top->top_off[i + 1];
        keys.clear();
        for (uint64_t e = e0; e < e1; e++) {
            if (e > e0) o.put(',');
            o.lit("{\"Key\":");
            o.put_u64(top->top_pid[e]);
            o.lit(",\"Kmatch\":");
            o.put_u64(top->top_kmatch[e]);
            o.lit(",\"Alignment\":");
            o.lit(EMPTY_ALIGNMENT);
            o.put('}');
            keys.push_back(make_key(top->top_pid[e], e));
        }
        o.lit("],\"PositionHits\":{");
        if (positions) {
            std::sort(keys.begin(), keys.end());
            const int64_t bits = pos_bits_len[i], trim = top->trim ? top->trim[i] : 0;
            for (size_t k = 0; k < keys.size(); k++) {
                if (k) o.put(',');
                o.put('"');
                o.put(keys[k].s, keys[k].n);
                o.lit("\":[");
                const uint64_t *w = pos_bits + pos_off[keys[k].e];
                const int64_t first = trim < 0 ? 0 : trim;   // dna.go:260-262: the first `trim` bits are dropped
                for (int64_t b = first; b < bits; b++) {
                    if (b > first) o.put(',');
                    o.lit((w[b >> 6] >> (b & 63)) & 1 ? "true" : "false");
                }
                o.put(']');
            }
        }
        o.lit("}},\"HitEntries\":{");
        // FetchHitsInformation returns at the first id without an entry (search.go:461-463), in reporting order
        keys.clear();
        for (uint64_t e = e0; e < e1 && proteins; e++) {
            kaamer_protein_entry ent;
            memset(&ent, 0, sizeof ent);
            (void)kaamer_fetch_hits(proteins, &top->top_pid[e], 1, &ent);
            if (!ent.found) break;
            keys.push_back(make_key(top->top_pid[e], e));
        }
        std::sort(keys.begin(), keys.end());
        for (size_t k = 0; k < keys.size(); k++) {
            kaamer_protein_entry ent;
            memset(&ent, 0, sizeof ent);
            (void)kaamer_fetch_hits(proteins, &top->top_pid[keys[k].e], 1, &ent);
            if (k) o.put(',');
            o.put('"');
            o.put(keys[k].s, keys[k].n);
            o.lit("\":");
            put_protein(o, ent, names.empty() ? nullptr : names.data(), order);
        }
        o.lit("}}");
    }
    if (obj_off) obj_off[top->n_reported] = o.len;
    o.finish();
    return (int64_t)o.len;
}

}  // extern "C"
