// host_out_text.hip.inc — the response text as part of a text call (the kaamer_*_top_tsv_flat, *_top_aln_tsv_flat and
// *_top_json_flat calls, which stand next to their twins in host_text.hip.inc): behind the packed block on the slot's stream
// (included by search.hip inside its extern "C" block, after host_tsv.hip.inc and host_json.hip.inc, whose stages it runs).
//
// The text and the offsets of its units -- rows or objects -- have a buffer of their own next to the block (the block's
// format is unchanged): one more device-to-host copy per call.  Both bounds -- bytes and units -- start from what the slot's
// previous call of the format needed plus a quarter; a batch beyond them reports how much it needs, and is repeated from the
// parsed buffers with exactly that.
//   top_enqueue_out / out_needs_repeat / out_finish_host   the three steps of host_top.hip.inc's enqueue and wait
//   batch_top_out                                          kaamer_batch_top_tsv / kaamer_batch_top_json
struct OutFormatRule {
    const char *noun;              // in error texts
    bool unit_per_hit;             // the hard limit of units: queries x max_results, else queries
    uint64_t first_bytes;          // per unit, where no call has run yet
};
static const OutFormatRule OUT_RULES[OUT_FORMATS] = { { "", false, 0 }, { "TSV rows", true, 64 }, { "JSON objects", false, 2048 } };

static OutStage *slot_stage(TopSlot &h, OutFormat f) { return f == OUT_TSV ? static_cast<OutStage *>(h.tsv) : static_cast<OutStage *>(h.json); }

static int top_enqueue_out(kaamer_ticket *t, TopSlot &h, const kaamer_topn_result *tr, hipStream_t s)
{
    kaamer_index *ix = t->ix;
    const OutFormat f = t->out_fmt;
    const OutFormatRule &rule = OUT_RULES[f];
    // the bounds: the ticket's (a repeat), the slot's guess, the rule
    const uint64_t hard = rule.unit_per_hit ? (uint64_t)h.ws->q_cap * tr->max_results : (uint64_t)h.ws->q_cap;
    uint64_t units = t->out_units_cap ? t->out_units_cap : (h.guess_units[f] ? h.guess_units[f] : (uint64_t)t->n_seqs + 1024);
    if (units > hard) units = hard;
    const uint64_t bytes = t->out_bytes_cap ? t->out_bytes_cap : (h.guess_bytes[f] ? h.guess_bytes[f] : units * rule.first_bytes);
    t->out_units_cap = units; t->out_bytes_cap = bytes;
    if (!slot_stage(h, f) || h.stage_queries[f] < h.ws->q_cap || h.stage_units[f] < units) {
        HIPCHK(hipStreamSynchronize(s));
        int rc;
        if (f == OUT_TSV) { kaamer_tsv_stage_free(h.tsv); h.tsv = nullptr; rc = kaamer_tsv_stage_create(ix, h.ws->q_cap, units, &h.tsv); }
        else { kaamer_json_stage_free(h.json); h.json = nullptr; rc = kaamer_json_stage_create(ix, h.ws->q_cap, units, &h.json); }
        if (rc) return rc;
        h.stage_queries[f] = h.ws->q_cap; h.stage_units[f] = units;
    }
    OutStage *st = slot_stage(h, f);
    { const int rc = reserve(h.d_out, (size_t)bytes + 16, GROW_EXACT, s); if (rc) return rc; }
    const size_t off_bytes = ((size_t)units + 1) * 8, need = off_bytes + (size_t)bytes;
    if (t->h_out_cap < need) {
        if (t->h_out) pinned_put(t->h_out, t->h_out_cap);
        t->h_out = (uint8_t *)pinned_get(need, &t->h_out_cap);
        if (!t->h_out) { t->h_out_cap = 0; return kaamer_fail(KAAMER_E_NOMEM, "pinned %s (%zu bytes)", rule.noun, need); }
    }
    kaamer_json_rows_in jin;
    memset(&jin, 0, sizeof jin);
    kaamer_tsv_rows_in &in = jin.rows;
    in.top = *tr;
    in.d_q = h.ws->d_q; in.d_n_queries = h.ws->d_nq; in.n_queries_cap = h.ws->q_cap;
    in.n_names = t->n_seqs; in.d_name_bytes = t->d_names; in.name_bytes_len = t->names_len; in.d_spans = t->d_spans;
    kaamer_topn_positions pos;
    memset(&pos, 0, sizeof pos);
    if (t->out_pos) {   // the bitmaps are in the block (topn_pack_positions); the per-query layout is the workspace's
        pos.d_pos_base = h.ws->d_tp_base; pos.d_pos_bits_len = h.ws->d_tp_len;
        pos.d_pos_bits = reinterpret_cast<const uint64_t *>(h.d_block.get());   // (replaced on the device by the block's section)
        in.pos = &pos;
    }
    in.extract_positions = t->out_pos; in.annotations = t->out_ann;
    int rc;
    if (f == OUT_JSON) {
        const bool nucl = is_nucl(t->seq_type);
        jin.d_aa = nucl ? h.ws->d_orf_aa.get() : t->d_text_seqs;
        jin.aa_len = nucl ? h.ws->aa_cap : t->seq_bytes;
        jin.seq_type = t->seq_type; jin.text_format = t->json_fasta ? 0 : 1;
        rc = json_enqueue(h.json, &jin, h.d_out, bytes, st->d_unit_off, units + 1, s, h.d_block);
    } else if (t->want_aln) {   // the -aln rows: behind the alignment stage, on the pair records it laid out in the block
        TsvAlnSource src;
        src.on = t->aln.on; src.lambda = t->aln.lambda; src.kk = t->aln.kk; src.seq_type = t->seq_type;
        src.pair_off = h.ws->d_rep_eoff;
        if (src.on) src.lay = h.ws->d_ta_lay;
        rc = tsv_aln_enqueue(h.tsv, &in, src, h.d_out, bytes, st->d_unit_off, units + 1, s, h.d_block);
    } else rc = tsv_enqueue(h.tsv, &in, h.d_out, bytes, st->d_unit_off, units + 1, s, h.d_block);
    if (rc) return rc;
    // the bounds are what the previous call needed plus a quarter: all of both goes home with the block
    HIPCHK(hipMemcpyAsync(t->h_out, st->d_unit_off, off_bytes, hipMemcpyDeviceToHost, s));
    if (bytes) HIPCHK(hipMemcpyAsync(t->h_out + off_bytes, h.d_out, (size_t)bytes, hipMemcpyDeviceToHost, s));
    return KAAMER_OK;
}

// after the stream is done and the block was fine: 1 when the text did not fit (the ticket's bounds are then what it needs)
static int out_needs_repeat(kaamer_ticket *t, TopSlot &h, int *rc)
{
    const OutStage *st = slot_stage(h, t->out_fmt);
    const unsigned long long status = st->h_counts[OUT_C_STATUS], units = st->h_counts[OUT_C_UNITS], bytes = st->h_counts[OUT_C_BYTES];
    if (t->out_fmt == OUT_TSV) {
        if (status & OUT_ST_UPSTREAM) { *rc = kaamer_fail(KAAMER_E_HIP, "tsv rows: the block carries no bitmaps"); return 0; }
        if (t->want_aln && st->h_counts[OUT_C_RAW]) return 0;   // a raw score outside the table: the host prints this batch (tsv_aln_host_rows)
    } else if (status & (OUT_ST_UPSTREAM | OUT_ST_OBJECT | OUT_ST_MISMATCH)) { *rc = kaamer_fail(KAAMER_E_HIP, "json objects: status %llu", status); return 0; }
    if (!status) return 0;
    t->out_units_cap = units + 1; t->out_bytes_cap = bytes + 16;
    return 1;
}

static void out_finish_host(kaamer_ticket *t, TopSlot &h, batch_top_owner *bo)
{
    const OutStage *st = slot_stage(h, t->out_fmt);
    const uint64_t units = st->h_counts[OUT_C_UNITS], bytes = st->h_counts[OUT_C_BYTES];
    h.guess_units[t->out_fmt] = units + units / 4 + 64; h.guess_bytes[t->out_fmt] = bytes + bytes / 4 + 4096;
    bo->out_fmt = t->out_fmt;
    bo->out = t->h_out; bo->out_cap = t->h_out_cap;
    bo->out_units = units; bo->out_len = bytes;
    bo->out_text = reinterpret_cast<const char *>(t->h_out + ((size_t)t->out_units_cap + 1) * 8);
    t->h_out = nullptr;
}

// the text of format f a result carries, with the offsets of its units; a result of any other call: nothing
static int batch_top_out(const kaamer_batch_top *out, OutFormat f, const char *who, const char **text, uint64_t *len, const uint64_t **unit_off)
{
    if (text) *text = nullptr;
    if (len) *len = 0;
    if (unit_off) *unit_off = nullptr;
    if (!out) return kaamer_fail(KAAMER_E_ARG, "%s: bad argument", who);
    const batch_top_owner *bo = reinterpret_cast<const batch_top_owner *>(out);  // pub is the first member
    if (!bo->out || bo->out_fmt != f) return KAAMER_OK;
    if (text) *text = bo->out_text;
    if (len) *len = bo->out_len;
    if (unit_off) *unit_off = reinterpret_cast<const uint64_t *>(bo->out);
    return KAAMER_OK;
}

int kaamer_batch_top_tsv(const kaamer_batch_top *out, const char **text, uint64_t *len, const uint64_t **line_off)
{
    return batch_top_out(out, OUT_TSV, "batch_top_tsv", text, len, line_off);   // nothing: format the rows on the host (kaamer_format_tsv)
}

int kaamer_batch_top_json(const kaamer_batch_top *out, const char **text, uint64_t *len, const uint64_t **obj_off)
{
    return batch_top_out(out, OUT_JSON, "batch_top_json", text, len, obj_off);   // nothing: format the objects on the host (kaamer_format_json)
}
