// json_rows.hip.inc — the JSON objects of the reported queries, written on the device (included by search.hip after
// tsv_aln_rows.hip.inc; tiles, scans, counts and the scan kernel are out_rows.hip.inc's; the host side is host_json.hip.inc,
// the contract and the host formatter are in json_format.cpp).
//
// json.Marshal(QueryResult) (search.go:497-503) needs what the TSV rows need plus the query's residues, the trim and every
// hit's whole entry (kaamer_index_attach_subject_json: the HitEntries values, rendered on the host).  A row is short and a
// lane writes it; an object runs from a few hundred bytes to hundreds of KB, so here a WAVE takes an object and its 64 lanes
// share every piece of it:
//   strings    64 bytes per step: every lane the expansion length of its byte (json_esc_len: context-free, a lead byte or an
//              ASCII byte always starts a rune, a continuation byte is looked up from the at most three bytes before it), a
//              wave prefix sum, every lane writes its own expansion
//   bitmaps    64 bits per step, funnelled out of two words (the trim moves the bit origin off the word boundary); lane i
//              writes "true," or "false," at 6 i - popcount(bits below i)
//   entries, literals   byte copies, 16 bytes per lane and step
//   json_len_kernel    a workgroup per tile of OUT_TILE queries: the reported ones are listed, the waves take them in turn;
//                      json_object into a counting sink; the order of the query's keys (as decimal strings) is ranked here,
//                      once, and kept for the write pass; lengths per query, sums per tile
//   out_scan_kernel    (out_rows.hip.inc), one separator byte per object: the comma between two objects
//   json_write_kernel  the same tiles and turns; json_object into a sink that builds the object in the wave's LDS buffer and
//                      stores it in runs aligned to 16 bytes in the output, 16 bytes per lane, consecutive lanes consecutive
//                      addresses; the bytes an object shares a 16-byte chunk with its neighbours in go out one by one
// The same json_object serves both passes, so they cannot disagree about an object; should they ever, nothing is stored
// beyond the object's counted end and the status word says so.
#define JSON_WAVES (OUT_TILE / 64u)
#define JSON_WIN 4096u     /* bytes of a wave's LDS buffer */
#define JSON_STEP 1024u    /* the most one step appends */
#define JSON_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

struct JsonParams : OutParams {    // positions: the bitmaps are printed; a unit is an object
    const int32_t *trim;           // NULL: none
    const uint8_t *aa;             // what q[].aa_off indexes
    uint64_t aa_len;
    int protein, fasta;
    // the subject entries: entry i is sj_bytes[sj_off[i], + sj_len[i]), sj_off[i] a multiple of 16
    const uint8_t *sj_bytes;
    const uint64_t *sj_off;
    const uint32_t *sj_len;
    // the stage's own
    uint32_t *obj_len;             // per query
    uint16_t *order;               // [q * K + k]: the hit whose key is k-th in string order
};

__device__ __forceinline__ uint32_t json_wave_incl(uint32_t v)
{
    const uint32_t lane = lane_id();
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// utf8.DecodeRune on s[i ..), s[i] >= 0xC0: the rune's size, 0 for the size-1 RuneError
__device__ __forceinline__ uint32_t json_rune_size(const uint8_t *s, uint64_t len, uint64_t i)
{
    const uint32_t b0 = s[i];
    uint32_t lo = 0x80u, hi = 0xBFu, size;
    if (b0 >= 0xC2u && b0 <= 0xDFu) size = 2;
    else if (b0 >= 0xE0u && b0 <= 0xEFu) { size = 3; if (b0 == 0xE0u) lo = 0xA0u; if (b0 == 0xEDu) hi = 0x9Fu; }
    else if (b0 >= 0xF0u && b0 <= 0xF4u) { size = 4; if (b0 == 0xF0u) lo = 0x90u; if (b0 == 0xF4u) hi = 0x8Fu; }
    else return 0;
    if (len - i < size) return 0;
    const uint32_t b1 = s[i + 1];
    if (b1 < lo || b1 > hi) return 0;
    for (uint32_t k = 2; k < size; k++) {
        const uint32_t b = s[i + k];
        if (b < 0x80u || b > 0xBFu) return 0;
    }
    return size;
}

enum { JSON_E_COPY = 0, JSON_E_SHORT = 1, JSON_E_U00 = 2, JSON_E_BAD = 3, JSON_E_2028 = 4, JSON_E_2029 = 5, JSON_E_NONE = 6 };

// what byte i of a string becomes (encodeState.string with escapeHTML): the kind, and through *n the bytes it puts out --
// a rune's bytes are put out by its first byte, the others put out nothing
__device__ __forceinline__ uint32_t json_esc_len(const uint8_t *s, uint64_t len, uint64_t i, uint32_t *n)
{
    const uint32_t b = s[i];
    if (b < 0x80u) {
        if (b == '"' || b == '\\' || b == '\n' || b == '\r' || b == '\t') { *n = 2; return JSON_E_SHORT; }
        if (b < 0x20u || b == '<' || b == '>' || b == '&') { *n = 6; return JSON_E_U00; }
        *n = 1;
        return JSON_E_COPY;
    }
    if (b < 0xC0u) {   // a continuation byte: inside a valid rune that starts up to three bytes before, or stray
        for (uint32_t k = 1; k <= 3u && k <= i; k++) {
            const uint32_t lead = s[i - k];
            if (lead >= 0xC0u) {
                if (json_rune_size(s, len, i - k) > k) { *n = 0; return JSON_E_NONE; }
                break;
            }
            if (lead < 0x80u) break;
        }
        *n = 6;
        return JSON_E_BAD;
    }
    const uint32_t size = json_rune_size(s, len, i);
    if (!size) { *n = 6; return JSON_E_BAD; }
    if (size == 3 && b == 0xE2u && s[i + 1] == 0x80u && (s[i + 2] == 0xA8u || s[i + 2] == 0xA9u)) { *n = 6; return s[i + 2] == 0xA8u ? JSON_E_2028 : JSON_E_2029; }
    *n = size;
    return JSON_E_COPY;
}

__device__ __forceinline__ char json_hex(uint32_t v) { return (char)(v < 10u ? '0' + v : 'a' + (v - 10u)); }

// counts the bytes of an object; every lane holds the same count
struct JsonCount {
    static constexpr bool ORDERED = false;   // members of a map in any order: the count is the same (the order is not ranked yet)
    unsigned long long n = 0;
    __device__ __forceinline__ void lit(const char *, uint32_t len) { n += len; }
    __device__ __forceinline__ void put_u32(uint32_t v) { n += out_digits(v); }
    __device__ __forceinline__ void copy(const uint8_t *, uint64_t len) { n += len; }
    __device__ __forceinline__ void escaped(const uint8_t *s, uint64_t len)
    {
        unsigned long long mine = 0;
        for (uint64_t i = lane_id(); i < len; i += 64u) {
            uint32_t e;
            (void)json_esc_len(s, len, i, &e);
            mine += e;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
        n += mine;
    }
    // m bits (1 .. 64) of a bitmap, the bits from m on cleared; last: no comma behind the last one
    __device__ __forceinline__ void bits64(unsigned long long w, uint32_t m, bool last) { n += 6ull * m - (uint32_t)__popcll(w) - (last ? 1u : 0u); }
};

// builds the object in the wave's LDS buffer: win[0] is byte `wbase` of the output (a multiple of 16), the object's bytes
// are [lo, end), `pos` is the next one.  Every step makes room first (at most JSON_STEP bytes a step), so a flush happens
// between steps only: it stores what is complete up to the last 16-byte boundary and keeps the rest.
struct JsonWrite {
    static constexpr bool ORDERED = true;
    char *win;
    char *out;
    unsigned long long pos, wbase, lo, end;
    __device__ __forceinline__ void flush(bool final)
    {
        JSON_SYNC();
        const uint32_t lane = lane_id();
        unsigned long long hi = final ? pos : pos & ~15ull;
        if (hi > end) hi = end;   // (never beyond what the length pass counted)
        const unsigned long long a = lo > wbase ? lo : wbase;
        if (hi > a) {
            unsigned long long a16 = (a + 15ull) & ~15ull, h16 = hi & ~15ull;
            if (a16 > hi) a16 = hi;
            if (h16 < a16) h16 = a16;
            if (a + lane < a16) out[a + lane] = win[a - wbase + lane];
            for (unsigned long long c = a16 + 16ull * lane; c < h16; c += 1024ull)
                *reinterpret_cast<uint4 *>(out + c) = *reinterpret_cast<const uint4 *>(win + (c - wbase));
            if (h16 + lane < hi) out[h16 + lane] = win[h16 - wbase + lane];
        }
        // the bytes behind the boundary move to the front
        const unsigned long long keep = pos & ~15ull;
        const uint32_t rest = (uint32_t)(pos - keep);
        const char c = lane < rest ? win[keep - wbase + lane] : (char)0;
        JSON_SYNC();
        if (lane < rest) win[lane] = c;
        wbase = keep;
        JSON_SYNC();
    }
    __device__ __forceinline__ uint32_t room()
    {
        if (pos - wbase + JSON_STEP > JSON_WIN) flush(false);
        return (uint32_t)(pos - wbase);
    }
    __device__ __forceinline__ void lit(const char *s, uint32_t len)
    {
        const uint32_t at = room();
        for (uint32_t i = lane_id(); i < len; i += 64u) win[at + i] = s[i];
        pos += len;
    }
    __device__ __forceinline__ void put_u32(uint32_t v)
    {
        const uint32_t at = room(), d = out_digits(v), lane = lane_id();
        if (lane < d) {
            uint32_t div = 1;
            for (uint32_t k = lane + 1; k < d; k++) div *= 10u;
            win[at + lane] = (char)('0' + v / div % 10u);
        }
        pos += d;
    }
    __device__ __forceinline__ void copy(const uint8_t *src, uint64_t len)
    {
        const uint32_t lane = lane_id();
        for (uint64_t done = 0; done < len; done += JSON_STEP) {
            const uint32_t at = room();
            const uint32_t n = len - done < JSON_STEP ? (uint32_t)(len - done) : JSON_STEP;
            const uint8_t *s = src + done + 16u * lane;
            char *d = win + at + 16u * lane;
            if (16u * lane + 16u <= n) {
                if (((uintptr_t)src & 15u) == 0) {   // (the entries: one 16-byte load; done is a multiple of 16)
                    const uint4 v = *reinterpret_cast<const uint4 *>(s);
                    const uint32_t w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
                    for (int k = 0; k < 16; k++) d[k] = (char)(w[k >> 2] >> (8 * (k & 3)));
                } else {
                    uint8_t t[16];
#pragma unroll
                    for (int k = 0; k < 16; k++) t[k] = s[k];
#pragma unroll
                    for (int k = 0; k < 16; k++) d[k] = (char)t[k];
                }
            } else {
                for (uint32_t k = 0; 16u * lane + k < n; k++) d[k] = (char)s[k];
            }
            pos += n;
        }
    }
    __device__ __forceinline__ void escaped(const uint8_t *s, uint64_t len)
    {
        const uint32_t lane = lane_id();
        for (uint64_t base = 0; base < len; base += 64u) {
            const uint32_t at = room();
            const uint64_t i = base + lane;
            uint32_t e = 0, kind = JSON_E_NONE;
            if (i < len) kind = json_esc_len(s, len, i, &e);
            const uint32_t incl = json_wave_incl(e);
            char *d = win + at + (incl - e);
            if (e) {
                const uint32_t b = s[i];
                if (kind == JSON_E_COPY) {
                    for (uint32_t k = 0; k < e; k++) d[k] = (char)s[i + k];
                } else if (kind == JSON_E_SHORT) {
                    d[0] = '\\';
                    d[1] = b == '\n' ? 'n' : b == '\r' ? 'r' : b == '\t' ? 't' : (char)b;
                } else {
                    d[0] = '\\'; d[1] = 'u';
                    if (kind == JSON_E_U00) { d[2] = '0'; d[3] = '0'; d[4] = json_hex(b >> 4); d[5] = json_hex(b & 15u); }
                    else if (kind == JSON_E_BAD) { d[2] = 'f'; d[3] = 'f'; d[4] = 'f'; d[5] = 'd'; }
                    else { d[2] = '2'; d[3] = '0'; d[4] = '2'; d[5] = kind == JSON_E_2028 ? '8' : '9'; }
                }
            }
            pos += __shfl(incl, 63, 64);
        }
    }
    __device__ __forceinline__ void bits64(unsigned long long w, uint32_t m, bool last)
    {
        const uint32_t at = room(), lane = lane_id();
        if (lane < m) {
            const bool set = (w >> lane) & 1ull;
            char *d = win + at + 6u * lane - (uint32_t)__popcll(w & ((1ull << lane) - 1ull));
            if (set) { d[0] = 't'; d[1] = 'r'; d[2] = 'u'; d[3] = 'e'; d += 4; }
            else { d[0] = 'f'; d[1] = 'a'; d[2] = 'l'; d[3] = 's'; d[4] = 'e'; d += 5; }
            if (!(last && lane + 1u == m)) d[0] = ',';
        }
        pos += 6ull * m - (uint32_t)__popcll(w) - (last ? 1u : 0u);
    }
};

#define JL(o, s) (o).lit(s, (uint32_t)(sizeof(s) - 1))

template <class Sink> __device__ __forceinline__ void json_put_i32(Sink &o, int32_t v)   // strconv.Itoa
{
    if (v < 0) { JL(o, "-"); o.put_u32(0u - (uint32_t)v); }
    else o.put_u32((uint32_t)v);
}

// bits [first, n) of a bitmap as true / false words
template <class Sink> __device__ __forceinline__ void json_put_bits(Sink &o, const uint64_t *bits, uint32_t n, uint32_t first)
{
    const uint32_t words = (n + 63u) >> 6;
    for (uint32_t b = first; b < n; b += 64u) {
        const uint32_t m = n - b < 64u ? n - b : 64u, wi = b >> 6, s = b & 63u;
        unsigned long long w = bits[wi] >> s;
        if (s && wi + 1u < words) w |= bits[wi + 1u] << (64u - s);
        if (m < 64u) w &= (1ull << m) - 1ull;
        o.bits64(w, m, b + m >= n);
    }
}

// is the decimal string of a before that of b?  (encoding/json sorts integer map keys as strings.)  The shorter one is
// scaled to the other's digits: equal then means it is a prefix of the other
__device__ __forceinline__ bool json_key_less(uint32_t a, uint32_t b)
{
    const uint32_t da = out_digits(a), db = out_digits(b);
    unsigned long long x = a, y = b;
    for (uint32_t k = da; k < db; k++) x *= 10ull;
    for (uint32_t k = db; k < da; k++) y *= 10ull;
    return x != y ? x < y : da < db;
}

// order[q * K + k] = the hit of query q whose key is k-th; by the wave: a lane ranks a hit against all the others
__device__ __forceinline__ void json_order(const JsonParams &p, uint64_t q, uint32_t cnt)
{
    const uint32_t *pid = p.top_pid + q * p.K;
    for (uint32_t r = lane_id(); r < cnt; r += 64u) {
        const uint32_t mine = pid[r];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < cnt; j++) {
            const uint32_t other = pid[j];
            rank += (other != mine ? json_key_less(other, mine) : j < r) ? 1u : 0u;
        }
        p.order[q * p.K + rank] = (uint16_t)r;
    }
}

// the object of query q with its cnt reported hits
template <class Sink> __device__ __forceinline__ void json_object(const JsonParams &p, Sink &o, uint64_t q, uint32_t cnt)
{
    const kaamer_query_meta m = p.q[q];
    const uint8_t *name = nullptr;
    uint32_t name_len = 0;
    if (m.src_seq < p.n_names) {
        const kaamer_text_span sp = p.spans[m.src_seq];
        if ((uint64_t)sp.name_off + sp.name_len <= p.names_len) { name = p.names + sp.name_off; name_len = sp.name_len; }
    }
    int32_t trim = p.trim ? p.trim[q] : 0;
    if (trim < 0) trim = 0;
    JL(o, "{\"Query\":{\"Sequence\":\"");
    if (m.aa_off + m.aa_len <= p.aa_len && m.aa_len > (uint32_t)trim) o.escaped(p.aa + m.aa_off + (uint32_t)trim, m.aa_len - (uint32_t)trim);
    JL(o, "\",\"Name\":\"");
    o.escaped(name, name_len);
    JL(o, "\",\"SizeInKmer\":");
    json_put_i32(o, p.size_out[q]);
    if (p.protein) JL(o, ",\"Type\":\"Protein Query\",\"Location\":{\"StartPosition\":");
    else JL(o, ",\"Type\":\"DNA Query\",\"Location\":{\"StartPosition\":");
    json_put_i32(o, p.start_pos[q]);
    JL(o, ",\"EndPosition\":");
    json_put_i32(o, m.end_position);
    if (p.protein) JL(o, ",\"PlusStrand\":false,\"StartsAlternative\":null},\"Contig\":\"");
    else if (m.plus_strand) JL(o, ",\"PlusStrand\":true,\"StartsAlternative\":[]},\"Contig\":\"");
    else JL(o, ",\"PlusStrand\":false,\"StartsAlternative\":[]},\"Contig\":\"");
    if (!p.protein && p.fasta) o.escaped(name, name_len);
    JL(o, "\"},\"SearchResults\":{\"Counter\":{},\"Hits\":[");
    const uint32_t *pid = p.top_pid + q * p.K, *km = p.top_km + q * p.K;
    uint32_t found = cnt;   // FetchHitsInformation returns at the first id without an entry (search.go:461-463)
    for (uint32_t r = 0; r < cnt; r++) {
        if (r) JL(o, ",{\"Key\":");
        else JL(o, "{\"Key\":");
        const uint32_t id = pid[r];
        if (found == cnt && out_entry(p, id) == OUT_NONE) found = r;
        o.put_u32(id);
        JL(o, ",\"Kmatch\":");
        o.put_u32(km[r]);
        JL(o, ",\"Alignment\":{\"Identity\":0,\"Similarity\":0,\"Length\":0,\"Mismatches\":0,\"GapOpenings\":0,\"Raw\":0,\"BitScore\":0,\"EValue\":0,\"AlnString\":\"\","
              "\"QueryStart\":0,\"QueryEnd\":0,\"SubjectStart\":0,\"SubjectEnd\":0}}");
    }
    JL(o, "],\"PositionHits\":{");
    const uint16_t *order = p.order + q * p.K;
    if (p.positions) {
        const int32_t n = p.pos_len[q];
        const uint32_t n_bits = n > 0 ? (uint32_t)n : 0u, words = (n_bits + 63u) >> 6;
        const uint32_t first = (uint32_t)trim < n_bits ? (uint32_t)trim : n_bits;   // dna.go:260-262
        bool any = false;
        for (uint32_t k = 0; k < cnt; k++) {
            const uint32_t r = Sink::ORDERED ? order[k] : k;
            if (r >= cnt) continue;
            if (any) JL(o, ",\"");
            else JL(o, "\"");
            any = true;
            o.put_u32(pid[r]);
            JL(o, "\":[");
            json_put_bits(o, p.pos_bits + p.pos_base[q] + (uint64_t)r * words, n_bits, first);
            JL(o, "]");
        }
    }
    JL(o, "}},\"HitEntries\":{");
    bool any = false;
    for (uint32_t k = 0; k < cnt; k++) {
        const uint32_t r = Sink::ORDERED ? order[k] : k;
        if (r >= found) continue;
        if (any) JL(o, ",\"");
        else JL(o, "\"");
        any = true;
        o.put_u32(pid[r]);
        JL(o, "\":");
        const uint32_t ent = out_entry(p, pid[r]);
        o.copy(p.sj_bytes + p.sj_off[ent], p.sj_len[ent]);
    }
    JL(o, "}}");
}

// the reported queries of the workgroup's tile, listed in list[] in query order (as their thread numbers); every thread
// gets its own query's hit count and its rank among the reported ones, *total how many there are
__device__ __forceinline__ uint32_t json_tile_list(const JsonParams &p, uint32_t nq, unsigned long long *sh, uint32_t *list, uint32_t *rank, uint32_t *total)
{
    const uint64_t q = (uint64_t)blockIdx.x * OUT_TILE + threadIdx.x;
    uint32_t cnt = 0;
    if (q < nq) {
        cnt = p.top_cnt[q];
        if (cnt > p.K) cnt = p.K;
    }
    unsigned long long n = 0;
    const unsigned long long incl = out_block_scan(cnt ? 1ull : 0ull, sh, &n);
    if (cnt) list[incl - 1ull] = threadIdx.x;
    *rank = (uint32_t)incl - (cnt ? 1u : 0u);
    *total = (uint32_t)n;
    __syncthreads();
    return cnt;
}

__global__ __launch_bounds__(OUT_TILE) void json_len_kernel(JsonParams p)
{
    __shared__ unsigned long long sh[OUT_TILE];
    __shared__ uint32_t list[OUT_TILE], lens[OUT_TILE];
    const uint32_t nq = out_nq(p);
    if ((uint64_t)blockIdx.x * OUT_TILE >= nq || !out_upstream(p)) return;
    uint32_t rank, total;
    (void)json_tile_list(p, nq, sh, list, &rank, &total);
    lens[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t i = threadIdx.x >> 6; i < total; i += JSON_WAVES) {
        const uint32_t t = list[i];
        const uint64_t q = (uint64_t)blockIdx.x * OUT_TILE + t;
        uint32_t cnt = p.top_cnt[q];
        if (cnt > p.K) cnt = p.K;
        JsonCount o;
        json_object(p, o, q, cnt);
        json_order(p, q, cnt);
        if (lane_id() == 0) {
            if (o.n > 0xFFFFFFF0ull) { atomicOr(&p.counts[OUT_C_STATUS], (unsigned long long)OUT_ST_OBJECT); o.n = 0; }
            lens[t] = (uint32_t)o.n;
        }
    }
    __syncthreads();
    const uint64_t q = (uint64_t)blockIdx.x * OUT_TILE + threadIdx.x;
    if (q < nq) p.obj_len[q] = lens[threadIdx.x];
    unsigned long long bytes = 0;
    (void)out_block_scan(lens[threadIdx.x], sh, &bytes);
    if (threadIdx.x == 0) { p.tile_bytes[blockIdx.x] = bytes; p.tile_units[blockIdx.x] = total; }
}

__global__ __launch_bounds__(OUT_TILE) void json_write_kernel(JsonParams p)
{
    __shared__ unsigned long long sh[OUT_TILE], start[OUT_TILE];
    __shared__ uint32_t list[OUT_TILE];
    __shared__ __attribute__((aligned(16))) char win[JSON_WAVES * JSON_WIN];
    const uint32_t nq = out_nq(p);
    if ((uint64_t)blockIdx.x * OUT_TILE >= nq) return;
    if (p.counts[OUT_C_STATUS]) return;   // (uniform: written by the scan kernel before this one started)
    (void)out_upstream(p);
    uint32_t rank, total;
    const uint32_t my_cnt = json_tile_list(p, nq, sh, list, &rank, &total);
    const uint64_t my_q = (uint64_t)blockIdx.x * OUT_TILE + threadIdx.x;
    const unsigned long long my_len = my_q < nq ? p.obj_len[my_q] : 0ull;
    unsigned long long tile_bytes = 0;
    const unsigned long long before = out_block_scan(my_len, sh, &tile_bytes) - my_len;
    // object number r of the batch starts behind the r objects and the r commas in front of it
    const unsigned long long first_obj = p.tile_units[blockIdx.x];
    if (my_cnt) {
        const unsigned long long at = p.tile_bytes[blockIdx.x] + before + first_obj + rank;
        start[rank] = at;
        p.unit_off[first_obj + rank] = at;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x >> 6; i < total; i += JSON_WAVES) {
        const uint32_t t = list[i];
        const uint64_t q = (uint64_t)blockIdx.x * OUT_TILE + t;
        uint32_t cnt = p.top_cnt[q];
        if (cnt > p.K) cnt = p.K;
        const unsigned long long at = start[i], first = at - (first_obj + i ? 1ull : 0ull);
        JsonWrite o = { win + (threadIdx.x >> 6) * JSON_WIN, p.out, first, first & ~15ull, first, at + p.obj_len[q] };
        if (first != at) JL(o, ",");
        json_object(p, o, q, cnt);
        if (lane_id() == 0 && o.pos != o.end) atomicOr(&p.counts[OUT_C_STATUS], (unsigned long long)OUT_ST_MISMATCH);
        o.flush(true);
    }
}
