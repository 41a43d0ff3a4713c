"""The JSON response of the reference (-fmt json), restated from its rules: json.Marshal(QueryResult) per reported query
(search.go:497-503) between SetResponseFormatAndHeader's opening bytes (search.go:672-688) and the closing bytes
(search.go:629-632), as encoding/json of the Go release go.mod names writes it.  Python's json module cannot produce these
bytes (HTML escaping, the replacement of invalid UTF-8, map keys sorted as strings), so nothing here is built on it.
Independent of the library: the tests hold kaamer_format_json, kaamer_json_escape and the device stage against this.

    entries    {protein id: dict(entry_id=bytes, sequence=bytes, length=int, features=[(name bytes, value bytes), ...])}
    a query    dict(name=bytes, sequence=bytes, size_in_kmer, start, end, plus=bool, trim=int,
                    hits=[dict(key=, kmatch=, bits=[bool, ...] as searched)] in reporting order)
Test infrastructure."""

BS = b"\x5c"   # the backslash
HEX = b"0123456789abcdef"


def _rune_size(s, i):
    """utf8.DecodeRune on s[i:], s[i] >= 0x80: the rune's size, 0 for the size-1 RuneError"""
    b0 = s[i]
    lo, hi = 0x80, 0xBF
    if 0xC2 <= b0 <= 0xDF:
        size = 2
    elif 0xE0 <= b0 <= 0xEF:
        size = 3
        if b0 == 0xE0:
            lo = 0xA0
        if b0 == 0xED:
            hi = 0x9F
    elif 0xF0 <= b0 <= 0xF4:
        size = 4
        if b0 == 0xF0:
            lo = 0x90
        if b0 == 0xF4:
            hi = 0x8F
    else:
        return 0
    if i + size > len(s) or not lo <= s[i + 1] <= hi:
        return 0
    for k in range(2, size):
        if not 0x80 <= s[i + k] <= 0xBF:
            return 0
    return size


def escape(s):
    """the bytes of a Go string between its quotes (encodeState.string, escapeHTML = true; no \\b / \\f forms)"""
    s = bytes(s)
    out = bytearray()
    i = 0
    while i < len(s):
        b = s[i]
        if b < 0x80:
            i += 1
            if b in (0x22, 0x5C):
                out += BS + bytes([b])
            elif b == 0x0A:
                out += BS + b"n"
            elif b == 0x0D:
                out += BS + b"r"
            elif b == 0x09:
                out += BS + b"t"
            elif b < 0x20 or b in (0x3C, 0x3E, 0x26):
                out += BS + b"u00" + HEX[b >> 4:(b >> 4) + 1] + HEX[b & 15:(b & 15) + 1]
            else:
                out.append(b)
            continue
        size = _rune_size(s, i)
        if size == 0:
            out += BS + b"ufffd"
            i += 1
        elif s[i:i + 3] == b"\xe2\x80\xa8":
            out += BS + b"u2028"
            i += 3
        elif s[i:i + 3] == b"\xe2\x80\xa9":
            out += BS + b"u2029"
            i += 3
        else:
            out += s[i:i + size]
            i += size
    return bytes(out)


def string(s):
    return b'"' + escape(s) + b'"'


def header(feature_names, annotations):
    """feature_names: KStats.Features, in its order; written unescaped, with Annotations only"""
    names = b",".join(b'"' + bytes(n) + b'"' for n in feature_names) if annotations else b""
    return b'{"dbProteinFeatures":[' + names + b'],"results":['


def trailer():
    return b"]}"


EMPTY_ALIGNMENT = (b'{"Identity":0,"Similarity":0,"Length":0,"Mismatches":0,"GapOpenings":0,"Raw":0,"BitScore":0,"EValue":0,'
                   b'"AlnString":"","QueryStart":0,"QueryEnd":0,"SubjectStart":0,"SubjectEnd":0}')


def protein(entry):
    """json.Marshal(kvstore.Protein): every field omitempty, the map's keys in byte order"""
    parts = []
    if entry["entry_id"]:
        parts.append(b'"EntryId":' + string(entry["entry_id"]))
    if entry["sequence"]:
        parts.append(b'"Sequence":' + string(entry["sequence"]))
    if entry["length"]:
        parts.append(b'"Length":%d' % entry["length"])
    if entry["features"]:
        members = [string(k) + b":" + string(v) for k, v in sorted(entry["features"], key=lambda kv: bytes(kv[0]))]
        parts.append(b'"Features":{' + b",".join(members) + b"}")
    return b"{" + b",".join(parts) + b"}"


def _by_string(ids):
    return sorted(ids, key=lambda i: b"%d" % i)


def one_object(q, entries, is_protein, text_format, positions):
    loc = b'{"StartPosition":%d,"EndPosition":%d,"PlusStrand":%s,"StartsAlternative":%s}' % (
        q["start"], q["end"], b"true" if (q["plus"] and not is_protein) else b"false", b"null" if is_protein else b"[]")
    contig = q["name"] if (not is_protein and text_format == 0) else b""
    query = b'{"Sequence":%s,"Name":%s,"SizeInKmer":%d,"Type":%s,"Location":%s,"Contig":%s}' % (
        string(q["sequence"]), string(q["name"]), q["size_in_kmer"], b'"Protein Query"' if is_protein else b'"DNA Query"', loc,
        string(contig))
    hits = b",".join(b'{"Key":%d,"Kmatch":%d,"Alignment":%s}' % (h["key"], h["kmatch"], EMPTY_ALIGNMENT) for h in q["hits"])
    pos = b""
    if positions or not is_protein:
        by_key = {h["key"]: h["bits"][q["trim"]:] for h in q["hits"]}
        pos = b",".join(b'"%d":[%s]' % (k, b",".join(b"true" if b else b"false" for b in by_key[k])) for k in _by_string(by_key))
    found = []
    for h in q["hits"]:
        if h["key"] not in entries:
            break
        found.append(h["key"])
    ents = b",".join(b'"%d":%s' % (k, protein(entries[k])) for k in _by_string(found))
    return (b'{"Query":' + query + b',"SearchResults":{"Counter":{},"Hits":[' + hits + b'],"PositionHits":{' + pos + b'}},"HitEntries":{' +
            ents + b"}}")


def objects(queries, entries, is_protein, text_format, positions):
    """the reported queries' objects joined by ',' -> (bytes, [the offset of every '{', the total])"""
    out = bytearray()
    off = []
    for q in queries:
        if not q["hits"]:
            continue
        if off:
            out += b","
        off.append(len(out))
        out += one_object(q, entries, is_protein, text_format, positions)
    off.append(len(out))
    return bytes(out), off
