"""The makedb TSV reader on the device (makedb_tsv.hip.inc: kaamer_makedb_tsv_device, kaamer_image_build_tsv_device,
kaamer_index_build_tsv) against the host reader, kaamer_makedb_tsv, on the same bytes: ids, packed sequences and offsets,
stats(), feature_names, every record's EntryId, Sequence and feature cells by position, fetch_hits of every id and of one
absent id, and the bytes save() writes.  Every text is read in both forms of the call -- the header as the text's first line,
and the header handed over with the rows as the text -- and where the line-by-line restatement of the reference
(oracle/makedb_ref.run_tsv) accepts the text (no row longer than the header) the device table is compared with it as well."""
import ctypes as C
import random

import numpy as np
import pytest

from kaamer_amd import abi, api, workload

pytestmark = pytest.mark.gpu

SEED = 20261021
HDR3 = b"EntryID\tName\tSequence"


@pytest.fixture(scope="module")
def geo(klib):
    g = api.text_parser_geometry()
    assert g["piece"] == 16 and g["wave_step"] == 64 * g["piece"] and g["tile"] % g["wave_step"] == 0 and g["lines"] == 1024
    return g


def _makedb_ref():
    from oracle import makedb_ref
    return makedb_ref


def _saved(p, tmp_path, name):
    f = tmp_path / name
    p.save(f)
    return f.read_bytes()


def _records(p):
    """(EntryId, Sequence, feature cells in column order) of every record, by position (feature names may repeat)"""
    ids = np.ascontiguousarray(p.ids, dtype=np.uint32)
    ent = (abi.ProteinEntry * max(1, len(ids)))()
    abi.check(abi.lib().kaamer_fetch_hits(p._h, ids.ctypes.data, len(ids), ent))
    out = []
    for e in ent[:len(ids)]:
        assert e.found
        fo = [e.feature_off[i] for i in range(e.n_features + 1)]
        out.append((C.string_at(e.entry_id, e.entry_id_len), C.string_at(e.sequence, e.sequence_len),
                    [C.string_at(e.features + fo[i], fo[i + 1] - fo[i]) if fo[i + 1] > fo[i] else b"" for i in range(e.n_features)]))
    return out


def _same(got, want, tmp_path):
    """every field of two tables; -> the number of records"""
    assert len(got) == len(want), (len(got), len(want))
    gi, wi = got.ids, want.ids
    assert gi.tolist() == wi.tolist()
    (gs, go), (ws, wo) = got.packed, want.packed
    assert go.tolist() == wo.tolist()
    if bytes(gs) != bytes(ws):
        at = next(i for i in range(len(ws)) if gs[i] != ws[i])
        raise AssertionError("packed sequences differ: first at %d of %d" % (at, len(ws)))
    assert got.stats() == want.stats()
    assert got.feature_names == want.feature_names
    assert _records(got) == _records(want)
    absent = max([int(x) for x in wi] + [0]) + 1
    ids = [int(x) for x in wi] + [absent]
    gh, wh = got.fetch_hits(ids), want.fetch_hits(ids)
    assert gh == wh
    assert gh[-1] is None
    assert _saved(got, tmp_path, "got.prot") == _saved(want, tmp_path, "want.prot")
    return len(want)


def _lines(text):
    """the lines of a text as the reader forms them"""
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines]


def _ref_accepts(text):
    lines = _lines(text)
    names = lines[0].split(b"\t")
    feats = [n for n in names if n.lower() not in (b"entryid", b"sequence")]
    return len(set(feats)) == len(feats) and all(ln.count(b"\t") < len(names) for ln in lines[1:])


def _check(text, device, tmp_path):
    """the text in both forms of the device call against the host reader; -> (accepted rows, rejected rows), or the host's
    error when it refuses the header (the device call must refuse it alike)"""
    text = bytes(text)
    try:
        want = api.Proteins.from_tsv(text)
    except abi.KaamerError as e:
        assert e.code == abi.E_FORMAT
        with pytest.raises(abi.KaamerError) as d:
            api.Proteins.from_tsv(text, device=device)
        assert d.value.code == abi.E_FORMAT and str(d.value) == str(e)
        return str(e)
    got = api.Proteins.from_tsv(text, device=device)
    n = _same(got, want, tmp_path)
    # the same rows under a header that is handed over: what is left of the header line's end is the text
    nl = text.find(b"\n")
    header, rows = (text, b"") if nl < 0 else (text[:nl], text[nl + 1:])
    _same(api.Proteins.from_tsv(rows, device=device, header=header[:-1] if header.endswith(b"\r") else header), want, tmp_path)
    if _ref_accepts(text):
        ref = _makedb_ref().run_tsv(text)
        names = want.feature_names
        assert [r[0] for r in ref] == got.ids.tolist()
        assert [(r[1], r[2], [r[3][k] for k in names]) for r in ref] == _records(got)
    return n, len(_lines(text)) - 1 - n


HAND = {   # text -> (accepted, rejected rows)
    "header only": (HDR3 + b"\n", 0, 0),
    "header without a line end": (HDR3, 0, 0),
    "one row": (HDR3 + b"\na\tone\tACDEFGH\n", 1, 0),
    "CRLF throughout": (HDR3 + b"\r\na\tone\tACDEFGH\r\nb\ttwo\tACDEFG\r\nc\t\tACDEFGHIK\r\n", 2, 1),
    "last row without a line end": (HDR3 + b"\na\tone\tACDEFGH\nb\ttwo\tKLMNPQRS", 2, 0),
    "last row without a line end, CR": (HDR3 + b"\na\tone\tACDEFGH\nb\ttwo\tKLMNPQR\r", 2, 0),
    "empty rows": (b"\n".join([HDR3, b"", b"a\tone\tACDEFGH", b"", b"", b"b\ttwo\tACDEFGH", b"\r", b""]) + b"\n", 2, 5),
    "a row of tabs only": (HDR3 + b"\n\t\t\na\tone\tACDEFGH\n\t\n\t\t\t\t\n", 1, 3),
    "Sequence of 6 and of 7 bytes": (HDR3 + b"\na\tx\tACDEFG\nb\ty\tACDEFGH\nc\tz\tACDEFG\r\n", 1, 2),
    "empty EntryId": (HDR3 + b"\n\tx\tACDEFGH\nb\ty\tACDEFGH\n", 1, 1),
    "lower case and bytes >= 0x80": (HDR3 + b"\na\tn\xc3\xa9\tacdefgh\n\x85b\t\xff\t\x85az\xff`{AZ\xe1\nc\tz\tAcDeFgHiK\n", 3, 0),
    "Sequence first": (b"Sequence\tEntryID\tName\nACDEFGH\ta\tone\nACDEFG\tb\ttwo\nACDEFGHIK\tc\n", 2, 1),
    "Sequence in the middle": (b"Name\tSequence\tOrg\tEntryID\none\tACDEFGH\to1\ta\ntwo\tACDEFGH\to2\n", 1, 1),
    "Sequence last": (b"EntryID\tName\tOrg\tSequence\na\tone\to1\tACDEFGH\nb\ttwo\to2\n", 1, 1),
    "only the two required columns": (b"sequence\tENTRYID\nACDEFGH\ta\nACDEFGHIK\tb\textra\n\tc\n", 2, 1),
    "fewer cells than the header": (b"EntryID\tSequence\tF1\tF2\tF3\na\tACDEFGH\nb\tACDEFGH\tx\nc\tACDEFGH\tx\ty\nd\tACDEFGH\tx\ty\tz\ne\n", 4, 1),
    "more cells than the header": (HDR3 + b"\na\tone\tACDEFGH\textra\tmore\nb\ttwo\tACDEFG\tACDEFGHIK\nc\tthree\tACDEFGH\t\n", 2, 1),
    "duplicated EntryID and Sequence": (b"EntryID\tSequence\tN\tEntryID\tSequence\na\tACDEFGH\tn1\tb\tKLMNPQRST\nc\tACDEFGHIK\tn2\nd\tACDEFGH\tn3\t\tKLMNPQR\n"
                                        b"e\tACDEFGH\tn4\tf\ng\tACDEFGH\tn5\th\tKLM\ni\tACDEFGH\tn6\tj\tKLMNPQR\tmore\n", 4, 2),
    "duplicate and empty feature names": (b"F\tEntryID\tF\t\tSequence\tF\n1\ta\t2\t3\tACDEFGH\t4\n1\tb\t\t3\tACDEFGH\n", 2, 0),
    "a CR inside a cell": (HDR3 + b"\na\rb\to\rne\tACD\rEFG\n\rc\t\r\tACDEFG\r\r\nd\tx\r\tACDEF\r\n", 2, 1),
    "spaces are bytes": (HDR3 + b"\n a \t one \t ACDEF \n \t \t       \n", 2, 0),
    "no EntryID column": (b"Name\tSequence\nx\tACDEFGH\n", "TSV file doesn't contain 'EntryID' header"),
    "no Sequence column": (b"EntryID\tName\na\tACDEFGH\n", "TSV file doesn't contain 'Sequence' header"),
    "empty text": (b"", "TSV file doesn't contain 'EntryID' header"),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(klib, gpu_device, tmp_path, name):
    text, *want = HAND[name]
    got = _check(text, gpu_device, tmp_path)
    if isinstance(want[0], str):
        assert isinstance(got, str) and want[0] in got
    else:
        assert got == tuple(want)


def test_hand_ids_and_cells(klib, gpu_device):
    """the rules, stated on the device table itself"""
    dev = gpu_device
    p = api.Proteins.from_tsv(b"EntryID\tSequence\tN\tEntryID\tSequence\na\tACDEFGH\tn1\tb\tKLMNPQRST\nx\tACD\nc\tACDEFGHIK\tn2\n", device=dev)
    assert p.ids.tolist() == [0, 1] and _records(p) == [(b"b", b"KLMNPQRST", [b"n1"]), (b"c", b"ACDEFGHIK", [b"n2"])]
    p = api.Proteins.from_tsv(b"a\tone\tacdefgh\n\nb\ttwo\tACDEFGH", device=dev, header=HDR3, id_base=7)
    assert p.ids.tolist() == [7, 8] and _records(p) == [(b"a", b"acdefgh", [b"one"]), (b"b", b"ACDEFGH", [b"two"])]
    assert api.Proteins.from_tsv(b"a\tone\tACDEFGH\n", device=dev, header=HDR3, id_base=2 ** 32 - 1).ids.tolist() == [2 ** 32 - 1]
    assert api.Proteins.from_tsv(b"a\tone\tACDEFGH\nb\ttwo\tACDEFGH\n", device=dev, header=HDR3, id_base=2 ** 32 - 1).ids.tolist() == [2 ** 32 - 1, 0]   # uint32
    assert len(api.Proteins.from_tsv(b"", device=dev, header=HDR3)) == 0
    assert api.Proteins.from_tsv(HDR3 + b"\na\tone\tACDEFGH\n", device=dev, header=HDR3).ids.tolist() == [0, 1]   # (the header line is a row then: "Sequence" has 8 bytes)
    assert _records(api.Proteins.from_tsv(HDR3 + b"\n", device=dev, header=HDR3)) == [(b"EntryID", b"Sequence", [b"Name"])]


def _filler(n):
    """exactly n >= 0 bytes of whole rows under HDR3: accepted rows of up to 61 bytes, empty rows where fewer than 12 are left"""
    out = []
    while n > 0:
        if n < 12:
            out.append(b"\n" * n)
            break
        k = n if n <= 72 else 61
        out.append(b"r\tf\t" + (b"ACgtTGca" * 9)[:k - 5] + b"\n")
        n -= k
    return b"".join(out)


def _boundaries(geo):
    """the last byte in front of a piece, a wave step and a tile, and the first two behind (pieces 2 and 3: a feature needs up to 19 bytes in front)"""
    return [(name, k * geo[name] + d) for name, ks in (("piece", (2, 3)), ("wave_step", (1, 2)), ("tile", (1, 2))) for k in ks for d in (-1, 0, 1)]


def _check_rows(rows, device, tmp_path, header=HDR3):
    """rows whose positions matter: read under a header that is handed over (the device sees exactly `rows`), against the host
    reader on header + rows; then through _check in both forms"""
    want = api.Proteins.from_tsv(header + b"\n" + rows)
    _same(api.Proteins.from_tsv(rows, device=device, header=header), want, tmp_path)
    return _check(header + b"\n" + rows, device, tmp_path)


# feature -> (rows, offset of the byte that goes to the boundary, the byte there)
FEATURES = {
    "tab behind the EntryId": (b"id1\tfeat\tACDEFGHIK\nx\ty\tACDEFG\n", 3, b"\t"),
    "tab in front of the Sequence": (b"id1\tfeat\tACDEFGHIK\nx\ty\tACDEFG\n", 8, b"\t"),
    "tab behind an empty cell": (b"id1\t\tACDEFGHIK\nx\ty\tACDEFG\n", 4, b"\t"),
    "line end": (b"id1\tfeat\tACDEFGHIK\nid2\tf\tKLMNPQR\nx\ty\tACDEFG\n", 18, b"\n"),
    "CR of a CR LF": (b"id1\tfeat\tACDEFGHIK\r\nid2\tf\tKLMNPQR\r\nx\ty\tACDEFG\r\n", 18, b"\r"),
    "LF of a CR LF": (b"id1\tfeat\tACDEFGHIK\r\nid2\tf\tKLMNPQR\r\nx\ty\tACDEFG\r\n", 19, b"\n"),
    "CR LF behind the 6th residue": (b"id\tf\tACDEFG\r\nid2\tf\tKLMNPQR\r\n", 11, b"\r"),
    "7th residue": (b"id\tf\tACDEFGH\nx\ty\tACDEFG\n", 11, b"H"),
    "first byte of a row": (b"x\ty\tACDEFG\nid\tf\tACDEFGH\n", 11, b"i"),
    "tab of an extra cell": (b"id\tf\tACDEFGH\tmore\nx\ty\tACDEFG\n", 12, b"\t"),
}


@pytest.mark.parametrize("name", sorted(FEATURES))
def test_tiling(klib, gpu_device, geo, tmp_path, name):
    feature, lead, byte = FEATURES[name]
    assert feature[lead:lead + 1] == byte
    for _, at in _boundaries(geo):
        rows = _filler(at - lead) + feature
        assert rows[at:at + 1] == byte
        acc, rej = _check_rows(rows, gpu_device, tmp_path)
        assert acc >= 1 and rej >= 1, at


def test_long_cells_and_rows(klib, gpu_device, geo, tmp_path):
    """a cell that spans three tiles, as a feature and as the Sequence; a row of thousands of cells"""
    big = 40000
    assert big > 2 * geo["tile"]
    cell = bytes(65 + (i * 7 + i // 251) % 26 for i in range(big))
    for pre in (b"", _filler(geo["tile"] - 100)):
        assert _check_rows(pre + b"a\t" + cell + b"\tACDEFGH\nb\tshort\tKLMNPQRS\n", gpu_device, tmp_path)[0] >= 2
        assert _check_rows(pre + b"a\tname\t" + cell + b"\nb\tshort\tKLMNPQRS\r\n\tx\t" + cell + b"\n", gpu_device, tmp_path)[0] >= 2
    many = 5000
    rows = b"\t" * (many - 1) + b"\n" + b"a\tone\tACDEFGH" + b"\t" * (many - 3) + b"\n" + b"b\ttwo\tACDEF" + b"\tGH" * (many - 3) + b"\n" + b"c\tthree\tKLMNPQR\n"
    assert rows.split(b"\n")[0].count(b"\t") + 1 == many
    assert _check_rows(rows, gpu_device, tmp_path) == (2, 2)
    # ... and a header of thousands of columns, the two required ones last, rows of every length
    header = b"\t".join(b"f%d" % i for i in range(many - 2)) + b"\tSequence\tEntryID"
    full = b"\t".join(b"v%d" % (i % 97) if i % 3 else b"" for i in range(many - 2))
    rows = full + b"\tACDEFGH\ta\n" + full + b"\tACDEFGH\n" + full + b"\tACDEFGHIK\tb\tmore\n" + b"\tACDEFGH\tc\n" + b"\t" * (many - 2) + b"KLMNPQR\td\n"
    assert _check_rows(rows, gpu_device, tmp_path, header=header) == (3, 2)


@pytest.mark.parametrize("n_lines", [1023, 1024, 1025, 2049])
def test_blocks_of_lines(klib, gpu_device, geo, tmp_path, n_lines):
    """the per-row pass works on blocks of geometry["lines"] lines and one scan joins them: 1, 2 and 3 blocks, accepted rows
    first and last in a block, a block without an accepted row"""
    L = geo["lines"]
    n_blocks = (n_lines + L - 1) // L
    assert n_blocks == {1023: 1, 1024: 1, 1025: 2, 2049: 3}[n_lines]
    edge = {i for b in range(n_blocks) for i in (b * L, b * L + L - 1) if i < n_lines} | {n_lines - 1}
    barren = 1 if n_blocks == 3 else None           # the block that holds no accepted row
    for dense in (False, True):
        oks = [(i in edge or (dense and i % 5 != 2)) and i // L != barren for i in range(n_lines)]
        lines = []
        for i, ok in enumerate(oks):
            lines.append(b"id%d\tname %d\t%s" % (i, i % 13, b"ACDEFGHIK"[:9 if ok else 6 - i % 3]) if i % 7 else (b"id%d\t\tACDEFGH" % i if ok else b""))
        for tail in (b"", b"\n"):   # (with the line end the kernels count one more, empty, line)
            acc, rej = _check_rows(b"\n".join(lines) + tail, gpu_device, tmp_path)
            want = sum(oks)
            assert (acc, rej) == (want, n_lines - want)
            assert acc >= 2 and rej >= 1


TOKENS = [b"\t"] * 7 + [b"\n"] * 3 + [b"\r", b"\r\n", b"EntryID", b"sequence", b"ACDEFGH", b"ACDEFGH", b"ACDEFGH", b"KLMNPQRST", b"A", b"c", b"x", b"id", b"\x85", b" "]
HEADERS = [HDR3, b"EntryID\tSequence", b"sequence\tentryid\tF", b"F\tF\tENTRYID\tSEQUENCE\tF", b"EntryID\tSequence\tEntryID\tSequence", b"EntryID\tN\tSequence\r",
           b"Sequence\tSequence\tEntryID", b"Name\tSequence", b"EntryID\t\t", b""]


def _token_text(rng):
    head = rng.choice(HEADERS) if rng.random() < 0.8 else b"".join(rng.choice(TOKENS) for _ in range(rng.randrange(0, 8)))
    return head + b"\n" + b"".join(rng.choice(TOKENS) for _ in range(rng.randrange(0, 400)))


FUZZ = 300


def test_token_fuzz_texts_are_not_trivial(klib):
    """on the host alone: at least a third of the fuzz texts yield accepted rows, and some are refused for their header"""
    rng = random.Random(SEED)
    n_acc = n_err = 0
    for _ in range(FUZZ):
        try:
            n_acc += 1 if len(api.Proteins.from_tsv(_token_text(rng))) else 0
        except abi.KaamerError:
            n_err += 1
    assert 3 * n_acc >= FUZZ and n_err >= 10, (n_acc, n_err)


@pytest.mark.parametrize("part", range(6))
def test_token_fuzz(klib, gpu_device, tmp_path, part):
    rng = random.Random(SEED)
    texts = [_token_text(rng) for _ in range(FUZZ)]   # (the same 300 texts in every part; this part checks its sixth)
    for text in texts[part::6]:
        _check(text, gpu_device, tmp_path)


def _db_rows(n, seed, extra=2):
    """n proteins of the project's generator as TSV rows under _db_header(extra): some too short, some without an EntryId, lower
    case here and there, some rows short of cells"""
    rng = random.Random(seed)
    buf, offs = workload.make_db(n, seed=seed)
    out = []
    for i in range(n):
        s = bytes(buf[int(offs[i]):int(offs[i + 1])])
        if i % 5 == 0:
            s = s.lower()
        if rng.random() < 0.05:
            s = s[:rng.randrange(0, 7)]
        eid = b"" if rng.random() < 0.03 else b"sp|P%05d|X%d" % (i, seed)
        cells = [eid, b"protein %d of family %d" % (i, i // 10), s] + [b"" if (i + k) % 4 == 0 else b"value %d.%d" % (k, i % (k + 3)) for k in range(extra)]
        out.append(b"\t".join(cells[:rng.randrange(3, len(cells) + 1)]) + (b"\r\n" if i % 11 == 0 else b"\n"))
    return out


def _db_header(extra=2):
    return b"\t".join([b"EntryID", b"ProteinName", b"Sequence"] + [b"Feature%d" % k for k in range(extra)])


def test_pieces(klib, gpu_device, geo, tmp_path):
    """a text cut at three line ends, every piece read on the device under the header and the rows accepted in front of it,
    merged: the one-call table, which is the host reader's"""
    rows = _db_rows(3000, seed=11)
    header = _db_header()
    text = header + b"\n" + b"".join(rows)
    want = api.Proteins.from_tsv(text)
    assert 2500 <= len(want) < 3000 and len(text) > 8 * geo["tile"]
    whole = api.Proteins.from_tsv(text, device=gpu_device)
    _same(whole, want, tmp_path)
    cuts = [0, 1, 1024, 2999, 3000]   # (in rows: a piece of one row, one of a block and a bit, the last of one row)
    tables, base = [], 0
    for a, b in zip(cuts, cuts[1:]):
        t = api.Proteins.from_tsv(b"".join(rows[a:b]), device=gpu_device, header=header, id_base=base)
        base += len(t)
        tables.append(t)
    assert all(len(t) for t in tables[:3])
    _same(api.Proteins.merge(tables), want, tmp_path)
    _same(api.Proteins.merge(tables), whole, tmp_path)


def _image_bytes(im, tmp_path, name):
    f = tmp_path / name
    im.save(f)
    return f.read_bytes()


@pytest.fixture(scope="module")
def db_text():
    return _db_header(3) + b"\n" + b"".join(_db_rows(300, seed=7, extra=3))


@pytest.mark.parametrize("shard,n_shards", [(0, 1), (1, 3)])
def test_image_from_text(klib, gpu_device, tmp_path, db_text, shard, n_shards):
    want = api.Proteins.from_tsv(db_text)
    assert 200 <= len(want) < 300
    prot, im = api.Image.from_tsv_text(db_text, shard=shard, n_shards=n_shards, device=gpu_device)
    _same(prot, want, tmp_path)
    assert _image_bytes(im, tmp_path, "dev.kht") == _image_bytes(want.image(shard=shard, n_shards=n_shards), tmp_path, "host.kht")


def test_image_from_text_edges(klib, gpu_device, tmp_path):
    """texts that leave the builder nothing, or next to nothing"""
    for text in (HDR3, HDR3 + b"\na\tx\tACDEFG\n", HDR3 + b"\na\tx\tacdefgh\n", b"Sequence\tEntryID\nACDEFGH\ta"):
        want = api.Proteins.from_tsv(text)
        prot, im = api.Image.from_tsv_text(text, device=gpu_device)
        _same(prot, want, tmp_path)
        assert _image_bytes(im, tmp_path, "dev.kht") == _image_bytes(want.image(), tmp_path, "host.kht")


def test_index_from_text(klib, gpu_device, tmp_path, db_text):
    """the index built from the text answers as the index opened from the host table's image does, and with the device
    table attached as the subject text a TSV response row carries the table's feature cells"""
    want = api.Proteins.from_tsv(db_text)
    prot, ix = api.Index.from_tsv_text(db_text, device=gpu_device)
    ref = api.Index.from_image(want.image(), gpu_device)
    try:
        _same(prot, want, tmp_path)
        assert ix.stats() == want.image().stats()
        seqs, offs = prot.packed
        ids = prot.ids.tolist()
        upper = [i for i in range(len(ids)) if bytes(seqs[int(offs[i]):int(offs[i + 1])]).isupper()]   # (the k-mer alphabet is upper case: rows kept in lower case are no queries)
        pick = upper[::len(upper) // 20][:20]
        assert len(pick) == 20
        queries = [bytes(seqs[int(offs[i]):int(offs[i + 1])]) for i in pick]
        kw = dict(min_k_ratio=0.0, min_k_match=1, max_results=10)
        res, res_ref = ix.search_top(queries, **kw), ref.search_top(queries, **kw)
        assert res.n_reported == 20 and res.rep_query.tolist() == list(range(20))
        for f in ("rep_query", "top_off", "top_pid", "top_kmatch"):
            assert getattr(res, f).tolist() == getattr(res_ref, f).tolist(), f
        for j, i in enumerate(pick):
            a, b = int(res.top_off[j]), int(res.top_off[j + 1])
            hits = dict(zip(res.top_pid[a:b].tolist(), res.top_kmatch[a:b].tolist()))
            assert hits.get(ids[i]) == len(queries[j]) - 6, (i, ids[i], hits)
        # the response writer on top of the new reader
        reads = workload.unpack(workload.make_reads(workload.make_db(300, seed=7), 40, seed=5))
        fastq = b"".join(b"@read/%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))
        ix.attach_subject_text(prot)
        ref.attach_subject_text(want)
        got = ix.search_text_top(fastq, seq_type=abi.READS, tsv=dict(annotations=True), **kw)
        assert got.n_reported >= 10 and got.tsv == ref.search_text_top(fastq, seq_type=abi.READS, tsv=dict(annotations=True), **kw).tsv
        row = got.tsv[int(got.tsv_line_off[0]):int(got.tsv_line_off[1])]
        hit = _records(prot)[ids.index(int(got.top_pid[0]))]
        assert len(hit[2]) == 4 and hit[2][0]
        assert row.split(b"\t")[1] == hit[0] and row.endswith(b"\t%d" % len(hit[1]) + b"".join(b"\t" + v for v in hit[2]) + b"\n")
    finally:
        ix.close()
        ref.close()


def test_errors_leave_no_table(klib, gpu_device):
    """a header the reader refuses and a text with more feature cells than it indexes: the code, and *out stays null"""
    L = abi.lib()
    for text, header, msg in ((b"Name\tSequence\nx\tACDEFGH\n", None, b"'EntryID'"), (b"x\tACDEFGH\n", b"EntryID\tName", b"'Sequence'"), (b"", None, b"'EntryID'")):
        h = C.c_void_p(1)
        assert L.kaamer_makedb_tsv_device(text, len(text), header, len(header or b""), 0, gpu_device, C.byref(h)) == abi.E_FORMAT and not h.value
        assert msg in L.kaamer_last_error()
        p, o = C.c_void_p(1), C.c_void_p(1)
        if header is None:
            assert L.kaamer_image_build_tsv_device(text, len(text), 0, 1, 0.5, gpu_device, C.byref(p), C.byref(o)) == abi.E_FORMAT and not p.value and not o.value
            p, o = C.c_void_p(1), C.c_void_p(1)
            assert L.kaamer_index_build_tsv(text, len(text), 0, 1, 0.5, gpu_device, C.byref(p), C.byref(o)) == abi.E_FORMAT and not p.value and not o.value
    # (2^19 + 1) accepted rows under 8192 feature columns: 2^32 + 8192 entries of feature_off -- refused once the rows are
    # counted, before the cells are laid out (the host reader would need 32 GiB for them)
    n_feat, n_rows = 8192, 2 ** 19 + 1
    header = b"EntryID\tSequence" + b"\tf" * n_feat
    rows = b"a\tACDEFGH\n" * n_rows
    h = C.c_void_p(1)
    assert L.kaamer_makedb_tsv_device(rows, len(rows), header, len(header), 0, gpu_device, C.byref(h)) == abi.E_CAPACITY and not h.value
    assert b"%d rows of %d features" % (n_rows, n_feat) in L.kaamer_last_error()
    text = header + b"\n" + rows
    for fn in (L.kaamer_image_build_tsv_device, L.kaamer_index_build_tsv):
        p, o = C.c_void_p(1), C.c_void_p(1)
        assert fn(text, len(text), 0, 1, 0.5, gpu_device, C.byref(p), C.byref(o)) == abi.E_CAPACITY and not p.value and not o.value
    # the same rows but one under eight feature columns are read: 2^19 records of 2^22 empty cells
    p = api.Proteins.from_tsv(rows[:-10], device=gpu_device, header=b"EntryID\tSequence" + b"\tf" * 8)
    assert len(p) == 2 ** 19 and p.stats()["NumberOfAA"] == 7 * 2 ** 19 and p.ids[-1] == 2 ** 19 - 1
