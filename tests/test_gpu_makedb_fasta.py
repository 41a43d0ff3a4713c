"""The makedb FASTA reader on the device (makedb_fasta.hip.inc: kaamer_makedb_fasta_device, kaamer_image_build_fasta_device,
kaamer_index_build_fasta) against the host reader, kaamer_makedb_fasta, on the same bytes: ids, packed sequences and offsets,
stats(), feature_names, fetch_hits of every id and of one absent id, and the bytes save() writes.  Where the line-by-line
restatement of the reference (oracle/makedb_ref.run_fasta) accepts the text (no empty lines), the device table is compared
with it as well."""
import random

import pytest

from kaamer_amd import api, workload

pytestmark = pytest.mark.gpu

SEED = 20261021
TOKENS = [bytes([c]) for c in b">>AAcg,  partial\t\r\n\n\n\x85\xff"] + [b", partial", b"\n>", b"ACDEFGH"]


@pytest.fixture(scope="module")
def geo(klib):
    g = api.text_parser_geometry()
    assert g["piece"] == 16 and g["wave_step"] == 64 * g["piece"] and g["tile"] % g["wave_step"] == 0 and g["lines"] >= 64
    return g


def _makedb_ref():
    from oracle import makedb_ref
    return makedb_ref


def _saved(p, tmp_path, name):
    f = tmp_path / name
    p.save(f)
    return f.read_bytes()


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
    assert got.feature_names == want.feature_names == [b"ProteinName"]
    absent = max([int(x) for x in wi] + [0]) + 1
    ids = [int(x) for x in wi] + [absent]
    gh, wh = got.fetch_hits(ids), want.fetch_hits(ids)
    assert gh == wh
    assert gh[-1] is None
    assert _saved(got, tmp_path, "got.prot") == _saved(want, tmp_path, "want.prot")
    return len(want)


def _n_entries(text):
    """entries of a text as the reader forms them: one per '>' line, and one for sequence lines in front of the first"""
    lines = [ln[:-1] if ln.endswith(b"\r") else ln for ln in text.split(b"\n")]
    lines = [ln for ln in lines if ln]
    n = sum(1 for ln in lines if ln[:1] == b">")
    return n + (1 if lines and lines[0][:1] != b">" else 0)


def _ref_accepts(text):
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return all(ln not in (b"", b"\r") for ln in lines)


def _check(text, device, tmp_path):
    text = bytes(text)
    want = api.Proteins.from_fasta(text)
    got = api.Proteins.from_fasta(text, device=device)
    n = _same(got, want, tmp_path)
    if _ref_accepts(text):
        ref = _makedb_ref().run_fasta(text)
        seqs, offs = got.packed
        assert [r[0] for r in ref] == got.ids.tolist()
        assert [r[2] for r in ref] == [bytes(seqs[int(offs[i]):int(offs[i + 1])]) for i in range(n)]
        last = {r[0]: r for r in ref}   # (a later record of an id wins)
        for pid, hit in zip(last, got.fetch_hits(list(last))):
            assert hit["EntryId"] == last[pid][1] and hit["Features"] == last[pid][3] and hit["Sequence"] == last[pid][2]
    return n, _n_entries(text) - n


HAND = {   # text -> (accepted, dropped)
    "empty text": (b"", 0, 0),
    "headers only": (b">a\n>b x\n>c\n", 0, 3),
    "S lines only": (b"ACDEFGH\nIKL\n", 1, 0),                     # id 0
    "S lines only, too short": (b"ACD\nEFG\n", 0, 1),
    "text before the first header": (b"ACDEFGHIK\nLM\n>a x\nACDEFGH\n>b\nACDEFGHI\n", 3, 0),
    "one header": (b">a one\nACDEFGHIK\n", 1, 0),
    "two headers": (b">a one\nACDEFGHIK\n>b two\nKLMNPQRST\n", 2, 0),   # both id 2
    "no final newline after an S line": (b">a\nACDEFGH\n>b\nACDEFG\nH", 2, 0),
    "no final newline after an H line": (b">a\nACDEFGH\n>b", 1, 1),
    "CRLF": (b">a x y\r\nACDEFGH\r\nIKL\r\n>b\r\nACDEFG\r\n>c z\r\nACDEFGH\r\n", 2, 1),
    "a line that is only CR": (b">a\n\r\nACDE\n\r\nFGH\n\r", 1, 0),
    "empty lines": (b"\n\n>a\n\nACDE\n\n\nFGH\n\n>b\n\n", 1, 1),
    "an interior CR": (b">a\nAC\rDEFG\n>b n\rm\nACDEFG\r\r\n", 2, 0),
    "whitespace-only lines as sequence": (b">a\n \n\t\t\n    \n>b\n  \t \n", 1, 1),
    "' >x' and 'A>C' as sequence": (b">a\n >x\nA>CD\n>b\nA>CDEF>\n", 2, 0),
    "lengths 6 and 7": (b">a\nACDEFG\n>b\nACDEFGH\n>c\nACDEFG\n", 1, 2),
    "7 across three lines": (b">a\nAC\nDEF\nGH\n>b\nAC\nDE\nFG\n", 1, 1),
    "lower case, the last entry too": (b">a\nacdefgh\n>b\nAcDeFgHiK\nlmn\n>c\nklmnpqrst\n", 3, 0),
    "bytes >= 0x80, ` and { next to a-z": (b">a\n\x85az\xff`{AZ\xe1\n>b\n`a{z|y}~@[\n", 2, 0),
    "empty EntryId": (b"> name of it\nACDEFGH\n", 1, 0),
    "a header without a space": (b">onlyid\nACDEFGH\n>\nACDEFGH\n", 2, 0),
    "two spaces": (b">id  two spaces\nACDEFGH\n>id2 \nACDEFGH\n", 2, 0),
    "partial at the start of the name": (b">a , partial cds\nACDEFGH\n>b x\nACDEFGH\n", 1, 1),
    "partial in the middle of the name": (b">a some protein, partial cds\nACDEFGH\n>b x\nACDEFGH\n", 1, 1),
    "partial at the end of the name": (b">a some protein, partial\nACDEFGH\n>b x\nACDEFGH\n", 1, 1),
    "partial at the end of the name, CRLF": (b">a some protein, partial\r\nACDEFGH\r\n>b x\r\nACDEFGH\r\n", 1, 1),
    "'>abc, partial' is kept": (b">abc, partial\nACDEFGH\n", 1, 0),
    "'>a , partial' is dropped": (b">a , partial\nACDEFGH\n>b\nACDEFGH\n", 1, 1),
    "'>a, partial, partial' is dropped": (b">a, partial, partial\nACDEFGH\n>b\nACDEFGH\n", 1, 1),
    "', partia' and a line end": (b">a x, partia\nl\nACDEFGH\n>b y, partia\r\nACDEFGH\n>c z, partia", 2, 1),
    "the pattern in a sequence line": (b">a x\nAC, partial\n>b\n, partial\n", 2, 0),
    "the pattern before any header": (b"x , partial\n>a\nACDEFGH\n", 2, 0),
    "Partial, partiaL and ',partial'": (b">a x, Partial\nACDEFGH\n>b x, partiaL\nACDEFGH\n>c x,partial\nACDEFGH\n", 3, 0),
    "commas at the text's end": (b">a x\nACDEFGH,,,\n>b ,,, parti", 1, 1),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(klib, gpu_device, tmp_path, name):
    text, acc, dropped = HAND[name]
    assert _check(text, gpu_device, tmp_path) == (acc, dropped)


def test_hand_ids(klib, gpu_device):
    """the id rule, stated: the last two entries share N; the entry without a header gets min(1, N); nb_before / more shift it"""
    dev = gpu_device
    assert api.Proteins.from_fasta(b"ACDEFGH\n", device=dev).ids.tolist() == [0]
    assert api.Proteins.from_fasta(b"ACDEFGH\n>a\nACDEFGH\n", device=dev).ids.tolist() == [1, 1]
    assert api.Proteins.from_fasta(b">a\nACDEFGH\n>b\nACDEFGH\n", device=dev).ids.tolist() == [2, 2]
    assert api.Proteins.from_fasta(b">a\nACDEFGH\n>b\nAC\n>c\nACDEFGH\n>d\nACDEFGH\n", device=dev).ids.tolist() == [2, 4, 4]
    assert api.Proteins.from_fasta(b">a\nACDEFGH\n>b\nACDEFGH\n", device=dev, nb_before=5, more=True).ids.tolist() == [7, 8]
    assert api.Proteins.from_fasta(b"ACDEFGH\n", device=dev, nb_before=5, more=True).ids.tolist() == [6]
    assert api.Proteins.from_fasta(b">a\nACDEFGH\n", device=dev, nb_before=2 ** 32 - 1).ids.tolist() == [0]   # uint32


def _filler(n):
    """exactly n >= 0 bytes of whole lines: sequence lines of up to 60 bytes (a lone '\\n' when one byte is left)"""
    out = []
    while n > 0:
        k = min(n, 61)
        out.append((b"ACgtTGca" * 8)[:k - 1] + b"\n")
        n -= k
    return b"".join(out)


def _boundaries(geo):
    return [(name, k * geo[name] + d) for name in ("piece", "wave_step", "tile") for k in (1, 2) for d in (-1, 0, 1)]


def _place(feature, lead, at):
    """a text whose byte `at` is byte `lead` of `feature`: an accepted entry of filler lines in front (without a header when
    there is no room for one)"""
    pre = at - lead
    assert pre >= 0
    text = (b">r\n" + _filler(pre - 3) if pre >= 3 else _filler(pre)) + feature
    assert text[at] == feature[lead]
    return text


PARTIAL = b", partial"
# feature -> (bytes, offset of the byte that goes to the boundary, the byte there)
FEATURES = {
    "line break": (b"ACGTacgt\nGGcc\n>s\nTTTTTT\n>u\nTTTTTTTT\n", 8, b"\n"),
    "first space, the pattern behind it": (b">id name, partial x\nACDEFGHIK\n>t\nACDEFGH\n", 3, b" "),
    "first space inside the pattern": (b">ab, partial rest\nACDEFGHIK\n>t\nAC\n", 4, b" "),
    "7th residue": (b">e\nACD\nEF\nGH\n>t\nACDEF\n", 11, b"H"),
    "line end behind the 6th residue": (b">e\nACD\nEF\nG\n>t\nACDEFGH\n", 11, b"\n"),
    "CR LF behind the 6th residue": (b">c d\nACDEFG\r\n>t\nACDEFGH\r\n", 11, b"\r"),
}
for _j in range(len(PARTIAL)):
    FEATURES["pattern byte %d" % _j] = (b">h nm" + PARTIAL + b"\nACDEFGHIK\n>t\nACDEFGH\n", 5 + _j, PARTIAL[_j:_j + 1])


@pytest.mark.parametrize("name", sorted(FEATURES))
def test_tiling(klib, gpu_device, geo, tmp_path, name):
    feature, lead, byte = FEATURES[name]
    assert feature[lead:lead + 1] == byte
    for _, at in _boundaries(geo):
        acc, dropped = _check(_place(feature, lead, at), gpu_device, tmp_path)
        assert acc >= 1 and dropped >= 1, at   # (the byte at the boundary decides one of them)


def test_blocks_of_lines(klib, gpu_device, geo, tmp_path):
    """the per-entry pass works on blocks of geometry["lines"] lines: an H line last in a block and its first S line first in
    the next, the last two entries on either side of a boundary, and entries whose S lines fill more than two blocks"""
    L = geo["lines"]
    for d in (-1, 0, 1):
        n_fill = L - 2 + d   # lines 1 .. n_fill are filler; the next H line is line n_fill + 1
        head = b">r x\n" + b"ACDEFGHIK\n" * n_fill
        # an H line and its first S line
        assert _check(head + b">h nm\nACD\nEFGH\n>t\nACDEFG\n", gpu_device, tmp_path) == (2, 1)
        assert _check(head + b">h nm, partial\nACD\nEFGH\n>t\nACDEFGH\n", gpu_device, tmp_path) == (2, 1)
        # the last two entries: the last S line of one, the H line of the other
        assert _check(head + b">last\nACDEFGH", gpu_device, tmp_path) == (2, 0)
        assert _check(head + b">last y, partial\nACDEFGH\n", gpu_device, tmp_path) == (1, 1)
        assert _check(b">r x\n" + b"A\n" * n_fill + b">last\nACDEFGH\n", gpu_device, tmp_path) == (2, 0)
    long_entry = b"AC\n" * (2 * L + 77)
    assert _check(b">a 1\nACDEFGH\n>b long\n" + long_entry + b">c\nACDEF\n", gpu_device, tmp_path) == (2, 1)
    assert _check(b">a 1\nACDEFGH\n>b long, partial\n" + long_entry + b">c\nACDEFGH\n", gpu_device, tmp_path) == (2, 1)
    assert _check(long_entry + b">c\nACDEFGH\n>d\n" + b"\n" * (L + 3) + b"ACDEFG\n", gpu_device, tmp_path) == (2, 1)
    assert _check(b">only\n" + b"\r\n" * (2 * L) + b"ACDE\n" + b"\n" * L + b"FGH", gpu_device, tmp_path) == (1, 0)


def _random_text(rng, geo):
    n = rng.choice([1, 2, 4]) * geo["tile"] - rng.randrange(0, 3 * geo["piece"])
    out = [b">ok one\nACDEFGHIK\n>no two, partial\nACDEFGHIK\n>sh\nACDEFG\n"]
    size = len(out[0])
    while size < n:
        t = rng.choice(TOKENS)
        out.append(t)
        size += len(t)
    return b"".join(out)[:n]


@pytest.mark.parametrize("case", range(10))
def test_random_texts(klib, gpu_device, geo, tmp_path, case):
    rng = random.Random(SEED + case)
    text = _random_text(rng, geo)
    want = api.Proteins.from_fasta(text)
    assert len(want) >= 1 and _n_entries(text) - len(want) >= 1   # (the comparison cannot pass on empty tables)
    acc, dropped = _check(text, gpu_device, tmp_path)
    assert acc >= 1 and dropped >= 1


def _db_text(n, seed, width=60):
    """n proteins of the project's generator as FASTA: '>id name words', some names with ', partial', lower case here and there"""
    rng = random.Random(seed)
    buf, offs = workload.make_db(n, seed=seed)
    out = []
    for i in range(n):
        s = bytes(buf[int(offs[i]):int(offs[i + 1])])
        if i % 5 == 0:
            s = s.lower()
        name = b"protein %d of family %d" % (i, i // 10) + (b", partial" if rng.random() < 0.1 else b"")
        out.append(b">sp|P%05d|X %s\n" % (i, name) + b"\n".join(s[j:j + width] for j in range(0, len(s), width)) + b"\n")
    return b"".join(out)


def test_pieces(klib, gpu_device, geo, tmp_path):
    """a text cut at kaamer_text_cut_fasta points, every piece read on the device with the '>' lines in front of it and
    more = 1 on all but the last, merged: the host reader's table of the whole text"""
    text = _db_text(40, seed=11, width=60) + b">short\nACD\n" + _db_text(110, seed=12, width=70) + b">tail one\nacdefghik\n>tail two\nKLMNPQRST"
    assert len(text) >= 3 * geo["tile"]
    cuts = []
    p = api.text_cut_fasta(text)
    while p:
        cuts.append(p)
        p = api.text_cut_fasta(text[:p])
    cuts = cuts[::-1]
    assert len(cuts) >= 8
    assert cuts[-1] == text.rindex(b">tail two")   # a cut inside the span of the last two entries
    keep = sorted(set(cuts[::7] + cuts[-2:]))      # every seventh cut and the last two: at least eight pieces
    assert len(keep) >= 8
    bounds = [0] + keep + [len(text)]
    tables = []
    for i in range(len(bounds) - 1):
        piece = text[bounds[i]:bounds[i + 1]]
        before = sum(1 for ln in text[:bounds[i]].split(b"\n") if ln[:1] == b">")
        tables.append(api.Proteins.from_fasta(piece, device=gpu_device, nb_before=before, more=i < len(bounds) - 2))
    want = api.Proteins.from_fasta(text)
    assert len(want) >= 100 and _n_entries(text) - len(want) >= 5
    _same(api.Proteins.merge(tables), want, tmp_path)


def _image_bytes(im, tmp_path, name):
    f = tmp_path / name
    im.save(f)
    return f.read_bytes()


@pytest.fixture(scope="module")
def db_text():
    return _db_text(300, seed=7)


@pytest.mark.parametrize("n_shards", [1, 2])
def test_image_from_text(klib, gpu_device, tmp_path, db_text, n_shards):
    want = api.Proteins.from_fasta(db_text)
    assert len(want) >= 200 and _n_entries(db_text) - len(want) >= 10
    for shard in range(n_shards):
        prot, im = api.Image.from_fasta_text(db_text, shard=shard, n_shards=n_shards, device=gpu_device)
        _same(prot, want, tmp_path)
        host = _image_bytes(want.image(shard=shard, n_shards=n_shards), tmp_path, "host.kht")
        assert _image_bytes(im, tmp_path, "dev.kht") == host
        # the route that was there before: the same proteins through the builder that takes host buffers
        assert _image_bytes(want.image(shard=shard, n_shards=n_shards, device=gpu_device), tmp_path, "dev2.kht") == host
        assert _image_bytes(api.Image.from_proteins(packed=want.packed, ids=want.ids, shard=shard, n_shards=n_shards, device=gpu_device),
                            tmp_path, "dev3.kht") == host


def test_image_from_text_edges(klib, gpu_device, tmp_path):
    """texts that leave the builder nothing, or next to nothing"""
    for text in (b"", b">a\nACDEFG\n", b">a x\nacdefgh\n", b"ACDEFGH\n"):
        want = api.Proteins.from_fasta(text)
        prot, im = api.Image.from_fasta_text(text, device=gpu_device)
        _same(prot, want, tmp_path)
        assert _image_bytes(im, tmp_path, "dev.kht") == _image_bytes(want.image(), tmp_path, "host.kht")


def test_index_from_text(klib, gpu_device, tmp_path, db_text):
    want = api.Proteins.from_fasta(db_text)
    prot, ix = api.Index.from_fasta_text(db_text, device=gpu_device)
    try:
        _same(prot, want, tmp_path)
        assert ix.stats() == want.image().stats()
        seqs, offs = prot.packed
        ids = prot.ids.tolist()
        pick = list(range(0, len(ids) - 2, max(1, (len(ids) - 2) // 20)))[:20]   # (the last two share an id)
        assert len(pick) == 20
        queries = [bytes(seqs[int(offs[i]):int(offs[i + 1])]) for i in pick]
        res = ix.search_top(queries, min_k_ratio=0.0, min_k_match=1, max_results=10)
        assert res.n_reported == 20
        assert res.rep_query.tolist() == list(range(20))
        for j, i in enumerate(pick):
            a, b = int(res.top_off[j]), int(res.top_off[j + 1])
            hits = dict(zip(res.top_pid[a:b].tolist(), res.top_kmatch[a:b].tolist()))
            assert hits.get(ids[i]) == len(queries[j]) - 6, (i, ids[i], hits)
    finally:
        ix.close()
