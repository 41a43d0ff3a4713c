"""The makedb GBK reader on the device (makedb_gbk.hip.inc: kaamer_makedb_gbk_device, kaamer_image_build_gbk_device,
kaamer_index_build_gbk) against the host reader, kaamer_makedb_gbk, on the same bytes: ids, packed sequences and offsets,
stats(), feature_names, every record's EntryId, stored Sequence and cells by position, fetch_hits of every id and of one
absent id, and the bytes save() writes.  The texts are gbkcases.py's, whose expected records test_makedb_gbk_abi_host.py pins
on the host reader."""
import ctypes as C
import gzip
import random

import pytest

import gbkcases as G
from kaamer_amd import abi, api, workload
from test_gpu_makedb_tsv import _image_bytes, _same
from test_makedb_embl_abi_host import _records

pytestmark = pytest.mark.gpu

KS = (0, 1, 2, 4, 5, 6, 12, 17, 19, 20)
SP12 = G.SP12


@pytest.fixture(scope="module")
def geo(klib):
    g = api.text_parser_geometry()
    assert g["piece"] == 16 and g["wave_step"] == 1024 and g["tile"] == 16384 and g["lines"] == 1024
    return g


def _check(text, device, tmp_path):
    """device against host; -> the host's table"""
    text = bytes(text)
    want = api.Proteins.from_gbk(text)
    _same(api.Proteins.from_gbk(text, device=device), want, tmp_path)
    return want


def test_hand_text(klib, gpu_device, tmp_path):
    want = _check(G.GBK, gpu_device, tmp_path)
    assert want.feature_names == G.FEATURES
    assert _records(api.Proteins.from_gbk(G.GBK, device=gpu_device)) == G.GBK_RECORDS


@pytest.mark.parametrize("name", sorted(G.RULES))
def test_rules(klib, gpu_device, tmp_path, name):
    text, want = G.RULES[name]
    _check(text, gpu_device, tmp_path)
    if want is not None:
        assert _records(api.Proteins.from_gbk(text, device=gpu_device)) == want


@pytest.mark.parametrize("name", sorted(G.ENDS))
def test_text_ends(klib, gpu_device, tmp_path, name):
    text, n = G.ENDS[name]
    assert len(_check(text, gpu_device, tmp_path)) == n


def _filler(n, eol):
    """all-space lines of n bytes in all, line ends included, each of 12 bytes or more: where they stand (state 0 or 5) they
    contribute nothing, and those beyond what a lane reads go to the wave that looks for a token"""
    out, low = [], 12 + len(eol)
    assert n == 0 or n >= low
    while n:
        m = min(n, 61)
        if 0 < n - m < low:
            m -= low
        out.append(b" " * (m - len(eol)) + eol)
        n -= m
    return b"".join(out)


TARGETS = {"keyword": 1, "VERSION": 3, "ORIGIN": 7, "sequence": 8, "terminator": 9}


def _tiled(kind, step, eol):
    """ten entries; the line under test of entry j starts KS[j] bytes in front of the (j + 1)-th multiple of step"""
    text = b""
    for j, k in enumerate(KS):
        lines = [b"LOCUS       T%d" % j, b"DEFINITION  name %d [Org %d]. tail %d" % (j, j, j), b"COMMENT     c", b"VERSION     T%d.1  GI:%d" % (j, j), b"  ORGANISM  Org %d" % j,
                 SP12 + b"Tax %d." % j, b"COMMENT     d", b"ORIGIN      ", b"        1 mafsaedvlk eydrrrrmea " + b"acd"[:j % 4], b"//"]
        at = TARGETS[kind]
        head = b"".join(ln + eol for ln in lines[:at])
        pad = step * (j + 1) - k - len(text) - len(head)
        text += head + _filler(pad, eol) + b"".join(ln + eol for ln in lines[at:])
        assert text.rindex(lines[at] + eol) == step * (j + 1) - k
    return text


@pytest.mark.parametrize("kind", sorted(TARGETS))
def test_tiling(klib, gpu_device, geo, tmp_path, kind):
    for step in (40 * geo["piece"], geo["wave_step"], geo["tile"]):
        for eol in (b"\n", b"\r\n") if kind == "terminator" else (b"\n",):
            want = _check(_tiled(kind, step, eol), gpu_device, tmp_path)
            recs = _records(want)
            assert len(recs) == len(KS)
            assert [r[1] for r in recs] == [b"T%d.1" % j for j in range(10)] and [r[4] for r in recs] == [[b"name %d tail %d" % (j, j), b"Org %d" % j, b"Tax %d." % j] for j in range(10)]


def test_leading_spaces(klib, gpu_device, tmp_path):
    """a keyword behind a run of spaces that a lane reads to its end, that ends at the edge of what it reads, and that only the
    wave's 64-byte steps find; lines that are nothing but such a run"""
    text = b""
    for n in (15, 16, 17, 31, 32, 33, 63, 64, 65, 5000):
        text += G.entry(b"DEFINITION  name %d" % n, b" " * n + b"SOURCE x", SP12 + b"lost", b" " * n + b"ORGANISM  Org", SP12 + b"Tax", b" " * n + b"DEFINITION  more",
                        b" " * n, b" " * n + b"x", b" " * n + b"// y", SP12 + b"lost", b" " * n + b"VERSION V", b" " * n + b"ORIGIN", SP12 + b"acdefghikl", ver=None, origin=None, seq=())
    text += G.entry(b"DEFINITION  all spaces", b" " * 5000, SP12 + b"behind")
    want = _check(text, gpu_device, tmp_path)
    recs = _records(want)
    assert len(recs) == 11 and all(b"lost" not in r[4][0] and r[4][2] == b"Tax" for r in recs[:10])
    assert recs[-1][4][0] == b"all spaces " + b" " * 4988 + b" behind"
    assert [r[1] for r in recs[:10]] == [b"VERSION"] * 10 and all(r[2].endswith(b"ORIGINACDEFGHIKL") for r in recs[:10])


def _carry_text(at, tail):
    """a short entry, then one whose ORGANISM line is line `at` of the text (0-based), DEFINITION continuation lines in front of
    it and `tail` FullTaxonomy lines behind it, then a short entry"""
    short = G.entry(b"LOCUS       S")   # 5 lines
    n_def = at - 5 - 2
    lines = [b"LOCUS       C%d" % at, b"DEFINITION  name"] + [SP12 + b"w%d" % i for i in range(n_def)] + [b"  ORGANISM  Org %d" % at] + [SP12 + b"t%d;" % i for i in range(tail)]
    text = short + G.entry(*lines) + short
    assert text.split(b"\n")[at].startswith(b"  ORGANISM")
    return text, n_def


@pytest.mark.parametrize("at", [1023, 1024, 1600])
def test_state_carry_at_block_edges(klib, gpu_device, geo, tmp_path, at):
    """the keyword line is the last line of a block of lines, the first of the next, and behind a DEFINITION of more than 1024
    lines; behind it more than two whole blocks of continuation lines carry its state, a short entry stands in front"""
    assert geo["lines"] == 1024
    text, n_def = _carry_text(at, 2100)
    recs = _records(_check(text, gpu_device, tmp_path))
    assert len(recs) == 3 and recs[1][4][1] == b"Org %d" % at
    assert recs[1][4][0].split(b" ") == [b"name"] + [b"w%d" % i for i in range(n_def)] and recs[1][4][2].split(b" ") == [b"t%d;" % i for i in range(2100)]


def _long_entry(n_lines, j):
    """an entry of n_lines lines, the terminator not counted: keyword lines spread over continuation lines, each of which means
    what the keyword line in front of it makes of it"""
    real = [b"LOCUS       L%d" % j, b"DEFINITION  name %d" % j, b"  ORGANISM  Org %d" % j, b"VERSION     L%d.1" % j, b"COMMENT     c", b"DEFINITION  second [x", b"FEATURES    f",
            b"ORIGIN      ", b"        1 mafsaedvlk", b"DBLINK      d"]
    lines = [SP12 + b"f%d]. g" % i for i in range(n_lines)]
    for i, ln in enumerate(real):
        lines[(i * (n_lines - 1)) // (len(real) - 1)] = ln
    return b"".join(ln + b"\n" for ln in lines + [b"//"])


@pytest.mark.parametrize("n_lines", [1023, 1024, 1025, 2049])
def test_blocks_of_lines(klib, gpu_device, geo, tmp_path, n_lines):
    """entries of about a block of lines, alone and with a short entry in front: the terminator is the block's last line, the
    next block's first, and a whole block lies inside one entry"""
    assert geo["lines"] == 1024
    for lead in (b"", G.entry(b"LOCUS       LEAD"), b"//\n"):
        text = lead + _long_entry(n_lines, 1) + _long_entry(n_lines, 2) + G.entry(b"LOCUS       TAIL")
        want = _check(text, gpu_device, tmp_path)
        assert len(want) == (4 if lead.startswith(b"LOCUS") else 3)


def test_searches_at_wave_step_edges(klib, gpu_device, tmp_path):
    """" [", "]." and ", partial" at 63 / 64 / 65 bytes of the joined name, inside a line and formed by a join"""
    text, n = b"", 0
    for off in (61, 62, 63, 64, 65, 126, 127, 128, 129):
        a = b"a" * off
        text += (G.entry(b"DEFINITION  " + a + b" [b]. tail") + G.entry(b"DEFINITION  " + a, SP12 + b"[b]. tail") + G.entry(b"DEFINITION  x [" + a + b"]. tail") +
                 G.entry(b"DEFINITION  x [" + a + b"]", SP12 + b". tail") + G.entry(b"DEFINITION  x [y]." + a + b"]. t") + G.entry(b"DEFINITION  " + a + b", partial") +
                 G.entry(b"DEFINITION  " + a + b",", SP12 + b"partial") + G.entry(b"DEFINITION  " + a + b", par", SP12 + b"tial") + G.entry(b"DEFINITION  " + a + b", parti", b"            al"))
        n += 7
    want = _check(text, gpu_device, tmp_path)
    assert len(want) == n


def test_long_things(klib, gpu_device, tmp_path):
    """one sequence of more than 64 KiB over many lines and in one line, a name and a taxonomy of tens of KB"""
    rng = random.Random(5)
    res = bytes(rng.choice(b"acdefghiklmnpqrstvwyACDEFGHIKLMNPQRSTVWY") for _ in range(72000))
    lines = [b"%9d " % (c + 1) + b" ".join(res[a:a + 10] for a in range(c, c + 60, 10)) for c in range(0, len(res), 60)]
    want = _check(G.entry(b"LOCUS       LONG", seq=lines) + G.entry(b"LOCUS       NEXT"), gpu_device, tmp_path)
    assert [r[2] for r in _records(want)] == [res.upper(), G.SEQ20]
    one = b"        1 " + bytes(rng.choice(b"acdefghiklmnpqrstvwy    ") for _ in range(90000))
    want = _check(G.entry(b"LOCUS       LINE", seq=(one,)) + G.entry(b"LOCUS       NEXT"), gpu_device, tmp_path)
    assert [len(r[2]) for r in _records(want)] == [len(one[10:].replace(b" ", b"")), 20] and len(_records(want)[0][2]) > 65536
    name = G.entry(b"DEFINITION  " + b"word " * 9000 + b"[Org", SP12 + b"x" * 30000 + b"]. tail", b"  ORGANISM  Org", SP12 + b"Taxon; " * 10000, SP12 + b"More.")
    recs = _records(_check(name, gpu_device, tmp_path))
    assert recs[0][4][0] == b"word " * 9000 + b"tail" and len(recs[0][4][2]) == 70000 + 6


def test_empty_records(klib, gpu_device, tmp_path):
    text = G.entry(b"LOCUS       A") + b"//\n" * 3000 + G.entry(b"LOCUS       B") + b"//\r\n" * 5
    want = _check(text, gpu_device, tmp_path)
    assert want.ids.tolist() == [1, 3002]


@pytest.mark.parametrize("part", range(6))
def test_fuzz(klib, gpu_device, tmp_path, part):
    for text in G.fuzz_texts()[part::6]:   # (the same texts in every part; this part checks its sixth)
        _check(text, gpu_device, tmp_path)


def _db_text(n, seed):
    """n proteins of the project's generator as GenPept entries: some partial, some too short, some with a line the reference
    panics on"""
    rng = random.Random(seed)
    buf, offs = workload.make_db(n, seed=seed)
    out = []
    for i in range(n):
        s = bytes(buf[int(offs[i]):int(offs[i + 1])]).lower()
        if rng.random() < 0.02:
            s = s[:6]
        lines = [b"LOCUS       P%05d_%d %15d aa            linear   BCT 01-JAN-2000" % (i, seed, len(s)),
                 b"DEFINITION  protein %d of family %d%s [Organism %d" % (i, i // 10, b", partial" if rng.random() < 0.02 else b"", i % 17), SP12 + b"(strain %d)]." % i,
                 b"ACCESSION   P%05d" % i, b"VERSION     P%05d.%d  GI:%d" % (i, 1 + i % 3, 1000 + i), b"DBSOURCE    accession X%05d.1" % i, b"KEYWORDS    .",
                 b"SOURCE      Organism %d" % (i % 17), b"  ORGANISM  Organism %d" % (i % 17), SP12 + b"Bacteria; Phylum%d;" % (i % 5), SP12 + b"Class%d." % (i % 7)]
        if i % 3 == 0:
            lines += [b"REFERENCE   1  (residues 1 to %d)" % len(s), b"  AUTHORS   Author,A.", b"  TITLE     Direct Submission", b"COMMENT     free text of entry %d." % i]
        lines += [b"FEATURES             Location/Qualifiers", b"     source          1..%d" % len(s), b"                     /organism=\"Organism %d\"" % (i % 17)]
        if rng.random() < 0.02:
            lines.append(b"VERSION")
        lines.append(b"ORIGIN      ")
        lines += [b"%9d " % (c + 1) + b" ".join(s[a:a + 10] for a in range(c, min(c + 60, len(s)), 10)) for c in range(0, len(s), 60)]
        out.append(b"".join(ln + (b"\r\n" if i % 11 == 0 else b"\n") for ln in lines + [b"//"]))
    return out


def test_pieces(klib, gpu_device, tmp_path):
    """a text cut at text_cut_gbk of several prefixes, every piece read with the terminators in front of it, merged: the
    whole text's table, which is the host reader's; what lies behind the last terminator is never read"""
    entries = _db_text(400, seed=11)
    text = b"".join(entries) + b"LOCUS       TAIL\n" + G.VER + b"\n" + G.ORIGIN + b"\n" + G.S20 + b"\n"
    want = api.Proteins.from_gbk(text)
    assert 330 <= len(want) < 400
    _same(api.Proteins.from_gbk(text, device=gpu_device), want, tmp_path)
    first, body = len(entries[0]), len(b"".join(entries))
    cuts = sorted({0} | {api.text_cut_gbk(text[:n]) for n in (first - 1, first, first + 1, len(text) // 3, len(text) // 3 + 1, 2 * len(text) // 3, len(text))})
    assert cuts[:3] == [0, first - 1, first] and cuts[-1] == body and len(cuts) >= 6   # (first - 1: behind a last "//" without its '\n')
    tables = []
    for a, b in zip(cuts, cuts[1:]):
        tables.append(api.Proteins.from_gbk(text[a:b], device=gpu_device, nb_before=G.n_terminators(text[:a])))
    _same(api.Proteins.merge(tables), want, tmp_path)
    # the id wraps at 2^32
    nb = 2 ** 32 - 3
    got = api.Proteins.from_gbk(text, device=gpu_device, nb_before=nb)
    assert got.ids.tolist() == [(int(i) + nb) % 2 ** 32 for i in want.ids] and min(got.ids.tolist()) < 400
    assert [r[1:] for r in _records(got)] == [r[1:] for r in _records(want)]


def test_gzip(klib, gpu_device, tmp_path):
    z = gzip.compress(G.GBK)
    want = _check(z, gpu_device, tmp_path)
    assert _records(want) == G.GBK_RECORDS
    prot, im = api.Image.from_gbk_text(z, device=gpu_device)
    _same(prot, want, tmp_path)
    assert _image_bytes(im, tmp_path, "dev.kht") == _image_bytes(want.image(), tmp_path, "host.kht")


@pytest.fixture(scope="module")
def db_text():
    return b"".join(_db_text(2000, seed=7))


@pytest.mark.parametrize("shard,n_shards", [(0, 1), (1, 3)])
def test_image_from_text(klib, gpu_device, tmp_path, db_text, shard, n_shards):
    want = api.Proteins.from_gbk(db_text)
    assert 1700 <= len(want) < 2000
    prot, im = api.Image.from_gbk_text(db_text, shard=shard, n_shards=n_shards, device=gpu_device)
    _same(prot, want, tmp_path)
    assert _image_bytes(im, tmp_path, "dev.kht") == _image_bytes(want.image(shard=shard, n_shards=n_shards), tmp_path, "host.kht")


def test_image_from_text_edges(klib, gpu_device, tmp_path):
    """texts that leave the builder nothing, or next to nothing"""
    for text in (b"", b"//\n", G.entry(seq=(b"        1 mafsaed",)), G.entry(seq=(b"        1 mafsae",))):
        want = api.Proteins.from_gbk(text)
        prot, im = api.Image.from_gbk_text(text, device=gpu_device)
        _same(prot, want, tmp_path)
        assert _image_bytes(im, tmp_path, "dev.kht") == _image_bytes(want.image(), tmp_path, "host.kht")


def test_index_from_text(klib, gpu_device, tmp_path, db_text):
    """the index built from the text answers as the index opened from the host table's image does"""
    want = api.Proteins.from_gbk(db_text)
    prot, ix = api.Index.from_gbk_text(db_text, device=gpu_device)
    ref = api.Index.from_image(want.image(), gpu_device)
    try:
        _same(prot, want, tmp_path)
        assert ix.stats() == want.image().stats()
        seqs, offs = prot.packed
        ids = prot.ids.tolist()
        pick = [3, len(ids) - 5]
        queries = [bytes(seqs[int(offs[i]):int(offs[i + 1])]) for i in pick]
        kw = dict(min_k_ratio=0.0, min_k_match=1, max_results=10)
        res, res_ref = ix.search_top(queries, **kw), ref.search_top(queries, **kw)
        assert res.n_reported == 2 and res.rep_query.tolist() == [0, 1]
        for f in ("rep_query", "top_off", "top_pid", "top_kmatch"):
            assert getattr(res, f).tolist() == getattr(res_ref, f).tolist(), f
        for j, i in enumerate(pick):   # (a record finds itself with all of its windows)
            a, b = int(res.top_off[j]), int(res.top_off[j + 1])
            hits = dict(zip(res.top_pid[a:b].tolist(), res.top_kmatch[a:b].tolist()))
            assert hits.get(ids[i]) == len(queries[j]) - 6, (i, ids[i], hits)
    finally:
        ix.close()
        ref.close()


def test_errors_leave_no_table(klib, gpu_device):
    """a device that is not there, a gzip signature with nothing behind it: the code, and *out stays null"""
    L = abi.lib()
    h = C.c_void_p(1)
    assert L.kaamer_makedb_gbk_device(G.GBK, len(G.GBK), 0, 4096, C.byref(h)) == abi.E_ARG and not h.value
    assert b"no device 4096" in L.kaamer_last_error()
    for fn in (L.kaamer_image_build_gbk_device, L.kaamer_index_build_gbk):
        p, o = C.c_void_p(1), C.c_void_p(1)
        assert fn(G.GBK, len(G.GBK), 0, 1, 0.5, 4096, C.byref(p), C.byref(o)) == abi.E_ARG and not p.value and not o.value
    # damaged gzip input: whatever the host reader makes of it -- its error, or the text up to the damage -- the device calls do
    z = gzip.compress(G.GBK)
    refused = 0
    for bad in (b"\x1f\x8b\x08", b"\x1f\x8b\x08\xe0" + b"\xff" * 20, z[:len(z) // 2], z[:-9] + b"\0" * 9, z + b"LOCUS       x\n"):
        host = C.c_void_p(1)
        code = L.kaamer_makedb_gbk(bad, len(bad), C.byref(host))
        h = C.c_void_p(1)
        assert L.kaamer_makedb_gbk_device(bad, len(bad), 0, gpu_device, C.byref(h)) == code
        p, o = C.c_void_p(1), C.c_void_p(1)
        assert L.kaamer_image_build_gbk_device(bad, len(bad), 0, 1, 0.5, gpu_device, C.byref(p), C.byref(o)) == code
        if code:
            refused += 1
            assert not host.value and not h.value and not p.value and not o.value
        else:
            want, got, prot = api.Proteins(host.value), api.Proteins(h.value), api.Proteins(p.value)
            api.Image(o.value)
            assert _records(got) == _records(want) == _records(prot)
    assert 1 <= refused < 5
