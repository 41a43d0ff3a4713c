"""The makedb EMBL reader on the device (makedb_embl.hip.inc: kaamer_makedb_embl_device, kaamer_image_build_embl_device,
kaamer_index_build_embl) against the host reader, kaamer_makedb_embl, on the same bytes: ids, packed sequences and offsets,
stats(), feature_names, every record's EntryId, stored Sequence and cells by position, fetch_hits of every id and of one
absent id, and the bytes save() writes (the whole strings of the records that hold more than they declare among them).  The
texts are emblcases.py's, whose expected records test_makedb_embl_abi_host.py pins on the host reader."""
import ctypes as C
import gzip
import random

import pytest

import emblcases as E
from kaamer_amd import abi, api, workload
from test_gpu_makedb_tsv import _image_bytes, _same
from test_makedb_embl_abi_host import _records

pytestmark = pytest.mark.gpu

KS = (0, 1, 2, 4, 5, 6, 12, 17, 19, 20)


@pytest.fixture(scope="module")
def geo(klib):
    g = api.text_parser_geometry()
    assert g["piece"] == 16 and g["wave_step"] == 1024 and g["tile"] == 16384 and g["lines"] == 1024
    return g


def _check(text, device, tmp_path):
    """device against host; -> the host's table"""
    text = bytes(text)
    want = api.Proteins.from_embl(text)
    _same(api.Proteins.from_embl(text, device=device), want, tmp_path)
    return want


def test_hand_text(klib, gpu_device, tmp_path):
    want = _check(E.EMBL, gpu_device, tmp_path)
    assert want.feature_names == E.FEATURES
    assert _records(api.Proteins.from_embl(E.EMBL, device=gpu_device)) == E.EMBL_RECORDS


@pytest.mark.parametrize("name", sorted(E.RULES))
def test_rules(klib, gpu_device, tmp_path, name):
    text, want = E.RULES[name]
    _check(text, gpu_device, tmp_path)
    if want is not None:
        assert _records(api.Proteins.from_embl(text, device=gpu_device)) == want


@pytest.mark.parametrize("name", sorted(E.ENDS))
def test_text_ends(klib, gpu_device, tmp_path, name):
    text, n = E.ENDS[name]
    assert len(_check(text, gpu_device, tmp_path)) == n


def _filler(n, eol):
    """CC lines of n bytes in all, line ends included"""
    out, low = [], 2 + len(eol)
    assert n == 0 or n >= low
    while n:
        m = min(n, 61)
        if 0 < n - m < low:
            m -= low
        out.append(b"CC" + b"x" * (m - low) + eol)
        n -= m
    return b"".join(out)


TARGETS = {"terminator": 6, "RecName": 1, "DR GO": 2, "SQ": 4, "sequence": 5}


def _tiled(kind, step, eol):
    """ten entries; the line under test of entry j starts KS[j] bytes in front of the (j + 1)-th multiple of step"""
    text = b""
    for j, k in enumerate(KS):
        lines = [b"ID   T%d_X Reviewed;" % j, b"DE   RecName: Full=Name %d; {ECO:%d}; tail %d; {ECO:0000255|HAMAP-Rule:MF_%05d};;" % (j, j, j, j),
                 b"DR   GO; GO:00%05d; F:molecular function %d;" % (j, j), b"OS   Organism %d." % j,
                 b"SQ   SEQUENCE   %d AA;  1 MW;  0 CRC64;" % (24 + j % 3), b"     MAFSAEDVLK EYDRRRRMEA MKTAYIA" + b"KQR"[:j % 4], b"//"]
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
            assert len(want) == len(KS) and sum(len(r[3]) > len(r[2]) for r in _records(want)) >= 3


def _long_entry(n_lines, j):
    """an entry of n_lines lines, the terminator not counted: its read lines spread over the CC lines"""
    real = [b"ID   L%d_X Reviewed;" % j, b"DE   SubName: Full=Sub %d;" % j, b"GN   Name=g%d;" % j, b"DR   KEGG; k:%d; -." % j, b"OC   Tax%d;" % j,
            b"SQ   SEQUENCE   20 AA;", b"     MAFSAEDVLK", b"DE   RecName: Full=Rec %d;" % j, b"      EYDRRRRMEA", b"OC   More."]
    lines = [b"CC   filler %d" % i for i in range(n_lines)]
    for i, ln in enumerate(real):
        lines[(i * (n_lines - 1)) // (len(real) - 1)] = ln
    return b"".join(ln + b"\n" for ln in lines + [b"//"])


@pytest.mark.parametrize("n_lines", [1023, 1024, 1025, 2049])
def test_blocks_of_lines(klib, gpu_device, geo, tmp_path, n_lines):
    """entries of about a block of lines, alone and with a short entry in front: the terminator is the block's last line, the
    next block's first, and a whole block lies inside one entry"""
    assert geo["lines"] == 1024
    for lead in (b"", E.entry(b"ID   LEAD x"), b"//\n"):
        text = lead + _long_entry(n_lines, 1) + _long_entry(n_lines, 2) + E.entry(b"ID   TAIL x")
        want = _check(text, gpu_device, tmp_path)
        assert len(want) == (4 if lead.startswith(b"ID") else 3)


def test_empty_records(klib, gpu_device, tmp_path):
    text = E.entry(b"ID   A x") + b"//\n" * 3000 + E.entry(b"ID   B x") + b"//\r\n" * 5
    want = _check(text, gpu_device, tmp_path)
    assert want.ids.tolist() == [1, 3002]


def test_long_things(klib, gpu_device, tmp_path):
    """more than 64 line records in one entry, cells of tens of KB, lines far longer than a wave step"""
    go = E.entry(b"ID   MANY_GO x", *[b"DR   GO; GO:%07d; F:x." % i for i in range(5000)], b"OS   Org.")
    want = _check(go + E.entry(b"ID   NEXT x", b"DR   GO; GO:1;"), gpu_device, tmp_path)
    assert len(_records(want)[0][4][3]) == 5000 * 11 - 1
    seq = E.entry(b"ID   MANY_SEQ x", sq=b"SQ   SEQUENCE   29000 AA;", seq=[b"     MAFSAEDVLK" if i % 2 else b"      EYDRRRRMEA " for i in range(3000)])
    want = _check(seq + E.entry(b"ID   NEXT x"), gpu_device, tmp_path)
    assert [len(r[2]) for r in _records(want)] == [29000, 20] and len(_records(want)[0][3]) == 30000
    oc = E.entry(b"ID   LONG_OC x", b"OC   " + b"Taxon; " * 10000, b"OC   More.")
    want = _check(oc, gpu_device, tmp_path)
    assert len(_records(want)[0][4][9]) == 70000 + 6
    rng = random.Random(5)
    line = b"     " + bytes(rng.choice(b"ACDEFGHIKLMNPQRSTVWY    ") for _ in range(40000))
    want = _check(E.entry(b"ID   LONG_SEQ x", sq=b"SQ   SEQUENCE   30000 AA;", seq=(line,)) + E.entry(b"ID   NEXT x"), gpu_device, tmp_path)
    assert [len(r[2]) for r in _records(want)] == [30000, 20] and len(_records(want)[0][3]) == len(line.replace(b" ", b""))
    rec = E.entry(b"ID   LONG_REC x", b"DE   RecName: Full=Front;; {" + b"ECO:1, }; {" * 7000 + b"};;", b"DE   SubName: Full=Sub {" + b"x" * 70000 + b"}; tail;")
    want = _check(rec, gpu_device, tmp_path)
    assert _records(want)[0][4][0] == b"Front;;Sub tail"


@pytest.mark.parametrize("part", range(6))
def test_fuzz(klib, gpu_device, tmp_path, part):
    for text in E.fuzz_texts()[part::6]:   # (the same 240 texts in every part; this part checks its sixth)
        _check(text, gpu_device, tmp_path)


def _db_text(n, seed):
    """n proteins of the project's generator as entries: some declare fewer residues than they hold, some too few or too many"""
    rng = random.Random(seed)
    buf, offs = workload.make_db(n, seed=seed)
    out = []
    for i in range(n):
        s = bytes(buf[int(offs[i]):int(offs[i + 1])])
        declared = len(s) - (rng.randrange(1, 9) if i % 7 == 0 and len(s) > 20 else 0)
        if rng.random() < 0.03:
            declared = rng.choice((3, len(s) + 1))
        lines = [b"ID   P%05d_X%d   Reviewed;  %d AA." % (i, seed, declared), b"AC   Q%05d;" % i, b"DE   RecName: Full=Protein %d of family %d {ECO:0000305};" % (i, i // 10)]
        if i % 3 == 0:
            lines.append(b"GN   Name=gene%d; ORFNames=o%d;" % (i, i))
        lines += [b"OS   Organism %d" % (i % 17), b"OS   (strain %d)." % i, b"OC   Bacteria; Phylum%d;" % (i % 5), b"OX   NCBI_TaxID=%d;" % (100000 + i),
                  b"CC   -!- FUNCTION: free text of entry %d." % i, b"DR   GO; GO:%07d; F:x." % i]
        if i % 4 == 0:
            lines.append(b"DR   KEGG; k:%d; -." % i)
        if rng.random() < 0.02:
            lines.append(b"DE   Flags: Fragment;")
        lines.append(b"SQ   SEQUENCE   %d AA;  1 MW;  0 CRC64;" % declared)
        lines += [b"     " + b" ".join(s[a:a + 10] for a in range(c, min(c + 60, len(s)), 10)) for c in range(0, len(s), 60)]
        out.append(b"".join(ln + (b"\r\n" if i % 11 == 0 else b"\n") for ln in lines + [b"//"]))
    return out


def test_pieces(klib, gpu_device, tmp_path):
    """a text cut at text_cut_embl of several prefixes, every piece read with the terminators in front of it, merged: the
    whole text's table, which is the host reader's; what lies behind the last terminator is never read"""
    entries = _db_text(400, seed=11)
    text = b"".join(entries) + b"ID   TAIL x\n" + E.SQ20 + b"\n" + E.S20 + b"\n"
    want = api.Proteins.from_embl(text)
    assert 330 <= len(want) < 400 and sum(len(r[3]) > len(r[2]) for r in _records(want)) >= 30
    _same(api.Proteins.from_embl(text, device=gpu_device), want, tmp_path)
    first, body = len(entries[0]), len(b"".join(entries))
    cuts = sorted({0} | {api.text_cut_embl(text[:n]) for n in (first - 1, first, first + 1, len(text) // 3, len(text) // 3 + 1, 2 * len(text) // 3, len(text))})
    assert cuts[:3] == [0, first - 1, first] and cuts[-1] == body and len(cuts) >= 6   # (first - 1: behind a last "//" without its '\n')
    tables = []
    for a, b in zip(cuts, cuts[1:]):
        tables.append(api.Proteins.from_embl(text[a:b], device=gpu_device, nb_before=E.n_terminators(text[:a])))
    _same(api.Proteins.merge(tables), want, tmp_path)
    # the id wraps at 2^32
    nb = 2 ** 32 - 3
    got = api.Proteins.from_embl(text, device=gpu_device, nb_before=nb)
    assert got.ids.tolist() == [(int(i) + nb) % 2 ** 32 for i in want.ids] and min(got.ids.tolist()) < 400
    assert [r[1:] for r in _records(got)] == [r[1:] for r in _records(want)]


def test_gzip(klib, gpu_device, tmp_path):
    z = gzip.compress(E.EMBL)
    want = _check(z, gpu_device, tmp_path)
    assert _records(want) == E.EMBL_RECORDS
    prot, im = api.Image.from_embl_text(z, device=gpu_device)
    _same(prot, want, tmp_path)
    assert _image_bytes(im, tmp_path, "dev.kht") == _image_bytes(want.image(), tmp_path, "host.kht")


@pytest.fixture(scope="module")
def db_text():
    return b"".join(_db_text(2000, seed=7))


@pytest.mark.parametrize("shard,n_shards", [(0, 1), (1, 3)])
def test_image_from_text(klib, gpu_device, tmp_path, db_text, shard, n_shards):
    want = api.Proteins.from_embl(db_text)
    assert 1700 <= len(want) < 2000 and sum(len(r[3]) > len(r[2]) for r in _records(want)) >= 100
    prot, im = api.Image.from_embl_text(db_text, shard=shard, n_shards=n_shards, device=gpu_device)
    _same(prot, want, tmp_path)
    assert _image_bytes(im, tmp_path, "dev.kht") == _image_bytes(want.image(shard=shard, n_shards=n_shards), tmp_path, "host.kht")


def test_image_from_text_edges(klib, gpu_device, tmp_path):
    """texts that leave the builder nothing, or next to nothing"""
    for text in (b"", b"//\n", E.entry(b"ID   A x", sq=b"SQ   SEQUENCE   7 AA;"), E.entry(b"ID   A x", seq=(b"     mafsaedvlk eydrrrrmea",))):
        want = api.Proteins.from_embl(text)
        prot, im = api.Image.from_embl_text(text, device=gpu_device)
        _same(prot, want, tmp_path)
        assert _image_bytes(im, tmp_path, "dev.kht") == _image_bytes(want.image(), tmp_path, "host.kht")


def test_index_from_text(klib, gpu_device, tmp_path, db_text):
    """the index built from the text answers as the index opened from the host table's image does"""
    want = api.Proteins.from_embl(db_text)
    prot, ix = api.Index.from_embl_text(db_text, device=gpu_device)
    ref = api.Index.from_image(want.image(), gpu_device)
    try:
        _same(prot, want, tmp_path)
        assert ix.stats() == want.image().stats()
        seqs, offs = prot.packed
        ids = prot.ids.tolist()
        pick = list(range(0, len(ids), len(ids) // 40))[:40]
        queries = [bytes(seqs[int(offs[i]):int(offs[i + 1])]) for i in pick]
        kw = dict(min_k_ratio=0.0, min_k_match=1, max_results=10)
        res, res_ref = ix.search_top(queries, **kw), ref.search_top(queries, **kw)
        assert res.n_reported == 40 and res.rep_query.tolist() == list(range(40))
        for f in ("rep_query", "top_off", "top_pid", "top_kmatch"):
            assert getattr(res, f).tolist() == getattr(res_ref, f).tolist(), f
        for j, i in enumerate(pick):   # (the builder saw the indexed prefix: a record finds itself with all of its windows)
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
    assert L.kaamer_makedb_embl_device(E.EMBL, len(E.EMBL), 0, 4096, C.byref(h)) == abi.E_ARG and not h.value
    assert b"no device 4096" in L.kaamer_last_error()
    for fn in (L.kaamer_image_build_embl_device, L.kaamer_index_build_embl):
        p, o = C.c_void_p(1), C.c_void_p(1)
        assert fn(E.EMBL, len(E.EMBL), 0, 1, 0.5, 4096, C.byref(p), C.byref(o)) == abi.E_ARG and not p.value and not o.value
    # damaged gzip input: whatever the host reader makes of it -- its error, or the text up to the damage -- the device calls do
    z = gzip.compress(E.EMBL)
    refused = 0
    for bad in (b"\x1f\x8b\x08", b"\x1f\x8b\x08\xe0" + b"\xff" * 20, z[:len(z) // 2], z[:-9] + b"\0" * 9, z + b"ID   x\n"):
        host = C.c_void_p(1)
        code = L.kaamer_makedb_embl(bad, len(bad), C.byref(host))
        h = C.c_void_p(1)
        assert L.kaamer_makedb_embl_device(bad, len(bad), 0, gpu_device, C.byref(h)) == code
        p, o = C.c_void_p(1), C.c_void_p(1)
        assert L.kaamer_image_build_embl_device(bad, len(bad), 0, 1, 0.5, gpu_device, C.byref(p), C.byref(o)) == code
        if code:
            refused += 1
            assert not host.value and not h.value and not p.value and not o.value
        else:
            want, got, prot = api.Proteins(host.value), api.Proteins(h.value), api.Proteins(p.value)
            api.Image(o.value)
            assert _records(got) == _records(want) == _records(prot)
    assert 1 <= refused < 5
