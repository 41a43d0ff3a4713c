"""kaamer-db -merge and the split makedb runs on the host: kaamer_image_merge against its specification
(kaamer_image_build_pairs over the inputs' enumerations, tests/mergeref.py) and against one build over all proteins,
kaamer_proteins_merge, and kaamer_makedb_text_range against the reference's scan loops (pkg/makedb/inputFASTA.go:64-125,
inputEMBL.go:66-119, inputGBK.go:94-118; pkg/mergedb/mergedb.go:42-135).  CPU only."""
import ctypes as C
import os

import numpy as np
import pytest

import mergecases as M
import mergeref
from kaamer_amd import abi, api


# ---- images ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_parts", [2, 3])
@pytest.mark.parametrize("shard,n_shards", [(0, 1), (1, 3)])
@pytest.mark.parametrize("load", [0.5, 0.9])
def test_merge_is_build_pairs_over_the_enumerations(klib, tmp_path, n_parts, shard, n_shards, load):
    parts = M.part_images(api, n_parts, shard, n_shards, load)
    merged = api.Image.merge(parts, load_factor=load)
    M.same_bytes(merged, M.merged_by_definition(api, parts, tmp_path, load), tmp_path)
    whole = api.Image.from_proteins(packed=M.db(), shard=shard, n_shards=n_shards, load_factor=load)
    sm, sw = merged.stats(), whole.stats()
    assert {c: sm[c] for c in M.COUNTERS} == {c: sw[c] for c in M.COUNTERS}
    assert merged.load_factor == whole.load_factor == load


def test_merged_sets_are_the_oracles(klib, oracle, tmp_path):
    """per key the union of the inputs' sets: what indexdb makes of the store mergedb leaves"""
    pr = oracle.Index.from_proteins(None, packed=M.db()).pairs()        # key << 32 | id, sorted, distinct
    keys, ids = (pr >> np.uint64(32)).astype(np.uint32), (pr & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    starts = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    ends = np.r_[starts[1:], len(keys)]
    for n_parts in (2, 3):
        merged = api.Image.merge(M.part_images(api, n_parts))
        assert merged.stats()["n_keys"] == len(starts) and merged.stats()["n_pairs"] == len(pr)
        for a, b in zip(starts.tolist(), ends.tolist()):
            assert merged.get(int(keys[a])).tolist() == ids[a:b].tolist(), hex(int(keys[a]))
    # A's locality survives: the lists of part 0 keep their relative order in the merged arena, and what part 1 adds follows
    parts = M.part_images(api, 2)
    merged = api.Image.merge(parts)
    ka, _ = mergeref.enumerate_image(parts[0], tmp_path)
    km, _ = mergeref.enumerate_image(merged, tmp_path)
    tm = mergeref.table_of(merged, tmp_path)
    ta = mergeref.table_of(parts[0], tmp_path)
    list_keys_a = [int(k) for k in dict.fromkeys(ka.tolist()) if not (ta.val(int(k)) & mergeref.INLINE)]
    offs = [tm.val(k) for k in list_keys_a]
    assert all(not (o & mergeref.INLINE) for o in offs) and offs == sorted(offs)
    only_b = [int(k) for k in dict.fromkeys(km.tolist()) if ta.val(int(k)) is None and not (tm.val(int(k)) & mergeref.INLINE)]
    assert only_b and min(tm.val(k) for k in only_b) > 1      # (lists of B's own keys exist and sit in the arena)


def test_merge_of_one_image_is_the_image(klib, tmp_path):
    rng = np.random.default_rng(3)
    keys = rng.integers(0, 5000, 20000).astype(np.uint32) * 7919
    ids = rng.integers(0, 40, 20000).astype(np.uint32)
    for img in (api.Image.from_proteins(packed=M.db()), api.Image.from_proteins(packed=M.db(), shard=2, n_shards=3, load_factor=0.9),
                api.Image.from_pairs(keys, ids), api.Image.from_pairs(keys, ids, load_factor=0.8)):
        M.same_bytes(api.Image.merge([img], load_factor=img.load_factor), img, tmp_path)
    # another load factor is a re-bucketing: same sets and lists, another table
    img = api.Image.from_pairs(keys, ids)
    re = api.Image.merge([img], load_factor=0.9)
    M.same_bytes(re, api.Image.from_pairs(*mergeref.enumerate_image(img, tmp_path), load_factor=0.9), tmp_path)
    assert re.stats()["n_buckets"] < img.stats()["n_buckets"] and re.stats()["arena_words"] == img.stats()["arena_words"]
    # a load factor outside (0.05, 0.95] becomes 0.5, as in the builders
    assert api.Image.merge([img], load_factor=7.0).load_factor == 0.5


def test_crafted_pairs(klib, tmp_path):
    for case in M.crafted(api):
        name, imgs, load, _, _ = case
        merged = api.Image.merge(imgs, load_factor=load)
        M.check_crafted(case, merged, tmp_path)
        M.same_bytes(merged, M.merged_by_definition(api, imgs, tmp_path, load), tmp_path)


def test_merge_errors(klib, tmp_path):
    k = np.array([1, 1, 2], np.uint32)
    i = np.array([1, 2, 3], np.uint32)
    a = api.Image.from_pairs(k, i)
    for other in (api.Image.from_pairs(k, i, shard=0, n_shards=2), ):
        with pytest.raises(abi.KaamerError) as e:
            api.Image.merge([a, other])
        assert e.value.code == abi.E_ARG
    with pytest.raises(abi.KaamerError) as e:
        api.Image.merge([api.Image.from_pairs(k, i, shard=0, n_shards=2), api.Image.from_pairs(k, i, shard=1, n_shards=2)])
    assert e.value.code == abi.E_ARG
    with pytest.raises(abi.KaamerError) as e:
        api.Image.merge([])
    assert e.value.code == abi.E_ARG
    h = C.c_void_p()
    arr = (C.c_void_p * 2)(a._h, None)
    assert abi.lib().kaamer_image_merge(arr, 2, 0.5, C.byref(h)) == abi.E_ARG and not h.value
    # A file whose slot value points beyond arena_words: kaamer_image_load refuses it already (KAAMER_E_FORMAT), so a
    # loaded image cannot carry such a reference into the merge ...
    raw = bytearray(M.image_bytes(a, tmp_path))
    w = np.frombuffer(raw, dtype=np.uint32)
    at = next(s for s in range(1024, 1024 + a.stats()["n_buckets"] * 16, 2) if w[s] != 0xFFFFFFFF and not (w[s + 1] & 0x80000000))
    w[at + 1] = a.stats()["arena_words"] // 4 + 3
    p = os.path.join(str(tmp_path), "bad.kgi")
    with open(p, "wb") as f:
        f.write(bytes(raw))
    with pytest.raises(abi.KaamerError) as e:
        api.Image.load(p)
    assert e.value.code == abi.E_FORMAT
    # ... and the merge's own check is reached with an image patched in memory: refused before anything is dereferenced
    for what in M.bad_reference_cases(a):
        with pytest.raises(abi.KaamerError) as e:
            api.Image.merge([a, a])
        assert e.value.code == abi.E_ARG, what
    assert api.Image.merge([a, a]).get(1).tolist() == [1, 2]


# ---- protein tables ---------------------------------------------------------------------------------------------------
def _fasta(recs):
    return b"".join(b">%s %s\n%s\n" % (e, n, s) for e, n, s in recs)


def test_proteins_merge(klib, tmp_path):
    a = api.Proteins.from_fasta(_fasta([(b"A1", b"first", b"MKTAYIAKQRQISTFVK"), (b"A2", b"second", b"ACDEFGHIKLMNPQRSTVWY"), (b"A3", b"third", b"YWVTSRQPNMLKIHGFEDCA")]))
    b = api.Proteins.from_fasta(_fasta([(b"B1", b"other first", b"MAFSAEDVLKEYDRRRRMEA"), (b"B2", b"other second", b"MKTAYIAKQR"), (b"B3", b"x", b"ACDEFGHIK")]))
    assert a.ids.tolist() == [2, 3, 3] and b.ids.tolist() == [2, 3, 3]
    m = api.Proteins.merge([a, b])
    assert m.ids.tolist() == [2, 3, 3, 2, 3, 3] and len(m) == 6
    # later wins on a duplicated id (store 2's Protein overwrites store 1's, mergedb.go:98)
    assert m.fetch_hits([2, 3, 9]) == b.fetch_hits([2, 3, 9])
    assert api.Proteins.merge([b, a]).fetch_hits([2, 3]) == a.fetch_hits([2, 3])
    # the counters are summed, duplicates included (mergedb.go:91-93)
    sa, sb, sm = a.stats(), b.stats(), m.stats()
    for c in ("NumberOfProteins", "NumberOfAA", "NumberOfKmers"):
        assert sm[c] == sa[c] + sb[c]
    assert sm["Features"] == sa["Features"]
    # fetch_hits over a union of distinct ids
    t = api.Proteins.from_tsv(b"EntryID\tSequence\tEC\nT0\tMKTAYIAKQR\t1.1\nT1\tACDEFGHIKLMN\t2.2\n")
    u = api.Proteins.from_tsv(b"EntryID\tSequence\tEC\nU0\tMAFSAEDVLK\t3.3\n")
    tu = api.Proteins.merge([t, u, t])
    assert tu.fetch_hits([1])[0]["EntryId"] == b"T1" and tu.fetch_hits([0])[0]["EntryId"] == b"T0" and tu.stats()["NumberOfProteins"] == 5
    assert api.Proteins.merge([u, t]).fetch_hits([0, 1]) == t.fetch_hits([0, 1])
    # the image of the merged table is the merge of the images' sets
    img = m.image()
    ia, ib = a.image(), b.image()
    mi = api.Image.merge([ia, ib])
    assert img.stats()["n_pairs"] == mi.stats()["n_pairs"] and img.stats()["n_keys"] == mi.stats()["n_keys"]
    # unequal feature names are refused (the reference keeps the first database's KStats.Features: documented divergence)
    with pytest.raises(abi.KaamerError) as e:
        api.Proteins.merge([a, t])
    assert e.value.code == abi.E_ARG
    with pytest.raises(abi.KaamerError) as e:
        api.Proteins.merge([])
    assert e.value.code == abi.E_ARG
    # save / load round trip, full_seq entries included
    embl = b"ID   X_1   Reviewed;  8 AA.\nSQ   SEQUENCE   8 AA;  1 MW;  0 CRC64;\n     MAFSAEDVLK EYD\n//\n"
    e1, e2 = api.Proteins.from_embl(embl), api.Proteins.from_embl(embl.replace(b"X_1", b"X_2"))
    em = api.Proteins.merge([e1, e2])
    for tab, ids in ((m, [2, 3]), (em, [1])):
        p = os.path.join(str(tmp_path), "t.kpt")
        tab.save(p)
        back = api.Proteins.load(p)
        assert back.ids.tolist() == tab.ids.tolist() and back.stats() == tab.stats() and back.fetch_hits(ids) == tab.fetch_hits(ids)
    got = em.fetch_hits([1])[0]
    assert got["EntryId"] == b"X_2" and got["Sequence"] == b"MAFSAEDVLKEYD" and got["Length"] == 8


# ---- -offset / -length ------------------------------------------------------------------------------------------------
_SEQS = [b"MKTAYIAKQRQISTFVK", b"ACDEFGHIKLMNPQRSTVWY", b"MKTAY", b"YWVTSRQPNMLKIHGFEDCA", b"MAFSAEDVLKEYDRRRRMEA", b"QISTFVKSHFSRQ", b"ACDEFGHIKL"]
FASTA = b"ACDEFGHIKLMN\n" + b"".join(b">F%d name %d%s\n%s\n%s\n" % (i, i, b", partial" if i == 3 else b"", s[:9], s[9:]) for i, s in enumerate(_SEQS))
EMBL = b"".join((b"ID   E%d_X   Reviewed;  %d AA.\nDE   RecName: Full=Name %d;\nSQ   SEQUENCE   %d AA;  1 MW;  0 CRC64;\n     %s\n//\n" % (i, len(s), i, len(s), s))
                + (b"//\n" if i == 1 else b"") for i, s in enumerate(_SEQS)) + b"ID   TAIL_X\n"
GBK = b"".join((b"LOCUS       G%d   %d aa\nDEFINITION  protein %d [Org].\nVERSION     G%d.1\nORIGIN      \n        1 %s\n//\n" % (i, len(s), i, i, s.lower()))
               + (b"//\n" if i == 4 else b"") for i, s in enumerate(_SEQS))
TSV = b"EntryID\tSequence\tEC\n" + b"".join(b"T%d\t%s\t%d.1\n" % (i, s, i) for i, s in enumerate(_SEQS))
RANGES = [(o, n) for o in (0, 1, 2, 6, 7, 8, 9, 12) for n in (0, 1, 2, 7, 8, None)] + [(3, 2 ** 64 - 1), (2 ** 64 - 1, 3), (1, 2 ** 63)]


def _records(p):
    buf, offs = p.packed
    return [(int(i), bytes(buf[int(offs[j]):int(offs[j + 1])])) for j, i in enumerate(p.ids)]


def _check_table(p, ref, flat):
    """`ref`: records as oracle.makedb_ref gives them (FASTA: id, entry id, sequence, features; flat files: id, entry id,
    indexed residues, stored sequence, features)"""
    assert _records(p) == [(r[0], r[2]) for r in ref]
    st = p.stats()
    assert (st["NumberOfProteins"], st["NumberOfAA"], st["NumberOfKmers"]) == (len(ref), sum(len(r[2]) for r in ref), sum(len(r[2]) - 6 for r in ref))
    last = {r[0]: r for r in ref}
    for e, i in zip(p.fetch_hits(sorted(last)), sorted(last)):
        r = last[i]
        assert e["EntryId"] == r[1] and e["Sequence"] == (r[3] if flat else r[2]) and e["Length"] == len(r[2])
        assert {k: v for k, v in e["Features"].items() if v != b""} == {k: v for k, v in r[-1].items() if v != b""}


@pytest.mark.parametrize("fmt,text,run,flat", [(abi.FASTA, FASTA, mergeref.run_fasta_range, False), (abi.EMBL, EMBL, mergeref.run_embl_range, True),
                                               (abi.GBK, GBK, mergeref.run_gbk_range, True)], ids=["fasta", "embl", "gbk"])
def test_ranges_follow_the_scan_loops(klib, fmt, text, run, flat):
    n_kept = 0
    for offset, length in RANGES:
        ref = run(text, offset, mergeref.MAX_INT if length is None else length)
        _check_table(api.Proteins.from_text(text, fmt, offset=offset, length=length), ref, flat)
        n_kept += len(ref)
    assert n_kept > 40
    # the range rule, as the header states it: a FASTA range holds records offset .. offset + length - 1 under ids k + 1,
    # a flat-file range records offset + 1 .. offset + length under ids k.  Of FASTA records 2..4 (F1, F2, F3) the second is
    # too short and the third partial; of EMBL records 3..5 one is empty and E2 too short; of GBK records 3..5 G2 is too short
    ids = api.Proteins.from_text(text, fmt, offset=2, length=3).ids.tolist()
    assert ids == {abi.FASTA: [3], abi.EMBL: [5], abi.GBK: [4, 5]}[fmt]
    # the defaults are kaamer_makedb_text: the unranged readers
    whole = {abi.FASTA: api.Proteins.from_fasta, abi.EMBL: api.Proteins.from_embl, abi.GBK: api.Proteins.from_gbk}[fmt](text)
    dflt = api.Proteins.from_text(text, fmt)
    assert _records(dflt) == _records(whole) and dflt.stats() == whole.stats()
    assert dflt.fetch_hits(whole.ids) == whole.fetch_hits(whole.ids)
    # consecutive ranges partition the file: their merge fetches every id as the unranged table does
    for step in (1, 2, 3, 5):
        tabs = [api.Proteins.from_text(text, fmt, offset=o, length=step) for o in range(0, 12, step)]
        merged = api.Proteins.merge(tabs)
        assert sorted(set(merged.ids.tolist())) == sorted(set(whole.ids.tolist())), step
        assert merged.fetch_hits(whole.ids) == whole.fetch_hits(whole.ids), step
        assert merged.image().stats() == whole.image().stats(), step


def test_fasta_range_end_queues_its_record_twice(klib):
    """inputFASTA.go:100-105 breaks without clearing the entry and :120-124 queues it again: one record twice, same id"""
    ref = mergeref.run_fasta_range(FASTA, 1, 2)
    assert [r[0] for r in ref] == [2, 3, 3]
    p = api.Proteins.from_text(FASTA, abi.FASTA, offset=1, length=2)
    assert _records(p) == [(2, _SEQS[0]), (3, _SEQS[1]), (3, _SEQS[1])]


def test_tsv_ignores_the_range_and_bad_formats_are_refused(klib):
    whole = api.Proteins.from_tsv(TSV)
    for offset, length in ((0, None), (3, 1), (100, 0)):
        p = api.Proteins.from_text(TSV, abi.TSV, offset=offset, length=length)
        assert _records(p) == _records(whole) and p.fetch_hits(whole.ids) == whole.fetch_hits(whole.ids)
    with pytest.raises(abi.KaamerError) as e:
        api.Proteins.from_text(TSV, 4)
    assert e.value.code == abi.E_ARG
