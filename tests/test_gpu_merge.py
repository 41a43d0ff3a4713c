"""kaamer_image_merge_device (merge_device.hip.inc) against kaamer_image_merge (builder.cpp): the same image, byte for
byte -- header, buckets, arena -- on the cuts, shards, load factors and crafted inputs of tests/test_merge_host.py, on
lists at both sides of the length from which a whole wave copies a list, through the collision retry the merge shares
with the device builder, and in the searches a merged image answers like one build over all proteins."""
import os

import numpy as np
import pytest

import mergecases as M
from kaamer_amd import abi

pytestmark = pytest.mark.gpu

# md_units(c) = (1 + c + 3) / 4 16-byte units hold a list of c ids and its count; a list goes to the whole wave from
# MD_WAVE_UNITS = 64 units on (one 16-byte read by each of 64 lanes): the first such length is 4 * 64 - 4 = 252
WAVE_FROM = 252


@pytest.mark.parametrize("n_parts", [2, 3])
@pytest.mark.parametrize("shard,n_shards", [(0, 1), (1, 3)])
@pytest.mark.parametrize("load", [0.5, 0.9])
def test_cuts_shards_and_loads(klib, gpu_device, tmp_path, n_parts, shard, n_shards, load):
    from kaamer_amd import api
    parts = M.part_images(api, n_parts, shard, n_shards, load)
    host = api.Image.merge(parts, load_factor=load)
    M.same_bytes(api.Image.merge(parts, load_factor=load, device=gpu_device), host, tmp_path)


def test_crafted_pairs_and_errors(klib, gpu_device, tmp_path):
    from kaamer_amd import api
    for case in M.crafted(api):
        name, imgs, load, _, _ = case
        dev = api.Image.merge(imgs, load_factor=load, device=gpu_device)
        M.check_crafted(case, dev, tmp_path)
        M.same_bytes(dev, api.Image.merge(imgs, load_factor=load), tmp_path)
    k, i = np.array([1, 1, 2], np.uint32), np.array([1, 2, 3], np.uint32)
    a = api.Image.from_pairs(k, i)
    for bad in ([], [a, api.Image.from_pairs(k, i, shard=0, n_shards=2)]):
        with pytest.raises(abi.KaamerError) as e:
            api.Image.merge(bad, device=gpu_device)
        assert e.value.code == abi.E_ARG
    # a reference outside the arena is refused on the host, before anything is uploaded
    for what in M.bad_reference_cases(a):
        with pytest.raises(abi.KaamerError) as e:
            api.Image.merge([a, a], device=gpu_device)
        assert e.value.code == abi.E_ARG, what
    assert api.Image.merge([a, a], device=gpu_device).get(1).tolist() == [1, 2]


def _lists(lengths, first_key, first_id, step=1):
    keys, ids = [], []
    for n, c in enumerate(lengths):
        keys.append(np.full(c, first_key + 977 * n, np.uint32))
        ids.append((first_id + n + step * np.arange(c)).astype(np.uint32))
    return np.concatenate(keys), np.concatenate(ids)


def test_lists_at_both_sides_of_the_wave_copy(klib, gpu_device, tmp_path):
    """one input with lists of WAVE_FROM - 1, WAVE_FROM and WAVE_FROM + 1 ids (the lane that owns the slot copies the first,
    the whole wave the others), one of 5000 ids (20 rounds of the wave, the last one partial), lists of 1..9 ids (every
    padding of the last unit) and inline ids; alone (the identity) and merged with an input that lengthens some of them"""
    from kaamer_amd import api
    lengths = [WAVE_FROM - 1, WAVE_FROM, WAVE_FROM + 1, 5000, 255, 256, 257] + list(range(1, 10))
    ka, ia = _lists(lengths, 1000, 10, step=2)
    a = api.Image.from_pairs(ka, ia)
    assert a.stats()["max_list"] == 5000 and a.stats()["n_inline"] == 1
    for n, c in enumerate(lengths):
        assert len(a.get(1000 + 977 * n)) == c
    M.same_bytes(api.Image.merge([a], device=gpu_device), a, tmp_path)
    kb, ib = _lists([3, WAVE_FROM, 1, 700, 40], 1000, 11, step=2)          # odd ids: every pair is new
    b = api.Image.from_pairs(np.concatenate([kb, np.array([77, 78], np.uint32)]), np.concatenate([ib, np.array([5, 0x80000001], np.uint32)]))
    for imgs in ([a, b], [b, a], [a, b, a]):
        host = api.Image.merge(imgs)
        M.same_bytes(api.Image.merge(imgs, device=gpu_device), host, tmp_path)
    assert len(api.Image.merge([a, b], device=gpu_device).get(1000 + 977)) == 2 * WAVE_FROM


def test_collision_retry_is_the_builders(klib, gpu_device, tmp_path, capfd):
    """KAAMER_BUILD_WEAK_HASH, as tests/test_builder_device.py uses it: the first content hash is the set's size, unequal
    sets meet, the word-by-word check sees it and the pass the merge shares with the device builder runs again"""
    from kaamer_amd import api
    parts = M.part_images(api, 2)
    host = api.Image.merge(parts)
    os.environ["KAAMER_BUILD_WEAK_HASH"] = "1"
    os.environ["KAAMER_BUILD_TRACE"] = "1"
    try:
        dev = api.Image.merge(parts, device=gpu_device)
    finally:
        del os.environ["KAAMER_BUILD_WEAK_HASH"]
        del os.environ["KAAMER_BUILD_TRACE"]
    assert "content-hash attempts: 2" in capfd.readouterr().err
    M.same_bytes(dev, host, tmp_path)


def test_merge_of_one_device_built_image_is_the_image(klib, gpu_device, tmp_path):
    from kaamer_amd import api
    for kw in (dict(), dict(shard=1, n_shards=3, load_factor=0.9)):
        img = api.Image.from_proteins(packed=M.db(), device=gpu_device, **kw)
        M.same_bytes(api.Image.merge([img], load_factor=img.load_factor, device=gpu_device), img, tmp_path)
        M.same_bytes(api.Image.merge([img], load_factor=img.load_factor), img, tmp_path)


# ---- a merged image searches like one build over all proteins -------------------------------------------------------
def _protein_expectation(oracle, oix, seqs, max_results):
    exp = []
    for s in seqs:
        size = oracle.size_in_kmer(s)
        hits = {}
        if size >= 7:
            pid, km, _ = oix.search(s)
            keep = oracle.filter_results(km, size, max_results=max_results) if len(km) else 0
            hits = dict(zip(pid[:keep].tolist(), km[:keep].tolist()))
        exp.append(hits)
    return exp


def _reads_expectation(oracle, oix, reads, max_results):
    exp = []
    for r in reads:
        for o in oracle.get_orfs(r):
            pid, km, pos = oix.search(o["seq"], want_positions=True)
            keep = 0
            if len(km) and km[0] >= 10:
                _, _, so = oracle.set_best_start_codon(km, pos, oracle.size_in_kmer(o["seq"]), o["starts"], o["plus"], o["seq"], o["start"])
                keep = oracle.filter_results(km, so, max_results=max_results)
            exp.append(dict(zip(pid[:keep].tolist(), km[:keep].tolist())))
    return exp


def _hit_sets(top):
    pid, km = top.dense()
    return [dict(zip(pid[q, :int(top.top_cnt[q])].tolist(), km[q, :int(top.top_cnt[q])].tolist())) for q in range(top.n_queries)]


def _embl_of(packed):
    from kaamer_amd import workload
    return "".join("ID   P%05d_X   Reviewed;  %d AA.\nDE   RecName: Full=Name %d;\nSQ   SEQUENCE   %d AA;  1 MW;  0 CRC64;\n     %s\n//\n"
                   % (i, len(s), i, len(s), s.decode()) for i, s in enumerate(workload.unpack(packed))).encode()


def test_searches_as_a_full_build(klib, oracle, gpu_device):
    from kaamer_amd import api, workload
    db = M.db()
    merged = api.Image.merge(M.part_images(api, 3), device=gpu_device)
    ix_m, ix_w = api.Index.from_image(merged, gpu_device), api.Index.from_proteins(packed=db, device=gpu_device)
    oix = oracle.Index.from_proteins(None, packed=db)
    q = workload.make_protein_queries(db, 100, seed=62)
    reads = workload.make_reads(db, 200, seed=63)
    got_m, got_w = _hit_sets(ix_m.search_top(packed=q)), _hit_sets(ix_w.search_top(packed=q))
    exp = _protein_expectation(oracle, oix, workload.unpack(q), 10)
    assert got_m == got_w == exp and sum(len(h) for h in exp) > 100
    got_m = _hit_sets(ix_m.search_top(packed=reads, seq_type=abi.READS))
    got_w = _hit_sets(ix_w.search_top(packed=reads, seq_type=abi.READS))
    exp = _reads_expectation(oracle, oix, workload.unpack(reads), 10)
    assert got_m == got_w == exp and sum(len(h) for h in exp) > 100


def test_alignments_with_the_merged_protein_table(klib, gpu_device):
    """Proteins.merge of the range tables of one EMBL file next to Image.merge of their images: the alignments of the
    reported hits are those of the one table and the one build, field for field (NumberOfAA, which the e-values read, is
    the sum of the ranges')"""
    from kaamer_amd import api, workload
    db = M.db()
    text = _embl_of(db)
    whole = api.Proteins.from_embl(text)
    tabs = [api.Proteins.from_text(text, abi.EMBL, offset=o, length=100) for o in (0, 100, 200, 300)]
    prot = api.Proteins.merge(tabs)
    assert prot.ids.tolist() == whole.ids.tolist() and prot.stats() == whole.stats() and len(tabs[3]) == 0
    merged = api.Image.merge([t.image() for t in tabs], device=gpu_device)
    assert {c: merged.stats()[c] for c in M.COUNTERS} == {c: whole.image().stats()[c] for c in M.COUNTERS}
    ix_m, ix_w = api.Index.from_image(merged, gpu_device), api.Index.from_image(whole.image(), gpu_device)
    ix_m.attach_proteins(prot)
    ix_w.attach_proteins(whole)
    aln = dict(sub_matrix="blosum62", gap_open=11, gap_extend=1, text=True)
    q = workload.make_protein_queries(db, 40, seed=64)
    tm, tw = ix_m.search_top(packed=q, max_results=5, align=aln), ix_w.search_top(packed=q, max_results=5, align=aln)
    assert tm.top_off.tolist() == tw.top_off.tolist() and len(tm.alignments) > 40
    assert tm.top_pid.tolist() == tw.top_pid.tolist() and tm.top_kmatch.tolist() == tw.top_kmatch.tolist()
    assert tm.alignments == tw.alignments


def test_sharded_index_over_merged_shards(klib, gpu_device):
    from kaamer_amd import api, workload
    db = M.db()
    shards = [api.Image.merge(M.part_images(api, 2, shard=s, n_shards=3), device=gpu_device) for s in range(3)]
    for s, img in enumerate(shards):
        st, sw = img.stats(), api.Image.from_proteins(packed=db, shard=s, n_shards=3).stats()
        assert {c: st[c] for c in M.COUNTERS} == {c: sw[c] for c in M.COUNTERS}
    sx = api.ShardedIndex.from_images(shards, [gpu_device] * 3)
    ix = api.Index.from_proteins(packed=db, device=gpu_device)
    q = workload.make_protein_queries(db, 100, seed=65)
    assert _hit_sets(sx.search_top(packed=q)) == _hit_sets(ix.search_top(packed=q))
