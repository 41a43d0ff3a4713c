"""Every stage of the G tier (kaamer_amd/csrc/count_global.hip.inc), pinned by input.

count_global_kernel counts a query in one of three places -- the whole query in its LDS table; the query's postings
partitioned into id-range buckets, sized by a guess or (a guessed bucket was full) by a counting sweep, each bucket in the
LDS table; a table in HBM -- and which one is decided by the data.  tests/gtierref.py restates the figures that decide it
from the oracle index; every test here asserts from them that its input enters the stage it is named for, and only then
compares hits, lowest positions and n_overflow with the oracle.  The first test (no GPU) proves the recipes."""
import numpy as np
import pytest

import gtierref
from kaamer_amd import abi

gpu = pytest.mark.gpu
_cases = {}


def _case(oracle, name):
    """-> dict(db, ids, q, oix, fig) of the input `name`, built once"""
    if name not in _cases:
        db, ids, q = getattr(gtierref, "input_" + name)()[:3]
        oix = oracle.Index.from_proteins(db, ids=ids)
        _cases[name] = dict(db=db, ids=ids, q=q, oix=oix, fig=None if name == "fresh" else gtierref.Figures(oracle, oix, q))
    return _cases[name]


def _assert_stage(name, f):
    """the regime of input `name`, from the restated figures"""
    print("%s: size %d, P %d, D %d, R %d, guess %d, items per range <= %d >= %d, distinct per range <= %d, long lists %d"
          % (name, f.size, f.P, f.D, f.R, f.guess, f.upper.max(), f.lower.max(), f.range_distinct.max(), f.n_long))
    if name == "lds":
        assert 4096 < f.D <= 5000 and f.lds_holds()
        assert gtierref.lds_longest_run(f.distinct) < gtierref.LDS_PROBES
    elif name == "guess_holds":
        assert f.D >= 8000 and f.size < gtierref.LDS_MAX_SIZE and not f.lds_holds()
        assert f.R > 2 and f.guess_holds() and f.buckets_fit()
    elif name == "guess_fails":
        assert f.D >= 8000 and f.size < gtierref.LDS_MAX_SIZE and not f.lds_holds()
        assert f.guess_fails() and f.lower.max() > 100000 and f.guess < 25000 and f.buckets_fit()
        at = int(f.lower.argmax())
        assert int((gtierref.range_of(f.distinct[np.isin(f.distinct, np.arange(8000, 20000))], f.R) == at).sum()) >= 30
        assert f.n_long > gtierref.LONG_SINK_CAP and f.sink_overflow() > 0 and f.window_beyond_registers()
    elif name == "bucket_overflows":
        assert f.size < gtierref.LDS_MAX_SIZE and not f.lds_holds()
        assert f.R == 3 and f.guess_holds() and f.bucket_overflows() and f.range_distinct.min() >= 8000
    elif name == "long_query":
        assert f.size >= gtierref.LDS_MAX_SIZE and f.D > gtierref.GRP_MAX_TABLE


STAGES = ["lds", "guess_holds", "guess_fails", "bucket_overflows", "long_query"]


def _fresh_orfs(oracle):
    c = _case(oracle, "fresh")
    dna, parent = gtierref.input_fresh()[2:]
    orfs = [o["seq"].encode("latin-1") for o in oracle.get_orfs(dna)]
    return c, dna, parent, [s for s in orfs if oracle.size_in_kmer(s) >= 7]


def test_recipes_reach_their_stage(oracle):
    """no GPU: every input's figures put it in its stage, and the databases stay under 10^6 residues"""
    for name in STAGES:
        c = _case(oracle, name)
        assert sum(len(s) for s in c["db"]) < 1000000, name
        _assert_stage(name, c["fig"])
    c, dna, parent, orfs = _fresh_orfs(oracle)
    big = [s for s in orfs if gtierref.pack_sends_unseen(oracle.size_in_kmer(s))]
    mine = [s for s in big if parent in s]          # (the other strand may hold a long ORF too: it hits nothing)
    assert len(dna) > 200 and len(mine) == 1 and 650 < oracle.size_in_kmer(mine[0]) < 750
    f = gtierref.Figures(oracle, c["oix"], mine[0])
    assert 200 <= f.D <= 300 and f.lds_holds()
    # the restated range hash and the occupancy walk, on values worked out by hand
    assert gtierref.range_of([0, 1, 3], 9).tolist() == [0, (0x85EBCA6B * 9) >> 32, ((3 * 0x85EBCA6B & 0xFFFFFFFF) * 9) >> 32]
    seen = {}
    for i in range(20000):
        h = ((i * 0x9E3779B1) & 0xFFFFFFFF) >> 19
        if h in seen:
            break
        seen[h] = i
    assert gtierref.lds_longest_run([seen[h], i]) == 2 and gtierref.lds_longest_run([5]) == 1


def _search(ix, seqs, **opts):
    from test_gpu_protein import _device_search
    return _device_search(ix, seqs, first_pos=1, **opts)


def _index(c, gpu_device):
    from kaamer_amd import api
    if "ix" not in c:
        c["ix"] = api.Index.from_image(api.Image.from_proteins(c["db"], ids=c["ids"]), gpu_device)
    return c["ix"]


def _expected(c, oracle):
    if "exp" not in c:
        pid, km, _ = c["oix"].search(c["q"])
        c["exp"] = dict(zip(pid.tolist(), km.tolist())), c["fig"].first_positions()
    return c["exp"]


@gpu
@pytest.mark.parametrize("name", STAGES)
def test_stage(klib, oracle, gpu_device, name):
    """(a) the LDS table, (b) the partition with guessed sizes, (c) with counted sizes -- and the sink, the waves' own
    expansion of the lists it has no room for, the loop for windows of more than 128 leftovers --, (d) a bucket that
    overflows and (e) a query of 65 535 k-mers or more, both in the HBM table"""
    c = _case(oracle, name)
    _assert_stage(name, c["fig"])
    hits, first, ctr = _search(_index(c, gpu_device), [c["q"]])
    exp, fp = _expected(c, oracle)
    assert len(exp) == c["fig"].D
    assert hits[0] == exp and first[0] == fp
    assert ctr["n_overflow"] >= 1 and ctr["n_hits"] == c["fig"].D and ctr["n_post"] == c["fig"].P
    assert ctr["n_lists"] == c["fig"].n_lists and ctr["n_list_ids"] == c["fig"].n_list_ids


@gpu
@pytest.mark.parametrize("name,slots", [("guess_fails", 4096), ("guess_fails", 100000), ("bucket_overflows", 32768)])
def test_arena_too_small(klib, oracle, gpu_device, name, slots):
    """(f) A G arena without room for the guessed buckets (4 096 slots), for the counted ones after the guessed ones
    (100 000: the guess takes R x guess / 2 = 89 000, the counted sizes 64 000 more), for the HBM table after the buckets
    (32 768: buckets 21 800, table 65 536): KAAMER_E_CAPACITY, never a partial list"""
    c = _case(oracle, name)
    f = c["fig"]
    _assert_stage(name, f)
    guessed = (f.R * f.guess + 1) // 2 + 1
    if name == "guess_fails":
        assert slots < guessed or guessed <= slots < guessed + (f.lower.sum() + 1) // 2 + 1
    else:
        assert guessed <= slots < guessed + 65536 and 2 * min(f.P, f.D) <= 65536
    with pytest.raises(abi.KaamerError) as e:
        _search(_index(c, gpu_device), [c["q"]], g_tier_slots=slots)
    assert e.value.code == abi.E_CAPACITY


@gpu
def test_fresh_item(klib, oracle, gpu_device):
    """(g) An ORF of 700 residues in a nucleotide sequence: its table does not fit a wave's arena, count_pack_kernel sends
    it on uncounted (wi.size < 0) and the G tier alone counts its postings, lists and list ids"""
    from test_gpu_reads import _check_reads
    c, dna, parent, orfs = _fresh_orfs(oracle)
    assert sum(gtierref.pack_sends_unseen(oracle.size_in_kmer(s)) and parent in s for s in orfs) == 1
    figs = [gtierref.Figures(oracle, c["oix"], s) for s in orfs]
    res = _index(c, gpu_device).search([dna], seq_type=abi.READS)
    assert _check_reads(res, [dna], oracle, c["oix"]) >= 1
    ctr = res.counters
    assert ctr["n_overflow"] >= 1
    assert ctr["n_post"] == sum(f.P for f in figs) > 100000
    assert ctr["n_lists"] == sum(f.n_lists for f in figs) and ctr["n_list_ids"] == sum(f.n_list_ids for f in figs)


@gpu
@pytest.mark.parametrize("name", ["guess_fails", "bucket_overflows"])
def test_positions(klib, oracle, gpu_device, name):
    """(h) PositionHits of (c) and (d): positions_global_kernel sweeps the query once more, into bitmaps"""
    c = _case(oracle, name)
    _assert_stage(name, c["fig"])
    res = _index(c, gpu_device).search([c["q"]], want_positions=True)
    pid, km, pos = c["oix"].search(c["q"], want_positions=True)
    exp, fp = _expected(c, oracle)
    assert res.hits(0) == exp and res.first_pos(0) == fp and res.counters["n_overflow"] >= 1
    got = res.positions(0)
    assert sorted(got) == sorted(pid.tolist())
    for j, p in enumerate(pid.tolist()):
        assert np.array_equal(got[p], pos[j]), p
