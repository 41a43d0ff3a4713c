"""The window steps of the LDS counting kernels (kaamer_amd/csrc/count_window.hip.inc: the window's query, the list head,
the flatten, the run add, the table add) at the numbers that decide them, in both kernels that inline them.

tests/windowcases.py builds one database with postings lists of chosen lengths and the batches: (a) lists of 1 to 9 ids --
inline, a list of one, the head's ids, the first arena load, the next 16-byte unit; (b) windows of 0 to 641 further ids,
on both sides of XIT * 64 = 128 and of every end of a round of GRP_LONG_UNROLL chunks; (c) owners whose first item is
item 127 or 128, and all further ids of a window in lane 0 or 63; (d) 63, 64, 65 ids in 64 slots, 65, 128, 129 in 128,
4096 and 4097 in 4096; (e) queries with more windows than carry a start hint; (f) runs of one id over a change of query,
and runs that cross the words of a bitmap; (g) the ORF forms.  tests/test_window_cases_host.py proves that every batch
meets its target.  Here every batch is compared with the oracle: hits, Kmatch, lowest positions, every PositionHits bit,
n_post, and n_overflow, n_lists, n_list_ids where the code makes them exact."""
import numpy as np
import pytest

import windowcases as wc
from kaamer_amd import abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def win(klib, oracle, gpu_device):
    from kaamer_amd import api
    d = wc.database(oracle)
    ix = api.Index.from_image(api.Image.from_proteins(d.db, ids=d.ids), gpu_device)
    rng = np.random.default_rng(818)
    # batches that hit nothing: the host-buffer call keeps its workspace, and with it the table scale the batch before left
    # on the device; a batch without hits leaves scale 1, the scale windowcases states the tables for
    quiet_aa = wc.hitless(d, rng, 40)
    for _ in range(200):
        quiet_nt = bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 150)])
        orfs = [o["seq"] for o in oracle.get_orfs(quiet_nt)]
        if any(oracle.size_in_kmer(o) >= 7 for o in orfs) and not any(d.counts(o.encode("latin-1")).any() for o in orfs):
            break
    yield d, ix, {False: quiet_aa, True: quiet_nt}
    ix.close()


_exp = {}


def _expected(d, case):
    """per query of a protein batch: ({id: Kmatch}, {id: lowest position}, {id: bits}); the batch's figures"""
    if id(case) not in _exp:
        per = []
        for q in case.seqs:
            pid, km, pos = d.oix.search(q, want_positions=True)
            per.append((dict(zip(pid.tolist(), km.tolist())), {int(p): int(np.argmax(pos[i])) for i, p in enumerate(pid)},
                        {int(p): pos[i] for i, p in enumerate(pid)}))
        figs = [d.figures(q) for q in case.seqs]
        _exp[id(case)] = per, sum(f.P for f in figs), sum(f.n_lists for f in figs), sum(f.n_list_ids for f in figs)
    return _exp[id(case)]


def _check_counters(case, c, n_post, n_lists, n_list_ids):
    assert c["n_post"] == n_post, case
    if case.overflow is not None:
        assert c["n_overflow"] == case.overflow, case
    if c["n_overflow"] == 0:     # (a query the G tier counts again is counted twice)
        assert (c["n_lists"], c["n_list_ids"]) == (n_lists, n_list_ids), case


def _quiet_then(ix, quiet, seqs, **kw):
    ix.search([quiet], **kw)
    return ix.search(seqs, **kw)


@pytest.mark.parametrize("first_pos", [1, -1])
@pytest.mark.parametrize("kind", ["a", "b", "c", "d", "e", "f"])
def test_protein_cases(win, oracle, kind, first_pos):
    """count_group_kernel, MODE 0, packed (first positions) and unpacked tables; a fresh workspace a batch: table scale 1"""
    from test_gpu_protein import _device_search
    d, ix, quiet = win
    for case in [c for c in wc.cases(oracle) if c.kind == kind]:
        per, n_post, n_lists, n_list_ids = _expected(d, case)
        hits, first, c = _device_search(ix, case.seqs, first_pos=first_pos)
        for i, (h, f, _) in enumerate(per):
            assert hits[i] == h, "%r query %d" % (case, i)
            if first_pos == 1:
                assert first[i] == f, "%r query %d" % (case, i)
        _check_counters(case, c, n_post, n_lists, n_list_ids)


@pytest.mark.parametrize("kind", ["a", "b", "c", "d", "e", "f"])
def test_position_hits(win, oracle, kind):
    """count_group_kernel, MODE 1: every bitmap bit for bit"""
    d, ix, quiet = win
    for case in [c for c in wc.cases(oracle) if c.kind == kind]:
        per, n_post, n_lists, n_list_ids = _expected(d, case)
        res = _quiet_then(ix, quiet[False], case.seqs, want_positions=True)
        for i, (h, f, bits) in enumerate(per):
            assert res.hits(i) == h and res.first_pos(i) == f, "%r query %d" % (case, i)
            got = res.positions(i)
            assert sorted(got) == sorted(bits), "%r query %d" % (case, i)
            for p in bits:
                assert np.array_equal(got[p], bits[p]), "%r query %d protein %d" % (case, i, p)
        _check_counters(case, res.counters, n_post, n_lists, n_list_ids)


@pytest.mark.parametrize("kind", ["a", "b", "c", "d"])
def test_orf_cases(win, oracle, kind):
    """count_pack_kernel, both arenas: the same amino-acid queries as reads, on both strands, and the contig"""
    from test_gpu_reads import _check_reads
    d, ix, quiet = win
    for case in [c for c in wc.orf_cases(oracle) if c.name.startswith(kind + ":")]:
        seq_type = abi.NUCLEOTIDE if "contig" in case.name else abi.READS
        res = _quiet_then(ix, quiet[True], case.seqs, seq_type=seq_type)
        assert _check_reads(res, case.seqs, oracle, d.oix) >= 1, case    # every ORF: hits, Kmatch, first positions
        figs = [d.figures(q) for q in wc.searched_queries(d, case.seqs, True) if oracle.size_in_kmer(q) >= 7]
        _check_counters(case, res.counters, sum(f.P for f in figs), sum(f.n_lists for f in figs), sum(f.n_list_ids for f in figs))
