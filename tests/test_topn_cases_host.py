"""The crafted world of tests/topncases.py on the CPU: every case's contract holds on the oracle's literal flow (get_orfs,
Index.search with positions, set_best_start_codon, filter_results), and the library's host post-steps (kaamer_sort_hits,
kaamer_set_best_start_codon, kaamer_filter_results) agree with it on every ORF and query of the world.  No device calls."""
import ctypes as C

import numpy as np
import pytest

import topncases as T


@pytest.fixture(scope="module")
def ref(oracle):
    seqs, ids = T.world().database()
    oix = oracle.Index.from_proteins(seqs, ids=ids)
    return oix, T.reference_orfs(oracle, oix, T.reads())


def test_the_builder_refuses_the_reserved_id():
    w = T.World()
    with pytest.raises(ValueError):
        w.add_hit(0xFFFFFFFF, "ACDEFGHK")
    assert 0xFFFFFFFF not in T.world().segs


def test_every_orf_case_meets_its_contract(ref):
    oix, views = ref
    cases = T.orf_cases()
    names = set()
    for ri, c in enumerate(cases):
        T.check_contract(c, T.target_of(c, views, ri))
        names.add(c["name"].split(" n=")[0])
    assert len(cases) > 400 and len(names) >= 20
    # both copies of the rule, both outcomes, on both strands, closed and open-ended
    for rescan in (False, True):
        for trimmed in (False, True):
            for plus, closed in T.ORIENTATIONS:
                assert any((c["n"] > 128) == rescan and (c["trim"] > 0) == trimmed and c["n_best"] >= 2 and c["plus"] == plus
                           and c["orf"].endswith("*") == closed for c in cases)


def test_wave_mix_is_present(ref):
    oix, views = ref
    assert len(T.wave_mix_groups(views)) >= 1


def test_protein_cases_meet_their_contract(ref, oracle):
    oix, _ = ref
    for c in T.protein_cases():
        pid, km, _ = oix.search(c["query"])
        T.check_protein_contract(c, pid, km)
    assert [c["n"] for c in T.protein_cases()] == list(T.PROTEIN_TIE_COUNTS)


def _host_flow(klib, v, rng, opts):
    """the library's host post-steps on the ORF's hits handed over in a shuffled order -> (order of ids, trim, start, size, kept)"""
    shuffle = rng.permutation(v.n)
    pid = np.ascontiguousarray(v.pid[shuffle], np.uint32)
    km = np.ascontiguousarray(v.km[shuffle], np.uint32)
    fp = np.ascontiguousarray(v.fp[shuffle], np.uint32)
    order = np.zeros(v.n, np.uint32)
    klib.kaamer_sort_hits(pid.ctypes.data, km.ctypes.data, v.n, order.ctypes.data)
    kms, fps = np.ascontiguousarray(km[order]), np.ascontiguousarray(fp[order])
    sa = np.array(v.starts, np.int32)
    seq = v.seq.encode("latin-1")
    sp, so = C.c_int32(v.start), C.c_int32(v.size)
    trim = klib.kaamer_set_best_start_codon(kms.ctypes.data, fps.ctypes.data, v.n, sa.ctypes.data if len(sa) else None, len(sa),
                                            int(v.plus), seq, len(seq), C.byref(sp), C.byref(so))
    kept = [klib.kaamer_filter_results(kms.ctypes.data, v.n, so.value, *o) for o in opts]
    return pid[order].tolist(), trim, sp.value, so.value, kept


def test_host_post_steps_match_the_oracle(ref, klib):
    oix, views = ref
    rng = np.random.default_rng(3)
    opts = [o for o in T.OPTS if o[1] == 1]                # (the gate of MinKMatch is the caller's: search_fastq.go:120)
    n = 0
    for v in views:
        if v.n == 0:
            continue
        order, trim, sp, so, kept = _host_flow(klib, v, rng, opts)
        assert order == v.pid.tolist()
        assert (trim, sp, so) == v.best_start(), v.seq
        assert kept == [v.flow(*o)[0] for o in opts]
        n += 1
    assert n >= len(T.orf_cases()) - 20
    for o in T.GATE_OPTS:                                   # the ratio and MinKMatch edges, on the trimmed size
        for v in views:
            f = v.flow(*o)
            if f is not None:
                kms = np.ascontiguousarray(v.km, np.uint32)
                assert klib.kaamer_filter_results(kms.ctypes.data, v.n, f[3], *o) == f[0]
