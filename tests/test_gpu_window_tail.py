"""The long tail of the flatten (count_window.hip.inc): windows whose lanes all carry a postings list of 12 ids.

Eight families of 12 proteins share a random core of 220 residues (private flanks of 20), so every k-mer of a core has a
list of exactly 12 ids and a full window of 64 positions carries 64 x 11 = 704 ids beyond the first of every lane: the
two flattened rounds (128) and a tail of 576 -- in the group kernel's count two full rounds of GRP_LONG_UNROLL chunks and
a third with one live chunk (the clamped addresses); a 150-nt read is 44 positions x 11 ids: in the ORF kernel a tail of
five full chunks and a partial one.  12 distinct hits fit the smallest table, so nothing may leave for the G tier
(n_overflow == 0: the LDS tier did the work), and adjacent lanes share their first id: every run add has the length of
the window or of what is left of it.  n_post, the postings the kernel walked, is the oracle's sum of Kmatch."""
import numpy as np
import pytest

from kaamer_amd import abi

pytestmark = pytest.mark.gpu

AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
CODON = dict(zip(b"ACDEFGHIKLMNPQRSTVWY", (b"GCT", b"TGT", b"GAT", b"GAA", b"TTT", b"GGT", b"CAT", b"ATT", b"AAA", b"CTG", b"ATG",
                                          b"AAT", b"CCT", b"CAA", b"CGT", b"TCT", b"ACT", b"GTT", b"TGG", b"TAT")))
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _nt(aa):
    return b"".join(CODON[a] for a in aa)


def _rc(nt):
    return nt.translate(COMP)[::-1]


@pytest.fixture(scope="module")
def families(klib, oracle, gpu_device):
    from kaamer_amd import api
    rng = np.random.default_rng(1212)
    rnd = lambda n: bytes(AA[rng.integers(0, 20, n)])
    cores = [rnd(220) for _ in range(8)]
    db = [rnd(20) + c + rnd(20) for c in cores for _ in range(12)] + [rnd(100) for _ in range(200)]
    ids = np.arange(len(db), dtype=np.uint32) * 5 + 3
    ix = api.Index.from_image(api.Image.from_proteins(db, ids=ids), gpu_device)
    oix = oracle.Index.from_proteins(db, ids=ids)
    assert all(len(oix.search(c)[0]) == 12 for c in cores)
    mutated = bytearray(cores[1])
    for i in range(15, 220, 30):   # a substitution every 30 residues: empty lists inside the windows
        mutated[i] = AA[(AA.tolist().index(mutated[i]) + 1) % 20]
    queries = [cores[0], bytes(mutated), cores[2] + cores[3], cores[4][100:130], rnd(100)]
    exp = []
    for q in queries:
        pid, km, pos = oix.search(q, want_positions=True)
        exp.append((dict(zip(pid.tolist(), km.tolist())), {int(p): int(np.argmax(pos[i])) for i, p in enumerate(pid)},
                    {int(p): pos[i] for i, p in enumerate(pid)}))
    assert [len(e[0]) for e in exp] == [12, 12, 24, 12, 0]
    yield cores, ix, oix, rng, queries, exp
    ix.close()


@pytest.mark.parametrize("first_pos", [1, -1])
def test_protein_batch(families, first_pos):
    from test_gpu_protein import _device_search
    cores, ix, oix, rng, queries, exp = families
    hits, first, c = _device_search(ix, queries, first_pos=first_pos)
    for i, (h, f, _) in enumerate(exp):
        assert hits[i] == h, "query %d" % i
        if first_pos == 1:
            assert first[i] == f, "query %d" % i
    assert c["n_overflow"] == 0
    assert c["n_post"] == sum(sum(h.values()) for h, _, _ in exp)


def test_positions_pass(families):
    cores, ix, oix, rng, queries, exp = families
    res = ix.search(queries, want_positions=True)
    for i, (h, f, bits) in enumerate(exp):
        assert res.hits(i) == h and res.first_pos(i) == f, "query %d" % i
        got = res.positions(i)
        assert sorted(got) == sorted(bits), "query %d" % i
        for p in bits:
            assert (got[p] == bits[p]).all(), "query %d protein %d" % (i, p)
    assert res.counters["n_overflow"] == 0
    assert res.counters["n_post"] == sum(sum(h.values()) for h, _, _ in exp)


def _check_nucleotide(res, seqs, oracle, oix):
    from test_gpu_reads import _check_reads
    _check_reads(res, seqs, oracle, oix)   # every ORF: hits, Kmatch, first positions
    n_post = n_long = 0
    for q in range(res.n_queries):
        m = res.meta[q]
        aa = bytes(res.orf_aa[int(m["aa_off"]):int(m["aa_off"]) + int(m["aa_len"])]).decode("latin-1")
        km = oix.search(aa)[1]
        n_post += int(km.sum())
        n_long += len(km) == 12
    assert res.counters["n_overflow"] == 0
    assert res.counters["n_post"] == n_post
    return n_long


def test_reads_both_strands(families, oracle):
    cores, ix, oix, rng, queries, exp = families
    reads = []
    for c in cores:
        for a in (0, 85, 170):
            r = _nt(c[a:a + 50])
            reads += [r, _rc(r)]
    assert all(len(r) == 150 for r in reads)
    res = ix.search(reads, seq_type=abi.READS)
    assert _check_nucleotide(res, reads, oracle, oix) >= len(reads)   # the ORF that spans the read meets the family


def test_contig_in_the_larger_arena(families, oracle):
    cores, ix, oix, rng, queries, exp = families
    gap = lambda: bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 300)])
    contig = gap() + _nt(cores[5]) + gap() + _rc(_nt(cores[6])) + gap() + _nt(cores[7][:120]) + gap()
    assert len(contig) > 200          # (mean sequence length above 200 nt: the ORF kernel with the arena for long ORFs)
    res = ix.search([contig], seq_type=abi.NUCLEOTIDE)
    assert _check_nucleotide(res, [contig], oracle, oix) >= 3
