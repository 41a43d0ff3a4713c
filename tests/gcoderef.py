"""The expected side of the genetic-code tests (test_genetic_codes.py, test_gpu_genetic_codes.py).

The oracle is fixed to table 11.  For any other code the ORFs come from tests/pyref.py::get_orfs with
pyref.GCODE_BACTERIA swapped for the fixture's table (tests/golden/gcodes.json, parsed from the reference's gcode_N maps as
text); those ORFs then go through the oracle as queries (Index.search, set_best_start_codon, filter_results)."""
import json
import os
import random

import numpy as np

import pyref

HERE = os.path.dirname(os.path.abspath(__file__))
CODES = (1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14, 15)
BASES = "tcag"
CODONS = [a + b + c for a in BASES for b in BASES for c in BASES]   # t-c-a-g order, as kaamer_genetic_code returns them

_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = json.load(open(os.path.join(HERE, "golden", "gcodes.json")))
    return _fixture


def table(code):
    """codon -> (AA, Start, Stop), the shape of pyref.GCODE_BACTERIA"""
    return {codon: (v[0], bool(v[1]), bool(v[2])) for codon, v in fixture()[str(code)].items()}


def expected_orfs(monkeypatch, code, seqs):
    """per input sequence the list of dict(seq, start, end, plus, starts), in the reference's order"""
    monkeypatch.setattr(pyref, "GCODE_BACTERIA", table(code))
    try:
        return [pyref.get_orfs(s.decode("latin-1") if isinstance(s, bytes) else s) for s in seqs]
    finally:
        monkeypatch.undo()


def revcomp(s):
    return s[::-1].translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))


# the codons whose class differs between the tables: stops that come and go (tga, aga, agg, taa, tag), sense changes
# (ctg, ata, aaa), start codons only some tables have (ttg, ctg, att, atc, ata, gtg, tta)
_SPECIAL = (b"TGA", b"AGA", b"AGG", b"TAA", b"TAG", b"CTG", b"ATA", b"AAA", b"TTG", b"ATT", b"GTG", b"TTA")


def _closing_reads():
    """an ORF of 22 codons, then a table-specific stop ON the frame's last codon, and one codon before it; in the three
    frames and on both strands; a start codon of some tables only right behind a stop"""
    out = []
    body = b"ATG" + b"GCA" * 21
    for stop in (b"TGA", b"AGA", b"AGG", b"TAA", b"TAG"):
        for pre in (b"", b"C", b"CC"):
            out += [pre + body + stop, pre + body + stop + b"GCA", revcomp(pre + body + stop + b"GCA"), revcomp(pre + body + stop)]
        for start in (b"TTG", b"CTG", b"ATT", b"GTG", b"TTA", b"ATA"):
            out.append(b"GCA" * 3 + stop + start + b"GCT" * 22 + stop)
    return out


def make_batches(db):
    """-> {"short": (seq_type name, reads <= 150 nt), "wide": (reads of 200 .. 384 nt, mean > 160), "contigs": three contigs};
    deterministic: the CPU tests check, for the same batches, that every code's expected ORFs differ from table 11's"""
    from kaamer_amd import workload
    rng = random.Random(1913)

    def rnd(n, alphabet="ACGT"):
        return "".join(rng.choice(alphabet) for _ in range(n)).encode()

    def salted(n):   # random sequence rich in the codons the tables disagree on
        out = b""
        while len(out) < n:
            out += rng.choice(_SPECIAL) if rng.random() < 0.25 else rnd(3)
        return out[:n]

    short = workload.unpack(workload.make_reads(db, 200, seed=1301))
    short += [rnd(rng.randint(60, 150)) for _ in range(30)] + [salted(rng.randint(90, 150)) for _ in range(40)]
    short += [rnd(rng.randint(60, 150), "ACGTacgtNn") for _ in range(20)]       # N and lower-case bytes
    short += [b"AC", rnd(20), b"", b"ACG"] + _closing_reads()
    assert max(len(r) for r in short) <= 150 and sum(len(r) for r in short) <= 160 * len(short)

    wide = workload.unpack(workload.make_reads(db, 40, read_len=250, seed=1302)) + workload.unpack(workload.make_reads(db, 25, read_len=384, seed=1303))
    wide += [rnd(rng.randint(200, 384)) for _ in range(10)] + [salted(rng.randint(200, 384)) for _ in range(20)]
    wide += [rnd(rng.randint(200, 384), "ACGTacgtNn") for _ in range(8)]
    wide += [r + rnd(140) for r in _closing_reads()[:12]] + [rnd(150) + r for r in _closing_reads()[12:24]]
    assert 200 <= min(len(r) for r in wide) and max(len(r) for r in wide) <= 384 and sum(len(r) for r in wide) > 160 * len(wide)

    def contig(n, seed):
        c = bytearray(salted(n))
        genes = workload.unpack(workload.make_reads(db, max(1, n // 2500), read_len=600, seed=seed))
        for i, g in enumerate(genes):
            at = 150 + i * 2400
            if at + len(g) <= n:
                c[at:at + len(g)] = g
        for at in range(97, n - 10, 1511):       # N and lower-case bytes
            c[at:at + 4] = b"nNac"
        return bytes(c)

    contigs = [contig(400, 1304), contig(13000, 1305), contig(30000, 1306)]   # 13 000 nt: 4 333 codons per frame, past one 4 096-codon piece
    return {"short": short, "wide": wide, "contigs": contigs}


class Expected:
    """the expected pipeline of one database, with the oracle's per-ORF searches cached across codes"""

    def __init__(self, oracle, oix):
        self.oracle, self.oix, self._hits = oracle, oix, {}

    def hits(self, seq):
        """(pids, Kmatch, PositionHits rows) of one ORF, sortMapByValue order"""
        if seq not in self._hits:
            self._hits[seq] = self.oix.search(seq, want_positions=True)
        return self._hits[seq]

    def top(self, orfs, ratio=0.05, mink=10, maxr=10):
        """per ORF of the batch (flat, in order): None, or dict(pid, km, fp, trim, start, size) of a reported query:
        search_fastq.go:119-124 -- the gate, SetBestStartCodon, FilterResults on the possibly shrunk SizeInKmer"""
        out = []
        for per_seq in orfs:
            for o in per_seq:
                size = self.oracle.size_in_kmer(o["seq"])
                pid, km, pos = self.hits(o["seq"])
                if len(km) == 0 or km[0] < mink:
                    out.append(None)
                    continue
                trim, start, size2 = self.oracle.set_best_start_codon(km, pos, size, o["starts"], o["plus"], o["seq"], o["start"])
                keep = self.oracle.filter_results(km, size2, ratio, mink, maxr)
                if not keep:
                    out.append(None)
                    continue
                out.append(dict(pid=pid[:keep].tolist(), km=km[:keep].tolist(), fp=[int(np.argmax(pos[h])) for h in range(keep)],
                                trim=int(trim), start=int(start), size=int(size2), seq=o["seq"][int(trim):], end=o["end"], plus=o["plus"]))
        return out


def check_full(res, orfs, exp):
    """a BatchResult (full hit lists) against the expected ORFs, bit for bit: ORF strings, Start / EndPosition, strand,
    StartsAlternative, ORF order, SizeInKmer, {protein id -> Kmatch}, lowest match position"""
    flat = [(r, o) for r, per_seq in enumerate(orfs) for o in per_seq]
    assert res.n_queries == len(flat)
    for q, (r, o) in enumerate(flat):
        m = res.meta[q]
        aa = bytes(res.orf_aa[int(m["aa_off"]):int(m["aa_off"]) + int(m["aa_len"])]).decode("latin-1")
        sa = res.starts_alt[int(m["sa_off"]):int(m["sa_off"]) + int(m["sa_len"])].tolist()
        got = dict(seq=aa, start=int(m["start_position"]), end=int(m["end_position"]), plus=bool(m["plus_strand"]), starts=sa)
        assert int(m["src_seq"]) == r and got == o, "sequence %d query %d" % (r, q)
        assert int(m["size_in_kmer"]) == exp.oracle.size_in_kmer(aa)
        pid, km, pos = exp.hits(aa)
        assert res.hits(q) == dict(zip(pid.tolist(), km.tolist())), "sequence %d query %d" % (r, q)
        assert res.first_pos(q) == {int(p): int(np.argmax(pos[i])) for i, p in enumerate(pid)}
    return len(flat)


def check_top(top, exp_top):
    """a TopResult against Expected.top: reported queries, trim, StartPosition and SizeInKmer after SetBestStartCodon,
    the trimmed ORF, hits and top_first_pos"""
    assert top.n_queries == len(exp_top)
    rep = [q for q, e in enumerate(exp_top) if e is not None]
    assert top.rep_query.tolist() == rep
    for i, q in enumerate(rep):
        e, m = exp_top[q], top.meta[i]
        a, b = int(top.top_off[i]), int(top.top_off[i + 1])
        assert top.top_pid[a:b].tolist() == e["pid"] and top.top_kmatch[a:b].tolist() == e["km"], q
        assert top.top_first_pos[a:b].tolist() == e["fp"], q
        assert int(top.trim[i]) == e["trim"] and int(m["start_position"]) == e["start"] and int(m["size_in_kmer"]) == e["size"], q
        assert int(m["end_position"]) == e["end"] and bool(m["plus_strand"]) == e["plus"]
        assert bytes(top.orf_aa[int(m["aa_off"]):int(m["aa_off"]) + int(m["aa_len"])]).decode("latin-1") == e["seq"], q
    return len(rep)


def same_reported(got, ref):
    """two TopResults report the same queries and hits (the forms with alignments order a query's hits by BitScore)"""
    assert got.n_queries == ref.n_queries and got.rep_query.tolist() == ref.rep_query.tolist()
    assert got.top_off.tolist() == ref.top_off.tolist() and got.trim.tolist() == ref.trim.tolist()
    assert got.meta.tolist() == ref.meta.tolist() and bytes(got.orf_aa) == bytes(ref.orf_aa)
    for i in range(ref.n_reported):
        a, b = int(ref.top_off[i]), int(ref.top_off[i + 1])
        g = sorted(zip(got.top_pid[a:b].tolist(), got.top_kmatch[a:b].tolist(), got.top_first_pos[a:b].tolist()))
        assert g == sorted(zip(ref.top_pid[a:b].tolist(), ref.top_kmatch[a:b].tolist(), ref.top_first_pos[a:b].tolist())), i
        if got.alignments is None:
            assert got.top_pid[a:b].tolist() == ref.top_pid[a:b].tolist()
