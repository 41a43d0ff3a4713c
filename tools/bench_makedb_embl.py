#!/usr/bin/env python3
"""What reading a database EMBL file (UniProt flat file) on the device costs and buys (profiles/r25_makedb_embl.md).

    python tools/bench_makedb_embl.py [--proteins N] [--rounds R] [--device D] [--out FILE]

On one MI355X.  The input is DB-SP of the project's generator (workload.make_db) written as flat-file entries, twice: lean,
with only the lines the reader reads (ID DE GN OS OC OX DR SQ and the sequence lines), and, for a third of the proteins,
UniProt-shaped, with AC / DT / R* / CC / FT / KW / PE lines and DR lines of other databases to 5 KB per entry, most of which
the reader skips (one text, under 2^32 - 1 bytes).  Every seventh entry declares fewer residues than it holds.  On the same
bytes, rounds alternating, every round listed:
  1. kaamer_makedb_embl (host) against kaamer_makedb_embl_device: wall time of the whole call, so upload, download and the
     assembly of the table are in it; the two tables are compared first;
  2. kaamer_makedb_embl + kaamer_index_build_proteins against kaamer_index_build_embl;
  3. the device reader's stages by HIP events (KAAMER_MAKEDB_TRACE), with bytes of text per second, and beside their sum the
     time a device-to-device copy of the same text takes: the ceiling of anything that reads the text once and writes it once.
Everything is reported; the bar the profile states (on every input the device route's median not above the host route's) is
printed as held or missed, nothing gates."""
import argparse
import ctypes as C
import os
import re
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from kaamer_amd import abi, api, workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--proteins", type=int, default=560_000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--device", type=int, default=0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_makedb_embl.md"))
args = ap.parse_args()
assert args.rounds >= 5, "at least five rounds per route"
assert torch.cuda.is_available(), "this measurement needs the GPU: there is no fallback"

L = abi.lib()
out = []


def say(line=""):
    print(line, flush=True)
    out.append(line)


def rounds(xs, fmt="%.3f"):
    return ", ".join(fmt % x for x in xs)


def _place(text, at, pieces):
    """pieces[i] (bytes) to text[at[i] ...]"""
    lens = np.fromiter((len(p) for p in pieces), dtype=np.int64, count=len(pieces))
    src = np.frombuffer(b"".join(pieces), dtype=np.uint8)
    off = np.zeros(len(pieces), dtype=np.int64)
    np.cumsum(lens[:-1], out=off[1:])
    text[np.repeat(at - off, lens) + np.arange(len(src), dtype=np.int64)] = src


AC_DT = (b"AC   Q%07d; P%07d;\nDT   01-JAN-1990, integrated into UniProtKB/Swiss-Prot.\nDT   01-JAN-1990, sequence version 1.\n"
         b"DT   02-OCT-2024, entry version %d.\n")
REFS = b"".join(b"RN   [%d]\nRP   NUCLEOTIDE SEQUENCE [LARGE SCALE GENOMIC DNA].\nRC   STRAIN=K12 / MG1655 / ATCC 47076;\nRX   PubMed=9278503; "
                b"DOI=10.1126/science.277.5331.1453;\nRA   Blattner F.R., Plunkett G. III, Bloch C.A., Perna N.T., Burland V., Riley M.,\n"
                b"RA   Collado-Vides J., Glasner J.D., Rode C.K., Mayhew G.F., Gregor J., Davis N.W.;\nRT   \"The complete genome sequence of Escherichia "
                b"coli K-12.\";\nRL   Science 277:1453-1462(1997).\n" % k for k in (1, 2, 3))
CC = (b"CC   -!- FUNCTION: Catalyzes the reversible transfer of the terminal phosphate group between\nCC       ATP and AMP. Plays an important role in "
      b"cellular energy homeostasis and in adenine\nCC       nucleotide metabolism. {ECO:0000255|HAMAP-Rule:MF_00235}.\nCC   -!- CATALYTIC ACTIVITY:\n"
      b"CC       Reaction=AMP + ATP = 2 ADP; Xref=Rhea:RHEA:12973, ChEBI:CHEBI:30616,\nCC         ChEBI:CHEBI:456215, ChEBI:CHEBI:456216; EC=2.7.4.3;\n"
      b"CC   -!- SUBUNIT: Monomer. {ECO:0000255|HAMAP-Rule:MF_00235}.\nCC   -!- SUBCELLULAR LOCATION: Cytoplasm {ECO:0000255|HAMAP-Rule:MF_00235}.\n"
      b"CC   -!- SIMILARITY: Belongs to the adenylate kinase family.\nCC   ---------------------------------------------------------------------------\n"
      b"CC   Copyrighted by the UniProt Consortium, see https://www.uniprot.org/terms\nCC   Distributed under the Creative Commons Attribution (CC BY 4.0) "
      b"License\nCC   ---------------------------------------------------------------------------\n")
DR_OTHER = b"".join(b"DR   %s; %s; -.\n" % (d, v) for d, v in ((b"EMBL", b"U00096; AAC73576.1; -; Genomic_DNA"), (b"PIR", b"A64778"), (b"RefSeq", b"NP_415007.1; NC_000913.3"),
                                                               (b"PDB", b"1AKE; X-ray; 2.00 A; A/B=1-214"), (b"SMR", b"P69441"), (b"STRING", b"511145.b0474"),
                                                               (b"InterPro", b"IPR006259; Adenyl_kin_sub"), (b"Pfam", b"PF00406; ADK; 1"), (b"PROSITE", b"PS00113; ADENYLATE_KINASE; 1")))
TAIL = (b"PE   1: Evidence at protein level;\nKW   ATP-binding; Cytoplasm; Kinase; Nucleotide-binding; Reference proteome; Transferase.\n"
        + b"".join(b"FT   %-15s %d..%d\nFT                   /note=\"feature %d of the chain\"\nFT                   /evidence=\"ECO:0000255|HAMAP-Rule:MF_00235\"\n"
                   % (k, 1 + 7 * i, 9 + 7 * i, i) for i, k in enumerate((b"CHAIN", b"REGION", b"BINDING", b"BINDING", b"BINDING", b"HELIX", b"STRAND", b"TURN"))))


def embl_of(db, fat, chunk=40_000):
    """packed proteins -> flat-file text; fat: with the lines the reader skips.  Sequence lines as UniProt writes them: five
    spaces, sixty residues in groups of ten"""
    buf, offs = db
    n = len(offs) - 1
    return b"".join(_entries(buf, offs[a:min(a + chunk, n) + 1].astype(np.int64), a, fat) for a in range(0, n, chunk))


def _entries(buf, offs, first, fat):
    """the entries of proteins first .. first + len(offs) - 2"""
    lens = offs[1:] - offs[:-1]
    n = len(lens)
    heads = []
    for i in range(first, first + n):
        ln = int(lens[i - first])
        d = ln - (1 + i % 5 if i % 7 == 0 and ln > 20 else 0)
        h = b"ID   P%07d_GEN              Reviewed;  %9d AA.\n" % (i, d)
        if fat:
            h += AC_DT % (i, i + 1, 100 + i % 50)
        h += (b"DE   RecName: Full=Protein %d of family %d {ECO:0000255|HAMAP-Rule:MF_%05d};\nDE            EC=2.7.%d.%d {ECO:0000255|HAMAP-Rule:MF_%05d};\n"
              b"GN   Name=gene%d; OrderedLocusNames=b%04d;\nOS   Organism %d (strain K%d / substrain %d).\nOC   Bacteria; Phylum%d; Class%d; Order%d;\n"
              b"OC   Family%d; Genus%d.\nOX   NCBI_TaxID=%d;\n" % (i, i // 10, i % 99999, i % 9, i % 50, i % 99999, i, i % 9999, i % 997, i % 13, i % 7, i % 5, i % 11,
                                                                i % 17, i % 101, i % 499, 100000 + i % 900000))
        if fat:
            h += REFS + CC
        h += b"DR   GO; GO:%07d; F:ATP binding; IEA:UniProtKB-UniRule.\nDR   GO; GO:%07d; P:nucleotide metabolic process; IEA:InterPro.\nDR   KEGG; eco:b%04d; -.\n" % (
            i % 99991, (3 * i) % 99991, i % 9999)
        if fat:
            h += DR_OTHER
        h += b"DR   HAMAP; MF_%05d; Adenylate_kinase_Adk; 1.\n" % (i % 99999)
        if fat:
            h += TAIL
        h += b"SQ   SEQUENCE   %d AA;  %d MW;  0123456789ABCDEF CRC64;\n" % (d, 110 * ln)
        heads.append(h)
    hl = np.fromiter((len(h) for h in heads), dtype=np.int64, count=n)
    full, rem = lens // 60, lens % 60
    sl = full * 71 + np.where(rem > 0, 5 + rem + (rem - 1) // 10 + 1, 0)   # the sequence lines of a protein, line ends included
    start = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(hl + sl + 3, out=start[1:])
    text = np.full(int(start[-1]), ord(" "), dtype=np.uint8)
    _place(text, start[:-1], heads)
    del heads
    seq_at = start[:-1] + hl
    j = np.arange(int(offs[-1] - offs[0]), dtype=np.int64) - np.repeat(offs[:-1] - offs[0], lens)   # a residue's index in its protein
    text[np.repeat(seq_at, lens) + (j // 60) * 71 + 5 + (j % 60) + (j % 60) // 10] = buf[int(offs[0]):int(offs[-1])]
    del j
    n_lines = full + (rem > 0)
    k = np.arange(int(n_lines.sum()), dtype=np.int64) - np.repeat(np.cumsum(n_lines) - n_lines, n_lines)   # a line's index in its protein
    text[np.minimum(np.repeat(seq_at, n_lines) + (k + 1) * 71, np.repeat(seq_at + sl, n_lines)) - 1] = ord("\n")
    term = seq_at + sl
    text[term] = ord("/")
    text[term + 1] = ord("/")
    text[term + 2] = ord("\n")
    return text.tobytes()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def host_table(text):
    return api.Proteins.from_embl(text)


def device_table(text):
    return api.Proteins.from_embl(text, device=args.device)


def host_index(text):
    """the route that was there before: the host reader's table, its arrays handed to the device builder as they lie"""
    p = api.Proteins.from_embl(text)
    ptr = [C.cast(f(p._h), C.c_void_p) for f in (L.kaamer_proteins_seqs, L.kaamer_proteins_offsets, L.kaamer_proteins_ids)]
    ix = C.c_void_p()
    abi.check(L.kaamer_index_build_proteins(*ptr, len(p), 0, 1, 0.5, args.device, C.byref(ix)))
    return p, api.Index(ix, args.device)


def device_index(text):
    return api.Index.from_embl_text(text, device=args.device)


def close(r):
    for x in (r if isinstance(r, tuple) else (r,)):
        x.close()


def trace_of(text):
    """the stage lines the library prints under KAAMER_MAKEDB_TRACE -> [(stage, ms)]"""
    os.environ["KAAMER_MAKEDB_TRACE"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            device_table(text).close()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["KAAMER_MAKEDB_TRACE"]
        f.seek(0)
        lines = f.read().decode("latin-1").splitlines()
    got = []
    for ln in lines:
        m = re.match(r"\[kaamer makedb embl\] (.+?)\s+([0-9.]+) ms", ln)
        if m:
            got.append((m.group(1).strip(), float(m.group(2))))
    return got


def copy_ms(n_bytes, reps=20):
    a = torch.empty(n_bytes, dtype=torch.uint8, device="cuda:%d" % args.device)
    b = torch.empty_like(a)
    b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


say("# r25: the makedb EMBL reader on the device")
say()
say("`tools/bench_makedb_embl.py --proteins %d --rounds %d`, one %s; wall times in seconds of the whole call (host clock, the"
    % (args.proteins, args.rounds, torch.cuda.get_device_name(args.device)))
say("call ends synchronised), rounds alternating host / device after one warm-up of each, every round listed, `med` = median.")
say()
t0 = time.perf_counter()
db = workload.make_db(args.proteins)
third = args.proteins // 3
inputs = [("DB-SP as flat-file entries, lean: only the lines the reader reads", embl_of(db, False)),
          ("a third of DB-SP, UniProt-shaped: AC / DT / R* / CC / FT / KW / PE and other DR lines in every entry", embl_of((db[0], db[1][:third + 1]), True))]
say("Inputs generated in %.1f s (workload.make_db, seed %d)." % (time.perf_counter() - t0, workload.SEED))
say()
held = True
for name, text in inputs:
    assert len(text) < 2 ** 32, "one text"
    mb = len(text) / 1e6
    h, d = host_table(text), device_table(text)
    hs, ho = h.packed
    ds, do = d.packed
    with tempfile.TemporaryDirectory() as tmp:
        h.save(os.path.join(tmp, "h"))
        d.save(os.path.join(tmp, "d"))
        same_file = open(os.path.join(tmp, "h"), "rb").read() == open(os.path.join(tmp, "d"), "rb").read()
    pick = np.concatenate([h.ids[:50], h.ids[::max(1, len(h) // 50)]])
    hits = h.fetch_hits(pick)
    same = (np.array_equal(h.ids, d.ids) and np.array_equal(ho, do) and np.array_equal(hs, ds) and h.stats() == d.stats()
            and h.feature_names == d.feature_names and hits == d.fetch_hits(pick) and same_file)
    n_acc, n_more = len(h), sum(len(e["Sequence"]) > e["Length"] for e in hits)
    close((h, d))
    say("## %s: %.1f MB of text, %d lines, %d entries, %d kept" % (name, mb, text.count(b"\n"), text.count(b"\n//\n"), n_acc))
    say()
    say("Device table equals the host table (ids, offsets, sequences, stats, feature names, %d entries of which %d hold more than they declare, the saved "
        "file with the whole strings): **%s**" % (len(pick), n_more, "yes" if same else "NO"))
    say()
    for title, host_fn, dev_fn in (("table: `kaamer_makedb_embl` / `kaamer_makedb_embl_device`", host_table, device_table),
                                   ("index: `kaamer_makedb_embl` + `kaamer_index_build_proteins` / `kaamer_index_build_embl`", host_index, device_index)):
        wh, r = timed(lambda: host_fn(text))
        close(r)
        wd, r = timed(lambda: dev_fn(text))
        close(r)
        th, td = [], []
        for _ in range(args.rounds):
            t, r = timed(lambda: host_fn(text))
            close(r)
            th.append(t)
            t, r = timed(lambda: dev_fn(text))
            close(r)
            td.append(t)
        ok = statistics.median(td) <= statistics.median(th)
        held = held and ok
        say("- %s" % title)
        say("  - host route:   %s; med %.3f s (%.0f MB/s)" % (rounds(th), statistics.median(th), mb / statistics.median(th)))
        say("  - device route: %s; med %.3f s (%.0f MB/s)" % (rounds(td), statistics.median(td), mb / statistics.median(td)))
        say("  - warm-up calls (not counted): host %.3f, device %.3f" % (wh, wd))
        say("  - ratio of the medians %.1f x; device median not above the host median: %s; device not slower in any round: %s"
            % (statistics.median(th) / statistics.median(td), "yes" if ok else "NO", "yes" if all(b <= a for a, b in zip(th, td)) else "no"))
    trace_of(text)
    stages = trace_of(text)
    cp = copy_ms(len(text))
    kernels = [(s, ms) for s, ms in stages if s not in ("upload", "host table", "download")]
    say("- stages of one `kaamer_makedb_embl_device` call by HIP events (second traced call):")
    say()
    say("  | stage | ms | GB/s of text |")
    say("  |---|---|---|")
    for s, ms in stages:
        say("  | %s | %.3f | %.1f |" % (s, ms, len(text) / ms * 1e-6 if ms > 0 else 0.0))
    ksum = sum(ms for _, ms in kernels)
    say("  | kernels, sum (without upload / host table / download) | %.3f | %.1f |" % (ksum, len(text) / ksum * 1e-6 if ksum else 0.0))
    say("  | device-to-device copy of the text (ceiling) | %.3f | %.1f |" % (cp, len(text) / cp * 1e-6))
    say()
say("## The bar")
say()
say("On every measured input the device route's median is not above the host route's: **%s**." % ("held" if held else "MISSED"))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(out) + "\n")
