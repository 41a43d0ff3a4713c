#!/usr/bin/env python3
"""What reading a database GBK file (GenBank / GenPept flat file) on the device costs and buys (profiles/r26_makedb_gbk.md).

    python tools/bench_makedb_gbk.py [--proteins N] [--rounds R] [--device D] [--out FILE]

On one MI355X.  The input is DB-SP of the project's generator (workload.make_db) written as GenPept entries, twice: lean, with
LOCUS, DEFINITION, VERSION, SOURCE / ORGANISM with two taxonomy lines, ORIGIN and the sequence lines of 60 residues in blocks
of ten, and, for a third of the proteins, GenPept-shaped, with ACCESSION, DBSOURCE, KEYWORDS, three REFERENCE blocks, a
COMMENT and a FEATURES table, which the reader classifies and then leaves alone (one text, under 2^32 - 1 bytes).  Every
second entry's DEFINITION runs over two lines, so that the " [" ... "]." removal crosses a join.  On the same bytes, rounds
alternating, every round listed:
  1. kaamer_makedb_gbk (host) against kaamer_makedb_gbk_device: wall time of the whole call, so upload, download and the
     assembly of the table are in it; the two tables are compared first;
  2. kaamer_makedb_gbk + kaamer_index_build_proteins against kaamer_index_build_gbk;
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_makedb_gbk.md"))
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


REFS = b"".join(b"REFERENCE   %d  (residues 1 to 214)\n  AUTHORS   Blattner,F.R., Plunkett,G. III, Bloch,C.A., Perna,N.T., Burland,V.,\n"
                b"            Riley,M., Collado-Vides,J., Glasner,J.D., Rode,C.K., Mayhew,G.F.,\n            Gregor,J. and Davis,N.W.\n"
                b"  TITLE     The complete genome sequence of Escherichia coli K-12\n  JOURNAL   Science 277 (5331), 1453-1462 (1997)\n"
                b"   PUBMED   9278503\n" % k for k in (1, 2, 3))
COMMENT = (b"COMMENT     PROVISIONAL REFSEQ: This record has not yet been subject to final\n            NCBI review. The reference sequence is identical to the\n"
           b"            submitted protein. Catalyzes the reversible transfer of the\n            terminal phosphate group between ATP and AMP; plays an important\n"
           b"            role in cellular energy homeostasis and in adenine nucleotide\n            metabolism.\n            Method: conceptual translation.\n")
FEATURES = (b"FEATURES             Location/Qualifiers\n     source          1..214\n                     /organism=\"Escherichia coli str. K-12 substr. MG1655\"\n"
            b"                     /strain=\"K-12\"\n                     /sub_strain=\"MG1655\"\n                     /db_xref=\"taxon:511145\"\n"
            + b"".join(b"     %-15s %d..%d\n                     /region_name=\"feature %d of the chain\"\n                     /note=\"adenylate kinase family; "
                       b"evidence by similarity\"\n                     /db_xref=\"CDD:%d\"\n" % (k, 1 + 7 * i, 9 + 7 * i, i, 238000 + i)
                       for i, k in enumerate((b"Protein", b"Region", b"Site", b"Site", b"Site", b"Region", b"Region", b"CDS")))
            + b"                     /coded_by=\"NC_000913.3:496399..497043\"\n                     /transl_table=11\n")

SEQ_LINE = 76   # "%9d " + six blocks of ten residues with a space between + '\n'


def gbk_of(db, fat, chunk=40_000):
    """packed proteins -> GenPept text; fat: with the sections the reader only classifies.  Sequence lines as NCBI writes
    them: the residue number right-aligned in nine columns, sixty lower-case residues in blocks of ten"""
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
        h = b"LOCUS       P%07d_GEN %14d aa            linear   BCT 02-OCT-2024\n" % (i, ln)
        if i % 2:
            h += b"DEFINITION  protein %d of family %d [Organism %d (strain K%d /\n            substrain %d)].\n" % (i, i // 10, i % 997, i % 13, i % 7)
        else:
            h += b"DEFINITION  protein %d of family %d\n            [Organism %d (strain K%d)].\n" % (i, i // 10, i % 997, i % 13)
        if fat:
            h += b"ACCESSION   P%07d\n" % i
        h += b"VERSION     P%07d.%d\n" % (i, 1 + i % 3)
        if fat:
            h += b"DBSOURCE    REFSEQ: accession NC_%06d.%d\nKEYWORDS    RefSeq.\n" % (i % 999983, 1 + i % 3)
        h += (b"SOURCE      Organism %d (strain K%d)\n  ORGANISM  Organism %d (strain K%d)\n            Bacteria; Phylum%d; Class%d; Order%d;\n            Family%d; Genus%d.\n"
              % (i % 997, i % 13, i % 997, i % 13, i % 5, i % 11, i % 17, i % 101, i % 499))
        if fat:
            h += REFS + COMMENT + FEATURES
        h += b"ORIGIN      \n"
        heads.append(h)
    hl = np.fromiter((len(h) for h in heads), dtype=np.int64, count=n)
    full, rem = lens // 60, lens % 60
    sl = full * SEQ_LINE + np.where(rem > 0, 10 + rem + (rem - 1) // 10 + 1, 0)   # the sequence lines of a protein, line ends included
    start = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(hl + sl + 3, out=start[1:])
    text = np.full(int(start[-1]), ord(" "), dtype=np.uint8)
    _place(text, start[:-1], heads)
    del heads
    seq_at = start[:-1] + hl
    j = np.arange(int(offs[-1] - offs[0]), dtype=np.int64) - np.repeat(offs[:-1] - offs[0], lens)   # a residue's index in its protein
    text[np.repeat(seq_at, lens) + (j // 60) * SEQ_LINE + 10 + (j % 60) + (j % 60) // 10] = buf[int(offs[0]):int(offs[-1])] | 0x20   # lower case
    del j
    n_lines = full + (rem > 0)
    k = np.arange(int(n_lines.sum()), dtype=np.int64) - np.repeat(np.cumsum(n_lines) - n_lines, n_lines)   # a line's index in its protein
    line_at = np.repeat(seq_at, n_lines) + k * SEQ_LINE
    text[np.minimum(line_at + SEQ_LINE, np.repeat(seq_at + sl, n_lines)) - 1] = ord("\n")
    number = k * 60 + 1   # right-aligned in columns 0 .. 8
    for d in range(9):
        has = number >= 10 ** d
        if not has.any():
            break
        text[line_at[has] + 8 - d] = ord("0") + (number[has] // 10 ** d) % 10
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
    return api.Proteins.from_gbk(text)


def device_table(text):
    return api.Proteins.from_gbk(text, device=args.device)


def host_index(text):
    """the route that was there before: the host reader's table, its arrays handed to the device builder as they lie"""
    p = api.Proteins.from_gbk(text)
    ptr = [C.cast(f(p._h), C.c_void_p) for f in (L.kaamer_proteins_seqs, L.kaamer_proteins_offsets, L.kaamer_proteins_ids)]
    ix = C.c_void_p()
    abi.check(L.kaamer_index_build_proteins(*ptr, len(p), 0, 1, 0.5, args.device, C.byref(ix)))
    return p, api.Index(ix, args.device)


def device_index(text):
    return api.Index.from_gbk_text(text, device=args.device)


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
        m = re.match(r"\[kaamer makedb gbk\] (.+?)\s+([0-9.]+) ms", ln)
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


say("# r26: the makedb GBK reader on the device")
say()
say("`tools/bench_makedb_gbk.py --proteins %d --rounds %d`, one %s; wall times in seconds of the whole call (host clock, the"
    % (args.proteins, args.rounds, torch.cuda.get_device_name(args.device)))
say("call ends synchronised), rounds alternating host / device after one warm-up of each, every round listed, `med` = median.")
say()
t0 = time.perf_counter()
db = workload.make_db(args.proteins)
third = args.proteins // 3
inputs = [("DB-SP as GenPept entries, lean: LOCUS, DEFINITION, VERSION, SOURCE / ORGANISM, ORIGIN and the sequence", gbk_of(db, False)),
          ("a third of DB-SP, GenPept-shaped: ACCESSION, DBSOURCE, KEYWORDS, REFERENCE blocks, COMMENT and a FEATURES table in every entry", gbk_of((db[0], db[1][:third + 1]), True))]
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
    n_acc = len(h)
    close((h, d))
    say("## %s: %.1f MB of text, %d lines, %d entries, %d kept" % (name, mb, text.count(b"\n"), text.count(b"\n//\n"), n_acc))
    say()
    say("Device table equals the host table (ids, offsets, sequences, stats, feature names, %d entries, the saved file): **%s**" % (len(pick), "yes" if same else "NO"))
    say()
    for title, host_fn, dev_fn in (("table: `kaamer_makedb_gbk` / `kaamer_makedb_gbk_device`", host_table, device_table),
                                   ("index: `kaamer_makedb_gbk` + `kaamer_index_build_proteins` / `kaamer_index_build_gbk`", host_index, device_index)):
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
    say("- stages of one `kaamer_makedb_gbk_device` call by HIP events (second traced call):")
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
