#!/usr/bin/env python3
"""What the device FASTA reader costs and buys (profiles/r17_fasta_parse.md).

    python tools/fasta_parse_bench.py [--queries N] [--reads N] [--contig-mb M] [--db-proteins P] [--rounds R] [--out FILE] [--resources FILE]

On one MI355X, MaxResults 10, three inputs:
  (a) N protein queries of the bench.py protein workload as 60-column FASTA (PROTEIN),
  (b) reads of 150 nt as two-line FASTA (READS),
  (c) contigs of 30 kb totalling about M MB at 80 columns (NUCLEOTIDE),
and for each of them
  1. the parser alone: HIP-event time of kaamer_parse_fasta_device, text bytes in and sequence bytes out per second;
  2. the host-buffer call kaamer_search_fasta_top_flat against the parent route, kaamer_parse_fasta +
     kaamer_search_batch_top_flat, on the same text, one caller and four, wall time, rounds alternating;
  3. for (b) and (c) the file driver kaamer_search_fasta_file against kaamer_search_file, plain and gzip.
Everything is reported, nothing gates.  --resources: a file with the kernels' -Rpass-analysis=kernel-resource-usage
remarks, appended as it is."""
import argparse
import ctypes as C
import gzip
import os
import statistics
import sys
import tempfile
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from kaamer_amd import abi, api, workload

ap = argparse.ArgumentParser()
ap.add_argument("--queries", type=int, default=10_000)
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--contig-mb", type=int, default=300)
ap.add_argument("--db-proteins", type=int, default=560000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--chunk-text-bytes", type=int, default=64 << 20)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r17_fasta_parse.md"))
ap.add_argument("--resources", default=None)
args = ap.parse_args()

L = abi.lib()
RATIO, MINK, K = 0.05, 10, 10
R15_FASTQ_MS_PER_M = 0.907   # kaamer_parse_fastq_device per 1 M reads of 150 nt, profiles/r15_text_parse.md section 1
out = []


def say(line=""):
    print(line, flush=True)
    out.append(line)


def med(xs):
    return statistics.median(xs)


def rounds(xs, scale=1.0, fmt="%.3f"):
    return ", ".join(fmt % (x * scale) for x in xs)


def rows_text(seqs2d, header=b">r\n"):
    """(n, w) residues -> FASTA text with one line per record (no per-record Python)"""
    n = seqs2d.shape[0]
    head = np.broadcast_to(np.frombuffer(header, dtype=np.uint8), (n, len(header)))
    return np.concatenate([head, seqs2d, np.full((n, 1), 10, dtype=np.uint8)], axis=1).tobytes()


db = workload.make_db(args.db_proteins)
q = workload.make_protein_queries(db, args.queries)
text_a = workload.fasta_text(q, 60)
reads = workload.make_reads(db, args.reads, seed=workload.SEED + 2)
text_b = rows_text(reads[0].reshape(args.reads, 150))
CONTIG = 30000                                   # 375 lines of 80
n_contigs = max(1, args.contig_mb * 1000000 // CONTIG)
c_reads = workload.make_reads(db, n_contigs * CONTIG // 150, seed=workload.SEED + 5)
lines = np.concatenate([c_reads[0].reshape(-1, 80), np.full((n_contigs * CONTIG // 80, 1), 10, dtype=np.uint8)], axis=1)
text_c = rows_text(lines.reshape(n_contigs, -1)[:, :-1])     # (the rows' own '\n' closes the last line)
del lines, c_reads
INPUTS = [("a", "%d protein queries, 60 columns" % args.queries, text_a, abi.PROTEIN, args.queries, int(q[1][-1])),
          ("b", "%d reads of 150 nt, two lines each" % args.reads, text_b, abi.READS, args.reads, args.reads * 150),
          ("c", "%d contigs of %d nt, 80 columns" % (n_contigs, CONTIG), text_c, abi.NUCLEOTIDE, n_contigs, n_contigs * CONTIG)]

say("# Device FASTA reader: the parser, the text call, the file driver")
say()
say("`tools/fasta_parse_bench.py --queries %d --reads %d --contig-mb %d --db-proteins %d --rounds %d --chunk-text-bytes %d` on one MI355X; medians of "
    "the rounds, every round listed.  The comparison is always the parent route (the host reader `kaamer_parse_fasta` / `kaamer_search_file`, "
    "unchanged by this work) in the same session." % (args.queries, args.reads, args.contig_mb, args.db_proteins, args.rounds, args.chunk_text_bytes))
say()
say("| input | records | text bytes | sequence bytes | lines |")
say("|---|---|---|---|---|")
for key, what, text, st, n_rec, seq_bytes in INPUTS:
    say("| (%s) %s | %d | %d | %d | %d |" % (key, what, n_rec, len(text), seq_bytes, text.count(b"\n")))
say()

# ---- 1. the parser alone ------------------------------------------------------------------------------------------
say("## 1. The parser alone")
say()
say("HIP events around the seven launches of `kaamer_parse_fasta_device` (its four memsets and the result copy included), text resident in HBM, "
    "`upper_last = 0`.")
say()
say("| input | time | text in | sequence out |")
say("|---|---|---|---|")
parse_ms = {}
for key, what, text, st, n_rec, seq_bytes in INPUTS:
    parser = api.TextParser(len(text), max_records=n_rec + 16, max_lines=text.count(b"\n") + 16)
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    stream = torch.cuda.Stream()
    res = abi.TextParseResult()
    ms = []
    with torch.cuda.stream(stream):
        for it in range(args.rounds + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            abi.check(L.kaamer_parse_fasta_device(parser._h, d_text.data_ptr(), len(text), 0, stream.cuda_stream))
            e1.record(stream)
            abi.check(L.kaamer_text_parser_finish(parser._h, stream.cuda_stream, C.byref(res)))
            if it >= 2:
                ms.append(e0.elapsed_time(e1))
    assert res.n_records == n_rec and res.seq_bytes == seq_bytes, (res.n_records, res.seq_bytes)
    m = parse_ms[key] = med(ms)
    say("| (%s) | %.3f ms (rounds: %s) | %.0f GB/s | %.0f GB/s |" % (key, m, rounds(ms), len(text) / m / 1e6, seq_bytes / m / 1e6))
    parser.close()
    del d_text
say()
say("(b) is %.3f ms per 1 M reads; the FASTQ parser took %.3f ms per 1 M reads of the same length (profiles/r15_text_parse.md, 307 MB of text "
    "there against %d MB here)." % (parse_ms["b"] * 1e6 / args.reads, R15_FASTQ_MS_PER_M, len(text_b) // 1000000))
say()

# ---- 2. the host-buffer call ----------------------------------------------------------------------------------------
img = api.Image.from_proteins(packed=db, device=0)
ix = api.Index.from_image(img, 0)


def text_route(t, st):
    o = C.POINTER(abi.BatchTop)()
    abi.check(L.kaamer_search_fasta_top_flat(ix._h, t, len(t), st, 0, RATIO, MINK, K, C.byref(o)))
    n = o.contents.n_reported
    L.kaamer_batch_top_free(o)
    return n


def parent_route(t, st):
    h = C.c_void_p()
    abi.check(L.kaamer_parse_fasta(t, len(t), C.byref(h)))
    o = C.POINTER(abi.BatchTop)()
    abi.check(L.kaamer_search_batch_top_flat(ix._h, L.kaamer_reads_seqs(h), L.kaamer_reads_offsets(h), L.kaamer_reads_count(h), st, RATIO, MINK, K,
                                             C.byref(o)))
    n = o.contents.n_reported
    L.kaamer_batch_top_free(o)
    L.kaamer_reads_free(h)
    return n


def callers(fn, n, t, st):
    """n threads, one call each on the same text (ctypes releases the GIL): wall time of all"""
    th = [threading.Thread(target=fn, args=(t, st)) for _ in range(n)]
    t0 = time.perf_counter()
    for x in th:
        x.start()
    for x in th:
        x.join()
    return time.perf_counter() - t0


say("## 2. The host-buffer call")
say()
say("`kaamer_search_fasta_top_flat` (text route) against `kaamer_parse_fasta` + `kaamer_search_batch_top_flat` (parent route) on the same text, database "
    "of %d proteins, wall time of the calls in ms; four callers = four threads, one call each, at once; rounds alternate between the routes." % args.db_proteins)
say()
say("| input | callers | text route | parent route | parent / text |")
say("|---|---|---|---|---|")
host_parse = {}
for key, what, text, st, n_rec, seq_bytes in INPUTS:
    assert text_route(text, st) == parent_route(text, st) > 0
    hp = []
    for it in range(args.rounds):
        t0 = time.perf_counter()
        h = C.c_void_p()
        abi.check(L.kaamer_parse_fasta(text, len(text), C.byref(h)))
        hp.append(time.perf_counter() - t0)
        L.kaamer_reads_free(h)
    host_parse[key] = hp
    for n in (1, 4):
        for fn in (text_route, parent_route, text_route, parent_route):
            callers(fn, n, text, st)   # warm-up: slots, bounds, staging
        a, b = [], []
        for it in range(args.rounds):
            a.append(callers(text_route, n, text, st))
            b.append(callers(parent_route, n, text, st))
        say("| (%s) | %d | %.2f (rounds: %s) | %.2f (rounds: %s) | %.2f |" % (key, n, med(a) * 1e3, rounds(a, 1e3, "%.2f"), med(b) * 1e3,
                                                                            rounds(b, 1e3, "%.2f"), med(b) / med(a)))
say()
say("The parent's host parse alone (`kaamer_parse_fasta`, the caller's thread): " +
    "; ".join("(%s) %.2f ms (rounds: %s)" % (k, med(v) * 1e3, rounds(v, 1e3, "%.2f")) for k, v in host_parse.items()) +
    ".  The device parse of the same texts: " + ", ".join("(%s) %.3f ms" % (k, v) for k, v in parse_ms.items()) + " (section 1).")
say()
ix.close()

# ---- 3. the file driver -------------------------------------------------------------------------------------------
NOOP_H = api.Replicas.CHUNK_CB(lambda user, first, chunk_, top: 0)
NOOP_T = api.Replicas.TEXT_CHUNK_CB(lambda user, first, t, n, spans, nr, top: 0)
seen = {}


def run_host(reps, p, st, chunk_seqs):
    c = abi.Counters()
    t0 = time.perf_counter()
    abi.check(L.kaamer_search_file(reps._h, p.encode(), 0, 0, st, RATIO, MINK, K, chunk_seqs, 1 << 40, 3, C.cast(NOOP_H, C.c_void_p), None, C.byref(c)))
    seen["host"] = c.n_queries
    return time.perf_counter() - t0


def run_text(reps, p, st, chunk_seqs):
    c = abi.Counters()
    t0 = time.perf_counter()
    abi.check(L.kaamer_search_fasta_file(reps._h, p.encode(), st, RATIO, MINK, K, args.chunk_text_bytes, 3, C.cast(NOOP_T, C.c_void_p), None, C.byref(c)))
    seen["text"] = c.n_queries
    return time.perf_counter() - t0


say("## 3. The file driver")
say()
say("`kaamer_search_fasta_file` against `kaamer_search_file` (format 0; unchanged from the parent commit) on the texts of (b) and (c) as files in the "
    "page cache, plain and gzip (one member, level 1), one replica, in_flight 3, chunks of %d bytes of text and as many records for the host "
    "reader, callbacks that do nothing; seconds per file." % args.chunk_text_bytes)
say()
say("| input | file | text driver | host-reader driver | host / text |")
say("|---|---|---|---|---|")
tmpd = tempfile.mkdtemp(prefix="fasta_parse_bench_")
reps = api.Replicas.from_image(img, [0])
rounds3 = args.rounds
for key, what, text, st, n_rec, seq_bytes in INPUTS[1:]:
    plain, gz = os.path.join(tmpd, key + ".fa"), os.path.join(tmpd, key + ".fa.gz")
    with open(plain, "wb") as f:
        f.write(text)
    with open(gz, "wb") as f:
        f.write(gzip.compress(text, compresslevel=1))
    chunk_seqs = max(1, int(args.chunk_text_bytes / (len(text) / n_rec)))
    for name, p in (("plain", plain), ("gzip, %d bytes" % os.path.getsize(gz), gz)):
        run_text(reps, p, st, chunk_seqs)
        run_host(reps, p, st, chunk_seqs)
        assert seen["text"] == seen["host"] > 0, seen
        a, b = [], []
        for it in range(rounds3):
            a.append(run_text(reps, p, st, chunk_seqs))
            b.append(run_host(reps, p, st, chunk_seqs))
        say("| (%s) | %s | %.3f s = %.0f MB of text/s (rounds: %s) | %.3f s (rounds: %s) | %.2f |"
            % (key, name, med(a), len(text) / med(a) / 1e6, rounds(a), med(b), rounds(b), med(b) / med(a)))
    os.unlink(plain)
    os.unlink(gz)
reps.close()
os.rmdir(tmpd)
say()
if args.resources and os.path.exists(args.resources):
    say("## Kernel resources")
    say()
    say("`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage` on `parse_fasta.hip.inc`'s kernels (`pt_count_kernel` and "
        "`pt_tile_scan_kernel`, the first two launches, are the FASTQ parser's: profiles/r15_text_parse.md):")
    say()
    say("```")
    with open(args.resources) as f:
        for line in f.read().rstrip().split("\n"):
            say(line)
    say("```")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(out) + "\n")
