#!/usr/bin/env python3
"""What the device FASTQ reader costs and buys (profiles/r15_text_parse.md).

    python tools/text_parse_bench.py [--reads N] [--file-reads M] [--db-proteins P] [--rounds R] [--out FILE] [--resources FILE]

On one MI355X, reads of 150 nt from the bench.py reads workload as FASTQ text (workload.fastq_text), MaxResults 10:
  1. the parser alone: HIP-event time of kaamer_parse_fastq_device per N reads, text bytes in and sequence bytes out as
     GB/s next to the HBM figures bench.py's roofline uses;
  2. the host-buffer calls: kaamer_search_text_top_flat against kaamer_parse_fastq + kaamer_search_batch_top_flat on the
     same text, one caller and four, wall time per N reads, with the upload and the parse of the text route on their own;
  3. the file drivers: kaamer_search_text_file against kaamer_search_file on a plain and a gzip file of M reads, one and
     two replicas on the one card, reads/s; next to them what the host thread's stages cost when run alone over the same
     file (read, inflate, cut, the host reader), and the per-chunk device call from memory.
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
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from kaamer_amd import abi, api, workload

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--file-reads", type=int, default=10_000_000)
ap.add_argument("--db-proteins", type=int, default=560000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--chunk-text-bytes", type=int, default=64 << 20)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r15_text_parse.md"))
ap.add_argument("--resources", default=None)
args = ap.parse_args()

L = abi.lib()
RATIO, MINK, K = 0.05, 10, 10
HBM_PEAK_GBPS, HBM_ACHIEVABLE_GBPS = 8000.0, 6300.0   # bench.py's roofline: spec peak, and what streaming reaches
TRANSLATE_MS_PER_M = 1.09                             # translate_reads_kernel, profiles/r13_genetic_codes.md
out = []


def say(line=""):
    print(line, flush=True)
    out.append(line)


def med(xs):
    return statistics.median(xs)


db = workload.make_db(args.db_proteins)
reads = workload.make_reads(db, args.reads, seed=workload.SEED + 2)
text = bytes(workload.fastq_text(reads))
seq_bytes = int(reads[1][-1])
per_m = 1e6 / args.reads
say("# Device FASTQ reader: the parser, the text calls, the file drivers")
say()
say("`tools/text_parse_bench.py --reads %d --file-reads %d --db-proteins %d --rounds %d --chunk-text-bytes %d` on one MI355X; "
    "medians of the rounds, every round listed where it matters.  %d reads of 150 nt: %d bytes of FASTQ text, %d bytes of sequence "
    "(text / sequence = %.2f)." % (args.reads, args.file_reads, args.db_proteins, args.rounds, args.chunk_text_bytes, args.reads, len(text),
                                   seq_bytes, len(text) / seq_bytes))
say()

# ---- 1. the parser alone ------------------------------------------------------------------------------------------
parser = api.TextParser(len(text), max_records=args.reads + 16)
d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
st = torch.cuda.Stream()
res = abi.TextParseResult()
ms = []
with torch.cuda.stream(st):
    for it in range(args.rounds + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        abi.check(L.kaamer_parse_fastq_device(parser._h, d_text.data_ptr(), len(text), st.cuda_stream))
        e1.record(st)
        abi.check(L.kaamer_text_parser_finish(parser._h, st.cuda_stream, C.byref(res)))
        if it >= 2:
            ms.append(e0.elapsed_time(e1))
assert res.n_records == args.reads and res.seq_bytes == seq_bytes
m = med(ms)
say("## 1. The parser alone")
say()
say("HIP events around the seven launches of `kaamer_parse_fastq_device` (its two memsets and the result copy included), text resident in HBM.")
say()
say("| quantity | value |")
say("|---|---|")
say("| time per %d reads | %.3f ms (rounds: %s) |" % (args.reads, m, ", ".join("%.3f" % x for x in ms)))
say("| per 1 M reads | %.3f ms |" % (m * per_m))
say("| text in | %.0f GB/s |" % (len(text) / m / 1e6))
say("| sequence out | %.0f GB/s |" % (seq_bytes / m / 1e6))
say("| bytes the kernels move at least (text read by the count, line and gather passes; sequences written) | %.0f GB/s of the %.0f achievable / %.0f peak bench.py's roofline uses |"
    % ((2 * len(text) + 2 * seq_bytes) / m / 1e6, HBM_ACHIEVABLE_GBPS, HBM_PEAK_GBPS))
say("| next to `translate_reads_kernel`, the stage it now precedes | %.2f ms per 1 M reads there (profiles/r13_genetic_codes.md): the parse is %.2fx that |"
    % (TRANSLATE_MS_PER_M, m * per_m / TRANSLATE_MS_PER_M))
say()
parser.close()
del d_text

# ---- 2. the host-buffer calls ---------------------------------------------------------------------------------------
img = api.Image.from_proteins(packed=db, device=0)
ix = api.Index.from_image(img, 0)


def text_route(t):
    o = C.POINTER(abi.BatchTop)()
    abi.check(L.kaamer_search_text_top_flat(ix._h, t, len(t), 1, abi.READS, RATIO, MINK, K, C.byref(o)))
    L.kaamer_batch_top_free(o)


def parent_route(t):
    h = C.c_void_p()
    abi.check(L.kaamer_parse_fastq(t, len(t), C.byref(h)))
    o = C.POINTER(abi.BatchTop)()
    abi.check(L.kaamer_search_batch_top_flat(ix._h, L.kaamer_reads_seqs(h), L.kaamer_reads_offsets(h), L.kaamer_reads_count(h), abi.READS, RATIO, MINK,
                                             K, C.byref(o)))
    L.kaamer_batch_top_free(o)
    L.kaamer_reads_free(h)


def callers(fn, n):
    """n threads, one call each on the same text (ctypes releases the GIL): wall time of all"""
    th = [threading.Thread(target=fn, args=(text,)) for _ in range(n)]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    return time.perf_counter() - t0


# the parts of the text route, alone: the host copy into pinned staging + the upload, the parse, the parent's host parse
pin = torch.empty(len(text), dtype=torch.uint8).pin_memory()
dev = torch.empty(len(text), dtype=torch.uint8, device="cuda")
src = np.frombuffer(text, dtype=np.uint8)
up = []
for it in range(args.rounds + 1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pin.numpy()[:] = src
    dev.copy_(pin, non_blocking=True)
    torch.cuda.synchronize()
    up.append(time.perf_counter() - t0)
up = up[1:]
del pin, dev
hp = []
for it in range(args.rounds):
    t0 = time.perf_counter()
    h = C.c_void_p()
    abi.check(L.kaamer_parse_fastq(text, len(text), C.byref(h)))
    hp.append(time.perf_counter() - t0)
    L.kaamer_reads_free(h)
say("## 2. The host-buffer calls")
say()
say("`kaamer_search_text_top_flat` (text route) against `kaamer_parse_fastq` + `kaamer_search_batch_top_flat` (parent route) on the same %d-read text, "
    "database of %d proteins, wall time of the calls; four callers = four threads, one call each, at once." % (args.reads, args.db_proteins))
say()
say("| callers | text route | parent route | parent / text |")
say("|---|---|---|---|")
for n in (1, 4):
    for fn in (text_route, parent_route):
        callers(fn, n)   # warm-up: slots, bounds, staging
    a, b = [], []
    for it in range(args.rounds):   # alternating
        a.append(callers(text_route, n))
        b.append(callers(parent_route, n))
    say("| %d | %.1f ms per call batch = %.1f ms per 1 M reads (rounds: %s) | %.1f ms = %.1f ms per 1 M reads (rounds: %s) | %.2f |"
        % (n, med(a) * 1e3, med(a) * 1e3 * per_m / n, ", ".join("%.0f" % (x * 1e3) for x in a), med(b) * 1e3, med(b) * 1e3 * per_m / n,
           ", ".join("%.0f" % (x * 1e3) for x in b), med(b) / med(a)))
say()
say("The split of one text call, each part alone: host copy into pinned memory + upload of the %d bytes of text %.1f ms (the parent uploads %d bytes of "
    "sequence and offsets); device parse %.2f ms (section 1); the parent's host parse of the same text %.1f ms."
    % (len(text), med(up) * 1e3, seq_bytes + 8 * (args.reads + 1), m, med(hp) * 1e3))
say()
ix.close()

# ---- 3. the file drivers ------------------------------------------------------------------------------------------
n_rep = max(1, args.file_reads // args.reads)
tmpd = tempfile.mkdtemp(prefix="text_parse_bench_")
plain, gz = os.path.join(tmpd, "q.fastq"), os.path.join(tmpd, "q.fastq.gz")
member = gzip.compress(text, compresslevel=1)
with open(plain, "wb") as f, open(gz, "wb") as g:
    for _ in range(n_rep):
        f.write(text)
        g.write(member)
file_reads = n_rep * args.reads
for p in (plain, gz):   # into the page cache
    with open(p, "rb") as f:
        while f.read(1 << 26):
            pass


def stage_read(p):
    t0 = time.perf_counter()
    with open(p, "rb", buffering=0) as f:
        buf = bytearray(4 << 20)
        while f.readinto(buf):
            pass
    return time.perf_counter() - t0


def stage_inflate(p):
    t0 = time.perf_counter()
    with open(p, "rb", buffering=0) as f:
        z = zlib.decompressobj(16 + zlib.MAX_WBITS)
        while True:
            raw = f.read(1 << 20)
            if not raw:
                break
            while raw:
                z.decompress(raw, 4 << 20)
                raw = z.unconsumed_tail
                if z.eof:
                    raw, z = z.unused_data, zlib.decompressobj(16 + zlib.MAX_WBITS)
    return time.perf_counter() - t0


def stage_host_reader(p):
    t0 = time.perf_counter()
    rd = api.Reader(p, "fastq")
    while True:
        h = rd.next_handle(1 << 20, 1 << 40)
        if h is None:
            break
        L.kaamer_reads_free(h)
    rd.close()
    return time.perf_counter() - t0


chunk = text[:api.text_cut_fastq(text[:args.chunk_text_bytes])] if len(text) > args.chunk_text_bytes else text
t0 = time.perf_counter()
for _ in range(20):
    api.text_cut_fastq(chunk)
cut_s = (time.perf_counter() - t0) / 20
NOOP_H = api.Replicas.CHUNK_CB(lambda user, first, chunk_, top: 0)
NOOP_T = api.Replicas.TEXT_CHUNK_CB(lambda user, first, t, n, spans, nr, top: 0)
chunk_seqs = max(1, int(len(chunk) / (len(text) / args.reads)))   # the host driver's chunks hold as many reads as the text driver's


seen = {}   # ORFs each driver searched in its last run: the same file, so the same number


def run_host(reps, p):
    c = abi.Counters()
    t0 = time.perf_counter()
    abi.check(L.kaamer_search_file(reps._h, p.encode(), 1, 0, abi.READS, RATIO, MINK, K, chunk_seqs, 1 << 40, 3, C.cast(NOOP_H, C.c_void_p), None, C.byref(c)))
    seen["host"] = c.n_queries
    return time.perf_counter() - t0


def run_text(reps, p):
    c = abi.Counters()
    t0 = time.perf_counter()
    abi.check(L.kaamer_search_text_file(reps._h, p.encode(), 1, abi.READS, RATIO, MINK, K, args.chunk_text_bytes, 3, C.cast(NOOP_T, C.c_void_p), None,
                                        C.byref(c)))
    seen["text"] = c.n_queries
    return time.perf_counter() - t0


say("## 3. The file drivers")
say()
say("`kaamer_search_text_file` against `kaamer_search_file` (unchanged from the parent commit: its loop is shared, its reader is the same code) on files "
    "of %d reads (%d bytes of text; gzip: %d members, level 1, %d bytes), in the page cache, in_flight 3, chunks of %d bytes of text / %d reads, "
    "callbacks that do nothing." % (file_reads, len(text) * n_rep, n_rep, len(member) * n_rep, args.chunk_text_bytes, chunk_seqs))
say()
say("| file | replicas | text driver | host-reader driver | text / host |")
say("|---|---|---|---|---|")
rounds3 = max(2, min(3, args.rounds))
for n_replicas in (1, 2):
    reps = api.Replicas.from_image(img, [0] * n_replicas)
    for name, p in (("plain", plain), ("gzip", gz)):
        run_text(reps, p)
        run_host(reps, p)
        assert seen["text"] == seen["host"] > 0, seen
        a, b = [], []
        for it in range(rounds3):
            a.append(run_text(reps, p))
            b.append(run_host(reps, p))
        say("| %s | %d | %.2f M reads/s (%s s) | %.2f M reads/s (%s s) | %.2f |"
            % (name, n_replicas, file_reads / med(a) / 1e6, ", ".join("%.2f" % x for x in a), file_reads / med(b) / 1e6,
               ", ".join("%.2f" % x for x in b), med(b) / med(a)))
    reps.close()
say()
rd_s, inf_s, hr_plain, hr_gz = stage_read(plain), stage_inflate(gz), stage_host_reader(plain), stage_host_reader(gz)
n_chunks = (len(text) * n_rep) / max(1, len(chunk))
say("The stages of the host thread, each run alone over the same files (they are not timed inside the drivers): read %.2f s; inflate (zlib, one thread) "
    "%.2f s; cut %.3f ms per chunk = %.3f s per file; host copy + upload %.2f s per file (section 2's figure scaled); the host reader alone "
    "(`kaamer_reader_*`: read + split + classify + append) %.2f s plain, %.2f s gzip; the callbacks do nothing."
    % (rd_s, inf_s, cut_s * 1e3, cut_s * n_chunks, med(up) * n_rep, hr_plain, hr_gz))
say()
os.unlink(plain)
os.unlink(gz)
os.rmdir(tmpd)
if args.resources and os.path.exists(args.resources):
    say("## Kernel resources")
    say()
    say("`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage` on `parse_text.hip.inc`'s kernels:")
    say()
    say("```")
    with open(args.resources) as f:
        for line in f.read().rstrip().split("\n"):
            say(line)
    say("```")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(out) + "\n")
