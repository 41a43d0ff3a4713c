#!/usr/bin/env python3
"""What writing the TSV rows on the device costs and buys (profiles/r19_tsv_rows.md).

    python tools/tsv_bench.py [--reads N] [--queries N] [--db-proteins P] [--rounds R] [--out FILE] [--resources FILE]

On one MI355X, MaxResults 10, MinKMatch 10, MinKRatio 0.05, two inputs sampled from the synthetic database so that rows come
out: N reads of 150 nt as FASTQ (READS) and N protein queries as 60-column FASTA (PROTEIN); Annotations off and on
(ExtractPositions off: the rows of a plain request).
  1. the stage alone: HIP-event time of kaamer_tsv_rows_device behind a device-resident search of the same batch, rows and
     bytes per second, beside the search (kaamer_search_device + kaamer_topn_device) itself;
  2. the host-buffer call, one caller and four, wall time, three routes on the same text, rounds alternating:
       (a) the text call without rows, (b) the same call followed by kaamer_format_tsv on the caller's thread,
       (c) the call that returns the rows (kaamer_search_*_top_tsv_flat).
     (b) is the host formatter this work itself supplies: the parent commit has none.
Everything is reported, nothing gates.  --resources: a file with the kernels' -Rpass-analysis=kernel-resource-usage
remarks, appended as it is."""
import argparse
import ctypes as C
import os
import statistics
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from kaamer_amd import abi, api, workload

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--queries", type=int, default=10_000)
ap.add_argument("--db-proteins", type=int, default=560000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r19_tsv_rows.md"))
ap.add_argument("--resources", default=None)
args = ap.parse_args()

L = abi.lib()
RATIO, MINK, K = 0.05, 10, 10
out = []


def say(line=""):
    print(line, flush=True)
    out.append(line)


def med(xs):
    return statistics.median(xs)


def rounds(xs, scale=1.0, fmt="%.2f"):
    return ", ".join(fmt % (x * scale) for x in xs)


db = workload.make_db(args.db_proteins)
buf, offs = db
# the protein table: EntryId as UniProt writes it, three annotation columns of the usual sizes
rows = [b"EntryID\tSequence\tProteinName\tOrganism\tEC"]
raw = buf.tobytes()
for i in range(args.db_proteins):
    rows.append(b"sp|P%06d|PROT%d_SYNTH\t%s\tSynthetic protein %d of family %d\tSyntheticus exemplaris (strain %d)\t%s"
                % (i, i % 97, raw[int(offs[i]):int(offs[i + 1])], i, i // 10, i % 13, b"" if i % 3 else b"2.7.%d.%d" % (i % 11, i % 89)))
table = api.Proteins.from_tsv(b"\n".join(rows) + b"\n")
del rows, raw
assert len(table) == args.db_proteins
reads = workload.make_reads(db, args.reads, seed=workload.SEED + 2)
r2 = reads[0].reshape(args.reads, 150)
names = np.frombuffer(b"".join(b"@SRR0000001.%08d %08d length=150\n" % (i, i) for i in range(args.reads)), np.uint8).reshape(args.reads, -1)
text_r = np.concatenate([names, r2, np.broadcast_to(np.frombuffer(b"\n+\n", np.uint8), (args.reads, 3)),
                         np.full((args.reads, 150), ord("I"), np.uint8), np.full((args.reads, 1), 10, np.uint8)], axis=1).tobytes()
del names
q = workload.make_protein_queries(db, args.queries)
qs = workload.unpack(q)
text_p = b"".join(b">query_%05d some description of the query\n" % i + b"\n".join(s[j:j + 60] for j in range(0, len(s), 60)) + b"\n"
                  for i, s in enumerate(qs))
INPUTS = [("reads", "%d FASTQ reads of 150 nt" % args.reads, text_r, abi.READS, "fastq", args.reads),
          ("proteins", "%d protein queries, 60-column FASTA" % args.queries, text_p, abi.PROTEIN, "fasta", args.queries)]

img = api.Image.from_proteins(packed=db, device=0)
ix = api.Index.from_image(img, 0)
ix.attach_subject_text(table)
info = ix.subject_text_info()

say("# TSV response rows on the device: the stage, the text calls, the host formatter")
say()
say("`tools/tsv_bench.py --reads %d --queries %d --db-proteins %d --rounds %d` on one MI355X; medians of the rounds, every round listed, routes "
    "alternating within one session.  MaxResults %d, MinKMatch %d, MinKRatio %.2f, ExtractPositions off.  The subject text of the %d entries "
    "(EntryId, Length, three annotation columns pre-joined) takes %.1f MB of HBM; the longest row suffix is %d bytes."
    % (args.reads, args.queries, args.db_proteins, args.rounds, K, MINK, RATIO, info["entries"], info["table_bytes"] / 1e6, info["max_row_suffix"]))
say()


def call(fn, *a):
    o = C.POINTER(abi.BatchTop)()
    abi.check(fn(*a, C.byref(o)))
    return o


def route_a(text, st, fmt, ann):
    o = call(L.kaamer_search_text_top_flat, ix._h, text, len(text), 1, st, RATIO, MINK, K) if fmt == "fastq" else \
        call(L.kaamer_search_fasta_top_flat, ix._h, text, len(text), st, 0, RATIO, MINK, K)
    L.kaamer_batch_top_free(o)


def route_b(text, st, fmt, ann, keep=None):
    o = call(L.kaamer_search_text_top_flat, ix._h, text, len(text), 1, st, RATIO, MINK, K) if fmt == "fastq" else \
        call(L.kaamer_search_fasta_top_flat, ix._h, text, len(text), st, 0, RATIO, MINK, K)
    sp, ns = C.POINTER(abi.TextSpan)(), C.c_uint32()
    abi.check(L.kaamer_batch_top_text_spans(o, C.byref(sp), C.byref(ns)))
    need = L.kaamer_format_tsv(o, text, len(text), sp, ns.value, table._h, 0, ann, None, 0, None)
    assert need >= 0
    b = C.create_string_buffer(need + 1)
    got = L.kaamer_format_tsv(o, text, len(text), sp, ns.value, table._h, 0, ann, b, need + 1, None)
    assert got == need
    if keep is not None:
        keep.append(b.raw[:need])
    L.kaamer_batch_top_free(o)


def route_c(text, st, fmt, ann, keep=None):
    o = call(L.kaamer_search_text_top_tsv_flat, ix._h, text, len(text), 1, st, RATIO, MINK, K, 0, ann) if fmt == "fastq" else \
        call(L.kaamer_search_fasta_top_tsv_flat, ix._h, text, len(text), st, 0, RATIO, MINK, K, 0, ann)
    vp, vn, vo = C.c_void_p(), C.c_uint64(), C.POINTER(C.c_uint64)()
    abi.check(L.kaamer_batch_top_tsv(o, C.byref(vp), C.byref(vn), C.byref(vo)))
    if keep is not None:
        keep.append(C.string_at(vp.value, vn.value))
        keep.append(int(o.contents.top_off[o.contents.n_reported]))
    L.kaamer_batch_top_free(o)


def callers(fn, n, *a):
    """n threads, one call each on the same text (ctypes releases the GIL): wall time of all"""
    th = [threading.Thread(target=fn, args=a) for _ in range(n)]
    t0 = time.perf_counter()
    for x in th:
        x.start()
    for x in th:
        x.join()
    return time.perf_counter() - t0


say("| input | text bytes | annotations | rows per batch | bytes per batch | bytes per row |")
say("|---|---|---|---|---|---|")
SHAPE = {}
for key, what, text, st, fmt, n_rec in INPUTS:
    for ann in (0, 1):
        kb, kc = [], []
        route_b(text, st, fmt, ann, kb)
        route_c(text, st, fmt, ann, kc)
        assert kb[0] == kc[0] and kc[1] > 0, "the two formatters differ"
        SHAPE[key, ann] = (kc[1], len(kc[0]))
        say("| %s | %d | %s | %d | %d | %.0f |" % (what, len(text), "on" if ann else "off", kc[1], len(kc[0]), len(kc[0]) / kc[1]))
say()
say("(The rows of route (b) and route (c) were compared byte for byte on every input before anything was timed.)")
say()

# ---- 1. the stage alone ---------------------------------------------------------------------------------------------
say("## 1. The stage alone")
say()
say("Device-resident: the text parsed on the device, `kaamer_search_device` + `kaamer_topn_device` (HIP events around the two: \"search\"), then "
    "`kaamer_tsv_rows_device` (HIP events around its four launches and the copy of the counts: \"rows\"), one stream.")
say()
say("| input | annotations | search | rows | rows/s | bytes/s |")
say("|---|---|---|---|---|---|")
stream = torch.cuda.Stream()
for key, what, text, st, fmt, n_rec in INPUTS:
    parser = api.TextParser(len(text), max_records=n_rec + 16, max_lines=text.count(b"\n") + 16)
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        pr = parser.parse_device(d_text.data_ptr(), len(text), stream=stream.cuda_stream, fmt=fmt)
        ws = api.Workspace(ix, int(pr.seq_bytes) + 4096, n_rec + 16, seq_type=st)
        for ann in (0, 1):
            n_rows, n_bytes = SHAPE[key, ann]
            stage = api.TsvStage(ix, ws.query_capacity, n_rows + 16)
            d_out = torch.empty(n_bytes + 4096, dtype=torch.uint8, device="cuda")
            ms_s, ms_r = [], []
            for it in range(args.rounds + 2):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record(stream)
                dr = ws.search_device(pr.d_seqs, pr.d_offsets, int(pr.n_records), int(pr.seq_bytes), seq_type=st,
                                      stream=stream.cuda_stream)
                top = ws.topn_device(RATIO, MINK, K, best_start_codon=(st != abi.PROTEIN), stream=stream.cuda_stream)
                e[1].record(stream)
                rin = abi.TsvRowsIn()
                rin.top = top
                rin.d_q, rin.d_n_queries, rin.n_queries_cap = dr.d_q, dr.d_n_queries, dr.n_queries_cap
                rin.n_names, rin.d_name_bytes, rin.name_bytes_len, rin.d_spans = int(pr.n_records), d_text.data_ptr(), len(text), pr.d_spans
                rin.pos, rin.extract_positions, rin.annotations = None, 0, ann
                stage.rows_device(rin, d_out.data_ptr(), n_bytes + 4096, stream=stream.cuda_stream)
                e[2].record(stream)
                got = stage.finish(stream.cuda_stream)
                ws.finish(stream.cuda_stream)
                assert got == (n_rows, n_bytes), (got, n_rows, n_bytes)
                if it >= 2:
                    ms_s.append(e[0].elapsed_time(e[1]))
                    ms_r.append(e[1].elapsed_time(e[2]))
            m = med(ms_r)
            say("| %s | %s | %.3f ms (rounds: %s) | %.3f ms (rounds: %s) | %.0f M | %.1f GB |"
                % (key, "on" if ann else "off", med(ms_s), rounds(ms_s, 1, "%.3f"), m, rounds(ms_r, 1, "%.3f"), n_rows / m / 1e3, n_bytes / m / 1e6))
            stage.close()
            del d_out
        ws.close()
    parser.close()
    del d_text
say()

# ---- 2. the host-buffer call ----------------------------------------------------------------------------------------
say("## 2. The host-buffer call")
say()
say("Wall time of the calls in ms; four callers = four threads, one call each on the same text, at once.  (a) the text call without rows; (b) the "
    "same call, then `kaamer_format_tsv` into a buffer of the needed size on the caller's thread (two passes: the length, then the bytes); (c) the "
    "`_tsv_` call.  (b) is the baseline this work itself supplies: the parent commit has no formatter.")
say()
say("| input | annotations | callers | (a) | (b) | (c) | (b) - (a) | (c) - (a) |")
say("|---|---|---|---|---|---|---|---|")
for key, what, text, st, fmt, n_rec in INPUTS:
    for ann in (0, 1):
        for n in (1, 4):
            for fn in (route_a, route_b, route_c) * 2:
                callers(fn, n, text, st, fmt, ann)   # warm-up: slots, bounds, staging
            t = {route_a: [], route_b: [], route_c: []}
            for it in range(args.rounds):
                for fn in (route_a, route_b, route_c):
                    t[fn].append(callers(fn, n, text, st, fmt, ann))
            a, b, c = (med(t[f]) * 1e3 for f in (route_a, route_b, route_c))
            say("| %s | %s | %d | %.2f (rounds: %s) | %.2f (rounds: %s) | %.2f (rounds: %s) | %.2f | %.2f |"
                % (key, "on" if ann else "off", n, a, rounds(t[route_a], 1e3), b, rounds(t[route_b], 1e3), c, rounds(t[route_c], 1e3), b - a, c - a))
say()
ix.close()
if args.resources and os.path.exists(args.resources):
    say("## Kernel resources")
    say()
    say("`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage` on the kernels of `tsv_rows.hip.inc`:")
    say()
    say("```")
    with open(args.resources) as f:
        for line in f.read().rstrip().split("\n"):
            say(line)
    say("```")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(out) + "\n")
