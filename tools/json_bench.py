#!/usr/bin/env python3
"""What writing the JSON objects on the device costs and buys (profiles/r21_json_rows.md).

    python tools/json_bench.py [--reads N] [--queries N] [--db-proteins P] [--rounds R] [--out FILE] [--resources FILE]

On one MI355X, MaxResults 10, MinKMatch 10, MinKRatio 0.05, two inputs sampled from the synthetic database: N protein queries
(with and without ExtractPositions) and N reads of 150 nt (READS: PositionHits always).  For each:
  1. the structured result of the packed-batch call with bitmaps, and kaamer_format_json_arrays on one caller thread
     (two passes: the length, then the bytes): wall time;
  2. the stage alone: HIP-event time of kaamer_json_rows_device behind a device-resident search of the same batch
     (kaamer_search_device + kaamer_topn_device + kaamer_topn_positions_device), objects and bytes per second.
The device's bytes and offsets are compared with the host formatter's before anything is timed.  Everything is reported,
nothing gates.  --resources: a file with the kernels' -Rpass-analysis=kernel-resource-usage remarks, appended as it is."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from kaamer_amd import abi, api, workload

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=100_000)
ap.add_argument("--queries", type=int, default=10_000)
ap.add_argument("--db-proteins", type=int, default=560000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r21_json_rows.md"))
ap.add_argument("--resources", default=None)
args = ap.parse_args()

RATIO, MINK, K = 0.05, 10, 10
out = []


def say(line=""):
    print(line, flush=True)
    out.append(line)


def rounds(xs, fmt="%.3f"):
    return ", ".join(fmt % x for x in xs)


db = workload.make_db(args.db_proteins)
buf, offs = db
rows = [b"EntryID\tSequence\tProteinName\tOrganism\tEC"]
raw = buf.tobytes()
for i in range(args.db_proteins):
    rows.append(b"sp|P%06d|PROT%d_SYNTH\t%s\tSynthetic protein %d of family %d\tSyntheticus exemplaris (strain %d)\t%s"
                % (i, i % 97, raw[int(offs[i]):int(offs[i + 1])], i, i // 10, i % 13, b"" if i % 3 else b"2.7.%d.%d" % (i % 11, i % 89)))
table = api.Proteins.from_tsv(b"\n".join(rows) + b"\n")
del rows, raw
reads = workload.make_reads(db, args.reads, seed=workload.SEED + 2)
prot = workload.make_protein_queries(db, args.queries)


def names_of(n, pattern):
    text = b"".join(pattern % (i, i) for i in range(n))
    ln = len(pattern % (0, 0))
    spans = np.zeros(n, api.SPAN_DTYPE)
    spans["name_off"] = np.arange(n, dtype=np.uint32) * ln + 1
    spans["name_len"] = ln - 2
    return text, spans


INPUTS = [("proteins", "%d protein queries" % args.queries, prot, abi.PROTEIN, 0, False, names_of(args.queries, b">query_%05d some description of query %05d\n")),
          ("proteins -pos", "%d protein queries, ExtractPositions" % args.queries, prot, abi.PROTEIN, 0, True,
           names_of(args.queries, b">query_%05d some description of query %05d\n")),
          ("reads", "%d reads of 150 nt" % args.reads, reads, abi.READS, 1, False, names_of(args.reads, b"@SRR0000001.%08d %08d length=150\n"))]

img = api.Image.from_proteins(packed=db, device=0)
ix = api.Index.from_image(img, 0)
ix.attach_subject_json(table)
info = ix.subject_json_info()

say("# JSON objects on the device: the stage against the host formatter")
say()
say("`tools/json_bench.py --reads %d --queries %d --db-proteins %d --rounds %d` on one MI355X; medians of the rounds, every round listed.  MaxResults %d, "
    "MinKMatch %d, MinKRatio %.2f.  The HitEntries values of the %d entries take %.1f MB of HBM; the longest is %d bytes."
    % (args.reads, args.queries, args.db_proteins, args.rounds, K, MINK, RATIO, info["entries"], info["table_bytes"] / 1e6, info["max_entry"]))
say()
say("| input | objects | bytes | bytes per object | host formatter, one thread (ms) | search + top-N + bitmaps on the device (ms) | stage (ms) | objects/s | bytes/s written |")
say("|---|---|---|---|---|---|---|---|---|")
stream = torch.cuda.Stream()
for key, what, packed, st, fmt, positions, (name_bytes, spans) in INPUTS:
    pbuf, poff = packed
    bitmaps = positions or st != abi.PROTEIN
    top = ix.search_top(packed=packed, seq_type=st, min_k_ratio=RATIO, min_k_match=MINK, max_results=K, want_positions=bitmaps)
    want, want_off = api.format_json(top, name_bytes, spans, table, seqs=pbuf if st == abi.PROTEIN else None, offsets=poff if st == abi.PROTEIN else None,
                                     seq_type=st, text_format=fmt, positions=positions)
    t_host = []
    for it in range(args.rounds):
        t0 = time.perf_counter()
        api.format_json(top, name_bytes, spans, table, seqs=pbuf if st == abi.PROTEIN else None, offsets=poff if st == abi.PROTEIN else None, seq_type=st,
                        text_format=fmt, positions=positions)
        t_host.append((time.perf_counter() - t0) * 1e3)
    n_obj, n_bytes = len(want_off) - 1, len(want)
    d_buf = torch.from_numpy(np.ascontiguousarray(pbuf)).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(poff).view(np.int64)).cuda()
    d_names = torch.frombuffer(bytearray(name_bytes) + bytearray(16), dtype=torch.uint8).cuda()
    d_spans = torch.frombuffer(bytearray(spans.tobytes()) + bytearray(16), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    n_seqs = len(poff) - 1
    ms_s, ms_r = [], []
    with torch.cuda.stream(stream):
        ws = api.Workspace(ix, len(pbuf) + 4096, n_seqs + 16, seq_type=st, first_pos=1)
        stage = api.JsonStage(ix, ws.query_capacity, n_obj + 16)
        d_out = torch.empty(n_bytes + 4096, dtype=torch.uint8, device="cuda")
        for it in range(args.rounds + 2):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record(stream)
            dr = ws.search_device(d_buf.data_ptr(), d_off.data_ptr(), n_seqs, len(pbuf), seq_type=st, stream=stream.cuda_stream)
            t = ws.topn_device(RATIO, MINK, K, best_start_codon=(st != abi.PROTEIN), stream=stream.cuda_stream)
            pos = ws.topn_positions_device(t, stream=stream.cuda_stream) if bitmaps else None
            e[1].record(stream)
            jin = abi.JsonRowsIn()
            jin.rows.top = t
            jin.rows.d_q, jin.rows.d_n_queries, jin.rows.n_queries_cap = dr.d_q, dr.d_n_queries, dr.n_queries_cap
            jin.rows.n_names, jin.rows.d_name_bytes, jin.rows.name_bytes_len, jin.rows.d_spans = len(spans), d_names.data_ptr(), len(name_bytes), d_spans.data_ptr()
            jin.rows.pos = abi.C.pointer(pos) if bitmaps else None
            jin.rows.extract_positions = int(positions)
            jin.d_aa = d_buf.data_ptr() if st == abi.PROTEIN else dr.d_orf_aa
            jin.aa_len = len(pbuf) if st == abi.PROTEIN else 1 << 40   # (the workspace's own residues: every window lies inside)
            jin.seq_type, jin.text_format = st, fmt
            res = stage.rows_device(jin, d_out.data_ptr(), n_bytes + 4096, stream=stream.cuda_stream)
            e[2].record(stream)
            got = stage.finish(stream.cuda_stream)
            ws.finish(stream.cuda_stream)
            assert got == (n_obj, n_bytes), (got, n_obj, n_bytes)
            if it == 0:   # the same bytes as the host formatter's, before anything is timed
                assert d_out[:n_bytes].cpu().numpy().tobytes() == want, "%s: the device's objects differ from the host formatter's" % key
            if it >= 2:
                ms_s.append(e[0].elapsed_time(e[1]))
                ms_r.append(e[1].elapsed_time(e[2]))
        stage.close()
        ws.close()
    m = statistics.median(ms_r)
    say("| %s | %d | %d | %.0f | %.1f (rounds: %s) | %.3f (rounds: %s) | %.3f (rounds: %s) | %.2f M | %.1f GB |"
        % (what, n_obj, n_bytes, n_bytes / max(n_obj, 1), statistics.median(t_host), rounds(t_host, "%.1f"), statistics.median(ms_s), rounds(ms_s), m, rounds(ms_r),
           n_obj / m / 1e3, n_bytes / m / 1e6))
    del d_out, d_buf, d_off, top, want
say()
say("(The device's bytes were compared with the host formatter's, byte for byte, on every input before anything was timed.)")
say()

# ---- 2. the text calls ------------------------------------------------------------------------------------------------
import ctypes as C
L = abi.lib()
say("## 2. The text calls, one caller")
say()
say("Wall time in ms.  (a) the text call without objects -- for the inputs whose objects carry bitmaps there is no text call that returns them without "
    "rows, so (a) is the plain call and (c) - (a) also holds the bitmaps' own cost; (b) `kaamer_format_json` on the caller's thread for the result of "
    "the packed call with bitmaps (section 1's column, repeated here); (c) the `_json_` call; copy: the device-to-host copy of the objects alone, "
    "bytes / 50 GB/s as a lower bound (not measured separately).")
say()
say("| input | text bytes | (a) | (c) | (c) - (a) | objects' bytes | copy at 50 GB/s |")
say("|---|---|---|---|---|---|---|")
qs = workload.unpack(prot)
text_p = b"".join(b">query_%05d some description of query %05d\n" % (i, i) + b"\n".join(s[j:j + 60] for j in range(0, len(s), 60)) + b"\n" for i, s in enumerate(qs))
r2 = reads[0].reshape(args.reads, 150)
text_r = b"".join(b"@SRR0000001.%08d %08d length=150\n%s\n+\n%s\n" % (i, i, r2[i].tobytes(), b"I" * 150) for i in range(args.reads))


def call(fn, *a):
    o = C.POINTER(abi.BatchTop)()
    abi.check(fn(*a, C.byref(o)))
    return o


def plain(text, st, fasta):
    o = call(L.kaamer_search_fasta_top_flat, ix._h, text, len(text), st, 0, RATIO, MINK, K) if fasta else \
        call(L.kaamer_search_text_top_flat, ix._h, text, len(text), 1, st, RATIO, MINK, K)
    L.kaamer_batch_top_free(o)
    return 0


def objects(text, st, fasta, positions):
    o = call(L.kaamer_search_fasta_top_json_flat, ix._h, text, len(text), st, 0, RATIO, MINK, K, positions) if fasta else \
        call(L.kaamer_search_text_top_json_flat, ix._h, text, len(text), 1, st, RATIO, MINK, K, positions)
    vn = C.c_uint64()
    abi.check(L.kaamer_batch_top_json(o, None, C.byref(vn), None))
    L.kaamer_batch_top_free(o)
    return int(vn.value)


for what, text, st, fasta, positions in (("%d protein queries, 60-column FASTA" % args.queries, text_p, abi.PROTEIN, True, 0),
                                         ("the same, ExtractPositions", text_p, abi.PROTEIN, True, 1),
                                         ("%d FASTQ reads of 150 nt" % args.reads, text_r, abi.READS, False, 0)):
    for _ in range(2):
        plain(text, st, fasta)
        nb = objects(text, st, fasta, positions)
    ta, tc = [], []
    for it in range(args.rounds):
        t0 = time.perf_counter(); plain(text, st, fasta); ta.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); objects(text, st, fasta, positions); tc.append((time.perf_counter() - t0) * 1e3)
    a_, c_ = statistics.median(ta), statistics.median(tc)
    say("| %s | %d | %.2f (rounds: %s) | %.2f (rounds: %s) | %.2f | %d | %.2f |" % (what, len(text), a_, rounds(ta, "%.2f"), c_, rounds(tc, "%.2f"), c_ - a_, nb, nb / 50e6))
say()
ix.close()
if args.resources and os.path.exists(args.resources):
    say("## Kernel resources")
    say()
    say("`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage` on the kernels of `json_rows.hip.inc`:")
    say()
    say("```")
    with open(args.resources) as f:
        for line in f.read().rstrip().split("\n"):
            say(line)
    say("```")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(out) + "\n")
