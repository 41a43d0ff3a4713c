#!/usr/bin/env python3
"""What writing the -aln TSV rows on the device costs (profiles/r20_tsv_aln_rows.md).

    python tools/tsv_aln_bench.py [--reads N] [--queries N] [--db-proteins P] [--rounds R] [--out FILE] [--resources FILE]

On one MI355X, MaxResults 10, MinKMatch 10, MinKRatio 0.05, BLOSUM62 11 / 1, the inputs of tools/tsv_bench.py: N reads of
150 nt as FASTQ (READS) and N protein queries as 60-column FASTA (PROTEIN), sampled from the synthetic database;
Annotations off and on, ExtractPositions off.
  1. the stage alone: HIP-event time of kaamer_tsv_aln_rows_device behind a device-resident search and alignment of the
     same batch (text parsed on the device, kaamer_search_device + kaamer_topn_device, kaamer_topn_align_device), rows per
     second, beside the two stages before it;
  2. the host-buffer call, one caller and four, wall time, two routes on the same text, alternating within every round:
       (host) the host reader, kaamer_search_batch_top_aln_flat, kaamer_format_tsv_aln on the caller's thread,
       (device) kaamer_search_text_top_aln_tsv_flat / kaamer_search_fasta_top_aln_tsv_flat;
     their rows are compared byte for byte first.
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
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r20_tsv_aln_rows.md"))
ap.add_argument("--resources", default=None)
args = ap.parse_args()

RATIO, MINK, K = 0.05, 10, 10
out = []


def say(line=""):
    print(line, flush=True)
    out.append(line)


def med(xs):
    return statistics.median(xs)


def rounds(xs, fmt="%.3f"):
    return ", ".join(fmt % x for x in xs)


def home(ptr, n, dtype):
    a = np.zeros(n, dtype)
    if a.nbytes:
        assert api._hip_runtime().hipMemcpy(a.ctypes.data, C.c_void_p(ptr), a.nbytes, 2) == 0
    return a


db = workload.make_db(args.db_proteins)
buf, offs = db
rows = [b"EntryID\tSequence\tProteinName\tOrganism\tEC"]
raw = buf.tobytes()
for i in range(args.db_proteins):
    rows.append(b"sp|P%06d|PROT%d_SYNTH\t%s\tSynthetic protein %d of family %d\tSyntheticus exemplaris (strain %d)\t%s"
                % (i, i % 97, raw[int(offs[i]):int(offs[i + 1])], i, i // 10, i % 13, b"" if i % 3 else b"2.7.%d.%d" % (i % 11, i % 89)))
print("database text ready", file=sys.stderr, flush=True)
table = api.Proteins.from_tsv(b"\n".join(rows) + b"\n")
print("protein table ready", file=sys.stderr, flush=True)
del rows, raw
reads = workload.make_reads(db, args.reads, seed=workload.SEED + 2)
r2 = reads[0].reshape(args.reads, 150)
names = np.frombuffer(b"".join(b"@SRR0000001.%08d %08d length=150\n" % (i, i) for i in range(args.reads)), np.uint8).reshape(args.reads, -1)
text_r = np.concatenate([names, r2, np.broadcast_to(np.frombuffer(b"\n+\n", np.uint8), (args.reads, 3)),
                         np.full((args.reads, 150), ord("I"), np.uint8), np.full((args.reads, 1), 10, np.uint8)], axis=1).tobytes()
del names
qs = workload.unpack(workload.make_protein_queries(db, args.queries))
text_p = b"".join(b">query_%05d some description of the query\n" % i + b"\n".join(s[j:j + 60] for j in range(0, len(s), 60)) + b"\n"
                  for i, s in enumerate(qs))
INPUTS = [("reads", "%d FASTQ reads of 150 nt" % args.reads, text_r, abi.READS, "fastq", args.reads, 64),
          ("proteins", "%d protein queries, 60-column FASTA" % args.queries, text_p, abi.PROTEIN, "fasta", args.queries, max(len(s) for s in qs))]

print("inputs ready", file=sys.stderr, flush=True)
ix = api.Index.from_image(api.Image.from_proteins(packed=db, device=0), 0)
ix.attach_proteins(table)
ix.attach_subject_text(table)
naa = ix.align_info()["number_of_aa"]

say("# -aln TSV response rows on the device: the stage, the aligning text calls, the host route")
say()
say("`tools/tsv_aln_bench.py --reads %d --queries %d --db-proteins %d --rounds %d` on one MI355X; medians of the rounds, every round listed.  "
    "MaxResults %d, MinKMatch %d, MinKRatio %.2f, BLOSUM62 11 / 1, ExtractPositions off." % (args.reads, args.queries, args.db_proteins, args.rounds, K, MINK, RATIO))
say()
say("## 1. The stage alone")
say()
say("Device-resident, one stream, HIP events: the text parsed on the device, `kaamer_search_device` + `kaamer_topn_device` (\"search\"), "
    "`kaamer_topn_align_device` (\"align\"), `kaamer_tsv_aln_rows_device` (its five launches and the copy of the counts: \"rows\").")
say()
say("| input | annotations | rows | bytes | search | align | rows | rows/s |")
say("|---|---|---|---|---|---|---|---|")
stream = torch.cuda.Stream()
for key, what, text, st, fmt, n_rec, max_qlen in INPUTS:
    parser = api.TextParser(len(text), max_records=n_rec + 16, max_lines=text.count(b"\n") + 16)
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        pr = parser.parse_device(d_text.data_ptr(), len(text), stream=stream.cuda_stream, fmt=fmt)
        ws = api.Workspace(ix, int(pr.seq_bytes) + 4096, n_rec + 16, seq_type=st)
        max_rows = min(ws.query_capacity * K, 4 * n_rec + 4096)
        stage = api.TsvStage(ix, ws.query_capacity, max_rows)
        cap = max_rows * 256
        d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        for ann in (0, 1):
            ms = ([], [], [])
            for it in range(args.rounds + 2):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                e[0].record(stream)
                dr = ws.search_device(pr.d_seqs, pr.d_offsets, int(pr.n_records), int(pr.seq_bytes), seq_type=st, stream=stream.cuda_stream)
                top = ws.topn_device(RATIO, MINK, K, best_start_codon=(st != abi.PROTEIN), stream=stream.cuda_stream)
                e[1].record(stream)
                alns = ws.topn_align_device(top, max_query_len=max_qlen, max_pairs=max_rows, stream=stream.cuda_stream)
                e[2].record(stream)
                rin = abi.TsvRowsIn()
                rin.top = top
                rin.d_q, rin.d_n_queries, rin.n_queries_cap = dr.d_q, dr.d_n_queries, dr.n_queries_cap
                rin.n_names, rin.d_name_bytes, rin.name_bytes_len, rin.d_spans = int(pr.n_records), d_text.data_ptr(), len(text), pr.d_spans
                rin.pos, rin.extract_positions, rin.annotations = None, 0, ann
                res = stage.aln_rows_device(rin, alns, d_out.data_ptr(), cap, seq_type=st, stream=stream.cuda_stream)
                e[3].record(stream)
                ws.finish(stream.cuda_stream)
                try:
                    n_rows, n_bytes = stage.finish(stream.cuda_stream)
                except abi.KaamerError as err:
                    if err.code != abi.E_RANGE:
                        raise
                    # a raw score outside the stage's table: show the records before giving up
                    nq = int(home(dr.d_n_queries, 1, np.uint32)[0])
                    n_pairs = int(home(alns.d_pair_off, nq + 1, np.uint64)[nq])
                    pairs = home(alns.d_pairs, n_pairs, api.PAIR_DTYPE)
                    bad = np.nonzero((pairs["status"] == 0) & ((pairs["raw"] < 0) | (pairs["raw"] >= stage.aln_info()["table"])))[0]
                    print("%s: %d queries, %d pairs, %d outside the table; the first: %s" % (key, nq, n_pairs, len(bad), pairs[bad[:8]]), file=sys.stderr)
                    raise
                if it >= 2:
                    for k in range(3):
                        ms[k].append(e[k].elapsed_time(e[k + 1]))
            m = med(ms[2])
            say("| %s | %s | %d | %d | %.3f ms (rounds: %s) | %.3f ms (rounds: %s) | %.3f ms (rounds: %s) | %.0f M |"
                % (key, "on" if ann else "off", n_rows, n_bytes, med(ms[0]), rounds(ms[0]), med(ms[1]), rounds(ms[1]), m, rounds(ms[2]),
                   n_rows / m / 1e3))
        stage.close()
        del d_out
        ws.close()
    parser.close()
    del d_text
say()

# ---- 2. the host-buffer call ----------------------------------------------------------------------------------------
L = abi.lib()
MATRIX = b"blosum62"


def call(fn, *a):
    o = C.POINTER(abi.BatchTop)()
    abi.check(fn(*a, C.byref(o)))
    return o


def route_host(text, st, fmt, ann, keep=None):
    """what a caller has without the aligning text calls: the host reader, the packed aligning call, the host formatter"""
    h = C.c_void_p()
    abi.check((L.kaamer_parse_fastq if fmt == "fastq" else L.kaamer_parse_fasta)(text, len(text), C.byref(h)))
    n = L.kaamer_reads_count(h)
    noff = np.ctypeslib.as_array(L.kaamer_reads_name_offsets(h), shape=(n + 1,))
    spans = np.zeros(n, api.SPAN_DTYPE)
    spans["name_off"], spans["name_len"] = noff[:-1], np.diff(noff)
    o = call(L.kaamer_search_batch_top_aln_flat, ix._h, C.cast(L.kaamer_reads_seqs(h), C.c_void_p), C.cast(L.kaamer_reads_offsets(h), C.c_void_p), n, st,
             RATIO, MINK, K, 0, MATRIX, 11, 1, 0)
    names = C.cast(L.kaamer_reads_names(h), C.c_void_p)
    need = L.kaamer_format_tsv_aln(o, names, int(noff[n]), spans.ctypes.data, n, table._h, st, 0, ann, None, 0, None)
    assert need >= 0
    b = C.create_string_buffer(need + 1)
    assert L.kaamer_format_tsv_aln(o, names, int(noff[n]), spans.ctypes.data, n, table._h, st, 0, ann, b, need + 1, None) == need
    if keep is not None:
        keep.append(b.raw[:need])
    L.kaamer_batch_top_free(o)
    L.kaamer_reads_free(h)


def route_device(text, st, fmt, ann, keep=None):
    o = call(L.kaamer_search_text_top_aln_tsv_flat, ix._h, text, len(text), 1, st, RATIO, MINK, K, 0, ann, MATRIX, 11, 1) if fmt == "fastq" else \
        call(L.kaamer_search_fasta_top_aln_tsv_flat, ix._h, text, len(text), st, 0, RATIO, MINK, K, 0, ann, MATRIX, 11, 1)
    if keep is not None:
        vp, vn, vo = C.c_void_p(), C.c_uint64(), C.POINTER(C.c_uint64)()
        abi.check(L.kaamer_batch_top_tsv(o, C.byref(vp), C.byref(vn), C.byref(vo)))
        keep.append(C.string_at(vp.value, vn.value))
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


say("## 2. The host-buffer call")
say()
say("Wall time of the calls in ms; four callers = four threads, one call each on the same text, at once; the two routes alternate within every "
    "round.  (host) the route a caller has without the aligning text calls: `kaamer_parse_fastq` / `kaamer_parse_fasta` on the host, "
    "`kaamer_search_batch_top_aln_flat` (numbers only), `kaamer_format_tsv_aln` into a buffer of the needed size on the caller's thread (two passes: "
    "the length, then the bytes).  (device) `kaamer_search_text_top_aln_tsv_flat` / `kaamer_search_fasta_top_aln_tsv_flat`.  The rows of the two "
    "routes were compared byte for byte on every input before anything was timed; batches the host printed inside the device route: %s.")
say()
say("| input | annotations | callers | (host) | (device) | (host) / (device) |")
say("|---|---|---|---|---|---|")
for key, what, text, st, fmt, n_rec, max_qlen in INPUTS:
    for ann in (0, 1):
        ka, kb = [], []
        route_host(text, st, fmt, ann, ka)
        route_device(text, st, fmt, ann, kb)
        assert ka[0] == kb[0] and len(ka[0]) > 0, "the two routes differ"
        del ka, kb
        for n in (1, 4):
            for fn in (route_host, route_device):
                callers(fn, n, text, st, fmt, ann)   # warm-up: slots, bounds, staging
            t = {route_host: [], route_device: []}
            for it in range(args.rounds):
                for fn in (route_host, route_device):
                    t[fn].append(callers(fn, n, text, st, fmt, ann) * 1e3)
            a, b = med(t[route_host]), med(t[route_device])
            say("| %s | %s | %d | %.2f (rounds: %s) | %.2f (rounds: %s) | %.2f |"
                % (key, "on" if ann else "off", n, a, rounds(t[route_host], "%.2f"), b, rounds(t[route_device], "%.2f"), a / b))
out[:] = [line.replace("inside the device route: %s.", "inside the device route: %d." % ix.tsv_aln_info()["host_batches"]) for line in out]
say()
ix.close()
if args.resources and os.path.exists(args.resources):
    with open(args.resources) as f:
        for line in f.read().rstrip().split("\n"):
            say(line)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(out) + "\n")
