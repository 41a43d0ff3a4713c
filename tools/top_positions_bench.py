#!/usr/bin/env python3
"""What PositionHits for the reported hits costs on the host-buffer calls (profiles/r06_top_positions.md).

    python tools/top_positions_bench.py --workload protein|reads --mode top|top_pos|full_pos [--repeats N] [--warmup W]

  top       kaamer_search_batch_top_flat                       (no bitmaps; runs on older commits too)
  top_pos   kaamer_search_batch_top_pos_flat                   (bitmaps of the reported hits in the packed block)
  full_pos  kaamer_search_batch_flat(want_positions = 1)       (bitmaps of every hit), then kaamer_sort_hits +
            kaamer_filter_results per query on the host: the only way to the same information without top_pos
The batch is BASELINE configs[1] (10 000 protein queries against DB-SP) or a configs[2] batch (1 M reads).  Every call is
timed on its own, PCIe and host work included (the C call only: no numpy copies); prints one JSON line with the median,
the extremes and the bytes the call brought back.  Informational (never bench.py's `value`)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401  (one HIP runtime for the library)

from kaamer_amd import abi, api, workload

ap = argparse.ArgumentParser()
ap.add_argument("--workload", choices=["protein", "reads"], default="protein")
ap.add_argument("--mode", choices=["top", "top_pos", "full_pos"], default="top")
ap.add_argument("--queries", type=int, default=0)
ap.add_argument("--db-proteins", type=int, default=560000)
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()

L = abi.lib()
db = workload.make_db(args.db_proteins)
ix = api.Index.from_proteins(packed=db, device=0)
reads = args.workload == "reads"
n = args.queries or (1_000_000 if reads else 10_000)
buf, offs = workload.make_reads(db, n, seed=workload.SEED + 2) if reads else workload.make_protein_queries(db, n, seed=workload.SEED + 1)
buf = np.ascontiguousarray(buf, dtype=np.uint8)
offs = np.ascontiguousarray(offs, dtype=np.uint64)
seq_type = abi.READS if reads else abi.PROTEIN
RATIO, MINK, MAXR = 0.05, 10, 10


def align8(x):
    return (x + 7) & ~7


def run_top(pos):
    out = C.POINTER(abi.BatchTop)()
    fn = L.kaamer_search_batch_top_pos_flat if pos else L.kaamer_search_batch_top_flat
    t0 = time.perf_counter()
    abi.check(fn(ix._h, buf.ctypes.data, offs.ctypes.data, len(offs) - 1, seq_type, RATIO, MINK, MAXR, C.byref(out)))
    dt = time.perf_counter() - t0
    o = out.contents
    r = o.n_reported
    ne = int(o.top_off[r])
    n_aa = int(sum(o.q[i].aa_len for i in range(r))) if reads and r < 200000 else 0
    # the packed block: header, rep_query, trim, q, top_off, pid / kmatch / first_pos, ORF residues (topn.hip.inc)
    nbytes = 256 + align8(4 * r) * 2 + align8(40 * r) + 8 * (r + 1) + 3 * align8(4 * ne) + align8(n_aa)
    extra = dict(n_reported=r, n_entries=ne, host_ms=0.0)
    if pos:
        po, pb = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        abi.check(L.kaamer_batch_top_positions(out, None, C.byref(po), C.byref(pb)))
        nw = int(po[ne])
        nbytes += align8(4 * r) + 8 * (ne + 1) + 8 * nw
        extra["pos_words"] = nw
    L.kaamer_batch_top_free(out)
    return dt, nbytes, extra


def run_full():
    out = C.POINTER(abi.BatchOut)()
    t0 = time.perf_counter()
    abi.check(L.kaamer_search_batch_flat(ix._h, buf.ctypes.data, offs.ctypes.data, len(offs) - 1, seq_type, 1, C.byref(out)))
    dt = time.perf_counter() - t0
    res = api.BatchResult(out)
    nq, nh = res.n_queries, int(res.hit_off[res.n_queries])
    nbytes = nq * (40 + 8 + 4) + nh * (12 + 8) + res.pos_bits.nbytes + res.orf_aa.nbytes + res.starts_alt.nbytes
    # sortMapByValue + FilterResults on the host, per query (SetBestStartCodon of a reads batch is NOT included)
    t1 = time.perf_counter()
    order = np.empty(int(res.hit_cnt.max()) if nq else 0, np.uint32)
    kept = 0
    pid, km, sizes = res.hit_pid, res.hit_kmatch, res.meta["size_in_kmer"]
    for q in np.nonzero(res.hit_cnt)[0].tolist():
        a, c = int(res.hit_off[q]), int(res.hit_cnt[q])
        L.kaamer_sort_hits(pid[a:a + c].ctypes.data, km[a:a + c].ctypes.data, c, order.ctypes.data)
        ks = np.ascontiguousarray(km[a:a + c][order[:c]])
        kept += L.kaamer_filter_results(ks.ctypes.data, c, int(sizes[q]), RATIO, MINK, MAXR)
    host = time.perf_counter() - t1
    extra = dict(n_queries=nq, n_hits=nh, pos_words=int(res.pos_bits.size), kept=int(kept), host_ms=host * 1e3)
    res.close()
    return dt, nbytes, extra


run = {"top": lambda: run_top(False), "top_pos": lambda: run_top(True), "full_pos": run_full}[args.mode]
for _ in range(args.warmup):
    run()
ts, last = [], None
for _ in range(args.repeats):
    dt, nbytes, extra = run()
    ts.append(dt * 1e3)
    last = (nbytes, extra)
print(json.dumps(dict(workload=args.workload, mode=args.mode, queries=n, repeats=args.repeats, warmup=args.warmup,
                      call_ms_median=round(statistics.median(ts), 3), call_ms_min=round(min(ts), 3), call_ms_max=round(max(ts), 3),
                      d2h_bytes=int(last[0]), **last[1])))
