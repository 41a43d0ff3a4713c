#!/usr/bin/env python3
"""What PositionHits for the reported hits costs on the one-process sharded handle (profiles/r07_sharded_top_positions.md).

    python tools/sharded_top_positions_bench.py --workload protein|reads --mode top|top_pos|full_pos --world W
                                                [--repeats N] [--warmup W] [--tree DIR]

  top       kaamer_sharded_search_batch_top_flat                     (no bitmaps; runs on older commits too)
  top_pos   kaamer_sharded_search_batch_top_pos_flat                 (bitmaps of the reported hits; one more round trip)
  full_pos  kaamer_sharded_search_batch_flat(want_positions = 1)     (bitmaps of every hit through the exchange)
All W shards sit on device 0.  The batch is BASELINE configs[1] (10 000 protein queries against DB-SP) or a configs[2]
batch (1 M reads of 150 nt).  Every call is timed on its own, copies and host work included (the C call only: no numpy
copies); one process per line: prints one JSON line with the median, the extremes, the bytes the call brought back and,
for top_pos, kaamer_sharded_positions_info.  --tree: the checkout whose kaamer_amd (and built library) is measured, for
the parent / head comparison of `top`.  Informational (never bench.py's `value`)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--workload", choices=["protein", "reads"], default="protein")
ap.add_argument("--mode", choices=["top", "top_pos", "full_pos"], default="top")
ap.add_argument("--world", type=int, default=2)
ap.add_argument("--queries", type=int, default=0)
ap.add_argument("--db-proteins", type=int, default=560000)
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()

sys.path.insert(0, os.path.abspath(args.tree))
import numpy as np
import torch  # noqa: F401  (one HIP runtime for the library)

from kaamer_amd import abi, api, workload

L = abi.lib()
W = args.world
db = workload.make_db(args.db_proteins)
sx = api.ShardedIndex.from_images([api.Image.from_proteins(packed=db, shard=r, n_shards=W) for r in range(W)], [0] * W)
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
    fn = L.kaamer_sharded_search_batch_top_pos_flat if pos else L.kaamer_sharded_search_batch_top_flat
    t0 = time.perf_counter()
    abi.check(fn(sx._h, buf.ctypes.data, offs.ctypes.data, len(offs) - 1, seq_type, RATIO, MINK, MAXR, C.byref(out)))
    dt = time.perf_counter() - t0
    o = out.contents
    r = o.n_reported
    ne = int(o.top_off[r])
    n_aa = 0
    if reads and r:   # the reported ORFs' residues (every owner's orf_aa section)
        meta = np.ctypeslib.as_array(C.cast(o.q, C.POINTER(C.c_uint8)), shape=(r * C.sizeof(abi.QueryMeta),)).view(api.META_DTYPE)
        n_aa = int(meta["aa_len"].sum(dtype=np.int64))
    # the owners' packed blocks (topn.hip.inc): W headers, the sections of all reported queries
    nbytes = 256 * W + align8(4 * r) * 2 + align8(40 * r) + 8 * (r + W) + 3 * align8(4 * ne) + align8(n_aa)
    extra = dict(n_reported=r, n_entries=ne, orf_aa_bytes=n_aa)
    if pos:
        po, pb = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        abi.check(L.kaamer_batch_top_positions(out, None, C.byref(po), C.byref(pb)))
        nw = int(po[ne])
        nbytes += align8(4 * r) + 8 * (ne + W) + 8 * nw
        extra["pos_words"] = nw
        extra["positions_info"] = sx.positions_info()
    L.kaamer_batch_top_free(out)
    return dt, nbytes, extra


def run_full():
    out = C.POINTER(abi.BatchOut)()
    t0 = time.perf_counter()
    abi.check(L.kaamer_sharded_search_batch_flat(sx._h, buf.ctypes.data, offs.ctypes.data, len(offs) - 1, seq_type, 1, C.byref(out)))
    dt = time.perf_counter() - t0
    res = api.BatchResult(out)
    nq, nh = res.n_queries, int(res.hit_off[res.n_queries])
    nbytes = nq * (40 + 8 + 4) + nh * (12 + 8) + res.pos_bits.nbytes + res.orf_aa.nbytes + res.starts_alt.nbytes
    extra = dict(n_queries=nq, n_hits=nh, pos_words=int(res.pos_bits.size))
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
print(json.dumps(dict(workload=args.workload, mode=args.mode, world=W, queries=n, repeats=args.repeats, warmup=args.warmup,
                      call_ms_median=round(statistics.median(ts), 3), call_ms_min=round(min(ts), 3), call_ms_max=round(max(ts), 3),
                      d2h_bytes=int(last[0]), exchange_info=sx.exchange_info(), **last[1])))
sx.close()
