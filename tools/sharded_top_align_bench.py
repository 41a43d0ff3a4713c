#!/usr/bin/env python3
"""What `-aln` in one call costs on the one-process sharded handle (profiles/r10_sharded_top_align.md).

    python tools/sharded_top_align_bench.py --workload protein|reads --worlds 1,2,8 [--max-results K] [--rounds N]
                                            [--db-proteins P] [--queries Q]

  new        kaamer_sharded_search_batch_top_aln_flat (top-N, the subject exchange and the alignment, one block per owner)
  parent     the route a sharded handle had before: kaamer_sharded_search_batch_top_flat + kaamer_fetch_hits + packing on
             the host (numpy: every distinct sequence once) + kaamer_align_pairs
  unsharded  kaamer_search_batch_top_aln_flat on an index of the whole database with the whole table attached
alternating `rounds` times in one process, all W shards on device 0, one JSON line per W.  Beside the wall times: the
HIP-event times of the gather, assemble and alignment stages of the last call (kaamer_sharded_index_set_align_timing; the
slowest device's), the bytes of an ids block and of a subject segment as they travelled (W x W of each per call), the
payload (the stored lengths of the reported pairs' subjects, summed), the table's bytes and the largest device's share.
Informational (never bench.py's `value`)."""
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
ap.add_argument("--worlds", default="1,2,8")
ap.add_argument("--queries", type=int, default=0)
ap.add_argument("--db-proteins", type=int, default=560000)
ap.add_argument("--max-results", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--text", type=int, default=1)
args = ap.parse_args()

L = abi.lib()
db = workload.make_db(args.db_proteins)
recs = workload.unpack(db)
prot = api.Proteins.from_fasta(b"".join(b">sp|P%07d|N\n%s\n" % (i, s) for i, s in enumerate(recs)))
del recs
ix = api.Index.from_image(prot.image(device=0), 0)
ix.attach_proteins(prot)
n_aa = prot.stats()["NumberOfAA"]
reads = args.workload == "reads"
n = args.queries or (1_000_000 if reads else 10_000)
buf, offs = workload.make_reads(db, n, seed=workload.SEED + 2) if reads else workload.make_protein_queries(db, n, seed=workload.SEED + 1)
buf = np.ascontiguousarray(buf, dtype=np.uint8)
offs = np.ascontiguousarray(offs, dtype=np.uint64)
seq_type = abi.READS if reads else abi.PROTEIN
RATIO, MINK, K = 0.05, 10, args.max_results
ALN = (b"blosum62", 11, 1, args.text)
sx = None


def one_call(fn, handle):
    out = C.POINTER(abi.BatchTop)()
    t0 = time.perf_counter()
    abi.check(fn(handle, buf.ctypes.data, offs.ctypes.data, len(offs) - 1, seq_type, RATIO, MINK, K, 0, *ALN, C.byref(out)))
    dt = time.perf_counter() - t0
    o = out.contents
    r = o.n_reported
    ne = int(o.top_off[r])
    pid = np.ctypeslib.as_array(o.top_pid, shape=(ne,)).copy() if ne else np.zeros(0, np.uint32)
    L.kaamer_batch_top_free(out)
    return dt, r, pid


def parent_call():
    t0 = time.perf_counter()
    out = C.POINTER(abi.BatchTop)()
    abi.check(L.kaamer_sharded_search_batch_top_flat(sx._h, buf.ctypes.data, offs.ctypes.data, len(offs) - 1, seq_type, RATIO, MINK, K, C.byref(out)))
    o = out.contents
    r = o.n_reported
    ne = int(o.top_off[r])
    top_off = np.ctypeslib.as_array(o.top_off, shape=(r + 1,)).astype(np.int64)
    pid = np.ctypeslib.as_array(o.top_pid, shape=(ne,)).copy() if ne else np.zeros(0, np.uint32)
    meta = np.ctypeslib.as_array(C.cast(o.q, C.POINTER(C.c_uint8)), shape=(r * C.sizeof(abi.QueryMeta),)).copy().view(api.META_DTYPE)
    src = np.ctypeslib.as_array(o.orf_aa, shape=(int((meta["aa_off"] + meta["aa_len"]).max()),)).copy() if reads and r else buf
    L.kaamer_batch_top_free(out)
    t1 = time.perf_counter()
    uniq, inv = np.unique(pid, return_inverse=True)
    ent = (abi.ProteinEntry * max(1, len(uniq)))()
    abi.check(L.kaamer_fetch_hits(prot._h, uniq.ctypes.data, len(uniq), ent))
    qlen, qoff = meta["aa_len"].astype(np.int64), meta["aa_off"].astype(np.int64)
    slen = np.array([ent[i].sequence_len for i in range(len(uniq))], dtype=np.int64)
    lens = np.concatenate([qlen, slen])
    poffs = np.zeros(len(lens) + 1, np.uint64)
    poffs[1:] = np.cumsum(lens)
    pbuf = np.empty(int(poffs[-1]), np.uint8)
    idx = workload._gather_index(qoff, qlen) if r else np.zeros(0, np.int64)
    pbuf[:int(qlen.sum())] = src[idx]
    at = int(qlen.sum())
    for i in range(len(uniq)):
        ln = int(slen[i])
        C.memmove(pbuf.ctypes.data + at, ent[i].sequence, ln)
        at += ln
    pq = np.repeat(np.arange(r, dtype=np.uint32), np.diff(top_off)).astype(np.uint32)
    ps = (inv + r).astype(np.uint32)
    t2 = time.perf_counter()
    h = C.c_void_p()
    abi.check(L.kaamer_align_pairs(0, pbuf.ctypes.data, poffs.ctypes.data, len(poffs) - 1, pq.ctypes.data, ps.ctypes.data, len(pq), n_aa,
                                   b"blosum62", 11, 1, C.byref(h)))
    L.kaamer_alignments_free(h)
    t3 = time.perf_counter()
    payload = int(slen[inv].sum()) if ne else 0
    return t3 - t0, dict(search_ms=(t1 - t0) * 1e3, fetch_pack_ms=(t2 - t1) * 1e3, align_pairs_ms=(t3 - t2) * 1e3), payload


new = lambda: one_call(L.kaamer_sharded_search_batch_top_aln_flat, sx._h)
uns = lambda: one_call(L.kaamer_search_batch_top_aln_flat, ix._h)
med = lambda v: round(statistics.median(v), 3)
for W in [int(w) for w in args.worlds.split(",")]:
    sx = api.ShardedIndex.from_images([prot.image(shard=r, n_shards=W, device=0) for r in range(W)], [0] * W)
    sx.attach_proteins(prot)
    sx.set_align_timing(True)
    for _ in range(2):
        new(); parent_call(); uns()
    new_ms, par_ms, uns_ms, parts, payload, r, pid = [], [], [], None, 0, 0, None
    for _ in range(args.rounds):
        dt, r, pid = new()
        new_ms.append(dt * 1e3)
        dt, parts, payload = parent_call()
        par_ms.append(dt * 1e3)
        uns_ms.append(uns()[0] * 1e3)
    new()   # (the info calls describe the last ALIGNING call on the set)
    info, stage = sx.align_info(), sx.align_stage_info()
    print(json.dumps(dict(workload=args.workload, world=W, queries=n, db_proteins=args.db_proteins, max_results=K, rounds=args.rounds,
                          text=args.text, reported=r, pairs=int(len(pid)), new_ms=[round(x, 3) for x in new_ms],
                          parent_ms=[round(x, 3) for x in par_ms], unsharded_ms=[round(x, 3) for x in uns_ms], new_ms_median=med(new_ms),
                          parent_ms_median=med(par_ms), unsharded_ms_median=med(uns_ms),
                          parent_parts={k: round(v, 3) for k, v in parts.items()},
                          gather_event_ms=stage["gather_us"] / 1e3, assemble_event_ms=stage["assemble_us"] / 1e3,
                          align_event_ms=stage["align_us"] / 1e3, waves=stage["waves"], long_waves=stage["long_waves"],
                          ids_block_bytes=stage["ids_block_bytes"], ids_blocks_travelled_bytes=stage["ids_block_bytes"] * W * W,
                          segment_bytes=info["segment_bytes"], segments_travelled_bytes=info["segment_bytes"] * W * W,
                          largest_segment_need_bytes=info["need_bytes"], subjects_payload_bytes=payload, attempts=info["attempts"],
                          table_bytes=info["table_bytes"], largest_share=info["largest_share"],
                          unsharded_table_bytes=ix.align_info()["table_bytes"])), flush=True)
    sx.close()
