#!/usr/bin/env python3
"""What `-aln` costs in one call against the route it replaces (profiles/r09_top_align.md).

    python tools/top_align_bench.py --workload protein|reads [--max-results K] [--rounds N] [--db-proteins P] [--queries Q]

  new     kaamer_search_batch_top_aln_flat (top-N + the alignment of the reported hits, one packed block), one call at a
          time, and three tickets in flight (kaamer_submit_batch_top_aln_flat / kaamer_wait_batch_top)
  parent  kaamer_search_batch_top_flat + kaamer_fetch_hits + packing on the host (numpy: every distinct sequence once)
          + kaamer_align_pairs
alternating new / parent `rounds` times in one process on one card.  Beside the wall times: the HIP-event time of the
new alignment stage alone (kaamer_topn_align_device behind kaamer_topn_device) with its cells, the bytes that cross PCIe
each way, the grid and slab the budget produced.  Prints one JSON line.  Informational (never bench.py's `value`)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from kaamer_amd import abi, api, workload

ap = argparse.ArgumentParser()
ap.add_argument("--workload", choices=["protein", "reads"], default="protein")
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


def new_call():
    out = C.POINTER(abi.BatchTop)()
    t0 = time.perf_counter()
    abi.check(L.kaamer_search_batch_top_aln_flat(ix._h, buf.ctypes.data, offs.ctypes.data, len(offs) - 1, seq_type, RATIO, MINK, K, 0,
                                                 *ALN, C.byref(out)))
    dt = time.perf_counter() - t0
    o = out.contents
    ne = int(o.top_off[o.n_reported])
    items = C.POINTER(abi.Alignment)()
    abi.check(L.kaamer_batch_top_alignments(out, C.byref(items), None))
    ops = sum(items[e].length for e in range(ne)) if ne < 400000 else -1
    L.kaamer_batch_top_free(out)
    return dt, ne, ops


def new_three():
    t0 = time.perf_counter()
    tk = []
    for _ in range(3):
        t = C.c_void_p()
        abi.check(L.kaamer_submit_batch_top_aln_flat(ix._h, buf.ctypes.data, offs.ctypes.data, len(offs) - 1, seq_type, RATIO, MINK, K, 0,
                                                     *ALN, C.byref(t)))
        tk.append(t)
    for t in tk:
        out = C.POINTER(abi.BatchTop)()
        abi.check(L.kaamer_wait_batch_top(t, C.byref(out)))
        L.kaamer_batch_top_free(out)
    return (time.perf_counter() - t0) / 3


def parent_call():
    t0 = time.perf_counter()
    out = C.POINTER(abi.BatchTop)()
    abi.check(L.kaamer_search_batch_top_flat(ix._h, buf.ctypes.data, offs.ctypes.data, len(offs) - 1, seq_type, RATIO, MINK, K, C.byref(out)))
    o = out.contents
    r = o.n_reported
    ne = int(o.top_off[r])
    top_off = np.ctypeslib.as_array(o.top_off, shape=(r + 1,)).astype(np.int64)
    pid = np.ctypeslib.as_array(o.top_pid, shape=(ne,)).copy() if ne else np.zeros(0, np.uint32)
    meta = np.ctypeslib.as_array(C.cast(o.q, C.POINTER(C.c_uint8)), shape=(r * C.sizeof(abi.QueryMeta),)).copy().view(api.META_DTYPE)
    src = np.ctypeslib.as_array(o.orf_aa, shape=(int((meta["aa_off"] + meta["aa_len"]).max()),)).copy() if reads and r else buf
    L.kaamer_batch_top_free(out)
    t1 = time.perf_counter()
    # FetchHitsInformation for the distinct ids, then every distinct sequence once into one packed buffer
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
    return t3 - t0, dict(search_ms=(t1 - t0) * 1e3, fetch_pack_ms=(t2 - t1) * 1e3, align_pairs_ms=(t3 - t2) * 1e3, h2d_bytes=int(pbuf.nbytes + poffs.nbytes + 8 * len(pq)))


def device_stage():
    """HIP-event time of the alignment stage alone (the same pairs as the host call's)"""
    d_buf = torch.from_numpy(buf).cuda()
    d_off = torch.from_numpy(offs.view(np.int64)).cuda()
    longest = int(np.diff(offs.astype(np.int64)).max())
    ws = api.Workspace(ix, len(buf), len(offs) - 1, seq_type=seq_type)
    st = torch.cuda.Stream()
    ms = []
    for it in range(4):
        with torch.cuda.stream(st):
            ws.search_device(d_buf.data_ptr(), d_off.data_ptr(), len(offs) - 1, len(buf), stream=st.cuda_stream)
            t = ws.topn_device(RATIO, MINK, K, best_start_codon=reads, stream=st.cuda_stream)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            r = ws.topn_align_device(t, max_query_len=(longest // 3 + 2) if reads else longest, stream=st.cuda_stream)
            e1.record(st)
        ctr = ws.finish(st.cuda_stream)
        ms.append(e0.elapsed_time(e1))
    # the cells of the stage: query_len x subject_len over the aligned pairs, from the pair records it left on the device
    hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    torch.cuda.synchronize()
    nq = int(ctr["n_queries"])   # (ORFs for nucleotide input)
    off = np.empty(nq + 1, np.uint64)
    assert hip.hipMemcpy(off.ctypes.data, C.c_void_p(r.d_pair_off), off.nbytes, 2) == 0
    npairs = int(off[nq])
    rec = np.empty((npairs, 16), np.uint32)
    if npairs:
        assert hip.hipMemcpy(rec.ctypes.data, C.c_void_p(r.d_pairs), rec.nbytes, 2) == 0
    ok = rec[:, 0] == 0
    ql, sl = rec[ok, 11].astype(np.int64), rec[ok, 15].astype(np.int64)
    cells = dict(aligned_pairs=int(ok.sum()), cells=int((ql * sl).sum()), long_subject_pairs=int((sl > 2048).sum()),
                 long_subject_cells=int((ql * sl)[sl > 2048].sum()), longest_pair_cells=int((ql * sl).max()) if ok.any() else 0)
    return ms, r, cells


for _ in range(2):
    new_call()
    parent_call()
new_ms, new3_ms, par_ms, parts = [], [], [], None
pairs = ops = 0
for _ in range(args.rounds):
    dt, pairs, ops = new_call()
    new_ms.append(dt * 1e3)
    dt, parts = parent_call()
    par_ms.append(dt * 1e3)
    new3_ms.append(new_three() * 1e3)
stage_ms, r, cells = device_stage()
info = ix.align_info()
med = lambda v: round(statistics.median(v), 3)
print(json.dumps(dict(workload=args.workload, queries=n, db_proteins=args.db_proteins, max_results=K, rounds=args.rounds, text=args.text,
                      pairs=pairs, new_ms=[round(x, 3) for x in new_ms], parent_ms=[round(x, 3) for x in par_ms],
                      new_three_in_flight_ms_per_batch=[round(x, 3) for x in new3_ms], new_ms_median=med(new_ms), parent_ms_median=med(par_ms),
                      new3_ms_median=med(new3_ms), parent_parts={k: round(v, 3) if isinstance(v, float) else v for k, v in parts.items()},
                      new_h2d_bytes=int(buf.nbytes + offs.nbytes), new_d2h_ops_bytes=ops, new_d2h_pair_bytes=64 * pairs,
                      align_stage_event_ms=[round(x, 3) for x in stage_ms[1:]], waves=int(r.n_waves), long_waves=int(r.n_long_waves),
                      slab_bytes=int(r.slab_bytes), stage_gcups=round(cells['cells'] / (statistics.median(stage_ms[1:]) * 1e6), 2), **cells, table_bytes=info["table_bytes"], budget_bytes=info["budget_bytes"])))
