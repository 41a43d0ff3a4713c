#!/usr/bin/env python3
"""What the whole-file drivers cost next to the per-chunk calls they wrap (profiles/r11_search_file.md).

    python tools/search_file_bench.py [--reads N] [--db-proteins P] [--worlds 1,3] [--chunk-seqs C] [--rounds R]

A plain FASTQ file of N reads of 150 nt (in the page cache: it is written, then read once, before anything is timed) is
searched on DB-SP as the other tools build it, MaxResults 10:
  (a) kaamer_search_file, one replica, in_flight 3: the driver as it was;
  (b) kaamer_search_file_opts, one replica, in_flight 3: plain, with positions, with positions + alignments (text);
  (c) kaamer_sharded_search_file at each W of --worlds (all shards on device 0), in_flight 3, the same three kinds;
  (d) the same chunks, parsed beforehand, from memory through the one-call submit / wait forms with three tickets in flight:
      what a caller could already do without the drivers.
The callbacks do nothing.  One JSON line per (handle, kind): reads/s of the driver and of (d), their ratio, and the time
of the reader alone over the file (what the driver adds in front of the queue).  Informational (never bench.py's `value`)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401  (one HIP runtime for the library)

from kaamer_amd import abi, api, workload

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--db-proteins", type=int, default=560000)
ap.add_argument("--worlds", default="1,3")
ap.add_argument("--chunk-seqs", type=int, default=100000)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--kinds", default="plain,pos,aln")
args = ap.parse_args()

L = abi.lib()
RATIO, MINK, K, IN_FLIGHT = 0.05, 10, 10, 3
KINDS = {"plain": (0, 0), "pos": (1, 0), "aln": (1, 1)}   # (want_positions, want_aln)
db = workload.make_db(args.db_proteins)
recs = workload.unpack(db)
prot = api.Proteins.from_fasta(b"".join(b">sp|P%07d|N\n%s\n" % (i, s) for i, s in enumerate(recs)))
del recs
img = prot.image(device=0)
reps = api.Replicas.from_image(img, [0])
reps.attach_proteins(prot)
ix_h = L.kaamer_replicas_index(reps._h, 0)
reads = workload.make_reads(db, args.reads, seed=workload.SEED + 2)
tmp = tempfile.NamedTemporaryFile(suffix=".fastq", delete=False)
tmp.write(workload.fastq_text(reads))
tmp.close()
path = tmp.name.encode()
with open(tmp.name, "rb") as f:   # into the page cache
    while f.read(1 << 26):
        pass

# the reader alone, and the chunks of (d)
t0 = time.perf_counter()
rd = api.Reader(tmp.name, "fastq")
chunks = []
while True:
    c = rd.next(args.chunk_seqs, 1 << 40)
    if c is None:
        break
    chunks.append((np.ascontiguousarray(c[0]), np.ascontiguousarray(c[1])))
rd.close()
reader_with_copies_s = time.perf_counter() - t0
t0 = time.perf_counter()
rd = api.Reader(tmp.name, "fastq")
while True:
    h = rd.next_handle(args.chunk_seqs, 1 << 40)
    if h is None:
        break
    L.kaamer_reads_free(h)
rd.close()
reader_s = time.perf_counter() - t0
assert sum(len(o) - 1 for _, o in chunks) == args.reads

NOOP = api.Replicas.CHUNK_CB(lambda user, first, chunk, top: 0)
CB = C.cast(NOOP, C.c_void_p)


def file_run(fn, handle, kind):
    pos, aln = KINDS[kind]
    c = abi.Counters()
    t0 = time.perf_counter()
    if fn is L.kaamer_search_file:
        rc = fn(handle, path, 1, 0, abi.READS, RATIO, MINK, K, args.chunk_seqs, 1 << 40, IN_FLIGHT, CB, None, C.byref(c))
    else:
        rc = fn(handle, path, 1, 0, abi.READS, RATIO, MINK, K, pos, aln, b"blosum62", 11, 1, 1, args.chunk_seqs, 1 << 40, IN_FLIGHT, CB, None,
                C.byref(c))
    abi.check(rc)
    assert c.n_in > 0
    return time.perf_counter() - t0


def memory_run(handle, sharded, kind):
    """(d): three tickets in flight over the parsed chunks"""
    pos, aln = KINDS[kind]
    pre = "kaamer_sharded_" if sharded else "kaamer_"
    wait = getattr(L, pre + "wait_batch_top")
    t0 = time.perf_counter()
    fifo = []

    def pop():
        out = C.POINTER(abi.BatchTop)()
        abi.check(wait(fifo.pop(0), C.byref(out)))
        L.kaamer_batch_top_free(out)
    for buf, offs in chunks:
        if len(fifo) == IN_FLIGHT:
            pop()
        t = C.c_void_p()
        head = (handle, buf.ctypes.data, offs.ctypes.data, len(offs) - 1, abi.READS, RATIO, MINK, K)
        if aln:
            abi.check(getattr(L, pre + "submit_batch_top_aln_flat")(*(head + (pos, b"blosum62", 11, 1, 1, C.byref(t)))))
        elif pos:
            abi.check(getattr(L, pre + "submit_batch_top_pos_flat")(*(head + (C.byref(t),))))
        else:
            abi.check(getattr(L, pre + "submit_batch_top_flat")(*(head + (C.byref(t),))))
        fifo.append(t)
    while fifo:
        pop()
    return time.perf_counter() - t0


def report(name, W, kind, drv, mem):
    d, m = statistics.median(drv), statistics.median(mem)
    print(json.dumps(dict(driver=name, world=W, kind=kind, reads=args.reads, chunk_seqs=args.chunk_seqs, chunks=len(chunks), in_flight=IN_FLIGHT,
                          db_proteins=args.db_proteins, rounds=args.rounds, driver_s=[round(x, 4) for x in drv], memory_s=[round(x, 4) for x in mem],
                          driver_reads_per_s=round(args.reads / d), memory_reads_per_s=round(args.reads / m), driver_over_memory=round(d / m, 3),
                          reader_alone_s=round(reader_s, 4), reader_with_copies_s=round(reader_with_copies_s, 4))), flush=True)


def measure(name, W, fn, handle, mem_handle, sharded, kinds):
    for kind in kinds:
        file_run(fn, handle, kind)
        memory_run(mem_handle, sharded, kind)   # (warm-up: slots, bounds)
        drv, mem = [], []
        for _ in range(args.rounds):            # alternating
            drv.append(file_run(fn, handle, kind))
            mem.append(memory_run(mem_handle, sharded, kind))
        report(name, W, kind, drv, mem)


kinds = [k for k in args.kinds.split(",") if k in KINDS]
measure("kaamer_search_file", 0, L.kaamer_search_file, reps._h, ix_h, False, ["plain"])
measure("kaamer_search_file_opts", 0, L.kaamer_search_file_opts, reps._h, ix_h, False, kinds)
for W in [int(w) for w in args.worlds.split(",") if w]:
    sx = api.ShardedIndex.from_images([prot.image(shard=r, n_shards=W, device=0) for r in range(W)], [0] * W)
    sx.attach_proteins(prot)
    measure("kaamer_sharded_search_file", W, L.kaamer_sharded_search_file, sx._h, sx._h, True, kinds)
    sx.close()
os.unlink(tmp.name)
