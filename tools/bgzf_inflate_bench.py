#!/usr/bin/env python3
"""What inflating BGZF on the device costs and buys (profiles/r16_bgzf_inflate.md).

    python tools/bgzf_inflate_bench.py [--reads N] [--db-proteins P] [--rounds R] [--out FILE] [--resources FILE]

On one MI355X, text_parse_bench.py's read set (reads of 150 nt as FASTQ text, workload.fastq_text) written as BGZF -- blocks of
65 280 bytes of text, as bgzip cuts them -- at zlib levels 1 and 6:
  1. the inflate alone: HIP-event time of kaamer_inflate_bgzf_device per N reads, GB/s of text out and of compressed bytes
     in, next to the parse and the search of the same reads and to single-thread zlib on the same box;
  2. the host-buffer calls: kaamer_search_bgzf_top_flat against host gzip inflate + kaamer_search_text_top_flat on the same
     bytes, one caller and four;
  3. the file driver: kaamer_search_text_file_opts on the M-read BGZF file (level 6), device_inflate 1 against 0 (0 is the
     parent commit's code path), rounds alternating, and the plain file of the same reads beside them.
Every round is listed, nothing gates.  --resources: a file with the kernels' -Rpass-analysis=kernel-resource-usage remarks,
appended as it is."""
import argparse
import ctypes as C
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
ap.add_argument("--db-proteins", type=int, default=560000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--file-reads", type=int, default=10_000_000)
ap.add_argument("--chunk-text-bytes", type=int, default=64 << 20)
ap.add_argument("--block-bytes", type=int, default=65280)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r16_bgzf_inflate.md"))
ap.add_argument("--resources", default=None)
args = ap.parse_args()

L = abi.lib()
RATIO, MINK, K = 0.05, 10, 10
PARSE_MS_PER_M, SEARCH_MS_PER_M = 0.91, 6.3   # profiles/r15_text_parse.md: the device parse and the search of 1 M reads
out = []


def say(line=""):
    print(line, flush=True)
    out.append(line)


def med(xs):
    return statistics.median(xs)


def rounds(xs, scale=1.0, fmt="%.2f"):
    return ", ".join(fmt % (x * scale) for x in xs)


def bgzf(text, level):
    """the text as bgzip writes it: one member per block_bytes of text, then the empty end-of-file block"""
    parts = []
    for i in list(range(0, len(text), args.block_bytes)) + [len(text)]:
        piece = text[i:i + args.block_bytes] if i < len(text) else b""
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        payload = c.compress(piece) + c.flush()
        bsize = 18 + len(payload) + 8 - 1
        parts.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + bsize.to_bytes(2, "little") + payload +
                     zlib.crc32(piece).to_bytes(4, "little") + len(piece).to_bytes(4, "little"))
    return b"".join(parts)


def host_inflate(data):
    """every member of a gzip stream, one zlib thread (what the byte source of the file drivers does)"""
    parts, z, view = [], zlib.decompressobj(16 + zlib.MAX_WBITS), memoryview(data)
    for at in range(0, len(data), 1 << 20):   # 1 MiB at a time, as a file is read
        raw = view[at:at + (1 << 20)]
        while len(raw):
            parts.append(z.decompress(raw))
            raw = b""
            if z.eof:
                raw, z = z.unused_data, zlib.decompressobj(16 + zlib.MAX_WBITS)
    return b"".join(parts)


db = workload.make_db(args.db_proteins)
reads = workload.make_reads(db, args.reads, seed=workload.SEED + 2)
text = bytes(workload.fastq_text(reads))
per_m = 1e6 / args.reads
files = {level: bgzf(text, level) for level in (1, 6)}
say("# BGZF inflated on the device: the inflate alone, the host-buffer call")
say()
say("`tools/bgzf_inflate_bench.py --reads %d --db-proteins %d --rounds %d --block-bytes %d` on one MI355X.  %d reads of 150 nt: %d bytes of "
    "FASTQ text; as BGZF in blocks of %d bytes of text: %d bytes at level 1, %d bytes at level 6 (%d blocks)."
    % (args.reads, args.db_proteins, args.rounds, args.block_bytes, args.reads, len(text), args.block_bytes, len(files[1]), len(files[6]),
       len(api.bgzf_scan(files[6])[0])))
say()

# ---- 1. the inflate alone -----------------------------------------------------------------------------------------
say("## 1. The inflate alone")
say()
say("HIP events around the launches of `kaamer_inflate_bgzf_device` (offsets, blocks, status reduce, first bad status) and its result copy; compressed bytes and "
    "block table resident in HBM, every status word 0 and the text compared with the input once.  zlib: `zlib.decompressobj` over the same "
    "bytes, one thread, same box.")
say()
say("| level | time per %d reads | text out | compressed in | zlib, one thread | zlib / device |" % args.reads)
say("|---|---|---|---|---|---|")
st = torch.cuda.Stream()
for level in (1, 6):
    data = files[level]
    blocks, used = api.bgzf_scan(data)
    assert used == len(data)
    inf = api.Inflater(len(data), len(blocks))
    d_comp = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    d_blocks = torch.frombuffer(bytearray(blocks.tobytes()), dtype=torch.uint8).cuda()
    d_out = torch.empty(len(text) + 64, dtype=torch.uint8, device="cuda")
    res = abi.InflateResult()
    ms = []
    with torch.cuda.stream(st):
        for it in range(args.rounds + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            abi.check(L.kaamer_inflate_bgzf_device(inf._h, d_comp.data_ptr(), len(data), d_blocks.data_ptr(), len(blocks), d_out.data_ptr(), len(text), st.cuda_stream))
            e1.record(st)
            abi.check(L.kaamer_inflater_finish(inf._h, st.cuda_stream, C.byref(res)))
            if it >= 2:
                ms.append(e0.elapsed_time(e1))
    assert res.n_bad == 0 and res.out_bytes == len(text)
    assert d_out[:len(text)].cpu().numpy().tobytes() == text
    zs = []
    for it in range(2):
        t0 = time.perf_counter()
        assert len(host_inflate(data)) == len(text)
        zs.append(time.perf_counter() - t0)
    m = med(ms)
    say("| %d | %.2f ms = %.2f ms per 1 M reads (rounds: %s) | %.1f GB/s | %.1f GB/s | %.0f ms (rounds: %s) | %.0fx |"
        % (level, m, m * per_m, rounds(ms), len(text) / m / 1e6, len(data) / m / 1e6, med(zs) * 1e3, rounds(zs, 1e3, "%.0f"), med(zs) * 1e3 / m))
    inf.close()
    del d_comp, d_blocks, d_out
say()
say("Beside it, per 1 M reads: the device parse %.2f ms and the search %.1f ms (profiles/r15_text_parse.md, same reads, same database)."
    % (PARSE_MS_PER_M, SEARCH_MS_PER_M))
say()

# ---- 2. the host-buffer calls ---------------------------------------------------------------------------------------
img = api.Image.from_proteins(packed=db, device=0)
ix = api.Index.from_image(img, 0)


def bgzf_route(data):
    o = C.POINTER(abi.BatchTop)()
    abi.check(L.kaamer_search_bgzf_top_flat(ix._h, data, len(data), abi.READS, RATIO, MINK, K, C.byref(o)))
    n = o.contents.n_reported
    L.kaamer_batch_top_free(o)
    return n


def host_route(data):
    t = host_inflate(data)
    o = C.POINTER(abi.BatchTop)()
    abi.check(L.kaamer_search_text_top_flat(ix._h, t, len(t), 1, abi.READS, RATIO, MINK, K, C.byref(o)))
    n = o.contents.n_reported
    L.kaamer_batch_top_free(o)
    return n


def callers(fn, data, n):
    """n threads, one call each on the same bytes (ctypes and zlib release the GIL): wall time of all"""
    th = [threading.Thread(target=fn, args=(data,)) for _ in range(n)]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    return time.perf_counter() - t0


say("## 2. The host-buffer calls")
say()
say("`kaamer_search_bgzf_top_flat` (compressed bytes up, inflate + parse + search on the device, text and result back) against host inflate "
    "(zlib, in the caller's thread) + `kaamer_search_text_top_flat` on the same %d-read BGZF bytes, database of %d proteins, wall time of "
    "the calls; four callers = four threads, one call each, at once.  Rounds alternate between the two routes." % (args.reads, args.db_proteins))
say()
say("| level | callers | device inflate | host inflate | host / device | every device round faster than every host round |")
say("|---|---|---|---|---|---|")
for level in (1, 6):
    data = files[level]
    assert bgzf_route(data) == host_route(data) > 0
    for n in (1, 4):
        callers(bgzf_route, data, n)   # warm-up: slots, bounds, staging
        callers(host_route, data, n)
        a, b = [], []
        for it in range(args.rounds):
            a.append(callers(bgzf_route, data, n))
            b.append(callers(host_route, data, n))
        say("| %d | %d | %.0f ms = %.0f ms per 1 M reads (rounds: %s) | %.0f ms = %.0f ms per 1 M reads (rounds: %s) | %.2f | %s |"
            % (level, n, med(a) * 1e3, med(a) * 1e3 * per_m / n, rounds(a, 1e3, "%.0f"), med(b) * 1e3, med(b) * 1e3 * per_m / n,
               rounds(b, 1e3, "%.0f"), med(b) / med(a), "yes" if max(a) < min(b) else "NO"))
say()
ix.close()

# ---- 3. the file driver ---------------------------------------------------------------------------------------------
n_rep = max(1, args.file_reads // args.reads)
file_reads = n_rep * args.reads
tmpd = tempfile.mkdtemp(prefix="bgzf_inflate_bench_")
plain, gz = os.path.join(tmpd, "q.fastq"), os.path.join(tmpd, "q.fastq.gz")
body = files[6][:-28]   # without the end-of-file block, which goes once at the file's end
with open(plain, "wb") as f, open(gz, "wb") as g:
    for _ in range(n_rep):
        f.write(text)
        g.write(body)
    g.write(files[6][-28:])
for p in (plain, gz):   # into the page cache
    with open(p, "rb") as f:
        while f.read(1 << 26):
            pass
NOOP = api.Replicas.TEXT_CHUNK_CB(lambda user, first, t, n, spans, nr, top: 0)
reps = api.Replicas.from_image(img, [0])
seen = {}


def run_file(p, flag):
    c = abi.Counters()
    t0 = time.perf_counter()
    abi.check(L.kaamer_search_text_file_opts(reps._h, p.encode(), 1, abi.READS, RATIO, MINK, K, args.chunk_text_bytes, 3, flag, C.cast(NOOP, C.c_void_p), None,
                                             C.byref(c)))
    seen[(p, flag)] = c.n_queries
    return time.perf_counter() - t0


say("## 3. The file driver")
say()
say("`kaamer_search_text_file_opts` on a BGZF file of %d reads (%d bytes of text, %d bytes compressed, level 6, blocks of %d bytes of text), in the page "
    "cache, one replica, in_flight 3, chunks of %d bytes of text, a callback that does nothing.  `device_inflate` 0 is the parent commit's code "
    "path (zlib on the host thread).  Rounds alternate." % (file_reads, len(text) * n_rep, len(body) * n_rep + 28, args.block_bytes, args.chunk_text_bytes))
say()
for p, flag in ((gz, 1), (gz, 0), (plain, 0)):   # warm-up: slots, bounds, staging
    run_file(p, flag)
assert seen[(gz, 1)] == seen[(gz, 0)] == seen[(plain, 0)] > 0, seen
on, off, pl = [], [], []
for it in range(args.rounds):
    on.append(run_file(gz, 1))
    off.append(run_file(gz, 0))
    pl.append(run_file(plain, 0))
say("| file | device_inflate | reads/s | rounds (s) |")
say("|---|---|---|---|")
say("| BGZF | 1 | %.2f M | %s |" % (file_reads / med(on) / 1e6, rounds(on)))
say("| BGZF | 0 | %.2f M | %s |" % (file_reads / med(off) / 1e6, rounds(off)))
say("| plain | - | %.2f M | %s |" % (file_reads / med(pl) / 1e6, rounds(pl)))
say()
say("Flag on against flag off: %.2fx (medians); every flag-on round faster than every flag-off round: %s.  Against the plain file: %.2f of its rate."
    % (med(off) / med(on), "yes" if max(on) < min(off) else "NO", med(pl) / med(on)))
say()
reps.close()
os.unlink(plain)
os.unlink(gz)
os.rmdir(tmpd)
if args.resources and os.path.exists(args.resources):
    say("## Kernel resources")
    say()
    say("`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage` on `inflate.hip.inc`'s kernels:")
    say()
    say("```")
    with open(args.resources) as f:
        for line in f.read().rstrip().split("\n"):
            say(line)
    say("```")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(out) + "\n")
