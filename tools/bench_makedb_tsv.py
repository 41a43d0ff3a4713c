#!/usr/bin/env python3
"""What reading a database TSV file on the device costs and buys (profiles/r24_makedb_tsv.md).

    python tools/bench_makedb_tsv.py [--proteins N] [--rounds R] [--device D] [--out FILE]

On one MI355X.  The input is DB-SP of the project's generator (workload.make_db) written as TSV: the columns EntryID,
ProteinName, Sequence; the same with eight more feature columns behind them (a quarter of those cells empty); and the three
columns with a quarter of the proteins.  On the same bytes, rounds alternating, every round listed:
  1. kaamer_makedb_tsv (host) against kaamer_makedb_tsv_device: wall time of the whole call, so upload, download and the
     assembly of the table are in it; the two tables are compared first;
  2. kaamer_makedb_tsv + kaamer_index_build_proteins against kaamer_index_build_tsv;
  3. the device reader's stages by HIP events (KAAMER_MAKEDB_TRACE), with bytes of text per second, and beside their sum the
     time a device-to-device copy of the same text takes: the ceiling of anything that reads the text once and writes it once.
Everything is reported; the bar the profile states (on every input the device route's median not above the host route's) is
printed as held or missed, nothing gates."""
import argparse
import ctypes as C
import os
import re
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from kaamer_amd import abi, api, workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--proteins", type=int, default=560_000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--device", type=int, default=0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_makedb_tsv.md"))
args = ap.parse_args()
assert args.rounds >= 5, "at least five rounds per route"
assert torch.cuda.is_available(), "this measurement needs the GPU: there is no fallback"

L = abi.lib()
out = []


def say(line=""):
    print(line, flush=True)
    out.append(line)


def rounds(xs, fmt="%.3f"):
    return ", ".join(fmt % x for x in xs)


def _place(text, at, pieces):
    """pieces[i] (bytes) to text[at[i] ...]"""
    lens = np.fromiter((len(p) for p in pieces), dtype=np.int64, count=len(pieces))
    src = np.frombuffer(b"".join(pieces), dtype=np.uint8)
    off = np.zeros(len(pieces), dtype=np.int64)
    np.cumsum(lens[:-1], out=off[1:])
    text[np.repeat(at - off, lens) + np.arange(len(src), dtype=np.int64)] = src


def tsv_of(db, extra):
    """packed proteins -> database TSV text: 'sp|P<i>|G<family>', 'protein <i> of family <f>', the sequence, and `extra` more
    feature cells per row (every fourth of them empty)"""
    buf, offs = db
    offs = offs.astype(np.int64)
    lens = offs[1:] - offs[:-1]
    n = len(lens)
    header = b"\t".join([b"EntryID", b"ProteinName", b"Sequence"] + [b"Feature%d" % k for k in range(extra)]) + b"\n"
    heads = [b"sp|P%07d|G%06d\tprotein %d of family %d\t" % (i, i // 10, i, i // 10) for i in range(n)]
    tails = [b"".join(b"\t" if (i + k) % 4 == 0 else b"\tvalue %d of %d" % (k, i % (k + 3)) for k in range(extra)) + b"\n" for i in range(n)]
    hl = np.fromiter((len(h) for h in heads), dtype=np.int64, count=n)
    tl = np.fromiter((len(t) for t in tails), dtype=np.int64, count=n)
    start = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(hl + lens + tl, out=start[1:])
    start += len(header)
    text = np.empty(int(start[-1]), dtype=np.uint8)
    text[:len(header)] = np.frombuffer(header, dtype=np.uint8)
    _place(text, start[:-1], heads)
    _place(text, start[:-1] + hl + lens, tails)
    j = np.arange(int(offs[-1]), dtype=np.int64) - np.repeat(offs[:-1], lens)
    text[np.repeat(start[:-1] + hl, lens) + j] = buf[:int(offs[-1])]
    return text.tobytes()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def host_table(text):
    return api.Proteins.from_tsv(text)


def device_table(text):
    return api.Proteins.from_tsv(text, device=args.device)


def host_index(text):
    """the route that was there before: the host reader's table, its arrays handed to the device builder as they lie"""
    p = api.Proteins.from_tsv(text)
    ptr = [C.cast(f(p._h), C.c_void_p) for f in (L.kaamer_proteins_seqs, L.kaamer_proteins_offsets, L.kaamer_proteins_ids)]
    ix = C.c_void_p()
    abi.check(L.kaamer_index_build_proteins(*ptr, len(p), 0, 1, 0.5, args.device, C.byref(ix)))
    return p, api.Index(ix, args.device)


def device_index(text):
    return api.Index.from_tsv_text(text, device=args.device)


def close(r):
    for x in (r if isinstance(r, tuple) else (r,)):
        x.close()


def trace_of(text):
    """the stage lines the library prints under KAAMER_MAKEDB_TRACE -> [(stage, ms)]"""
    os.environ["KAAMER_MAKEDB_TRACE"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            device_table(text).close()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["KAAMER_MAKEDB_TRACE"]
        f.seek(0)
        lines = f.read().decode("latin-1").splitlines()
    got = []
    for ln in lines:
        m = re.match(r"\[kaamer makedb tsv\] (.+?)\s+([0-9.]+) ms", ln)
        if m:
            got.append((m.group(1).strip(), float(m.group(2))))
    return got


def copy_ms(n_bytes, reps=20):
    a = torch.empty(n_bytes, dtype=torch.uint8, device="cuda:%d" % args.device)
    b = torch.empty_like(a)
    b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


say("# r24: the makedb TSV reader on the device")
say()
say("`tools/bench_makedb_tsv.py --proteins %d --rounds %d`, one %s; wall times in seconds of the whole call (host clock, the"
    % (args.proteins, args.rounds, torch.cuda.get_device_name(args.device)))
say("call ends synchronised), rounds alternating host / device after one warm-up of each, every round listed, `med` = median.")
say()
t0 = time.perf_counter()
db = workload.make_db(args.proteins)
q = args.proteins // 4
inputs = [("DB-SP, EntryID / ProteinName / Sequence", tsv_of(db, 0)),
          ("DB-SP, the same with eight more feature columns", tsv_of(db, 8)),
          ("a quarter of it, three columns", tsv_of((db[0], db[1][:q + 1]), 0))]
say("Inputs generated in %.1f s (workload.make_db, seed %d)." % (time.perf_counter() - t0, workload.SEED))
say()
held = True
for name, text in inputs:
    mb = len(text) / 1e6
    h, d = host_table(text), device_table(text)
    hs, ho = h.packed
    ds, do = d.packed
    with tempfile.TemporaryDirectory() as tmp:
        h.save(os.path.join(tmp, "h"))
        d.save(os.path.join(tmp, "d"))
        same_file = open(os.path.join(tmp, "h"), "rb").read() == open(os.path.join(tmp, "d"), "rb").read()
    same = (np.array_equal(h.ids, d.ids) and np.array_equal(ho, do) and np.array_equal(hs, ds) and h.stats() == d.stats()
            and h.feature_names == d.feature_names and h.fetch_hits(h.ids[:50]) == d.fetch_hits(h.ids[:50]) and same_file)
    n_acc, n_feat = len(h), len(h.feature_names)
    close((h, d))
    say("## %s: %.1f MB of text, %d lines, %d tabs, %d accepted rows, %d feature columns" % (name, mb, text.count(b"\n"), text.count(b"\t"), n_acc, n_feat))
    say()
    say("Device table equals the host table (ids, offsets, sequences, stats, feature names, 50 entries, the saved file): **%s**" % ("yes" if same else "NO"))
    say()
    for title, host_fn, dev_fn in (("table: `kaamer_makedb_tsv` / `kaamer_makedb_tsv_device`", host_table, device_table),
                                   ("index: `kaamer_makedb_tsv` + `kaamer_index_build_proteins` / `kaamer_index_build_tsv`", host_index, device_index)):
        wh, r = timed(lambda: host_fn(text))
        close(r)
        wd, r = timed(lambda: dev_fn(text))
        close(r)
        th, td = [], []
        for _ in range(args.rounds):
            t, r = timed(lambda: host_fn(text))
            close(r)
            th.append(t)
            t, r = timed(lambda: dev_fn(text))
            close(r)
            td.append(t)
        ok = statistics.median(td) <= statistics.median(th)
        held = held and ok
        say("- %s" % title)
        say("  - host route:   %s; med %.3f s (%.0f MB/s)" % (rounds(th), statistics.median(th), mb / statistics.median(th)))
        say("  - device route: %s; med %.3f s (%.0f MB/s)" % (rounds(td), statistics.median(td), mb / statistics.median(td)))
        say("  - warm-up calls (not counted): host %.3f, device %.3f" % (wh, wd))
        say("  - ratio of the medians %.1f x; device median not above the host median: %s; device not slower in any round: %s"
            % (statistics.median(th) / statistics.median(td), "yes" if ok else "NO", "yes" if all(b <= a for a, b in zip(th, td)) else "no"))
    trace_of(text)
    stages = trace_of(text)
    cp = copy_ms(len(text))
    kernels = [(s, ms) for s, ms in stages if s not in ("upload", "host table", "download")]
    say("- stages of one `kaamer_makedb_tsv_device` call by HIP events (second traced call):")
    say()
    say("  | stage | ms | GB/s of text |")
    say("  |---|---|---|")
    for s, ms in stages:
        say("  | %s | %.3f | %.1f |" % (s, ms, len(text) / ms * 1e-6 if ms > 0 else 0.0))
    ksum = sum(ms for _, ms in kernels)
    say("  | kernels, sum (without upload / host table / download) | %.3f | %.1f |" % (ksum, len(text) / ksum * 1e-6 if ksum else 0.0))
    say("  | device-to-device copy of the text (ceiling) | %.3f | %.1f |" % (cp, len(text) / cp * 1e-6))
    say()
say("## The bar")
say()
say("On every measured input the device route's median is not above the host route's: **%s**." % ("held" if held else "MISSED"))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(out) + "\n")
