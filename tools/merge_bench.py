#!/usr/bin/env python3
"""What a merge of two images costs next to the rebuild it replaces (profiles/r14_image_merge.md).

    python tools/merge_bench.py [--db-proteins P] [--rounds N] [--load L]

DB-SP of kaamer_amd.workload (560 000 proteins) is cut 1:1 and 99:1 into runs of consecutive proteins; the parts' images
are built on the device.  Per cut, alternating `rounds` times in one process on one card:

  merge    kaamer_image_merge_device over the two images (upload, expansion, the shared build, download)
  rebuild  kaamer_image_build_proteins_device over all proteins: the only other route to the same table
and once each the host forms (kaamer_image_merge, kaamer_image_build_proteins), for scale.  One further merge and one
further rebuild run under KAAMER_BUILD_TRACE; their per-stage laps are reported as they were printed.  The merged image's
counters are checked against the rebuild's.  Prints one JSON line.  Informational (never bench.py's `value`)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401  (one HIP runtime in the process)

from kaamer_amd import api, workload

ap = argparse.ArgumentParser()
ap.add_argument("--db-proteins", type=int, default=560000)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--load", type=float, default=0.5)
ap.add_argument("--host", type=int, default=1)
args = ap.parse_args()

COUNTERS = ("n_keys", "n_pairs", "n_buckets", "n_lists", "n_inline", "max_list", "arena_words", "max_protein_id", "n_displaced")
db = workload.make_db(args.db_proteins)
buf, offs = db
n = len(offs) - 1


def part(a, b):
    o = offs[a:b + 1]
    return (buf[int(o[0]):int(o[-1])].copy(), (o - o[0]).astype(np.uint64)), np.arange(a, b, dtype=np.uint32)


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def traced(f):
    """f() under KAAMER_BUILD_TRACE -> the laps the library printed on stderr"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["KAAMER_BUILD_TRACE"] = "1"
        try:
            f()
        finally:
            del os.environ["KAAMER_BUILD_TRACE"]
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        lines = tmp.read().decode("utf-8", "replace").splitlines()
    laps = []
    for l in lines:
        if l.startswith("[kaamer device build]") and " s " in l:
            what, rest = l[len("[kaamer device build]"):].rsplit(" s ", 1)
            name, sec = what.rsplit(None, 1)
            laps.append([name.strip(), float(sec), int(rest.strip(" ()"))])
    return laps


def rebuild():
    return api.Image.from_proteins(packed=db, load_factor=args.load, device=0)


out = {"db_proteins": n, "residues": int(offs[-1]), "load_factor": args.load, "rounds": args.rounds, "cuts": {}}
whole = rebuild()   # warm-up of the device, the allocator and rocPRIM's kernels
out["stats"] = {c: whole.stats()[c] for c in COUNTERS}
for name, at in (("1:1", n // 2), ("99:1", n * 99 // 100)):
    imgs = [api.Image.from_proteins(packed=p, ids=ids, load_factor=args.load, device=0) for p, ids in (part(0, at), part(at, n))]
    m = api.Image.merge(imgs, load_factor=args.load, device=0)   # warm-up
    assert {c: m.stats()[c] for c in COUNTERS} == out["stats"], (m.stats(), out["stats"])
    t_merge, t_rebuild = [], []
    for _ in range(args.rounds):
        t_merge.append(timed(lambda: api.Image.merge(imgs, load_factor=args.load, device=0))[0])
        t_rebuild.append(timed(rebuild)[0])
    cut = {"proteins": [at, n - at], "pairs": [im.stats()["n_pairs"] for im in imgs],
           "merge_device_s": {"median": statistics.median(t_merge), "min": min(t_merge), "all": t_merge},
           "rebuild_device_s": {"median": statistics.median(t_rebuild), "min": min(t_rebuild), "all": t_rebuild},
           "merge_laps": traced(lambda: api.Image.merge(imgs, load_factor=args.load, device=0)),
           "rebuild_laps": traced(rebuild)}
    if args.host:
        cut["merge_host_s"] = timed(lambda: api.Image.merge(imgs, load_factor=args.load))[0]
    out["cuts"][name] = cut
if args.host:
    out["rebuild_host_s"] = timed(lambda: api.Image.from_proteins(packed=db, load_factor=args.load))[0]
print(json.dumps(out))
