"""What a request's genetic code costs in the 6-frame translation: the same batch of reads (default 1 M of 150 nt, DB-SP
sized database) through the device-resident call under code 11 (translate_reads_kernel<192, false>: table 11 compiled in)
and under another code (default 4: <192, true>, table and class masks from the call's parameters).

Times come from the workspace's HIP events (kaamer_workspace_set_timing): per call the whole search, the probe kernel and
the counting kernels.  The last figure printed is a DIFFERENCE, whole call minus probe minus count: all translation kernels,
the ORFs' prep, the table layout and the finalize step together -- NOT translate_reads_kernel alone (the library records no
event pair around that launch).  The two codes produce different ORFs, so their ORF and residue counts are printed beside the
times.  For the kernel alone run this script in a run of its own under
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/gcode_translate_timing.py --reps 5`: the two
instantiations show up as separate kernels in DIR's kernel_stats.csv.

    python tools/gcode_translate_timing.py [--reads N] [--proteins N] [--codes 11,4] [--reps K]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from kaamer_amd import abi, api, workload  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--proteins", type=int, default=20000)
ap.add_argument("--codes", default="11,4")
ap.add_argument("--reps", type=int, default=10)
a = ap.parse_args()

db = workload.make_db(a.proteins, seed=3)
ix = api.Index.from_image(api.Image.from_proteins(packed=db), 0)
buf, offs = workload.make_reads(db, a.reads, seed=9)
n = len(offs) - 1
d_buf, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(offs.view(np.int64)).cuda()
ws = api.Workspace(ix, len(buf), n, seq_type=abi.READS)
st = torch.cuda.current_stream().cuda_stream
codes = [int(c) for c in a.codes.split(",")]
for rnd in range(2):                       # the codes alternate: A B A B on one device
    for code in codes:
        t = abi.seq_type(abi.READS, code)
        ws.set_timing(0)
        for _ in range(2):
            ws.search_device(d_buf.data_ptr(), d_off.data_ptr(), n, len(buf), seq_type=t, stream=st)
        c = ws.finish(st)
        ws.set_timing(1)
        ws.reset_timers()
        for _ in range(a.reps):
            ws.search_device(d_buf.data_ptr(), d_off.data_ptr(), n, len(buf), seq_type=t, stream=st)
        c = ws.finish(st)
        tm = ws.kernel_ms_sum()
        k = tm["calls"]
        residues = c["n_lookup"] + 6 * c["n_queries"]   # upper figure: SizeInKmer + 6 per ORF (one less for an ORF closed by a stop)
        print("code %2d round %d: %d reads -> %d ORFs, %d k-mer lookups (<= %d residues); per call: total %.3f ms, probe %.3f, count %.3f, "
              "rest by difference (translation + prep + layout + finalize) %.3f ms" % (code, rnd, n, c["n_queries"], c["n_lookup"], residues, tm["total_ms"] / k,
                                                                  tm["probe_ms"] / k, tm["count_ms"] / k,
                                                                  (tm["total_ms"] - tm["probe_ms"] - tm["count_ms"]) / k), flush=True)
ws.close()
