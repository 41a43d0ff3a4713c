"""Open, use and close everything that owns device memory, six times over in one process: an index with the protein table
and the subject text attached, one call of every kind that allocates on first use or regrows (full search, top-N at
K = 5 then K = 50, with positions, with alignments, a text call, a TSV call, the split count-stream path of a workspace),
and a two-shard ShardedIndex with one top call with positions and alignments.  Every result of cycles 2..6 equals the
first cycle's byte for byte, and the device's free memory after each of them is not below its value after cycle 1 by
more than MARGIN.

MARGIN: the largest drift of the commit before the owning buffer type over the same cycles, plus one allocation granule
as mem_get_info steps on the MI355X: 23068672 bytes + 2 MiB.  Measured there: free memory after cycles 2..6 of that
commit was 12582912, 16777216, 18874368, 20971520 and 23068672 bytes below its value after cycle 1 (the runtime's own
per-cycle state: two torch streams, the slots' streams and events), and this commit gave the same six figures;
mem_get_info moves in steps of 2097152 bytes."""
import numpy as np
import pytest

from kaamer_amd import abi, api, workload

pytestmark = pytest.mark.gpu

CYCLES = 6
DRIFT_BEFORE = 23068672     # bytes: the parent commit's largest drop below cycle 1 over cycles 2..6
GRANULE = 2 << 20           # bytes: the step of mem_get_info for one small allocation
MARGIN = DRIFT_BEFORE + GRANULE
FIELDS = ("rep_query", "meta", "trim", "top_off", "top_pid", "top_kmatch", "top_first_pos", "orf_aa")
KW = dict(min_k_ratio=0.0, min_k_match=1)


def make_inputs():
    db = workload.make_db(300)
    seqs = workload.unpack(db)
    rows = [b"EntryID\tSequence\tOrganism\tEC"]
    for i, s in enumerate(seqs):
        rows.append(b"\t".join([b"sp|P%05d|X%d_TEST" % (i, i % 7), s, b"Organism number %d" % (i % 11), b"1.2.%d.-" % i]))
    table = api.Proteins.from_tsv(b"\n".join(rows) + b"\n")
    prot = workload.unpack(workload.make_protein_queries(db, 8, seed=31))
    reads = workload.unpack(workload.make_reads(db, 8, seed=33))
    fastq = b"".join(b"@read/%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))
    return dict(table=table, prot=prot, reads=reads, fastq=fastq)


@pytest.fixture(scope="module")
def inputs(klib):
    return make_inputs()


def _top(r):
    """everything a TopResult carries, as comparable values"""
    out = {f: getattr(r, f).tobytes() for f in FIELDS}
    out["shape"] = (r.n_queries, r.n_reported, r.max_results)
    for f in ("pos_bits_len", "pos_off", "pos_bits", "text_spans", "tsv_line_off"):
        v = getattr(r, f)
        out[f] = None if v is None else v.tobytes()
    out["tsv"] = r.tsv
    out["alignments"] = None if r.alignments is None else repr(r.alignments)
    return out


def _full(r):
    """a full result: the queries, and per query its hits as a set (the order inside a hit list is the counting tables',
    like the reference's map order: not part of the result), sorted by protein id"""
    out = {f: getattr(r, f).tobytes() for f in ("meta", "hit_cnt", "orf_aa", "starts_alt")}
    out["hits"] = []
    for q in range(r.n_queries):
        a, b = r.span(q)
        order = np.argsort(r.hit_pid[a:b], kind="stable")
        out["hits"].append(tuple(x[a:b][order].tobytes() for x in (r.hit_pid, r.hit_kmatch, r.hit_first_pos)))
    return out


def _dev(ptr, n, dtype):
    from test_gpu_protein import _from_ptr
    return _from_ptr(ptr, n, dtype).tobytes()


def _split_path(ix, seqs):
    """a workspace of its own with the counting stage on a count stream: search, top-N, its positions"""
    import torch
    buf, offs = api.pack_sequences(seqs)
    d_buf = torch.from_numpy(buf).cuda()
    d_off = torch.from_numpy(offs.view(np.int64)).cuda()
    torch.cuda.synchronize()
    own, cnt_stream = torch.cuda.Stream(), torch.cuda.Stream()
    n = len(seqs)
    ws = api.Workspace(ix, len(buf), n, first_pos=1)
    ws.set_count_stream(cnt_stream.cuda_stream)
    st = own.cuda_stream
    ws.search_device(d_buf.data_ptr(), d_off.data_ptr(), n, len(buf), stream=st)
    t = ws.topn_device(0.0, 1, 10, stream=st)
    r = ws.topn_positions_device(t, stream=st)
    ws.finish(st)
    base = np.frombuffer(_dev(r.d_pos_base, n + 1, np.uint64), np.uint64)
    cnt = np.frombuffer(_dev(t.d_top_cnt, n, np.uint32), np.uint32)
    kept = (np.arange(10)[None, :] < cnt[:, None]).ravel()   # (the rows of the result arrays are defined up to top_cnt)
    pid, km = (np.frombuffer(_dev(p, n * 10, np.uint32), np.uint32)[kept].tobytes() for p in (t.d_top_pid, t.d_top_kmatch))
    out = dict(cnt=cnt.tobytes(), pid=pid, km=km, base=base.tobytes(), blen=_dev(r.d_pos_bits_len, n, np.int32),
               bits=_dev(r.d_pos_bits, int(base[n]), np.uint64))
    ws.close()
    del d_buf, d_off
    return out


def cycle(s, gpu_device):
    """one cycle -> {call: its result}"""
    table, prot, reads, fastq = s["table"], s["prot"], s["reads"], s["fastq"]
    out = {}
    ix = api.Index.from_image(table.image(), gpu_device)
    ix.attach_proteins(table)
    ix.attach_subject_text(table)
    out["full protein"] = _full(ix.search(prot))
    out["full reads"] = _full(ix.search(reads, seq_type=abi.READS))
    out["top 5"] = _top(ix.search_top(prot, max_results=5, **KW))
    out["top 50"] = _top(ix.search_top(prot, max_results=50, **KW))     # (the result arrays of the slot's workspace regrow)
    out["top reads"] = _top(ix.search_top(reads, seq_type=abi.READS, max_results=10, **KW))
    out["top pos"] = _top(ix.search_top(prot, max_results=10, want_positions=True, **KW))
    out["top pos reads"] = _top(ix.search_top(reads, seq_type=abi.READS, max_results=10, want_positions=True, **KW))
    out["top aln"] = _top(ix.search_top(prot, max_results=10, align=dict(), **KW))
    out["text"] = _top(ix.search_text_top(fastq, seq_type=abi.READS, max_results=10, **KW))
    out["tsv"] = _top(ix.search_text_top(fastq, seq_type=abi.READS, max_results=10, tsv=dict(positions=True, annotations=True), **KW))
    out["split"] = _split_path(ix, prot)
    sx = api.ShardedIndex.from_images([table.image(shard=r, n_shards=2, device=gpu_device) for r in range(2)], [gpu_device] * 2)
    sx.attach_proteins(table)
    out["sharded pos aln"] = _top(sx.search_top(prot, max_results=10, want_positions=True, align=dict(), **KW))
    out["sharded pos aln reads"] = _top(sx.search_top(reads, seq_type=abi.READS, max_results=10, want_positions=True, align=dict(), **KW))
    sx.close()
    ix.close()
    return out


def free_bytes(gpu_device):
    import gc
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return int(torch.cuda.mem_get_info(gpu_device)[0])


def run_cycles(s, gpu_device, n=CYCLES):
    """-> (the results of every cycle, free device memory after every cycle)"""
    results, free = [], []
    for _ in range(n):
        results.append(cycle(s, gpu_device))
        free.append(free_bytes(gpu_device))
    return results, free


def test_six_cycles_same_results_no_drift(inputs, gpu_device):
    results, free = run_cycles(inputs, gpu_device)
    first = results[0]
    assert first["top 5"]["shape"][1] > 0 and first["top reads"]["shape"][1] > 0 and first["top aln"]["alignments"] not in (None, "[]")
    assert first["tsv"]["tsv"] and first["sharded pos aln"]["pos_bits"] and first["split"]["bits"]
    for c, r in enumerate(results[1:], 2):
        assert sorted(r) == sorted(first)
        for call in first:
            assert r[call] == first[call], "cycle %d: the result of '%s' differs from the first cycle's" % (c, call)
    print("free device memory after cycles 1..%d: %s; largest drop below cycle 1: %d bytes (margin %d)"
          % (CYCLES, free, max(free[0] - f for f in free[1:]), MARGIN))
    for c, f in enumerate(free[1:], 2):
        assert f >= free[0] - MARGIN, "free device memory after cycle %d is %d bytes below its value after cycle 1 (margin %d): %s" % (c, free[0] - f, MARGIN, free)
