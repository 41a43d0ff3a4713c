"""The post-step kernel (topn.hip.inc: topn_kernel<16> for ORFs, topn_kernel<64> for protein queries, rep_block_kernel) on
the crafted world of tests/topncases.py, against the CPU oracle's literal flow: the start-codon rule and its tie rule in the
cached and the re-scanning form, hit counts at the cache edges of both widths, the gate and the filter on the trimmed size,
four ORFs of one wave on different loops, the grid's second pass, and the rule behind the sharded merge.  Every comparison
is exact."""
import math

import numpy as np
import pytest

import topncases as T

pytestmark = pytest.mark.gpu


def _dev(ptr, n, dtype):
    from test_gpu_protein import _from_ptr
    return _from_ptr(ptr, n, dtype)


@pytest.fixture(scope="module")
def crafted(klib, oracle, gpu_device):
    """the crafted database on the device and in the oracle, and the oracle's view of every ORF of the crafted reads"""
    from kaamer_amd import api
    seqs, ids = T.world().database()
    ix = api.Index.from_image(api.Image.from_proteins(seqs, ids=ids), gpu_device)
    oix = oracle.Index.from_proteins(seqs, ids=ids)
    views = T.reference_orfs(oracle, oix, T.reads())
    return ix, oix, views


class _ReadsOnDevice:
    """a reads batch searched once in a workspace; topn(options) -> the arrays of kaamer_topn_result on the host"""

    def __init__(self, ix, read_list, n_hits):
        import torch
        from kaamer_amd import abi, api
        buf, offs = T.pack(read_list)
        self.d_buf = torch.from_numpy(buf).cuda()
        self.d_off = torch.from_numpy(offs.view(np.int64)).cuda()
        self.st = torch.cuda.current_stream().cuda_stream
        self.ws = api.Workspace(ix, len(buf), len(read_list), seq_type=abi.READS, max_hits=4 * n_hits + (1 << 16))
        self.ws.search_device(self.d_buf.data_ptr(), self.d_off.data_ptr(), len(read_list), len(buf), stream=self.st)

    def topn(self, ratio, mink, maxr):
        t = self.ws.topn_device(ratio, mink, maxr, best_start_codon=True, stream=self.st)
        nq = self.ws.finish(self.st)["n_queries"]
        two = lambda p: _dev(p, nq * maxr, np.uint32).reshape(nq, maxr)
        return dict(nq=nq, cnt=_dev(t.d_top_cnt, nq, np.uint32), pid=two(t.d_top_pid), km=two(t.d_top_kmatch), fp=two(t.d_top_first_pos),
                    trim=_dev(t.d_trim, nq, np.int32), sp=_dev(t.d_start_position, nq, np.int32), so=_dev(t.d_size_in_kmer, nq, np.int32))


def _check_orfs(views, a, opts):
    """every ORF of the batch against the reference's flow under the options"""
    assert a["nq"] == len(views)
    n_rep = n_trim = 0
    for qi, v in enumerate(views):
        f = v.flow(*opts)
        got = (int(a["cnt"][qi]), int(a["trim"][qi]), int(a["sp"][qi]), int(a["so"][qi]))
        if f is None:                                    # the reference returns before SetBestStartCodon: untrimmed
            assert got == (0, 0, v.start, v.size), (qi, opts, got)
            continue
        keep = f[0]
        assert got == f, (qi, opts, got, f)
        assert a["pid"][qi, :keep].tolist() == v.pid[:keep].tolist(), (qi, opts)
        assert a["km"][qi, :keep].tolist() == v.km[:keep].tolist(), (qi, opts)
        assert a["fp"][qi, :keep].tolist() == v.fp[:keep].tolist(), (qi, opts)
        n_rep += keep > 0
        n_trim += f[1] > 0
    return n_rep, n_trim


def test_start_codon_cases(crafted):
    ix, oix, views = crafted
    assert 0 in T.wave_mix_groups(views)                 # ORFs 0..3: re-scanned | cached | no hit | gated, one wave
    dev = _ReadsOnDevice(ix, T.reads(), sum(v.n for v in views))
    for opts in T.OPTS:
        n_rep, n_trim = _check_orfs(views, dev.topn(*opts), opts)
        assert n_rep >= (100 if opts[0] < 0.5 else 10) and n_trim >= 100, opts


def test_reported_block_of_the_cases(crafted):
    from kaamer_amd import abi
    ix, oix, views = crafted
    packed = T.pack(T.reads())
    for opts in ((0.0, 1, 1), (0.05, 10, 10), (0.6, 10, 10), (0.0, 1, 10), (0.0, 10, 65), (0.0, 1, 65)):
        top = ix.search_top(packed=packed, seq_type=abi.READS, min_k_ratio=opts[0], min_k_match=opts[1], max_results=opts[2])
        flows = [v.flow(*opts) for v in views]
        reported = [q for q, f in enumerate(flows) if f is not None and f[0] > 0]
        assert top.n_queries == len(views) and top.rep_query.tolist() == reported and len(reported) >= 100
        if opts[2] == 65:
            assert max(flows[q][0] for q in reported) == 65      # rep_block_kernel copies more than a wave's worth of hits
        at = 0
        for i, q in enumerate(reported):
            v, (keep, trim, sp, so) = views[q], flows[q]
            m = top.meta[i]
            assert int(top.trim[i]) == trim, (q, opts)
            assert (int(m["start_position"]), int(m["size_in_kmer"]), int(m["aa_len"])) == (sp, so, len(v.seq) - trim), (q, opts)
            assert (int(m["src_seq"]), int(m["end_position"]), bool(m["plus_strand"])) == (v.read_index, v.o["end"], v.plus), q
            assert (int(top.top_off[i]), int(top.top_off[i + 1])) == (at, at + keep), (q, opts)
            assert top.top_pid[at:at + keep].tolist() == v.pid[:keep].tolist(), (q, opts)
            assert top.top_kmatch[at:at + keep].tolist() == v.km[:keep].tolist(), (q, opts)
            assert top.top_first_pos[at:at + keep].tolist() == v.fp[:keep].tolist(), (q, opts)
            a0 = int(m["aa_off"])
            assert bytes(top.orf_aa[a0:a0 + int(m["aa_len"])]).decode("latin-1") == v.seq[trim:], (q, opts)
            at += keep


def test_ties_at_the_cache_boundaries(crafted, oracle):
    import torch
    from kaamer_amd import api
    ix, oix, views = crafted
    # ORFs (16 lanes, best_start_codon): 16 | 17 and 128 | 129 tied hits, in ascending id
    cases = T.orf_cases()
    tied = [(c, views.index(T.target_of(c, views, ri))) for ri, c in enumerate(cases) if c["name"].startswith("all hits tied")]
    assert sorted({c["n"] for c, _ in tied}) == list(T.ORF_TIE_COUNTS)
    dev = _ReadsOnDevice(ix, T.reads(), sum(v.n for v in views))
    for maxr in sorted({1, 10} | {n + d for n in T.ORF_TIE_COUNTS for d in (0, 1)}):
        a = dev.topn(0.0, 1, maxr)
        for c, qi in tied:
            keep = min(c["n"], maxr)
            assert int(a["cnt"][qi]) == keep and int(a["trim"][qi]) == c["trim"], (c["name"], maxr)
            assert a["pid"][qi, :keep].tolist() == c["ids"][:keep], (c["name"], maxr)
            assert set(a["km"][qi, :keep].tolist()) == {T.BEST}
    # protein queries (64 lanes, no start codon): 64 | 65 and 511 | 512 | 513 tied hits
    seqs = T.protein_queries()
    pcases = T.protein_cases()
    buf, offs = T.pack(seqs)
    d_buf = torch.from_numpy(buf).cuda()
    d_off = torch.from_numpy(offs.view(np.int64)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    exp = [oix.search(s) if oracle.size_in_kmer(s) >= 7 else None for s in seqs]
    ws = api.Workspace(ix, len(buf), len(seqs), max_hits=4 * sum(len(e[0]) for e in exp if e) + (1 << 16))
    ws.search_device(d_buf.data_ptr(), d_off.data_ptr(), len(seqs), len(buf), stream=st)
    for maxr in sorted({1, 10} | {n + d for n in T.PROTEIN_TIE_COUNTS for d in (0, 1)}):
        t = ws.topn_device(0.0, 1, maxr, stream=st)
        ws.finish(st)
        cnt = _dev(t.d_top_cnt, len(seqs), np.uint32)
        pid = _dev(t.d_top_pid, len(seqs) * maxr, np.uint32).reshape(len(seqs), maxr)
        km = _dev(t.d_top_kmatch, len(seqs) * maxr, np.uint32).reshape(len(seqs), maxr)
        for i, (s, e) in enumerate(zip(seqs, exp)):
            keep = oracle.filter_results(e[1], oracle.size_in_kmer(s), 0.0, 1, maxr) if e else 0
            assert int(cnt[i]) == keep, (i, maxr)
            if keep:
                assert pid[i, :keep].tolist() == e[0][:keep].tolist() and km[i, :keep].tolist() == e[1][:keep].tolist(), (i, maxr)
        for j, c in enumerate(pcases):                   # (the tied query is every third one)
            keep = min(c["n"], maxr)
            assert int(cnt[3 * j]) == keep and pid[3 * j, :keep].tolist() == c["ids"][:keep], (c["name"], maxr)


def test_second_pass_of_the_grid(crafted, oracle, gpu_device):
    """more ORFs than n_cu * 128 groups of 16 lanes, more protein queries than n_cu * 32 waves: a group serves a second query"""
    import torch
    from kaamer_amd import api
    ix, oix, views = crafted
    n_cu = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    rng = np.random.default_rng(77)
    crafted_reads = T.reads()
    by_read = {}
    for v in views:
        by_read.setdefault(v.read_index, []).append(v)
    n_random = math.ceil(n_cu * 128 / 4.0) + 200
    acgt = np.frombuffer(b"ACGT", np.uint8)
    random_reads = [bytes(r) for r in acgt[rng.integers(0, 4, (n_random, 150))]]
    random_views = T.reference_orfs(oracle, oix, random_reads)
    # the crafted reads at the front and at the very end, one more of them after every 64 random reads
    all_views = list(views)
    all_reads = list(crafted_reads)
    at = 0
    for b in range(0, n_random, 64):
        all_reads += random_reads[b:b + 64]
        while at < len(random_views) and random_views[at].read_index < b + 64:
            all_views.append(random_views[at])
            at += 1
        c = (b // 64) % len(crafted_reads)
        all_reads.append(crafted_reads[c])
        all_views += by_read.get(c, [])
    all_reads += crafted_reads
    all_views += views
    assert len(all_views) > n_cu * 128 + len(views)      # the copies at the end are served by a second pass
    dev = _ReadsOnDevice(ix, all_reads, sum(v.n for v in all_views))
    for opts in ((0.05, 10, 10), (0.0, 1, 3)):
        n_rep, _ = _check_orfs(all_views, dev.topn(*opts), opts)
        assert n_rep >= 300
    # protein queries
    db_seqs = [s for s in T.world().database()[0] if len(s) >= 13]
    letters = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    lens = rng.integers(13, 41, n_cu * 32 + 200)
    middle = []
    for i, n in enumerate(lens.tolist()):
        if i % 8 == 0:                                   # a piece of a database protein: a query with hits
            middle.append(db_seqs[int(rng.integers(0, len(db_seqs)))][:n])
        else:
            middle.append(bytes(letters[rng.integers(0, 20, n)]))
    seqs = T.protein_queries() + middle + T.protein_queries()
    assert len(seqs) > n_cu * 32 + len(T.protein_queries())
    buf, offs = T.pack(seqs)
    d_buf = torch.from_numpy(buf).cuda()
    d_off = torch.from_numpy(offs.view(np.int64)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    exp = [oix.search(s) if oracle.size_in_kmer(s) >= 7 else None for s in seqs]
    assert sum(1 for e in exp[len(T.protein_queries()):-len(T.protein_queries())] if e and len(e[0])) >= 500
    ws = api.Workspace(ix, len(buf), len(seqs), max_hits=4 * sum(len(e[0]) for e in exp if e) + (1 << 16))
    ws.search_device(d_buf.data_ptr(), d_off.data_ptr(), len(seqs), len(buf), stream=st)
    for (ratio, mink, maxr) in ((0.05, 10, 10), (0.0, 1, 513)):
        t = ws.topn_device(ratio, mink, maxr, stream=st)
        ws.finish(st)
        cnt = _dev(t.d_top_cnt, len(seqs), np.uint32)
        pid = _dev(t.d_top_pid, len(seqs) * maxr, np.uint32).reshape(len(seqs), maxr)
        km = _dev(t.d_top_kmatch, len(seqs) * maxr, np.uint32).reshape(len(seqs), maxr)
        size_out = _dev(t.d_size_in_kmer, len(seqs), np.int32)
        for i, (s, e) in enumerate(zip(seqs, exp)):
            size = oracle.size_in_kmer(s)
            assert int(size_out[i]) == size
            keep = oracle.filter_results(e[1], size, ratio, mink, maxr) if e and len(e[0]) else 0
            assert int(cnt[i]) == keep, (i, maxr)
            if keep:
                assert pid[i, :keep].tolist() == e[0][:keep].tolist() and km[i, :keep].tolist() == e[1][:keep].tolist(), (i, maxr)


def test_sharded_merge_keeps_the_rule(crafted, gpu_device):
    """three shards on the one device: a best hit's Kmatch is a sum over shards and its first position a minimum, and the
    tie rule and the trim come out as on the unsharded index"""
    from kaamer_amd import abi, api
    from test_gpu_top_positions import _same_hits
    ix, oix, views = crafted
    seqs, ids = T.world().database()
    packed = T.pack(T.reads())
    images = [api.Image.from_proteins(seqs, ids=ids, shard=r, n_shards=3) for r in range(3)]
    sx = api.ShardedIndex.from_images(images, [gpu_device] * 3)
    for (ratio, mink, maxr) in ((0.05, 10, 10), (0.0, 1, 3), (0.0, 1, 65)):
        ref = ix.search_top(packed=packed, seq_type=abi.READS, min_k_ratio=ratio, min_k_match=mink, max_results=maxr)
        top = sx.search_top(packed=packed, seq_type=abi.READS, min_k_ratio=ratio, min_k_match=mink, max_results=maxr)
        assert ref.n_reported >= 100 and int((ref.trim > 0).sum()) >= 100
        _same_hits(top, ref)
        assert bytes(top.orf_aa) == bytes(ref.orf_aa)
    sx.close()
    # a tied best hit whose k-mers lie on two shards
    parts = [api.Index.from_image(im, gpu_device).search(packed=packed, seq_type=abi.READS) for im in images]
    n_split = 0
    for ri, c in enumerate(T.orf_cases()):
        if c["n_best"] < 2:
            continue
        qi = views.index(T.target_of(c, views, ri))
        hits = [p.hits(qi) for p in parts]
        for pid in views[qi].pid[:c["n_best"]].tolist():
            per_shard = [h[pid] for h in hits if pid in h]
            assert sum(per_shard) == int(views[qi].km[0]), (c["name"], pid)
            n_split += len(per_shard) >= 2
    assert n_split >= 1
