"""scan_u32_on (search.hip) through every caller the device-resident API exposes, on both sides of the bound that picks
its form: one workgroup that walks the tiles with a carry (scan_single_kernel) while the bound is at most
kaamer_scan_geometry's single_max, three tiled launches above it.  What the bound is differs by caller: the batch's
sequence count (CSR compaction, PositionHits layout), the workspace's query capacity (the top-N family, the reported-hit
block), the piece bound of a nucleotide batch (the translate step).  Every offset array is compared with numpy's cumulative
sum of the counts it was made from, every hit list with the CPU oracle's.

One tiny database and a pool of about 500 distinct short queries, half of them windows of database records (guaranteed
hits), half random (mostly misses); the oracle is asked once per pool entry, a batch indexes into the pool.  The queries on
either side of every tile edge and the last one are guaranteed hits, so a carry that is off shows in a non-zero count.  The
pool's queries have 7 to 12 k-mers (13 to 18 residues): a protein query of fewer than 7 k-mers is not searched
(search_protein.go:74-76).  Every tenth window is a long one (up to 200 residues), so the bitmaps are not all one word."""
import numpy as np
import pytest

from kaamer_amd import abi, api, workload

pytestmark = pytest.mark.gpu

K = 5                      # max_results of the top-N cases
TOP = (0.0, 1, K)          # (min_k_ratio, min_k_match, max_results): the pool's queries have fewer than 10 k-mers
N_HIT = N_MISS = 250
PAIR_DTYPE = np.dtype([(k, "<i4") for k in ("status", "n_ops", "start_i", "start_j", "end_i", "end_j", "identical", "similar", "mismatches",
                                             "gap_openings", "raw")] + [("query_len", "<u4"), ("off", "<u8"), ("entry", "<u4"), ("subject_len", "<u4")])
SIZES = ["1", "tile - 1", "tile", "tile + 1", "2 * tile", "8 * tile - 1", "8 * tile", "8 * tile + 1", "9 * tile", "9 * tile + 1"]
TILED = {"8 * tile + 1", "9 * tile", "9 * tile + 1"}


def _dev(ptr, n, dtype):
    from test_gpu_protein import _from_ptr
    return _from_ptr(ptr, int(n), dtype)


def _cumsum0(v):
    return np.concatenate([np.zeros(1, np.uint64), np.cumsum(v, dtype=np.uint64)])


def _gather(first, lengths):
    """indices of the concatenated ranges [first[i], first[i] + lengths[i])"""
    lengths = np.asarray(lengths, np.int64)
    if len(lengths) == 0 or int(lengths.sum()) == 0:
        return np.zeros(0, np.int64)
    return workload._gather_index(np.asarray(first, np.int64), lengths)


class Pool:
    """the distinct queries and the oracle's answer for each"""

    def __init__(self, db, oracle, oix, seed=20261021):
        rng = np.random.default_rng(seed)
        recs = workload.unpack(db)
        aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
        seqs, seen = [], set()
        while len(seqs) < N_HIT:                              # exact windows of database records
            rec = recs[int(rng.integers(0, len(recs)))]
            n = int(rng.integers(70, 201)) if len(seqs) % 10 == 0 else int(rng.integers(13, 19))
            if len(rec) < n:
                continue
            a = int(rng.integers(0, len(rec) - n + 1))
            s = rec[a:a + n]
            if s not in seen:
                seen.add(s)
                seqs.append(s)
        while len(seqs) < N_HIT + N_MISS:                     # random residues
            s = aa[rng.integers(0, 20, int(rng.integers(13, 19)))].tobytes()
            if s not in seen:
                seen.add(s)
                seqs.append(s)
        self.seqs = seqs
        self.buf, self.off = api.pack_sequences(seqs)
        self.len = np.diff(self.off.astype(np.int64))
        self.size = np.array([oracle.size_in_kmer(s) for s in seqs], np.int64)
        self.answers = [oix.search(s, size=int(z), want_positions=True) for s, z in zip(seqs, self.size)]   # (Kmatch desc, id asc)
        self.cnt = np.array([len(a[0]) for a in self.answers], np.int64)
        self.hit_off = _cumsum0(self.cnt).astype(np.int64)
        by_id = [np.argsort(a[0], kind="stable") for a in self.answers]
        self.pid = np.concatenate([a[0][o] for a, o in zip(self.answers, by_id)]).astype(np.uint32)
        self.km = np.concatenate([a[1][o] for a, o in zip(self.answers, by_id)]).astype(np.uint32)
        # what the post-step reports of each: sortMapByValue's order, FilterResults with TOP
        self.top_cnt = np.array([oracle.filter_results(a[1], int(z), *TOP) if len(a[1]) else 0 for a, z in zip(self.answers, self.size)], np.int64)
        self.top_off = _cumsum0(self.top_cnt).astype(np.int64)
        self.top_pid = np.concatenate([a[0][:k] for a, k in zip(self.answers, self.top_cnt)]).astype(np.uint32)
        self.top_km = np.concatenate([a[1][:k] for a, k in zip(self.answers, self.top_cnt)]).astype(np.uint32)
        # the pool is what the tests need it to be
        assert len(set(seqs)) == N_HIT + N_MISS and (self.size >= 7).all() and self.size[N_HIT:].max() <= 12
        assert (self.cnt[:N_HIT] >= 1).all() and (self.top_cnt[:N_HIT] >= 1).all()
        assert all(int(a[1][0]) == z for a, z in zip(self.answers[:N_HIT], self.size[:N_HIT]))       # a window matches its record in full
        assert int((self.cnt[N_HIT:] == 0).sum()) >= 200
        assert (self.size[:N_HIT] > 64).sum() >= 10 and (self.size[:N_HIT] <= 12).sum() >= 200

    def rows(self, e):
        """{protein id: PositionHits row} of pool entry e"""
        pid, km, pos = self.answers[e]
        return {int(p): np.asarray(pos[i], bool) for i, p in enumerate(pid)}


def edges_of(n, tile):
    """the queries on either side of every tile edge, and the last one"""
    e = {n - 1}
    for k in range(1, n // tile + 2):
        e |= {q for q in (k * tile - 1, k * tile, k * tile + 1) if 0 <= q < n}
    return sorted(e)


def batch_of(pool, n, tile):
    """-> (pool entry of every query, packed batch, edge queries): a fixed pattern over the whole pool; the edge queries take
    guaranteed hits, long and short windows in turn"""
    i = np.arange(n, dtype=np.int64)
    idx = (i * 7 + (i // 500) * 3) % (N_HIT + N_MISS)
    edges = edges_of(n, tile)
    idx[edges] = (np.arange(len(edges)) * 5) % N_HIT
    assert (pool.cnt[idx[edges]] >= 1).all() and (pool.top_cnt[idx[edges]] >= 1).all()               # guaranteed hits, by the oracle
    lens = pool.len[idx]
    buf = pool.buf[_gather(pool.off[:-1][idx], lens)]
    offs = _cumsum0(lens)
    return idx, (np.ascontiguousarray(buf), offs), edges


def expected_hits(pool, idx):
    """-> (hits per query, protein ids and Kmatch of all queries' hits, each query's by id)"""
    cnt = pool.cnt[idx]
    g = _gather(pool.hit_off[:-1][idx], cnt)
    return cnt, pool.pid[g], pool.km[g]


def by_id(off, cnt, pid, km):
    """the hit lists at off[q] .. off[q] + cnt[q] of the device arrays, each query's sorted by id -> (ids, Kmatch, where each lay)"""
    g = _gather(off, cnt)
    q = np.repeat(np.arange(len(cnt)), np.asarray(cnt, np.int64))
    order = np.lexsort((pid[g], q))
    return pid[g][order], km[g][order], g[order]


@pytest.fixture(scope="module")
def geo(klib):
    g = api.scan_geometry()
    # the sizes below were written for these; every size is derived from them
    assert g["tile"] == 16384 == g["block"] * g["items"] and g["single_max"] == 131072 == 8 * g["tile"]
    return g


@pytest.fixture(scope="module")
def world(klib, oracle, gpu_device, geo):
    db = workload.make_db(300, seed=11)
    rows = [b"EntryID\tSequence\tNote"] + [b"P%d\t%s\tn%d" % (i, s, i) for i, s in enumerate(workload.unpack(db))]
    prot = api.Proteins.from_tsv(b"\n".join(rows) + b"\n")             # (the TSV rule: ids 0, 1, ... in row order, as the oracle's)
    assert np.array_equal(prot.packed[0], db[0]) and prot.ids.tolist() == list(range(300))
    ix = api.Index.from_image(prot.image(), gpu_device)
    ix.attach_proteins(prot)
    oix = oracle.Index.from_proteins(None, packed=db)
    pool = Pool(db, oracle, oix)
    tile = geo["tile"]
    batches = {}

    def batch(n):
        if n not in batches:
            batches[n] = batch_of(pool, n, tile)
        return batches[n]
    max_bytes = len(batch(9 * tile + 1)[1][0]) + 4096
    w = dict(db=db, prot=prot, ix=ix, oix=oix, pool=pool, batch=batch, max_bytes=max_bytes, max_n=9 * tile + 1, ws={})
    yield w
    for ws in w["ws"].values():
        ws.close()
    ix.close()


def _ws(world, name, **kw):
    """the module's workspaces, each made once"""
    if name not in world["ws"]:
        world["ws"][name] = api.Workspace(world["ix"], world["max_bytes"], kw.pop("max_seqs", world["max_n"]), **kw)
    return world["ws"][name]


def _upload(packed):
    import torch
    buf, offs = packed
    d_buf = torch.from_numpy(buf if len(buf) else np.zeros(1, np.uint8)).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(offs).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return d_buf, d_off, torch.cuda.current_stream().cuda_stream


def _search(ws, packed, dev):
    d_buf, d_off, st = dev
    n = len(packed[1]) - 1
    r = ws.search_device(d_buf.data_ptr(), d_off.data_ptr(), n, len(packed[0]), stream=st)
    return r, ws.finish(st)


def _form(geo, expr):
    """n of a size expression, and the form a scan bounded by n takes"""
    n = int(eval(expr, {"tile": geo["tile"]}))
    tiled = n > geo["single_max"]
    assert tiled == (expr in TILED)
    return n, tiled


@pytest.mark.parametrize("expr", SIZES)
def test_csr_compaction(world, geo, expr):
    """Workspace(compact=True): the bound is the batch's sequence count.  8 * tile is the last single-form size, its total
    written by a ninth round of the loop; at 9 * tile the tiled form's total sits alone in block 9."""
    tile = geo["tile"]
    n, tiled = _form(geo, expr)
    if expr == "8 * tile":
        assert n % tile == 0 and n == geo["single_max"] and n // tile + 1 == 9
    if expr == "9 * tile":
        assert n % tile == 0 and (n + 1 + tile - 1) // tile == 10
    pool = world["pool"]
    idx, packed, edges = world["batch"](n)
    want_cnt, want_pid, want_km = expected_hits(pool, idx)
    dev = _upload(packed)
    r, c = _search(_ws(world, "compact", compact=True), packed, dev)
    cnt = _dev(r.d_hit_cnt, n, np.uint32)
    off = _dev(r.d_hit_off, n + 1, np.uint64)
    assert np.array_equal(off, _cumsum0(cnt))
    assert int(off[n]) == c["n_hits"] == int(want_cnt.sum()) and c["n_queries"] == n
    assert np.array_equal(cnt, want_cnt)
    nh = int(off[n])
    pid, km, _ = by_id(off[:n], cnt, _dev(r.d_hit_pid, nh, np.uint32), _dev(r.d_hit_kmatch, nh, np.uint32))
    assert np.array_equal(pid, want_pid) and np.array_equal(km, want_km)
    # the sparse form of the same batch holds the same hit sets
    r2, c2 = _search(_ws(world, "sparse"), packed, dev)
    cnt2 = _dev(r2.d_hit_cnt, n, np.uint32)
    off2 = _dev(r2.d_hit_off, n, np.uint64)
    assert np.array_equal(cnt2, cnt) and c2 == c
    m = int((off2 + cnt2).max())
    assert m <= r2.hit_capacity
    pid2, km2, _ = by_id(off2, cnt2, _dev(r2.d_hit_pid, m, np.uint32), _dev(r2.d_hit_kmatch, m, np.uint32))
    assert np.array_equal(pid2, want_pid) and np.array_equal(km2, want_km)


@pytest.mark.parametrize("expr", ["tile", "8 * tile", "8 * tile + 1", "9 * tile"])
def test_position_hits_layout(world, geo, expr):
    """want_positions=True: d_pos_base is the scan of the queries' bitmap words, bounded by the batch's sequence count"""
    n, tiled = _form(geo, expr)
    pool = world["pool"]
    idx, packed, edges = world["batch"](n)
    want_cnt, want_pid, want_km = expected_hits(pool, idx)
    r, c = _search(_ws(world, "positions", want_positions=True), packed, _upload(packed))
    cnt = _dev(r.d_hit_cnt, n, np.uint32).astype(np.int64)
    off = _dev(r.d_hit_off, n, np.uint64).astype(np.int64)
    assert np.array_equal(cnt, want_cnt)
    words = (pool.size[idx] + 63) // 64                            # u64 words per hit: SizeInKmer bits
    base = _dev(r.d_pos_base, n + 1, np.uint64)
    assert np.array_equal(base, _cumsum0(cnt * words))
    m = int((off + cnt).max())
    pid, km, where = by_id(off, cnt, _dev(r.d_hit_pid, m, np.uint32), _dev(r.d_hit_kmatch, m, np.uint32))
    assert np.array_equal(pid, want_pid) and np.array_equal(km, want_km)
    # every hit's bitmap starts where the scan puts its query's, the query's hits one after the other in list order
    pos_off = _dev(r.d_pos_off, m, np.uint64).astype(np.int64)
    g = _gather(off, cnt)
    within = g - np.repeat(off, cnt)
    assert np.array_equal(pos_off[g], np.repeat(base[:-1].astype(np.int64), cnt) + within * np.repeat(words, cnt))
    bits = _dev(r.d_pos_bits, int(base[n]), np.uint64)
    hit_pid = _dev(r.d_hit_pid, m, np.uint32)
    n_rows = 0
    for q in edges:
        rows, nw, size = pool.rows(int(idx[q])), int(words[q]), int(pool.size[idx[q]])
        assert cnt[q] == len(rows) >= 1
        for h in range(int(off[q]), int(off[q] + cnt[q])):
            got = np.unpackbits(bits[int(pos_off[h]):int(pos_off[h]) + nw].view(np.uint8), bitorder="little")[:size].astype(bool)
            assert np.array_equal(got, rows[int(hit_pid[h])]), (q, h)
            n_rows += 1
    assert n_rows >= len(edges)


def _topn(world, ws, packed, dev, step):
    """search, top-N and one of the two stages behind it on `ws` -> dict of what the stage left, copied home"""
    d_buf, d_off, st = dev
    n = len(packed[1]) - 1
    ws.search_device(d_buf.data_ptr(), d_off.data_ptr(), n, len(packed[0]), stream=st)
    t = ws.topn_device(*TOP, stream=st)
    out = {}
    if step == "positions":
        r = ws.topn_positions_device(t, stream=st)
    else:
        r = ws.topn_align_device(t, max_query_len=int(np.diff(packed[1].astype(np.int64)).max()), stream=st)
    ws.finish(st)
    out["cnt"] = _dev(t.d_top_cnt, n, np.uint32).astype(np.int64)
    live = np.arange(K)[None, :] < out["cnt"][:, None]              # (slots beyond top_cnt are not part of the result)
    out["pid"] = np.where(live, _dev(t.d_top_pid, n * K, np.uint32).reshape(n, K), 0)
    out["km"] = np.where(live, _dev(t.d_top_kmatch, n * K, np.uint32).reshape(n, K), 0)
    if step == "positions":
        out["base"] = _dev(r.d_pos_base, n + 1, np.uint64)
        out["len"] = _dev(r.d_pos_bits_len, n, np.int32)
        assert int(out["base"][n]) <= r.pos_words_capacity
        out["bits"] = _dev(r.d_pos_bits, int(out["base"][n]), np.uint64)
    else:
        out["pair_off"] = _dev(r.d_pair_off, n + 1, np.uint64)
        assert int(out["pair_off"][n]) <= r.pair_capacity
        out["pairs"] = _dev(r.d_pairs, int(out["pair_off"][n]) * PAIR_DTYPE.itemsize, np.uint8).view(PAIR_DTYPE)
    return out


def test_topn_family_by_capacity(world, geo, oracle):
    """the top-N positions scan and the top-N alignment scan are bounded by the workspace's query capacity: the same batch of
    tile + 1 queries on a workspace made for 8 * tile + 1 queries (tiled form) and on one made for the batch (single form)"""
    tile = geo["tile"]
    n = tile + 1
    pool = world["pool"]
    idx, packed, edges = world["batch"](n)
    dev = _upload(packed)
    big = _ws(world, "topn big", max_seqs=n, max_queries=8 * tile + 1, first_pos=1)
    fit = _ws(world, "topn fit", max_seqs=n, max_queries=n, first_pos=1)
    assert big.query_capacity == 8 * tile + 1 > geo["single_max"] >= fit.query_capacity == n
    assert PAIR_DTYPE.itemsize == abi.C.sizeof(abi.AlignPair)
    want_cnt = pool.top_cnt[idx]
    slot = np.arange(K)[None, :]
    live = slot < want_cnt[:, None]
    src = np.where(live, pool.top_off[:-1][idx][:, None] + slot, 0)
    want_pid, want_km = np.where(live, pool.top_pid[src], 0), np.where(live, pool.top_km[src], 0)
    words = (pool.size[idx] + 63) // 64
    recs = workload.unpack(world["db"])
    n_aa = world["prot"].stats()["NumberOfAA"]
    for step in ("positions", "align"):
        a, b = _topn(world, big, packed, dev, step), _topn(world, fit, packed, dev, step)
        for got in (a, b):
            assert np.array_equal(got["cnt"], want_cnt) and np.array_equal(got["pid"], want_pid) and np.array_equal(got["km"], want_km)
        if step == "positions":
            for got in (a, b):
                assert np.array_equal(got["base"], _cumsum0(want_cnt * words))
                assert np.array_equal(got["len"], np.where(want_cnt > 0, pool.size[idx], 0))
            assert np.array_equal(a["bits"], b["bits"])
            for q in edges:
                rows, nw, size = pool.rows(int(idx[q])), int(words[q]), int(pool.size[idx[q]])
                for h in range(int(want_cnt[q])):
                    at = int(a["base"][q]) + h * nw
                    got = np.unpackbits(a["bits"][at:at + nw].view(np.uint8), bitorder="little")[:size].astype(bool)
                    assert np.array_equal(got, rows[int(want_pid[q, h])]), (q, h)
        else:
            for got in (a, b):
                assert np.array_equal(got["pair_off"], _cumsum0(want_cnt))
            fields = [k for k in PAIR_DTYPE.names if k != "off"]          # (off: where the pair's operations lie in the stage's own buffer)
            assert np.array_equal(a["pairs"][fields], b["pairs"][fields])
            n_pairs = 0
            for q in edges:
                query = pool.seqs[int(idx[q])]
                for h in range(int(want_cnt[q])):
                    p = a["pairs"][int(a["pair_off"][q]) + h]
                    assert int(p["query_len"]) == len(query) and int(p["entry"]) == int(want_pid[q, h])
                    try:
                        e = oracle.align(query, recs[int(want_pid[q, h])], n_aa)
                    except ValueError:                                    # a letter outside the aligner's alphabet: no alignment
                        assert int(p["status"]) != 0
                        continue
                    assert int(p["status"]) == 0
                    assert (int(p["n_ops"]), int(p["mismatches"]), int(p["gap_openings"]), int(p["raw"])) == \
                        (e["length"], e["mismatches"], e["gap_openings"], e["raw"])
                    assert (int(p["start_i"]) + 1, int(p["end_i"]), int(p["start_j"]) + 1, int(p["end_j"])) == \
                        (e["q_start"], e["q_end"], e["s_start"], e["s_end"])
                    n_pairs += 1
            assert n_pairs >= len(edges)


def test_reported_hit_block(world, geo):
    """Index.search_top of 8 * tile + 1 queries: the slot's query capacity follows the batch, so rep_rank, rep_eoff and
    rep_aoff take the tiled form.  The whole unpacked result against the pool's post-step answers, with numpy."""
    tile = geo["tile"]
    n = 8 * tile + 1
    assert n > geo["single_max"]
    pool = world["pool"]
    idx, packed, edges = world["batch"](n)
    top = world["ix"].search_top(packed=packed, min_k_ratio=TOP[0], min_k_match=TOP[1], max_results=K)
    want_cnt = pool.top_cnt[idx]
    reported = np.flatnonzero(want_cnt)
    assert set(edges) <= set(reported.tolist()) and 0 < len(reported) < n
    assert top.n_queries == n and top.n_reported == len(reported)
    assert np.array_equal(top.rep_query, reported)
    assert np.array_equal(top.top_off, _cumsum0(want_cnt[reported]))
    g = _gather(pool.top_off[:-1][idx[reported]], want_cnt[reported])
    assert np.array_equal(top.top_pid, pool.top_pid[g]) and np.array_equal(top.top_kmatch, pool.top_km[g])
    assert np.array_equal(top.meta["size_in_kmer"], pool.size[idx[reported]])
    assert np.array_equal(top.meta["end_position"], pool.len[idx[reported]])


READS_MAX, PIECE_CODONS = 192, 4096      # translate.hip.inc: the narrow lane-per-read kernel's limit; codons per piece of a frame


def test_translate_piece_scans(world, geo, oracle):
    """21 900 contigs of 193 to 260 nt and one of 3 * 4096 + 5 nt: each is a long sequence of one piece per frame (the long
    one: two), 131 412 piece items; the three piece-item scans are bounded by 6 * (seq_bytes / 12288 + n_long_bound + 1),
    above single_max.  The narrow lane-per-read kernel is forced (KAAMER_WIDE_READS=0, read when the workspace is made):
    a batch of this mean length would else go through the wide one, which takes reads of up to 384 nt, and leave 12 items."""
    import torch
    from test_gpu_reads import _check_reads
    db, ix, oix = world["db"], world["ix"], world["oix"]
    rng = np.random.default_rng(5)
    nt = np.frombuffer(b"ACGT", np.uint8)
    n_short, mid = 21900, 10950
    contigs = [nt[rng.integers(0, 4, int(ln))].tobytes() for ln in rng.integers(193, 261, n_short)]
    planted = workload.unpack(workload.make_reads(db, 12, read_len=240, seed=3, db_frac=1.0))
    item_edge = geo["tile"] // 6                                    # the sequence whose items straddle piece item 16 384
    assert item_edge == 2730
    chosen = [0, item_edge - 1, item_edge, item_edge + 1, item_edge + 2, mid - 1, mid + 1, n_short - 1]
    for i, r in zip(chosen, planted):
        contigs[i] = r
    long_one = bytearray(nt[rng.integers(0, 4, 3 * PIECE_CODONS + 5)].tobytes())
    long_one[5000:5000 + len(planted[8])] = planted[8]
    contigs.insert(mid, bytes(long_one))
    chosen = [c + (c >= mid) for c in chosen] + [mid]
    buf, offs = api.pack_sequences(contigs)
    n, lens = len(contigs), np.diff(offs.astype(np.int64))
    assert n == n_short + 1 and lens.min() > READS_MAX and (lens // 3 // PIECE_CODONS + 1).sum() == n + 1
    n_long_bound = min(n, len(buf) // (READS_MAX + 1) + 1)
    piece_bound = 6 * (len(buf) // 3 // PIECE_CODONS + n_long_bound + 1)
    n_items = 6 * (n + 1)
    assert n_long_bound == n and n_items <= piece_bound and piece_bound > geo["single_max"]       # the tiled form, over ...
    assert n_items > 8 * geo["tile"] and 6 * (item_edge + 1) > geo["tile"] > 6 * item_edge        # ... items that fill nine tiles
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("KAAMER_WIDE_READS", "0")
        ws = api.Workspace(ix, len(buf), n, seq_type=abi.NUCLEOTIDE)
    try:
        dev = _upload((buf, offs))
        r, c = _search(ws, (buf, offs), dev)
        nq = int(_dev(r.d_n_queries, 1, np.uint32)[0])
        assert nq == c["n_queries"] <= r.n_queries_cap
        res = api.BatchResult.__new__(api.BatchResult)
        res.n_queries = nq
        res.meta = _dev(r.d_q, nq * api.META_DTYPE.itemsize, np.uint8).view(api.META_DTYPE)
        res.hit_off = _dev(r.d_hit_off, nq, np.uint64)
        res.hit_cnt = _dev(r.d_hit_cnt, nq, np.uint32)
        m = int((res.hit_off + res.hit_cnt).max())
        res.hit_pid, res.hit_kmatch, res.hit_first_pos = (_dev(p, m, np.uint32) for p in (r.d_hit_pid, r.d_hit_kmatch, r.d_hit_first_pos))
        res.orf_aa = _dev(r.d_orf_aa, int((res.meta["aa_off"] + res.meta["aa_len"]).max()), np.uint8)
        res.starts_alt = _dev(r.d_starts_alt, int((res.meta["sa_off"].astype(np.int64) + res.meta["sa_len"]).max()), np.int32)
        torch.cuda.synchronize()
    finally:
        ws.close()
    # the ORFs of every sequence, as test_gpu_reads._check_reads(..., check_hits=False) checks them
    meta = res.meta.tolist()
    aa, sa = res.orf_aa.tobytes(), res.starts_alt.tolist()
    names = api.META_DTYPE.names
    f = {k: names.index(k) for k in names}
    src = [m[f["src_seq"]] for m in meta]
    assert src == sorted(src)                                       # grouped by input sequence, in input order
    first = np.searchsorted(np.asarray(src), np.arange(n + 1))
    n_orfs = 0
    for s, contig in enumerate(contigs):
        exp = oracle.get_orfs(contig)
        got = []
        for m in meta[int(first[s]):int(first[s + 1])]:
            seq = aa[m[f["aa_off"]]:m[f["aa_off"]] + m[f["aa_len"]]].decode("latin-1")
            got.append(dict(seq=seq, start=m[f["start_position"]], end=m[f["end_position"]], plus=bool(m[f["plus_strand"]]),
                            starts=sa[m[f["sa_off"]]:m[f["sa_off"]] + m[f["sa_len"]]]))
            assert m[f["size_in_kmer"]] == len(seq) - 6 - seq.endswith("*")
        assert got == exp, "sequence %d" % s
        n_orfs += len(exp)
    assert n_orfs == nq > 100000
    # ... and the hits of the first, the last and the long sequence and of those around the first tile edge of the piece items
    n_hits = 0
    for s in sorted(chosen):
        sub = api.BatchResult.__new__(api.BatchResult)
        a, b = int(first[s]), int(first[s + 1])
        sub.n_queries = b - a
        sub.meta = res.meta[a:b].copy()
        sub.meta["src_seq"] = 0
        sub.hit_off, sub.hit_cnt = res.hit_off[a:b], res.hit_cnt[a:b]
        sub.hit_pid, sub.hit_kmatch, sub.hit_first_pos, sub.orf_aa, sub.starts_alt = res.hit_pid, res.hit_kmatch, res.hit_first_pos, res.orf_aa, res.starts_alt
        assert _check_reads(sub, [contigs[s]], oracle, oix, check_hits=True) == b - a
        n_hits += int(sub.hit_cnt.sum())
    assert n_hits >= len(chosen)
