"""kaamer_tsv_aln_rows_device on fabricated device arrays against the restatement of search.go:556-604 (tsvalnref.py), byte
for byte, with the line offsets exact and nothing written behind the rows; the two number formats on the device against
Python over every vector the host test uses; the order of the hits; the raw score outside the table; the capacity status.
The floats of the reference rows are kaamer_align_finish's (kaamer_align_finish_pairs): the rows compare them bit for bit
through their exact decimal forms."""
import ctypes as C

import numpy as np
import pytest

import tsvalncases
import tsvalnref
import tsvcases
import tsvref
from kaamer_amd import abi, api
from test_gpu_tsv_rows import _dev, _home
from test_tsv_aln_host import double_vectors

pytestmark = pytest.mark.gpu

FLAGS = [(False, False), (False, True), (True, False), (True, True)]


@pytest.fixture(scope="module")
def setup(klib, gpu_device):
    table = tsvcases.standard_table()
    ix = api.Index.from_image(table.image(), gpu_device)
    ix.attach_proteins(table)
    ix.attach_subject_text(table)
    naa = ix.align_info()["number_of_aa"]
    assert naa == table.stats()["NumberOfAA"]
    yield dict(ix=ix, table=table, entries=tsvref.entries_of(table), features=table.feature_names, naa=naa)
    ix.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_doubles_in_one_launch(klib, gpu_device, mode):
    import torch
    values = np.array(double_vectors(), np.float64)
    d_in = torch.from_numpy(values).cuda()
    d_out = torch.full((len(values) * 32 + 64,), 0x55, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    api.format_doubles_device(d_in.data_ptr(), len(values), mode, d_out.data_ptr())
    home = d_out.cpu().numpy().tobytes()
    assert home[len(values) * 32:] == b"\x55" * 64
    ref = tsvalnref.e_ref if mode == 0 else tsvalnref.f2_ref
    long_ones = 0
    for i, x in enumerate(values.tolist()):
        want = ref(x).encode()
        long_ones += len(want) > 31
        want = want[:31]                       # (a slot holds 31 bytes: "%.2f" of 1e29 and beyond is cut there)
        assert home[i * 32:(i + 1) * 32] == want + b"\0" * (32 - len(want)), "mode %d of %r" % (mode, x)
    assert (long_ones == 0) if mode == 0 else (long_ones > 1000)


def run_stage(setup, names, queries, K, positions, annotations, seq_type, out_cap, stage=None, max_lines=None, top_cnt=None):
    """-> (rows, line_off, the bytes behind the rows) or raises; the stage is made for the batch unless given; top_cnt: the
    counts the stage is told instead of the queries' own"""
    import torch
    ix = setup["ix"]
    a = tsvalncases.device_arrays(queries, K)
    if top_cnt is not None:
        a.top_cnt[:len(top_cnt)] = top_cnt
    buf, spans = tsvcases.names_buffer(names)
    n_lines = sum(len(q["hits"]) for q in queries)
    own = stage is None
    if own:
        stage = api.TsvStage(ix, len(queries), n_lines if max_lines is None else max_lines)
    t = {k: _dev(v) for k, v in dict(meta=a.meta, cnt=a.top_cnt, pid=a.top_pid, km=a.top_km, start=a.start, size=a.size, plen=a.pos_len,
                                     pbase=a.pos_base, pbits=a.pos_bits, names=np.frombuffer(buf, np.uint8), spans=spans,
                                     nq=np.array([len(queries)], np.uint32), poff=a.pair_off, pairs=a.pairs).items()}
    out = torch.full((int(out_cap) + 64,), 0x55, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    rin = abi.TsvRowsIn()
    rin.top = abi.TopnResult(K, t["cnt"].data_ptr(), t["pid"].data_ptr(), t["km"].data_ptr(), None, None, t["start"].data_ptr(),
                             t["size"].data_ptr())
    rin.d_q, rin.d_n_queries, rin.n_queries_cap = t["meta"].data_ptr(), t["nq"].data_ptr(), len(queries)
    rin.n_names, rin.d_name_bytes, rin.name_bytes_len, rin.d_spans = len(names), t["names"].data_ptr(), len(buf), t["spans"].data_ptr()
    pos = abi.TopnPositions(t["pbase"].data_ptr(), t["plen"].data_ptr(), t["pbits"].data_ptr(), len(a.pos_bits))
    rin.pos = C.pointer(pos) if positions else None
    rin.extract_positions, rin.annotations = int(positions), int(annotations)
    alns = abi.TopnAlignments(t["poff"].data_ptr(), t["pairs"].data_ptr(), n_lines, 0, 0, 0)
    try:
        res = stage.aln_rows_device(rin, alns, out.data_ptr(), out_cap, seq_type=seq_type)
        lines, nbytes = stage.finish()
        assert lines == n_lines and nbytes <= out_cap
        home = out.cpu().numpy().tobytes()
        off = _home(res.d_line_off, lines + 1, np.uint64)
        run_stage.counts = _home(res.d_counts, 4, np.uint64).tolist()      # rows, bytes, status, raw scores outside the table
        return home[:nbytes], off, home[nbytes:]
    finally:
        if own:
            torch.cuda.synchronize()
            stage.close()


def reference(setup, names, queries, positions, annotations, seq_type):
    queries = tsvalncases.with_alignments(queries, setup["naa"])
    protein = abi.seq_type_base(seq_type) == abi.PROTEIN
    return tsvalnref.rows_ref(tsvalncases.ref_queries(names, queries), setup["entries"], setup["features"], positions, annotations, protein)


def check(setup, names, queries, K, positions, annotations, seq_type, slack=0):
    want, want_off = reference(setup, names, queries, positions, annotations, seq_type)
    got, off, rest = run_stage(setup, names, queries, K, positions, annotations, seq_type, len(want) + slack)
    assert got == want
    assert off.tolist() == want_off.tolist()
    assert rest == b"\x55" * len(rest)            # nothing behind the rows
    return got


@pytest.mark.parametrize("seq_type", [abi.PROTEIN, abi.READS])
@pytest.mark.parametrize("positions,annotations", FLAGS)
def test_hand_built_batches(setup, positions, annotations, seq_type):
    """the order of the hits (ties, reversal, failed hits in the middle, the missing-entry rule), the numbers (no columns,
    raw 0 and the table's last raw score, 2^BitScore at its overflow, integers at their bounds), the float32 Identity sweep,
    names, bitmaps that travel with their hit, an empty batch; K at and above the counts"""
    for name, (names, queries) in tsvalncases.standard_cases().items():
        K = max([len(q["hits"]) for q in queries] + [1])
        got = check(setup, names, queries, K, positions, annotations, seq_type, slack=0 if name != "order" else 5)
        if K < 10:
            assert check(setup, names, queries, 10, positions, annotations, seq_type) == got


def test_no_queries(setup):
    got, off, rest = run_stage(setup, [], [], 1, True, True, abi.READS, 64)
    assert got == b"" and off.tolist() == [0] and rest == b"\x55" * len(rest) and run_stage.counts == [0, 0, 0, 0]


def test_more_tiles_than_one_round_of_the_scan(setup):
    """65 537 queries are 257 tiles: the scan kernel, one workgroup of 256 threads, goes round twice; hits on the first and
    the last query of the first tile, the first of the second, and on either side of the second round's first tile"""
    hit = (0, 255, 256, 65535, 65536)
    queries = [tsvalncases.aquery(0, [(i % tsvcases.N_ENTRIES, tsvalncases.aligned(40 + i % 7, shift=i % 5))] if i in hit else []) for i in range(65537)]
    got = check(setup, [b"sweep of tiles"], queries, 1, False, True, abi.PROTEIN)
    assert got.count(b"\n") == len(hit) and run_stage.counts[:1] + run_stage.counts[2:] == [len(hit), 0, 0]


def test_counts_above_max_results_are_clipped(setup):
    """top_cnt beyond K: the stage reads K hits per query, as the arrays hold them"""
    names, queries = tsvalncases.standard_cases()["order"]
    clipped = [dict(q, hits=q["hits"][:3]) for q in queries]
    want, want_off = reference(setup, names, clipped, False, True, abi.PROTEIN)
    got, off, rest = run_stage(setup, names, clipped, 3, False, True, abi.PROTEIN, len(want), top_cnt=[len(q["hits"]) for q in queries])
    assert got == want and off.tolist() == want_off.tolist() and rest == b"\x55" * len(rest)
    assert max(len(q["hits"]) for q in queries) == 10 and len(want_off) - 1 == sum(min(len(q["hits"]), 3) for q in queries)


def tiles_batch(rng, n_queries, window):
    """n_queries queries of 1 to 10 hits (every tenth reports nothing), raw scores with ties, failed hits and a missing id
    here and there, bitmaps of 70 bits; the names are chosen afterwards"""
    queries = []
    for i in range(n_queries):
        cnt = 0 if i % 10 == 3 else int(rng.integers(1, 11))
        hits = []
        pids = rng.permutation(tsvcases.N_ENTRIES)      # (a query reports a protein once)
        for r in range(cnt):
            roll = rng.random()
            pid = int(pids[r])
            if roll < 0.05:
                p = tsvalncases.pair(status=int(rng.choice([2, 3])))
            else:
                cols = int(rng.integers(1, 400))
                p = tsvalncases.aligned(int(rng.integers(0, 6)) * 37 + int(rng.integers(-2500, 3000) if roll > 0.6 else 0), cols=cols,
                                        identical=int(rng.integers(0, cols + 1)), query_len=int(rng.integers(7, 900)), shift=int(rng.integers(0, 50)))
            hits.append((pid, p, (rng.random(70) < 0.3).tolist()))
        if cnt > 2 and i % 17 == 5:   # a missing id: every later hit of the query is status 4, as the alignment stage leaves it
            at = int(rng.integers(0, cnt))
            hits = hits[:at] + [(tsvcases.MISSING if k == at else h[0], tsvalncases.pair(status=4), h[2]) for k, h in enumerate(hits) if k >= at]
        queries.append(tsvalncases.aquery(i, hits, start=int(rng.integers(1, 450)), end=int(rng.integers(1, 450)), pos_len=70))
    return queries


@pytest.mark.parametrize("seq_type", [abi.PROTEIN, abi.READS])
@pytest.mark.parametrize("positions,annotations", FLAGS)
def test_two_tiles_and_one_across_windows(setup, seq_type, positions, annotations):
    """513 queries -- two tiles plus one -- of 1 to 10 hits: several LDS windows per tile; the names are then sized so that a
    row ends exactly on a window boundary and the first tile ends exactly on one"""
    g = api.tsv_geometry()
    n = 2 * g["tile"] + 1
    rng = np.random.default_rng(20261003)
    queries = tiles_batch(rng, n, g["window"])
    names = [b"q%d" % i for i in range(n)]
    _, off = reference(setup, names, queries, positions, annotations, seq_type)
    assert int(off[-1]) > 2 * g["window"]
    rep = [i for i, q in enumerate(queries) if q["hits"]]
    csr = np.concatenate([[0], np.cumsum([len(queries[i]["hits"]) for i in rep])])

    def pad_to_boundary(single_rep, last_rep):
        """lengthens the name of a one-row query at or before last_rep so that last_rep's last row ends on a window boundary"""
        _, off = reference(setup, names, queries, positions, annotations, seq_type)
        names[rep[single_rep]] += b"x" * (-int(off[csr[last_rep + 1]]) % g["window"])
    single = [k for k in range(len(rep)) if len(queries[rep[k]]["hits"]) == 1]
    k0 = next(k for k in single if k > 5)
    pad_to_boundary(k0, k0 + 3)
    last_of_tile = max(k for k in range(len(rep)) if rep[k] < g["tile"])
    k1 = max(k for k in single if k0 + 3 < k <= last_of_tile)
    pad_to_boundary(k1, last_of_tile)
    want, off = reference(setup, names, queries, positions, annotations, seq_type)
    assert int(off[csr[k0 + 4]]) % g["window"] == 0 and int(off[csr[last_of_tile + 1]]) % g["window"] == 0
    assert check(setup, names, queries, 10, positions, annotations, seq_type) == want
    assert check(setup, names, queries, 12, positions, annotations, seq_type) == want        # K above every count


def test_order_is_the_host_finish_order(setup):
    """the rows' SubjectIds, query by query, are the hits in the stable BitScore order of kaamer_align_finish's floats"""
    rng = np.random.default_rng(7)
    queries = [q for q in tiles_batch(rng, 300, 0)]
    names = [b"q%d" % i for i in range(300)]
    got = check(setup, names, queries, 10, False, False, abi.PROTEIN)
    rows = [r.split(b"\t") for r in got.split(b"\n")[:-1]]
    at = 0
    for q in tsvalncases.with_alignments(queries, setup["naa"]):
        bits = [float(h["rec"]["bitscore"]) for h in q["hits"]]
        order = sorted(range(len(bits)), key=lambda k: -bits[k])
        for k in order:
            h = q["hits"][k]
            gone = h["pair"]["status"] == 4      # at or behind the missing id BEFORE the sort, wherever the sort puts the hit
            assert rows[at][1] == (b"" if gone else setup["entries"][h["key"]]["EntryId"])
            assert rows[at][-1] == tsvalnref.f2_ref(bits[k]).encode() and rows[at][-2] == tsvalnref.e_ref(float(h["rec"]["evalue"])).encode()
            at += 1
    assert at == len(rows)


def test_raw_score_outside_the_table(setup):
    """one pair beyond each end of the table: KAAMER_E_RANGE, counted; that batch's rows are the host
    formatter's, and the stage prints the next batch"""
    import torch
    names, queries = tsvalncases.standard_cases()["order"]
    bad = [dict(q, hits=[dict(h) for h in q["hits"]]) for q in queries]
    bad[2]["hits"][4]["pair"] = tsvalncases.aligned(tsvalncases.RAW_MAX + 1)
    bad[3]["hits"][0]["pair"] = tsvalncases.aligned(tsvalncases.RAW_MIN - 1)
    want, want_off = reference(setup, names, queries, False, True, abi.PROTEIN)
    n_lines = len(want_off) - 1
    stage = api.TsvStage(setup["ix"], len(queries), n_lines)
    try:
        with pytest.raises(abi.KaamerError) as e:
            run_stage(setup, names, bad, 10, False, True, abi.PROTEIN, len(want) + 4096, stage=stage)
        assert e.value.code == abi.E_RANGE and "kaamer_format_tsv_aln" in str(e.value)
        info = stage.aln_info()
        assert info["outside"] == 2 and info["table"] == tsvalncases.RAW_TABLE and info["tables"] == 1
        # the host route for that batch
        with_aln = tsvalncases.with_alignments(bad, setup["naa"])
        buf, spans = tsvcases.names_buffer(names)
        host, host_off = api.format_tsv(tsvalncases.host_top(with_aln), buf, spans, setup["table"], False, True, align=True, seq_type=abi.PROTEIN)
        ref, ref_off = tsvalnref.rows_ref(tsvalncases.ref_queries(names, with_aln), setup["entries"], setup["features"], False, True, True)
        assert host == ref and host_off.tolist() == ref_off.tolist()
        got, off, rest = run_stage(setup, names, queries, 10, False, True, abi.PROTEIN, len(want), stage=stage)
        assert got == want and off.tolist() == want_off.tolist() and rest == b"\x55" * len(rest)
        assert stage.aln_info() == dict(outside=0, table=tsvalncases.RAW_TABLE, tables=1)      # the table is kept with the options
    finally:
        torch.cuda.synchronize()
        stage.close()


def test_capacity_and_the_next_call(setup):
    import torch
    names, queries = tsvalncases.standard_cases()["bitmaps"]
    want, want_off = reference(setup, names, queries, True, True, abi.READS)
    n_lines = len(want_off) - 1
    stage = api.TsvStage(setup["ix"], len(queries), n_lines)
    try:
        with pytest.raises(abi.KaamerError) as e:
            run_stage(setup, names, queries, 10, True, True, abi.READS, len(want) - 1, stage=stage)
        assert e.value.code == abi.E_CAPACITY and e.value.counts == (n_lines, len(want))    # ... and says what was needed
        got, off, rest = run_stage(setup, names, queries, 10, True, True, abi.READS, len(want), stage=stage)
        assert got == want and off.tolist() == want_off.tolist() and rest == b"\x55" * len(rest)
        # the plain rows on the same stage afterwards
        import test_gpu_tsv_rows as plain
        pn, pq = tsvcases.standard_cases()["entries"]
        pwant, _ = tsvref.rows_ref(tsvcases.ref_queries(pn, pq), setup["entries"], setup["features"], False, True)
    finally:
        torch.cuda.synchronize()
        stage.close()
    assert plain.run_stage(setup["ix"], pn, pq, 10, False, True, len(pwant))[0] == pwant
    with pytest.raises(abi.KaamerError) as e:      # one row more than the stage holds
        run_stage(setup, names, queries, 10, True, True, abi.READS, len(want), max_lines=n_lines - 1)
    assert e.value.code == abi.E_CAPACITY and e.value.counts == (n_lines, len(want))


def test_missing_attaches(setup, gpu_device):
    names, queries = [b"q"], [tsvalncases.aquery(0, [(0, tsvalncases.aligned(50))])]
    for attach, missing in (("attach_subject_text", "kaamer_index_attach_proteins"), ("attach_proteins", "kaamer_index_attach_subject_text")):
        ix2 = api.Index.from_image(setup["table"].image(), gpu_device)
        try:
            getattr(ix2, attach)(setup["table"])
            with pytest.raises(abi.KaamerError) as e:
                run_stage(dict(setup, ix=ix2), names, queries, 1, False, False, abi.PROTEIN, 256)
            assert e.value.code == abi.E_ARG and missing in str(e.value)
        finally:
            ix2.close()
