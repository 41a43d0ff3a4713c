"""kaamer_tsv_rows_device on fabricated device arrays against the restatement of search.go:505-554 (tsvref.py), byte for
byte, with the line offsets exact: the float sweep, name / id / value lengths, rows that start and end on every boundary
kaamer_tsv_geometry names, empty queries, result counts, bitmaps, the missing-entry rule and the capacity status."""
import ctypes as C

import numpy as np
import pytest

import tsvcases
import tsvref
from kaamer_amd import abi, api

pytestmark = pytest.mark.gpu

FLAGS = [(False, False), (False, True), (True, False), (True, True)]


@pytest.fixture(scope="module")
def setup(klib, gpu_device):
    table = tsvcases.standard_table()
    img = table.image()
    ix = api.Index.from_image(img, gpu_device)
    ix.attach_subject_text(table)
    yield dict(ix=ix, table=table, entries=tsvref.entries_of(table), features=table.feature_names)
    ix.close()


def _dev(arr):
    import torch
    raw = bytearray(arr.tobytes()) + bytearray(16)
    return torch.frombuffer(raw, dtype=torch.uint8).cuda()


def _home(ptr, n, dtype):
    out = np.zeros(n, dtype)
    if out.nbytes:
        assert api._hip_runtime().hipMemcpy(out.ctypes.data, C.c_void_p(ptr), out.nbytes, 2) == 0
    return out


def run_stage(ix, names, queries, K, positions, annotations, out_cap, stage=None, max_lines=None):
    """-> (rows, line_off, the bytes behind the rows) or raises; the stage is made for the batch unless given"""
    import torch
    a = tsvcases.device_arrays(queries, K)
    buf, spans = tsvcases.names_buffer(names)
    n_lines = sum(len(q["hits"]) for q in queries)
    own = stage is None
    if own:
        stage = api.TsvStage(ix, len(queries), n_lines if max_lines is None else max_lines)
    t = {k: _dev(v) for k, v in dict(meta=a.meta, cnt=a.top_cnt, pid=a.top_pid, km=a.top_km, start=a.start, size=a.size, plen=a.pos_len,
                                     pbase=a.pos_base, pbits=a.pos_bits, names=np.frombuffer(buf, np.uint8), spans=spans,
                                     nq=np.array([len(queries)], np.uint32)).items()}
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
    try:
        res = stage.rows_device(rin, out.data_ptr(), out_cap)
        lines, nbytes = stage.finish()
        assert lines == n_lines and nbytes <= out_cap
        home = out.cpu().numpy().tobytes()
        off = _home(res.d_line_off, lines + 1, np.uint64)
        run_stage.counts = _home(res.d_counts, 4, np.uint64).tolist()      # rows, bytes, status, raw scores outside the table
        run_stage.off = off
        return home[:nbytes], off, home[nbytes:]
    finally:
        if own:
            torch.cuda.synchronize()
            stage.close()


def check(setup, names, queries, K, positions, annotations, slack=0):
    want, want_off = tsvref.rows_ref(tsvcases.ref_queries(names, queries), setup["entries"], setup["features"], positions, annotations)
    got, off, rest = run_stage(setup["ix"], names, queries, K, positions, annotations, len(want) + slack)
    assert got == want
    assert off.tolist() == want_off.tolist()
    assert rest == b"\x55" * len(rest)            # nothing behind the rows
    if positions:                                  # field 6 is the comma count of field 11
        for row in got.split(b"\n")[:-1]:
            f = row.split(b"\t")
            f = f[len(f) - (14 if annotations else 11):]      # (a tab in the name is an ordinary byte of field 1)
            assert int(f[5]) == f[10].count(b",")
    return got


def test_geometry_and_info(setup):
    g = api.tsv_geometry()
    assert g["tile"] == g["threads"] and g["window"] % g["store"] == 0 and g["store"] == 16
    info = setup["ix"].subject_text_info()
    ent = setup["entries"]
    longest = max(len(e["EntryId"]) + len(str(e["Length"])) + sum(1 + len(v) for v in e["Features"].values()) for e in ent.values())
    assert (info["entries"], info["features"], info["max_row_suffix"]) == (len(ent), 3, longest)
    assert info["table_bytes"] > sum(len(e["EntryId"]) for e in ent.values())


def test_no_queries(setup):
    got, off, rest = run_stage(setup["ix"], [], [], 1, True, True, 64)
    assert got == b"" and off.tolist() == [0] and rest == b"\x55" * len(rest) and run_stage.counts == [0, 0, 0, 0]


def test_float_sweep_in_one_launch(setup):
    names, queries = tsvcases.float_sweep()
    got = check(setup, names, queries, 1, False, False)
    rows = got.split(b"\n")
    for i, ((k, n), text) in enumerate(tsvcases.FLOAT_VECTORS):
        assert rows[400 * 401 // 2 + i].split(b"\t")[2] == text.encode()


@pytest.mark.parametrize("positions,annotations", FLAGS)
def test_hand_built_batches(setup, positions, annotations):
    """names, ids and values of every length, ORFs of one record with a trimmed start, queries that report nothing between
    reporting ones, one to ten hits, the missing-entry rule, bitmaps, an empty batch"""
    for name, (names, queries) in tsvcases.standard_cases().items():
        K = max([len(q["hits"]) for q in queries] + [1])
        got = check(setup, names, queries, K, positions, annotations, slack=0 if name != "entries" else 5)
        if K < 10:
            assert check(setup, names, queries, 10, positions, annotations) == got      # counts below max_results


def test_missing_entry_rule(setup):
    names, queries = tsvcases.standard_cases()["missing"]
    got = check(setup, names, queries, 3, False, True)
    rows = [r.split(b"\t") for r in got.split(b"\n")[:-1]]
    assert [bool(r[1]) for r in rows] == [True, False, False, True, False, False, True, True, False]
    assert [r[9] for r in rows if not r[1]] == [b"0"] * 5 and all(r[10:] == [b"", b"", b""] for r in rows if not r[1])


def _line_len(setup, name_len, annotations):
    q = [tsvcases.query(0, 20, [(1, 5)])]
    return len(tsvref.rows_ref(tsvcases.ref_queries([b"n" * name_len], q), setup["entries"], setup["features"], False, annotations)[0])


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_rows_on_window_and_tile_boundaries(setup, delta):
    """rows that end (and the next ones start) `delta` bytes from every multiple of the LDS window, in a batch of several
    tiles whose first bytes fall anywhere; unreported queries in between; one row longer than two windows"""
    g = api.tsv_geometry()
    base = _line_len(setup, 0, False)
    rng = np.random.default_rng(5 + delta)
    names, queries, at = [], [], 0

    def add(name_len):
        nonlocal at
        names.append(b"n" * name_len)
        queries.append(tsvcases.query(len(names) - 1, 20, [(1, 5)]))
        at += base + name_len
        if rng.random() < 0.2:
            queries.append(tsvcases.query(0, 9, []))
    targets = [g["window"] * k + delta for k in (1, 2, 3)]
    for i, t in enumerate(targets):
        while t - at > 400:
            add(int(rng.integers(0, 41)))
        add(t - at - base)
        assert at == t
        if i == 1:
            add(2 * g["window"] + 77)             # a row across two whole windows
            targets[2] = (at // g["window"] + 2) * g["window"] + delta
    for _ in range(50):
        add(int(rng.integers(0, 41)))
    assert len(queries) > 3 * g["tile"]
    got = check(setup, names, queries, 1, False, False)
    assert len(got) == at


def test_tiles_that_end_on_window_boundaries(setup):
    """every row 64 bytes: each tile of queries fills a whole number of windows' 16-byte chunks exactly"""
    g = api.tsv_geometry()
    name_len = 64 - _line_len(setup, 0, False)
    assert name_len >= 0
    n = g["tile"] * 5 + 3
    names = [b"n" * name_len]
    got = check(setup, names, [tsvcases.query(0, 20, [(1, 5)]) for _ in range(n)], 1, False, False)
    assert len(got) == 64 * n and g["tile"] * 64 == g["window"]


def test_more_tiles_than_one_round_of_the_scan(setup):
    """65 537 queries are 257 tiles: out_scan_kernel, one workgroup that takes `threads` tiles per round, goes round twice
    under the plain rows as well; hits on the first and the last query of the first tile, the first of the second, and on
    either side of the second round's first tile.  Rows and line offsets against the restatement (check) and against the
    host formatter."""
    g = api.tsv_geometry()
    n = g["tile"] * g["threads"] + 1
    assert n == 65537 and (n + g["tile"] - 1) // g["tile"] == g["threads"] + 1        # the second round holds one tile
    hit = (0, g["tile"] - 1, g["tile"], n - 2, n - 1)
    assert hit == (0, 255, 256, 65535, 65536)
    names = [b"sweep of tiles"]
    queries = [tsvcases.query(0, 20 + i % 7, [(i % tsvcases.N_ENTRIES, 5 + i % 11)] if i in hit else []) for i in range(n)]
    got = check(setup, names, queries, 1, False, True)
    off = run_stage.off
    assert got.count(b"\n") == len(hit) and run_stage.counts[:1] + run_stage.counts[2:] == [len(hit), 0, 0]
    buf, spans = tsvcases.names_buffer(names)
    host, host_off = api.format_tsv(tsvcases.host_top(queries), buf, spans, setup["table"], False, True)
    assert got == host and off.tolist() == host_off.tolist()


def test_capacity_and_the_next_call(setup):
    import torch
    names, queries = tsvcases.standard_cases()["entries"]
    ix = setup["ix"]
    want, want_off = tsvref.rows_ref(tsvcases.ref_queries(names, queries), setup["entries"], setup["features"], True, True)
    n_lines = len(want_off) - 1
    stage = api.TsvStage(ix, len(queries), n_lines)
    try:
        with pytest.raises(abi.KaamerError) as e:
            run_stage(ix, names, queries, 10, True, True, len(want) - 1, stage=stage)
        assert e.value.code == abi.E_CAPACITY and e.value.counts == (n_lines, len(want))    # ... and says what was needed
        got, off, rest = run_stage(ix, names, queries, 10, True, True, len(want), stage=stage)
        assert got == want and off.tolist() == want_off.tolist() and rest == b"\x55" * len(rest)
    finally:
        torch.cuda.synchronize()
        stage.close()
    with pytest.raises(abi.KaamerError) as e:      # one row more than the stage holds
        run_stage(ix, names, queries, 10, True, True, len(want), max_lines=n_lines - 1)
    assert e.value.code == abi.E_CAPACITY


def test_no_subject_text_attached(setup, gpu_device):
    ix2 = api.Index.from_image(setup["table"].image(), gpu_device)
    try:
        with pytest.raises(abi.KaamerError) as e:
            run_stage(ix2, [b"q"], [tsvcases.query(0, 10, [(0, 5)])], 1, False, False, 256)
        assert e.value.code == abi.E_ARG and "kaamer_index_attach_subject_text" in str(e.value)
        assert ix2.subject_text_info()["entries"] == 0
    finally:
        ix2.close()
