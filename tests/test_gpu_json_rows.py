"""kaamer_json_rows_device on fabricated device arrays against the host formatter (kaamer_format_json_arrays) and the
restatement of encoding/json's rules (jsonref.py), byte for byte, with the object offsets exact: every case of jsoncases.py,
an object far larger than a wave's LDS buffer, objects that start at every alignment and end around every flush of that
buffer, 1 to 257 queries with empty ones in between, the capacity status and the missing attach."""
import ctypes as C

import numpy as np
import pytest

import jsoncases
import jsonref
from kaamer_amd import abi, api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup(klib, gpu_device):
    tables = {name: jsoncases.table(name) for name in jsoncases.TABLES}
    ix = api.Index.from_image(tables["std"][0].image(), gpu_device)
    state = dict(ix=ix, tables=tables, attached=None)
    yield state
    ix.close()


def _attach(setup, name):
    if setup["attached"] != name:   # (a second attach replaces the first)
        setup["ix"].attach_subject_json(setup["tables"][name][0])
        setup["attached"] = name


def _dev(arr):
    import torch
    raw = bytearray(arr.tobytes()) + bytearray(16)
    return torch.frombuffer(raw, dtype=torch.uint8).cuda()


def _home(ptr, n, dtype):
    out = np.zeros(n, dtype)
    if out.nbytes:
        assert api._hip_runtime().hipMemcpy(out.ctypes.data, C.c_void_p(ptr), out.nbytes, 2) == 0
    return out


def _seq_type(c):
    return abi.PROTEIN if c["protein"] else (abi.READS if c["fmt"] == 1 else abi.NUCLEOTIDE)


def run_stage(ix, c, out_cap, stage=None, max_objects=None, K=None):
    """-> (objects, obj_off, the bytes behind the objects) or raises; the stage is made for the batch unless given"""
    import torch
    queries = c["queries"]
    K = K or max([len(q["hits"]) for q in queries] + [1])
    a = jsoncases.device_arrays(c, K)
    buf, spans = jsoncases.names_buffer(c["names"])
    n_objects = sum(1 for q in queries if q["hits"])
    own = stage is None
    if own:
        stage = api.JsonStage(ix, len(queries), n_objects if max_objects is None else max_objects)
    t = {k: _dev(v) for k, v in dict(meta=a.meta, cnt=a.top_cnt, pid=a.top_pid, km=a.top_km, start=a.start, size=a.size, trim=a.trim, plen=a.pos_len,
                                     pbase=a.pos_base, pbits=a.pos_bits, names=np.frombuffer(buf, np.uint8), spans=spans, aa=a.aa,
                                     nq=np.array([len(queries)], np.uint32)).items()}
    out = torch.full((int(out_cap) + 64,), 0x55, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    jin = abi.JsonRowsIn()
    rin = jin.rows
    rin.top = abi.TopnResult(K, t["cnt"].data_ptr(), t["pid"].data_ptr(), t["km"].data_ptr(), None, t["trim"].data_ptr(), t["start"].data_ptr(),
                             t["size"].data_ptr())
    rin.d_q, rin.d_n_queries, rin.n_queries_cap = t["meta"].data_ptr(), t["nq"].data_ptr(), len(queries)
    rin.n_names, rin.d_name_bytes, rin.name_bytes_len, rin.d_spans = len(c["names"]), t["names"].data_ptr(), len(buf), t["spans"].data_ptr()
    pos = abi.TopnPositions(t["pbase"].data_ptr(), t["plen"].data_ptr(), t["pbits"].data_ptr(), len(a.pos_bits))
    rin.pos = C.pointer(pos) if (c["positions"] or not c["protein"]) else None
    rin.extract_positions, rin.annotations = int(c["positions"]), 0
    jin.d_aa, jin.aa_len, jin.seq_type, jin.text_format = t["aa"].data_ptr(), a.aa_len, _seq_type(c), c["fmt"]
    try:
        res = stage.rows_device(jin, out.data_ptr(), out_cap)
        objects, nbytes = stage.finish()
        assert objects == n_objects and nbytes <= out_cap
        home = out.cpu().numpy().tobytes()
        off = _home(res.d_obj_off, objects + 1, np.uint64)
        run_stage.counts = _home(res.d_counts, 4, np.uint64).tolist()      # objects, bytes, status, (unused)
        return home[:nbytes], off, home[nbytes:]
    finally:
        if own:
            torch.cuda.synchronize()
            stage.close()


def host_format(setup, c):
    names, spans = jsoncases.names_buffer(c["names"])
    seqs, offsets = jsoncases.packed(c) if c["protein"] else (None, None)
    return api.format_json(jsoncases.host_top(c), names, spans, setup["tables"][c["table"]][0], seqs=seqs, offsets=offsets, seq_type=_seq_type(c),
                           text_format=c["fmt"], positions=c["positions"])


def check(setup, c, slack=0):
    _attach(setup, c["table"])
    want, want_off = host_format(setup, c)
    ref, ref_off = jsonref.objects(jsoncases.ref_queries(c), setup["tables"][c["table"]][1], c["protein"], c["fmt"], c["positions"])
    assert want == ref and want_off.tolist() == ref_off
    got, off, rest = run_stage(setup["ix"], c, len(want) + slack)
    assert len(got) == len(want)
    if got != want:
        at = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError("first difference at byte %d of %d: %r, expected %r" % (at, len(want), got[max(at - 40, 0):at + 40], want[max(at - 40, 0):at + 40]))
    assert off.tolist() == want_off.tolist()
    assert rest == b"\x55" * len(rest)            # nothing behind the objects
    return got


def test_geometry_and_info(setup):
    g = api.json_geometry()
    assert g["tile"] == g["threads"] and g["window"] % g["store"] == 0 and g["store"] == 16
    _attach(setup, "std")
    info = setup["ix"].subject_json_info()
    ent = setup["tables"]["std"][1]
    assert (info["entries"], info["max_entry"]) == (len(ent), max(len(jsonref.protein(e)) for e in ent.values()))
    assert info["table_bytes"] > sum(len(jsonref.protein(e)) for e in ent.values())


@pytest.mark.parametrize("name", sorted(jsoncases.standard_cases()))
def test_hand_built_cases(setup, name):
    c = jsoncases.standard_cases()[name]
    got = check(setup, c, slack=0 if name != "orfs fasta" else 33)
    if name == "large":   # one object far larger than a wave's buffer
        assert len(got) > 60 * api.json_geometry()["window"]


@pytest.mark.parametrize("n,seed", [(1, 1), (63, 2), (64, 3), (65, 4), (257, 5), (700, 6)])
def test_many_queries_with_empty_ones_between(setup, n, seed):
    check(setup, jsoncases.many_queries(n, seed))


def test_no_queries(setup):
    _attach(setup, "std")
    got, off, rest = run_stage(setup["ix"], jsoncases.standard_cases()["empty"], 64)
    assert got == b"" and off.tolist() == [0] and rest == b"\x55" * len(rest) and run_stage.counts == [0, 0, 0, 0]


def test_more_tiles_than_one_round_of_the_scan(setup):
    """65 537 queries are 257 tiles: the scan kernel, one workgroup of 256 threads, goes round twice; objects on the first and
    the last query of the first tile, the first of the second, and on either side of the second round's first tile"""
    hit = (0, 255, 256, 65535, 65536)
    qs = [jsoncases.query(0, [(5 + i % 9, 3)] if i in hit else []) for i in range(65537)]
    got = check(setup, jsoncases.case("std", True, 0, False, [b"sweep of tiles"], qs, [jsoncases.residues(20)]))
    assert got.count(b'{"Query"') == len(hit) and run_stage.counts[:1] + run_stage.counts[2:] == [len(hit), 0, 0]


def test_objects_at_every_alignment_and_around_every_flush(setup):
    """objects whose length sweeps across the fill at which a wave's buffer is flushed, behind a first object that moves them
    over every alignment to the 16-byte chunks of the output"""
    w = api.json_geometry()["window"]
    for shift in (0, 1, 7, 15, 16):
        names = [b"s" * shift] + [b"n" * n for n in range(w - 1500, w - 1100, 23)] + [b"m" * n for n in (2 * w - 300, 2 * w, 3 * w + 5)]
        qs = [jsoncases.query(i, [(5, 3)], seq=jsoncases.residues(20, i), start=4, end=60) for i in range(len(names))]
        check(setup, jsoncases.case("std", False, 0, False, names, qs))


def test_capacity_and_the_next_call(setup):
    import torch
    _attach(setup, "std")
    c = jsoncases.standard_cases()["orfs fastq"]
    want, want_off = host_format(setup, c)
    ix = setup["ix"]
    stage = api.JsonStage(ix, len(c["queries"]), len(want_off) - 1)
    try:
        with pytest.raises(abi.KaamerError) as e:   # one byte short: nothing is to be read, the needed size is reported
            run_stage(ix, c, len(want) - 1, stage=stage)
        assert e.value.code == abi.E_CAPACITY and e.value.counts == (len(want_off) - 1, len(want))
        got, off, rest = run_stage(ix, c, len(want), stage=stage)   # ... and the stage stays usable
        assert got == want and off.tolist() == want_off.tolist() and rest == b"\x55" * len(rest)
        torch.cuda.synchronize()
    finally:
        stage.close()
    small = api.JsonStage(ix, len(c["queries"]), len(want_off) - 2)   # one object too few
    try:
        with pytest.raises(abi.KaamerError) as e:
            run_stage(ix, c, len(want), stage=small)
        assert e.value.code == abi.E_CAPACITY and e.value.counts == (len(want_off) - 1, len(want))
        torch.cuda.synchronize()
    finally:
        small.close()


def test_no_subject_json_attached(setup, gpu_device):
    ix = api.Index.from_image(setup["tables"]["nofeat"][0].image(), gpu_device)
    try:
        assert ix.subject_json_info() == dict(table_bytes=0, entries=0, max_entry=0)
        with pytest.raises(abi.KaamerError) as e:
            run_stage(ix, jsoncases.standard_cases()["no features"], 4096)
        assert e.value.code == abi.E_ARG and "kaamer_index_attach_subject_json" in str(e.value)
    finally:
        ix.close()
