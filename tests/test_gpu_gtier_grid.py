"""The G-tier launches of a search, sized from the last finished batch (search.hip: g_tier_grid).

kaamer_workspace_finish learns how many queries the finished batch sent to the G tier; behind a batch that sent none,
count_global_kernel and positions_global_kernel are launched with KAAMER_G_FLOOR workgroups instead of the full grid.  A
batch that overflows after a clean one (a "surprise") is then counted by the floor's workgroups alone, and must still be
exact.  Every batch here is compared with the oracle and with the same batch on a fresh workspace (nothing known: the
full grid): hit lists per query in protein-id order, lowest positions, and all of kaamer_counters.

The database: 4 800 proteins around one 20-residue motif (a query that holds it has 4 800 distinct hits: more than the
largest group table, GRP_MAX_TABLE, so it goes to the G tier and is counted in its LDS table: tests/gtierref.py) and 60
around another (a query that holds that one stays in its group table)."""
import numpy as np
import pytest

import gtierref
from kaamer_amd import abi
from test_gpu_protein import _from_ptr

gpu = pytest.mark.gpu
FLOOR = 2
# the completion count of count_global_kernel has eight sub-counters: fewer workgroups than that take part, exactly as
# many, more; and one item per workgroup, exactly one, many
N_ITEMS = sorted({1, 7, 8, 9, FLOOR - 1, FLOOR, FLOOR + 1, 8 * FLOOR + 3})
N_CLEAN = 24
BIG, SMALL = 4800, 60


@pytest.fixture(autouse=True)
def _floor(monkeypatch):
    monkeypatch.setenv("KAAMER_G_FLOOR", str(FLOOR))   # read when a workspace is created


@pytest.fixture(scope="module")
def world(klib, oracle, gpu_device):
    from kaamer_amd import api
    rng = np.random.default_rng(1701)
    big, small = gtierref._fill(rng, 20), gtierref._fill(rng, 20)
    db = gtierref.motif_family(rng, BIG, big) + gtierref.motif_family(rng, SMALL, small)
    w = dict(ix=api.Index.from_image(api.Image.from_proteins(db), gpu_device), oix=oracle.Index.from_proteins(db), oracle=oracle,
             over=[gtierref._fill(rng, 30) + big + gtierref._fill(rng, 30) for _ in range(4)],
             clean=[gtierref._fill(rng, 30) + small + gtierref._fill(rng, 30) for _ in range(5)] + [db[BIG + 7], gtierref._fill(rng, 80), b"ACDEF"],
             exp={}, fresh={})
    f = gtierref.Figures(oracle, w["oix"], w["over"][0])
    assert gtierref.GRP_MAX_TABLE < f.D == BIG and f.lds_holds()
    f = gtierref.Figures(oracle, w["oix"], w["clean"][0])
    assert f.D == SMALL <= gtierref.table_slots_for(f.size)
    return w


def _batch(w, n):
    """N_CLEAN queries that stay in their group tables and n that leave them, interleaved"""
    seqs = [w["clean"][i % len(w["clean"])] for i in range(N_CLEAN)]
    for j in range(n):
        seqs.insert((j * 7) % (len(seqs) + 1), w["over"][j % len(w["over"])])
    return seqs


def _expected(w, s):
    """(ids ascending, Kmatch, lowest position, PositionHits rows) of one query, from the oracle"""
    if s not in w["exp"]:
        O = w["oracle"]
        size = O.size_in_kmer(s)
        if size < 7:
            w["exp"][s] = (np.zeros(0, np.uint32), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, max(size, 0)), bool))
        else:
            pid, km, pos = w["oix"].search(s, want_positions=True)
            o = np.argsort(pid)
            w["exp"][s] = (pid[o], km[o], pos[o].argmax(axis=1), pos[o])
    return w["exp"][s]


def _workspace(w, max_seqs=64, **kw):
    from kaamer_amd import api
    return api.Workspace(w["ix"], 1 << 16, max_seqs, first_pos=1, max_hits=1 << 16, g_tier_slots=1 << 20, **kw)


def _enqueue(ws, seqs):
    import torch
    from kaamer_amd import api
    buf, offs = api.pack_sequences(seqs)
    d_buf, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(offs.view(np.int64)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    r = ws.search_device(d_buf.data_ptr(), d_off.data_ptr(), len(seqs), len(buf), stream=st)
    torch.cuda.synchronize()   # (the inputs may go once the batch has run)
    return r, st


def _read(w, r, seqs, positions=False):
    """the device-resident result -> per query (ids ascending, Kmatch, lowest position[, PositionHits rows]), counters"""
    n = len(seqs)
    off, cnt = _from_ptr(r.d_hit_off, n, np.uint64), _from_ptr(r.d_hit_cnt, n, np.uint32)
    out = []
    for q in range(n):
        a, c = int(off[q]), int(cnt[q])
        assert a + c <= int(r.hit_capacity)
        pid, km, fp = (_from_ptr(p + 4 * a, c, np.uint32) for p in (r.d_hit_pid, r.d_hit_kmatch, r.d_hit_first_pos))
        o = np.argsort(pid)
        row = [pid[o], km[o].astype(np.int64), fp[o].astype(np.int64)]
        if positions:
            size = w["oracle"].size_in_kmer(seqs[q])
            words = (max(size, 0) + 63) // 64
            bits = np.zeros((c, max(size, 0)), bool)
            if c and words:
                poff = _from_ptr(r.d_pos_off + 8 * a, c, np.uint64).astype(np.int64)
                lo, hi = int(poff.min()), int(poff.max()) + words
                blk = _from_ptr(r.d_pos_bits + 8 * lo, hi - lo, np.uint64)
                rows = blk[(poff - lo)[:, None] + np.arange(words)[None, :]]
                bits = np.unpackbits(np.ascontiguousarray(rows).view(np.uint8), axis=1, bitorder="little")[:, :size].astype(bool)
            row.append(bits[o])
        out.append(row)
    ctr = abi.Counters.from_buffer_copy(_from_ptr(r.d_counters, 10, np.uint64).tobytes()).as_dict()
    return out, ctr


def _fresh(w, n, positions=False):
    """batch n on a workspace that knows nothing (the full grid), once"""
    key = (n, positions)
    if key not in w["fresh"]:
        ws = _workspace(w, want_positions=positions)
        seqs = _batch(w, n)
        r, st = _enqueue(ws, seqs)
        ctr = ws.finish(st)
        got, dctr = _read(w, r, seqs, positions)
        assert ctr == dctr
        ws.close()
        w["fresh"][key] = (got, ctr)
    return w["fresh"][key]


def _check(w, n, got, ctr, positions=False):
    seqs = _batch(w, n)
    ref, ref_ctr = _fresh(w, n, positions)
    print("batch of %d queries, %d of them G-tier items: n_overflow %d, n_hits %d (fresh workspace: %d, %d), longest list read back %d"
          % (len(seqs), n, ctr["n_overflow"], ctr["n_hits"], ref_ctr["n_overflow"], ref_ctr["n_hits"], max(len(g[0]) for g in got)))
    assert len(got) == len(seqs) == len(ref)
    for q, s in enumerate(seqs):
        exp = _expected(w, s)
        for k in range(4 if positions else 3):
            assert np.array_equal(got[q][k], exp[k]), "batch of %d items, query %d, field %d: differs from the oracle" % (n, q, k)
            assert np.array_equal(got[q][k], ref[q][k]), "batch of %d items, query %d, field %d: differs from a fresh workspace" % (n, q, k)
    assert ctr == ref_ctr
    assert ctr["n_overflow"] == n     # (the entries of LIST_G: what the next launch is sized from)
    assert ctr["n_hits"] == sum(len(_expected(w, s)[0]) for s in seqs)


def _run(w, ws, n, finish=True, positions=False):
    seqs = _batch(w, n)
    r, st = _enqueue(ws, seqs)
    ctr = ws.finish(st) if finish else None
    got, dctr = _read(w, r, seqs, positions)
    assert ctr is None or ctr == dctr
    _check(w, n, got, dctr, positions)


@gpu
@pytest.mark.parametrize("n", N_ITEMS)
def test_clean_then_surprise(world, n):
    """a clean batch is finished (the next launch gets the floor), then a batch with n G-tier items; a further overflowing
    batch (the full grid again), a clean one, the surprise again; a last known batch shows that every one of them left
    the per-batch state clean"""
    ws = _workspace(world)
    for k in (0, n, 5, 0, n, 3):
        _run(world, ws, k)
    ws.close()


@gpu
def test_surprise_with_positions(world):
    """the same with PositionHits: positions_global_kernel at the floor, the batch finalized by finalize_kernel"""
    ws = _workspace(world, want_positions=True)
    for k in (0, FLOOR + 1, 0, 8 * FLOOR + 3, 1):
        _run(world, ws, k, positions=True)
    ws.close()


@gpu
def test_never_finished(world):
    """a workspace nobody finishes learns nothing: every launch has the full grid, the results are today's"""
    ws = _workspace(world)
    for k in (0, 3, 0, 9, 8 * FLOOR + 3, 0, 1):
        _run(world, ws, k, finish=False)
    ws.close()


@gpu
def test_bad_status_forgets(world):
    """a batch that ends with a status (more hits than the hit arrays hold) resets what the workspace knows; the batches
    after it are exact"""
    ws = _workspace(world, max_seqs=320)
    _run(world, ws, 0)
    r, st = _enqueue(ws, _batch(world, 1))
    ws.finish(st)
    n_bad = int(r.hit_capacity) // BIG + 2     # their lists alone exceed the hit arrays
    assert N_CLEAN + n_bad <= 320
    _run(world, ws, 0)                          # (the bad batch, too, comes after a clean one)
    r, st = _enqueue(ws, _batch(world, n_bad))
    with pytest.raises(abi.KaamerError) as e:
        ws.finish(st)
    assert e.value.code == abi.E_CAPACITY
    for k in (9, 0, FLOOR + 1):
        _run(world, ws, k)
    ws.close()
