"""The order of the postings arena: lists sit in ascending rank, the rank of a list being the smallest
window index that refers to it -- proteins in input order, positions ascending, the minimum over every key that
shares the list.  A walk over the proteins' windows therefore meets the lists at strictly increasing offsets, one
right behind the other from unit 1 to the end of the arena.

The walk here is Python (tests/pyref.py for the key encoding) and resolves every key through the buckets of the
saved image; the ids behind every key are checked against the oracle index.  Host builder only: that the device
builder lands on the same bytes is tests/test_builder_device.py."""
import ctypes

import numpy as np
import pytest

import pyref
from tableref import EMPTY, INLINE, _Table, _image_bytes, _shard_of


def _check_walk_order(api, oracle, tmp_path, db, shard, n_shards):
    from kaamer_amd import workload
    img = api.Image.from_proteins(packed=db, shard=shard, n_shards=n_shards)
    st = img.stats()
    t = _Table(_image_bytes(img, tmp_path), st)
    oix = oracle.Index.from_proteins(None, packed=db)
    first_touch, seen, sizes, key_val = [], set(), [], {}
    for seq in workload.unpack(db):
        for i in range(len(seq) - pyref.KMER_SIZE + 1):
            key = pyref.encode_kmer(seq[i:i + pyref.KMER_SIZE])
            if n_shards > 1 and _shard_of(key, n_shards) != shard:
                continue
            if key not in key_val:
                v = t.val(key)
                assert v is not None and v != 0, "key %08x of a window is not in the table" % key
                key_val[key] = v
                # the ids behind the key are what the oracle index holds, ascending
                assert t.ids(v) == sorted(oix.get(key).tolist()), "ids of key %08x" % key
            v = key_val[key]
            if not (v & INLINE) and v not in seen:
                seen.add(v)
                first_touch.append(v)
                sizes.append(int(t.arena[v * 4]))
    assert len(key_val) == st["n_keys"]
    assert len(first_touch) == st["n_lists"] > 0
    # (1) the walk meets the lists at strictly increasing offsets
    assert all(a < b for a, b in zip(first_touch, first_touch[1:])), "first-touch offsets do not increase"
    # (2) no gaps, no overlaps: from unit 1, every list starts where the one before ends, the last ends the arena
    at = 1
    for v in first_touch:
        assert v == at, "list at unit %d, expected at %d" % (v, at)
        at += t.units(v)
    assert at * 4 == st["arena_words"]
    # padding words of every list are the empty id
    for v in first_touch:
        c = int(t.arena[v * 4])
        assert (t.arena[v * 4 + 1 + c:(v + t.units(v)) * 4] == EMPTY).all()
    # the database exercises what the order has to cope with: lists of 2-10 ids, and lists shared between keys
    n_list_keys = sum(1 for v in key_val.values() if not (v & INLINE))
    assert any(2 <= c <= 10 for c in sizes) and any(c > 3 for c in sizes)
    assert st["n_lists"] < n_list_keys, "no shared list in this database"
    return img, st


@pytest.mark.parametrize("shard,n_shards", [(0, 1), (0, 2), (1, 2)])
def test_lists_lie_in_protein_walk_order(klib, oracle, tmp_path, shard, n_shards):
    from kaamer_amd import api, workload
    db = workload.make_db(240, seed=17, family=8)   # families of 8 with 10-30 % substitutions: shared k-mers
    _check_walk_order(api, oracle, tmp_path, db, shard, n_shards)


def test_explicit_ids_do_not_change_the_order(klib, oracle, tmp_path):
    """The order follows the proteins' position in the input, not their ids."""
    from kaamer_amd import api, workload
    db = workload.make_db(120, seed=19, family=6)
    n = len(db[1]) - 1
    ids = np.random.default_rng(3).permutation(n).astype(np.uint32) * 5 + 2
    b = api.Image.from_proteins(packed=db, ids=ids)
    tb = _Table(_image_bytes(b, tmp_path), b.stats())
    seen, last = set(), 0
    for seq in workload.unpack(db):
        for i in range(len(seq) - pyref.KMER_SIZE + 1):
            v = tb.val(pyref.encode_kmer(seq[i:i + pyref.KMER_SIZE]))
            if v & INLINE or v in seen:
                continue
            seen.add(v)
            assert v > last
            last = v
    assert len(seen) == b.stats()["n_lists"] > 0


@pytest.mark.parametrize("shard,n_shards", [(0, 1), (1, 2)])
def test_relayout_first_touch_reproduces_a_built_image(klib, tmp_path, shard, n_shards):
    """kaamer_exp_relayout_first_touch (kept for bench.py) lays lists in the order the builders already use."""
    from kaamer_amd import abi, api, workload
    db = workload.make_db(200, seed=23, family=8)
    img = api.Image.from_proteins(packed=db, shard=shard, n_shards=n_shards)
    before = _image_bytes(img, tmp_path, "before.kgi")
    L = abi.lib()
    L.kaamer_exp_relayout_first_touch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    L.kaamer_exp_relayout_first_touch.restype = ctypes.c_int
    buf, offs = np.ascontiguousarray(db[0]), np.ascontiguousarray(db[1])
    abi.check(L.kaamer_exp_relayout_first_touch(img._h, buf.ctypes.data, offs.ctypes.data, len(offs) - 1))
    assert _image_bytes(img, tmp_path, "after.kgi") == before
    assert img.stats()["n_lists"] > 0
