"""Inputs shared by tests/test_merge_host.py and tests/test_gpu_merge.py: a family-structured database cut into parts,
and small crafted pair sets, each with what the merged image must show.  Test infrastructure only."""
import ctypes as C
import os

import numpy as np

import mergeref
import tableref

N_DB = 300
DB_SEED = 61
COUNTERS = ("n_keys", "n_pairs", "n_buckets", "n_lists", "n_inline", "max_list", "arena_words", "max_protein_id", "n_displaced")
_cache = {}


def image_bytes(img, tmp_path, name="m.kgi"):
    """the saved file, header included"""
    p = os.path.join(str(tmp_path), name)
    img.save(p)
    with open(p, "rb") as f:
        b = f.read()
    os.unlink(p)
    return b


def same_bytes(a, b, tmp_path):
    ba, bb = image_bytes(a, tmp_path, "a.kgi"), image_bytes(b, tmp_path, "b.kgi")
    if ba != bb:
        x, y = np.frombuffer(ba, dtype=np.uint8), np.frombuffer(bb, dtype=np.uint8)
        assert len(x) == len(y), (len(x), len(y), a.stats(), b.stats())
        at = int(np.flatnonzero(x != y)[0])
        nb = a.stats()["n_buckets"]
        where = "header" if at < 4096 else ("buckets" if at < 4096 + nb * 64 else "arena")
        raise AssertionError("images differ first at byte %d (%s); %d bytes differ" % (at, where, int((x != y).sum())))


def db():
    """(buf, offs) of the whole database; protein p has id p"""
    from kaamer_amd import workload
    if "db" not in _cache:
        _cache["db"] = workload.make_db(N_DB, seed=DB_SEED)
    return _cache["db"]


def cut(n_parts):
    """the database in n_parts runs of consecutive proteins -> [((buf, offs), ids)]"""
    buf, offs = db()
    n = len(offs) - 1
    edges = [n * i // n_parts for i in range(n_parts + 1)]
    out = []
    for a, b in zip(edges[:-1], edges[1:]):
        o = offs[a:b + 1]
        out.append(((buf[int(o[0]):int(o[-1])].copy(), (o - o[0]).astype(np.uint64)), np.arange(a, b, dtype=np.uint32)))
    return out


def part_images(api, n_parts, shard=0, n_shards=1, load_factor=0.5, device=None):
    return [api.Image.from_proteins(packed=p, ids=ids, shard=shard, n_shards=n_shards, load_factor=load_factor, device=device)
            for p, ids in cut(n_parts)]


def merged_by_definition(api, imgs, tmp_path, load_factor):
    """kaamer_image_build_pairs(E(img_0) ++ E(img_1) ++ ...): the specification of the merge"""
    keys, ids = mergeref.enumerate_images(imgs, tmp_path)
    st = imgs[0].stats()
    return api.Image.from_pairs(keys, ids, shard=st["shard"], n_shards=st["n_shards"], load_factor=load_factor)


def _from(api, pairs, load_factor=0.5):
    return api.Image.from_pairs(np.array([p[0] for p in pairs], np.uint32), np.array([p[1] for p in pairs], np.uint32), load_factor=load_factor)


def wrap_keys():
    """15 keys for a table of two buckets at load factor 0.95 (15 / 7.6 + 1): twelve whose home is bucket 1, the last one,
    so four of them go on at bucket 0, and three whose home is bucket 0"""
    home1 = [k for k in range(1000, 3000) if tableref._home(k, 1, 2) == 1][:12]
    home0 = [k for k in range(1000, 3000) if tableref._home(k, 1, 2) == 0][:3]
    return home1, home0


def crafted(api):
    """-> [(name, [images], load factor, {key: merged id list}, {counter: value})]"""
    K1, K2, K3 = 0x01234567, 0x0ABCDEF0, 0x00000042
    BIG = 0x80000005
    home1, home0 = wrap_keys()
    wrap_a = [(k, 1) for k in home1[:7]] + [(k, 2) for k in home0[:2]]
    wrap_b = [(k, 3) for k in home1[5:]] + [(home0[2], 4)]
    wrap_exp = {k: [1] for k in home1[:5]}
    wrap_exp.update({k: [1, 3] for k in home1[5:7]})
    wrap_exp.update({k: [3] for k in home1[7:]})
    wrap_exp.update({home0[0]: [2], home0[1]: [2], home0[2]: [4]})
    empty = []
    return [
        ("inline in both, same id", [_from(api, [(K1, 5)]), _from(api, [(K1, 5)])], 0.5, {K1: [5]}, dict(n_inline=1, n_lists=0, n_pairs=1)),
        ("inline in both, other id", [_from(api, [(K1, 5)]), _from(api, [(K1, 9)])], 0.5, {K1: [5, 9]}, dict(n_inline=0, n_lists=1, n_pairs=2)),
        ("superset", [_from(api, [(K1, 1), (K1, 2), (K1, 3)]), _from(api, [(K1, 2), (K1, 3)])], 0.5, {K1: [1, 2, 3]}, dict(n_lists=1, n_pairs=3)),
        ("a shared list whose keys diverge", [_from(api, [(K1, 1), (K1, 2), (K2, 1), (K2, 2)]), _from(api, [(K2, 3)])], 0.5,
         {K1: [1, 2], K2: [1, 2, 3]}, dict(n_lists=2, n_pairs=5)),
        ("two lists that become equal", [_from(api, [(K1, 1), (K1, 2), (K2, 1), (K2, 3)]), _from(api, [(K1, 3), (K2, 2)])], 0.5,
         {K1: [1, 2, 3], K2: [1, 2, 3]}, dict(n_lists=1, n_pairs=6, arena_words=8)),
        ("a single id of 2^31 and more", [_from(api, [(K1, BIG)]), _from(api, [(K2, 7)])], 0.5, {K1: [BIG], K2: [7]},
         dict(n_inline=1, n_lists=1, max_protein_id=BIG)),
        ("empty with non-empty", [_from(api, empty), _from(api, [(K3, 1), (K1, 2), (K1, 4)])], 0.5, {K3: [1], K1: [2, 4]}, dict(n_keys=2, n_pairs=3)),
        ("non-empty with empty", [_from(api, [(K3, 1), (K1, 2), (K1, 4)]), _from(api, empty)], 0.5, {K3: [1], K1: [2, 4]}, dict(n_keys=2, n_pairs=3)),
        ("two empty images", [_from(api, empty), _from(api, empty)], 0.5, {K1: []}, dict(n_keys=0, n_pairs=0, n_buckets=1, arena_words=4)),
        ("two buckets that wrap", [_from(api, wrap_a, 0.95), _from(api, wrap_b, 0.95)], 0.95, wrap_exp, dict(n_keys=15, n_buckets=2)),
    ]


def check_crafted(case, merged, tmp_path):
    name, _, _, exp, counters = case
    for k, ids in exp.items():
        assert merged.get(k).tolist() == ids, (name, hex(k))
    st = merged.stats()
    assert {c: st[c] for c in counters} == counters, (name, st)
    if name == "two buckets that wrap":
        t = tableref.table_of(merged, tmp_path, "wrap.kgi")
        _, walked, wrapped = t.walk(np.array(sorted(exp), np.uint32))
        assert wrapped.any() and st["n_displaced"] >= 4, name


def _slot_words(img):
    """the slots of a live image as a writable uint32 view (kaamer_image: header page, then the two array pointers)"""
    h = img._h.value
    nb = img.stats()["n_buckets"]
    buckets = C.c_void_p.from_address(h + 4096).value
    arena = C.c_void_p.from_address(h + 4096 + 8).value
    return (np.ctypeslib.as_array(C.cast(buckets, C.POINTER(C.c_uint32)), shape=(nb * 16,)),
            np.ctypeslib.as_array(C.cast(arena, C.POINTER(C.c_uint32)), shape=(img.stats()["arena_words"],)))


def bad_reference_cases(img):
    """yields after pointing a list reference of `img` outside its arena, by offset and by count; puts the words back"""
    slots, arena = _slot_words(img)
    at = next(i for i in range(0, len(slots), 2) if slots[i] != 0xFFFFFFFF and not (slots[i + 1] & 0x80000000))
    val = int(slots[at + 1])
    slots[at + 1] = len(arena) // 4 + 3
    yield "offset"
    slots[at + 1] = val
    cnt = int(arena[val * 4])
    arena[val * 4] = len(arena)
    yield "count"
    arena[val * 4] = cnt
