"""Lookups in crowded bucket tables, on the CPU: the numpy restatement of the walk (tests/tableref.py) against the
oracle index and against kaamer_image_get (builder.cpp), on images of the host builder at load factors 0.5, 0.75, 0.9
and 0.95 and on some forty tiny tables (one, two and three buckets, a database without proteins).

Open addressing in 8-slot buckets: at load 0.5 one key in a hundred sits outside its home bucket and no lookup walks far;
at 0.95 one key in six does, absent keys walk for dozens of buckets and some for hundreds, and in a table of a few buckets a walk
passes the last bucket and goes on at bucket 0.  The expected ids do not depend on the load factor at all.

The databases, the queries and the seeds are fixed, and tests/test_gpu_crowded_tables.py searches the same images with
the same queries: what is asserted here about them (displaced share, longest walk, walks that wrap) is what keeps the
GPU tests from passing without entering the probe kernel's continuation path."""
import ctypes as C

import numpy as np
import pytest

import pyref
import tableref

LOADS = (0.5, 0.75, 0.9, 0.95)
DB_PROTEINS, DB_SEED = 3400, 41


def crowded_db():
    from kaamer_amd import workload
    return workload.make_db(DB_PROTEINS, seed=DB_SEED)


def query_windows(oracle, seqs):
    """-> (packed queries, keys of the windows the search looks up: the first SizeInKmer windows of every query whose
    SizeInKmer is 7 or more (search_protein.go:74-76), in batch order)"""
    packed = oracle.pack(seqs)
    sizes = np.array([oracle.size_in_kmer(s) for s in seqs], dtype=np.int64)
    sizes[sizes < 7] = 0
    return packed, tableref.encode_windows(packed[0], tableref.window_starts(packed[1], sizes))


def oracle_keys(oix):
    """the distinct keys the oracle index holds, ascending"""
    return np.unique((oix.pairs() >> np.uint64(32)).astype(np.uint32))


def oracle_lists(oracle, oix, keys):
    """what oracle.Index.get returns for every key (the same two calls of ko_index_get: the count, then the ids), the
    lists one behind the other, each ascending -> (counts, ids)"""
    f, h = oracle.lib().ko_index_get, oix._h
    cnt = np.array([f(h, k, None, 0) for k in keys.tolist()], dtype=np.int64)
    off = np.zeros(len(keys) + 1, dtype=np.int64)
    np.cumsum(cnt, out=off[1:])
    ids = np.zeros(int(off[-1]) + 1, dtype=np.uint32)
    base = ids.ctypes.data
    for k, o, c in zip(keys.tolist(), off[:-1].tolist(), cnt.tolist()):
        f(h, k, base + 4 * o, c)
    ids = ids[:-1]
    seg = np.repeat(np.arange(len(keys), dtype=np.int64), cnt)
    return cnt, ids[np.lexsort((ids, seg))]


def random_seqs(rng, n, lo, hi):
    alpha = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    return [bytes(alpha[rng.integers(0, 20, int(m))]) for m in rng.integers(lo, hi, n)]


def tiny_cases():
    """Forty small databases with fixed seeds -> [(packed db, load factor)]: the recipe of
    test_builder_device.py::test_runs_that_wrap_and_tiny_tables, one protein cut to 13, 21 and 28 residues at load 0.95
    (7, 15 and 22 keys: tables of one, two and three buckets with at most one or two free slots), no protein at all."""
    from kaamer_amd import workload
    rng = np.random.default_rng(77)
    out = []
    for case in range(27):
        n = int(rng.integers(1, 60))
        db = workload.make_db(n, seed=1000 + case, family=int(rng.integers(1, 6)))
        out.append((db, float(rng.choice([0.5, 0.8, 0.95]))))
    for seed in range(4):
        prot = workload.unpack(workload.make_db(1, seed=2000 + seed, family=1))[0]
        out += [(_pack([prot[:n_res]]), 0.95) for n_res in (13, 21, 28)]
    out.append((_pack([]), 0.95))
    return out


def _pack(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if seqs:
        offs[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    return np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(), offs


def tiny_queries(db, case):
    """the queries of tiny database `case`: its own proteins, mutants of them (5 % substitutions), and random sequences
    (which share no key with it: asserted where they are used)"""
    from kaamer_amd import workload
    own = workload.unpack(db)
    mutants = workload.unpack(workload.make_protein_queries(db, 12, seed=3000 + case)) if own else []
    return own, mutants, random_seqs(np.random.default_rng(4000 + case), 6, 30, 120)


def _get_all(klib, img, keys, counts):
    """kaamer_image_get for every key, the ids written one list behind the other -> (returned counts, ids)"""
    off = np.zeros(len(keys) + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    ids = np.full(int(off[-1]) + 1, 0xFFFFFFFF, dtype=np.uint32)
    base, h, f = ids.ctypes.data, img._h, klib.kaamer_image_get
    got = [f(h, k, C.c_void_p(base + 4 * o), c) for k, o, c in zip(keys.tolist(), off[:-1].tolist(), np.asarray(counts).tolist())]
    return np.array(got, dtype=np.int64), ids[:-1]


@pytest.fixture(scope="module")
def big(klib, oracle):
    """the database, the oracle index, its keys with their ids through oracle.Index.get (once), and absent keys"""
    from kaamer_amd import workload
    db = crowded_db()
    oix = oracle.Index.from_proteins(None, packed=db)
    keys = np.unique(tableref.db_window_keys(db))
    cnt, ids = oracle_lists(oracle, oix, keys)
    assert (cnt > 0).all()
    # absent keys: windows of mutated database proteins and of random sequences, minus what the oracle index holds
    seqs = workload.unpack(workload.make_protein_queries(db, 200, seed=DB_SEED + 1, subst=0.2))
    _, wk = query_windows(oracle, seqs)
    absent = np.setdiff1d(wk, oracle_keys(oix))[:12000]
    assert len(absent) >= 10000
    assert all(len(oix.get(k)) == 0 for k in absent.tolist())
    return dict(db=db, oix=oix, keys=keys, cnt=cnt, ids=ids, absent=absent)


@pytest.fixture(scope="module")
def tables(klib, big, tmp_path_factory):
    from kaamer_amd import api
    tmp = tmp_path_factory.mktemp("walk")
    out = {}
    for load in LOADS:
        img = api.Image.from_proteins(packed=big["db"], load_factor=load)
        out[load] = (img, tableref.table_of(img, tmp))
    return out


def test_numpy_encoding_equals_both_scalar_encoders(oracle):
    """tableref.encode_windows against tests/pyref.py and the oracle: windows of database proteins, and windows over
    every kind of byte the closed form treats apart -- the alphabet, 'U', '.', 'X', '*', lower case, bytes >= 0x80."""
    rng = np.random.default_rng(5)
    prot = crowded_db()[0][:6000]
    special = np.frombuffer(b"ACDEFGHIKLMNPQRSTUVWY" * 2 + b"X.*Uacdy-BZJO \x00\x7f\x80\x9c\xc1\xff", dtype=np.uint8)
    mixed = special[rng.integers(0, len(special), 6000)]
    buf = np.concatenate([prot, mixed, np.arange(256, dtype=np.uint8)])
    starts = np.arange(len(buf) - 6)
    keys = tableref.encode_windows(buf, starts)
    assert len(keys) >= 10000
    raw = bytes(buf)
    for c in b"X.*Ua\x80\xff":
        assert c in raw[6000:]
    assert keys.tolist() == [pyref.encode_kmer(raw[i:i + 7]) for i in starts.tolist()]
    assert keys.tolist() == [oracle.encode_kmer(raw[i:i + 7]) for i in starts.tolist()]
    assert tableref.encode_windows(b"YYYYYYY", [0]).tolist() == [0xE773B9D4]      # the largest key (kaamer_layout.h)


@pytest.mark.parametrize("load", LOADS)
def test_present_and_absent_keys_at_every_load(klib, big, tables, load):
    """Every key of the database is found and its ids are what oracle.Index.get returns; 10 000 keys the oracle index does
    not hold are not found; kaamer_image_get (the library's own host walk) says the same for both sets."""
    img, t = tables[load]
    keys, cnt = big["keys"], big["cnt"]
    assert len(keys) == img.stats()["n_keys"]
    val, walked, _ = t.walk(keys)
    assert (val != 0).all() and (walked >= 1).all()
    off, ids = t.ids_csr(val)
    assert np.array_equal(np.diff(off), cnt)
    assert np.array_equal(ids, big["ids"])                   # lists hold their ids ascending
    assert int((walked > 1).sum()) == img.stats()["n_displaced"]
    aval, awalked, _ = t.walk(big["absent"])
    assert (aval == 0).all() and (awalked >= 1).all()
    # the scalar walk of the helper agrees with the vectorised one
    for i in np.random.default_rng(1).integers(0, len(keys), 300).tolist():
        assert t.val(int(keys[i])) == int(val[i])
    assert all(t.val(int(k)) is None for k in big["absent"][:300])
    got, gids = _get_all(klib, img, keys, cnt)
    assert np.array_equal(got, cnt) and np.array_equal(gids, big["ids"])
    agot, _ = _get_all(klib, img, big["absent"], np.zeros(len(big["absent"]), dtype=np.int64))
    assert (agot == 0).all()


def test_walks_are_long_at_load_095(big, tables):
    """What the crowded images really look like (printed: pytest -s), and the thresholds the GPU tests rely on at load 0.95.

    Printed for this database (3 400 proteins, seed 41: 884 798 keys) -- present keys outside their home bucket and the
    longest walk of a present key; absent lookups that start in a full bucket, their mean and longest walk, in buckets:
        load 0.50, 221 200 buckets:  0.9 %,   6;   5.4 %,  1.06,   5
        load 0.75, 147 467 buckets:  6.1 %,  18;  32.9 %,  1.70,  18
        load 0.90, 122 889 buckets: 13.3 %, 114;  67.9 %,  7.03, 137
        load 0.95, 116 421 buckets: 16.6 %, 549;  83.2 %, 27.52, 556
    (The keys are placed first come, first served in ascending key order, which the hash makes a random order: a key
    placed while the table was still sparse sits at home, so the displaced share stays far below the share of full buckets.)
    Asserted at 0.95, a third below what was printed: displaced share > 0.11 (printed 0.166), longest walk of a present
    key > 366 buckets (printed 549), longest walk of an absent key > 370 buckets (printed 556)."""
    rows = {}
    for load in LOADS:
        _, t = tables[load]
        _, w, _ = t.walk(big["keys"])
        _, aw, _ = t.walk(big["absent"])
        rows[load] = (float((w > 1).mean()), int(w.max()), float((aw > 1).mean()), float(aw.mean()), int(aw.max()))
        print("load %.2f: %d keys in %d buckets; displaced %.3f, longest walk %d; absent: start full %.3f, mean walk %.2f, longest %d"
              % ((load, len(big["keys"]), t.nb) + rows[load]))
    share, longest, _, _, alongest = rows[0.95]
    assert share > 0.11 and longest > 366 and alongest > 370
    assert rows[0.5][0] < 0.05                         # and the default load factor shows none of it


def test_tiny_tables_and_walks_that_wrap(klib, oracle, tmp_path):
    """Forty tiny tables, every key and the windows of their queries: present keys are found with the oracle's ids, absent
    ones are not, kaamer_image_get agrees; tables of one, two and three buckets and an empty database are among them; and
    over the queries' windows at least one lookup of a present key and one of an absent key go on from the last bucket
    at bucket 0."""
    from kaamer_amd import api
    sizes, wrap_present, wrap_absent = set(), 0, 0
    cases = tiny_cases()
    assert len(cases) == 40
    for case, (db, load) in enumerate(cases):
        img = api.Image.from_proteins(packed=db, load_factor=load)
        t = tableref.table_of(img, tmp_path)
        oix = oracle.Index.from_proteins(None, packed=db)
        keys = np.unique(tableref.db_window_keys(db))
        assert len(keys) == img.stats()["n_keys"] and np.array_equal(keys, oracle_keys(oix))
        sizes.add((t.nb, len(keys)))
        val, walked, _ = t.walk(keys)
        assert (val != 0).all()
        exp = [np.sort(oix.get(k)) for k in keys.tolist()]
        off, ids = t.ids_csr(val)
        assert [ids[a:b].tolist() for a, b in zip(off[:-1], off[1:])] == [e.tolist() for e in exp], case
        assert [img.get(k).tolist() for k in keys.tolist()] == [e.tolist() for e in exp], case
        assert int((walked > 1).sum()) == img.stats()["n_displaced"]
        own, mutants, rnd = tiny_queries(db, case)
        _, wk = query_windows(oracle, own + mutants + rnd)
        present = np.isin(wk, keys)
        qval, qwalked, qwrapped = t.walk(wk)
        assert ((qval != 0) == present).all(), case
        assert all(len(img.get(k)) == 0 for k in wk[~present].tolist()), case
        assert (qwalked >= 1).all() and (qwalked <= t.nb).all()
        _, rk = query_windows(oracle, rnd)
        assert len(rk) > 100 and not np.isin(rk, keys).any()       # the random sequences share no key with the database
        wrap_present += int((qwrapped & present).sum())
        wrap_absent += int((qwrapped & ~present).sum())
    assert (1, 0) in sizes                                         # no protein: one bucket, every slot empty
    assert {nb for nb, _ in sizes} >= {1, 2, 3}
    assert any(nb == 1 and n == 7 for nb, n in sizes) and any(nb == 2 and n == 15 for nb, n in sizes)
    assert wrap_present >= 1 and wrap_absent >= 1, (wrap_present, wrap_absent)


def test_shard_tables_find_the_keys_they_own(klib, big, tmp_path):
    """Three shard images at load 0.95: every key is owned by exactly one shard (kh_shard_of), that shard's table finds
    it with the right ids through kh_home_bucket with n_shards = 3, the others skip it without reading a bucket."""
    from kaamer_amd import api
    keys = big["keys"]
    owner = tableref.shard_of_v(keys, 3)
    found = np.zeros(len(keys), dtype=np.int64)
    for s in range(3):
        img = api.Image.from_proteins(packed=big["db"], shard=s, n_shards=3, load_factor=0.95)
        t = tableref.table_of(img, tmp_path)
        val, walked, _ = t.walk(keys)
        mine = owner == s
        assert int(mine.sum()) == img.stats()["n_keys"]
        assert (val[mine] != 0).all() and (val[~mine] == 0).all() and (walked[~mine] == 0).all()
        assert float((walked[mine] > 1).mean()) > 0.11               # as crowded as the unsharded table
        off, ids = t.ids_csr(val[mine])
        assert np.array_equal(np.diff(off), big["cnt"][mine])
        assert np.array_equal(ids, big["ids"][np.repeat(mine, big["cnt"])])
        aval, awalked, _ = t.walk(big["absent"])
        assert (aval == 0).all() and ((awalked == 0) == (tableref.shard_of_v(big["absent"], 3) != s)).all()
        found += mine
    assert (found == 1).all()
