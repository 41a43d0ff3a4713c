"""CPU-side checks of the product library: it loads, exports every symbol the
header declares, and its host logic (builder, codec, filter) agrees with the
oracle.  No device calls here."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    src = open(os.path.join(ROOT, "include", "kaamer_hip.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def _declared_symbols():
    return sorted(set(re.findall(r"\b(kaamer_[a-z_0-9]+)\s*\(", _header())))


def _declared_arity():
    """{function: number of parameters} of every declaration in the header; (void) is none.  The callback typedefs are
    `(*name)(...)`, so their names are followed by ')' and do not match."""
    out = {}
    for name, params in re.findall(r"\b(kaamer_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", _header()):
        params = params.strip()
        assert name not in out, "%s is declared twice" % name
        out[name] = 0 if params in ("", "void") else params.count(",") + 1
    return out


HOST_ONLY = bool(os.environ.get("KAAMER_HOST_ONLY"))   # the sanitized CPU build holds the host sources only


def test_abi_arity_equals_the_header():
    """abi.SYMBOLS is built from named argument groups: every entry has as many argtypes as the header's declaration has
    parameters, and the header declares nothing else.  Needs the header's text and the table only."""
    from kaamer_amd import abi
    arity = _declared_arity()
    assert sorted(arity) == _declared_symbols() == sorted(abi.SYMBOLS)
    assert len(arity) >= 253
    # the geometry getters the tests build their boundary cases from: each fills one u32 array
    for n in ("kaamer_scan_geometry", "kaamer_text_parser_geometry", "kaamer_inflater_geometry", "kaamer_tsv_geometry", "kaamer_json_geometry"):
        assert arity[n] == 1 and abi.SYMBOLS[n][0] is None, n
    wrong = {n: (k, len(abi.SYMBOLS[n][1])) for n, k in arity.items() if k != len(abi.SYMBOLS[n][1])}
    assert not wrong, "header parameters vs argtypes: %s" % wrong
    for res, args in abi.SYMBOLS.values():
        assert isinstance(args, list)


@pytest.mark.skipif(HOST_ONLY, reason="host-only sanitized library")
def test_library_exports_every_declared_symbol(klib):
    from kaamer_amd import abi
    names = _declared_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(klib, n), "libkaamer_hip.so lacks %s" % n
    assert sorted(abi.SYMBOLS) == names, "abi.py and include/kaamer_hip.h disagree"
    assert klib.kaamer_abi_version() == 4
    from kaamer_amd import api
    g = api.scan_geometry()
    assert g == dict(block=1024, items=16, tile=16384, single_max=131072) and g["tile"] == g["block"] * g["items"]
    assert api.inflater_geometry()["scan_threads"] == 1024


def test_product_does_not_use_the_oracle():
    """No file of the product may import/link/execute anything under oracle/."""
    for d, _, files in os.walk(os.path.join(ROOT, "kaamer_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                txt = open(os.path.join(d, f), errors="replace").read()
                assert "oracle" not in txt.lower(), os.path.join(d, f)


def test_codec_host_matches_oracle(klib, oracle):
    import random
    rng = random.Random(2)
    alpha = "ACDEFGHIKLMNPQRSTUVWYBJOXZ*a-"
    for _ in range(5000):
        k = "".join(rng.choice(alpha) for _ in range(7)).encode()
        assert klib.kaamer_encode_kmer(k) == oracle.encode_kmer(k)
    for b in range(256):
        k = bytes([b]) * 7
        assert klib.kaamer_encode_kmer(k) == oracle.encode_kmer(k)


@pytest.mark.parametrize("n_shards", [1, 2, 8])
def test_builder_image_equals_oracle_index(klib, oracle, n_shards):
    from kaamer_amd import api, workload
    db = workload.make_db(300, seed=5)
    oi = oracle.Index.from_proteins(None, packed=db)
    pairs = oi.pairs()
    keys = np.unique(pairs >> 32).astype(np.uint32)
    imgs = [api.Image.from_proteins(packed=db, shard=s, n_shards=n_shards) for s in range(n_shards)]
    st = [im.stats() for im in imgs]
    assert sum(s["n_pairs"] for s in st) == len(pairs)
    assert sum(s["n_keys"] for s in st) == len(keys)
    rng = np.random.default_rng(0)
    for k in rng.choice(keys, 3000, replace=False):
        s = klib.kaamer_shard_of(int(k), n_shards)
        got = np.sort(imgs[s].get(int(k)))
        assert np.array_equal(got, oi.get(int(k)))
        for t in range(n_shards):
            if t != s:
                assert len(imgs[t].get(int(k))) == 0
    for k in (0, 1, 0x12345678, 0xE773B9D4, 0xFFFFFFFE):
        if k not in keys:
            assert all(len(im.get(k)) == 0 for im in imgs)


def test_builder_pairs_dedup_and_sharing(klib, oracle):
    from kaamer_amd import api
    # duplicates (makedb writes one version per window; indexdb de-duplicates: kv_store.go:284-305)
    keys = np.array([5, 5, 5, 9, 9, 7, 7, 7, 7, 11, 12, 12], dtype=np.uint32)
    ids = np.array([3, 3, 1, 2, 2, 4, 1, 4, 3, 0x80000005, 1, 3], dtype=np.uint32)
    img = api.Image.from_pairs(keys, ids)
    assert sorted(img.get(5).tolist()) == [1, 3]
    assert img.get(9).tolist() == [2]
    assert sorted(img.get(7).tolist()) == [1, 3, 4]
    assert img.get(11).tolist() == [0x80000005]          # id >= 2^31 cannot be stored inline
    assert sorted(img.get(12).tolist()) == [1, 3]
    st = img.stats()
    assert st["n_pairs"] == 9 and st["n_keys"] == 5 and st["n_inline"] == 1
    assert st["n_lists"] == 3                             # {1,3} stored once, shared by keys 5 and 12
    oi = oracle.Index.from_pairs(keys, ids)
    for k in (5, 7, 9, 11, 12, 13):
        assert np.array_equal(np.sort(img.get(k)), oi.get(k))


def test_builder_rejects_reserved_values(klib):
    from kaamer_amd import abi, api
    with pytest.raises(abi.KaamerError):
        api.Image.from_pairs([0xFFFFFFFF], [1])
    with pytest.raises(abi.KaamerError):
        api.Image.from_pairs([1], [0xFFFFFFFF])


def test_image_save_load_roundtrip(klib, tmp_path):
    from kaamer_amd import abi, api, workload
    db = workload.make_db(50, seed=9)
    img = api.Image.from_proteins(packed=db)
    p = tmp_path / "db.kaamerht"
    img.save(p)
    img2 = api.Image.load(p)
    assert img.stats() == img2.stats()
    k = int(klib.kaamer_encode_kmer(bytes(db[0][:7])))
    assert np.array_equal(img.get(k), img2.get(k)) and len(img.get(k)) >= 1
    # a truncated or padded file is refused at load time (the header drives allocations and device indexing)
    raw = p.read_bytes()
    for blob in (raw[:-4], raw + b"\0" * 4):
        t = tmp_path / "trunc"
        t.write_bytes(blob)
        with pytest.raises(abi.KaamerError) as e:
            api.Image.load(t)
        assert e.value.code == abi.E_FORMAT
    bad = tmp_path / "bad"
    bad.write_bytes(b"\0" * 8192)
    with pytest.raises(abi.KaamerError) as e:
        api.Image.load(bad)
    assert e.value.code == abi.E_FORMAT
    with pytest.raises(abi.KaamerError) as e:
        api.Image.load(tmp_path / "missing")
    assert e.value.code == abi.E_IO


def test_filter_and_sort_match_oracle(klib, oracle):
    import random
    rng = random.Random(4)
    for _ in range(300):
        n = rng.randint(0, 30)
        size = rng.randint(7, 400)
        pid = np.array(rng.sample(range(10000), n), dtype=np.uint32)
        km = np.array([rng.randint(1, size) for _ in range(n)], dtype=np.uint32)
        order = np.zeros(n, dtype=np.uint32)
        klib.kaamer_sort_hits(pid.ctypes.data, km.ctypes.data, n, order.ctypes.data)
        exp = sorted(range(n), key=lambda i: (-int(km[i]), int(pid[i])))
        assert order.tolist() == exp
        kms = np.ascontiguousarray(km[order])
        for opts in ((0.05, 10, 10), (0.3, 1, 5), (0.0, 0, 100)):
            assert klib.kaamer_filter_results(kms.ctypes.data, n, size, *opts) == \
                oracle.filter_results(kms.astype(np.int64), size, *opts)


@pytest.mark.skipif(HOST_ONLY, reason="host-only sanitized library")
def test_no_gpu_fails_loudly(klib):
    """Without a device the index cannot open: an error, never a CPU fallback."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from kaamer_amd import abi, api, workload
    img = api.Image.from_proteins(packed=workload.make_db(20, seed=1))
    with pytest.raises(abi.KaamerError) as e:
        api.Index.from_image(img, 0)
    assert e.value.code == abi.E_HIP


def test_readers_match_reference_restatement(klib):
    """GetQueriesFasta / GetQueriesFastq (search.go:222-412) incl. the quirks"""
    import random
    import pyref
    from kaamer_amd import api
    rng = random.Random(8)
    fasta = (">q1 first protein\nMKVLaagT\nACDEFGHIKL\n\n>q2\n  MELPNIMHPVAKLSTALAAALMLSGC*  \n>empty\n>q3 lower last\nmkvlaagtacdefgh\r\nik*\n")
    got = api.parse_reads(fasta, "fasta")
    exp = pyref.get_queries_fasta(fasta)
    assert [(g["seq"], g["name"], g["size"]) for g in got] == [(e["seq"], e["name"], e["size"]) for e in exp]
    assert got[0]["seq"] == "MKVLAAGTACDEFGHIKL" and got[-1]["seq"] == "mkvlaagtacdefghik*"   # last record keeps its case
    assert got[1]["size"] == len(got[1]["seq"]) - 7
    # Location.PlusStrand as the reader leaves it: true on the first record only (search.go:224-229 vs :297)
    assert [g["plus"] for g in got] == [e["plus"] for e in exp] == [True, False, False]
    for _ in range(50):
        recs = []
        for i in range(rng.randint(0, 6)):
            body = "".join(rng.choice("ACDEFGHIKLMNPQRSTVWYacdx* ") for _ in range(rng.randint(0, 90)))
            lines = [body[j:j + 30] for j in range(0, len(body), 30)] + ([""] if rng.random() < 0.3 else [])
            recs.append(">r%d desc\n" % i + "\n".join(lines))
        text = "\n".join(recs) + ("\n" if rng.random() < 0.5 else "")
        got = api.parse_reads(text, "fasta")
        exp = pyref.get_queries_fasta(text)
        assert [(g["seq"], g["name"], g["size"]) for g in got] == [(e["seq"], e["name"], e["size"]) for e in exp], text
    fastq = "@r1\nACGTNacgtn\n+\nIIIIIIIIII\n@r2 x\nACGTTTGA\n+r2\n@@@@IIII\n\n@r3\nACGU\n+\nIIII\n@r4\nGGGG\n+\nACGT\n"
    got = api.parse_reads(fastq, "fastq")
    exp = pyref.get_queries_fastq(fastq)
    assert [(g["seq"], g["name"], g["size"]) for g in got] == [(e["seq"], e["name"], e["size"]) for e in exp]
    assert api.parse_reads("", "fasta") == [] and api.parse_reads("", "fastq") == []


def test_set_best_start_codon_matches_oracle(klib, oracle):
    """dna.go:198-272 from hit_first_pos vs the oracle's literal PositionHits scan"""
    import ctypes as C
    import random
    rng = random.Random(5)
    for _ in range(400):
        n = rng.randint(21, 60)
        seq = ("".join(rng.choice("ACDEFGHIKLMNPQRSTVWY") for _ in range(n - 1)) + rng.choice(["*", "A"])).encode()
        size = oracle.size_in_kmer(seq)
        nh = rng.randint(1, 5)
        km = sorted((rng.randint(1, size) for _ in range(nh)), reverse=True)
        if rng.random() < 0.4 and nh > 1:
            km[1] = km[0]                                   # ties at the best score
        pos = np.zeros((nh, size), dtype=bool)
        for h in range(nh):
            pos[h, rng.sample(range(size), km[h])] = True
        starts = sorted(rng.sample(range(n), rng.randint(0, 4)))
        plus = rng.random() < 0.5
        sp0 = rng.randint(1, 500)
        t, sp, so = oracle.set_best_start_codon(km, pos, size, starts, plus, seq, sp0)
        kma = np.array(km, dtype=np.uint32)
        fpa = np.array([int(np.argmax(pos[h])) for h in range(nh)], dtype=np.uint32)
        sa = np.array(starts, dtype=np.int32)
        c_sp, c_so = C.c_int32(sp0), C.c_int32(size)
        got = klib.kaamer_set_best_start_codon(kma.ctypes.data, fpa.ctypes.data, nh, sa.ctypes.data if len(sa) else None,
                                               len(sa), int(plus), seq, len(seq), C.byref(c_sp), C.byref(c_so))
        assert (got, c_sp.value, c_so.value) == (t, sp, so)
