"""kaamer_search_fasta_top_flat: FASTA text in, reported hits out, against the parent route for the same text
(kaamer_parse_fasta, then kaamer_search_batch_top_flat) field for field -- protein queries, contigs and two-line reads."""
import gzip

import numpy as np
import pytest

from kaamer_amd import abi, api, workload

pytestmark = pytest.mark.gpu

FIELDS = ("rep_query", "meta", "trim", "top_off", "top_pid", "top_kmatch", "top_first_pos", "orf_aa")
SPACE = b" \t\n\v\f\r"


def _fasta(names, seqs, width):
    out = []
    for n, s in zip(names, seqs):
        out.append(b">" + n + b"\n")
        out.extend(s[i:i + width] + b"\n" for i in range(0, len(s), width))
    return b"".join(out)


@pytest.fixture(scope="module")
def setup(klib, gpu_device):
    db = workload.make_db(3000)
    rng = np.random.default_rng(7)
    prot = workload.unpack(workload.make_protein_queries(db, 300, seed=31))
    prot[-1], prot[-2] = prot[-1].lower(), prot[-2].lower()       # the last record keeps its case, the one before does not
    reads = workload.unpack(workload.make_reads(db, 2400, seed=33))
    contigs, at = [], 0
    while at < len(reads):
        k = int(rng.integers(20, 200))                            # 3 - 30 kb
        contigs.append(b"".join(reads[at:at + k]))
        at += k
    texts = dict(
        protein=_fasta([b"p%d some description" % i for i in range(len(prot))], prot, 60),
        contigs=_fasta([b"contig_%d" % i for i in range(len(contigs))], contigs, 80),
        reads=_fasta([b"read/%d" % i for i in range(2000)], reads[:2000], 1 << 20))
    img = api.Image.from_proteins(packed=db)
    ix = api.Index.from_image(img, gpu_device)
    recs = {k: api.parse_reads(t, "fasta") for k, t in texts.items()}
    assert len(recs["protein"]) == 300 and 15 <= len(recs["contigs"]) <= 40 and len(recs["reads"]) == 2000
    assert recs["protein"][-1]["seq"].islower() and recs["protein"][-2]["seq"].isupper()
    yield dict(ix=ix, img=img, texts=texts, recs=recs)
    ix.close()


def _same(a, b):
    assert (a.n_queries, a.n_reported, a.max_results) == (b.n_queries, b.n_reported, b.max_results)
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f
    assert a.counters == b.counters


def _check_spans(top, text, recs):
    sp = top.text_spans
    assert sp is not None and len(sp) == len(recs)
    for s, r in zip(sp, recs):
        rng = text[int(s["seq_off"]):int(s["seq_off"]) + int(s["seq_len"])]
        assert b"".join(ln.strip(SPACE) for ln in rng.split(b"\n")).decode("latin-1").upper() == r["seq"].upper()
        assert text[int(s["name_off"]):int(s["name_off"]) + int(s["name_len"])].decode("latin-1") == r["name"]


CASES = {"protein": (abi.PROTEIN, 100), "contigs": (abi.NUCLEOTIDE, 100), "reads": (abi.READS, 100),
         "reads-code4": (abi.seq_type(abi.READS, 4), 100), "contigs-code11": (abi.seq_type(abi.NUCLEOTIDE, 11), 100)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_fasta_text_equals_parsed_batch(setup, case):
    seq_type, least = CASES[case]
    kind = case.split("-")[0]
    ix, text, recs = setup["ix"], setup["texts"][kind], setup["recs"][kind]
    want = ix.search_top([r["seq"] for r in recs], seq_type=seq_type)
    got = ix.search_fasta_top(text, seq_type=seq_type)
    assert want.n_reported > least and want.text_spans is None
    _same(got, want)
    _check_spans(got, text, recs)


def test_upper_last_and_other_options(setup):
    ix, text, recs = setup["ix"], setup["texts"]["protein"], setup["recs"]["protein"]
    seqs = [r["seq"] for r in recs]
    as_is = ix.search_fasta_top(text)
    upper = ix.search_fasta_top(text, upper_last=True)
    _same(upper, ix.search_top(seqs[:-1] + [seqs[-1].upper()], seq_type=abi.PROTEIN))
    assert upper.n_reported >= as_is.n_reported
    kw = dict(min_k_ratio=0.2, min_k_match=12, max_results=3)
    _same(ix.search_fasta_top(text, **kw), ix.search_top(seqs, seq_type=abi.PROTEIN, **kw))
    for t in (b"", b">only a header\n", b"\n \n"):
        got = ix.search_fasta_top(t)
        assert got.n_reported == 0 and got.text_spans is not None and len(got.text_spans) == 0


def test_a_small_text_after_a_large_one(setup):
    ix = setup["ix"]
    big, small = setup["texts"]["contigs"], setup["texts"]["protein"]
    ix.search_fasta_top(big, seq_type=abi.NUCLEOTIDE)
    part = small[:api.text_cut_fasta(small[:5000])]
    prec = api.parse_reads(part, "fasta")
    assert 3 < len(prec) < 40
    got = ix.search_fasta_top(part)
    _same(got, ix.search_top([r["seq"] for r in prec], seq_type=abi.PROTEIN))
    _check_spans(got, part, prec)


def test_one_byte_lines_grow_the_line_bound(setup, gpu_device):
    # a fresh index: its first slot's parser starts from the FASTQ line rule, which a text of one-byte lines exceeds --
    # the device reports KAAMER_E_CAPACITY, the bounds grow and the text (already on the device) is parsed again
    small = setup["texts"]["protein"]
    part = small[:api.text_cut_fasta(small[:20000])]
    prec = api.parse_reads(part, "fasta")
    narrow = _fasta([r["name"].encode() for r in prec], [r["seq"].encode() for r in prec], 1)
    assert narrow.count(b"\n") > len(narrow) // 16 + 4 * (len(narrow) // 32 + 1024) + 1024      # where a slot's bounds start
    ix2 = api.Index.from_image(setup["img"], gpu_device)
    try:
        got = ix2.search_fasta_top(narrow, upper_last=True)
        _same(got, setup["ix"].search_fasta_top(part, upper_last=True))
        _check_spans(got, narrow, prec)
    finally:
        ix2.close()


def test_two_tickets_in_flight(setup):
    ix, text = setup["ix"], setup["texts"]["reads"]
    cut = api.text_cut_fasta(text[:len(text) // 2])
    a, b = text[:cut], text[cut:]
    one_a, one_b = ix.search_fasta_top(a, seq_type=abi.READS, upper_last=True), ix.search_fasta_top(b, seq_type=abi.READS)
    ta = ix.submit_fasta_top(a, seq_type=abi.READS, upper_last=True)
    tb = ix.submit_fasta_top(b, seq_type=abi.READS)
    got_b, got_a = tb.wait(), ta.wait()
    _same(got_a, one_a)
    _same(got_b, one_b)
    assert got_a.text_spans.tobytes() == one_a.text_spans.tobytes() and got_b.text_spans.tobytes() == one_b.text_spans.tobytes()
    assert len(got_a.text_spans) + len(got_b.text_spans) == 2000
    ix.submit_fasta_top(a, seq_type=abi.READS).discard()          # a ticket nobody waits for gives its slot back
    _same(ix.search_fasta_top(a, seq_type=abi.READS, upper_last=True), one_a)


def test_refusals(setup):
    ix, text = setup["ix"], setup["texts"]["protein"]
    small = text[:api.text_cut_fasta(text[:3000])]
    with pytest.raises(abi.KaamerError) as e:
        ix.search_fasta_top(gzip.compress(small))
    assert e.value.code == abi.E_ARG and "gzip" in str(e.value)
    assert ix.search_fasta_top(small).n_queries > 0               # the slot works again
    for bad in (3, 7, abi.seq_type(abi.READS, 7), 1 << 16):
        with pytest.raises(abi.KaamerError) as e:
            ix.search_fasta_top(small, seq_type=bad)
        assert e.value.code == abi.E_ARG
        assert ix.search_fasta_top(small).n_queries > 0
    # the FASTQ text calls keep refusing FASTA and PROTEIN: FASTA has entry points of its own
    with pytest.raises(abi.KaamerError) as e:
        ix.search_text_top(small, fmt="fasta")
    assert e.value.code == abi.E_ARG and "host reader" in str(e.value)
    with pytest.raises(abi.KaamerError) as e:
        ix.submit_text_top(small, fmt="fasta")
    assert e.value.code == abi.E_ARG and "host reader" in str(e.value)
    with pytest.raises(abi.KaamerError) as e:
        ix.search_text_top(small, seq_type=abi.PROTEIN)
    assert e.value.code == abi.E_ARG and "PROTEIN" in str(e.value)
