"""kaamer_search_text_top_flat: FASTQ text in, reported hits out, against the parent route for the same text
(kaamer_parse_fastq, then kaamer_search_batch_top_flat) field for field."""
import gzip

import numpy as np
import pytest

from kaamer_amd import abi, api, workload

pytestmark = pytest.mark.gpu

FIELDS = ("rep_query", "meta", "trim", "top_off", "top_pid", "top_kmatch", "top_first_pos", "orf_aa")


@pytest.fixture(scope="module")
def setup(klib, gpu_device):
    db = workload.make_db(1000)                      # DB-S
    reads = workload.make_reads(db, 2000, seed=11)
    text = bytes(workload.fastq_text(reads))
    ix = api.Index.from_image(api.Image.from_proteins(packed=db), gpu_device)
    recs = api.parse_reads(text, "fastq")
    assert len(recs) == 2000
    yield dict(ix=ix, text=text, recs=recs)
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
        assert text[int(s["seq_off"]):int(s["seq_off"]) + int(s["seq_len"])].decode("latin-1") == r["seq"]
        assert text[int(s["name_off"]):int(s["name_off"]) + int(s["name_len"])].decode("latin-1") == r["name"]


@pytest.mark.parametrize("seq_type", [abi.READS, abi.NUCLEOTIDE, abi.seq_type(abi.READS, 4)], ids=["reads", "nucleotide", "reads-code4"])
def test_text_equals_parsed_batch(setup, seq_type):
    ix, text, recs = setup["ix"], setup["text"], setup["recs"]
    want = ix.search_top([r["seq"] for r in recs], seq_type=seq_type)
    got = ix.search_text_top(text, seq_type=seq_type)
    assert want.n_reported > 100
    assert want.text_spans is None
    _same(got, want)
    _check_spans(got, text, recs)


def test_other_options_and_an_empty_text(setup):
    ix, text, recs = setup["ix"], setup["text"], setup["recs"]
    kw = dict(min_k_ratio=0.2, min_k_match=12, max_results=3)
    _same(ix.search_text_top(text, **kw), ix.search_top([r["seq"] for r in recs], seq_type=abi.READS, **kw))
    for t in (b"", b"@r\n+\nIIII\n"):
        got = ix.search_text_top(t)
        assert got.n_reported == 0 and got.text_spans is not None and len(got.text_spans) == 0
    part = text[:api.text_cut_fastq(text[:5000])]     # a text much smaller than the slot's buffers, after a larger one
    prec = api.parse_reads(part, "fastq")
    got = ix.search_text_top(part)
    _same(got, ix.search_top([r["seq"] for r in prec], seq_type=abi.READS))
    _check_spans(got, part, prec)


def test_refusals(setup):
    ix, text = setup["ix"], setup["text"]
    with pytest.raises(abi.KaamerError) as e:
        ix.search_text_top(b">p\nACGT\n", fmt="fasta")
    assert e.value.code == abi.E_ARG and "host reader" in str(e.value)
    with pytest.raises(abi.KaamerError) as e:
        ix.search_text_top(text, seq_type=abi.PROTEIN)
    assert e.value.code == abi.E_ARG and "PROTEIN" in str(e.value)
    with pytest.raises(abi.KaamerError) as e:
        ix.search_text_top(gzip.compress(text[:4000]))
    assert e.value.code == abi.E_ARG and "gzip" in str(e.value)
    with pytest.raises(abi.KaamerError) as e:
        ix.search_text_top(text, seq_type=abi.seq_type(abi.READS, 7))
    assert e.value.code == abi.E_ARG
    assert ix.search_text_top(text[:api.text_cut_fastq(text[:3000])]).n_queries > 0   # the slots are free again


def test_two_tickets_in_flight(setup):
    ix, text = setup["ix"], setup["text"]
    cut = api.text_cut_fastq(text[:len(text) // 2])
    a, b = text[:cut], text[cut:]
    one_a, one_b = ix.search_text_top(a), ix.search_text_top(b)
    ta = ix.submit_text_top(a)
    tb = ix.submit_text_top(b)
    got_b, got_a = tb.wait(), ta.wait()
    _same(got_a, one_a)
    _same(got_b, one_b)
    assert got_a.text_spans.tobytes() == one_a.text_spans.tobytes() and got_b.text_spans.tobytes() == one_b.text_spans.tobytes()
    assert len(got_a.text_spans) + len(got_b.text_spans) == 2000
    # a ticket nobody waits for gives its slot and its spans back
    ix.submit_text_top(a).discard()
    _same(ix.search_text_top(a), one_a)


# ---- the record bound of a slot's first parse is exceeded: the parse is repeated with grown bounds ----------------------------
@pytest.fixture(scope="module")
def growth(setup, gpu_device):
    """8 000 ten-byte records, then 200 ordinary reads: more records than the first bound of len / 32 + 1024.  Every call
    runs on a fresh index: a used slot keeps its larger parser and would not grow."""
    db = workload.make_db(1000)
    reads = workload.make_reads(db, 200, seed=12)
    text = b"@\nAC\n+\nII\n" * 8000 + bytes(workload.fastq_text(reads))
    recs = api.parse_reads(text, "fastq")
    assert len(recs) == 8200 and len(recs) > len(text) // 32 + 1024
    img = api.Image.from_proteins(packed=db)
    want = setup["ix"].search_top([r["seq"] for r in recs], seq_type=abi.READS)
    ix = api.Index.from_image(img, gpu_device)
    try:
        got = ix.search_text_top(text)
    finally:
        ix.close()
    return dict(img=img, text=text, recs=recs, want=want, got=got)


def test_fastq_record_bound_grows(growth):
    got = growth["got"]
    assert got.n_reported > 0
    _same(got, growth["want"])
    _check_spans(got, growth["text"], growth["recs"])


def test_record_bound_grows_on_inflated_text(growth, gpu_device):
    """the same text as BGZF blocks: the repeated parse reads a text that was inflated on the device, not uploaded"""
    import bgzfmake
    ix = api.Index.from_image(growth["img"], gpu_device)
    try:
        got = ix.search_bgzf_top(bgzfmake.bgzf_file(growth["text"], 4096))
    finally:
        ix.close()
    assert got.text == growth["text"]
    _same(got, growth["got"])
    assert got.text_spans.tobytes() == growth["got"].text_spans.tobytes()
    _check_spans(got, growth["text"], growth["recs"])
