"""Text calls of different response formats on one index with all three attaches: one slot that serves a TSV call, a JSON
call, an -aln TSV call and a plain call in turn (its stages and output buffers are reused across formats), the same with
first bounds so small that every formatted call is repeated once, and four concurrent callers of one format each.  Every
result equals the host formatter."""
import threading

import pytest

import tsvcases
import writercases as W
from kaamer_amd import api

pytestmark = pytest.mark.gpu

SEQUENCE = ("tsv", "json", "align+tsv", "plain", "json", "tsv")


@pytest.fixture(scope="module")
def setup(klib, gpu_device):
    table = tsvcases.standard_table()
    ix = api.Index.from_image(table.image(), gpu_device)
    ix.attach_proteins(table)
    ix.attach_subject_text(table)
    ix.attach_subject_json(table)
    yield dict(ix=ix, table=table)
    ix.close()


def test_one_slot_alternating_formats(setup):
    """one thread: every call takes slot 0"""
    ix, table = setup["ix"], setup["table"]
    texts = [W.queries(16 - k, seed=k) for k in range(len(SEQUENCE))]      # (another batch per call: nothing left over fits by chance)
    first = []
    for fmt, (text, seqs) in zip(SEQUENCE, texts):
        first.append(W.check(W.call(ix, fmt, text), fmt, text, seqs, table))
    for fmt, (text, seqs), want in zip(SEQUENCE, texts, first):
        ix.set_tsv_bounds(16, 1)       # before every call: a finished call leaves its own need as the slot's next bound,
        ix.set_json_bounds(16, 1)      # so that every formatted call is repeated once
        got = W.check(W.call(ix, fmt, text), fmt, text, seqs, table)
        assert (got.tsv, got.json) == (want.tsv, want.json) and (fmt == "plain" or len(got.tsv or got.json) > 16)
    ix.set_tsv_bounds(0, 0)
    ix.set_json_bounds(0, 0)


def test_four_concurrent_callers_of_four_formats(setup):
    ix, table = setup["ix"], setup["table"]
    texts = [W.queries(16, seed=7 + k) for k in range(4)]
    errors = []

    def work(fmt, text, seqs):
        try:
            for _ in range(3):
                W.check(W.call(ix, fmt, text), fmt, text, seqs, table)
        except BaseException as e:   # noqa: BLE001
            errors.append((fmt, e))
    threads = [threading.Thread(target=work, args=(fmt,) + t) for fmt, t in zip(W.FORMATS, texts)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
