"""kaamer_text_cut_fastq on the host: a FASTQ text cut before an '@' that opens a line parses, piece by piece, to the
records of the whole text (the chunk rule of the device reader, include/kaamer_hip.h).  CPU only."""
import random

import pytest

import pyref
from kaamer_amd import api

ALPHABET = "@ACNax+\r\n!G"
SEED = 20261003


def _cut(text):
    return api.text_cut_fastq(text)


def test_hand_cases(klib):
    assert _cut(b"") == 0
    assert _cut(b"@r1 ACGT") == 0                       # no '\n'
    assert _cut(b"@r1\nACGT\n+\nIIII\n") == 0           # '@' only at offset 0
    assert _cut(b"@a\nAC\r\n@b\nGT\n") == 7             # "\r\n@": the cut is behind the '\n'
    assert _cut(b"@a\nAC\n@") == 6                      # '@' as the last byte
    assert _cut(b"@a\nAC@GT\n+\nII@I\n") == 0           # '@' in mid-line only
    assert _cut(b"\n@") == 1                            # the smallest text with a cut
    assert _cut(b"@a\nAC\n+\n@@II\n@b\nGT\n") == 13     # the greatest one wins; a quality line that starts with '@' ...
    assert _cut(b"@a\nAC\n+\n@@II\n@b\nGT\n"[:13]) == 8  # ... is a cut too (the reader takes it for a header as well)
    assert klib.kaamer_text_cut_fastq(None, 0) == 0


def _pieces(text, budget):
    """the text cut as the file driver cuts it: read `budget` bytes, cut, carry the tail; without a cut read on"""
    out, at, n = [], 0, len(text)
    while at < n:
        want = budget
        while True:
            end = min(n, at + want)
            if end == n:
                cut = n - at
                break
            cut = _cut(text[at:end])
            if cut:
                break
            want += budget
        out.append(text[at:at + cut])
        at += cut
    return out


def _records(recs):
    return [(r["seq"], r["name"], r["size"]) for r in recs]


def test_pieces_parse_to_the_whole_text(klib):
    rng = random.Random(SEED)
    n_cut = 0
    for it in range(2000):
        n = rng.randrange(0, 400)
        weights = [1] * len(ALPHABET)
        weights[ALPHABET.index("\n")] = rng.choice([1, 2, 4])
        weights[ALPHABET.index("@")] = rng.choice([1, 2])
        text = "".join(rng.choices(ALPHABET, weights, k=n)).encode("latin-1")
        whole = api.parse_reads(text, "fastq")
        pieces = _pieces(text, rng.choice([1, 7, 16, 50]))
        assert b"".join(pieces) == text
        for p in pieces[1:]:
            assert p[:1] == b"@"
        for p in pieces[:-1]:
            assert p[-1:] == b"\n"
        n_cut += len(pieces) > 1
        got = []
        for p in pieces:
            got += api.parse_reads(p, "fastq")
        for i, r in enumerate(got):     # PlusStrand is the file's bookkeeping: 1 on the first record of the FILE
            r["plus"] = i == 0
        assert got == whole, (it, text)
        ref = pyref.get_queries_fastq(text.decode("latin-1"))
        assert _records(got) == [(r["seq"], r["name"], r["size"]) for r in ref], (it, text)
    assert n_cut > 1000   # (the budgets are small: most texts are cut)
