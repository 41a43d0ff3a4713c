"""The device FASTQ reader (parse_text.hip.inc) against the host reader (kaamer_parse_fastq) on the same bytes: record
count, every sequence, the offsets, and the name and sequence spans resolved against the text."""
import random

import numpy as np
import pytest

import scancases
from kaamer_amd import abi, api

pytestmark = pytest.mark.gpu

ALPHABET = "@ACNax+\r\n!G"
SEED = 20261003


@pytest.fixture(scope="module")
def geo(klib):
    g = api.text_parser_geometry()
    # the boundary cases below are built from these; they are what the kernels are compiled with
    assert g["piece"] == 16 and g["wave_step"] == 64 * g["piece"] and g["tile"] % g["wave_step"] == 0 and g["lines"] >= 64
    return g


@pytest.fixture(scope="module")
def parser(klib, gpu_device, geo):
    p = api.TextParser(4 * geo["tile"] + 200000, device=gpu_device)
    yield p
    p.close()


def _host(text):
    h = abi.C.c_void_p()
    abi.check(abi.lib().kaamer_parse_fastq(text, len(text), abi.C.byref(h)))
    try:
        seqs, offs, size, names, noff, plus = api._reads_to_arrays(h)
    finally:
        abi.lib().kaamer_reads_free(h)
    return seqs, offs, [names[int(noff[i]):int(noff[i + 1])] for i in range(len(size))]


def _check(parser, text):
    text = bytes(text)
    seqs, offs, names = _host(text)
    got = parser.parse(text)
    n = len(names)
    assert len(got["spans"]) == n, (len(got["spans"]), n)
    assert got["offsets"].tolist() == offs.tolist()
    assert bytes(got["seqs"]) == bytes(seqs)
    sb = bytes(seqs)
    for i, s in enumerate(got["spans"]):
        so, sl, no, nl = int(s["seq_off"]), int(s["seq_len"]), int(s["name_off"]), int(s["name_len"])
        assert so + sl <= len(text) and no + nl <= len(text)
        assert text[so:so + sl] == sb[int(offs[i]):int(offs[i + 1])], i
        assert text[no:no + nl] == names[i], i
    lines = text.split(b"\n")
    assert got["n_lines"] == len(lines) - (1 if lines[-1] == b"" else 0)
    return n


def _rec(name, seq, eol=b"\n"):
    return b"@" + name + eol + seq + eol + b"+" + eol + b"I" * len(seq) + eol


def _nt(rng, n):
    return bytes(rng.choice(b"ACGTNacgtn") for _ in range(n))


HAND = {
    "empty text": (b"", 0),
    "one line, final newline": (b"ACGT\n", 1),
    "one line, no final newline": (b"ACGT", 1),
    "one record, no final newline": (b"@r\nACGT\n+\nIIII", 1),
    "CRLF throughout": (b"@r1 x\r\nACGT\r\n+\r\nIIII\r\n@r2\r\nGGCC\r\n+\r\nIIII\r\n", 2),
    "a line that is only CR": (b"@r\n\r\nACGT\n\r\n+\nIIII\n\r", 1),
    "blank lines": (b"\n\n@r\n\nACGT\n\n\n+\nIIII\n\n@s\nGG\n\n", 2),
    "H H S": (b"@first\n@second\nACGT\n", 1),
    "S before any H": (b"ACGT\n@r\nGG\n", 2),
    "S S": (b"@r\nACGT\nGGCC\n+\n!!!!\n", 1),
    "H directly after H at the end": (b"@r\nACGT\n@s\n@t\n", 1),
    "quality line starting with @": (b"@r\nACGT\n+\n@III\n@s\nGG\n+\nII\n", 2),
    "quality line of only ACGTN": (b"@r\nACGT\n+\nNNNN\n@s\nGG\n+\nII\n", 2),
    "lower-case sequence": (b"@r\nacgtn\n+\nIIIII\n", 1),
    "bytes 0x00 and >= 0x80 inside a line": (b"@r\x00\xff\nAC\x00GT\nACGT\n+\nII\x80I\nAC\xc1T\n", 1),
    "@ alone on a line": (b"@\nACGT\n+\nIIII\n", 1),
    "CR inside a line": (b"@r\nAC\rGT\nGG\r\r\nTT\r\n", 1),
    "a sequence line with a trailing CR at the end of the text": (b"@r\nACGT\r", 1),
    "letters next to the alphabet": (b"@r\nACGT\n@s\nACGU\n@t\nBCGT\n@u\n`CGT\n@v\nAC{T\n@w\nAC@T\n", 1),
}


@pytest.mark.parametrize("case", sorted(HAND))
def test_hand_cases(parser, case):
    text, n = HAND[case]
    assert _check(parser, text) == n


def test_line_lengths_at_the_tile_edges(parser, geo):
    """sequence lines one below, at and one above a lane's piece, a wave's step and a workgroup's tile, and one of 70 000
    bytes.  The kernels classify and copy by position, not per line (kaamer_text_parser_geometry): there is no lane-to-wave
    switch, the wave step is where one would be."""
    rng = random.Random(SEED)
    lens = [15, 16, 17, 63, 64, 65, 1023, 1024, 1025]
    for edge in (geo["wave_step"], geo["tile"]):
        lens += [edge - 1, edge, edge + 1]
    lens.append(70000)
    both = b""
    for ln in lens:
        one = _rec(b"len%d" % ln, _nt(rng, ln))
        assert _check(parser, one) == 1
        spoiled = bytearray(one)                 # the same line with its last byte outside the alphabet: no record
        spoiled[one.index(b"\n") + ln] = ord("!")
        assert _check(parser, spoiled) == 0
        both += one
    assert _check(parser, both) == len(lens)     # all of them in one text: the gather crosses records at every alignment


def test_bytes_at_the_tile_edges(parser, geo):
    rng = random.Random(SEED + 1)
    T = geo["tile"]
    tail = _rec(b"b", _nt(rng, 40))
    # a '\n' as the last byte of a tile, and as the first byte of the next
    for at in (T - 1, T):
        text = b"@" + b"h" * (at - 1) + b"\n" + _nt(rng, 30) + b"\n" + tail
        assert text[at] == 10
        assert _check(parser, text) == 2
    # an '@' as the first byte of a tile: the line it opens is a header
    text = b"@a\n" + _nt(rng, T - 4) + b"\n" + tail
    assert text[T] == ord("@") and text[T - 1] == 10
    assert _check(parser, text) == 2
    # ... and in mid-line there: the line is no sequence
    text = b"@a\n" + _nt(rng, T - 3) + b"@" + _nt(rng, 5) + b"\n" + tail
    assert text[T] == ord("@")
    assert _check(parser, text) == 1
    # a '\r' and its '\n' on either side of a tile edge, and of a piece edge
    for edge in (T, geo["piece"] * 3, geo["wave_step"]):
        text = b"@a\n" + _nt(rng, edge - 4) + b"\r\n" + tail
        assert text[edge - 1] == 13 and text[edge] == 10
        assert _check(parser, text) == 2
        text = b"@a\n" + _nt(rng, edge - 4) + b"\r"        # ... and the '\r' as the last byte of the text
        assert _check(parser, text) == 1
        text = b"@a\n" + _nt(rng, edge - 4) + b"\rA\n"     # ... and a '\r' that no '\n' follows
        assert _check(parser, text) == 0
    # a total length one below, at and one above a tile multiple, the last line unterminated
    for k in (1, 2):
        for d in (-1, 0, 1):
            n = k * T + d
            text = _rec(b"x", _nt(rng, 100)) * 60
            text = text[:n - 50] if len(text) >= n - 50 else text
            text += b"@last\n" + _nt(rng, n - len(text) - 6)
            assert len(text) == n
            _check(parser, text)


def test_line_blocks(parser, geo):
    """records whose header, sequence and closing header lie in different blocks of lines, and runs of ignored lines longer
    than a block"""
    rng = random.Random(SEED + 2)
    L = geo["lines"]
    for gap in (L - 2, L - 1, L, L + 1, 2 * L + 5):
        blank = b"\n" * gap
        assert _check(parser, b"@a\n" + blank + b"ACGT\n" + blank + b"@b\nGG\n") == 2
        assert _check(parser, b"@a\n" + blank + b"ACGT\n" + blank + b"GGCC\n" + blank) == 1      # S ... S: the last one
        assert _check(parser, b"ACGT\n" + blank + b"!\n" * gap + b"@b\n") == 1                    # S before any H, H far behind
    for n in (L // 4 - 1, L // 4, L // 4 + 1, L // 2 + 1):   # four lines per record: the block edge falls on every line kind
        text = b"".join(_rec(b"r%d" % i, _nt(rng, 20 + i % 7)) for i in range(n))
        for lead in (b"", b"\n", b"\n\n", b"\n\n\n"):
            assert _check(parser, lead + text) == n


def test_fuzz(parser):
    rng = random.Random(SEED)
    n_rec = 0
    for it in range(300):
        n = rng.randrange(0, 3001)
        weights = [1] * len(ALPHABET)
        weights[ALPHABET.index("\n")] = rng.choice([1, 2, 4])
        for c in "ACNaG":
            weights[ALPHABET.index(c)] = rng.choice([1, 3, 8])
        text = "".join(rng.choices(ALPHABET, weights, k=n)).encode("latin-1")
        try:
            n_rec += _check(parser, text)
        except AssertionError:
            print("fuzz text %d: %r" % (it, text))
            raise
    assert n_rec > 1000


def test_capacity(klib, gpu_device):
    rng = random.Random(SEED + 3)
    text = b"".join(_rec(b"r%d" % i, _nt(rng, 30)) for i in range(100))
    p = api.TextParser(len(text), max_records=99, device=gpu_device)
    try:
        with pytest.raises(abi.KaamerError) as e:
            p.parse(text)
        assert e.value.code == abi.E_CAPACITY and "records" in str(e.value)
        assert _check(p, text[:text.rindex(b"@")]) == 99     # usable afterwards, and 99 records fit
        with pytest.raises(abi.KaamerError) as e:
            p.parse(text)
        assert e.value.code == abi.E_CAPACITY
    finally:
        p.close()
    # the bound on lines (text / 16 + 4 records + 1024): a text of nothing but short lines
    many = b"A\n" * 4000
    p = api.TextParser(len(many), max_records=10, device=gpu_device)
    try:
        with pytest.raises(abi.KaamerError) as e:
            p.parse(many)
        assert e.value.code == abi.E_CAPACITY and "lines" in str(e.value)
        assert _check(p, b"@r\nACGT\n") == 1
    finally:
        p.close()
    with pytest.raises(abi.KaamerError) as e:
        api.TextParser(1 << 32, max_records=1, device=gpu_device)
    assert e.value.code == abi.E_ARG


# ---- the second round of the one-workgroup scans: more than 1024 tiles of text, more than 1024 blocks of lines ----

@pytest.fixture(scope="module")
def big_parser(klib, gpu_device, geo):
    """a parser for texts of up to 2050 tiles and two rounds of line blocks"""
    assert geo["lines"] == scancases.ROUND == 1024       # the scans' workgroups have as many threads as a block has lines
    p = api.TextParser(2050 * geo["tile"], max_records=4096, device=gpu_device, max_lines=2 * scancases.ROUND * geo["lines"] + 4096)
    yield p
    p.close()


@pytest.fixture(scope="module")
def line_cases(geo):
    return scancases.line_block_cases("fastq", geo["lines"])


@pytest.mark.parametrize("n_tiles", [1024, 1025, 2049])
def test_more_tiles_than_one_round_of_the_tile_scan(big_parser, geo, n_tiles):
    """pt_tile_scan_kernel takes 1024 tiles per round and carries the lines before them into the next: 1024 tiles are one
    full round, 1025 a second round of one tile, 2049 a third.  Where a round ends, a '\\n' is the last byte of the tile
    before and another the first byte of the next, with records on both sides: every line base of the later round is
    wrong unless the carry is right."""
    text, edges, n_rec = scancases.tiles_text("fastq", geo["tile"], n_tiles)
    rounds = (n_tiles + scancases.ROUND - 1) // scancases.ROUND
    assert (len(text) + geo["tile"] - 1) // geo["tile"] == n_tiles and rounds == {1024: 1, 1025: 2, 2049: 3}[n_tiles]
    assert len(edges) == max(rounds - 1, 1) and all(text[e - 1:e + 1] == b"\n\n" for e in edges) and not text.endswith(b"\n")
    if rounds > 1:
        assert [e // geo["tile"] for e in edges] == [scancases.ROUND * k for k in range(1, rounds)]
    assert len(text) <= big_parser.max_text_bytes and 100 < n_rec < 300
    assert _check(big_parser, text) == n_rec


@pytest.mark.parametrize("case", scancases.LINE_CASES)
def test_more_line_blocks_than_one_round_of_the_block_scan(big_parser, geo, line_cases, case):
    """pt_block_scan_kernel takes 1024 blocks of lines per round: the record and byte bases, the nearest header before a
    block and the class of the lines around it cross from one round into the other"""
    text, n_rec, blocks = line_cases[case]
    assert scancases.kernel_blocks(text, geo["lines"]) == blocks
    assert (blocks > scancases.ROUND) == (case != "B lines, the last one S")         # (that one fills one round to its last block)
    assert _check(big_parser, text) == n_rec


def test_line_capacity_behind_one_round(klib, gpu_device, geo):
    B = scancases.ROUND * geo["lines"]
    mark = b"@"
    text = scancases.lines_text(B + 2, True, {B - 1: mark + b"h", B: b"ACGT"})
    p = api.TextParser(len(text), max_records=16, device=gpu_device, max_lines=B + 1)
    try:
        with pytest.raises(abi.KaamerError) as e:
            p.parse(text)
        assert e.value.code == abi.E_CAPACITY and "lines" in str(e.value)
        assert _check(p, mark + b"r\nACGT\n") == 1                              # usable afterwards
        assert _check(p, scancases.lines_text(B, False, {B - 2: mark + b"h", B - 1: b"ACGT"})) == 1
    finally:
        p.close()
