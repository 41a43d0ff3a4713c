"""The device FASTA reader (parse_fasta.hip.inc) against the host reader (kaamer_parse_fasta) on the same bytes: record
count, offsets, every packed byte, the names through the spans, and the sequence span: the lines of
text[seq_off : seq_off + seq_len], CR dropped, trimmed and joined, are the packed sequence modulo the case rule."""
import random

import pytest

import scancases
from kaamer_amd import abi, api

pytestmark = pytest.mark.gpu

SPACE = b" \t\n\v\f\r"
ALPHABET = b">>AAcg*  \t\r\n\n\n\v\f\x85\xff"   # the cut test's alphabet plus two bytes >= 0x80
SEED = 20261019
MORE = b"\n>\nA\n"   # appended for upper_last = 1: a header closes whatever record is pending, then one more record


@pytest.fixture(scope="module")
def geo(klib):
    g = api.text_parser_geometry()
    assert g["piece"] == 16 and g["wave_step"] == 64 * g["piece"] and g["tile"] % g["wave_step"] == 0 and g["lines"] >= 64
    return g


@pytest.fixture(scope="module")
def parser(klib, gpu_device, geo):
    p = api.TextParser(4 * geo["tile"] + 200000, device=gpu_device)
    yield p
    p.close()


def _host(text, upper_last):
    data = text + MORE if upper_last else text
    h = abi.C.c_void_p()
    abi.check(abi.lib().kaamer_parse_fasta(data, len(data), abi.C.byref(h)))
    try:
        seqs, offs, size, names, noff, plus = api._reads_to_arrays(h)
    finally:
        abi.lib().kaamer_reads_free(h)
    n = len(size) - (1 if upper_last else 0)
    return bytes(seqs)[:int(offs[n])], [int(x) for x in offs[:n + 1]], [bytes(names[int(noff[i]):int(noff[i + 1])]) for i in range(n)]


def _upper(b):
    return bytes(c - 32 if 97 <= c <= 122 else c for c in b)


def _check(parser, text, upper_last=False):
    text = bytes(text)
    seqs, offs, names = _host(text, upper_last)
    got = parser.parse(text, fmt="fasta", upper_last=upper_last)
    n = len(names)
    assert len(got["spans"]) == n, (len(got["spans"]), n)
    assert [int(x) for x in got["offsets"]] == offs
    packed = bytes(got["seqs"])
    if packed != seqs:
        at = next(i for i in range(min(len(packed), len(seqs))) if packed[i] != seqs[i]) if len(packed) == len(seqs) else -1
        raise AssertionError("packed bytes differ: first at %d of %d / %d" % (at, len(packed), len(seqs)))
    for i, s in enumerate(got["spans"]):
        so, sl, no, nl = int(s["seq_off"]), int(s["seq_len"]), int(s["name_off"]), int(s["name_len"])
        assert so + sl <= len(text) and no + nl <= len(text)
        assert text[no:no + nl] == names[i], i
        lines = text[so:so + sl].split(b"\n")
        assert not any(ln[:1] == b">" for ln in lines[1:]), i   # (no header line inside; the first line may be " >x" trimmed)
        joined = b"".join((ln[:-1] if ln[-1:] == b"\r" else ln).strip(SPACE) for ln in lines)
        want = seqs[offs[i]:offs[i + 1]]
        assert joined == want or _upper(joined) == want, i
        assert sl >= 1 and text[so:so + 1] not in SPACE_SET and text[so + sl - 1:so + sl] not in SPACE_SET, i
    lines = text.split(b"\n")
    assert got["n_lines"] == len(lines) - (1 if lines[-1] == b"" else 0)
    return n


SPACE_SET = {bytes([c]) for c in SPACE}


def _both(parser, text):
    n = _check(parser, text, False)
    _check(parser, text, True)
    return n


HAND = {
    "empty text": (b"", 0),
    "headers only": (b">a\n>b\n>c\n", 0),
    "whitespace only": (b" \n\t\t\n\r\n\n \v\f \n", 0),
    "no final newline": (b">a\nACGT\nac", 1),
    "a header without final newline": (b">a\nACGT\n>b", 1),
    "CRLF": (b">a x\r\nACGT\r\nacgt\r\n>b\r\nGG\r\n", 2),
    "a line that is only CR": (b">a\n\r\nAC\n\r\nGT\n\r", 1),
    "H H S": (b">first\n>second\nACGT\n", 1),
    "S before any H": (b"ACGT\nGG\n>r\nTT\n", 2),
    "a header, whitespace lines, a header": (b">a\n \n\t\n\n>b\nAC\n", 1),
    "' >x' is a sequence line": (b">a\n >x\nAC\n", 1),
    "'>' inside a line": (b">a\nAC>GT\nA>\n", 1),
    "interior spaces and tabs kept": (b">a\n  A C\tG  T \t\n\tA  \n", 1),
    "a trailing '*'": (b">a\nMKV*\n>b\nmk*\n", 2),
    "bytes that are not trimmed": (b">a\n\x00AC\x00\n\x1cAC\x1c\n\x85AC\x85\n\xa0AC\xa0\n\xffAC\xff\n>b\n\x1d\n\x1e\x1f\n", 2),
    "a single record": (b">only\nacgtACGT\n", 1),
    "last two lower-case": (b">a\nAC\n>b\nacgt\nac\n>c\nggtt\n", 3),
    "last lower-case, a header behind it": (b">a\nacgt\n>b\nggtt\n>c\n", 2),
    "last lower-case, blank lines behind it": (b">a\nacgt\n>b\nggtt\n\n \n\r\n", 2),
    "CR inside a line": (b">a\nAC\rGT\r\r\n\rAC\n", 1),
    "empty header name": (b">\nAC\n>\r\nGT\n", 2),
    "lower-case bytes around z": (b">a\n`az{|}~@[\n>b\nAZ\n", 2),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(parser, name):
    text, n = HAND[name]
    assert _both(parser, text) == n


def _filler(n):
    """exactly n >= 0 bytes of whole lines: sequence lines of up to 60 bytes (a lone '\\n' when one byte is left)"""
    out = []
    while n > 0:
        k = min(n, 61)
        out.append((b"ACgtTGca" * 8)[:k - 1] + b"\n")
        n -= k
    return b"".join(out)


def _boundaries(geo):
    return [(name, k * geo[name] + d) for name in ("piece", "wave_step", "tile") for k in (1, 2) for d in (-1, 0, 1)]


def test_line_breaks_at_the_tiling(parser, geo):
    for _, at in _boundaries(geo):
        text = b">r\n" + _filler(at - 11) + b"ACGTacgt\n" + b"GGcc\n>s\nTT\n"
        assert text[at:at + 1] == b"\n"
        assert _both(parser, text) == 2
    t = geo["tile"]
    text = b">r\n" + _filler(t - 5 - 3) + b"ACGT\r\n" + b"GGcc\r\n>s\r\nTT\r\n"   # '\r' last in a tile, '\n' first in the next
    assert text[t - 1:t + 1] == b"\r\n"
    assert _both(parser, text) == 2


def test_trim_runs_across_the_tiling(parser, geo):
    for _, at in _boundaries(geo):
        lead = b">r\n" + _filler(at - 5 - 3) + b"  \t  ACgT \t \n" + b"GGcc\n>s\nTT\n"     # the first kept byte at `at`
        assert lead[at:at + 1] == b"A" and lead[at - 1:at] == b" "
        assert _both(parser, lead) == 2
        trail = b">r\n" + _filler(at - 4 - 3) + b" ACgT \t \r\n" + b"GGcc\n>s\nTT\n"      # the last kept byte at `at`
        assert trail[at:at + 1] == b"T" and trail[at + 1:at + 2] == b" "
        assert _both(parser, trail) == 2
        # a whitespace run that holds the boundary on a line that keeps one byte on either side
        wide = b">r\n" + _filler(at - 9 - 3) + b"a" + b" " * 17 + b"c\n>s\nTT\n"
        assert _both(parser, wide) == 2


def test_long_lines(parser, geo):
    t = geo["tile"]
    rng = random.Random(SEED)
    long_seq = b"A" + bytes(rng.choice(b"ACGTacgt ") for _ in range(2 * t + 35)) + b"c"
    assert _both(parser, b">r\n" + long_seq + b"\n>s\nac\n") == 2
    assert _both(parser, b">r\nACgt\n" + b" \t" * (t // 2 + 9) + b"\nggTT\n>s\nac\n") == 2     # whitespace only, inside one record
    assert _both(parser, b">" + b"n a m e " * (t // 8 + 3) + b"\nACgt\n>s\nac\n") == 2
    assert _both(parser, b"  " + long_seq + b"  \r\n") == 1


def test_records_across_blocks_of_lines(parser, geo):
    ln = geo["lines"]
    assert _both(parser, b">r\n" + b"a\n" * (2 * ln + 3) + b">s\ncc\n") == 2
    assert _both(parser, b">r\n" + b"\n" * (ln + 5) + b"ac\n" + b" \n" * (ln + 1) + b"gt\n>s\ncc\n") == 2
    assert _both(parser, b"".join(b">h%d\n" % i for i in range(ln + 7)) + b"acgt\n") == 1
    assert _both(parser, b"\n" * (3 * ln + 1)) == 0
    for d in (-1, 0, 1):
        # the record's first sequence line is line ln + d; its header is the last line of the block before (d = 0)
        head = b">a\nAC\n" + b"x\n" * (ln + d - 4) + b">b\n"
        assert head.count(b"\n") == ln + d - 1
        assert _both(parser, head + b"\n" + b"gg\ntt\n>c\nA\n") == 3
        # ... and a record whose lines continue across the block's end
        assert _both(parser, b">a\n" + b"x\n" * (ln + d - 2) + b"y\nz\n") == 1


def test_gather_piece_boundaries(parser, geo):
    text = b"".join(b">r%d\n%s\n" % (i, b"acgtACGTacgtACGTxyz"[:n]) for i, n in enumerate((1, 15, 16, 17, 1, 1, 16, 15, 17, 33, 1)))
    assert _both(parser, text) == 11
    assert _both(parser, b"a\n" * 1000) == 1                     # one-byte sequence lines only: 16 source lines per piece
    assert _both(parser, b"a\n\n \n" * 300 + b">x\n" + b"b\r\n" * 50) == 2
    # the start of the last record at every offset inside a piece
    for k in range(17):
        assert _both(parser, b">a\n" + b"a" * (16 + k) + b"\n>b\n" + b"c" * 40 + b"\n") == 2


def test_capacity(klib, gpu_device, geo):
    max_text = 4 * geo["tile"] + 200000
    p = api.TextParser(max_text, max_records=100, device=gpu_device)
    try:
        text = b"".join(b">r%d\nac\n" % i for i in range(101))
        with pytest.raises(abi.KaamerError) as e:
            p.parse(text, fmt="fasta")
        assert e.value.code == abi.E_CAPACITY and "records" in str(e.value)
        assert _both(p, text[:text.rindex(b">")]) == 100
        bound = max_text // 16 + 4 * 100 + 1024
        many = b">r\n" + b"a\n" * bound
        assert len(many) <= max_text
        with pytest.raises(abi.KaamerError) as e:
            p.parse(many, fmt="fasta")
        assert e.value.code == abi.E_CAPACITY and "lines" in str(e.value)
        assert _both(p, b">r\nacgt\n>s\ngg\n") == 2
    finally:
        p.close()
    # the line bound can be created larger than the FASTQ rule
    p = api.TextParser(max_text, max_records=100, device=gpu_device, max_lines=bound + 10)
    try:
        assert _both(p, many) == 1
    finally:
        p.close()


def test_a_parser_takes_both_formats(parser):
    fq = b"@r\nACGT\n+\nIIII\n"
    assert _both(parser, b">r\nacgt\n") == 1
    got = parser.parse(fq)
    assert bytes(got["seqs"]) == b"ACGT" and len(got["spans"]) == 1
    assert _both(parser, b">r\nacgt\n>s\ngg\n") == 2
    with pytest.raises(ValueError):
        parser.parse(fq, fmt="embl")


def test_fuzz(parser, geo):
    rng = random.Random(SEED)
    for _ in range(300):
        text = bytes(rng.choice(ALPHABET) for _ in range(rng.randint(0, 3000)))
        _check(parser, text, rng.random() < 0.5)
    t = geo["tile"]
    for _ in range(20):
        out, size = [], 0
        while size < 2 * t:
            w = rng.choice((1, 7, 60, 80, 5000))
            if rng.random() < 0.08:
                ln = b">" + bytes(rng.choice(b"abc >\t") for _ in range(rng.randint(0, w)))
            elif rng.random() < 0.05:
                ln = bytes(rng.choice(b" \t\r") for _ in range(rng.randint(0, w)))
            else:
                ln = bytes(rng.choice(b"ACGTacgtn \t*") for _ in range(w))
            ln += rng.choice((b"\n", b"\n", b"\r\n"))
            out.append(ln)
            size += len(ln)
        _check(parser, b"".join(out), rng.random() < 0.5)


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
    return scancases.line_block_cases("fasta", geo["lines"])


@pytest.mark.parametrize("n_tiles", [1024, 1025, 2049])
def test_more_tiles_than_one_round_of_the_tile_scan(big_parser, geo, n_tiles):
    """pt_tile_scan_kernel takes 1024 tiles per round and carries the lines before them into the next: 1024 tiles are one
    full round, 1025 a second round of one tile, 2049 a third.  Where a round ends, a '\\n' is the last byte of the tile
    before and another the first byte of the next, with records on both sides: every line base of the later round is
    wrong unless the carry is right."""
    text, edges, n_rec = scancases.tiles_text("fasta", geo["tile"], n_tiles)
    rounds = (n_tiles + scancases.ROUND - 1) // scancases.ROUND
    assert (len(text) + geo["tile"] - 1) // geo["tile"] == n_tiles and rounds == {1024: 1, 1025: 2, 2049: 3}[n_tiles]
    assert len(edges) == max(rounds - 1, 1) and all(text[e - 1:e + 1] == b"\n\n" for e in edges) and not text.endswith(b"\n")
    if rounds > 1:
        assert [e // geo["tile"] for e in edges] == [scancases.ROUND * k for k in range(1, rounds)]
    assert len(text) <= big_parser.max_text_bytes and 100 < n_rec < 300
    assert _both(big_parser, text) == n_rec


@pytest.mark.parametrize("case", scancases.LINE_CASES)
def test_more_line_blocks_than_one_round_of_the_block_scan(big_parser, geo, line_cases, case):
    """pf_block_scan_kernel takes 1024 blocks of lines per round: the record and byte bases, the nearest header before a
    block and the class of the lines around it cross from one round into the other"""
    text, n_rec, blocks = line_cases[case]
    assert scancases.kernel_blocks(text, geo["lines"]) == blocks
    assert (blocks > scancases.ROUND) == (case != "B lines, the last one S")         # (that one fills one round to its last block)
    assert _both(big_parser, text) == n_rec


def test_line_capacity_behind_one_round(klib, gpu_device, geo):
    B = scancases.ROUND * geo["lines"]
    mark = b">"
    text = scancases.lines_text(B + 2, True, {B - 1: mark + b"h", B: b"ACGT"})
    p = api.TextParser(len(text), max_records=16, device=gpu_device, max_lines=B + 1)
    try:
        with pytest.raises(abi.KaamerError) as e:
            p.parse(text, fmt="fasta")
        assert e.value.code == abi.E_CAPACITY and "lines" in str(e.value)
        assert _both(p, mark + b"r\nACGT\n") == 1                              # usable afterwards
        assert _both(p, scancases.lines_text(B, False, {B - 2: mark + b"h", B - 1: b"ACGT"})) == 1
    finally:
        p.close()
