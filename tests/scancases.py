"""Texts for the second round of the text parsers' one-workgroup scans (test_gpu_text_parse.py, test_gpu_fasta_parse.py):
pt_tile_scan_kernel goes round once per 1024 tiles of text, pt_block_scan_kernel and pf_block_scan_kernel once per 1024
blocks of lines.  The texts are built from the geometry the library reports; the same builders serve FASTQ ("@") and FASTA
(">").  Test infrastructure."""
import numpy as np

ROUND = 1024          # tiles, and blocks of lines, per round of the scans (their workgroup's threads)
LONG = 70000          # bytes of a long line


def _mark(fmt):
    return {"fastq": b"@", "fasta": b">"}[fmt]


def tiles_text(fmt, tile, n_tiles, seed=20261021):
    """-> (text, edges, n_records): a text of n_tiles tiles (five bytes short of a whole number, the last line unterminated)
    made of records around lines of LONG bytes.  At every multiple E of ROUND tiles inside the text -- where a round of the
    tile scan ends -- the last byte of the tile before is the '\\n' of a sequence line and the first byte of the next tile
    is a '\\n' too, with records on both sides (FASTA: the record goes on behind the blank line).  A text of one round has
    the same pair at its last tile's start instead."""
    rng = np.random.default_rng(seed)
    pool = rng.choice(np.frombuffer(b"ACGTNacgtn", np.uint8), 6 * LONG).tobytes()
    mark, parts, at, n_rec = _mark(fmt), [], 0, 0
    total = n_tiles * tile - 5

    def seq(n):
        k = int(rng.integers(0, len(pool) - n))
        return pool[k:k + n]

    def add(b):
        nonlocal at
        parts.append(b)
        at += len(b)

    def rec(n=LONG):
        nonlocal n_rec
        if fmt == "fastq":
            add(b"@r%d x\n" % n_rec + seq(n) + b"\n+\n" + b"I" * n + b"\n")
        else:
            add(b">r%d x\n" % n_rec + seq(n) + b"\n" + seq(n) + b"\r\n")
        n_rec += 1

    edges = [k * ROUND * tile for k in range(1, n_tiles // ROUND + 1) if k * ROUND * tile < total] or [(n_tiles - 1) * tile]
    for e in edges:
        while e - at > 2 * LONG + 1000:
            rec()
        name = b"edge%d" % n_rec
        add(mark + name + b"\n" + seq(e - at - len(name) - 3) + b"\n")     # ... whose '\n' is the last byte before e
        n_rec += 1
        assert at == e
        add(b"\n")                                                         # the first byte of the tile at e
        if fmt == "fasta":
            add(seq(500) + b"\n")
        rec(3000)                                                          # (a last tile has room for it)
    while total - at > 2 * LONG + 1000:
        rec()
    add(mark + b"last\n")
    add(seq(total - at))
    n_rec += 1
    text = b"".join(parts)
    assert len(text) == total and (len(text) + tile - 1) // tile == n_tiles
    for e in edges:
        assert text[e - 1:e + 1] == b"\n\n" and text[e - 2:e - 1] != b"\n"
    return text, edges, n_rec


def lines_text(n_lines, terminated, placed):
    """a text of n_lines lines, all empty but those of `placed` ({line index: bytes}); terminated: the last line ends with
    '\\n' (else it must not be empty)"""
    lines = [b""] * n_lines
    for k, v in placed.items():
        assert 0 <= k < n_lines and b"\n" not in v
        lines[k] = v
    assert terminated or lines[-1]
    return b"\n".join(lines) + (b"\n" if terminated else b"")


def kernel_blocks(text, lines):
    """blocks of `lines` lines as the record kernels count them: the piece behind the last '\\n' is a line, empty or not"""
    return (text.count(b"\n") + 1 + lines - 1) // lines


def line_block_cases(fmt, lines):
    """name -> (text, records, blocks of lines): mostly-blank texts with more than ROUND blocks of lines.  H: a header line,
    S: a sequence line; B = ROUND * lines is the first line of the second round."""
    L, B = lines, ROUND * lines
    H = lambda k: _mark(fmt) + b"h%d" % k                      # noqa: E731
    S = lambda k: b"ACGTacgtnN"[:4 + k % 7]                     # noqa: E731
    c = {}
    # a header as the last line of block 1023, its sequence line the first of block 1024
    c["H ends round 0, S starts round 1"] = (lines_text(B + 3, True, {5: H(0), 6: S(0), B - 1: H(1), B: S(1), B + 2: H(2)}), 2)
    # the nearest header of block 1500 lies in block 3: blk_h_before crosses the round boundary
    c["H in block 3, S in block 1500"] = (lines_text(1500 * L + 11, True, {3 * L + 5: H(0), 1500 * L + 7: S(0), 1500 * L + 9: H(1),
                                                                          1500 * L + 10: S(1)}), 2)
    # what follows block 1023 is found in a block of the later round: the suffix pass carries it into the earlier one
    c["S ends round 0, H in block 1724"] = (lines_text(1724 * L + 5, True, {B - L + 2: H(0), B - L + 10: S(0), 1724 * L + 3: H(1),
                                                                            1724 * L + 4: S(1)}), 2)
    c["S ends round 0, S in block 1724"] = (lines_text(1724 * L + 4, False, {B - L + 2: H(0), B - L + 10: S(0), 1724 * L + 3: S(1)}), 1)
    # an undecided last S line in the very last block, which is the third round's only one
    c["2B + 1 lines, the last one S"] = (lines_text(2 * B + 1, False, {B - 2: H(0), B - 1: S(0), B: H(1), B + 1: S(1), 2 * B - 5: H(2),
                                                                       2 * B: S(2)}), 3)
    c["B lines, the last one S"] = (lines_text(B, False, {B - 2: H(0), B - 1: S(0)}), 1)
    c["B lines and a final newline"] = (lines_text(B, True, {B - 2: H(0), B - 1: S(0)}), 1)
    c["B + 1 lines, the last one S"] = (lines_text(B + 1, False, {B - 1: H(0), B: S(0)}), 1)
    want_blocks = {"H ends round 0, S starts round 1": ROUND + 1, "H in block 3, S in block 1500": 1501, "S ends round 0, H in block 1724": 1725,
                   "S ends round 0, S in block 1724": 1725, "2B + 1 lines, the last one S": 2 * ROUND + 1, "B lines, the last one S": ROUND,
                   "B lines and a final newline": ROUND + 1, "B + 1 lines, the last one S": ROUND + 1}
    out = {}
    for name, (text, n_rec) in c.items():
        assert kernel_blocks(text, L) == want_blocks[name], name
        out[name] = (text, n_rec, want_blocks[name])
    return out


LINE_CASES = ["H ends round 0, S starts round 1", "H in block 3, S in block 1500", "S ends round 0, H in block 1724",
              "S ends round 0, S in block 1724", "2B + 1 lines, the last one S", "B lines, the last one S", "B lines and a final newline",
              "B + 1 lines, the last one S"]
