"""kaamer_text_cut_fasta (CPU) against a Python statement of its rule, and the property the rule exists for: at every valid
cut, the records of the left piece with its last record upper-cased plus the records of the right piece are the records
of the whole text (through kaamer_parse_fasta)."""
import random

from kaamer_amd import api

SPACE = b" \t\n\v\f\r"
# weights chosen so that well over a quarter of the random texts hold a valid cut (asserted below)
ALPHABET = b">" * 3 + b"A" * 3 + b"c" * 2 + b"*" + b" " + b"\t" + b"\v" + b"\f" + b"\r" + b"\n" * 6
SEED = 20261019
N_TEXTS = 3000


def _has_s_line(tail):
    """an S line, complete or not: it does not start with '>' and holds a non-space byte"""
    for ln in tail.split(b"\n"):
        if ln[:1] != b">" and ln.strip(SPACE):
            return True
    return False


def valid_cuts(text):
    return [p for p in range(1, len(text)) if text[p - 1:p] == b"\n" and text[p:p + 1] == b">" and _has_s_line(text[p:])]


def ref_cut(text):
    v = valid_cuts(text)
    return v[-1] if v else 0


def _texts():
    rng = random.Random(SEED)
    return [bytes(rng.choice(ALPHABET) for _ in range(rng.randint(0, 60))) for _ in range(N_TEXTS)]


def _upper(s):
    return "".join(chr(ord(c) - 32) if "a" <= c <= "z" else c for c in s)


def _records(text, upper_last=False):
    recs = [(r["name"], r["seq"]) for r in api.parse_reads(text, "fasta")]
    if upper_last and recs:
        recs[-1] = (recs[-1][0], _upper(recs[-1][1]))
    return recs


HAND = {
    "no '>'": (b"ACGT\nACGT\n", 0),
    "'>' only mid-line": (b"AC>GT\nA>C\n x>\n", 0),
    "the tail holds only headers": (b">a\nAC\n>b\n>c\n", 0),
    "headers, then a sequence": (b">a\nAC\n>b\n>c\nG\n", 9),
    "the tail holds only whitespace lines": (b">a\nAC\n>b\n \t\n\r\n\n", 0),
    "partial last line beginning with '>'": (b">a\nAC\n>b\nGG\n>c", 6),
    "partial last line beginning with a letter": (b">a\nAC\n>b\nG", 6),
    "partial last line of spaces": (b">a\nAC\n>b\n  ", 0),
    "CRLF": (b">a\r\nAC\r\n>b\r\nGG\r\n", 8),
    "'>' at 0 is no cut": (b">a\nAC\n", 0),
    "leading blank line": (b"\n>a\nAC\n", 1),
    "' >x' is a sequence line": (b">a\nAC\n>b\n >x\n", 6),
    "len 0": (b"", 0),
    "len 1": (b">", 0),
    "len 1, newline": (b"\n", 0),
    "len 2": (b"\n>", 0),
}


def test_hand_cases(klib):
    for name, (text, want) in HAND.items():
        assert ref_cut(text) == want, name
        assert api.text_cut_fasta(text) == want, name


def test_random_texts_against_the_rule(klib):
    with_cut = 0
    for text in _texts():
        want = ref_cut(text)
        assert api.text_cut_fasta(text) == want, text
        with_cut += want != 0
    assert with_cut * 4 >= N_TEXTS, with_cut


def test_pieces_give_the_records_of_the_whole(klib):
    checked = 0
    for text in _texts()[:1500]:
        whole = None
        cuts = valid_cuts(text)
        assert api.text_cut_fasta(text) == (cuts[-1] if cuts else 0)
        # the library's own cuts, taken from the right until none is left: the chain of pieces parses to the whole
        pieces, rest = [], text
        while api.text_cut_fasta(rest):
            p = api.text_cut_fasta(rest)
            assert p in cuts
            pieces.insert(0, rest[p:])
            rest = rest[:p]
        if pieces:
            chain = _records(rest, upper_last=True)
            for k, piece in enumerate(pieces):
                chain += _records(piece, upper_last=k < len(pieces) - 1)
            assert chain == _records(text), text
        for p in cuts:
            if whole is None:
                whole = _records(text)
            assert _records(text[:p], upper_last=True) + _records(text[p:]) == whole, (text, p)
            checked += 1
    assert checked >= 1500 // 4


def test_the_s_line_condition_matters(klib):
    # a cut with nothing but headers behind it would leave a piece without a record: the rule refuses it, and the reader
    # upper-cases a record that a header line closes even when it is the input's last
    text = b">a\nacgt\n>b\n"
    assert api.text_cut_fasta(text) == 0
    assert _records(text) == [("a", "ACGT")]
    assert _records(b">a\nacgt\n") == [("a", "acgt")]
