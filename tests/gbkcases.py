"""Texts for the GBK reader's tests (test_makedb_gbk_abi_host.py on the host reader, test_gpu_makedb_gbk.py device against
host): a hand text with its expected records, one text or more per rule of process_gbk_entry, and the fuzz generator -- the
line lists of test_random_embl_and_gbk_against_the_restatement plus blocks of lines that join to ", partial" and " [" ...
"]." and the lines the reference panics on."""
import random

from emblcases import cut_ref, n_terminators  # noqa: F401  (the terminator is EMBL's, so are its restatements)

SEED = 20261021
N_FUZZ = 240
FEATURES = [b"ProteinName", b"Organism", b"FullTaxonomy"]

GBK = b"""LOCUS       AAT09660                  20 aa            linear   VRL 01-JAN-2000
DEFINITION  putative transcription factor 001R [Frog virus 3
            (isolate Goorha)].
ACCESSION   AAT09660
VERSION     AAT09660.1  GI:47060117
DBSOURCE    accession AY548484.1
KEYWORDS    .
SOURCE      Frog virus 3
  ORGANISM  Frog virus 3
            Viruses; Varidnaviria; Bamfordvirae;
            Iridoviridae.
REFERENCE   1  (residues 1 to 20)
  AUTHORS   Tan,W.G., Barkman,T.J.
  TITLE     Comparative genomic analyses
COMMENT     Method: conceptual translation.
FEATURES             Location/Qualifiers
     source          1..20
                     /organism="Frog virus 3"
     Protein         1..20
                     /product="putative transcription factor 001R"
ORIGIN
        1 mafsaedvlk eydrrrrmea
//
//
LOCUS       PART_X                    30 aa
DEFINITION  some enzyme, partial [Org].
VERSION     PART_X.1
ORIGIN
        1 mafsaedvlk eydrrrrmea mafsaedvlk
//
LOCUS       SHORT_Y                    6 aa
VERSION     SHORT_Y.1
ORIGIN
        1 mafsae
//
LOCUS       KEPT_Z                    32 aa
DEFINITION  protein kinase [Homo sapiens]. extra
VERSION     KEPT_Z.2
  ORGANISM  Homo sapiens
ORIGIN
        1 MAFSAEDVLK eydrrrrmea acdefghikl
       31 mn
//
LOCUS       NOT_TERMINATED            20 aa
VERSION     NT.1
ORIGIN
        1 mafsaedvlk eydrrrrmea
""".replace(b"ORIGIN\n", b"ORIGIN      \n")   # (as NCBI writes it: a bare ORIGIN of 6 bytes is a line the reference panics on)


def cells(**kw):
    """the three cells in the order of GBK_DEF_FTS, the named ones set"""
    return [kw.get(n.decode(), b"") for n in FEATURES]


SEQ20 = b"MAFSAEDVLKEYDRRRRMEA"


def rec(pid, entry_id=b"V1.1", seq=SEQ20, **kw):
    """(id, EntryId, indexed, stored Sequence, cells): GBK declares no length, so both strings are the same"""
    return (pid, entry_id, seq, seq, cells(**kw))


GBK_RECORDS = [
    rec(1, b"AAT09660.1", ProteinName=b"putative transcription factor 001R", Organism=b"Frog virus 3",
        FullTaxonomy=b"Viruses; Varidnaviria; Bamfordvirae; Iridoviridae."),
    rec(5, b"KEPT_Z.2", SEQ20 + b"ACDEFGHIKLMN", ProteinName=b"protein kinase extra", Organism=b"Homo sapiens"),
]

VER = b"VERSION     V1.1  GI:1"
ORIGIN = b"ORIGIN      "
S20 = b"        1 mafsaedvlk eydrrrrmea"
SP12 = b" " * 12


def entry(*lines, ver=VER, origin=ORIGIN, seq=(S20,), eol=b"\n"):
    """the lines, a VERSION line, an ORIGIN line and sequence lines (None / (): left out), the terminator"""
    body = list(lines) + ([ver] if ver is not None else []) + ([origin] if origin is not None else []) + list(seq)
    return b"".join(ln + eol for ln in body + [b"//"])


STATE0 = [b"LOCUS", b"ACCESSION", b"KEYWORDS", b"SOURCE", b"COMMENT", b"REFERENCE", b"DBLINK", b"DBSOURCE"]

# name -> (text, the records it keeps as (id, EntryId, indexed, stored, cells), or None where only device == host is asked)
RULES = {
    "every keyword": (
        entry(*[ln for j, kw in enumerate(STATE0 + [b"FEATURES"]) for ln in (b"DEFINITION  d%d" % j, kw.ljust(12) + b"x", SP12 + b"not taken")],
              b"  ORGANISM  Org", SP12 + b"Tax."),
        [rec(1, ProteinName=b" ".join(b"d%d" % j for j in range(9)), Organism=b"Org", FullTaxonomy=b"Tax.")]),
    "a keyword as the first word of a continuation line": (
        entry(b"DEFINITION  first", SP12 + b"SOURCE of the name", SP12 + b"lost", b"  ORGANISM  Org", SP12 + b"DEFINITION x", SP12 + b"more"),
        [rec(1, ProteinName=b"first DEFINITION x more", Organism=b"Org")]),
    "\" //\" and \"// x\" inside an entry": (
        entry(VER, b"DEFINITION  name", b" //", SP12 + b"lost", b"DEFINITION  again", ORIGIN, S20, b"// x", b"       21 acdefghikl", b"//x", b"       31 acdefghikl",
              ver=None, origin=None, seq=()),
        [rec(1, ProteinName=b"name again")]),
    "tab and '\\r' next to a keyword": (
        entry(b"DEFINITION  name", b"\tVERSION    X9", b"ORIGIN\r     1 abc", eol=b"\r\n") + entry(VER, b"ORIGIN\r", ver=None, eol=b"\r\n") +
        entry(b"DEFINITION  name", b"ORIGIN\t     1 abc") + entry(b"DEFINITION  name", b"VERSION\r", ver=None),
        [rec(1, ProteinName=b"name X9 1 abc"), rec(3, ProteinName=b"name 1 abc")]),
    "a lower-case keyword": (
        entry(VER, b"definition  lower", b"DEFINITION  name", b"version     x", b"Origin      y", ORIGIN, S20, ver=None, origin=None, seq=()),
        [rec(1, b"lower", ProteinName=b"name x y")]),
    "all-space lines of 11 and 12 bytes in DEFINITION": (
        entry(b"DEFINITION  name", SP12, SP12 + b"tail") + entry(b"DEFINITION  name", b" " * 11) + entry(b"DEFINITION  ", b" " * 14, SP12 + b"x") +
        entry(b"DEFINITION  name", b" " * 40),
        [rec(1, ProteinName=b"name  tail"), rec(3, ProteinName=b"   x"), rec(4, ProteinName=b"name " + b" " * 28)]),
    "VERSION: a continuation line wins, only white space behind column 12": (
        entry(ver=None, origin=None, seq=(VER, SP12 + b"W2 tail", ORIGIN, S20)) + entry(ver=b"VERSION     \t  ") + entry(ver=b"VERSION     V3", origin=None, seq=(SP12, ORIGIN, S20)) +
        entry(ver=b"VERSION") + entry(ver=b"VERSION     \t X5\ty") + entry(ver=b"VERSION    ") + entry(b"VERSION     first", b"LOCUS       x") + entry(ver=None) +
        entry(ver=b"VERSION     \x0b\x0c\rV9\x0bz"),
        [rec(1, b"W2"), rec(5, b"X5"), rec(7, b"V1.1"), rec(8, b""), rec(9, b"V9")]),
    "Organism and FullTaxonomy": (
        entry(b"  ORGANISM  ", SP12 + b"Org second", SP12 + b"Tax1;", SP12, SP12 + b"Tax2;", SP12 + b"Tax3.") + entry(b"  ORGANISM  Org", SP12, SP12 + b"Tax") +
        entry(b"  ORGANISM") + entry(b"  ORGANISM  Org", b"  too short"),
        [rec(1, Organism=b"Org second", FullTaxonomy=b"Tax1;  Tax2; Tax3."), rec(2, Organism=b"Org", FullTaxonomy=b"Tax")]),
    "ORIGIN: bare, and lines of 9 and 10 bytes behind it": (
        entry(origin=b"ORIGIN") + entry(seq=(b"        1", S20)) + entry(seq=(b"        1 ", S20)) + entry(origin=b"ORIGIN    mafsaedvlk eydrrrrmea", seq=()) +
        entry(origin=b"ORIGIN   x") + entry(origin=b"ORIGIN  x"),
        [rec(3), rec(4), rec(5)]),
    "sequence bytes: lower, mixed case and >= 0x80": (
        entry(seq=(b"        1 MafSaEdvlk \xc3\xa9\xffdrr\trmea 12", b"       21 @[`{az")),
        [rec(1, seq=b"MAFSAEDVLK\xc3\xa9\xffDRR\tRMEA12@[`{AZ")]),
    "6 and 7 residues": (
        entry(seq=(b"        1 mafsae",)) + entry(seq=(b"        1 mafsaed",)) + entry(seq=(b"        1 maf sae", b"        7  d ")) + entry(seq=()),
        [rec(2, seq=b"MAFSAED"), rec(3, seq=b"MAFSAED")]),
    "\", partial\" inside a line and across joins": (
        entry(b"DEFINITION  enzyme, partial [Org].") + entry(b"DEFINITION  enzyme,", SP12 + b"partial cds") + entry(b"DEFINITION  enzyme, par", SP12 + b"tial") +
        entry(b"DEFINITION  enzyme ,partial") + entry(b"DEFINITION  ,", SP12 + b"partial") + entry(b"DEFINITION  x,", SP12 + b" partial") +
        entry(b"DEFINITION  x,", SP12, b"            partial") + entry(b"DEFINITION  x, partia"),
        [rec(3, ProteinName=b"enzyme, par tial"), rec(4, ProteinName=b"enzyme ,partial"), rec(6, ProteinName=b"x,  partial"), rec(7, ProteinName=b"x,  partial"),
         rec(8, ProteinName=b"x, partia")]),
    "\" [\" inside a line and formed by a join": (
        entry(b"DEFINITION  kinase [Homo sapiens].") + entry(b"DEFINITION  kinase", SP12 + b"[Homo sapiens]. tail") + entry(b"DEFINITION  a [", SP12 + b"]. z") +
        entry(b"DEFINITION  [x]. y") + entry(b"DEFINITION  a", SP12, SP12 + b"[b].") + entry(b"DEFINITION  ", SP12 + b"[b]. c"),
        [rec(1, ProteinName=b"kinase"), rec(2, ProteinName=b"kinase tail"), rec(3, ProteinName=b"a z"), rec(4, ProteinName=b"[x]. y"), rec(5, ProteinName=b"a "),
         rec(6, ProteinName=b"[b]. c")]),
    "several \"].\", \"].\" in front of the only \" [\", \" [\" without \"].\"": (
        entry(b"DEFINITION  a [b]. c [d]. e") + entry(b"DEFINITION  a]. b [c") + entry(b"DEFINITION  a [b] c") + entry(b"DEFINITION  a [].b") + entry(b"DEFINITION  a [.]") +
        entry(b"DEFINITION  a [b]", SP12 + b". c") + entry(b"DEFINITION  a [b", SP12 + b"]. c].", SP12 + b"d") + entry(b"DEFINITION  a].[ [.]].]"),
        [rec(1, ProteinName=b"a e"), rec(2, ProteinName=b"a]. b [c"), rec(3, ProteinName=b"a [b] c"), rec(4, ProteinName=b"ab"), rec(5, ProteinName=b"a [.]"),
         rec(6, ProteinName=b"a [b] . c"), rec(7, ProteinName=b"a d"), rec(8, ProteinName=b"a].[]")]),
    "an empty entry between two \"//\", lines of 0 and 1 bytes": (
        entry(b"DEFINITION  one") + b"//\n" + entry(b"DEFINITION  name", b"", b"X", b" ", SP12 + b"more", b"", seq=(b"        1 mafsaedvlk", b"", b"x", b"       11 eydrrrrmea")) +
        b"\n\n//\n" + b"X\n//\n",
        [rec(1, ProteinName=b"one"), rec(3, ProteinName=b"name more")]),
}

ENDS = {   # text -> kept records
    "empty": (b"", 0), "one line end": (b"\n", 0), "a terminator alone": (b"//", 0), "two terminators": (b"//\n//\n", 0),
    "a final line end": (entry(b"LOCUS       A") + entry(b"LOCUS       B"), 2),
    "no final line end": ((entry(b"LOCUS       A") + entry(b"LOCUS       B"))[:-1], 2),
    "a last terminator with CR LF": (entry(b"LOCUS       A") + entry(b"LOCUS       B", eol=b"\r\n"), 2),
    "a last terminator with a bare CR": (entry(b"LOCUS       A") + entry(b"LOCUS       B")[:-1] + b"\r", 2),
    "text behind the last terminator": (entry(b"LOCUS       A") + b"LOCUS       B\n" + VER + b"\n" + ORIGIN + b"\n" + S20 + b"\n", 1),
    "CRLF throughout": (GBK.replace(b"\n", b"\r\n"), 2),
    "nothing but a tail": (b"LOCUS       B\n" + VER + b"\n" + ORIGIN + b"\n" + S20 + b"\n", 0),
}

LINES = [b"LOCUS       L%d   10 aa", b"DEFINITION  protein %d [Org]. tail", b"DEFINITION  enzyme, partial [Org].", b"            continued [Other].",
         b"ACCESSION   A%d", b"VERSION     V%d.1  GI:1", b"KEYWORDS    .", b"SOURCE      src", b"  ORGANISM  Org %d", b"            Bacteria; X%d.",
         b"COMMENT     c", b"FEATURES             Location/Qualifiers", b"     source          1..%d", b"ORIGIN      ", b"        1 mafsaedvlk eydrrrrmea",
         b"       21 acdefghikl", b"        1 mktay", b"REFERENCE   1", b"DBSOURCE    x", b"DBLINK      BioProject: %d", b"X", b"", b"DEFINITION  plain name %d",
         b"            ", b" //", b"                                  /note=\"deep %d\""]
PANICS = [b"DEFINITION", b"VERSION", b"VERSION     ", b"  ORGANISM", b"ORIGIN", b"        1"]
# runs of lines that belong together: names that join to ", partial" or to " [" ... "].", a whole ORGANISM section
BLOCKS = [[b"DEFINITION  enzyme %d,", b"            partial cds"], [b"DEFINITION  kinase %d", b"            [Org %d]. tail"],
          [b"DEFINITION  long name %d", b"            goes on", b"            [Org]."], [b"  ORGANISM  Org %d", b"            Bacteria; X%d;", b"            Y."],
          [b"DEFINITION  short, par", b"            tial %d"]]


def fuzz_text(rng, trial):
    """records assembled at random from well-formed and odd lines (repeated keywords, keywords in the wrong place, CR line
    ends, empty records, no terminator); about one record in six holds a line on which the Go would panic"""
    recs = []
    for _ in range(rng.randrange(0, 8)):
        body = []
        for _ in range(rng.randrange(0, 12)):
            t = LINES[rng.randrange(len(LINES))]
            body.append(t.replace(b"%d", b"%d" % rng.randrange(5, 40)))
        if rng.random() < 0.5:
            at = rng.randrange(len(body) + 1)
            body[at:at] = [t.replace(b"%d", b"%d" % rng.randrange(5, 40)) for t in BLOCKS[rng.randrange(len(BLOCKS))]]
        if rng.random() < 0.7:   # a well-formed end, so that a good share of the records is kept
            body += [b"VERSION     W%d.1" % len(recs), b"ORIGIN      ", b"        1 mafsaedvlk eydrrrrmea" if rng.random() < 0.8 else b"        1 mafsae"]
        if rng.random() < 0.17:
            body.insert(rng.randrange(len(body) + 1), PANICS[rng.randrange(len(PANICS))])
        recs.append(body)
    eol = b"\r\n" if trial % 3 == 0 else b"\n"
    text = b"".join(eol.join(b + [b"//"]) + eol for b in recs)
    if trial % 5 == 4:
        text += eol.join(LINES[:3])   # an unterminated tail
    return text


def fuzz_texts():
    """the generator's texts, then the hand text and every rule and end text: the device fuzz runs them all"""
    rng = random.Random(SEED)
    return [fuzz_text(rng, t) for t in range(N_FUZZ)] + [GBK] + [t for t, _ in RULES.values()] + [t for t, _ in ENDS.values()]


def name_pieces(entry_text, states):
    """the [12:] of every state-1 line of one entry's text, in order (states: token -> state, the restatement's table); None
    where a line under 12 bytes stands in state 1"""
    inside, out = 0, []
    for ln in entry_text.split(b"\n"):
        if len(ln) < 2:
            continue
        inside = states.get(ln.strip(b" ").split(b" ")[0], inside)
        if inside == 1:
            if len(ln) < 12:
                return None
            out.append(ln[12:])
    return out


def join_name(pieces):
    """-> (the joined ProteinName, the offsets of the spaces the joins put in)"""
    name, seps = b"", []
    for p in pieces:
        if name != b"":
            seps.append(len(name))
            name += b" "
        name += p
    return name, seps
