"""Texts for the EMBL reader's tests (test_makedb_embl_abi_host.py on the host reader, test_gpu_makedb_embl.py device against
host): the hand text of test_makedb.py with its expected records, one text per rule of process_embl_entry, and the fuzz
generator -- the line lists of test_random_embl_and_gbk_against_the_restatement plus a fragment flag among the lines and a
3-byte two-space line and a bare DE among the lines the reference panics on."""
import random

SEED = 20261021
N_FUZZ = 240
FEATURES = [b"ProteinName", b"GeneName", b"EC", b"GO", b"KEGG_ID", b"BioCyc_ID", b"HAMAP", b"Organism", b"TaxId", b"FullTaxonomy"]

EMBL = b"""ID   001R_FRG3G              Reviewed;         20 AA.
AC   Q6GZX4;
DE   RecName: Full=Putative transcription factor 001R {ECO:0000305};
DE   SubName: Full=Second name {ECO:1}; extra {ECO:2};
GN   Name=tf1; ORFNames=FV3-001R;
OS   Frog virus 3
OS   (isolate Goorha).
OC   Viruses; Varidnaviria;
OC   Bamfordvirae.
OX   NCBI_TaxID=654924;
DR   GO; GO:0046782; P:regulation of viral transcription; IEA:InterPro.
DR   GO; GO:0000001; F:x.
DR   KEGG; vg:2947773; -.
DR   EMBL; AY548484; AAT09660.1; -; Genomic_DNA.
SQ   SEQUENCE   20 AA;  29735 MW;  B4840739BF7D4121 CRC64;
     MAFSAEDVLK EYDRRRRMEA
//
//
ID   FRAG_X   Unreviewed;  30 AA.
DE   SubName: Full=Some fragment;
DE   Flags: Fragment;
SQ   SEQUENCE   30 AA;  1 MW;  0 CRC64;
     MAFSAEDVLK EYDRRRRMEA MAFSAEDVLK
//
ID   SHORT_Y   Unreviewed;  6 AA.
SQ   SEQUENCE   6 AA;  1 MW;  0 CRC64;
     MAFSAE
//
ID   lower_z   Unreviewed;  12 AA.
DE   RecName: Full=lower case stays, partial;
DE            EC=1.1.1.1 {ECO:3};
SQ   SEQUENCE   12 AA;  1 MW;  0 CRC64;
     mafsaedvlk ey
     extra residues beyond the declared length are not indexed
//
ID   NOT_TERMINATED   Unreviewed;  20 AA.
SQ   SEQUENCE   20 AA;  1 MW;  0 CRC64;
     MAFSAEDVLK EYDRRRRMEA
"""


def cells(**kw):
    """the ten cells in the order of EMBL_DEF_FTS, the named ones set"""
    return [kw.get(n.decode(), b"") for n in FEATURES]


# (id, EntryId, indexed, stored Sequence, cells) of the records EMBL keeps
EMBL_RECORDS = [
    (1, b"001R_FRG3G", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA",
     cells(ProteinName=b"Putative transcription factor 001R;;Second name", GeneName=b"tf1", GO=b"GO:0046782;GO:0000001", KEGG_ID=b"vg:2947773",
           Organism=b"Frog virus 3 (isolate Goorha)", TaxId=b"54924", FullTaxonomy=b"Viruses; Varidnaviria; Bamfordvirae.")),
    (5, b"lower_z", b"mafsaedvlkey", b"mafsaedvlkeyextraresiduesbeyondthedeclaredlengtharenotindexed",
     cells(ProteinName=b"lower case stays, partial", EC=b"1.1.1.1")),
]

SQ20 = b"SQ   SEQUENCE   20 AA;  1 MW;  0 CRC64;"
S20 = b"     MAFSAEDVLK EYDRRRRMEA"


def entry(*lines, sq=SQ20, seq=(S20,), eol=b"\n"):
    """the lines, an SQ line and sequence lines (None / (): left out), the terminator"""
    body = list(lines) + ([sq] if sq is not None else []) + list(seq)
    return b"".join(ln + eol for ln in body + [b"//"])


# name -> (text, the records it keeps as (id, EntryId, indexed, stored, cells), or None where only device == host is asked)
RULES = {
    "GN order: malformed before the deciding line": (entry(b"ID   A x", b"GN   Name=", b"GN   x Name=g0;", b"GN   Name=g1;") + entry(b"GN   Name=;;", b"GN      ", b"GN   Name= ", b"GN   N Name=q", b"GN   Name=g1;"), []),
    "GN order: malformed behind the deciding line": (
        entry(b"ID   A x", b"GN   ORFNames=o1;", b"GN   Name=;", b"GN   Name=g1;; x", b"GN   x Name=y;", b"GN   Name= ", b"GN   Nam", b"GN   Name=g2;"),
        [(1, b"A", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA", cells(GeneName=b"g1"))]),
    "GN: Name= anywhere in the line, also over the tag": (
        entry(b"GName=abcdefg;") + entry(b"GN   OrderedLocusNames=abc; Name=x;") + entry(b"GN   abc Name=x;") + entry(b"GN"),
        [(1, b"", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA", cells(GeneName=b"efg")),
         (2, b"", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA", cells(GeneName=b"edLocusNames=abc")),
         (4, b"", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA", cells())]),
    "RecName after SubNames": (
        entry(b"DE   SubName: Full=s1;", b"DE   SubName: Full=s2;", b"DE   RecName: Full=r1;", b"DE   RecName: Full=r2;", b"DE   SubName: Full=s3;",
              b"DE   SubName: Full=;", b"DE   SubName: Full=s4;"),
        [(1, b"", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA", cells(ProteinName=b"r2;;s3;;;;s4"))]),
    "SubName after an empty value": (
        entry(b"DE   RecName: Full=;;", b"DE   SubName: Full=;", b"DE   SubName: Full=s1;", b"DE   SubName: Full=s2") +
        entry(b"DE   SubName: Full=", b"DE   SubName: Full=t1"),
        [(1, b"", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA", cells(ProteinName=b"s1;;s2")),
         (2, b"", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA", cells(ProteinName=b"t1"))]),
    "empty OS / OC / DR contributions": (
        entry(b"OS   .", b"OS   ...", b"OS   Org.", b"OS   ", b"OC   ", b"OC   ", b"OC   Tax;", b"OC   ", b"OC   More.", b"DR   GO; ;", b"DR   GO; ;;;",
              b"DR   GO; GO:1;", b"DR   KEGG; ;", b"DR   HAMAP; ;", b"DR   HAMAP; ;", b"DR   BioCyc; b;;", b"DR   BioCyc; ;"),
        [(1, b"", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA",
          cells(GO=b";;GO:1", HAMAP=b";", BioCyc_ID=b"b;", Organism=b"  Org ", FullTaxonomy=b"Tax;  More."))]),
    "greedy removal: two brace groups, ';' runs on both sides": (
        entry(b"DE   RecName: Full=a;; {x}; mid {y};;;") + entry(b"DE   RecName: Full=a;; {x}; mid {y}; t;;") +
        entry(b"DE   RecName: Full=a {x;") + entry(b"DE   RecName: Full=a}; {") + entry(b"DE   RecName: Full= {};") +
        entry(b"DE            EC=1.2.3.4;; {a}; {b};", b"DE   RecName: Full=};b {c};"),
        [(1, b"", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA", cells(ProteinName=b"a")),
         (2, b"", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA", cells(ProteinName=b"a;; t")),
         (3, b"", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA", cells(ProteinName=b"a {x")),
         (4, b"", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA", cells(ProteinName=b"a}; {")),
         (5, b"", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA", cells()),
         (6, b"", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA", cells(ProteinName=b"};b", EC=b"1.2.3.4"))]),
    "DE: which word decides, and the short lines": (
        entry(b"DE   SubName RecName EC=") + entry(b"DE   RecName: Full=") + entry(b"DE   RecName: Full") + entry(b"DE   EC=1.1.1.1;x") +
        entry(b"DE   EC=1.1.1.1;") + entry(b"DE   Flags: Fragment; EC=1") + entry(b"DE   Flags: Fragment;") + entry(b"DE   Flags: Fragment") + entry(b"DE  "),
        None),
    "OX under 12": (entry(b"OX   NCBI_TaxID=1") + entry(b"OX   NCBI_TaxID=") + entry(b"OX   NCBI_TaxID= 9606;") + entry(b"OX   NCBI_TaxID=96;;", b"OX   NCBI_TaxID=12345;"),
                    [(1, b"", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA", cells()),
                     (4, b"", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA", cells(TaxId=b"2345"))]),
    "SQ twice": (entry(b"SQ   SEQUENCE   5 AA;") + entry(b"SQ   SEQUENCE   20 AA;", sq=b"SQ   SEQUENCE   5 AA;") + entry(b"SQ   SEQUENCE") + entry(sq=b"SQ   SEQUENCE   21 AA;")
                 + entry(sq=b"SQ   SEQUENCE   7 AA;"),
                 [(1, b"", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA", cells()),
                  (5, b"", b"MAFSAED", b"MAFSAEDVLKEYDRRRRMEA", cells())]),
    "Atoi refusals": (b"".join(entry(sq=b"SQ   SEQUENCE   " + n + b" AA;") for n in
                                (b"+", b"-7", b"12x", b"12345678901234567890", b"+12", b"0012", b"-0", b"99999999999", b"4294967303", b"000000000000000000000000000008",
                                 b"1" + b"0" * 200, b"12\r")),
                      [(5, b"", b"MAFSAEDVLKEY", b"MAFSAEDVLKEYDRRRRMEA", cells()), (6, b"", b"MAFSAEDVLKEY", b"MAFSAEDVLKEYDRRRRMEA", cells()),
                       (10, b"", b"MAFSAEDV", b"MAFSAEDVLKEYDRRRRMEA", cells()), (12, b"", b"MAFSAEDVLKEY", b"MAFSAEDVLKEYDRRRRMEA", cells())]),
    "a two-space line of 3 bytes": (entry(b"   ") + entry(b"  ") + entry(b"    ") + entry(b"     ") + entry(b"ID  ") + entry(b"OS") + entry(b"XX") + entry(b"X", b"", b"/"),
                                    [(4, b"", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA", cells()), (7, b"", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA", cells()),
                                     (8, b"", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA", cells())]),
    "sequence lines in front of the ID line": (
        b"     MKT AY\nSQ   SEQUENCE   9 AA;\n     IAKQ\nID   LATE x\n     RQ  \n//\n",
        [(1, b"LATE", b"MKTAYIAKQ", b"MKTAYIAKQRQ", cells())]),
    "an interior '\\r'": (
        entry(b"ID   A\rB x", b"OS   Org\r.", b"DR   GO;\rGO:1;\r x", b"DR   KEGG; k\r;", b"OC   a\r\r", seq=(b"     MAFS\rAEDVLK EYDRRRRMEA",), eol=b"\r\n") + b"//\r\r\n" + b"// \n///\n",
        [(1, b"A", b"MAFS\rAEDVLKEYDRRRRME", b"MAFS\rAEDVLKEYDRRRRMEA", cells(Organism=b"Org\r", GO=b"GO:1", KEGG_ID=b"k", FullTaxonomy=b"a\r\r"))]),
    "bytes >= 0x80": (
        entry(b"ID   \xc3\x89\xff x", b"DE   RecName: Full=\x80\xfe {\xff};", b"OS   \xe9t\xe9.", seq=(b"     MAFS\xc3\x89DVLK \xff\x80DRRRRMEA",)),
        [(1, b"\xc3\x89\xff", b"MAFS\xc3\x89DVLK\xff\x80DRRRRMEA", b"MAFS\xc3\x89DVLK\xff\x80DRRRRMEA", cells(ProteinName=b"\x80\xfe", Organism=b"\xe9t\xe9"))]),
    "ID / DR without a field, DR keys": (
        entry(b"ID   ") + entry(b"DR   \t ") + entry(b"DR   GO;") + entry(b"DR   GO; ") + entry(b"DR   GO;x y") + entry(b"DR   go; x", b"DR   KEGG;; x", b"DR   HAMAP;\tv;;  w") +
        entry(b"ID   first x", b"ID   \t second\ty"),
        [(5, b"", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA", cells()), (6, b"", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA", cells(HAMAP=b"v")),
         (7, b"second", b"MAFSAEDVLKEYDRRRRMEA", b"MAFSAEDVLKEYDRRRRMEA", cells())]),
}

ENDS = {   # text -> kept records
    "empty": (b"", 0), "one line end": (b"\n", 0), "a terminator alone": (b"//", 0), "two terminators": (b"//\n//\n", 0),
    "an unterminated tail": (entry(b"ID   A x") + b"ID   B x\n" + SQ20 + b"\n" + S20 + b"\n", 1),
    "a last terminator without its line end": (entry(b"ID   A x") + b"ID   B x\n" + SQ20 + b"\n" + S20 + b"\n//", 2),
    "a last terminator with a bare CR": (entry(b"ID   A x") + b"ID   B x\n" + SQ20 + b"\n" + S20 + b"\n//\r", 2),
    "CRLF throughout": (EMBL.replace(b"\n", b"\r\n"), 2),
    "nothing but a tail": (b"ID   B x\n" + SQ20 + b"\n" + S20 + b"\n", 0),
}

LINES = [b"ID   P%d_X   Reviewed;  %d AA.", b"DE   RecName: Full=Name %d {ECO:1};", b"DE   SubName: Full=Sub %d;;",
         b"DE            EC=2.7.%d.1;", b"DE   Flags: Precursor;", b"GN   Name=g%d;", b"GN   ORFNames=o%d;", b"OS   Org %d.",
         b"OC   Tax%d; More.", b"OX   NCBI_TaxID=12345%d;", b"DR   GO; GO:%d; F:x.", b"DR   KEGG; k:%d; -.", b"DR   BioCyc; B:%d; -.",
         b"DR   HAMAP; MF_%d; x.", b"DR   Pfam; PF%d; x.", b"XX", b"X", b"", b"CC   free text %d", b"     MAFSAEDVLK EYDRRRRMEA",
         b"     mktay iakqr", b"     A", b"SQ   SEQUENCE   %d AA;  1 MW;  0 CRC64;", b"DE   Flags: Fragment;"]
PANICS = [b"ID", b"DE  RecName: short", b"OX   x", b"DR   ", b"SQ   SEQUENCE", b"GN   Name=", b"SQ   SEQUENCE   999 AA;", b"   ", b"DE"]


def held(body):
    return sum(len(ln[5:].replace(b" ", b"")) for ln in body if ln[:2] == b"  " and len(ln) >= 5)


def fuzz_text(rng, trial):
    """records assembled at random from well-formed and odd lines (repeated tags, tags in the wrong place, CR line ends, empty
    records, no terminator); about one record in six holds a line on which the Go would panic"""
    recs = []
    for _ in range(rng.randrange(0, 8)):
        body = []
        for _ in range(rng.randrange(0, 12)):
            t = LINES[rng.randrange(len(LINES))]
            body.append(t.replace(b"%d", b"%d" % rng.randrange(5, 40)))
        if rng.random() < 0.6:   # a well-formed end, so that a good share of the records is kept: declares what it holds half the time
            seq = [b"     MAFSAEDVLK EYDRRRRMEA"] * rng.randrange(1, 3)
            n = held(body + seq) if rng.random() < 0.5 else rng.randrange(5, 21)
            body += [b"SQ   SEQUENCE   %d AA;  1 MW;  0 CRC64;" % n] + seq
        if rng.random() < 0.17:
            body.insert(rng.randrange(len(body) + 1), PANICS[rng.randrange(len(PANICS))])
        recs.append(body)
    eol = b"\r\n" if trial % 3 == 0 else b"\n"
    text = b"".join(eol.join(b + [b"//"]) + eol for b in recs)
    if trial % 5 == 4:
        text += eol.join(LINES[:3])   # an unterminated tail
    return text


def fuzz_texts():
    rng = random.Random(SEED)
    return [fuzz_text(rng, t) for t in range(N_FUZZ)]


def n_terminators(text):
    """the lines that are exactly "//" after the '\\r' drop"""
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return sum(1 for ln in lines if (ln[:-1] if ln.endswith(b"\r") else ln) == b"//")


def cut_ref(text):
    """kaamer_text_cut_embl, restated: the end of the last line that is a terminator"""
    at, best = 0, 0
    while at < len(text):
        nl = text.find(b"\n", at)
        end, nxt = (len(text), len(text)) if nl < 0 else (nl, nl + 1)
        ln = text[at:end]
        if (ln[:-1] if ln.endswith(b"\r") else ln) == b"//":
            best = nxt
        at = nxt
    return best
