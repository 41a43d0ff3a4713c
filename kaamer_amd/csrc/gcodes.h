// gcodes.h — the genetic codes a request may name (search.GCodes, pkg/search/gcode.go:21-34): the thirteen tables, once,
// as NCBI-style 64-letter strings in t-c-a-g order (amino acids; 'M' where the codon is a start codon).  They equal the
// reference's maps gcode_N (tests/golden/gcodes.json), which cite an older listing than today's NCBI pages: narrower
// start sets.  In all thirteen Stop <=> amino acid '*'.  The device copy (translate.hip.inc) and the host's
// (kaamer_genetic_code, host_search.cpp) both expand KT_GCODES.  Not part of the ABI.
#pragma once
#include <stdint.h>

#define KT_GCODES(X)                                                                                                                                  \
    X(1, "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "---M---------------M---------------M----------------------------")  \
    X(2, "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSS**VVVVAAAADDEEGGGG", "--------------------------------MMMM---------------M------------")  \
    X(3, "FFLLSSSSYY**CCWWTTTTPPPPHHQQRRRRIIMMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "-----------------------------------M----------------------------")  \
    X(4, "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "--MM---------------M------------MMMM---------------M------------")  \
    X(5, "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSSSSVVVVAAAADDEEGGGG", "---M----------------------------MMMM---------------M------------")  \
    X(6, "FFLLSSSSYYQQCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "-----------------------------------M----------------------------")  \
    X(9, "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNNKSSSSVVVVAAAADDEEGGGG", "-----------------------------------M----------------------------")  \
    X(10, "FFLLSSSSYY**CCCWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "-----------------------------------M----------------------------") \
    X(11, "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "---M---------------M------------MMMM---------------M------------") \
    X(12, "FFLLSSSSYY**CC*WLLLSPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "-------------------M---------------M----------------------------") \
    X(13, "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSSGGVVVVAAAADDEEGGGG", "-----------------------------------M----------------------------") \
    X(14, "FFLLSSSSYYY*CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNNKSSSSVVVVAAAADDEEGGGG", "-----------------------------------M----------------------------") \
    X(15, "FFLLSSSSYY*QCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "-----------------------------------M----------------------------")

#define KT_N_GCODES 13
#define KT_SLOT_DEFAULT 8   /* table 11, gcodeBacteria: what GetORFs consults whatever the request says (dna.go:106) */

// the host's copy: row = table slot
struct KtTable { int32_t code; const char *aa, *start; };
static inline const KtTable *kt_tables()
{
#define KT_ROW_(code_, aa_, start_) { code_, aa_, start_ },
    static const KtTable t[KT_N_GCODES] = { KT_GCODES(KT_ROW_) };
#undef KT_ROW_
    return t;
}

// the table slot of a request's genetic code; 0 = the reference's behaviour = table 11; -1: not a key of search.GCodes
static inline int kt_gcode_slot(int32_t code)
{
    if (code == 0) return KT_SLOT_DEFAULT;
    for (int i = 0; i < KT_N_GCODES; i++)
        if (kt_tables()[i].code == code) return i;
    return -1;
}
